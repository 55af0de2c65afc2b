"""Seeded inputs, the torch fp32 restatement and the error measures that tests/test_hier_sampling.py (CPU) and
tests/test_gpu_hier_sampling.py (GPU) share for the sampling path without the occupancy grid.  Everything is generated from a seed
on the CPU, once per case (cached), and never modified by a test.

Tolerances.  The kernels scan a ray in another order than torch's cumprod / cumsum / sum do, so they cannot match torch bit for
bit; the bar is the float64 witness (tests/hier_witness.py).  How far fp32 arithmetic sits from the witness is MEASURED: the torch
fp32 op sequence of the reference runs on the very inputs the kernels get, its error against the witness is taken over all cases
below (`measure_torch_errors`, run on the CPU; tests/test_hier_sampling.py re-measures and checks the record), and the kernels are
allowed four times that.  The recorded values are in TORCH_ERROR; profiles/hier_sampling.md has the same table."""
import functools

import numpy as np
import torch

import hier_witness as W

FLT_MAX = W.FLT_MAX
AABB = np.array([-1, -1, -1, 1, 1, 1], dtype=np.float32)
MIN_NEAR = 0.2
SCALE = 1.0

# (N, S, U): N in {1, 63, 65, 1500} x (S, U) in {(3, 1), (64, 48), (65, 63), (64, 0)}; (512, 128) — configs[0]'s own shape, several
# values per lane — at N = 65.  N = 1 comes twice: the one ray misses the box ("miss") or starts inside it ("inside").
SHAPES = [(3, 1), (64, 48), (65, 63), (64, 0)]
CASES = [(n, s, u, kind) for (s, u) in SHAPES for (n, kind) in ((1, "miss"), (1, "inside"), (63, "mixed"), (65, "mixed"), (1500, "mixed"))]
CASES.append((65, 512, 128, "mixed"))
UPSAMPLE_CASES = [c for c in CASES if c[2] > 0]


def case_id(c):
    return f"N{c[0]}-S{c[1]}-U{c[2]}-{c[3]}"


KIND = {"miss": 0, "inside": 1, "mixed": 2}


@functools.lru_cache(maxsize=None)
def rays(N, kind):
    """fp32 rays towards the box [-1, 1]^3 from a sphere of radius 2.5.  "mixed" (N >= 3): ray 0 misses the box, ray 1 starts
    inside it; "miss" / "inside": every ray is of that sort."""
    g = np.random.default_rng([7, N, KIND[kind]])
    o = g.normal(size=(N, 3))
    o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = g.uniform(-0.6, 0.6, size=(N, 3)) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    miss = np.zeros(N, bool)
    inside = np.zeros(N, bool)
    if kind == "mixed":
        assert N >= 3
        miss[0], inside[1] = True, True
    elif kind == "miss":
        miss[:] = True
    else:
        inside[:] = True
    # (a tangent of the sphere: the whole line stays 2.5 > sqrt(3) from the centre; pointing away would not do, the slab test
    #  intersects lines, not half-lines)
    tangent = np.cross(o[miss], g.normal(size=(int(miss.sum()), 3)))
    d[miss] = tangent / np.linalg.norm(tangent, axis=1, keepdims=True)
    o[inside] = g.uniform(-0.3, 0.3, size=(int(inside.sum()), 3))
    o, d = o.astype(np.float32), d.astype(np.float32)
    o.setflags(write=False); d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def upsample_inputs(N, S, U, kind):
    """well-conditioned input of the upsampling: rays of length 1 (near in [1, 1.5]), stratified depths jittered by +-0.2 of a
    stratum and sigma uniform in [0.6, 1], so that no pdf bin holds less than 1 / (4 (S - 2)) (spacing >= 0.6, sigma >= 0.75 and
    transmittance >= 0.65 of their means; tests/test_hier_sampling.py checks it), the inverse CDF is continuous in rounding and no
    bin trips the `denom < 1e-5` rule.  A ray that misses (near = far = FLT_MAX, every depth FLT_MAX) is part of the batch where
    `kind` says so."""
    g = np.random.default_rng([11, N, S, U, KIND[kind]])
    o, d = rays(N, kind)
    near = g.uniform(1.0, 1.5, size=N).astype(np.float32)
    far = (near + np.float32(1.0)).astype(np.float32)
    if kind != "inside":
        near[0] = far[0] = np.float32(FLT_MAX)
    noise = g.uniform(0.3, 0.7, size=(N, S)).astype(np.float32)
    lin = torch.linspace(0.0, 1.0, S).numpy()
    z = near[:, None] + (far - near)[:, None] * lin[None, :]
    z = (z + (noise - np.float32(0.5)) * ((far - near) / np.float32(S))[:, None]).astype(np.float32)
    sigma = g.uniform(0.6, 1.0, size=(N, S)).astype(np.float32)
    u = g.uniform(size=(N, max(U, 1))).astype(np.float32)[:, :U]
    out = dict(rays_o=o, rays_d=d, nears=near, fars=far, z=z, sigma=sigma, u=u)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def composite_inputs(N, S, U, kind):
    """given merged rows for the weights, the compositing and its backward: sorted depths, a random `order` (the identity for
    U = 0), sigma from empty to opaque (10 % exact zeros, 10 % in [1e2, 1e4], the rest in [1e-3, 10]: 1 - alpha reaches 0 and
    s = 1e-15), colours in [0, 1], and upstream gradients for all three outputs."""
    g = np.random.default_rng([13, N, S, U, KIND[kind]])
    K = S + U
    near = g.uniform(0.2, 1.5, size=N).astype(np.float32)
    far = (near + g.uniform(0.5, 2.0, size=N).astype(np.float32)).astype(np.float32)
    z = np.sort(near[:, None] + (far - near)[:, None] * g.uniform(size=(N, K)).astype(np.float32), axis=1).astype(np.float32)
    if kind != "inside":
        near[0] = far[0] = np.float32(FLT_MAX)
        z[0] = np.float32(FLT_MAX)
    order = None if U == 0 else np.argsort(g.uniform(size=(N, K)), axis=1).astype(np.int32)
    pick = g.uniform(size=(N, K))
    sigma = 10.0 ** g.uniform(-3, 1, size=(N, K))
    sigma = np.where(pick < 0.1, 0.0, np.where(pick > 0.9, 10.0 ** g.uniform(2, 4, size=(N, K)), sigma)).astype(np.float32)
    out = dict(nears=near, fars=far, z_sorted=z, sigma_cat=sigma, rgbs=g.uniform(size=(N, K, 3)).astype(np.float32),
               grad_image=g.normal(size=(N, 3)).astype(np.float32), grad_weights_sum=g.normal(size=N).astype(np.float32),
               grad_depth=g.normal(size=N).astype(np.float32))
    if order is not None:
        out["order"] = order
    for v in out.values():
        v.setflags(write=False)
    out.setdefault("order", None)
    return out


# ---- the semi-transparent scene of the whole-route tests -----------------------------------------------------------------------
# sigma(x) = 2.5 exp(-|x|^2 / (2 0.3^2)) in the box of bound 1: the line integral through the centre is 2.5 * 0.3 * sqrt(2 pi) = 1.88,
# so weights_sum <= 1 - exp(-1.88) = 0.85 on every ray; below 0.9 no pdf bin falls under the 1e-5 rule
SIGMA0, WIDTH = 2.5, 0.3


def gauss_density_np(x):
    return SIGMA0 * np.exp(-(x ** 2).sum(axis=1) / (2 * WIDTH ** 2))


def analytic_color_np(x, d):
    return np.clip(x * 0.5 + 0.5, 0, 1) * (0.5 + 0.5 * np.abs(d))


def gauss_renderer():
    from nerf import renderer

    class GaussRun(renderer.NeRFRenderer):
        def density(self, x):
            return {"sigma": SIGMA0 * torch.exp(-(x ** 2).sum(dim=-1) / (2 * WIDTH ** 2))}

        def color(self, x, dd, mask=None, **kw):
            rgb = (x * 0.5 + 0.5).clamp(0, 1) * (0.5 + 0.5 * dd.abs())
            if mask is None:
                return rgb
            out = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            out[mask] = rgb[mask]
            return out
    return GaussRun(bound=1, cuda_ray=False, density_scale=SCALE, min_near=MIN_NEAR)


# ---- the torch fp32 op sequence of the reference (nerf/renderer.py:12-46, :174-186, :205-229) on given inputs -------------------
def _tensor(v, dtype, device="cpu"):
    return torch.tensor(np.asarray(v)).to(device=device, dtype=dtype)  # (a copy: the cached arrays are read-only)


def torch_alpha_weights(z, sigma, sample_dist, scale):
    d = torch.cat([z[..., 1:] - z[..., :-1], sample_dist * torch.ones_like(z[..., :1])], dim=-1)
    alphas = 1 - torch.exp(-d * scale * sigma)
    shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], dim=-1)
    return alphas * torch.cumprod(shifted, dim=-1)[..., :-1], d


def torch_sample_pdf(bins, weights, u):
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = ca - cb
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return bb + (u - cb) / denom * (ba - bb)


def torch_upsample(inp, u, dtype=torch.float32, device="cpu"):
    """new_z of the torch op sequence; u None: the deterministic row"""
    t = {k: _tensor(v, dtype, device) for k, v in inp.items()}
    N, S = t["z"].shape
    sample_dist = ((t["fars"] - t["nears"]) / S).unsqueeze(-1)
    w, d = torch_alpha_weights(t["z"], t["sigma"], sample_dist, SCALE)
    z_mid = t["z"][..., :-1] + 0.5 * d[..., :-1]
    if u is None:
        U = inp["u"].shape[1]
        uu = torch.linspace(0.0 + 0.5 / U, 1.0 - 0.5 / U, steps=U).to(device=device, dtype=dtype).expand(N, U)
    else:
        uu = _tensor(u, dtype, device)
    return torch_sample_pdf(z_mid, w[:, 1:-1], uu)


def torch_composite(inp, S, dtype=torch.float32, device="cpu", grads=True):
    """weights (concatenated order), weights_sum, depth, image and — grads — d/d sigma_cat, d/d rgbs of the torch op sequence"""
    t = {k: _tensor(v, dtype, device) for k, v in inp.items() if v is not None and k != "order"}
    N, K = t["z_sorted"].shape
    order = torch.arange(K, device=device).expand(N, K) if inp["order"] is None else _tensor(inp["order"], torch.int64, device)
    sigma, rgbs = t["sigma_cat"].requires_grad_(grads), t["rgbs"].requires_grad_(grads)
    nears, fars = t["nears"].unsqueeze(-1), t["fars"].unsqueeze(-1)
    w_sorted, _ = torch_alpha_weights(t["z_sorted"], torch.gather(sigma, 1, order), (fars - nears) / S, SCALE)
    rgb_sorted = torch.gather(rgbs, 1, order.unsqueeze(-1).expand(N, K, 3))
    ws = w_sorted.sum(dim=-1)
    depth = torch.sum(w_sorted * ((t["z_sorted"] - nears) / (fars - nears)).clamp(0, 1), dim=-1)
    image = torch.sum(w_sorted.unsqueeze(-1) * rgb_sorted, dim=-2)
    weights = torch.empty_like(w_sorted).scatter_(1, order, w_sorted.detach())
    out = dict(weights=weights, weights_sum=ws.detach(), depth=depth.detach(), image=image.detach())
    if grads:
        # (a missing ray's depth is NaN and so is every sigma gradient of that ray, on every route: compared as a NaN pattern)
        loss = (image * t["grad_image"]).sum() + (ws * t["grad_weights_sum"]).sum() + (depth * t["grad_depth"]).sum()
        loss.backward()
        out["grad_sigma"], out["grad_rgbs"] = sigma.grad, rgbs.grad
    return out


# ---- error measures -------------------------------------------------------------------------------------------------------
def err_new_z(got, ref, inp):
    """largest |new_z - witness| in units of the ray's length, over the rays that hit (a miss must give FLT_MAX exactly)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    hit = inp["nears"] < FLT_MAX
    assert np.array_equal(got[~hit], ref[~hit])
    if not hit.any():
        return 0.0
    span = (inp["fars"].astype(np.float64) - inp["nears"].astype(np.float64))[hit]
    return float((np.abs(got[hit] - ref[hit]) / span[:, None]).max())


def err_abs(got, ref):
    """largest absolute error; NaNs must sit in the same places"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    return float(np.nanmax(np.abs(got - ref), initial=0.0))


def err_rel(got, ref):
    """largest absolute error over the largest magnitude of the witness"""
    return err_abs(got, ref) / max(float(np.nanmax(np.abs(np.asarray(ref, dtype=np.float64)), initial=0.0)), 1e-30)


def witness_composite(inp, S):
    """the witness on `composite_inputs`: weights, mask, weights_sum, depth, image, grad_sigma, grad_rgbs"""
    w, mask = W.weights(inp["z_sorted"], inp["order"], inp["sigma_cat"], inp["nears"], inp["fars"], SCALE, S)
    ws, depth, image = W.composite(w, inp["rgbs"], inp["z_sorted"], inp["order"], inp["nears"], inp["fars"])
    gs, gr = W.composite_backward(inp["grad_image"], inp["grad_weights_sum"], inp["grad_depth"], inp["sigma_cat"], inp["rgbs"],
                                  inp["z_sorted"], inp["order"], inp["nears"], inp["fars"], SCALE, S)
    return dict(weights=w, mask=mask, weights_sum=ws, depth=depth, image=image, grad_sigma=gs, grad_rgbs=gr)


def measure_torch_errors(cases=None):
    """the error of the torch fp32 op sequence against the float64 witness, largest over the cases: the provenance of TORCH_ERROR"""
    worst = dict.fromkeys(TORCH_ERROR, 0.0)

    def note(key, v):
        worst[key] = max(worst[key], v)
    for (N, S, U, kind) in (CASES if cases is None else cases):
        if U > 0:
            inp = upsample_inputs(N, S, U, kind)
            for u in (None, inp["u"]):
                ref = W.upsample(inp["z"], inp["sigma"], inp["nears"], inp["fars"], SCALE, u, U, inp["rays_o"], inp["rays_d"], AABB)[0]
                note("new_z", err_new_z(torch_upsample(inp, u).numpy(), ref, inp))
        inp = composite_inputs(N, S, U, kind)
        ref, got = witness_composite(inp, S), torch_composite(inp, S)
        note("weights", err_abs(got["weights"].numpy(), ref["weights"]))
        for k in ("weights_sum", "depth", "image"):
            note("composite", err_abs(got[k].numpy(), ref[k]))
        note("grad_sigma", err_rel(got["grad_sigma"].numpy(), ref["grad_sigma"]))
        note("grad_rgbs", err_rel(got["grad_rgbs"].numpy(), ref["grad_rgbs"]))
    return worst


# Measured with `measure_torch_errors()` on the CPU (torch fp32 against the float64 witness, largest over CASES); the kernels get
# KERNEL_MARGIN times these.  new_z: in units of the ray's length; weights, composite (weights_sum / depth / image): absolute, the
# values are O(1); grad_sigma, grad_rgbs: relative to the largest gradient of the case.
TORCH_ERROR = {
    "new_z": 9.6e-7,
    "weights": 2.8e-7,
    "composite": 2.2e-7,
    "grad_sigma": 4.3e-7,
    "grad_rgbs": 1.4e-7,
}
KERNEL_MARGIN = 4.0


def bound(key):
    return KERNEL_MARGIN * TORCH_ERROR[key]
