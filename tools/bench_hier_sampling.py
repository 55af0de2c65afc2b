#!/usr/bin/env python3
"""Cost of the sampling path without the occupancy grid (`NeRFRenderer.run`, cuda_ray off) on one MI355X: the native route
(csrc/hiersample.hip) against the torch route it replaces (`native_sampling = False`), in ONE process, the two alternating call by
call, device events around each call, medians; prints one JSON line.

  * route: the NGP network bench.py renders configs[0]'s frame with (nerf/network.py, hash table 2^19, fp16 autocast), 4,096 rays of
    the synthetic Lego-shaped scene at (num_steps, upsample_steps) = (128, 128) in one call and (512, 128) staged in 1,024-ray chunks
    as bench.py stages it: eval forward, and training forward + backward (perturb on, MSE on the image), with the number of device
    kernels either route launches per call (torch.profiler);
  * kernels: (a) - (d) and the backward alone on 4,096 rays against the torch ops they replace on the same inputs (a 15-wide
    geo_feat standing in for the density outputs the torch route reorders).

    python tools/bench_hier_sampling.py [--reps 15] [--only route|kernels] [--no_launch_counts]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]

N_RAYS = 4096
SHAPES = [(128, 128, N_RAYS), (512, 128, 1024)]  # (S, U, rays per call)


def _alternate(variants, reps, warm=3):
    """{name: fn} -> {name: {median, min, max} ms}, one call of each per round"""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}


def _launches(fn):
    """device kernels one call of fn launches"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def _rays():
    from nerf import synthetic as syn
    r = syn.get_rays(syn.orbit_poses(1, seed=0).cuda(), syn.lego_intrinsics(), 800, 800, N=N_RAYS, generator=torch.Generator().manual_seed(0))
    return r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()


def route(reps, launch_counts):
    from nerf.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, cuda_ray=False, density_scale=1, min_near=0.2).cuda()
    ro, rd = _rays()
    gt = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(1)).cuda()
    out = {}
    for S, U, chunk in SHAPES:
        def forward(native):
            def run():
                net.native_sampling = native
                net.eval()
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    net.render(ro[None], rd[None], staged=True, max_ray_batch=chunk, bg_color=1, perturb=False, num_steps=S, upsample_steps=U)
            return run

        def forward_backward(native):
            def run():
                net.native_sampling = native
                net.train()
                net.zero_grad(set_to_none=True)
                for head in range(0, N_RAYS, chunk):
                    with torch.autocast("cuda", dtype=torch.float16):
                        res = net.run(ro[head:head + chunk], rd[head:head + chunk], bg_color=1, perturb=True, num_steps=S, upsample_steps=U)
                        loss = ((res["image"].float() - gt[head:head + chunk]) ** 2).mean()
                    loss.backward()
            return run
        variants = {"native_eval": forward(True), "torch_eval": forward(False), "native_train": forward_backward(True),
                    "torch_train": forward_backward(False)}
        res = {"rays": N_RAYS, "rays_per_call": chunk, "ms": _alternate(variants, reps)}
        if launch_counts:
            try:
                res["device_kernels_per_call"] = {k: _launches(fn) for k, fn in variants.items()}
            except Exception as e:  # (a profiler that cannot trace this device: the timings stand, the counts are missing)
                res["device_kernels_per_call"] = f"not measured: {type(e).__name__}: {e}"
        forward(True)()
        assert net.last_sampling_route == "native"  # (the shape is one the kernels cover: the A side ran them)
        out[f"S{S}_U{U}"] = res
    net.native_sampling = True
    return out


def kernels(reps):
    import raymarching
    import s3d_hip
    from nerf.renderer import sample_pdf
    H = s3d_hip.HierBackend
    ro, rd = _rays()
    N = N_RAYS
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1], device="cuda")
    out = {}
    for S, U, _ in SHAPES:
        K = S + U
        g = torch.Generator().manual_seed(S)
        noise = torch.rand(N, S, generator=g).cuda()
        sigma = (torch.rand(N, K, generator=g) * 4).cuda()
        feat = torch.randn(N, K, 15, generator=g).cuda().half()
        rgbs = torch.rand(N, K, 3, generator=g).cuda()
        g_img = torch.randn(N, 3, generator=g).cuda()
        nears, fars, z, xyz = (torch.empty(s, device="cuda") for s in ((N,), (N,), (N, S), (N, S, 3)))
        new_z, new_xyz, zs = (torch.empty(s, device="cuda") for s in ((N, U), (N, U, 3), (N, K)))
        order = torch.empty(N, K, dtype=torch.int32, device="cuda")
        w, mask = torch.empty(N, K, device="cuda"), torch.empty(N, K, dtype=torch.bool, device="cuda")
        ws, dp, im = torch.empty(N, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, 3, device="cuda")
        gs, gr = torch.empty(N, K, device="cuda"), torch.empty(N, K, 3, device="cuda")
        sig_c = sigma[:, :S].contiguous()

        def pts(zz):
            return torch.min(torch.max(ro.unsqueeze(-2) + rd.unsqueeze(-2) * zz.unsqueeze(-1), aabb[:3]), aabb[3:])

        def alpha_weights(zz, sg, sd):
            d = torch.cat([zz[..., 1:] - zz[..., :-1], sd * torch.ones_like(zz[..., :1])], dim=-1)
            al = 1 - torch.exp(-d * sg)
            sh = torch.cat([torch.ones_like(al[..., :1]), 1 - al + 1e-15], dim=-1)
            return al * torch.cumprod(sh, dim=-1)[..., :-1], d

        def t_coarse():
            n, f = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
            n, f = n.unsqueeze(-1), f.unsqueeze(-1)
            zz = n + (f - n) * torch.linspace(0.0, 1.0, S, device="cuda").unsqueeze(0).expand((N, S))
            zz = zz + (noise - 0.5) * ((f - n) / S)
            return zz, pts(zz), n, f
        tz, txyz, tn, tf = t_coarse()
        sd = (tf - tn) / S

        def t_upsample():  # coarse weights, sample_pdf (deterministic: no host draw inside the timing), sort, the reordering gathers
            ww, d = alpha_weights(tz, sig_c, sd)
            zm = tz[..., :-1] + 0.5 * d[..., :-1]
            nz = sample_pdf(zm, ww[:, 1:-1], U, det=True)
            nx = pts(nz)
            zz, od = torch.sort(torch.cat([tz, nz], dim=1), dim=1)
            xx = torch.gather(torch.cat([txyz, nx], dim=1), 1, od.unsqueeze(-1).expand(N, K, 3))
            sg = torch.gather(sigma, 1, od)
            ft = torch.gather(feat, 1, od.unsqueeze(-1).expand_as(feat))
            return zz, od, xx, sg, ft
        tzs, tod, _, tsg, _ = t_upsample()
        trgb = torch.gather(rgbs, 1, tod.unsqueeze(-1).expand(N, K, 3))

        def t_weights():
            ww, _ = alpha_weights(tzs, tsg, sd)
            return ww, ww > 1e-4

        def t_composite(ww=None):
            ww = t_weights()[0] if ww is None else ww
            return ww.sum(dim=-1), torch.sum(ww * ((tzs - tn) / (tf - tn)).clamp(0, 1), dim=-1), torch.sum(ww.unsqueeze(-1) * trgb, dim=-2)
        tw = t_weights()[0]

        def t_forward_backward():  # weights + compositing + autograd to sigma and rgbs (the image's gradient)
            sg, cc = tsg.detach().requires_grad_(True), trgb.detach().requires_grad_(True)
            ww, _ = alpha_weights(tzs, sg, sd)
            (torch.sum(ww.unsqueeze(-1) * cc, dim=-2) * g_img).sum().backward()
            return sg.grad, cc.grad

        def n_forward_composite():
            H.weights(zs, order, sigma, nears, fars, 1.0, S, w, mask)
            H.composite_forward(w, rgbs, zs, order, nears, fars, S, ws, dp, im)

        def n_forward_backward():
            n_forward_composite()
            H.composite_backward(g_img, None, None, sigma, rgbs, zs, order, nears, fars, 1.0, S, gs, gr)
        H.coarse_samples(ro, rd, aabb, 0.2, S, nears, fars, z, xyz, noise)
        H.upsample(z, sig_c, nears, fars, 1.0, None, ro, rd, aabb, U, new_z, new_xyz, zs, order)
        out[f"S{S}_U{U}"] = {"rays": N, "ms": _alternate({
            "a_coarse": lambda: H.coarse_samples(ro, rd, aabb, 0.2, S, nears, fars, z, xyz, noise),
            "a_coarse_torch": t_coarse,
            "b_upsample": lambda: H.upsample(z, sig_c, nears, fars, 1.0, None, ro, rd, aabb, U, new_z, new_xyz, zs, order),
            "b_upsample_torch": t_upsample,
            "c_weights": lambda: H.weights(zs, order, sigma, nears, fars, 1.0, S, w, mask),
            "c_weights_torch": t_weights,
            "d_composite": lambda: H.composite_forward(w, rgbs, zs, order, nears, fars, S, ws, dp, im),
            "d_composite_torch": lambda: t_composite(tw),
            "cd_forward_backward": n_forward_backward,
            "cd_forward_backward_torch": t_forward_backward,
        }, reps)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["route", "kernels"], default=None)
    ap.add_argument("--no_launch_counts", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hier_sampling: needs a GPU (no CPU timing is meaningful here)")
    res = {"metric": "sampling path without the occupancy grid: native vs torch route", "device": torch.cuda.get_device_name(0)}
    if a.only in (None, "kernels"):
        res["kernels"] = kernels(a.reps)
    if a.only in (None, "route"):
        res["route"] = route(a.reps, not a.no_launch_counts)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
