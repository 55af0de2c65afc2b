#!/usr/bin/env python3
"""Cost of the SDF backbone's data path and training step on one MI355X, in ONE process with device events around each call,
medians; prints one JSON line.

  * mesh_sdf: s3d_mesh_sdf at N = 2^17 points against UV spheres of F = 1,280 triangles and upwards in steps of 4x until a call
    takes more than 100 ms: pair tests per second, and the share of the fp32 vector rate (157.3 TFLOP/s, which counts a fused
    multiply-add as two; the library is built without contraction, so a kernel of separate multiplies and adds can reach half of it)
    at OPS_PER_PAIR fp32 operations per pair test, counted from the source of csrc/sdf.hip with atan2f taken as 40 and sqrtf as 1;
  * torch: the same query as a chunked torch op sequence on the device (what a user would otherwise write), at the sizes it
    finishes in reasonable time;
  * sampler: the s3d_sdf_sample_points launch at 2^18 rows; item: a whole dataset item (sample + distance) at 2^18 rows;
  * step: the training step (forward, criterion, backward, Adam, scaler) at the reference's 2^18 points under fp16 autocast,
    fused route against torch route, alternating call by call on one model.

    python tools/bench_sdf.py [--reps 9]

`--accel bvh` or `--accel both` prints the BVH sweep instead (profiles/sdf_bvh.md): s3d_mesh_sdf_bvh, alone or alternating call by
call with s3d_mesh_sdf, at N = 2^17 uniform points and at an item's own rows [N/2, N), on UV spheres and tori of 1,280 faces and
upwards in steps of 4x up to 327,680; the BVH on the same rows in Morton order; max |dw|, bit equality of distance and face;
the host build; a whole 2^18-row item.  The default, `--accel brute`, is the line described above.
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]

N_QUERY = 2 ** 17
OPS_PER_PAIR = 180
PEAK_FP32 = 157.3e12


def uv_sphere(nu, nv, radius=0.8, weld=False):
    """(vertices, faces) of a latitude / longitude sphere with 2 nu nv outward-facing triangles, of which the 2 nv that touch a pole
    with two corners have no area; `weld`: the poles' corners share one vertex each and those triangles are dropped (a closed mesh)"""
    th = np.linspace(0, np.pi, nu + 1)[:, None]
    ph = np.linspace(0, 2 * np.pi, nv, endpoint=False)[None, :]
    v = radius * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * np.ones_like(ph)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b, c, d = i * nv + j, i * nv + (j + 1) % nv, (i + 1) * nv + j, (i + 1) * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, c, d], -1).reshape(-1, 3), np.stack([a, d, b], -1).reshape(-1, 3)])
    if weld:
        f = np.where(f < nv, 0, np.where(f >= nu * nv, nu * nv, f))
        f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    return v, f


def _timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "invocations": reps}


def _alternate(variants, reps, warm=2):
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
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "invocations": reps} for k, v in ms.items()}


def torch_mesh_sdf(points, tris, chunk=16):
    """the contract of s3d_mesh_sdf as torch ops, `chunk` faces at a time against all points"""
    def dot(a, b):
        return (a * b).sum(-1)

    def seg2(p, e):
        ee = dot(e, e)
        t = torch.where(ee > 1e-30, dot(p, e) / ee.clamp_min(1e-30), torch.zeros_like(ee)).clamp(0, 1)
        v = p - t.unsqueeze(-1) * e
        return dot(v, v)
    N = points.shape[0]
    best = torch.full((N,), float("inf"), device=points.device)
    omega = torch.zeros(N, device=points.device)
    p = points[:, None, :]
    for head in range(0, tris.shape[0], chunk):
        t = tris[head:head + chunk]
        A, B, C = t[None, :, 0], t[None, :, 1], t[None, :, 2]
        ab, ac, bc = B - A, C - A, C - B
        ap = p - A
        d2 = torch.minimum(torch.minimum(seg2(ap, ab.expand_as(ap)), seg2(ap, ac.expand_as(ap))), seg2(p - B, bc.expand_as(ap)))
        # (products and differences as separate ops: torch.cross contracts them into fused multiply-adds, which leaves rounding noise
        #  instead of an exact zero as the normal of a triangle whose two edges are equal in fp32)
        n = torch.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                         ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], dim=-1)
        nn = dot(n, n)
        d00, d01, d11, d20, d21 = dot(ab, ab), dot(ab, ac), dot(ac, ac), dot(ap, ab), dot(ap, ac)
        v, w = d11 * d20 - d01 * d21, d00 * d21 - d01 * d20
        pn = dot(ap, n)
        inside = (nn > 1e-30) & (v >= 0) & (w >= 0) & (v + w <= d00 * d11 - d01 * d01)
        d2 = torch.where(inside, torch.minimum(d2, pn * pn / nn.clamp_min(1e-30)), d2)
        best = torch.minimum(best, d2.min(dim=1).values)
        a, b, c = -ap, B - p, C - p
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        om = 2 * torch.atan2(-pn, den)
        omega += torch.where((nn > 1e-30) & (pn != 0), om, torch.zeros_like(om)).sum(dim=1)
    dist = best.sqrt()
    return torch.where(omega / (4 * np.pi) > 0.5, -dist, dist)


def query(reps):
    import s3d_hip
    S = s3d_hip.SdfBackend
    pts = (torch.rand(N_QUERY, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
    out = {"points": N_QUERY, "ops_per_pair": OPS_PER_PAIR, "sizes": {}}
    nu, nv = 20, 32
    while True:
        v, f = uv_sphere(nu, nv)
        tris = torch.from_numpy(v[f].astype(np.float32)).cuda()
        F = tris.shape[0]
        r = _timed(lambda: S.mesh_sdf(pts, tris), reps)
        rate = N_QUERY * F / (r["median"] * 1e-3)
        r.update(pairs_per_second=rate, share_of_fp32_vector_peak=rate * OPS_PER_PAIR / PEAK_FP32)
        if F <= 5120:
            got, ref = S.mesh_sdf(pts, tris), torch_mesh_sdf(pts, tris)
            r["torch_chunked"] = _timed(lambda: torch_mesh_sdf(pts, tris), max(reps // 3, 2), warm=1)
            r["torch_chunked"]["max_abs_difference"] = float((got - ref).abs().max())
        out["sizes"][str(F)] = r
        if r["median"] > 100.0 or F > 4_000_000:
            break
        nu, nv = nu * 2, nv * 2
    return out


def sampler_and_item(reps):
    import s3d_hip
    from sdf.provider import SDFDataset
    v, f = uv_sphere(20, 32, weld=True)
    with contextlib.redirect_stdout(sys.stderr):  # (the dataset reports the mesh it loaded: not part of the result line)
        ds = SDFDataset((v, f), num_samples=2 ** 18, accel="brute")
    return {"rows": 2 ** 18, "faces": len(ds.faces),
            "sampler": _timed(lambda: s3d_hip.SdfBackend.sample_points(ds.triangles, ds.cdf, 2 ** 18, 0, 1), reps),
            "item": _timed(lambda: ds[1], reps)}


def step(reps):
    from sdf.network import SDFNetwork
    from sdf.provider import SDFDataset
    from sdf.utils import Trainer
    v, f = uv_sphere(20, 32, weld=True)
    with contextlib.redirect_stdout(sys.stderr):  # (the dataset reports the mesh it loaded: not part of the result line)
        ds = SDFDataset((v, f), num_samples=2 ** 18, accel="brute")
    torch.manual_seed(0)
    net = SDFNetwork(encoding="hashgrid")
    tr = Trainer("bench", net, fp16=True, mute=True)
    data = {k: t[None] for k, t in ds[0].items()}
    net.train()
    routes = {}

    def one(fused):
        def run():
            net.fused_mlp = fused
            tr.optimizer.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                _, _, loss = tr.train_step(data)
            tr.scaler.scale(loss).backward()
            tr.scaler.step(tr.optimizer)
            tr.scaler.update()
            routes[fused] = float(loss)
        return run
    res = _alternate({"fused": one(True), "torch": one(False)}, reps)
    net.fused_mlp = True
    return {"points": 2 ** 18, "ms": res, "last_loss": {"fused": routes[True], "torch": routes[False]}}


def torus(nu, nv, R=0.6, r=0.25):
    """(vertices, faces) of a closed torus with 2 nu nv outward-facing triangles, none without area"""
    th = np.linspace(0, 2 * np.pi, nu, endpoint=False)[:, None]
    ph = np.linspace(0, 2 * np.pi, nv, endpoint=False)[None, :]
    v = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph) * np.ones_like(th)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b, c, d = i * nv + j, i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, c, d], -1).reshape(-1, 3), np.stack([a, d, b], -1).reshape(-1, 3)])
    return v, f


def _morton_order(points):
    """row order of points in [-1, 1]^3 along a 30-bit Morton curve (an experiment: the cost of the sort is not timed)"""
    q = ((points.clamp(-1, 1) + 1) * 511.5).long().clamp(0, 1023)
    code = torch.zeros(points.shape[0], dtype=torch.long, device=points.device)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return torch.argsort(code)


def bvh_sweep(reps, accel, max_faces=327680):
    """brute force against the BVH in one process, alternating call by call: N = 2^17 uniform points and an item's own rows
    [N/2, N) (perturbed surface + uniform), UV spheres and tori of 1,280 faces and upwards in steps of 4x; the BVH also on the
    same rows in Morton order; the host build; a whole item of 2^18 rows"""
    import time
    import warnings
    import s3d_hip
    from sdf.provider import SDFDataset
    S = s3d_hip.SdfBackend
    uniform = (torch.rand(N_QUERY, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
    out = {"points": N_QUERY, "beta": 3.0, "leaf": S.bvh_leaf(), "meshes": {}}
    for mesh_name, make in (("uv_sphere", uv_sphere), ("torus", torus)):
        sizes, nu, nv = {}, 20, 32
        while 2 * nu * nv <= max_faces:
            v, f = make(nu, nv)
            with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                ds = SDFDataset((v, f), num_samples=2 * N_QUERY, accel="bvh")
                t_ds = time.perf_counter() - t0
                t0 = time.perf_counter()
                type(ds.bvh)(ds.bvh.triangles_sorted)
                t_build = time.perf_counter() - t0
            item_rows = S.sample_points(ds.triangles, ds.cdf, 2 * N_QUERY, 0, 1)[N_QUERY:].contiguous()
            r = {"host_build_s": t_build, "dataset_init_s": t_ds, "leaves": ds.bvh.L}
            for set_name, pts in (("uniform", uniform), ("item_rows", item_rows)):
                ordered = pts[_morton_order(pts)].contiguous()
                variants = {}
                if accel in ("brute", "both"):
                    variants["brute"] = lambda pts=pts: S.mesh_sdf(pts, ds.triangles)
                if accel in ("bvh", "both"):
                    variants["bvh"] = lambda pts=pts: S.mesh_sdf_bvh(pts, ds.bvh)
                    variants["bvh_morton_ordered_rows"] = lambda ordered=ordered: S.mesh_sdf_bvh(ordered, ds.bvh)
                res = _alternate(variants, reps)
                if accel == "both":
                    s0, w0, f0 = S.mesh_sdf(pts, ds.triangles, want_winding=True, want_face=True)
                    s1, w1, f1 = S.mesh_sdf_bvh(pts, ds.bvh, want_winding=True, want_face=True)
                    res["max_abs_dw"] = float((w0 - w1).abs().max())
                    res["distance_bits_equal"] = bool(torch.equal(s0.abs().view(torch.int32), s1.abs().view(torch.int32)))
                    res["faces_equal"] = bool(torch.equal(f0, f1))
                    res["signs_differ"] = int(((s0 < 0) != (s1 < 0)).sum())
                    res["nan"] = int(torch.isnan(s1).sum())
                r[set_name] = res
            if accel in ("bvh", "both"):
                r["item_2^18_rows_bvh"] = _timed(lambda: ds[1], reps)
            sizes[str(len(f))] = r
            nu, nv = nu * 2, nv * 2
        out["meshes"][mesh_name] = sizes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--accel", choices=("brute", "bvh", "both"), default="brute",
                    help="brute: the figures above (the default); bvh / both: the BVH sweep instead, alone or against brute force")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdf: needs a GPU (no CPU timing is meaningful here)")
    if a.accel != "brute":
        print(json.dumps({"metric": "SDF mesh distance query: brute force against the BVH", "device": torch.cuda.get_device_name(0),
                          "sweep": bvh_sweep(a.reps, a.accel)}))
        return
    res = {"metric": "SDF backbone: mesh distance query, sampler, dataset item, training step", "device": torch.cuda.get_device_name(0),
           "mesh_sdf": query(a.reps), "dataset": sampler_and_item(a.reps), "step": step(a.reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
