#!/usr/bin/env python3
"""Cost of the mesh export on one MI355X; prints one JSON line.

  * s3d_mc_count (classify + count + scan) and s3d_mc_emit (with its read-back of the two totals) on a synthetic volume — a
    gyroid with four periods per axis, so the surface grows with n^2 — at 64^3, 256^3 and 512^3: wall time per call around a
    device synchronise, median of --reps after a warm-up; the mesh's size; the streaming lower bound of one pass (one 4-byte
    read per grid point at 8.0 TB/s, the HBM3E peak);
  * Trainer.save_mesh of the bench scene's model (nerf/network_ff on the synthetic Lego-like scene, --pretrain graph-replayed
    steps) at the same three resolutions: field extraction + marching cubes + the PLY on disk, wall time, median of 3.

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py` run.  Without a GPU the
script fails: it has no CPU path.

    python tools/bench_mesh.py [--reps 20] [--pretrain 256] [--sizes 64 256 512]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]

HBM_PEAK = 8.0e12  # bytes / s


def _wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def gyroid(n, periods=4.0):
    g = torch.linspace(0.0, periods * 2.0 * torch.pi, n, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return (torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)).contiguous()


def bench_kernels(n, reps):
    import s3d_hip
    lib = s3d_hip.lib()
    u = gyroid(n)
    u32 = C.c_uint32
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(lib.s3d_mc_workspace_bytes(u32(n), u32(n), u32(n))), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int32, device="cuda")
    bounds = torch.tensor([-1.0, -1, -1, 1, 1, 1], device="cuda")

    def count():
        rc = lib.s3d_mc_count(p(u), u32(n), u32(n), u32(n), C.c_float(0.0), p(ws), p(totals), stream)
        assert rc == 0, lib.s3d_last_error()
    count()
    V, T = (int(v) for v in totals.cpu().numpy().view("uint32"))
    verts = torch.empty(V, 3, device="cuda")
    tris = torch.empty(T, 3, dtype=torch.int32, device="cuda")

    def emit():
        rc = lib.s3d_mc_emit(p(u), u32(n), u32(n), u32(n), C.c_float(0.0), p(ws), p(bounds), p(verts), u32(V), p(tris), u32(T), stream)
        assert rc == 0, lib.s3d_last_error()
    c_med, c_min = _wall_ms(count, reps)
    e_med, e_min = _wall_ms(emit, reps)
    both_med, _ = _wall_ms(lambda: s3d_hip.MeshBackend.marching_cubes(u, 0.0, bounds), reps)
    return {"n": n, "points": n ** 3, "vertices": V, "triangles": T, "workspace_bytes": ws.numel(),
            "count_ms_median": c_med, "count_ms_min": c_min, "emit_ms_median": e_med, "emit_ms_min": e_min,
            "marching_cubes_ms_median": both_med, "stream_bound_ms_per_pass": 4.0 * n ** 3 / HBM_PEAK * 1e3,
            "output_bytes": 12 * (V + T)}


def bench_save_mesh(sizes, pretrain):
    import bench
    import s3d_hip
    from nerf import network_ff, synthetic as syn
    from nerf.trainer import GraphedTrainer
    torch.manual_seed(0)
    model = network_ff.NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    _, bits = syn.lego_like_density_grid(seed=0)
    batches, _ = bench.make_batches(16, 4096, 0, torch.device("cuda"), s3d_hip.RaymarchingBackend, torch.from_numpy(bits).cuda(),
                                    syn.lego_like_boxes(0))
    tr = GraphedTrainer(model, 4096, lr=1e-2, fp16=True)
    for i in range(pretrain):
        tr.train_step(*batches[i % len(batches)])
    torch.cuda.synchronize()
    out = []
    with tempfile.TemporaryDirectory() as d:
        for n in sizes:
            path = os.path.join(d, f"mesh_{n}.ply")
            med, lo = _wall_ms(lambda: tr.save_mesh(save_path=path, resolution=n, threshold=10), 3)
            from nerf.mesh import read_ply
            v, t = read_ply(path)
            out.append({"resolution": n, "save_mesh_ms_median": med, "save_mesh_ms_min": lo, "vertices": len(v), "triangles": len(t),
                        "file_bytes": os.path.getsize(path)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pretrain", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--no_save_mesh", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh needs a GPU: nothing is measured without one")
    res = {"metric": "mesh_export", "device": torch.cuda.get_device_name(0), "kernels": [bench_kernels(n, a.reps) for n in a.sizes]}
    if not a.no_save_mesh:
        res["save_mesh"] = bench_save_mesh(a.sizes, a.pretrain)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
