#!/usr/bin/env python3
"""Cost of the TensoRF CP backbone on one MI355X at its defaults (density rank 96, colour rank 288, resolution 300, 4,096 rays
of the synthetic Lego-shaped scene); prints one JSON line.  Everything is measured in ONE process, the variants alternating:

  * features: `get_sigma_feat` + `get_color_feat` on the marched samples of 4,096 rays under fp16 autocast, forward and
    forward + backward, fused kernels (csrc/tensorf_cp.hip) against the reference's grid_sample sequence (`fused_cp = False`);
  * step: the graph-replayed training step (tensoRF.utils.GraphedTrainer) with the fused kernels, with the torch sequence, and
    the VM-48 step at the same resolution for scale;
  * bytes: the algorithmic traffic per point, 6 taps x R x 4 B, from the shapes.  L2 / HBM counters come from a separate
    `rocprofv3 --pmc` run of `--only features` (counters and tracing are never collected together).

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_tensorf_cp.py --only features` run.

    python tools/bench_tensorf_cp.py [--steps 50] [--reps 20] [--only features|step]
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]


def _scene(net):
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens).cuda())
    net.density_bitfield.copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


def _cp(res=300):
    from tensoRF.network_cp import NeRFNetwork
    torch.manual_seed(0)
    return _scene(NeRFNetwork(resolution=[res] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda())


def _vm(res=300):
    from tensoRF.network import NeRFNetwork
    torch.manual_seed(0)
    return _scene(NeRFNetwork(resolution=[res] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda())


def _marched_samples(n_rays=4096):
    """ray-ordered samples of the synthetic scene, as the training step hands them to the feature kernels"""
    import raymarching
    from nerf import synthetic as syn
    _, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(2, seed=0)[:1].cuda(), syn.lego_intrinsics(), 800, 800, N=n_rays, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1], device="cuda")
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, _, _, _ = raymarching.march_rays_train(ro, rd, 1.0, torch.from_numpy(bits).cuda(), 1, 128, nears, fars, counter, 0, False, 128,
                                                 True, 0, 1024)
    m = int(counter[0]) // 128 * 128
    return xyzs[:m].contiguous()


def features(reps):
    from tensoRF.network import BINS
    net = _cp()
    x = _marched_samples()
    m = x.shape[0]
    g = torch.Generator().manual_seed(1)
    gs, gc = torch.randn(m, generator=g).cuda(), (torch.randn(m, 27, generator=g) * 0.1).cuda()

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            net.get_sigma_feat(x), net.get_color_feat(x)

    def fwd_bwd():
        net.zero_grad(set_to_none=True)
        net.__dict__[BINS] = {}
        with torch.autocast("cuda", dtype=torch.float16):
            s, c = net.get_sigma_feat(x), net.get_color_feat(x)
        ((s * gs).sum() + (c.float() * gc).sum()).backward()

    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))  # noqa: E731
    tot = {(f, k): 0.0 for f in (True, False) for k in ("fwd", "fwd_bwd")}
    for fused in (True, False):  # warm up every shape of the timed window
        net.fused_cp = fused
        for _ in range(3):
            fwd(), fwd_bwd()
    torch.cuda.synchronize()
    for _ in range(reps):  # alternating
        for fused in (True, False):
            net.fused_cp = fused
            for k, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                a, b = ev()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                tot[(fused, k)] += a.elapsed_time(b)
    net.fused_cp = True
    R_s, R_c = net.sigma_rank[0], net.color_rank[0]
    return {"points": m,
            "fused": {k: tot[(True, k)] / reps for k in ("fwd", "fwd_bwd")},
            "torch": {k: tot[(False, k)] / reps for k in ("fwd", "fwd_bwd")},
            "algorithmic_bytes_per_point": {"density": 6 * R_s * 4, "colour": 6 * R_c * 4},
            "factor_bytes": {"density": sum(v.numel() for v in net.sigma_vec) * 4, "colour": sum(v.numel() for v in net.color_vec) * 4}}


def steps(n_steps):
    from nerf import synthetic as syn
    from tensoRF.utils import GraphedTrainer
    poses = syn.orbit_poses(8, seed=0)
    batches = []
    for i in range(8):
        r = syn.get_rays(poses[i:i + 1], syn.lego_intrinsics(), 800, 800, N=4096, generator=torch.Generator().manual_seed(i))
        batches.append((r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous(),
                        torch.rand(4096, 3, generator=torch.Generator().manual_seed(100 + i)).cuda()))
    trs = {}
    for tag in ("cp_fused", "cp_torch", "vm48"):
        net = _vm() if tag == "vm48" else _cp()
        if tag == "cp_torch":
            net.fused_cp = False  # (an instance attribute: this model only)
        tr = GraphedTrainer(net, 4096, lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9)
        tr.global_step = 1
        net.mean_count = 4096 * 70
        for i in range(3):
            tr.train_step(*batches[i % 8])
        trs[tag] = tr
    torch.cuda.synchronize()
    tot = {k: 0.0 for k in trs}
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in trs}
    for i in range(n_steps):  # alternating, one step each
        for tag, tr in trs.items():
            a, b = ev[tag]
            a.record()
            tr.train_step(*batches[i % 8])
            b.record()
            torch.cuda.synchronize()
            tot[tag] += a.elapsed_time(b)
    out = {f"{k}_ms_per_step": v / n_steps for k, v in tot.items()}
    out["captures"] = {k: v.n_captures for k, v in trs.items()}
    out["samples_last_step"] = {k: int(v.model.step_counter[:, 0].max()) for k, v in trs.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["features", "step"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensorf_cp: needs a GPU (no CPU timing is meaningful here)")
    res = {"metric": "tensorf cp backbone cost"}
    if a.only in (None, "features"):
        res["features_ms"] = features(a.reps)
    if a.only in (None, "step"):
        res["train_step"] = steps(a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
