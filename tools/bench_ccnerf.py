#!/usr/bin/env python3
"""Cost of the CCNeRF backbone on one MI355X at its defaults (five groups: vector ranks 64, matrix ranks up to 16 / 64, degree 4,
resolution 300, 4,096 rays of the synthetic Lego-shaped scene, fp16 autocast); prints one JSON line.  Everything is measured in
ONE process, the variants alternating, device events around each call:

  * heads: the density head and the colour head in training mode (every level returned) on the marched samples of 4,096 rays,
    forward and forward + backward, fused kernels (csrc/tensorf_cc.hip) against the model's own grid_sample route
    (`fused_cc = False`) — the baseline, since no earlier CCNeRF path exists;
  * step: the eager training step (tensoRF.utils.Trainer) with the fused kernels, with the torch route, and the eager VM-48 step
    at the same resolution for scale.  The graph-replayed trainer refuses this backbone, so there is no graphed figure.

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_ccnerf.py --only heads` run.

    python tools/bench_ccnerf.py [--steps 20] [--reps 10] [--only heads|step] [--tags cc_torch]
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


def _cc(res=300):
    from tensoRF.network_cc import NeRFNetwork
    torch.manual_seed(0)
    return _scene(NeRFNetwork(resolution=[res] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda())


def _vm(res=300):
    from tensoRF.network import NeRFNetwork
    torch.manual_seed(0)
    return _scene(NeRFNetwork(resolution=[res] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda())


def _marched_samples(n_rays=4096):
    """ray-ordered samples and directions of the synthetic scene, as the training step hands them to the network"""
    import raymarching
    from nerf import synthetic as syn
    _, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(2, seed=0)[:1].cuda(), syn.lego_intrinsics(), 800, 800, N=n_rays, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1], device="cuda")
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, _, _ = raymarching.march_rays_train(ro, rd, 1.0, torch.from_numpy(bits).cuda(), 1, 128, nears, fars, counter, 0, False, 128,
                                                    True, 0, 1024)
    m = int(counter[0]) // 128 * 128
    return xyzs[:m].contiguous(), dirs[:m].contiguous()


def heads(reps):
    net = _cc().train()
    x, d = _marched_samples()
    m, K = x.shape[0], net.K[0]
    g = torch.Generator().manual_seed(1)
    gs, gc = (torch.randn(K, m, generator=g) * 0.1).cuda(), (torch.randn(K, m, 3, generator=g) * 0.1).cuda()

    def run():
        xm = net.normalize_coord(x)
        return net._head(xm, None, net._groups(True), True), net._head(xm, d, net._groups(False), True)

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            run()

    def fwd_bwd():
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            s, c = run()
        ((s.float() * gs).sum() + (c.float() * gc).sum()).backward()

    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))  # noqa: E731
    tot = {(f, k): 0.0 for f in (True, False) for k in ("fwd", "fwd_bwd")}
    for fused in (True, False):  # warm up every shape of the timed window
        net.fused_cc = fused
        for _ in range(2):
            fwd(), fwd_bwd()
    torch.cuda.synchronize()
    for _ in range(reps):  # alternating
        for fused in (True, False):
            net.fused_cc = fused
            for k, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                a, b = ev()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                tot[(fused, k)] += a.elapsed_time(b)
    net.fused_cc = True
    ranks = {"density": int(net.rank_vec_density[0][-1]) * 6 + int(net.rank_mat_density[0][-1]) * 12,
             "colour": int(net.rank_vec[0][-1]) * 6 + int(net.rank_mat[0][-1]) * 12}
    return {"points": m, "levels": K,
            "fused": {k: tot[(True, k)] / reps for k in ("fwd", "fwd_bwd")},
            "torch": {k: tot[(False, k)] / reps for k in ("fwd", "fwd_bwd")},
            "algorithmic_bytes_per_point": {k: v * 4 for k, v in ranks.items()},  # (taps x ranks x 4 B, read forward / added backward)
            "factor_bytes": {"density": sum(v.numel() for v in net.density_factors()) * 4,
                             "colour": sum(v.numel() for v in list(net.U_vec) + list(net.U_mat)) * 4}}


def steps(n_steps, tags=("cc_fused", "cc_torch", "vm48")):
    from nerf import synthetic as syn
    from tensoRF.utils import Trainer
    poses = syn.orbit_poses(8, seed=0)
    batches = []
    for i in range(8):
        r = syn.get_rays(poses[i:i + 1], syn.lego_intrinsics(), 800, 800, N=4096, generator=torch.Generator().manual_seed(i))
        batches.append((r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous(),
                        torch.rand(4096, 3, generator=torch.Generator().manual_seed(100 + i)).cuda()))
    trs = {}
    for tag in tags:
        net = _vm() if tag == "vm48" else _cc()
        if tag == "cc_torch":
            net.fused_cc = False  # (an instance attribute: this model only)
        tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9)
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
    out["samples_last_step"] = {k: int(v.model.step_counter[:, 0].max()) for k, v in trs.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["heads", "step"], default=None)
    ap.add_argument("--tags", default="cc_fused,cc_torch,vm48", help="the trainers of the step section (a kernel trace of one of them)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ccnerf: needs a GPU (no CPU timing is meaningful here)")
    res = {"metric": "ccnerf backbone cost"}
    if a.only in (None, "heads"):
        res["heads_ms"] = heads(a.reps)
    if a.only in (None, "step"):
        res["train_step"] = steps(a.steps, tuple(a.tags.split(",")))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
