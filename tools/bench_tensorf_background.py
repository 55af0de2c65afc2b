#!/usr/bin/env python3
"""Cost of the TensoRF background model (bg_radius > 0) on one MI355X; prints one JSON line.

  * bg forward and forward + backward per call (fused kernels vs the network's torch op sequence, `fused_background = False`, in
    the same process under fp16 autocast) at 4,096 and 640,000 rays, default plane [512, 512];
  * the graph-replayed TensoRF training step (VM-48 network at resolution 300, 4,096 rays, synthetic Lego-shaped scene) with and
    without the model, the two trainers stepped alternately in one process;
  * the 800x800 frame with and without the model.

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_tensorf_background.py` run.

    python tools/bench_tensorf_background.py [--steps 50] [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]


def _ms(fn, reps):
    for _ in range(3):  # (the second backward is the first to ACCUMULATE into .grad: its kernel loads lazily, outside the timing)
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _net(bg, res=300):
    from nerf import synthetic as syn
    from tensoRF.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(resolution=[res] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10,
                      **({"bg_radius": 32} if bg else {})).cuda()
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens).cuda())
    net.density_bitfield.copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


def bg_call(n, reps):
    import raymarching
    net = _net(True, res=32)  # (the background does not read the factors)
    g = torch.Generator().manual_seed(0)
    ro = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
    rd = torch.nn.functional.normalize(torch.rand(n, 3, generator=g) * 2 - 1, dim=-1).cuda()
    sph = raymarching.sph_from_ray(ro, rd, 32)
    grad = torch.rand(n, 3, generator=g).cuda()
    out = {}
    for fused in (True, False):
        net.fused_background = fused

        def step():
            with torch.autocast("cuda", dtype=torch.float16):
                rgb = net.background(sph, rd)
            rgb.float().backward(grad)

        def fwd():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                net.background(sph, rd)
        out["native" if fused else "torch"] = dict(fwd_ms=_ms(fwd, reps), fwd_bwd_ms=_ms(step, reps))
    net.fused_background = True
    return out


def train_steps(steps):
    from nerf import synthetic as syn
    from tensoRF.utils import GraphedTrainer
    poses = syn.orbit_poses(8, seed=0)
    batches = []
    for i in range(8):
        r = syn.get_rays(poses[i:i + 1], syn.lego_intrinsics(), 800, 800, N=4096, generator=torch.Generator().manual_seed(i))
        ro, rd = r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous()
        batches.append((ro, rd, torch.rand(4096, 3, generator=torch.Generator().manual_seed(100 + i)).cuda()))
    trs = {}
    for bg in (False, True):
        net = _net(bg)
        tr = GraphedTrainer(net, 4096, lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9)
        tr.global_step = 1
        net.mean_count = 4096 * 70
        for i in range(3):
            tr.train_step(*batches[i % 8])
        trs[bg] = tr
    torch.cuda.synchronize()
    tot = {False: 0.0, True: 0.0}
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in (False, True)}
    for i in range(steps):  # alternating, one step each
        for bg in (False, True):
            a, b = ev[bg]
            a.record()
            trs[bg].train_step(*batches[i % 8])
            b.record()
            torch.cuda.synchronize()
            tot[bg] += a.elapsed_time(b)
    return {"without_bg_ms": tot[False] / steps, "with_bg_ms": tot[True] / steps,
            "captures": {str(k): v.n_captures for k, v in trs.items()}}


def frame(reps):
    from nerf import synthetic as syn
    r = syn.get_rays(syn.orbit_poses(1, seed=3), syn.lego_intrinsics(), 800, 800)
    ro, rd = r["rays_o"].cuda().contiguous(), r["rays_d"].cuda().contiguous()
    out = {}
    for bg in (False, True):
        net = _net(bg).eval()

        def render():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                net.render(ro, rd, staged=False, perturb=False, max_steps=1024)
        out["with_bg_ms" if bg else "without_bg_ms"] = _ms(render, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"metric": "tensorf background model cost", "bg_call": {str(n): bg_call(n, a.reps) for n in (4096, 640000)},
           "train_step": train_steps(a.steps), "frame_800x800": frame(max(3, a.reps // 4))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
