#!/usr/bin/env python3
"""Cost of training on RGBA frames with the per-pixel random background on one MI355X; prints one JSON line.

  * the graph-replayed 4,096-ray NGP step on an 800 x 800 two-image RGBA dataset (fp16 frames; batch, targets and background
    drawn by sample(out=static_batch())) against the same trainer on the pre-blended RGB frames with bg_color=1, the two
    stepped alternately in one process;
  * the sampler launch with RGB / RGBA frames, fp32 / fp16, uniform and error-map mode;
  * s3d_rgba_targets at 4,096 and 2^20 rows against the torch op sequence it replaces.

Kernel times and launch counts come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_rgba_background.py`
run; run the script twice to see the spread.

    python tools/bench_rgba_background.py [--steps 50] [--reps 50]
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
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _frames():
    g = torch.Generator().manual_seed(0)
    img = torch.rand(2, 800, 800, 4, generator=g)
    img[..., 3] = (img[..., 3] * 1.5 - 0.25).clamp(0, 1)  # (alphas with exact 0 and 1, as rendered frames have)
    return img


def _dataset(images, error_map, fp16):
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    return NeRFDataset(images, syn.orbit_poses(2, seed=0), syn.lego_intrinsics(), num_rays=4096, error_map=error_map, device="cuda",
                       fp16=fp16)


def _net():
    from nerf import synthetic as syn
    from nerf.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens).cuda())
    net.density_bitfield.copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from nerf.trainer import GraphedTrainer, rgba_targets
    res = {"metric": "rgba_background", "n_rays": 4096}
    rgba = _frames()
    rgb = rgba[..., :3] * rgba[..., 3:] + (1 - rgba[..., 3:])  # pre-blended on white: what the README's numbers train on
    # the sampler launch
    for mode, emap in (("uniform", False), ("map", True)):
        for name, frames in (("rgb", rgb), ("rgba", rgba)):
            for fp16 in (False, True):
                ds = _dataset(frames, emap, fp16)
                res[f"sampler_ms_{mode}_{name}_{'fp16' if fp16 else 'fp32'}"] = _ms(lambda: ds.sample([1]), a.reps)
    # the stand-alone target kernel against torch's op sequence
    ctl = torch.zeros(2, dtype=torch.int32, device="cuda")
    for rows in (4096, 1 << 20):
        px = torch.rand(rows, 4, device="cuda")
        res[f"targets_ms_{rows}"] = _ms(lambda: rgba_targets(px, seed=1, ctl=ctl), a.reps)
        res[f"targets_torch_ms_{rows}"] = _ms(lambda: rgba_targets(px), a.reps)
    # graph-replayed step, RGBA frames with the random background against pre-blended RGB frames, alternately
    data = {"rgb": _dataset(rgb, False, True), "rgba": _dataset(rgba, False, True)}
    trs = {}
    for name in data:
        net = _net()
        tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
        tr.global_step = 1
        net.mean_count = 4096 * 40
        trs[name] = tr

    def step(name, k):
        tr = trs[name]
        bb = data[name].sample([k % 2], out=tr.static_batch())
        tr.train_step(bb["rays_o"][0], bb["rays_d"][0], bb["images"][0], bg_color=bb["bg_color"][0] if "bg_color" in bb else 1)

    for k in range(5):
        for name in data:
            step(name, k)
    torch.cuda.synchronize()
    tot = dict.fromkeys(data, 0.0)
    for k in range(a.steps):
        for name in (("rgb", "rgba") if k % 2 == 0 else ("rgba", "rgb")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(name, k)
            e1.record()
            torch.cuda.synchronize()
            tot[name] += e0.elapsed_time(e1)
    res["step_ms_rgb"] = tot["rgb"] / a.steps
    res["step_ms_rgba"] = tot["rgba"] / a.steps
    res["captures"] = {k: v.n_captures for k, v in trs.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
