#!/usr/bin/env python3
"""Time the brush tool's texture painting on the GPU and print one JSON object (timing scheme of tools/bench_seal_tools.py:
median of whole calls between two stream events).

  map_color_masked  a textured brush (`hsv` + `imageConfig`), native (s3d_seal_map_color_image) vs the torch op sequence
                    (native=False), at 200,000 / 2^18 / 2^20 samples with the brush's own mask share (the mask of
                    map_to_origin on points half of which lie around the edit), textures of 64^2, 512^2 and 2048^2 texels
                    (16 B each on the device: 64 KB, 4 MB, 64 MB).  Yardstick in the same run: the two-pass `hsv` + `rgb`
                    edit (s3d_seal_map_color) on the same colours and mask.
  fine-tuning       a replayed GraphedSealTrainer step (lego-like occupancy, 4096 rays) with the same dry brush, `hsv` only vs
                    `hsv` + a 512^2 texture.

Every figure is taken `--rounds` times, the variants alternating inside a round; the JSON holds each round's median, so the
run-to-run spread can be read next to the differences.

    python tools/bench_seal_texture.py [--reps 50] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "seal-3d_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_seal_tools import BRUSH, points, timed  # noqa: E402

HSV = [0.1, 0.0, -0.05]
# the image quad lies along the stroke (y = 0.3 + 0.08 x over x in [-0.25, 0.25], z around 0.05) and covers most of it
QUAD = dict(o=[-0.2, 0.284, -0.1], w=[0.2, 0.316, -0.1], h=[-0.2, 0.284, 0.2])


def texels(side, seed=0):
    """seeded float32 RGBA texels [side, side, 4] (inline `pixels`)"""
    g = torch.Generator().manual_seed(seed + side)
    return torch.rand(side, side, 4, generator=g).numpy()


def textured(side, mode="linear", native=True):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(dict(BRUSH, attenuationMode=mode, hsv=HSV, imageConfig=dict(QUAD, pixels=texels(side))))
    m.native = native
    return m


def color_times(n, sides, reps, rounds):
    from sealnerf import get_seal_mapper
    plain = get_seal_mapper(dict(BRUSH, hsv=HSV, rgb=[0.8, 0.2, 0.1]))
    p = points(plain, n)
    mapped, _, mask = plain.map_to_origin(p)
    cols = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).cuda()
    out = {"masked": int(mask.sum()), "rgb_two_pass_us": []}
    fns = {"rgb_two_pass_us": lambda: plain.map_color_masked(mapped, None, cols, mask)}
    for side in sides:
        for native in (True, False):
            m = textured(side, native=native)
            key = f"tex{side}_{'native' if native else 'torch'}_us"
            out[key] = []
            fns[key] = (lambda m=m: m.map_color_masked(mapped, None, cols, mask))
    for _ in range(rounds):
        for key, fn in fns.items():
            out[key].append(timed(fn, max(5, reps // 5) if key.endswith("torch_us") else reps))
    # the two routes agree (fp32): a figure for a wrong result is worth nothing
    for side in sides:
        a = fns[f"tex{side}_native_us"]()
        b = fns[f"tex{side}_torch_us"]()
        out[f"tex{side}_max_abs_diff"] = float((a - b).abs().max())
    return out


def trainer(cfg):
    from nerf import network, synthetic as syn
    from sealnerf import GraphedSealTrainer, get_seal_mapper, make_student, make_teacher
    torch.manual_seed(0)
    kw = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
    teacher = make_teacher(network.NeRFNetwork, **kw).cuda()
    student = make_student(network.NeRFNetwork, **kw).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    for net in (teacher, student):
        net.density_grid.copy_(torch.from_numpy(grid))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.iter_density = 100
    student.load_state_dict(teacher.state_dict())
    m = get_seal_mapper(cfg)
    teacher.init_mapper(m)
    student.init_mapper(m)
    return GraphedSealTrainer(student, teacher, 4096, lr=1e-2, fp16=True, update_extra_interval=16)


def step_times(reps, rounds, side=512):
    from nerf import synthetic as syn
    dry = dict(BRUSH, attenuationMode="dry", hsv=HSV)
    trainers = {"hsv": trainer(dry), "hsv_texture": trainer(dict(dry, imageConfig=dict(QUAD, pixels=texels(side))))}
    r = syn.get_rays(syn.orbit_poses(1, seed=0).cuda(), syn.lego_intrinsics(), 800, 800, N=4096,
                     generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    for tr in trainers.values():
        for _ in range(24):
            tr.train_step(ro, rd)
    out = {k: {"ms_per_step": []} for k in trainers}
    for _ in range(rounds):
        for k, tr in trainers.items():
            out[k]["ms_per_step"].append(timed(lambda: tr.train_step(ro, rd), reps) / 1e3)
    for k, tr in trainers.items():
        out[k]["n_captures"] = int(tr.n_captures)
        out[k]["proxy_graph"] = tr.proxy_graph is not None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[200000, 1 << 18, 1 << 20])
    ap.add_argument("--textures", type=int, nargs="*", default=[64, 512, 2048])
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seal_texture: no GPU (the figures are device times; there is no CPU stand-in)")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "map_color_masked": {},
           "fine_tuning_step": {}}
    for n in args.sizes:
        res["map_color_masked"][str(n)] = color_times(n, args.textures, args.reps, args.rounds)
    if not args.no_step:
        res["fine_tuning_step"] = step_times(args.reps, args.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
