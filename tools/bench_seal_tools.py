#!/usr/bin/env python3
"""Time the Seal proxy mappers on the GPU and print one JSON object.

  map_to_origin   native kernel vs the torch op sequence (native=False) at 2^18 and 2^20 points (half of them around the
                  edit): brush with B in {64, 1024, 8192} border points (set directly, in the stroke plane), anchor, and the
                  bbox tool for comparison; plus the teacher's batch size (2e5 samples)
  fine-tuning     a replayed GraphedSealTrainer step (lego-like occupancy, 4096 rays) with a bbox, a brush and an anchor edit

    python tools/bench_seal_tools.py [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "seal-3d_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BBOX = {"type": "bbox", "raw": [[x, y, z] for x in (-0.2, 0.2) for y in (0.0, 0.3) for z in (-0.2, 0.2)],
        "transform": [[1, 0, 0, 0.3], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], "scale": [1, 1, 1], "boundType": "both"}


def _stroke():
    x = np.linspace(-0.25, 0.25, 24)
    return np.stack([x, 0.3 + 0.08 * x, 0.05 + 0.08 * np.sin(9 * x)], 1).round(4).tolist()


BRUSH = dict(type="brush", raw=_stroke(), normal=[0, 1, 0], brushType="line", brushDepth=1.0, brushPressure=0.05,
             attenuationDistance=0.08, attenuationMode="linear")
ANCHOR = dict(type="anchor", raw=[[0.15 + 0.07 * np.cos(a), 0.1 + 0.03 * np.cos(a), -0.1 + 0.07 * np.sin(a)]
                                  for a in np.linspace(0, 2 * np.pi, 8, endpoint=False)],
              translation=[0.04, 0.12, -0.03], radius=0.1, scale=[1, 1, 1])


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return float(np.median(t))


def points(m, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    b = m.map_data["map_bound"].reshape(-1, 2, 3).cpu()
    lo, hi = b[:, 0].min(0).values - 0.03, b[:, 1].max(0).values + 0.03
    p[n // 2:] = lo + (hi - lo) * torch.rand(n - n // 2, 3, generator=g)
    return p.cuda()


def with_border(m, B):
    g = torch.Generator().manual_seed(B)
    ne, c = m.map_data["normal_expand"].cpu(), m.map_data["center"].cpu()
    q = c + (torch.rand(B, 3, generator=g) - 0.5) * 0.6
    m.map_data["border_points"] = (q - ((q - c) @ ne / (ne @ ne))[:, None] * ne).to(m.map_data["normal_expand"].device)
    m._dev.clear()
    return m


def map_times(cfg, n, reps, border=None):
    from sealnerf import get_seal_mapper
    out = {}
    for native in (True, False):
        m = get_seal_mapper(cfg)
        if border is not None:
            with_border(m, border)
        m.native = native
        p = points(m, n)
        out["native_us" if native else "torch_us"] = timed(lambda: m.map_to_origin(p), reps if native else max(5, reps // 5))
        if native:
            out["mapped"] = int(m.map_to_origin(p)[2].sum())
    return out


def step_time(cfg, reps):
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
    tr = GraphedSealTrainer(student, teacher, 4096, lr=1e-2, fp16=True, update_extra_interval=16)
    r = syn.get_rays(syn.orbit_poses(1, seed=0).cuda(), syn.lego_intrinsics(), 800, 800, N=4096,
                     generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    for _ in range(24):
        tr.train_step(ro, rd)
    ms = timed(lambda: tr.train_step(ro, rd), reps) / 1e3
    return {"ms_per_step": ms, "n_captures": int(tr.n_captures)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "map_to_origin": {}, "fine_tuning_step": {}}
    mt = res["map_to_origin"]
    for n in (200000, 1 << 18, 1 << 20):
        mt[f"bbox_{n}"] = map_times(BBOX, n, args.reps)
        for B in (64, 1024, 8192):
            mt[f"brush_B{B}_{n}"] = map_times(BRUSH, n, args.reps, border=B)
        mt[f"anchor_{n}"] = map_times(ANCHOR, n, args.reps)
    for name, cfg in (("bbox", BBOX), ("brush", BRUSH), ("anchor", ANCHOR)):
        res["fine_tuning_step"][name] = step_time(cfg, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
