#!/usr/bin/env python3
"""Cost of Seal-3D's custom-pose batches (`--custom_pose`) on one MI355X; prints one JSON line.

  * the sampler launch (s3d_orbit_rays through SealRandomDataset.sample into preallocated buffers) next to the torch GPU op
    sequence it replaces (SealRandomDataset.collate: rand_poses + get_rays), at the 64 x 64 training frame (800 x 800,
    num_rays 4,096) and at the 800 x 800 validation frame: wall time per call (device events around `reps` calls, a
    synchronise at the end), the two alternated over `rounds` rounds, and the number of kernels each issues per call (counted
    by torch.profiler in a pass of its own, outside the timed windows);
  * the graph-replayed custom-pose step (GraphedSealTrainer.train_step_random: sampler launch into s_ro / s_rd, proxy replay,
    student replay) next to the same trainer fed by collate (train_step(rays_o, rays_d): the torch sequence, a staging copy,
    the same two replays), two identically prepared trainers stepped alternately in one process.

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_custom_pose.py --no-step` run.

    python tools/bench_custom_pose.py [--reps 50] [--rounds 5] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]

BBOX = {"type": "bbox", "raw": [[x, y, z] for x in (-0.2, 0.2) for y in (0.0, 0.3) for z in (-0.2, 0.2)],
        "transform": [[1, 0, 0, 0.3], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], "scale": [1, 1, 1], "boundType": "both"}


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


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": len(v)}


def _kernels(fn):
    """kernels issued by one call of fn, or None where the profiler reports no device activity"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def _dataset(mapper, training):
    from nerf import synthetic as syn
    from sealnerf import SealRandomDataset
    return SealRandomDataset(mapper, syn.lego_intrinsics(), 800, 800, num_rays=4096, device="cuda", training=training)


def sampler_times(mapper, reps, rounds):
    out = {}
    for name, training in (("64x64", True), ("800x800", False)):
        ds = _dataset(mapper, training)
        n = ds.rays_per_batch
        buf = {"rays_o": torch.empty(1, n, 3, device="cuda"), "rays_d": torch.empty(1, n, 3, device="cuda"),
               "poses": torch.empty(1, 4, 4, device="cuda")}
        routes = {"sample": lambda: ds.sample([0], out=buf), "collate": lambda: ds.collate([0])}
        times = {k: [] for k in routes}
        for r in range(rounds):
            for k in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
                times[k].append(_ms(routes[k], reps))
        out[name] = {"rays": n, "bytes_written": 24 * n}
        for k in routes:
            out[name][f"{k}_ms"] = _spread(times[k])
            out[name][f"{k}_kernels"] = _kernels(routes[k])
    return out


def _trainer(mapper):
    from nerf import network, synthetic as syn
    from sealnerf import GraphedSealTrainer, make_student, make_teacher
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
    teacher.init_mapper(mapper)
    student.init_mapper(mapper)
    teacher.train()  # (the one-march proxy branch, replayed from its graph)
    return GraphedSealTrainer(student, teacher, 4096, lr=1e-2, fp16=True, update_extra_interval=16)


def step_times(reps, rounds):
    from sealnerf import get_seal_mapper
    trs, dss = {}, {}
    for k in ("random", "collate"):
        m = get_seal_mapper(BBOX)
        trs[k], dss[k] = _trainer(m), _dataset(m, True)

    def step(k):
        if k == "random":
            trs[k].train_step_random(dss[k])
        else:
            b = dss[k].collate([0])
            trs[k].train_step(b["rays_o"], b["rays_d"])
    for k in trs:
        for _ in range(24):  # 16 eager steps (sample statistics), the capture, replays
            step(k)
    times = {k: [] for k in trs}
    for r in range(rounds):
        for k in (list(trs) if r % 2 == 0 else list(trs)[::-1]):
            times[k].append(_ms(lambda: step(k), reps))
    out = {k: {"ms_per_step": _spread(times[k]), "n_captures": int(trs[k].n_captures), "proxy_graph": trs[k].proxy_graph is not None}
           for k in trs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_custom_pose: no GPU (the figures are device times; there is no CPU stand-in)")
    from sealnerf import get_seal_mapper
    res = {"metric": "custom_pose", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds}
    res["sampler"] = sampler_times(get_seal_mapper(BBOX), a.reps, a.rounds)
    if not a.no_step:
        res["fine_tuning_step"] = step_times(a.reps, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
