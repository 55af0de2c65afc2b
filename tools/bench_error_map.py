#!/usr/bin/env python3
"""Cost of error-map importance sampling on one MI355X; prints one JSON line.

  * the sampler launch (s3d_sample_train_rays) at N = 4,096 on one 800 x 800 image, next to the torch GPU op sequence it
    replaces (multinomial, rand, ray math and the target gather of get_rays + collate);
  * the update launch (s3d_error_map_update) for 4,096 rays;
  * the graph-replayed 4,096-ray NGP step with and without the map, the two trainers stepped alternately in one process (the
    map's batches drawn by the sampler into the step's static buffers; the plain trainer's staged as before).

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_error_map.py` run.

    python tools/bench_error_map.py [--steps 50] [--reps 50]
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


def _dataset(error_map):
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    g = torch.Generator().manual_seed(0)
    imgs = torch.rand(2, 800, 800, 3, generator=g)
    return NeRFDataset(imgs, syn.orbit_poses(2, seed=0), syn.lego_intrinsics(), num_rays=4096, error_map=error_map, device="cuda")


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
    import s3d_hip
    from nerf.trainer import GraphedTrainer
    res = {"metric": "error_map", "n_rays": 4096}
    ds = _dataset(True)
    ds.error_map.copy_(torch.rand(2, 128 * 128, generator=torch.Generator().manual_seed(1)).cuda() + 0.01)
    out = {"rays_o": torch.empty(1, 4096, 3, device="cuda"), "rays_d": torch.empty(1, 4096, 3, device="cuda"),
           "images": torch.empty(1, 4096, 3, device="cuda"), "inds": torch.empty(1, 4096, dtype=torch.int64, device="cuda"),
           "inds_coarse": torch.empty(1, 4096, dtype=torch.int64, device="cuda")}
    res["sampler_ms"] = _ms(lambda: ds.sample([1], out=out), a.reps)
    res["torch_collate_ms"] = _ms(lambda: ds.collate([1]), a.reps)
    b = ds.sample([1])
    image, gt = torch.rand(4096, 3, device="cuda"), torch.rand(4096, 3, device="cuda")
    ws = torch.rand(4096, device="cuda")
    res["update_ms"] = _ms(lambda: s3d_hip.RaySampleBackend.error_map_update(ds.error_map, b["index"], b["inds_coarse"], image, gt, ws,
                                                                               (1.0, 1.0, 1.0)), a.reps)
    # graph-replayed step with and without the map, alternately
    plain = _dataset(False)
    trs = {}
    for name in ("plain", "map"):
        net = _net()
        tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
        tr.global_step = 1
        net.mean_count = 4096 * 40
        if name == "map":
            tr.error_map = ds.error_map
        trs[name] = tr

    def step(name, k):
        tr = trs[name]
        if name == "map":
            bb = ds.sample([k % 2], out=tr.static_batch())
            tr.train_step(bb["rays_o"][0], bb["rays_d"][0], bb["images"][0], index=bb["index"], inds_coarse=bb["inds_coarse"])
        else:
            bb = plain.sample([k % 2])
            tr.train_step(bb["rays_o"][0], bb["rays_d"][0], bb["images"][0])

    for k in range(5):
        step("plain", k)
        step("map", k)
    torch.cuda.synchronize()
    tot = {"plain": 0.0, "map": 0.0}
    for k in range(a.steps):
        for name in (("plain", "map") if k % 2 == 0 else ("map", "plain")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(name, k)
            e1.record()
            torch.cuda.synchronize()
            tot[name] += e0.elapsed_time(e1)
    res["step_ms_plain"] = tot["plain"] / a.steps
    res["step_ms_map"] = tot["map"] / a.steps
    res["captures"] = {k: v.n_captures for k, v in trs.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
