#!/usr/bin/env python3
"""Cost of an interactive preview frame's tail on one MI355X, native route next to the torch route in the same run; prints one
JSON line.

Frame sizes 800 x 800 and 1920 x 1080, each rendered at downscale 1 and 0.5.  Per size:

  * the frame rays: one s3d_frame_rays launch next to nerf.synthetic.get_rays (torch on the GPU);
  * the resolve: one s3d_preview_resolve launch next to resolve_torch + prepare_torch + accumulate_torch on the same inputs,
    plain (image mode, no mask, the first frame) and loaded (three masks at alpha 0.35, accumulation onto 5 frames), with the bytes
    the launch moves per destination pixel and the fraction of 8 TB/s that makes;
  * mask positions at about 5 % coverage: s3d_mask_positions_* next to boolean indexing (both read their counts on the host);
  * a whole Trainer.test_gui call on a small NGP model, either route, to set the tail against the render beside it;
  * a PreviewSession.step() loop with dynamic resolution on (64 steps: the accumulation fills), ms per step and the downscale it
    settles at.

Wall time per call: device events around `reps` calls with a synchronise at the end, the two routes alternated over `rounds`
rounds; median and min - max of the rounds.  Kernels per call: counted by torch.profiler in a pass of its own.

    python tools/bench_preview.py [--reps 50] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]

SIZES = ((800, 800), (1080, 1920))
HBM_BYTES_PER_S = 8e12


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
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def _compare(routes, reps, rounds):
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(_ms(fn, reps))
    return {k: dict(_spread(v), kernels=_kernels(routes[k])) for k, v in times.items()}


def _model():
    from nerf import network, synthetic as syn
    net = network.NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, log2_hashmap_size=14).cuda()
    for k, p in net.named_parameters():
        p.data.copy_((torch.rand(p.shape, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()) % 1000)) - 0.5).to(p.device))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import s3d_hip
    from nerf import synthetic as syn
    from nerf.preview import PreviewSession, accumulate_torch, mask_positions, prepare_torch, resolve_torch
    from nerf.trainer import Trainer
    s3d_hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "sizes": {}}
    pose = syn.orbit_poses(1, seed=0)[0].numpy()
    tr = Trainer(_model(), fp16=True)
    color = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    for H, W in SIZES:
        for ds in (1, 0.5):
            rH, rW = int(H * ds), int(W * ds)
            intr = syn.lego_intrinsics(H, W)
            entry = {}
            # frame rays
            ro, rd = torch.empty(rH * rW, 3, device="cuda"), torch.empty(rH * rW, 3, device="cuda")
            flat = pose.reshape(-1).tolist()
            pose_d = torch.from_numpy(pose)[None].cuda()
            entry["frame_rays"] = _compare({
                "native": lambda: s3d_hip.RaySampleBackend.frame_rays(flat, intr * ds, rH, rW, ro, rd),
                "torch": lambda: syn.get_rays(pose_d, intr * ds, rH, rW, -1)}, args.reps, args.rounds)
            # resolve
            g = torch.Generator().manual_seed(1)
            image, depth = torch.rand(rH, rW, 3, generator=g).cuda(), (torch.rand(rH, rW, generator=g) * 4).cuda()
            masks = (torch.rand(3, H, W, generator=g) < 0.05).to(torch.uint8).cuda()
            buf = torch.rand(H, W, 3, generator=g).cuda()
            for name, K, alpha, spp in (("plain", 0, 1.0, 0), ("loaded", 3, 0.35, 5)):
                m = masks[:K].contiguous()

                def native():
                    s3d_hip.PreviewBackend.resolve(image, depth, H, W, False, buffer=buf, mode="image", masks=m, color=color, alpha=alpha, spp=spp)

                def torch_route():
                    fi, fd, _ = resolve_torch(image, depth, H, W)
                    buf.copy_(accumulate_torch(buf, prepare_torch(fi, fd, "image", m, color, alpha), spp))
                r = _compare({"native": native, "torch": torch_route}, args.reps, args.rounds)
                # bytes per destination pixel: frame image 12 + depth 4 + buffer 12 written, the buffer's 12 read when accumulating,
                # one byte per mask; the source gather (16 bytes per SOURCE pixel) comes from cache
                # (at downscale 1 the frame image is the renderer's own: not written)
                per_pixel = (16 if ds == 1 else 28) + (12 if spp else 0) + K
                r["bytes_per_pixel"] = per_pixel
                r["native_fraction_of_8TBps"] = per_pixel * H * W / (r["native"]["median"] * 1e-3) / HBM_BYTES_PER_S
                entry[f"resolve_{name}"] = r
            # mask positions
            pos = torch.rand(H, W, 3, generator=g).cuda()
            entry["mask_positions_5pct_k3"] = _compare({
                "native": lambda: mask_positions(pos, masks, True),
                "torch": lambda: mask_positions(pos, masks, False)}, max(args.reps // 5, 5), args.rounds)
            # the whole call
            entry["test_gui"] = _compare({
                "native": lambda: tr.test_gui(pose, intr, W, H, downscale=ds),
                "torch": lambda: tr.test_gui(pose, intr, W, H, downscale=ds, native=False)}, max(args.reps // 5, 5), args.rounds)
            res["sizes"][f"{W}x{H}@{ds}"] = entry
        # a session with dynamic resolution
        for native in (True, False):
            s = PreviewSession(tr, W, H, max_spp=64, native=native)
            s.cam = types.SimpleNamespace(pose=pose, intrinsics=syn.lego_intrinsics(H, W))
            s.step()
            loops = []
            for _ in range(args.rounds):
                s.need_update = True
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                n = 0
                while s.step():
                    n += 1
                b.record()
                torch.cuda.synchronize()
                loops.append(a.elapsed_time(b) / n)
            res["sizes"].setdefault(f"{W}x{H}_session", {})["native" if native else "torch"] = dict(_spread(loops), steps=n, downscale=s.downscale)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
