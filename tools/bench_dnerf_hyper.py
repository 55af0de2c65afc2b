#!/usr/bin/env python3
"""Cost of the D-NeRF hyper backbone on one MI355X at its defaults (4-D tiled grid 16 x 2 at 2^19 rows, ambient MLP 5 x 128 on one row,
4,096 rays of the synthetic Lego-shaped scene at one time, fp16 autocast), under linear and under smoothstep interpolation; prints
one JSON line.  Everything is measured in ONE process, the variants alternating, device events around each call (the method of
tools/bench_dnerf_basis.py):

  * model: network forward and forward + backward on the marched samples of 4,096 rays, and the eager training step
    (dnerf.utils.Trainer) under a sample budget, on the fused route (csrc/dnerf_hyper.hip, the basis model's density-head kernel and
    the fused MLP entry points) against the model's own torch route (`fused_mlp = False`) — the baseline, since no earlier path exists;
  * kernels: the two kernels of csrc/dnerf_hyper.hip, and the generic route's forward (the cat and s3d_grid_encode_forward with
    D = 4 and dy_dx) for comparison, with the bytes per row each streams (the gathered table rows, 16 x 4 B per level and row and
    mostly cache hits, are not counted; at 8 TB/s: bytes / 8e6 = microseconds) and the fraction of 8 TB/s the measured time amounts
    to.  For kernel times proper run this part under a kernel trace: `rocprofv3 --kernel-trace --stats -- python
    tools/bench_dnerf_hyper.py --only kernels --reps 5` (kernels k_dnerf_hyper_grid, k_dnerf_hyper_backward, k_grid_forward).

    python tools/bench_dnerf_hyper.py [--steps 20] [--reps 10] [--only model|kernels]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd"), HERE]
from bench_dnerf import _alternate, _marched_samples  # noqa: E402

INNER = 20
INTERPOLATIONS = ("linear", "smoothstep")
# fp16 table, 16 levels: x 12 + feat 64 + x4 16 (+ dy_da 64); grad_feat 64 + grad_levels 64 (+ dy_da 64); the generic forward reads
# the [B, 4] row (16) and writes the level-major features (64) and dy_dx [B, 16, 4, 2] (256), behind a cat that writes those 16
BYTES_ROW = {"hyper_forward_linear": 12 + 64 + 16, "hyper_forward_smoothstep": 12 + 64 + 16 + 64,
             "hyper_backward_linear": 64 + 64, "hyper_backward_smoothstep": 64 + 64 + 64,
             "generic_forward_smoothstep": 12 + 16 + 16 + 64 + 256}


def _net(interpolation, time_size=2):
    from dnerf.network_hyper import NeRFNetwork
    from nerf import synthetic as syn
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, time_size=time_size,
                      interpolation=interpolation).cuda()
    _, bits = syn.lego_like_density_grid(seed=0)
    for t in range(time_size):
        net.density_bitfield[t].copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


def model(reps, n_steps, interpolation):
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    net = _net(interpolation).train()
    x, d = _marched_samples()
    m = x.shape[0]
    t = torch.tensor([[0.37]], device="cuda")
    g = torch.Generator().manual_seed(1)
    gs, gc = (torch.randn(m, generator=g) * 0.1).cuda(), (torch.randn(m, 3, generator=g) * 0.1).cuda()

    def fwd(fused):
        def run():
            net.fused_mlp = fused
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                net(x, d, t)
        return run

    def fwd_bwd(fused):
        def run():
            net.fused_mlp = fused
            net.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                s, c, _ = net(x, d, t)
            ((s.float() * gs).sum() + (c.float() * gc).sum()).backward()
        return run
    out = {"points": m}
    out["network_ms"] = _alternate({"fused_fwd": fwd(True), "torch_fwd": fwd(False), "fused_fwd_bwd": fwd_bwd(True),
                                    "torch_fwd_bwd": fwd_bwd(False)}, reps)
    del net
    poses = syn.orbit_poses(8, seed=0)
    batches = []
    for i in range(8):
        r = syn.get_rays(poses[i:i + 1], syn.lego_intrinsics(), 800, 800, N=4096, generator=torch.Generator().manual_seed(i))
        batches.append((r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous(),
                        torch.rand(4096, 3, generator=torch.Generator().manual_seed(100 + i)).cuda(), (i + 0.5) / 8))
    trs = {}
    for tag in ("fused", "torch"):
        n = _net(interpolation)
        n.fused_mlp = tag == "fused"
        tr = Trainer(n, fp16=True, update_extra_interval=10 ** 9)
        tr.global_step = 1
        n.mean_count = 4096 * 32  # (steady state: a sample budget, the marcher's padded buffers and the count's read-back)
        trs[tag] = tr
    out["eager_step_ms"] = _alternate({tag: (lambda tr=tr, c=[0]: (tr.train_step(*batches[c[0] % 8]), c.__setitem__(0, c[0] + 1)))
                                       for tag, tr in trs.items()}, n_steps, warm=3)
    out["samples_last_step"] = {k: int(v.model.step_counter[:, 0].max()) for k, v in trs.items()}
    return out


def kernels(reps):
    import s3d_hip
    K, G = s3d_hip.DnerfHyperBackend, s3d_hip.GridBackend
    x, _ = _marched_samples()
    B = x.shape[0]
    ambient = torch.tensor([0.3], device="cuda")
    g = torch.Generator().manual_seed(2)
    g_feat = (torch.randn(B, 32, generator=g) * 0.1).half().cuda()
    calls = {}
    for interpolation in INTERPOLATIONS:
        enc = _net(interpolation).encoder
        table = enc.embeddings.detach().half().contiguous()
        S, H = float(np.log2(enc.per_level_scale)), enc.base_resolution
        geo = (enc.gridtype_id, enc.align_corners, enc.interp_id)
        feat = torch.empty(B, 32, dtype=torch.float16, device="cuda")
        x4 = torch.empty(B, 4, device="cuda")
        smooth = interpolation == "smoothstep"
        dy_da = torch.empty(B, 16, 2, dtype=torch.float16, device="cuda") if smooth else None
        levels = torch.empty(16, B, 2, dtype=torch.float16, device="cuda")
        g_amb = torch.empty(1, device="cuda") if smooth else None
        K.grid_forward(x, ambient, table, enc.offsets, S, H, *geo, 1.0, feat, x4, dy_da)
        calls[f"hyper_forward_{interpolation}"] = (lambda table=table, enc=enc, S=S, H=H, geo=geo, feat=feat, x4=x4, dy_da=dy_da:
                                                   K.grid_forward(x, ambient, table, enc.offsets, S, H, *geo, 1.0, feat, x4, dy_da))
        calls[f"hyper_backward_{interpolation}"] = (lambda dy_da=dy_da, levels=levels, g_amb=g_amb:
                                                    K.grid_backward(g_feat, dy_da, 0.5, levels, g_amb))
        if smooth:
            out = torch.empty(16, B, 2, dtype=torch.float16, device="cuda")
            dy_dx = torch.empty(B, 16 * 8, dtype=torch.float16, device="cuda")

            def generic(table=table, enc=enc, S=S, H=H, geo=geo, out=out, dy_dx=dy_dx):
                x01 = (torch.cat([x, ambient.reshape(1, 1).repeat(B, 1)], dim=1) + 1.0) * 0.5
                G.grid_encode_forward(x01, table, enc.offsets, out, B, 4, 2, 16, S, H, dy_dx, *geo)
            calls["generic_forward_smoothstep"] = generic
    # (calls of a few microseconds: INNER calls back to back between the two events, so that the launch gap of a single call is not
    #  what is timed)
    ms = _alternate({k: (lambda fn=fn: [fn() for _ in range(INNER)]) for k, fn in calls.items()}, reps)
    ms = {k: v / INNER for k, v in ms.items()}
    return {"rows": B, "calls_per_timing": INNER, "ms": ms, "bytes_per_row": BYTES_ROW, "us_at_8TBps": {k: v * B / 8e6 for k, v in BYTES_ROW.items()},
            "fraction_of_8TBps": {k: v * B / 8e6 / (ms[k] * 1e3) for k, v in BYTES_ROW.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["model", "kernels"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dnerf_hyper: needs a GPU (no CPU timing is meaningful here)")
    res = {"metric": "dnerf hyper backbone cost", "reps": a.reps, "steps": a.steps}
    if a.only in (None, "kernels"):
        res["kernels"] = kernels(a.reps)
    if a.only in (None, "model"):
        res["model"] = {interpolation: model(a.reps, a.steps, interpolation) for interpolation in INTERPOLATIONS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
