#!/usr/bin/env python3
"""Cost of the D-NeRF backbone on one MI355X at its defaults (tiled grid 16 x 2 at 2^19 rows, deformation MLP 5 x 128, 4,096 rays of
the synthetic Lego-shaped scene at one time, fp16 autocast); prints one JSON line.  Everything is measured in ONE process, the
variants alternating, device events around each call (the method of tools/bench_ccnerf.py):

  * model: network forward and forward + backward on the marched samples of 4,096 rays, and the eager training step
    (dnerf.utils.Trainer) under a sample budget (mean_count > 0, as after the first occupancy update), on the fused route
    (csrc/dnerf.hip + the fused MLP entry points) against the model's own torch route (`fused_mlp = False`) — the baseline,
    since no earlier D-NeRF path exists;
  * kernels: each of the four glue kernels against the torch ops it replaces, with its algorithmic byte count (at 8 TB/s:
    bytes / 8e6 = microseconds).

    python tools/bench_dnerf.py [--steps 20] [--reps 10] [--only model|kernels]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd")]


def _net(time_size=2):
    from dnerf.network import NeRFNetwork
    from nerf import synthetic as syn
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, time_size=time_size).cuda()
    with torch.no_grad():
        for l in net.deform_net:
            l.weight.mul_(0.5)  # (a small warp: the samples stay inside the box)
    _, bits = syn.lego_like_density_grid(seed=0)
    for t in range(time_size):
        net.density_bitfield[t].copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


def _marched_samples(n_rays=4096):
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


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _alternate(variants, reps, warm=2):
    """{name: fn} -> {name: mean ms}, one call of each per round"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    tot = {k: 0.0 for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = _events()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            tot[k] += a.elapsed_time(b)
    return {k: v / reps for k, v in tot.items()}


def model(reps, n_steps):
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    net = _net().train()
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
                s, c, df = net(x, d, t)
                reg = net._deform_reg[0] / (3 * m) if net._deform_reg is not None else df.float().abs().mean()
            ((s.float() * gs).sum() + (c.float() * gc).sum() + reg).backward()
        return run
    out = {"points": m}
    res = _alternate({"fused_fwd": fwd(True), "torch_fwd": fwd(False), "fused_fwd_bwd": fwd_bwd(True), "torch_fwd_bwd": fwd_bwd(False)}, reps)
    out["network_ms"] = res
    poses = syn.orbit_poses(8, seed=0)
    batches = []
    for i in range(8):
        r = syn.get_rays(poses[i:i + 1], syn.lego_intrinsics(), 800, 800, N=4096, generator=torch.Generator().manual_seed(i))
        batches.append((r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous(),
                        torch.rand(4096, 3, generator=torch.Generator().manual_seed(100 + i)).cuda(), (i + 0.5) / 8))
    trs = {}
    for tag in ("fused", "torch"):
        n = _net()
        n.fused_mlp = tag == "fused"
        tr = Trainer(n, fp16=True, update_extra_interval=10 ** 9)
        tr.global_step = 1
        n.mean_count = 4096 * 32  # (steady state: a sample budget, the marcher's padded buffers and the count's read-back)
        trs[tag] = tr
    step = _alternate({tag: (lambda tr=tr, c=[0]: (tr.train_step(*batches[c[0] % 8]), c.__setitem__(0, c[0] + 1))) for tag, tr in trs.items()},
                      n_steps, warm=3)
    out["eager_step_ms"] = step
    out["samples_last_step"] = {k: int(v.model.step_counter[:, 0].max()) for k, v in trs.items()}
    return out


def kernels(reps):
    import s3d_hip
    from gridencoder import GridEncoder
    D = s3d_hip.DnerfBackend
    net = _net()
    enc = net.encoder.eval()
    x, _ = _marched_samples()
    B, L = x.shape[0], enc.num_levels
    t = torch.tensor([0.37], device="cuda")
    table = enc.embeddings.detach().half().contiguous()
    S, H = float(np.log2(enc.per_level_scale)), enc.base_resolution
    din = torch.empty(B, 80, dtype=torch.float16, device="cuda")
    sin = torch.empty(B, 112, dtype=torch.float16, device="cuda")
    dout = (torch.randn(B, 16, device="cuda") * 0.01).half()
    xw, deform = torch.empty(B, 3, device="cuda"), torch.empty(B, 3, device="cuda")
    dy_dx = torch.empty(B, L * 6, dtype=torch.float16, device="cuda")
    reg = torch.zeros((), device="cuda")
    g_sin = torch.randn(B, 112, device="cuda").half()
    g_lv = torch.empty(L, B, 2, dtype=torch.float16, device="cuda")
    g_xw = torch.randn(B, 3, device="cuda").half()
    g_dout = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    coef = torch.tensor([0.5], device="cuda")
    tt = t.reshape(1, 1)

    def torch_encode():
        with torch.autocast("cuda", dtype=torch.float16):
            ex, et = net.encoder_deform(x), net.encoder_time(tt).repeat(B, 1)
            return torch.cat([ex, et], dim=1).half()

    def torch_warp_grid():
        with torch.autocast("cuda", dtype=torch.float16):
            d3 = dout[:, :3]
            xq = (x + d3).requires_grad_(True)
            return torch.cat([enc(xq, bound=1), din[:, :76]], dim=1), d3.float().abs().sum()

    def torch_split():
        return g_sin[:, :32].reshape(B, L, 2).permute(1, 0, 2).contiguous()

    def torch_warp_bwd():
        return torch.nn.functional.pad((coef * torch.sign(deform) + g_xw.float() * 0.5).half(), (0, 13))
    D.warp_grid_forward(x, dout, table, enc.offsets, S, H, enc.gridtype_id, False, 0, 1.0, sin, xw, deform, dy_dx, reg)
    ms = _alternate({
        "encode": lambda: D.encode_forward(x, t, din, sin),
        "encode_torch": torch_encode,
        "warp_grid": lambda: D.warp_grid_forward(x, dout, table, enc.offsets, S, H, enc.gridtype_id, False, 0, 1.0, sin, xw, deform, dy_dx, reg),
        "warp_grid_no_jacobian": lambda: D.warp_grid_forward(x, dout, table, enc.offsets, S, H, enc.gridtype_id, False, 0, 1.0, sin, xw, deform, None, None),
        "warp_grid_torch": torch_warp_grid,
        "split_grad": lambda: D.split_grad(g_sin, g_lv),
        "split_grad_torch": torch_split,
        "warp_backward": lambda: D.warp_backward(g_xw, 0.5, deform, coef, g_dout),
        "warp_backward_torch": torch_warp_bwd,
    }, reps)
    # algorithmic bytes per row: what has to cross HBM once (table gathers are L2 / MALL traffic and not counted)
    bytes_row = {"encode": 12 + 160 + 160, "warp_grid": 12 + 6 + 12 + 12 + 64 + L * 12, "warp_grid_no_jacobian": 12 + 6 + 12 + 12 + 64,
                 "split_grad": 64 + 64, "warp_backward": 6 + 12 + 32}
    return {"rows": B, "ms": ms, "algorithmic_bytes_per_row": bytes_row,
            "us_at_8TBps": {k: v * B / 8e6 for k, v in bytes_row.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["model", "kernels"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dnerf: needs a GPU (no CPU timing is meaningful here)")
    res = {"metric": "dnerf backbone cost"}
    if a.only in (None, "kernels"):
        res["kernels"] = kernels(a.reps)
    if a.only in (None, "model"):
        res["model"] = model(a.reps, a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
