#!/usr/bin/env python3
"""Cost of the D-NeRF temporal-basis backbone on one MI355X at its defaults (tiled grid 16 x 2 at 2^19 rows, basis MLP 5 x 128 on one
row, 4,096 rays of the synthetic Lego-shaped scene at one time, fp16 autocast); prints one JSON line.  Everything is measured in ONE
process, the variants alternating, device events around each call (the method of tools/bench_dnerf.py):

  * model: network forward and forward + backward on the marched samples of 4,096 rays, and the eager training step
    (dnerf.utils.Trainer) under a sample budget, on the fused route (csrc/dnerf_basis.hip, the colour fold and the fused MLP entry
    points) against the model's own torch route (`fused_mlp = False`) — the baseline, since no earlier path exists;
  * kernels: the density-head pair against its torch op sequence, with its byte count per row (whole rows: 240 B forward, 356 B
    backward; at 8 TB/s: bytes / 8e6 = microseconds) and the fraction of 8 TB/s the measured time amounts to.

    python tools/bench_dnerf_basis.py [--steps 20] [--reps 10] [--only model|kernels]
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "seal-3d_amd"), HERE]
from bench_dnerf import _alternate, _marched_samples  # noqa: E402

INNER = 20
BYTES_ROW = {"mid_forward": 128 + 12 + 4 + 96, "mid_backward": 96 + 4 + 128 + 128}


def _net(time_size=2):
    from dnerf.network_basis import NeRFNetwork
    from nerf import synthetic as syn
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, time_size=time_size).cuda()
    _, bits = syn.lego_like_density_grid(seed=0)
    for t in range(time_size):
        net.density_bitfield[t].copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


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
                s, c, _ = net(x, d, t)
            ((s.float() * gs).sum() + (c.float() * gc).sum()).backward()
        return run
    out = {"points": m}
    out["network_ms"] = _alternate({"fused_fwd": fwd(True), "torch_fwd": fwd(False), "fused_fwd_bwd": fwd_bwd(True),
                                    "torch_fwd_bwd": fwd_bwd(False)}, reps)
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
    out["eager_step_ms"] = _alternate({tag: (lambda tr=tr, c=[0]: (tr.train_step(*batches[c[0] % 8]), c.__setitem__(0, c[0] + 1)))
                                       for tag, tr in trs.items()}, n_steps, warm=3)
    out["samples_last_step"] = {k: int(v.model.step_counter[:, 0].max()) for k, v in trs.items()}
    return out


def kernels(reps):
    import s3d_hip
    from activation import trunc_exp
    K = s3d_hip.DnerfBasisBackend
    net = _net()
    _, d = _marched_samples()
    B = d.shape[0]
    g = torch.Generator().manual_seed(2)
    h = (torch.randn(B, 64, generator=g) * 0.5).half().cuda()
    sb = (torch.randn(32, generator=g) * 0.2).half().cuda()
    sigma = torch.empty(B, device="cuda")
    cin = torch.empty(B, 48, dtype=torch.float16, device="cuda")
    g_cin = torch.randn(B, 48, generator=g).half().cuda()
    g_sigma = (torch.randn(B, generator=g) * 0.1).cuda()
    g_h = torch.empty(B, 64, dtype=torch.float16, device="cuda")
    g_sb = torch.empty(32, device="cuda")
    state = {}

    def torch_forward():
        hh, sbb = h.clone().requires_grad_(True), sb.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            s = trunc_exp(hh[..., :32] @ sbb)
            c = torch.cat([net.encoder_dir(d), hh[..., 32:]], dim=-1).half()
        state.update(hh=hh, sbb=sbb, s=s, c=c)

    def torch_backward():
        state["hh"].grad = state["sbb"].grad = None
        torch.autograd.backward([state["s"], state["c"]], [g_sigma, g_cin], retain_graph=True)
    torch_forward()
    # (a call of a few microseconds: INNER calls back to back between the two events, so that the launch gap of a single call is
    #  not what is timed)

    def many(fn):
        return lambda: [fn() for _ in range(INNER)]
    ms = _alternate({
        "mid_forward": many(lambda: K.mid_forward(h, d, sb, sigma, cin)),
        "mid_forward_torch": many(torch_forward),
        "mid_backward": many(lambda: K.mid_backward(g_cin, g_sigma, h, sb, g_h, g_sb)),
        "mid_backward_torch": many(torch_backward),
    }, reps)
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
        raise SystemExit("bench_dnerf_basis: needs a GPU (no CPU timing is meaningful here)")
    res = {"metric": "dnerf temporal-basis backbone cost", "reps": a.reps, "steps": a.steps}
    if a.only in (None, "kernels"):
        res["kernels"] = kernels(a.reps)
    if a.only in (None, "model"):
        res["model"] = model(a.reps, a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
