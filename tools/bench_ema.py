"""Cost of the parameter EMA (nerf/ema.py, csrc/ema.hip) at the bench model's parameter set, one invocation, variants alternating
inside every repeat:

  update    s3d_ema_update_multi (one streaming launch + the one-thread count advance)
            vs torch_ema's sequence per tensor (tmp = s - p; tmp.mul_(c); s.sub_(tmp))
            vs the same sequence through torch._foreach_sub / _foreach_mul_ / _foreach_sub_
  exchange  s3d_ema_exchange_multi (parameters <-> shadows, what evaluation costs twice)
  step      the graph-replayed NGP training step (bench.py's model, rays and batches) with ema_decay=None and with 0.95

Times are device events around `--calls` back-to-back calls (per-call time: kernel plus whatever launch gap the stream cannot
hide), `--repeats` times; median and min..max are printed.  The update's traffic model is 12 B per parameter (read parameter and
shadow, write shadow), the exchange's 16 B; both are set against 8 TB/s.  Needs a GPU; prints one JSON line per figure.

    python tools/bench_ema.py [--net ff|seal] [--repeats 7] [--calls 50] [--steps 96] [--no_step]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "seal-3d_amd"))

PEAK = 8.0e12  # B/s


def make_model(net):
    from nerf import network, network_ff
    torch.manual_seed(0)
    cls = network_ff.NeRFNetwork if net == "ff" else network.NeRFNetwork
    return cls(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()


def timed(fn, calls):
    """seconds per call: `calls` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def report(name, xs, **extra):
    s = spread(xs)
    print(json.dumps(dict(figure=name, unit="us", **{k: (round(v * 1e6, 2) if k != "n" else v) for k, v in s.items()}, **extra)), flush=True)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=["ff", "seal"], default="ff", help="bench.py's --net: ff = nerf/network_ff, seal = the two-encoder network")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=96, help="replayed training steps per repeat and variant")
    ap.add_argument("--num_rays", type=int, default=4096)
    ap.add_argument("--no_step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: needs a GPU (nothing here is measured on the CPU)")
    import s3d_hip
    E = s3d_hip.EmaBackend

    model = make_model(args.net)
    params = [p.detach() for p in model.parameters()]
    n = sum(p.numel() for p in params)
    shadows = {k: [p.clone() for p in params] for k in ("native", "torch", "foreach", "exchange")}
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    c = 1.0 - 0.95
    pairs = list(zip(params, shadows["native"]))
    xpairs = list(zip([p.clone() for p in params], shadows["exchange"]))

    def native():
        E.update_multi(pairs, 0.95, count)

    def per_tensor():
        for p, s in zip(params, shadows["torch"]):
            tmp = s - p
            tmp.mul_(c)
            s.sub_(tmp)

    def foreach():
        tmp = torch._foreach_sub(shadows["foreach"], params)
        torch._foreach_mul_(tmp, c)
        torch._foreach_sub_(shadows["foreach"], tmp)

    def exchange():
        E.exchange_multi(xpairs)

    variants = [("update_native", native), ("update_torch_per_tensor", per_tensor), ("update_torch_foreach", foreach),
                ("exchange_native", exchange)]
    for _, fn in variants:  # warm-up: code objects, allocator pools
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            times[name].append(timed(fn, args.calls))
    print(json.dumps({"figure": "parameters", "net": args.net, "tensors": len(params), "elements": n, "update_bytes": 12 * n}), flush=True)
    out = {}
    for name, _ in variants:
        per = 16 if name == "exchange_native" else 12
        med = statistics.median(times[name])
        out[name] = report(name, times[name], model_bytes_per_parameter=per, model_TBps=round(per * n / med / 1e12, 2),
                           share_of_8TBps=round(per * n / med / PEAK, 3))
    print(json.dumps({"figure": "update_speedup", "native_vs_per_tensor": round(out["update_torch_per_tensor"]["median"] / out["update_native"]["median"], 2),
                      "native_vs_foreach": round(out["update_torch_foreach"]["median"] / out["update_native"]["median"], 2)}), flush=True)
    if args.no_step:
        return

    # the graph-replayed training step with and without the EMA: bench.py's batches, a converged occupancy grid
    import bench
    from nerf import synthetic as syn
    from nerf.trainer import GraphedTrainer
    del shadows, pairs, xpairs
    grid, bits = syn.lego_like_density_grid(seed=0)
    batches, _ = bench.make_batches(16, args.num_rays, 0, torch.device("cuda"), s3d_hip.RaymarchingBackend, torch.from_numpy(bits).cuda(),
                                    syn.lego_like_boxes(0))
    trainers = {}
    for name, decay in (("step_without_ema", None), ("step_with_ema", 0.95)):
        m = make_model(args.net)
        m.density_grid.copy_(torch.from_numpy(grid).cuda())
        m.density_bitfield.copy_(torch.from_numpy(bits).cuda())
        m.iter_density = 100
        tr = GraphedTrainer(m, args.num_rays, lr=1e-2, fp16=True, ema_decay=decay)
        for i in range(48):  # sample statistics, capture, replays
            tr.train_step(*batches[i % len(batches)])
        torch.cuda.synchronize()
        assert tr.graph is not None
        trainers[name] = tr
    k = [0]

    def stepper(tr):
        def fn():
            k[0] += 1
            tr.train_step(*batches[k[0] % len(batches)])
        return fn
    times = {name: [] for name in trainers}
    for _ in range(args.repeats):
        for name, tr in trainers.items():
            times[name].append(timed(stepper(tr), args.steps))
    for name in trainers:
        out[name] = report(name, times[name], captures=trainers[name].n_captures)
    d = out["step_with_ema"]["median"] - out["step_without_ema"]["median"]
    print(json.dumps({"figure": "step_cost_of_ema", "unit": "us", "median_difference": round(d * 1e6, 2),
                      "relative": round(d / out["step_without_ema"]["median"], 4)}), flush=True)


if __name__ == "__main__":
    main()
