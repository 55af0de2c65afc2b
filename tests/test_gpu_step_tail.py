"""GPU: the step tail — the training step's four small closing launches (the MLPs' weight-gradient reduce, the criterion's sum,
the MLPs' Adam, the scaler update with the ring push) run inside the hash table's two binned backward launches
(s3d_grid_encode_backward_adam_tail).  Everything the step leaves must equal the separate launches bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

L, T_LOG2, BASE = 16, 14, 16
INTERVAL = 2000
# (grid points, MLP rows, rays, depth term): B = 8,192 is the first size on the binned path and 8,320 is no multiple of the
# scatter's 512-point chunk; 128 MLP rows leave ONE partial per element, fewer than the reduce's split of eight; N = 1,000 and 1
# leave most of the criterion's 1,024 virtual threads without a ray
SHAPES = [(8192, 8192, 4096, False), (8320, 128, 1000, True), (8192, 128, 1, True), (8320, 8192, 1, False),
          (8192, 8192, 1000, False), (8320, 128, 4096, True)]
CASES = ["clean", "mlp_inf", "grid_nan", "growth", "cursor15"]
NETS = [(32, 64, 2), (32, 64, 3)]  # (input, hidden, num_layers): the flagship's 32-64-64-16 and 32-64-64-64-16


def _encoder():
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=L, level_dim=2, base_resolution=BASE, log2_hashmap_size=T_LOG2, desired_resolution=2048)
    return enc.offsets.cuda(), float(np.log2(enc.per_level_scale))


def _state(B, rows_mlp, N, depth, case, table_rows):
    """every buffer of one step, seeded: the same call gives the reference route and the tail route identical starts"""
    g = torch.Generator().manual_seed(B * 7 + rows_mlp * 3 + N + (1 if depth else 0))
    rnd = lambda *s: torch.rand(*s, generator=g)
    s = {}
    s["x"] = rnd(B, 3).cuda()
    grad = (torch.randn(L, B, 2, generator=g) * 3.0).half()
    if case == "grid_nan":
        grad[3, 77, 0] = float("nan")
    s["grad"] = grad.cuda()
    p = (rnd(table_rows, 2) * 2e-4 - 1e-4).cuda()
    s["table"] = [p, (rnd(table_rows, 2) * 1e-3).cuda(), (rnd(table_rows, 2) * 1e-6).cuda(), p.half()]
    s["ge"] = torch.zeros(table_rows, 2, dtype=torch.half, device="cuda")
    nblk = min((rows_mlp // 32 + 3) // 4, 256)
    s["mlp"] = []
    for k, (fin, W, nl) in enumerate(NETS):
        numel = W * fin + (nl - 1) * W * W + 16 * W
        ws = torch.randn((nl + 1) * nblk * 64 * 64, generator=g) * 0.05
        if case == "mlp_inf" and k == 1:
            ws[64 * 64 * nblk + 5 * 64 + 9] = float("inf")  # element (5, 9) of the second layer's first partial
        w = (rnd(numel) - 0.5).cuda()
        s["mlp"].append(dict(ws=ws.cuda(), dims=(fin, W, nl), gw=(torch.randn(numel, generator=g) * 0.01).half().cuda(),
                             p=w, m=(rnd(numel) * 1e-3).cuda(), v=(rnd(numel) * 1e-6).cuda(), h=w.half()))
    s["lws"] = rnd(4 * N).cuda()
    s["loss"] = torch.full((), -1.0, device="cuda")
    s["flag"] = torch.zeros(1, device="cuda")
    s["scale"] = torch.full((1,), 1024.0, device="cuda")
    s["tracker"] = torch.full((1,), INTERVAL - 1 if case == "growth" else 5, dtype=torch.int32, device="cuda")
    s["step"] = torch.full((1,), 3.0, device="cuda")
    s["counter"] = torch.tensor([12345, 678], dtype=torch.int32, device="cuda")
    s["loss_ring"] = torch.zeros(1024, device="cuda")
    s["counter_ring"] = torch.zeros(16, 2, dtype=torch.int32, device="cuda")
    s["cursor"] = torch.tensor([15 if case == "cursor15" else 4, 1030], dtype=torch.int32, device="cuda")
    s["meta"] = (B, rows_mlp, N, depth)
    return s


def _pieces(s):
    B, rows_mlp, N, depth = s["meta"]
    pair = tuple((m["ws"], rows_mlp, m["dims"][0], m["dims"][1], m["dims"][2], m["gw"], True, s["flag"]) for m in s["mlp"])
    loss = (s["lws"], N, depth, 0.25, s["loss"])
    items = [(m["p"], m["gw"], m["m"], m["v"], m["h"], 1e-2, 0.9, 0.99, 1e-15, True) for m in s["mlp"]]
    scaler = (s["scale"], s["tracker"], 2.0, 0.5, INTERVAL, s["step"])
    ring = (s["loss"], s["counter"], s["loss_ring"], s["counter_ring"], s["cursor"])
    t = s["table"]
    adam = dict(param=t[0], exp_avg=t[1], exp_avg_sq=t[2], param_half=t[3], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, step=s["step"],
                grad_scale=s["scale"], lr_scale=None)
    return pair, loss, items, scaler, ring, adam


def _buffers(s):
    out = list(s["table"]) + [s["ge"], s["loss"], s["flag"], s["scale"], s["tracker"], s["step"], s["counter"], s["loss_ring"],
                              s["counter_ring"], s["cursor"]]
    for m in s["mlp"]:
        out += [m["gw"], m["p"], m["m"], m["v"], m["h"]]
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "B%d-mlp%d-N%d-%s" % (v[0], v[1], v[2], "depth" if v[3] else "rgb"))
def test_tail_equals_the_separate_entry_points(hip, shape, case):
    """s3d_grid_encode_backward_adam_tail against wgrad_reduce_pair -> loss_terms_reduce -> grid_encode_backward_adam ->
    adam_step_multi -> step_epilogue on identical state, two consecutive calls on the same control block: every buffer equal,
    every part reported as applied (T = 2^14, base 16 rides: no fallback), control block and found_inf left zero."""
    G, O, F, R = hip.GridBackend, hip.OptimBackend, hip.FFMLPBackend, hip.RaymarchingBackend
    offs, S = _encoder()
    rows = int(offs[-1])
    B = shape[0]
    ref, tail = _state(*shape, case, rows), _state(*shape, case, rows)
    table = ref["table"][3].clone()  # (the forward's table: an input of neither route)
    for rnd in range(2):
        for s in (ref, tail):  # what the rest of a step leaves behind before the table's backward runs
            s["counter"].copy_(torch.tensor([12345 + rnd, 678], dtype=torch.int32))
        pair, loss, items, scaler, ring, adam = _pieces(ref)
        F.wgrad_reduce_pair(*pair)
        R.loss_terms_reduce(*loss)
        assert G.grid_encode_backward_adam(ref["grad"], ref["x"], table, offs, ref["ge"], B, 3, 2, L, S, BASE, 0, False, 0, adam,
                                           found_inf=ref["flag"])
        O.adam_step_multi(items, ref["step"], ref["scale"], ref["flag"])
        O.step_epilogue(*scaler[:2], ref["flag"], *scaler[2:], *ring)
        pair, loss, items, scaler, ring, adam = _pieces(tail)
        applied, parts = G.grid_encode_backward_adam_tail(
            tail["grad"], tail["x"], table, offs, tail["ge"], B, 3, 2, L, S, BASE, 0, False, 0, adam,
            dict(reduce=pair, loss=loss, adam=items, epilogue=scaler + ring), found_inf=tail["flag"])
        assert applied and parts == (G.TAIL_WGRAD_REDUCE | G.TAIL_LOSS | G.TAIL_ADAM | G.TAIL_EPILOGUE), (applied, parts)
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(_buffers(ref), _buffers(tail))):
            assert torch.equal(a, b), (rnd, k, a.flatten()[:4], b.flatten()[:4])
        assert float(tail["flag"]) == 0.0
        ctl = hip._ctl.buf[torch.cuda.current_device()]
        assert int(ctl.count_nonzero()) == 0, "the control block must be left all zero"
        skipped = case in ("mlp_inf", "grid_nan")
        assert float(tail["step"]) == (3.0 if skipped else 4.0 + rnd)
        if rnd == 0:
            assert float(tail["scale"]) == {"mlp_inf": 512.0, "grid_nan": 512.0, "growth": 2048.0}.get(case, 1024.0)
            assert int(tail["cursor"][0]) == (0 if case == "cursor15" else 5) and int(tail["cursor"][1]) == 1031
            assert float(tail["loss_ring"][1030 % 1024]) == float(tail["loss"]) and float(tail["loss"]) > 0
            assert tail["counter_ring"][15 if case == "cursor15" else 4].tolist() == [12345, 678] and tail["counter"].tolist() == [0, 0]
        if skipped:  # nothing moved but the consumed MLP gradients, which are cleared on a skipped step too
            fresh = _state(*shape, case, rows)
            assert all(torch.equal(a, b) for a, b in zip(fresh["table"], tail["table"]))
            assert all(torch.equal(f["p"], m["p"]) and float(m["gw"].abs().max()) == 0.0 for f, m in zip(fresh["mlp"], tail["mlp"]))
            assert float(tail["scale"]) == (512.0 if rnd == 0 else 256.0)  # (the inputs stay poisoned: the second call backs off again)


def test_tail_falls_back_below_the_binned_path(hip):
    """4,096 points take the direct-atomics kernels: nothing rides, the reduce and the criterion's sum are issued in front of the
    backward by the call itself, Adam and the epilogue are left to the caller."""
    G = hip.GridBackend
    offs, S = _encoder()
    rows = int(offs[-1])
    s = _state(4096, 128, 1000, True, "clean", rows)
    gw0 = [m["gw"].clone() for m in s["mlp"]]
    pair, loss, items, scaler, ring, adam = _pieces(s)
    applied, parts = G.grid_encode_backward_adam_tail(s["grad"], s["x"], s["table"][3].clone(), offs, s["ge"], 4096, 3, 2, L, S, BASE, 0,
                                                      False, 0, adam, dict(reduce=pair, loss=loss, adam=items, epilogue=scaler + ring),
                                                      found_inf=s["flag"])
    assert not applied and parts == 0
    assert float(s["loss"]) > 0 and not any(torch.equal(a, m["gw"]) for a, m in zip(gw0, s["mlp"]))
    assert float(s["step"]) == 3.0 and int(s["cursor"][1]) == 1030 and float(s["ge"].abs().max()) > 0


def _malformed(what, s):
    """(reduce pair, loss terms, scaler, ring) of `s` with ONE part malformed.  Wrong dtypes of at least the right byte size, or
    views one element short of the right one: a launch that went unchecked would still stay inside the tensors' allocations."""
    pair, loss, _, scaler, ring, _ = _pieces(s)
    N = s["meta"][2]
    if what == "fp32_grad_weights":
        pair = (pair[0][:5] + (pair[0][5].float(),) + pair[0][6:], pair[1])
    elif what == "fp16_loss_workspace":
        loss = (loss[0].half(),) + loss[1:]
    elif what == "short_loss_workspace":
        loss = (loss[0][:4 * N - 1],) + loss[1:]
    elif what == "int64_growth_tracker":
        scaler = (scaler[0], scaler[1].long()) + scaler[2:]
    elif what == "fp16_adam_step":
        scaler = scaler[:5] + (scaler[5].half(),)
    elif what == "int64_cursor":
        ring = ring[:4] + (ring[4].long(),)
    elif what == "one_element_cursor":
        ring = ring[:4] + (ring[4][:1],)
    elif what == "counter_ring_16x3":
        ring = ring[:3] + (torch.zeros(16, 3, dtype=torch.int32, device="cuda"), ring[4])
    else:
        raise AssertionError(what)
    return pair, loss, scaler, ring


@pytest.mark.parametrize("what", ["fp32_grad_weights", "fp16_loss_workspace", "short_loss_workspace", "int64_growth_tracker",
                                  "fp16_adam_step", "int64_cursor", "one_element_cursor", "counter_ring_16x3"])
def test_a_malformed_tail_part_is_refused_like_its_own_entry_point(hip, what):
    """every part of a step tail is checked as its stand-alone entry point checks it: both refuse the same malformed part with a
    RuntimeError, and the refused tail call has launched nothing — no gradient, no loss, no Adam, no scaler update, no ring push"""
    G, O, F, R = hip.GridBackend, hip.OptimBackend, hip.FFMLPBackend, hip.RaymarchingBackend
    offs, S = _encoder()
    shape = (8192, 128, 1, True)
    s = _state(*shape, "clean", int(offs[-1]))
    adam = _pieces(s)[5]
    pair, loss, scaler, ring = _malformed(what, s)
    with pytest.raises(RuntimeError):
        if what == "fp32_grad_weights":
            F.wgrad_reduce_pair(*pair)
        elif what in ("fp16_loss_workspace", "short_loss_workspace"):
            R.loss_terms_reduce(*loss)
        elif what in ("int64_growth_tracker", "fp16_adam_step"):
            O.scaler_update(*scaler[:2], s["flag"], *scaler[2:])
        else:
            O.step_ring_push(*ring)
    with pytest.raises(RuntimeError):
        G.grid_encode_backward_adam_tail(s["grad"], s["x"], s["table"][3].clone(), offs, s["ge"], shape[0], 3, 2, L, S, BASE, 0, False, 0,
                                         adam, dict(reduce=pair, loss=loss, epilogue=scaler + ring), found_inf=s["flag"])
    torch.cuda.synchronize()
    assert int(s["ge"].count_nonzero()) == 0 and float(s["loss"]) == -1.0
    assert float(s["step"]) == 3.0 and float(s["scale"]) == 1024.0 and s["cursor"].tolist() == [4, 1030]


class _Count:
    """call counters on the binding's entry points (class attributes: every module's `_backend` is the class itself)"""
    NAMES = [("FFMLPBackend", "wgrad_reduce_pair"), ("OptimBackend", "adam_step_multi"), ("OptimBackend", "step_epilogue"),
             ("OptimBackend", "scaler_update"), ("GridBackend", "grid_encode_backward_adam_tail"),
             ("RaymarchingBackend", "loss_terms_reduce")]

    def __init__(self, monkeypatch, hip):
        self.n = {name: 0 for _, name in self.NAMES}
        self.parts = []  # TAIL_* bits reported by each grid_encode_backward_adam_tail call
        for cls, name in self.NAMES:
            inner = getattr(getattr(hip, cls), name)

            def counted(*a, _inner=inner, _name=name, **k):
                self.n[_name] += 1
                out = _inner(*a, **k)
                if _name == "grid_encode_backward_adam_tail":
                    self.parts.append(out[1] if out[0] else 0)
                return out
            monkeypatch.setattr(getattr(hip, cls), name, staticmethod(counted))


def _snapshot(tr, model, losses):
    opt = tr.optimizer
    out = [losses, tr.scaler._scale.clone(), tr.scaler._growth_tracker.clone(), opt.step_count.clone(), model.step_counter.clone()]
    for p in model.parameters():
        st = opt.state[p]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), p._s3d.half.clone(), p._s3d.grad.clone()]
    return out


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_trainer_with_the_tail_equals_the_separate_launches(hip, monkeypatch, graphed):
    """40 steps (occupancy update every 16, one overflow step at loss scale 2^40) with `fuse_step_tail` on and off: losses,
    parameters, moments, fp16 copies, hand-over buffers, scale, growth tracker, step count and the sample-counter ring are
    identical; with the tail on none of the four separate launches is issued by the host.
    The first 16 steps of this run have no sample budget yet and march into 2,048 x 1,024 = 2.1e6 rows, more than the binned
    backward's fixed-scale path takes (2^20 points): there the table's own update does not ride either (parent and branch
    alike), the call reports a fallback, and — as a fallback has to — it issues the reduce itself and leaves Adam and the
    scaler's update to their launches.  So the zero is asserted for every step whose call did not fall back, the fallbacks are
    pinned to exactly those 16 steps, and each of them makes exactly one Adam and one scaler launch.  [measured: eager 40 tail
    calls, 16 fallbacks, 16 adam_step_multi, 16 scaler_update, 0 wgrad_reduce_pair, 0 loss_terms_reduce]"""
    from nerf.trainer import GraphedTrainer, Trainer
    from test_gpu_trainer import _setup
    res, calls, captures = {}, {}, {}
    for on in (True, False):
        model, batches = _setup()
        kw = dict(lr=1e-2, fp16=True, update_extra_interval=16)
        tr = GraphedTrainer(model, 2048, **kw) if graphed else Trainer(model, **kw)
        tr.fuse_step_tail = on
        if graphed:
            tr.noise_key = 1234
        torch.manual_seed(7)
        cnt = _Count(monkeypatch, hip)
        losses = []
        for i in range(40):
            if i == 29:
                tr.scaler._scale.fill_(2.0 ** 40)  # every gradient overflows: the step is skipped, the scale backs off
            if i == 30:
                assert tr.scaler.get_scale() == 2.0 ** 39 and float(tr.optimizer.step_count) == 29.0
                tr.scaler._scale.fill_(2.0 ** 16)
            losses.append(tr.train_step(*batches[i % len(batches)]).float().reshape(()).clone())
        torch.cuda.synchronize()
        monkeypatch.undo()
        print("fuse_step_tail", on, "calls", cnt.n, "captures", getattr(tr, "n_captures", 0))
        if on:
            parts_on = cnt.parts
        res[on], calls[on], captures[on] = _snapshot(tr, model, torch.stack(losses).cpu()), cnt.n, getattr(tr, "n_captures", 0)
        assert float(tr.optimizer.step_count) == 39.0 and float(tr.scaler._found_inf) == 0.0
        assert tr.scaler.get_scale() == 2.0 ** 16
        if graphed:
            assert tr.graph is not None
    for k, (a, b) in enumerate(zip(res[True], res[False])):
        assert torch.equal(a, b), k
    assert torch.isfinite(res[True][0]).all()
    assert captures[True] == captures[False]
    on, off = calls[True], calls[False]
    assert on["grid_encode_backward_adam_tail"] > 0 and off["grid_encode_backward_adam_tail"] == 0
    assert on["wgrad_reduce_pair"] == 0 and on["loss_terms_reduce"] == 0, on
    every = hip.GridBackend.TAIL_WGRAD_REDUCE | hip.GridBackend.TAIL_LOSS | hip.GridBackend.TAIL_ADAM | hip.GridBackend.TAIL_EPILOGUE
    fell_back = [k for k, v in enumerate(parts_on) if v == 0]
    assert fell_back == list(range(16)) and all(v == every for v in parts_on[16:]), parts_on
    assert on["adam_step_multi"] == len(fell_back) and on["step_epilogue"] + on["scaler_update"] == len(fell_back), on
    assert off["wgrad_reduce_pair"] > 0 and off["adam_step_multi"] > 0 and off["step_epilogue"] + off["scaler_update"] > 0, off


@pytest.mark.parametrize("why", ["fuse_table_updates_off", "background_model"])
def test_nothing_rides_where_the_tables_update_does_not(hip, monkeypatch, why):
    """without the in-backward table update, and with a background model (its backward is not ordered behind the table's), the
    step keeps its separate launches"""
    import bench
    from nerf import network, synthetic as syn
    from nerf.trainer import Trainer
    from test_gpu_trainer import _setup
    if why == "background_model":
        torch.manual_seed(0)
        model = network.NeRFNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14, density_scale=1, min_near=0.2, density_thresh=10,
                                    bg_radius=32).cuda()
        _, bits = syn.lego_like_density_grid(seed=0)
        batches, _ = bench.make_batches(4, 2048, 0, torch.device("cuda"), hip.RaymarchingBackend, torch.from_numpy(bits).cuda(),
                                        syn.lego_like_boxes(0))
    else:
        model, batches = _setup(n_batches=4)
    tr = Trainer(model, lr=1e-2, fp16=True)
    assert tr.fuse_step_tail
    if why == "fuse_table_updates_off":
        tr.fuse_table_updates = False
    cnt = _Count(monkeypatch, hip)
    for i in range(4):
        loss = tr.train_step(*batches[i])
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and hip.StepTail.current is None
    assert cnt.n["grid_encode_backward_adam_tail"] == 0 and cnt.n["loss_terms_reduce"] == 0, cnt.n
    assert cnt.n["adam_step_multi"] > 0 and cnt.n["scaler_update"] + cnt.n["step_epilogue"] > 0, cnt.n
    if why == "fuse_table_updates_off":
        assert cnt.n["wgrad_reduce_pair"] > 0, cnt.n
