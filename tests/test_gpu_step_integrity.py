"""GPU: a training step updates every parameter or none — the host-side rules around the hash table's in-backward Adam
(NativeAdam.arm_fused_tables -> gridencoder.grid._table_backward -> s3d_grid_encode_backward_adam).

The kernel is pinned elsewhere (test_gpu_optim.py, test_gpu_step_tail.py).  Here the STEP is: with the in-backward update on,
everything a step leaves — master tables, moments, fp16 copies, every other parameter, the step count, the scaler's scale,
growth tracker and flag, the hand-over buffers — equals, bit for bit and after every step, what the same sequence leaves with
`optimizer.fuse_table_updates = False` (the separate update, which test_gpu_optim.py pins against torch.optim.Adam +
torch.amp.GradScaler).  Cases: two tables on two autograd nodes (A), the pair route (B), one table on two nodes (C), a moving
learning-rate schedule on an optimizer whose lr has been captured once (D), a row sum beyond binary16 (E: the one documented
deviation, pinned against a float64 restatement of s3d_adam.hpp), and two-table trainers under a per-step schedule (F).

Shapes: 8,192 points (the first size on the binned backward, below it no update is applied in the backward), tables of
2^14 rows per level, loss scale 1,024, upstream gradients of magnitude <= 24.  Every case that is meant to fuse asserts
`fused_done` between the backward and the step, so no case can quietly compare the separate route with itself."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

B, L = 8192, 16
SCALE = 1024.0
K = 2.0 ** -6  # loss factor: the scaled upstream gradient is SCALE * K * |c| * |w| <= 16 * 1.5


def _encoder(seed):
    from gridencoder import GridEncoder
    torch.manual_seed(seed)
    return GridEncoder(num_levels=L, level_dim=2, base_resolution=16, log2_hashmap_size=14, desired_resolution=2048).cuda()


def _rand(shape, seed, lo=-1.0, hi=1.0):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo).cuda()


class _Rig:
    """tables, plain parameters, optimizer and scaler of one route"""

    def __init__(self, fuse, n_tables, plain_lr=None):
        from nerf.optim import NativeAdam, NativeGradScaler
        self.encs = [_encoder(11 + k) for k in range(n_tables)]
        for e in self.encs:
            e.train()
        self.w = torch.nn.Parameter(_rand((2 * L,), 5, 0.5, 1.5))  # multiplies every table's features, in fp16
        groups = [{"params": [e.embeddings for e in self.encs]}, {"params": [self.w]}]
        if plain_lr is not None:
            groups[1]["lr"] = plain_lr
        self.opt = NativeAdam(groups, lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
        self.opt.fuse_table_updates = fuse
        self.scaler = NativeGradScaler("cuda", init_scale=SCALE)
        self.scaler.attach(self.opt)
        self.tables = [e.embeddings for e in self.encs]
        # device-side poison switches, one per hooked output: 1 = this step's gradient of that output holds an inf
        self.flags = [torch.zeros(1, device="cuda") for _ in range(2)]
        self.masks = {}

    def poisoned(self, y, k, at):
        """y with a hook that sets element `at` of its gradient to inf while flags[k] is 1 (torch.where: capturable)"""
        mask = self.masks.get((k, at))  # (made once, by the first eager step: writing one element is not capturable)
        if mask is None:
            mask = torch.zeros(y.shape, dtype=torch.bool)
            mask[at] = True
            mask = self.masks[(k, at)] = mask.to(y.device)
        flag = self.flags[k]
        y.register_hook(lambda g: torch.where(mask & (flag != 0), torch.full_like(g, float("inf")), g))
        return y

    def snapshot(self):
        opt, sc = self.opt, self.scaler
        out = [("step_count", opt.step_count), ("scale", sc._scale), ("growth_tracker", sc._growth_tracker), ("found_inf", sc._found_inf)]
        for i, p in enumerate(self.tables + [self.w]):
            st = opt.state[p]
            out += [(f"p{i}", p.detach()), (f"p{i}.exp_avg", st["exp_avg"]), (f"p{i}.exp_avg_sq", st["exp_avg_sq"])]
            h = getattr(p, "_s3d", None)
            if h is not None:
                out += [(f"p{i}.half", h.half), (f"p{i}.handover", h.grad)]
        return [(n, t.clone()) for n, t in out]

    def step(self, loss_fn, expect_fused=None):
        """zero_grad -> forward under fp16 autocast -> arm -> backward -> [fused_done as expected] -> step -> update"""
        opt, sc = self.opt, self.scaler
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            loss = loss_fn(self)
        opt.arm_fused_tables(grad_scale=sc._scale)
        sc.backward(loss)
        fused = [bool(t._s3d.fused_done) for t in self.tables]
        if expect_fused is not None and opt.fuse_table_updates:
            expect_fused(fused)
        if not opt.fuse_table_updates:
            assert not any(fused)
        assert all(t._s3d.arm is None for t in self.tables)
        flag = sc._found_inf.clone()
        sc.step(opt)
        sc.update()
        return flag


def _first_difference(a, b):
    """None, or (name, flat index, value a, value b) of the first tensor of two snapshots that differs"""
    for (n, x), (_, y) in zip(a, b):
        if not torch.equal(x, y):
            # (NaN != NaN would show a difference torch.equal does not: compare bits)
            xi, yi = x.flatten().view(torch.int32 if x.element_size() == 4 else torch.int16), y.flatten().view(
                torch.int32 if y.element_size() == 4 else torch.int16)
            k = int((xi != yi).nonzero()[0]) if bool((xi != yi).any()) else 0
            return n, k, float(x.flatten()[k]), float(y.flatten()[k])
    return None


def _assert_skipped(before, after, what):
    """the plain statement of a skipped step: nothing moved, the scale halved, the count stands, the flag is back at 0"""
    a, b = dict(before), dict(after)
    for n in a:
        if n in ("scale", "growth_tracker"):
            continue
        assert torch.equal(a[n], b[n]), (what, "moved in a skipped step", n)
    assert float(b["scale"]) == 0.5 * float(a["scale"]) and int(b["growth_tracker"]) == 0, what
    assert float(b["found_inf"]) == 0.0, what


def _trajectory(fuse, n_tables, loss_fn, plan, expect_fused, check=True):
    """the eager sequence `plan` ((flag 0, flag 1) per step): one snapshot per step, taken behind the next zero_grad"""
    rig = _Rig(fuse, n_tables)
    snaps = [rig.snapshot()]
    for k, switches in enumerate(plan):
        for f, v in zip(rig.flags, switches):
            f.fill_(float(v))
        flag = rig.step(loss_fn, expect_fused if check else None)
        rig.opt.zero_grad()
        snaps.append(rig.snapshot())
        if check:
            assert float(flag) == (1.0 if any(switches) else 0.0), (k, "the poison did not reach the scaler's flag" if any(switches)
                                                                     else "a clean step raised the flag")
            if any(switches):
                _assert_skipped(snaps[-2], snaps[-1], ("fused" if fuse else "separate", "step", k))
            else:
                assert float(snaps[-1][0][1]) == float(snaps[-2][0][1]) + 1.0
    return snaps


def _assert_same(fused, separate, what):
    for k, (a, b) in enumerate(zip(fused, separate)):
        d = _first_difference(a, b)
        assert d is None, (what, "after step", k - 1, "first difference (name, index, fused, separate)", d)


FIVE = [(0, 0), (0, 0), (0, 1), (1, 0), (0, 0)]  # clean, clean, poison in b's gradient, poison in a's gradient, clean
X = lambda seed=3: _rand((B, 3), seed)


def _loss_two_nodes(x, ca, cb):
    def loss_fn(rig):
        wh = rig.w.to(torch.float16)
        ya = rig.poisoned(rig.encs[0](x), 0, (77, 6))      # (point 77, level 3, feature 0)
        yb = rig.poisoned(rig.encs[1](x), 1, (4099, 21))   # (point 4,099, level 10, feature 1)
        return (((ya * wh) * ca).float().sum() + ((yb * wh) * cb).float().sum()) * K
    return loss_fn


def _exactly_one(fused):
    # (which node autograd runs last is its choice: the last one fuses, the other one must not)
    assert sum(fused) == 1, ("of two armed tables on two nodes exactly the last one applies its update in the backward", fused)


def test_a_two_tables_on_two_nodes_skip_or_update_together(hip):
    """A, eager.  enc_a(x), enc_b(x) and one fp16 weight vector on both; clean, clean, inf in b's gradient, inf in a's gradient,
    clean.  Whatever order autograd runs the two nodes in, one of the two poisoned steps has the clean table's node first: a
    table that applies its update there has moved in a step the scaler skips.
    [parent commit: both tables report fused_done; with that assertion off, first difference after the first poisoned step whose
    clean table ran first — the clean table's master weights, moments and fp16 copy moved although the step was skipped]"""
    x, ca, cb = X(), _rand((B, 2 * L), 7).half(), _rand((B, 2 * L), 8).half()
    res = {fuse: _trajectory(fuse, 2, _loss_two_nodes(x, ca, cb), FIVE, _exactly_one) for fuse in (True, False)}
    _assert_same(res[True], res[False], "A eager")
    assert float(dict(res[True][-1])["scale"]) == SCALE / 4 and float(dict(res[True][-1])["step_count"]) == 3.0


def _graphed_trajectory(fuse, x, ca, cb, check=True):
    """A with the whole step in one graph: step 0 eagerly on a side stream (the warm-up), then the capture, then four replays
    with the poison switches flipped on the device in between"""
    from nerf.trainer import _capturing
    rig = _Rig(fuse, 2)
    loss_fn = _loss_two_nodes(x, ca, cb)
    snaps = [rig.snapshot()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rig.step(loss_fn, _exactly_one if check else None)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    snaps.append(rig.snapshot())
    graph = torch.cuda.CUDAGraph()
    with _capturing(graph):
        rig.step(loss_fn, _exactly_one if check else None)
    for k, switches in enumerate(FIVE[1:], start=1):
        for f, v in zip(rig.flags, switches):
            f.fill_(float(v))
        graph.replay()
        torch.cuda.synchronize()
        snaps.append(rig.snapshot())
        if check:
            assert [float(f) for f in rig.flags] == [float(v) for v in switches]  # (the switch the replay read)
            if any(switches):
                _assert_skipped(snaps[-2], snaps[-1], ("fused" if fuse else "separate", "replay", k))
            else:
                assert float(snaps[-1][0][1]) == float(snaps[-2][0][1]) + 1.0
    return snaps


def test_a_two_tables_on_two_nodes_in_a_replayed_graph(hip):
    """A, captured: the same five steps with the step replayed from a graph; the poison switches are device words the hooks read
    through torch.where, so the same graph runs clean and poisoned steps.
    [parent commit: as the eager case — table b moved in the replay whose poison sat in a's gradient]"""
    x, ca, cb = X(), _rand((B, 2 * L), 7).half(), _rand((B, 2 * L), 8).half()
    res = {fuse: _graphed_trajectory(fuse, x, ca, cb) for fuse in (True, False)}
    _assert_same(res[True], res[False], "A graph")
    assert float(dict(res[True][-1])["scale"]) == SCALE / 4 and float(dict(res[True][-1])["step_count"]) == 3.0


def _loss_pair(x, ca, cb):
    from gridencoder.grid import grid_encode_pair

    def loss_fn(rig):
        wh = rig.w.to(torch.float16).view(L, 1, 2)
        pair = grid_encode_pair(rig.encs[0], rig.encs[1], x)
        assert pair is not None
        ya, yb = rig.poisoned(pair[0], 0, (3, 77, 0)), rig.poisoned(pair[1], 1, (10, 4099, 1))  # level-major [L, B, 2]
        return (((ya * wh) * ca).float().sum() + ((yb * wh) * cb).float().sum()) * K
    return loss_fn


def _second_only(fused):
    assert fused == [False, True], ("the pair route applies the second table's update in the backward and no other", fused)


def test_b_the_pair_route_keeps_fusing_its_last_table(hip):
    """B: grid_encode_pair(enc_a, enc_b, x), the same five steps.  The pair's backward scatters a before b and lets only b's
    kernel take the skip decision: a regression guard — the last table must still fuse."""
    x, ca, cb = X(), _rand((L, B, 2), 7).half(), _rand((L, B, 2), 8).half()
    res = {fuse: _trajectory(fuse, 2, _loss_pair(x, ca, cb), FIVE, _second_only) for fuse in (True, False)}
    _assert_same(res[True], res[False], "B")
    assert float(dict(res[True][-1])["step_count"]) == 3.0


def _loss_one_table_twice(x1, x2, c1, c2):
    def loss_fn(rig):
        wh = rig.w.to(torch.float16)
        y1 = rig.encs[0](x1)
        y2 = rig.poisoned(rig.encs[0](x2), 1, (77, 6))
        return (((y1 * wh) * c1).float().sum() + ((y2 * wh) * c2).float().sum()) * K
    return loss_fn


def _none(fused):
    assert fused == [False], ("a table that feeds two nodes of one backward keeps the separate update", fused)


def test_c_one_table_on_two_nodes_loses_no_gradient(hip):
    """C: enc(x1) and enc(x2) in one loss; clean, inf in the second node's gradient, clean.  The in-backward update is formed from
    ONE call's row sums, so a table with two nodes in the pass must not take it: the separate route sums both nodes' gradients
    in the hand-over buffer, and that is what the step has to equal.
    [parent commit: the node that runs first reports fused_done; with that assertion off, first difference after step 0 — the
    table was updated from one node's gradient and the other node's was dropped]"""
    x1, x2, c1, c2 = X(3), X(4), _rand((B, 2 * L), 7).half(), _rand((B, 2 * L), 8).half()
    plan = [(0, 0), (0, 1), (0, 0)]
    res = {fuse: _trajectory(fuse, 1, _loss_one_table_twice(x1, x2, c1, c2), plan, _none) for fuse in (True, False)}
    _assert_same(res[True], res[False], "C")
    assert float(dict(res[True][-1])["step_count"]) == 2.0


def _scheduled_trajectory(fuse, x, c, check=True):
    """D: capture_lr() once, then 8 eager steps with every group's lr at base * 0.1 ** (i / 8), then one step with the first
    group's lr halved (the groups move apart: the optimizer rebases)"""
    rig = _Rig(fuse, 1, plain_lr=3e-3)

    def loss_fn(r):
        return ((r.encs[0](x) * r.w.to(torch.float16)) * c).float().sum() * K

    def fused_here(fused):
        assert fused == [True], ("the one-table route applies its update in the backward", fused)
    base = [g["lr"] for g in rig.opt.param_groups]
    rig.opt.capture_lr()
    snaps = [rig.snapshot()]
    for i in range(9):
        for g, b in zip(rig.opt.param_groups, base):
            g["lr"] = b * 0.1 ** (min(i, 7) / 8)
        if i == 8:
            rig.opt.param_groups[0]["lr"] *= 0.5
        rig.step(loss_fn, fused_here if check else None)
        rig.opt.zero_grad()
        snaps.append(rig.snapshot())
    if check:
        assert float(rig.opt.step_count) == 9.0
        assert rig.opt._lr_captured == [g["lr"] for g in rig.opt.param_groups] and float(rig.opt.lr_scale) == 1.0  # (rebased)
    return snaps


def test_d_a_moving_schedule_reaches_the_in_backward_update_in_the_same_step(hip):
    """D: an optimizer whose lr has been captured once (the eager twin of a graphed trainer) under a per-step schedule.  Launches
    carry the captured lr and a device word carries the schedule's factor; the in-backward update reads that word before step()
    runs, so it must have been brought up to date by then.
    [parent commit: first difference after step 1 — the table was updated with step 0's factor, the plain tensor with step 1's]"""
    x, c = X(), _rand((B, 2 * L), 7).half()
    res = {fuse: _scheduled_trajectory(fuse, x, c) for fuse in (True, False)}
    _assert_same(res[True], res[False], "D")


def test_e_a_row_sum_beyond_binary16_is_the_one_documented_deviation(hip):
    """E: 8,192 points at the centre of the box, which is vertex (8, 8, 8) of level 0 (scale 15: 0.5 * 15 + 0.5 = 8 exactly): one
    row, 8 + 17 * 8 + 289 * 8 = 2,456, takes every point's gradient with weight 1.  Feature 0 gets 8 from every point (exact sum
    65,536 > 65,504), feature 1 gets 1 from every point but 1 + 2^-5 from the first 192 (exact sum 8,198, binary16 8,200); the
    other levels get none.  Every product and every partial sum of 64 neighbours is a binary16 number, so the sums are exact in
    any order.
    Separate route: the gradient table cannot hold 65,536 — the flag is raised, the step is skipped, the scale is halved.
    Fused route (csrc/gridencoder.hip, k_bin_accumulate6<ADAM>): the flag stays 0 and the row is updated by s3d_adam.hpp's rule
    from the exact sum where binary16 overflows and from the binary16-rounded sum elsewhere — restated below in float64.
    Tolerance: rtol 2e-6, atol 1e-7, the suite's fp32-Adam-against-a-reference tolerance (test_native_adam_matches_torch_adam)."""
    ROW = 8 + 17 * 8 + 289 * 8
    x = torch.zeros(B, 3, device="cuda")
    g = torch.zeros(B, 2 * L)
    g[:, 0] = 8.0
    g[:, 1] = 1.0
    g[:192, 1] = 1.0 + 2.0 ** -5
    assert float(g.abs().max()) < 64 and torch.equal(g.half().float(), g)
    W = (g / SCALE).cuda()  # (a power of two: the scaled gradient is g again, exactly)
    out = {}
    for fuse in (True, False):
        rig = _Rig(fuse, 1)
        before = dict(rig.snapshot())

        def fused_here(fused):
            assert fused == [True], fused
        flag = rig.step(lambda r: (r.encs[0](x).float() * W).sum(), fused_here)
        rig.opt.zero_grad()
        out[fuse] = (float(flag), before, dict(rig.snapshot()))
    # separate route: an overflow step like any other
    flag, before, after = out[False]
    assert flag == 1.0
    _assert_skipped(before, after, "E separate")
    assert float(after["step_count"]) == 0.0 and float(after["scale"]) == SCALE / 2
    # fused route: no flag, one step taken, the scale stays
    flag, before, after = out[True]
    assert flag == 0.0 and float(after["found_inf"]) == 0.0
    assert float(after["step_count"]) == 1.0 and float(after["scale"]) == SCALE and int(after["growth_tracker"]) == 1
    assert all(bool(torch.isfinite(t.float()).all()) for t in after.values())
    # float64 restatement: products rounded to binary16 as the scatter forms them (weight 1), summed exactly, the sum rounded
    # to binary16 unless that overflows
    prod = (g[:, :2].numpy().astype(np.float64) * 1.0).astype(np.float16)
    exact = prod.astype(np.float64).sum(axis=0)
    assert exact.tolist() == [65536.0, 8198.0]
    with np.errstate(over="ignore"):
        rounded = exact.astype(np.float16).astype(np.float64)
    assert rounded.tolist() == [float("inf"), 8200.0]
    grad = np.where(np.isfinite(rounded), rounded, exact) / SCALE
    b1, b2, lr, eps, t = float(np.float32(0.9)), float(np.float32(0.99)), float(np.float32(1e-2)), 1e-15, 1.0
    p0 = before["p0"][ROW].cpu().numpy().astype(np.float64)
    m = (1.0 - b1) * grad
    v = (1.0 - b2) * grad * grad
    p = p0 - lr / (1.0 - b1 ** t) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps))
    tol = dict(rtol=2e-6, atol=1e-7)
    print("E fused row", after["p0"][ROW].tolist(), "restated", p.tolist(), "exp_avg", after["p0.exp_avg"][ROW].tolist(), m.tolist(),
          "exp_avg_sq", after["p0.exp_avg_sq"][ROW].tolist(), v.tolist())
    torch.testing.assert_close(after["p0"][ROW].cpu().double(), torch.from_numpy(p), **tol)
    torch.testing.assert_close(after["p0.exp_avg"][ROW].cpu().double(), torch.from_numpy(m), **tol)
    torch.testing.assert_close(after["p0.exp_avg_sq"][ROW].cpu().double(), torch.from_numpy(v), **tol)
    assert torch.equal(after["p0.half"], after["p0"].half())
    # ... and nothing else: rows without a gradient and with zero moments stay where they were
    others = torch.ones(after["p0"].shape[0], dtype=torch.bool, device="cuda")
    others[ROW] = False
    assert torch.equal(after["p0"][others], before["p0"][others])
    assert float(after["p0.exp_avg"][others].abs().max()) == 0.0 and float(after["p0.exp_avg_sq"][others].abs().max()) == 0.0
    assert float(after["p0.handover"].abs().max()) == 0.0  # (the gradient table is neither read nor written)


def _train(hip, monkeypatch, graphed, fused_encoders, fuse):
    """20 steps of the two-table NGP network (2^14-row tables, 2,048 rays) under the reference's per-step LambdaLR"""
    import bench
    from torch.optim.lr_scheduler import LambdaLR
    from nerf import network, synthetic as syn
    from nerf.trainer import GraphedTrainer, Trainer
    from test_gpu_trainer import _run
    torch.manual_seed(0)
    model = network.NeRFNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    model.fused_encoders = fused_encoders
    _, bits = syn.lego_like_density_grid(seed=0)
    batches, _ = bench.make_batches(8, 2048, 0, torch.device("cuda"), hip.RaymarchingBackend, torch.from_numpy(bits).cuda(),
                                    syn.lego_like_boxes(0))
    kw = dict(lr=1e-2, fp16=True, lr_scheduler=lambda o: LambdaLR(o, lambda it: 0.1 ** min(it / 20, 1)))
    tr = GraphedTrainer(model, 2048, **kw) if graphed else Trainer(model, **kw)
    tr.fuse_table_updates = fuse
    if graphed:
        tr.noise_key = 1234
    applied = []
    G = hip.GridBackend
    for name in ("grid_encode_backward_adam", "grid_encode_backward_adam_tail"):
        inner = getattr(G, name)

        def counted(*a, _inner=inner, **k):
            out = _inner(*a, **k)
            applied.append(bool(out[0] if isinstance(out, tuple) else out))
            return out
        monkeypatch.setattr(G, name, staticmethod(counted))
    torch.manual_seed(7)
    losses = _run(tr, batches, 20)
    torch.cuda.synchronize()
    monkeypatch.undo()
    opt = tr.optimizer
    out = [("losses", losses), ("step_count", opt.step_count.clone()), ("scale", tr.scaler._scale.clone()),
           ("growth_tracker", tr.scaler._growth_tracker.clone())]
    names = {id(p): n for n, p in model.named_parameters()}
    params = [p for g in opt.param_groups for p in g["params"]]
    assert len(params) == len(names)
    for p in params:
        n, st = names[id(p)], opt.state[p]
        out += [(n, p.detach().clone()), (n + ".exp_avg", st["exp_avg"].clone()), (n + ".exp_avg_sq", st["exp_avg_sq"].clone())]
        if getattr(p, "_s3d", None) is not None:
            out.append((n + ".half", p._s3d.half.clone()))
    return out, sum(applied)


@pytest.mark.parametrize("variant", ["eager-pair", "eager-two-nodes", "graph-pair"])
def test_f_two_table_trainers_under_a_moving_schedule(hip, monkeypatch, variant):
    """F: nerf.network.NeRFNetwork (density and colour table) trained by Trainer / GraphedTrainer with `fuse_table_updates` on and
    off: losses, every parameter, moments, fp16 copies, step count and scale identical after 20 steps — with the two encoders on
    the pair route and on two separate nodes — and the in-backward update did run where it was switched on.
    [parent commit: passes.  The eager Trainer never captures its lr, so launches carry the group's current value; GraphedTrainer
    brings the factor up to date before every replay; and none of the few steps that fuse here (the first 16 march more points
    than the fixed-scale path takes) overflows, so the two-node order is never put to the test — cases A and D are what sees
    those.  A regression guard: the pair's second table and, on two nodes, the last table keep fusing.]"""
    graphed, fused_encoders = variant == "graph-pair", variant != "eager-two-nodes"
    on, n_on = _train(hip, monkeypatch, graphed, fused_encoders, True)
    off, n_off = _train(hip, monkeypatch, graphed, fused_encoders, False)
    print("F", variant, "in-backward updates applied:", n_on, "/", n_off, "steps taken:", float(dict(on)["step_count"]))
    assert n_on > 0 and n_off == 0, (n_on, n_off)
    assert bool(torch.isfinite(dict(on)["losses"]).all()) and float(dict(on)["step_count"]) > 0
    d = _first_difference(on, off)
    assert d is None, ("F", variant, "first difference (name, index, fused, separate)", d)
