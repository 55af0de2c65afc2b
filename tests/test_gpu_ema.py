"""GPU: csrc/ema.hip (s3d_ema_update_multi, s3d_ema_exchange_multi) against the numpy witness (tests/ema_witness.py), bit for bit
— the update is elementwise with three fp32 roundings and the library is built without contraction, so there is no tolerance —
and the trainers' use of nerf.ema.NativeEMA: update behind every step (eager, captured, skipped, Seal pretraining), evaluation on
the averaged weights by an in-place swap, checkpoints."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import ema_witness as W  # noqa: E402

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 65537]


def _pairs(seed, long_list=True):
    """(param, shadow) pairs: the sizes above, a [4099, 2] table, views that start one element into their allocation (both, and
    the parameter alone: no common 16-byte alignment), a zero-size tensor, and enough small tensors for a second launch batch"""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device="cuda")
    out = [(rnd(n), rnd(n)) for n in SIZES]
    out.append((rnd(4099, 2), rnd(4099, 2)))
    out.append((rnd(1030)[1:], rnd(1030)[1:]))
    out.append((rnd(302)[1:], rnd(301)))
    out.append((rnd(70)[2:], rnd(71)[3:]))
    out.append((torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda")))
    if long_list:
        out += [(rnd(7 + k), rnd(7 + k)) for k in range(70)]
    assert out[10][0].data_ptr() % 16 == 4 and out[10][1].data_ptr() % 16 == 4 and out[11][0].data_ptr() % 16 != out[11][1].data_ptr() % 16
    return out


def _np(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def test_update_multi_matches_the_witness_over_12_updates(hip):
    pairs = _pairs(0)
    assert len([1 for p, _ in pairs if p.numel()]) > 64  # more than one launch's batch
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    wit = W.Witness(_np([s for _, s in pairs]), 0.95)
    g = torch.Generator(device="cuda").manual_seed(1)
    for k in range(12):
        for p, _ in pairs:  # the parameters move between the updates
            p.add_(torch.randn(p.shape, generator=g, device="cuda") * (10.0 ** (k % 5 - 3)))
        hip.EmaBackend.update_multi(pairs, 0.95, count)
        wit.update(_np([p for p, _ in pairs]))
        if k in (0, 5, 11):
            for i, ((_, s), w) in enumerate(zip(pairs, wit.shadows)):
                assert W.same_bits(s.cpu().numpy(), w), (k, i)
    assert int(count.item()) == 12  # (the only read of the count)
    # the constant-decay form: no count, c = float32(1 - decay) at every update
    pairs = _pairs(2, long_list=False)
    wit = W.Witness(_np([s for _, s in pairs]), 0.9, use_num_updates=False)
    for _ in range(2):
        hip.EmaBackend.update_multi(pairs, 0.9, None, use_num_updates=False)
        wit.update(_np([p for p, _ in pairs]))
    assert all(W.same_bits(s.cpu().numpy(), w) for (_, s), w in zip(pairs, wit.shadows))


def test_special_values_behave_as_the_torch_ops_do(hip):
    vals = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1e-45, -1e-40, 1.17549435e-38, 1.0, -2.5, 3e38, -3e38]
    s0 = torch.tensor([a for a in vals for _ in vals], device="cuda")
    p0 = torch.tensor([b for _ in vals for b in vals], device="cuda")
    same = torch.randn(37, device="cuda")
    s0, p0 = torch.cat([s0, same]), torch.cat([p0, same.clone()])  # (s == p: the shadow stays where it is)
    for n in (1, 7, 500):
        s, ref = s0.clone(), s0.clone()
        count = torch.full((1,), n - 1, dtype=torch.int64, device="cuda")
        hip.EmaBackend.update_multi([(p0, s)], 0.95, count)
        tmp = ref - p0
        tmp.mul_(1.0 - W.decay_at(0.95, n))
        ref.sub_(tmp)
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(s), nan) and int(nan.sum()) > 0
        assert torch.equal(s[~nan].view(torch.int32), ref[~nan].view(torch.int32)), n
        assert torch.equal(s[-37:], same) and int(count.item()) == n


def test_captured_update_reads_the_count_on_the_device(hip):
    """one capture, five replays == five eager updates: the decay follows the device count, nothing is baked into the graph"""
    from nerf.trainer import _capturing
    a, b = _pairs(3, long_list=False), _pairs(3, long_list=False)
    ca, cb = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    for pairs, c in ((a, ca), (b, cb)):
        hip.EmaBackend.update_multi(pairs, 0.95, c)  # (update 1, eager on both sides: the first launch loads the kernel)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _capturing(graph):
        hip.EmaBackend.update_multi(a, 0.95, ca)
    for k in range(5):
        for (pa, _), (pb, _) in zip(a, b):
            pa.mul_(1.25)
            pb.mul_(1.25)
        graph.replay()
        hip.EmaBackend.update_multi(b, 0.95, cb)
    torch.cuda.synchronize()
    assert int(ca.item()) == 6 == int(cb.item())
    for i, ((_, sa), (_, sb)) in enumerate(zip(a, b)):
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)), i
    wit = W.Witness(_np([s for _, s in _pairs(3, long_list=False)]), 0.95)
    params = _np([p for p, _ in _pairs(3, long_list=False)])
    for k in range(6):
        if k:
            params = [(p * np.float32(1.25)).astype(np.float32) for p in params]
        wit.update(params)
    assert all(W.same_bits(s.cpu().numpy(), w) for (_, s), w in zip(a, wit.shadows))


def test_exchange_multi_swaps_and_twice_is_the_identity(hip):
    pairs = _pairs(4)
    p0, s0 = [p.clone() for p, _ in pairs], [s.clone() for _, s in pairs]
    hip.EmaBackend.exchange_multi(pairs)
    for (p, s), a, b in zip(pairs, p0, s0):
        assert torch.equal(p.view(torch.int32), b.view(torch.int32)) and torch.equal(s.view(torch.int32), a.view(torch.int32))
    hip.EmaBackend.exchange_multi(pairs)
    for (p, s), a, b in zip(pairs, p0, s0):
        assert torch.equal(p.view(torch.int32), a.view(torch.int32)) and torch.equal(s.view(torch.int32), b.view(torch.int32))
    x = torch.zeros(8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for bad in ([(torch.zeros(8), x)], [(x, torch.zeros(8))], [(x, torch.zeros(9, device="cuda"))], [(x, x.half())],
                [(torch.zeros(4, 4, device="cuda").t(), torch.zeros(16, device="cuda"))]):
        with pytest.raises(RuntimeError):
            hip.EmaBackend.exchange_multi(bad)
        with pytest.raises(RuntimeError):
            hip.EmaBackend.update_multi(bad, 0.95, count)
    with pytest.raises(RuntimeError):
        hip.EmaBackend.update_multi([(x, x.clone())], 0.95, torch.zeros(1, dtype=torch.int64))  # the count is device memory
    with pytest.raises(RuntimeError):
        hip.EmaBackend.update_multi([(x, x.clone())], 1.5, count)
    torch.cuda.synchronize()
    assert int(count.item()) == 0


# ------------------------------------------------------------------ trainers

_BATCHES = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """A trainer is part of a reference cycle, so the ones made here — with their captured graphs and those graphs' private memory
    pools — would otherwise be destroyed whenever the collector next runs, inside some later test.  They go when this module ends."""
    yield
    import gc
    _BATCHES.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _fresh():
    """tests/test_gpu_trainer.py's model and batches (the batches made once), on a settled occupancy grid so that the first step
    already runs — and a graphed trainer already captures — the steady-state step"""
    from nerf import network_ff, synthetic as syn
    from test_gpu_trainer import _setup
    if "b" not in _BATCHES:
        model, _BATCHES["b"] = _setup(n_batches=8)
    else:
        torch.manual_seed(0)
        model = network_ff.NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    model.density_grid.copy_(torch.from_numpy(grid).cuda())
    model.density_bitfield.copy_(torch.from_numpy(bits).cuda())
    model.iter_density = 100
    model.mean_count = 2048 * 40
    return model, _BATCHES["b"]


def _trainer(graphed, **kw):
    from nerf.trainer import GraphedTrainer, Trainer
    model, batches = _fresh()
    kw = dict(dict(lr=1e-2, fp16=True, update_extra_interval=10 ** 9), **kw)
    tr = GraphedTrainer(model, 2048, **kw) if graphed else Trainer(model, **kw)
    tr.global_step = 1
    if graphed:
        tr.noise_key = 1234
    torch.manual_seed(7)
    return tr, model, batches


class _Calls:
    def __init__(self, monkeypatch, hip):
        self.n = {"update_multi": 0, "exchange_multi": 0}
        for name in self.n:
            inner = getattr(hip.EmaBackend, name)

            def counted(*a, _inner=inner, _name=name, **k):
                self.n[_name] += 1
                return _inner(*a, **k)
            monkeypatch.setattr(hip.EmaBackend, name, staticmethod(counted))


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_trainer_shadows_follow_the_witness_and_the_parameters_are_only_read(hip, monkeypatch, graphed):
    """6 steps with ema_decay=0.95: the shadows are the witness applied to the parameters after each step; a twin without an EMA
    gets the same parameters bit for bit and never calls the EMA entry points (its capture records the launches it always did);
    then a step the scaler skips: parameters unchanged, count advanced, shadows moved by the same rule."""
    calls = _Calls(monkeypatch, hip)
    tr, model, batches = _trainer(graphed, ema_decay=0.95)
    params = list(model.parameters())
    assert len(tr.ema.shadow_params) == len(params)
    wit = W.Witness(_np(params), 0.95)
    for i in range(6):
        tr.train_step(*batches[i])
        wit.update(_np(params))
    assert all(W.same_bits(s.cpu().numpy(), w) for s, w in zip(tr.ema.shadow_params, wit.shadows))
    after6 = [p.detach().clone() for p in params]
    if graphed:  # captured at the first step (its warm-up is that step): two host calls, five replays with no host call
        assert tr.graph is not None and tr.n_captures == 1 and calls.n == {"update_multi": 2, "exchange_multi": 0}
    else:
        assert calls.n == {"update_multi": 6, "exchange_multi": 0}
    # the skipped step
    steps0, scale0 = float(tr.optimizer.step_count), tr.scaler.get_scale()
    ro, rd, gt = batches[6]
    bad = gt.clone()
    bad[::3] = float("inf")
    tr.train_step(ro, rd, bad)
    assert float(tr.optimizer.step_count) == steps0 and tr.scaler.get_scale() == 0.5 * scale0
    assert all(torch.equal(a, p.detach()) for a, p in zip(after6, params))
    wit.update(_np(params))
    assert all(W.same_bits(s.cpu().numpy(), w) for s, w in zip(tr.ema.shadow_params, wit.shadows))
    assert tr.ema.state_dict()["num_updates"] == 7
    assert not any(torch.equal(s, p.detach()) for s, p in zip(tr.ema.shadow_params[:1], params[:1]))
    # the twin without an EMA
    n_before = dict(calls.n)
    tw, model2, _ = _trainer(graphed)
    assert tw.ema is None
    for i in range(6):
        tw.train_step(*batches[i])
    assert calls.n == n_before
    assert all(torch.equal(a, p.detach()) for a, p in zip(after6, model2.parameters()))
    if graphed:
        assert tw.graph is not None and tw.n_captures == 1


def _state(tr, model):
    out = []
    for p in model.parameters():
        st = tr.optimizer.state[p]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), p._s3d.half.clone()]
    return out


def test_evaluation_swaps_the_average_in_and_back_without_a_recapture(hip, monkeypatch):
    from nerf.trainer import Trainer
    tr, model, batches = _trainer(True, ema_decay=0.95)
    for i in range(4):
        tr.train_step(*batches[i])
    tw, model2, _ = _trainer(True, ema_decay=0.95)  # the twin never evaluates
    for i in range(4):
        tw.train_step(*batches[i])
    assert all(torch.equal(a, b) for a, b in zip(_state(tr, model), _state(tw, model2)))
    before, shadows = _state(tr, model), [s.clone() for s in tr.ema.shadow_params]
    calls = _Calls(monkeypatch, hip)
    ro, rd, _ = batches[0]
    img = tr.render_image(ro, rd)["image"].clone()
    assert calls.n == {"update_multi": 0, "exchange_multi": 2}
    assert all(torch.equal(a, b) for a, b in zip(before, _state(tr, model)))
    assert all(torch.equal(a, b) for a, b in zip(shadows, tr.ema.shadow_params))
    # ... differs from a render on the raw weights, equals a render of a copy of the model that holds the shadows
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        raw = model.render(ro, rd, bg_color=1, perturb=False, **tr.render_kwargs)["image"].clone()
    copy, _ = _fresh()
    copy.load_state_dict(model.state_dict())
    with torch.no_grad():
        for p, s in zip(copy.parameters(), shadows):
            p.copy_(s)
    ref = Trainer(copy, lr=1e-2, fp16=True).render_image(ro, rd)["image"]
    print("max |ema render - raw render|", float((img - raw).abs().max()), " |ema render - copy's render|", float((img - ref).abs().max()))
    assert not torch.equal(img, raw)
    assert torch.equal(img, ref)
    # the next step: the same loss as the twin's, replayed from the graph captured before the evaluation
    la, lb = tr.train_step(*batches[4]), tw.train_step(*batches[4])
    assert float(la) == float(lb) and tr.n_captures == 1 and tr.graph is not None
    assert all(torch.equal(a, b) for a, b in zip(_state(tr, model), _state(tw, model2)))
    assert all(torch.equal(a, b) for a, b in zip(tr.ema.shadow_params, tw.ema.shadow_params))


def test_checkpoint_restores_shadows_and_count_and_training_resumes_bit_for_bit(hip, tmp_path):
    tr, model, batches = _trainer(True, ema_decay=0.95)
    for i in range(4):
        tr.train_step(*batches[i])
    tr.epoch = 1
    path = tr.save_checkpoint(str(tmp_path), full=True)
    saved = [s.clone() for s in tr.ema.shadow_params]
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck["ema"]) == {"decay", "num_updates", "shadow_params", "collected_params"} and ck["ema"]["num_updates"] == 4
    tr2, model2, _ = _trainer(True, ema_decay=0.95)
    tr2.train_step(*batches[7])  # (own shadows, count and captured graph: all replaced by the load)
    assert tr2.load_checkpoint(path) == ([], [])
    assert tr2.ema.state_dict()["num_updates"] == 4 and tr2.graph is None
    assert all(torch.equal(a, b) for a, b in zip(saved, tr2.ema.shadow_params))
    for t in (tr, tr2):
        # the per-ray jitter of a captured step is drawn from the trainer's running step number, which the reference's checkpoint
        # format does not carry: both runs continue from the same number
        t.s_cursor[1].fill_(100)
        t._pushes = 100
    for i in (4, 5):
        la, lb = tr.train_step(*batches[i]), tr2.train_step(*batches[i])
        assert float(la) == float(lb), i
    assert all(torch.equal(a, b) for a, b in zip(_state(tr, model), _state(tr2, model2)))
    assert all(torch.equal(a, b) for a, b in zip(tr.ema.shadow_params, tr2.ema.shadow_params))
    assert tr.ema.state_dict()["num_updates"] == 6 == tr2.ema.state_dict()["num_updates"]


def test_seal_pretraining_steps_with_frozen_mlps_advance_the_ema(hip):
    from nerf import synthetic as syn
    from sealnerf import SealTrainer
    from test_gpu_configs import _seal_pair
    teacher, student = _seal_pair()
    for m in (teacher, student):
        m.iter_density = 100
    tr = SealTrainer(student, teacher, lr=1e-2, fp16=True, ema_decay=0.95)
    params = list(student.parameters())
    n_params = len(tr.ema.shadow_params)
    assert n_params == len(params)
    tr.init_pretraining(batch_size=6144000, lr=0.05, local_point_step=0.02)
    wit = W.Witness(_np(params), 0.95)
    for k in range(3):  # (eager step, capture of the chunk's graph with the update inside, replay)
        tr.pretrain_one_epoch()
        wit.update(_np(params))
    frozen = [p for p in params if not p.requires_grad]
    assert frozen and len(tr.ema.shadow_params) == n_params == len(list(student.parameters()))
    steps = len(tr.last_pretrain_losses)
    assert steps == 1 and tr.ema.state_dict()["num_updates"] == 3 * steps
    assert all(W.same_bits(s.cpu().numpy(), w) for s, w in zip(tr.ema.shadow_params, wit.shadows))
    assert any(not torch.equal(s, p.detach()) for s, p in zip(tr.ema.shadow_params, params))
