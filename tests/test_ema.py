"""CPU: nerf/ema.py (NativeEMA: torch_ema 0.3's interface and state layout) against the numpy witness (tests/ema_witness.py), bit
for bit — the update is elementwise with three fp32 roundings, so there is no tolerance to choose — and the trainers' use of it:
update behind every step, checkpoints with an `ema` entry, the `best` file from the averaged weights, re-seeding from a file
without the entry, and identical shadows on the ranks of a data-parallel run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import ema_witness as W


def _params(seed=0, shapes=((7, 3), (5,), (1,), (33, 2))):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]


def _np(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def test_update_matches_the_witness_bit_for_bit_over_200_updates():
    from nerf.ema import NativeEMA
    ps = _params()
    ema, wit = NativeEMA(ps, decay=0.95), W.Witness(_np(ps), 0.95)
    g = torch.Generator().manual_seed(1)
    for k in range(200):
        with torch.no_grad():
            for p in ps:  # (the parameters move between updates, at very different scales)
                p.add_(torch.randn(p.shape, generator=g) * (10.0 ** ((k % 7) - 4)))
        ema.update()
        wit.update(_np(ps))
        for s, w in zip(ema.shadow_params, wit.shadows):
            assert W.same_bits(s.numpy(), w), k
    assert ema.state_dict()["num_updates"] == 200 == wit.num_updates
    assert not any(torch.equal(s, p.detach()) for s, p in zip(ema.shadow_params, ps))


def test_decay_schedule():
    from nerf.ema import NativeEMA, decay_at
    ds = [W.decay_at(0.95, n) for n in range(1, 400)]
    first = next(n for n in range(1, 400) if (1 + n) / (10 + n) >= 0.95)
    assert first == 170
    assert all(ds[n - 1] == (1 + n) / (10 + n) for n in range(1, first)) and all(d == 0.95 for d in ds[first - 1:])
    assert all(decay_at(0.95, n) == ds[n - 1] for n in range(1, 400)) and decay_at(0.95, None) == 0.95
    assert all(W.decay_at(0.95, n, use_num_updates=False) == 0.95 for n in (1, 5, 1000))
    # the constant form through the class: every update uses c = float32(1 - 0.95), and nothing is counted
    ps = _params(2)
    ema, wit = NativeEMA(ps, decay=0.95, use_num_updates=False), W.Witness(_np(ps), 0.95, use_num_updates=False)
    for k in range(3):
        with torch.no_grad():
            ps[0].add_(1.0)
        ema.update()
        assert wit.update(_np(ps)) == np.float32(1.0 - 0.95)
    assert all(W.same_bits(s.numpy(), w) for s, w in zip(ema.shadow_params, wit.shadows))
    assert ema.state_dict()["num_updates"] is None
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            NativeEMA(_params(), decay=bad)


def test_a_contracted_multiply_subtract_would_be_seen():
    """the bitwise comparison discriminates: one rounding instead of two in `s - t * c` changes a sizeable share of elements"""
    rng = np.random.default_rng(0)
    s, p = rng.standard_normal(100000).astype(np.float32), rng.standard_normal(100000).astype(np.float32)
    for n in (1, 12, 1000):
        c = W.coefficient(0.95, n)
        share = float(np.mean(W.update(s, p, c).view(np.uint32) != W.contracted_update(s, p, c).view(np.uint32)))
        assert 0.05 < share < 0.6, (n, share)


def test_state_dict_layout_load_and_validation():
    from nerf.ema import NativeEMA
    ps = _params(3)
    ps[1].requires_grad_(False)  # a frozen parameter stays in the list
    ema = NativeEMA(ps, decay=0.9)
    for _ in range(3):
        with torch.no_grad():
            ps[0].mul_(1.5)
        ema.update()
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert sd["decay"] == 0.9 and isinstance(sd["decay"], float) and sd["num_updates"] == 3 and isinstance(sd["num_updates"], int)
    assert isinstance(sd["shadow_params"], list) and len(sd["shadow_params"]) == len(ps) and sd["collected_params"] is None
    assert all(s.shape == p.shape and s.dtype == p.dtype and not s.requires_grad for s, p in zip(sd["shadow_params"], ps))
    ema.store()
    assert [c.shape for c in ema.state_dict()["collected_params"]] == [p.shape for p in ps]
    # a dict fabricated in the layout, in fp64 (and on another device where there is one): cast to each parameter's dtype / device
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    fab = {"decay": 0.5, "num_updates": 41, "shadow_params": [torch.full(p.shape, 0.1 * k, dtype=torch.float64, device=dev) for k, p in enumerate(ps)],
           "collected_params": [torch.full(p.shape, -1.0 * k, dtype=torch.float64, device=dev) for k, p in enumerate(ps)]}
    ema.load_state_dict(fab)
    out = ema.state_dict()
    assert out["decay"] == 0.5 and out["num_updates"] == 41
    for k, (s, c, p) in enumerate(zip(out["shadow_params"], out["collected_params"], ps)):
        assert s.dtype == p.dtype and s.device == p.device and torch.equal(s, torch.full(p.shape, 0.1 * k, dtype=torch.float64).float())
        assert c.dtype == p.dtype and c.device == p.device and torch.equal(c, torch.full(p.shape, -1.0 * k))
    # the next update is number 42
    wit = W.Witness(_np(out["shadow_params"]), 0.5)
    wit.num_updates = 41
    ema.update()
    wit.update(_np(ps))
    assert all(W.same_bits(s.numpy(), w) for s, w in zip(ema.shadow_params, wit.shadows))
    for broken, exc in ((dict(fab, shadow_params=fab["shadow_params"][:-1]), ValueError),
                        (dict(fab, collected_params=fab["collected_params"] + [torch.zeros(1)]), ValueError),
                        (dict(fab, shadow_params=tuple(fab["shadow_params"])), TypeError),
                        (dict(fab, shadow_params=[t.tolist() for t in fab["shadow_params"]]), TypeError),
                        (dict(fab, num_updates=1.5), TypeError), (dict(fab, decay=2.0), ValueError)):
        with pytest.raises(exc):
            ema.load_state_dict(broken)
    with pytest.raises(ValueError):
        ema.update(ps[:-1])


def test_store_copy_to_restore_and_average_parameters():
    from nerf.ema import NativeEMA
    ps = _params(4)
    calls = []
    ema = NativeEMA(ps, decay=0.9, on_weights_changed=lambda: calls.append(1))
    with pytest.raises(RuntimeError):
        ema.restore()
    with torch.no_grad():
        for p in ps:
            p.add_(1.0)
    ema.update()
    own, avg = [p.detach().clone() for p in ps], [s.clone() for s in ema.shadow_params]
    ema.store()
    assert all(c is not p and torch.equal(c, p) for c, p in zip(ema.collected_params, ps))
    ema.copy_to()
    assert all(torch.equal(p, a) for p, a in zip(ps, avg)) and len(calls) == 1
    ema.restore()
    assert all(torch.equal(p, o) for p, o in zip(ps, own)) and len(calls) == 2
    with ema.average_parameters():
        assert all(torch.equal(p, a) for p, a in zip(ps, avg))
    assert all(torch.equal(p, o) for p, o in zip(ps, own)) and all(torch.equal(s, a) for s, a in zip(ema.shadow_params, avg))
    assert len(calls) == 4


# ------------------------------------------------------------------ trainers on the CPU (the marcher runs on the oracle)

def _analytic_model(seed):
    from nerf import renderer, synthetic as syn
    lo, hi = syn.lego_like_boxes(0)

    class Analytic(renderer.NeRFRenderer):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.w = torch.nn.Parameter(torch.ones(3))
            self.mix = torch.nn.Linear(3, 3, bias=False)
            self.frozen = torch.nn.Parameter(torch.full((2,), 3.0), requires_grad=False)

        def forward(self, x, dd):
            rgb = torch.sigmoid(self.mix((x * 0.5 + 0.5).clamp(0, 1) * (0.5 + 0.5 * dd.abs())) * self.w)
            return syn.box_density(x, lo, hi, sigma=40.0), rgb

        def density(self, x):
            return {"sigma": syn.box_density(x, lo, hi, sigma=40.0)}

        def get_params(self, lr):
            return [{"params": [self.w, self.mix.weight], "lr": lr}]

    torch.manual_seed(seed)
    R = Analytic(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
    R.grid_size = 32
    R.density_grid = torch.zeros(1, 32 ** 3)
    R.density_bitfield = torch.zeros(32 ** 3 // 8, dtype=torch.uint8)
    R.train()
    for it in range(3):
        R.iter_density = max(R.iter_density, 15 if it == 1 else R.iter_density)
        R.update_extra_state()
    return R


def _batches(n, rays=96):
    from nerf import synthetic as syn
    r = syn.get_rays(syn.orbit_poses(1, seed=0), syn.lego_intrinsics(32, 32), 32, 32)
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(n):
        idx = torch.randint(0, 32 * 32, (rays,), generator=g)
        out.append((r["rays_o"][0, idx].contiguous(), r["rays_d"][0, idx].contiguous(), torch.rand(rays, 3, generator=g)))
    return out


@pytest.fixture()
def cpu_marcher(oracle, monkeypatch):
    import raymarching.raymarching as rm
    monkeypatch.setattr(rm, "_backend", oracle.RaymarchingBackend)


def _cpu_trainer(seed=0, **kw):
    from nerf.trainer import Trainer
    tr = Trainer(_analytic_model(seed), lr=1e-2, fp16=False, update_extra_interval=10 ** 9, native_optim=False, **kw)
    tr.global_step = 1  # (no occupancy sweep at the first step: the grid above is settled)
    return tr


def test_cpu_trainer_updates_checkpoints_and_reseeds(cpu_marcher, tmp_path):
    tr = _cpu_trainer(ema_decay=0.95)
    model = tr.model
    assert len(tr.ema.shadow_params) == len(list(model.parameters())) == 3  # the frozen parameter is in the list
    assert _cpu_trainer().ema is None
    wit = W.Witness(_np(model.parameters()), 0.95)
    batches = _batches(5)
    for b in batches:
        before = _np(model.parameters())
        tr.train_step(*b)
        assert not all(np.array_equal(a, p) for a, p in zip(before, _np(model.parameters())))
        wit.update(_np(model.parameters()))
        assert all(W.same_bits(s.numpy(), w) for s, w in zip(tr.ema.shadow_params, wit.shadows))
    assert tr.ema.state_dict()["num_updates"] == 5
    # full checkpoint: an `ema` entry in torch_ema's layout, restored into a fresh trainer
    tr.epoch = 1
    path = tr.save_checkpoint(str(tmp_path), name="a", full=True)
    ck = torch.load(path, weights_only=False)
    assert set(ck["ema"]) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert ck["ema"]["decay"] == 0.95 and ck["ema"]["num_updates"] == 5 and ck["ema"]["collected_params"] is None
    assert all(torch.equal(a, b) for a, b in zip(ck["ema"]["shadow_params"], tr.ema.shadow_params))
    tr2 = _cpu_trainer(seed=1, ema_decay=0.95)
    tr2.load_checkpoint(path)
    assert tr2.ema.state_dict()["num_updates"] == 5
    assert all(torch.equal(a, b) for a, b in zip(tr2.ema.shadow_params, tr.ema.shadow_params))
    assert all(torch.equal(a, b) for a, b in zip(tr2.model.parameters(), model.parameters()))
    # evaluation renders with the averaged weights and leaves the trainer's own in place
    own = [p.detach().clone() for p in model.parameters()]
    ro, rd, _ = batches[0]
    img = tr.render_image(ro, rd)["image"]
    assert all(torch.equal(a, p.detach()) for a, p in zip(own, model.parameters()))
    with tr.ema.average_parameters():
        model.eval()
        with torch.no_grad():
            ref = model.render(ro, rd, bg_color=1, perturb=False, **tr.render_kwargs)["image"]
    with torch.no_grad():
        raw = model.render(ro, rd, bg_color=1, perturb=False, **tr.render_kwargs)["image"]
    assert torch.equal(img, ref) and not torch.equal(img, raw)
    # `best`: the averaged weights; a file without `ema` (this one) re-seeds shadows and count from the loaded weights
    tr.stats["results"].append(0.5)
    best = tr.save_checkpoint(str(tmp_path), name="a", best=True)
    bk = torch.load(best, weights_only=False)
    assert "ema" not in bk and "density_grid" not in bk["model"]
    names = [n for n, _ in model.named_parameters()]
    assert all(torch.equal(bk["model"][n], s) for n, s in zip(names, tr.ema.shadow_params))
    assert all(torch.equal(a, p.detach()) for a, p in zip(own, model.parameters()))
    tr3 = _cpu_trainer(seed=2, ema_decay=0.95)
    tr3.ema.update()
    tr3.load_checkpoint(best, model_only=True)
    assert tr3.ema.state_dict()["num_updates"] == 0
    assert all(torch.equal(s, p.detach()) and torch.equal(s, b) for s, p, b in zip(tr3.ema.shadow_params, tr3.model.parameters(),
                                                                                   tr.ema.shadow_params))


_DP_SCRIPT = r'''
import os, sys, torch, torch.distributed as dist
repo = os.environ["S3D_REPO"]
sys.path.insert(0, repo); sys.path.insert(0, os.path.join(repo, "seal-3d_amd")); sys.path.insert(0, os.path.join(repo, "tests"))
from parallel import RayShardedDP, init_from_env, shard_slice
rank, world, _ = init_from_env("gloo")
from oracle import oracle_backend as ob
import raymarching.raymarching as rm
rm._backend = ob.RaymarchingBackend
ob.set_threads(1)
import test_ema as T
from nerf.trainer import Trainer
model = T._analytic_model(100 + rank)     # replicas start DIFFERENT: the trainer's register() adopts rank 0's weights
with torch.no_grad():
    model.w.add_(float(rank))
tr = Trainer(model, lr=1e-2, fp16=False, update_extra_interval=10 ** 9, native_optim=False, dist=RayShardedDP(), ema_decay=0.95)
tr.global_step = 1
seeded = all(torch.equal(s, p.detach()) for s, p in zip(tr.ema.shadow_params, model.parameters()))
for ro, rd, gt in T._batches(3, rays=96):
    lo, hi = shard_slice(96, rank, world)
    tr.train_step(ro[lo:hi], rd[lo:hi], gt[lo:hi])
flat = torch.cat([s.reshape(-1) for s in tr.ema.shadow_params])
got = [torch.zeros_like(flat) for _ in range(world)]
dist.all_gather(got, flat)
same = all(torch.equal(got[0].view(torch.int32), g.view(torch.int32)) for g in got)
moved = not all(torch.equal(s, p.detach()) for s, p in zip(tr.ema.shadow_params, model.parameters()))
print(f"RANK{rank} seeded={seeded} same={same} moved={moved} n={tr.ema.state_dict()['num_updates']}")
dist.destroy_process_group()
'''


def test_shadows_agree_across_two_gloo_ranks(oracle, tmp_path):
    """data parallelism: every rank holds the same parameters after a step, so the shadows agree with no communication"""
    script = tmp_path / "dp_ema.py"
    script.write_text(_DP_SCRIPT)
    env = dict(os.environ, S3D_REPO=REPO, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", str(script)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    for r in (0, 1):
        assert f"RANK{r} seeded=True same=True moved=True n=3" in res.stdout, res.stdout + res.stderr[-1500:]


class _Items:
    """a loader of fixed items (sdf/utils.py reads `loader.dataset.epoch` where there is one)"""
    dataset = None

    def __init__(self, items):
        self.items = items

    def __iter__(self):
        return iter(self.items)


def test_sdf_trainer_keeps_the_average_and_evaluates_on_it(oracle_wrappers, tmp_path):
    from sdf.network import SDFNetwork
    from sdf.utils import Trainer
    torch.manual_seed(0)
    net = SDFNetwork(encoding="hashgrid")
    g = torch.Generator().manual_seed(1)
    items = [{"points": torch.rand(1, 64, 3, generator=g) * 2 - 1, "sdfs": torch.rand(1, 64, 1, generator=g) - 0.5} for _ in range(3)]
    tr = Trainer("s", net, fp16=False, device="cpu", mute=True, workspace=str(tmp_path), use_checkpoint="scratch", ema_decay=0.95,
                 optimizer=lambda m: torch.optim.Adam(m.parameters(), lr=1e-2))
    assert Trainer("s", SDFNetwork(encoding="hashgrid"), fp16=False, device="cpu", mute=True).ema is None
    params = list(net.parameters())
    wit = W.Witness(_np(params), 0.95)
    for item in items:  # (one step per epoch: the parameters after every step are on hand for the witness)
        tr.train_one_epoch(_Items([item]))
        wit.update(_np(params))
    assert tr.ema.state_dict()["num_updates"] == 3
    assert all(W.same_bits(s.numpy(), w) for s, w in zip(tr.ema.shadow_params, wit.shadows))
    own = [p.detach().clone() for p in params]
    avg_loss = tr.evaluate_one_epoch(_Items(items[:1]))
    assert all(torch.equal(a, p.detach()) for a, p in zip(own, params))
    net.eval()
    with torch.no_grad():
        raw_loss = float(tr.eval_step(items[0])[2])
        with tr.ema.average_parameters():
            ref_loss = float(tr.eval_step(items[0])[2])
    assert avg_loss == ref_loss and avg_loss != raw_loss
    tr.epoch = 1
    ck = torch.load(tr.save_checkpoint(full=True), weights_only=False)
    assert ck["ema"]["num_updates"] == 3 and len(ck["ema"]["shadow_params"]) == len(params)
