"""CPU: the CCNeRF backbone (tensoRF/network_cc.py).

1. tests/cc_witness.py (float64 numpy statement of the contract: align_corners=False sampling, per-group products, level sums,
   the SH contraction, gradients of lines, planes and S) against torch's CPU grid_sample sequence and its autograd, at the
   tolerances tests/test_tensorf_cp.py uses for the CP witness;
2. the build's network on the torch route against the REFERENCE's, executed (tests/golden/ccnerf.npz from
   tools/gen_ccnerf_golden.py), at the tolerances of tests/test_tensorf_golden.py: parameters, groups, train / eval / K = 2
   forward, density, the L1 term, shrink + upsample, finalize, compress, compose;
3. tensoRF.utils.Trainer on a CCNeRF model: the K-level loss and the L1 term against the golden step; the graphed trainer refuses;
4. a reference-named state dict loads strictly; checkpoints at two compression levels load back, into a model of another
   structure too; a composed scene is refused by the checkpoint code;
5. the renderer's path for 1-D densities is untouched: an existing backbone's training render equals the sequence it ran before."""
import os
import zlib

import numpy as np
import pytest
import torch

import cc_witness as cw
from conftest import GOLDEN

NET = dict(resolution=[20, 17, 13], rank_vec_density=[8, 8, 8], rank_mat_density=[0, 2, 5], rank_vec=[8, 8, 12], rank_mat=[0, 4, 4],
           bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
OTHER = dict(resolution=[9, 14, 11], rank_vec_density=[3, 5], rank_mat_density=[2, 3], rank_vec=[4, 6], rank_mat=[1, 3],
             bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
EMPTY = dict(resolution=[1, 1, 1], rank_vec_density=[1], rank_mat_density=[1], rank_vec=[1], rank_mat=[1],
             bound=2, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
COMPOSE = (dict(s=0.4, t=np.array([0.0, 0.2, 0.0])),
           dict(s=0.6, t=np.array([0.3, -0.1, -0.5]),
                R=np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]) @ np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])))


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


@pytest.fixture(scope="module")
def T():
    return np.load(os.path.join(GOLDEN, "ccnerf.npz"))


def seed_params(net, lo=-0.5, hi=0.5):
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, lo, hi))
    return net


def _net(cfg=NET, lo=-0.5, hi=0.5, grid=True):
    from nerf import synthetic as syn
    from tensoRF import network_cc as cc
    net = seed_params(cc.NeRFNetwork(**cfg), lo, hi)
    if grid:
        dens, bits = syn.lego_like_density_grid(seed=0)
        net.density_grid.copy_(torch.from_numpy(dens))
        net.density_bitfield.copy_(torch.from_numpy(bits))
    return net


def witness_groups(groups):
    """a network's group tuples as the witness's dicts"""
    return [dict(lines=None if l is None else [t.detach().cpu().numpy()[0, :, :, 0] for t in l],
                 planes=None if p is None else [t.detach().cpu().numpy()[0] for t in p],
                 s_vec=None if sv is None else sv.detach().cpu().numpy(), s_mat=None if sm is None else sm.detach().cpu().numpy())
            for l, p, sv, sm in groups]


def edge_points(n, res, seed):
    """uniform points in [-1.3, 1.3]^3 with rows on u = +-1, 0, +-(1 + 0.5 / D), +-(1 + 1 / D), +-(1 + 2^-20) and 3 per axis"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 2.6 - 1.3
    row = 0
    for a in range(3):
        D = float(res[a])
        edge = [-1.0, 1.0, 0.0, -(1 + 0.5 / D), 1 + 0.5 / D, -(1 + 1 / D), 1 + 1 / D, -1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 3.0]
        x[row:row + len(edge), a] = torch.tensor(edge)
        row += len(edge)
    k = 10
    x[row:row + k] = torch.tensor([-1.0, 1.0, 0.0, -1.0001, 1.0001, -1.02, 1.02, -1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 3.0])[:, None]
    return x


RESOLUTIONS = [(12, 20, 16), (1, 2, 65), (65, 1, 2), (2, 65, 1)]


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_witness_matches_the_grid_sample_sequence_and_its_autograd(oracle_wrappers, res):
    from tensoRF import network_cc as cc
    torch.manual_seed(5)
    net = cc.NeRFNetwork(resolution=list(res), degree=3, rank_vec_density=[2, 2, 5], rank_mat_density=[0, 3, 3], rank_vec=[3, 3, 4],
                         rank_mat=[0, 2, 5], bound=1, cuda_ray=False)
    x = edge_points(1500, res, 6)
    d = torch.nn.functional.normalize(_seeded((1500, 3), 7, -1, 1), dim=-1)
    xs, ds = x.numpy(), d.numpy()
    inside = (x.abs() <= 1).all(1).numpy()
    assert 0.2 < inside.mean() < 0.8
    for residual in (True, False):
        net.zero_grad()
        dg, cg = net._groups(True), net._groups(False)
        wd, wc = witness_groups(dg), witness_groups(cg)
        s_ref = net._head(x, None, dg, residual)
        c_ref = net._head(x, d, cg, residual)
        s_wit, c_wit = cw.features(xs, wd, residual), cw.color(xs, ds, wc, 3, residual)
        assert s_ref.shape == s_wit.shape == ((3 if residual else 1), 1500) and c_ref.shape == c_wit.shape
        np.testing.assert_allclose(s_wit, s_ref.detach().numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(c_wit, c_ref.detach().numpy(), rtol=1e-5, atol=1e-7)
        # the align_corners=False property: a point outside [-1, 1] still reads a value
        assert np.abs(s_wit[:, ~inside]).max() > 0 and np.abs(c_wit[:, ~inside]).max() > 0
        gs = torch.randn(s_ref.shape, generator=torch.Generator().manual_seed(8))
        gc = torch.randn(c_ref.shape, generator=torch.Generator().manual_seed(9))
        (s_ref.mul(gs).sum() + c_ref.mul(gc).sum()).backward()
        for groups, wit in ((dg, cw.grads(xs, wd, gs.numpy(), residual)), (cg, cw.grads(xs, wc, gc.numpy(), residual, ds, 3))):
            for (lines, planes, s_vec, s_mat), w in zip(groups, wit):
                pairs = []
                if lines is not None:
                    pairs += list(zip(lines, w["lines"])) + [(s_vec, w["s_vec"])]
                if planes is not None:
                    pairs += list(zip(planes, w["planes"])) + [(s_mat, w["s_mat"])]
                assert pairs
                for p, g in pairs:
                    np.testing.assert_allclose(g.reshape(p.grad.shape), p.grad.numpy(), rtol=2e-4, atol=1e-6)


def test_witness_sh_basis_is_the_encoder(oracle_wrappers):
    from encoding import get_encoder
    d = torch.nn.functional.normalize(_seeded((64, 3), 3, -1, 1), dim=-1)
    for degree in (1, 2, 3, 4):
        enc, _ = get_encoder("sphere_harmonics", degree=degree)
        np.testing.assert_allclose(cw.sh_basis(d.numpy(), degree), enc(d).numpy(), rtol=1e-5, atol=1e-6)


def test_parameters_groups_forward_and_density_loss(oracle_wrappers, T):
    net = _net()
    assert [k for k, _ in net.named_parameters()] == T["param_names"].tolist() and len(T["param_names"]) == 24
    assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["param_shapes"].tolist()
    names = {id(p): k for k, p in net.named_parameters()}
    groups = net.get_params(2e-2, 1e-3)
    assert [g["lr"] for g in groups] == T["group_lrs"].tolist() == [2e-2, 1e-3] * 4
    assert [",".join(names[id(p)] for p in g["params"]) for g in groups] == T["group_members"].tolist()
    assert net.K == [3] and not net.finalized and [g.tolist() for g in net.group_mat_density] == [[0, 2, 3]]
    x, d = torch.from_numpy(T["fw_x"]), torch.from_numpy(T["fw_d"])
    assert (np.abs(T["fw_x"]) > 1).any()
    with torch.no_grad():
        net.train()
        sg, cl = net(x, d)
        assert sg.shape == (3, 300) and cl.shape == (3, 300, 3)
        np.testing.assert_allclose(sg.numpy(), T["train_sigma"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy(), T["train_color"], rtol=1e-6, atol=1e-7)
        sg, cl = net(x, d, K=2)
        assert sg.shape == (2, 300) and cl.shape == (2, 300, 3)
        np.testing.assert_allclose(sg.numpy(), T["train_k2_sigma"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy(), T["train_k2_color"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(net.density(x)["sigma"].numpy(), T["train_density"], rtol=1e-6, atol=1e-7)
        net.eval()
        sg, cl = net(x, d)
        assert sg.shape == (300,) and cl.shape == (1, 300, 3)
        np.testing.assert_allclose(sg.numpy(), T["eval_sigma"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy(), T["eval_color"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(net.density(x)["sigma"].numpy(), T["eval_density"], rtol=1e-6, atol=1e-7)
        # the one extension: eval with K > 0 is the first K groups' output, i.e. level K - 1 of the training output
        sg, cl = net(x, d, K=2)
        assert sg.shape == (300,) and cl.shape == (1, 300, 3)
        np.testing.assert_allclose(sg.numpy(), T["train_k2_sigma"][1], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy()[0], T["train_k2_color"][1], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(net.density(x, K=1)["sigma"].numpy(), T["train_sigma"][0], rtol=1e-6, atol=1e-7)
        for fused in (True, False):
            net.fused_l1 = fused
            assert abs(float(net.density_loss()) - float(T["density_loss"])) <= 1e-6 * float(T["density_loss"])
        assert abs(float(net.density_loss_value()) - float(T["density_loss"])) <= 1e-6 * float(T["density_loss"])
    # the witness on the fixture's own numbers (the reference's forward)
    np.testing.assert_allclose(np.exp(cw.features(T["fw_x"], witness_groups(net._groups(True)))), T["train_sigma"], rtol=1e-5, atol=1e-6)
    logits = cw.color(T["fw_x"], T["fw_d"], witness_groups(net._groups(False)), 4)
    np.testing.assert_allclose(1 / (1 + np.exp(-logits)), T["train_color"], rtol=1e-5, atol=1e-6)


def _check_grads(net, T, prefix, rtol=1e-6):
    for k, p in net.named_parameters():
        key = f"{prefix}_{k.replace('.', '_')}"
        g = p.grad.detach().reshape(-1)
        assert abs(float(g.double().norm()) - float(T[key + "_norm"])) <= rtol * max(float(T[key + "_norm"]), 1e-12), k
        if key in T.files:
            np.testing.assert_allclose(g.numpy(), T[key], rtol=1e-5, atol=rtol * float(np.abs(T[key]).max()), err_msg=k)
        else:
            np.testing.assert_allclose(g[torch.from_numpy(T[key + "_at"])].numpy(), T[key + "_at_values"], rtol=1e-5,
                                       atol=rtol * float(np.abs(T[key + "_at_values"]).max()), err_msg=k)


def test_train_step_with_the_level_loss_and_the_l1_term_matches_the_reference_trainer(oracle_wrappers, T, monkeypatch):
    from tensoRF.utils import Trainer
    net = _net()
    net.mean_count = 32768
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=float(T["ts_l1_weight"]), fp16=False, update_extra_interval=10 ** 9)
    assert [g["lr"] for g in tr.optimizer.param_groups] == T["group_lrs"].tolist()
    tr.global_step = 1
    net.train()
    torch.manual_seed(5)
    ro, rd, gt = (torch.from_numpy(T[k]) for k in ("ts_rays_o", "ts_rays_d", "ts_images"))
    seen = {}
    monkeypatch.setattr(tr, "_reduce_and_step", lambda: seen.update({k: p.grad.clone() for k, p in net.named_parameters()}))
    loss = tr.train_step(ro[0], rd[0], gt[0])
    assert abs(float(loss) - float(T["ts_loss"])) <= 1e-6 * float(T["ts_loss"])
    assert np.array_equal(net.step_counter[0].numpy(), T["ts_counter"])
    for k, p in net.named_parameters():
        p.grad = seen[k]
    _check_grads(net, T, "ts_grad")
    # the per-level prediction, and the criterion as the mean over the levels of the per-level means
    torch.manual_seed(5)
    net.local_step = 0
    with torch.no_grad():
        out = net.render(ro[0], rd[0], bg_color=1, perturb=True, force_all_rays=False, max_steps=1024, dt_gamma=0, T_thresh=1e-4)
    assert out["image"].shape == (3, 256, 3) and out["depth"].shape == (3, 256) and out["weights_sum"].shape == (256,)
    np.testing.assert_allclose(out["image"].numpy(), T["ts_pred"].reshape(3, 256, 3), rtol=1e-5, atol=1e-6)
    from nerf.trainer import render_loss
    per_level = [float(torch.nn.functional.mse_loss(out["image"][k], gt[0])) for k in range(3)]
    assert abs(float(render_loss(out, gt[0])) - np.mean(per_level)) <= 1e-6 * np.mean(per_level)
    want = np.mean(per_level) + float(T["ts_l1_weight"]) * float(T["density_loss"])
    assert abs(float(T["ts_loss"]) - want) <= 1e-5 * want


def test_error_map_takes_the_mean_over_the_levels():
    from nerf.trainer import render_loss
    image = _seeded((3, 8, 3), 1)
    gt = _seeded((8, 3), 2)
    emap = torch.zeros(2, 128 * 128)
    inds = torch.arange(8).reshape(1, 8) * 5
    loss = render_loss({"levels": 3, "image": image, "depth": torch.zeros(3, 8), "weights_sum": torch.ones(8)}, gt, error_map=(emap, [1], inds))
    per_ray = ((image - gt[None]) ** 2).mean(-1).mean(0)
    np.testing.assert_allclose(float(loss), float(per_ray.mean()), rtol=1e-6)
    np.testing.assert_allclose(emap[1, inds[0]].numpy(), 0.9 * per_ray.numpy(), rtol=1e-6)
    assert not emap[0].any()


def test_shrink_and_upsample_follow_the_reference(oracle_wrappers, T):
    net = _net().eval()
    net.mean_density = 5.0
    tl, br = net.shrink_model()
    np.testing.assert_allclose(net.aabb_train.numpy(), T["shrink_aabb"], rtol=0, atol=1e-7)
    assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["shrink_shapes"].tolist()
    assert net.resolution == [b - a for a, b in zip(tl, br)]  # (follows the crop)
    net.upsample_model([30, 26, 22])
    assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["up_shapes"].tolist()
    with torch.no_grad():
        sg, cl = net(torch.from_numpy(T["up_x"]), torch.from_numpy(T["fw_d"][:200]))
    np.testing.assert_allclose(sg.numpy(), T["up_sigma"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(cl.numpy(), T["up_color"], rtol=1e-5, atol=1e-7)


def test_finalize_and_compress_follow_the_reference(oracle_wrappers, T):
    net = _net(grid=False).eval()
    x, d = torch.from_numpy(T["fw_x"]), torch.from_numpy(T["fw_d"])
    with torch.no_grad():
        before = net(x, d)
        net.finalize()
        assert net.finalized and net.K == [1] and net.rank_mat_density == [[5]] and net.rank_vec == [[12]]
        assert [k for k, _ in net.named_parameters()] == T["fin_names"].tolist()
        assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["fin_shapes"].tolist()
        for k, p in net.named_parameters():  # (the importance order of the ranks)
            np.testing.assert_array_equal(p.numpy(), T["fin_param_" + k.replace(".", "_")])
        sg, cl = net(x, d)
        np.testing.assert_allclose(sg.numpy(), T["fin_sigma"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy(), T["fin_color"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(sg.numpy(), before[0].numpy(), rtol=1e-5, atol=1e-6)  # (the same field, re-ordered)
        net.compress((4, 2, 4, 2))
        assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["comp_shapes"].tolist()
        assert net.rank_vec_density == [[4]] and net.group_mat == [[2]]
        sg, cl = net(x, d)
        np.testing.assert_allclose(sg.numpy(), T["comp_sigma"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy(), T["comp_color"], rtol=1e-6, atol=1e-7)
        assert all(p.untyped_storage().nbytes() == p.numel() * 4 for p in net.parameters())  # (clone: no hidden full storage)


def compose_scene(device="cpu"):
    """the golden's scene: two finalized seeded objects in an empty scene, the density-grid sweeps skipped (the forward does not
    read the grid, and the fixture does not record it)"""
    scene = _net(EMPTY, grid=False).eval().to(device)
    scene.update_extra_state = lambda *a, **k: None
    for (cfg, lo, hi), how in zip(((NET, -0.5, 0.5), (OTHER, -0.6, 0.4)), COMPOSE):
        scene.compose(_net(cfg, lo, hi, grid=False).eval().to(device), **how)
    return scene


def test_compose_follows_the_reference(oracle_wrappers, T):
    scene = compose_scene()
    assert scene.K == [1, 1, 1] and scene.rank_vec == [[1], [12], [6]]
    assert [k for k, _ in scene.named_buffers()] == T["cmp_buffers"].tolist()
    with torch.no_grad():
        sg, cl = scene(torch.from_numpy(T["cmp_x"]), torch.from_numpy(T["fw_d"]))
        assert sg.shape == (300,) and cl.shape == (300, 3)
        np.testing.assert_allclose(sg.numpy(), T["cmp_sigma"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(cl.numpy(), T["cmp_color"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(scene.density(torch.from_numpy(T["cmp_x"]))["sigma"].numpy(), T["cmp_density"], rtol=1e-5, atol=1e-6)


def test_a_composed_scene_is_refused_by_the_checkpoint_code(oracle_wrappers, tmp_path):
    from tensoRF.utils import Trainer
    scene = compose_scene()
    tr = Trainer(scene, fp16=False, update_extra_interval=10 ** 9)
    with pytest.raises(ValueError, match="cannot save a composed CCNeRF scene"):
        tr.save_checkpoint(str(tmp_path), name="scene")
    single = Trainer(_net().eval(), fp16=False, update_extra_interval=10 ** 9)
    path = single.save_checkpoint(str(tmp_path), name="single", remove_old=False)
    with pytest.raises(ValueError, match="cannot load a composed CCNeRF scene"):
        tr.load_checkpoint(path)


def test_reference_named_state_dict_loads_strictly(oracle_wrappers, T):
    from tensoRF import network_cc as cc
    net = cc.NeRFNetwork(**NET)
    state = {k: _seeded(eval(s), zlib.crc32(k.encode()) % 1000, -0.5, 0.5) for k, s in zip(T["param_names"].tolist(), T["param_shapes"].tolist())}
    for k, v in net.state_dict().items():  # (buffers of the renderer: not parameters of the reference's class either)
        state.setdefault(k, v.clone())
    net.load_state_dict(state, strict=True)
    with torch.no_grad():
        sg = net.eval().density(torch.from_numpy(T["fw_x"]))["sigma"]
    np.testing.assert_allclose(sg.numpy(), T["eval_density"], rtol=1e-6, atol=1e-7)


def test_checkpoints_at_two_compression_levels_load_back(oracle_wrappers, T, tmp_path):
    from tensoRF import network_cc as cc
    from tensoRF.utils import Trainer
    x, d = torch.from_numpy(T["fw_x"]), torch.from_numpy(T["fw_d"])
    net = _net().eval()
    tr = Trainer(net, fp16=False, update_extra_interval=10 ** 9)
    net.finalize()
    want, paths = {}, {}
    for ranks in ((8, 5, 12, 4), (4, 2, 4, 2)):
        net.compress(ranks)
        name = f"{ranks[0]}_{ranks[1]}-{ranks[2]}_{ranks[3]}"
        paths[name] = tr.save_checkpoint(str(tmp_path), name=name, remove_old=False)
        ckpt = torch.load(paths[name], weights_only=False)
        assert [ckpt[k] for k in ("rank_vec_density", "rank_mat_density", "rank_vec", "rank_mat")] == [[r] for r in ranks]
        assert ckpt["resolution"] == NET["resolution"]
        with torch.no_grad():
            want[name] = [t.numpy().copy() for t in net(x, d)]
    np.testing.assert_allclose(want["4_2-4_2"][0], T["comp_sigma"], rtol=1e-6, atol=1e-7)
    for name, path in paths.items():
        # into an untrained model of the training structure (K = 3, another resolution): re-created from the rank lists
        fresh = Trainer(cc.NeRFNetwork(**{**NET, "resolution": [6, 6, 6]}).eval(), fp16=False, update_extra_interval=10 ** 9)
        old = fresh.model
        missing, unexpected = fresh.load_checkpoint(path)
        assert not missing and not unexpected and fresh.model is not old and fresh.model.finalized and fresh.model.K == [1]
        assert [id(p) for g in fresh.optimizer.param_groups for p in g["params"]] == [id(p) for p in fresh.model.parameters()]
        with torch.no_grad():
            got = fresh.model.eval()(x, d)
        for a, b in zip(got, want[name]):
            np.testing.assert_array_equal(a.numpy(), b)
    # a model that already has the checkpoint's structure is kept
    again = tr.model
    tr.load_checkpoint(paths["4_2-4_2"])
    assert tr.model is again


def test_graphed_trainer_refuses_a_rank_residual_model():
    from tensoRF import network_cc as cc
    from tensoRF.utils import GraphedTrainer
    net = cc.NeRFNetwork(resolution=[4, 5, 6], rank_vec_density=[2, 2], rank_mat_density=[0, 1], rank_vec=[2, 2], rank_mat=[0, 1], cuda_ray=True)
    with pytest.raises(NotImplementedError, match="rank-residual"):
        GraphedTrainer(net, 64)


def test_constructor_defaults_and_refusals():
    from tensoRF import network_cc as cc
    net = cc.NeRFNetwork(resolution=[4, 5, 6])
    assert net.K == [5] and net.degree == 4 and net.out_dim == 48
    assert [g.tolist() for g in (net.group_vec_density[0], net.group_mat_density[0], net.group_vec[0], net.group_mat[0])] == \
        [[64, 0, 0, 0, 0], [0, 4, 4, 4, 4], [64, 0, 0, 0, 0], [0, 4, 12, 16, 32]]
    assert len(net.U_vec_density) == 3 and len(net.U_mat_density) == 12 and len(net.S_mat) == 4
    assert [tuple(v.shape) for v in net.U_vec[:3]] == [(1, 64, 6, 1), (1, 64, 5, 1), (1, 64, 4, 1)]
    assert [tuple(v.shape) for v in net.U_mat[:3]] == [(1, 4, 5, 4), (1, 4, 6, 4), (1, 4, 6, 5)] and tuple(net.S_mat[3].shape) == (48, 32)
    assert 0.17 < float(torch.cat([v.detach().reshape(-1) for v in net.U_vec]).std()) < 0.23  # (init scale 0.2)
    with pytest.raises(ValueError, match="one entry per group"):
        cc.NeRFNetwork(resolution=[4, 5, 6], rank_vec=[8, 8])
    bg = cc.NeRFNetwork(resolution=[4, 5, 6], bg_radius=2.0, bg_resolution=[8, 9], bg_rank=3)
    assert tuple(bg.bg_mat.shape) == (1, 3, 8, 9) and tuple(bg.bg_S.shape) == (48, 3) and len(bg.get_params(1e-2, 1e-3)) == 10


def test_binding_refuses_what_the_kernels_do_not_cover():
    import s3d_hip
    line = [torch.zeros(1, 200, 4, 1)] * 3
    cpu = [(line, None, torch.zeros(1, 200), None)]
    assert "GPU" in s3d_hip.CcBackend.refusal(cpu, 0)
    assert "degree 5" in s3d_hip.CcBackend.refusal([], 5)
    assert "groups" in s3d_hip.CcBackend.refusal([(None, None, None, None)] * 9, 0)
    assert "no component" in s3d_hip.CcBackend.refusal([(None, None, None, None)] * 2, 0)  # (a head compressed to rank 0)
    meta = [([torch.zeros(1, 200, 4, 1, device="meta")] * 3, None, torch.zeros(48, 200, device="meta"), None)]
    assert "table" in s3d_hip.CcBackend.refusal(meta, 4)
    with pytest.raises(RuntimeError, match="fp32 GPU tensors"):
        s3d_hip.CcBackend._groups(cpu, [4, 4, 4], 0, "cc forward")


def test_the_renderer_path_for_1d_densities_is_the_sequence_it_ran_before(oracle_wrappers):
    """a model of an existing backbone (CP): run_cuda's training branch against the same sequence stated by hand — march,
    network, one composite, background — bit for bit, and the reference's recorded prediction of that step"""
    import raymarching
    from nerf import synthetic as syn
    from tensoRF import network_cp as cp
    G = np.load(os.path.join(GOLDEN, "tensorf_cp.npz"))
    net = cp.NeRFNetwork(resolution=[20, 17, 13], sigma_rank=[8, 8, 8], color_rank=[24, 24, 24], bound=1, cuda_ray=True, density_scale=1,
                         min_near=0.2, density_thresh=10)
    seed_params(net)
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net.mean_count = 32768
    net.train()
    ro, rd = torch.from_numpy(G["ts_rays_o"])[0], torch.from_numpy(G["ts_rays_d"])[0]
    with torch.no_grad():
        torch.manual_seed(5)
        out = net.render(ro, rd, bg_color=1, perturb=True, force_all_rays=False, max_steps=1024, dt_gamma=0, T_thresh=1e-4)
        assert out["image"].shape == (256, 3) and out["depth"].shape == (256,) and "loss" not in out
        np.testing.assert_allclose(out["image"].numpy(), G["ts_pred"].reshape(256, 3), rtol=1e-5, atol=1e-6)
        torch.manual_seed(5)
        nears, fars = raymarching.near_far_from_aabb(ro, rd, net.aabb_train, net.min_near)
        counter = net.step_counter[1]
        counter.zero_()
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(ro, rd, net.bound, net.density_bitfield, net.cascade, net.grid_size, nears,
                                                                fars, counter, net.mean_count, True, 128, False, 0, 1024)
        sigmas, rgbs = net(xyzs, dirs)
        assert sigmas.dim() == 1
        weights_sum, depth, image = raymarching.composite_rays_train(sigmas, rgbs, deltas, rays, 1e-4)
        image = image + (1 - weights_sum).unsqueeze(-1) * 1
    assert torch.equal(out["image"], image) and torch.equal(out["depth"], depth) and torch.equal(out["weights_sum"], weights_sum)
