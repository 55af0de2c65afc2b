"""RGBA frames on the reference's per-pixel random background, torch route (CPU): nerf.trainer.rgba_targets and the eager
trainer against tests/golden/rgba_background.npz (written by tools/gen_rgba_background_golden.py from the reference's executed
`Trainer.train_step` / `eval_step`), and the numpy restatement of the device RNG that the GPU tests compare against."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_golden_trainstep import _check_grads, _student

M32 = 0xFFFFFFFF


# ---- the device RNG of s3d_rgba_targets, restated from the description in include/seal3d_hip.h (uint32 arithmetic in uint64)
def pcg_hash(v):
    v = (np.asarray(v, dtype=np.uint64) * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(M32)
    w = (((v >> ((v >> np.uint64(28)) + np.uint64(4))) ^ v) * np.uint64(277803737)) & np.uint64(M32)
    return (w >> np.uint64(22)) ^ w


def hash_u32(key, step, n):
    k = pcg_hash(np.uint64(key) ^ np.uint64((step * 0x9E3779B9) & M32))
    return pcg_hash((k + np.asarray(n, dtype=np.uint64)) & np.uint64(M32))


def bg_uniforms(seed, step, rows):
    """bg [rows, 3] of seed / step: u = (float)(hash_u32(bg_key, step, 3 * row + c) >> 8) * 2^-24, bg_key = pcg_hash(seed ^ 0x3C6EF372)"""
    key = int(pcg_hash((seed & M32) ^ 0x3C6EF372))
    h = hash_u32(key, step, np.arange(3 * rows, dtype=np.uint64))
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(rows, 3)


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "rgba_background.npz"))


def test_fixture_alphas_cover_zero_one_and_between(G):
    a = G["images"][..., 3]
    assert (a == 0).any() and (a == 1).any() and ((a > 0) & (a < 1)).any()


def test_rgba_targets_torch_route_reproduces_the_reference_bit_for_bit(G):
    from nerf.trainer import rgba_targets
    torch.manual_seed(int(G["seed"]))
    gt, bg = rgba_targets(torch.from_numpy(G["images"]))
    assert gt.dtype == torch.float32 and np.array_equal(bg.numpy(), G["a_bg_color"]) and np.array_equal(gt.numpy(), G["a_gt_rgb"])
    torch.manual_seed(int(G["seed"]))
    gt, bg = rgba_targets(torch.from_numpy(G["d_images"]))  # fp16 frames: the reference's half arithmetic
    assert gt.dtype == torch.half and np.array_equal(bg.numpy(), G["d_bg_color"]) and np.array_equal(gt.numpy(), G["d_gt_rgb"])
    gt, bg = rgba_targets(torch.from_numpy(G["c_images"]), random_bg=False)  # evaluation: onto white
    assert bg == 1 and np.array_equal(gt.numpy(), G["c_gt_rgb"])
    rgb = torch.from_numpy(G["images"][..., :3].copy())
    gt, bg = rgba_targets(rgb)
    assert gt is rgb and bg == 1
    g1, b1 = rgba_targets(torch.from_numpy(G["images"]), generator=torch.Generator().manual_seed(3))
    g2, b2 = rgba_targets(torch.from_numpy(G["images"]), generator=torch.Generator().manual_seed(3))
    assert torch.equal(b1, b2) and torch.equal(g1, g2) and not np.array_equal(b1.numpy(), G["a_bg_color"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_eager_step_on_blended_targets_matches_reference_train_step(oracle_wrappers, G, tag):
    """Trainer(native_optim=False) on (gt_rgb, bg_color) of rgba_targets: loss and every gradient of the reference's executed
    step (1e-6, tests/test_golden_trainstep.py), with the map its touched entries (1e-6 absolute, tests/test_error_map.py)"""
    from nerf.trainer import Trainer, rgba_targets
    net = _student()
    net.mean_count = int(G["mean_count"])
    tr = Trainer(net, lr=1e-2, fp16=False, native_optim=False, update_extra_interval=10 ** 9)
    tr.global_step = 1
    kw = {}
    if tag == "b":
        emap = torch.from_numpy(G["b_map"].copy())
        tr.error_map = emap
        kw = dict(index=[0], inds_coarse=torch.from_numpy(G["b_inds_coarse"]))
    torch.manual_seed(int(G["seed"]))
    gt, bg = rgba_targets(torch.from_numpy(G["images"]))  # (the step's first draw, as in the reference; the jitter follows)
    loss = tr.train_step(torch.from_numpy(G[f"{tag}_rays_o"])[0], torch.from_numpy(G[f"{tag}_rays_d"])[0], gt[0], bg_color=bg[0], **kw)
    print(tag, "loss", float(loss), "reference", float(G[f"{tag}_loss"]))
    assert abs(float(loss) - float(G[f"{tag}_loss"])) <= 1e-6 * float(G[f"{tag}_loss"])
    if tag == "a":
        assert np.array_equal(net.step_counter[0].numpy(), G["a_counter"])
        _check_grads(net, G, "a_grad")
    else:
        ic = G["b_inds_coarse"][0]
        np.testing.assert_allclose(emap[0, ic].numpy(), G["b_touched"], rtol=0, atol=1e-6)
        mask = np.ones(emap.shape, dtype=bool)
        mask[0, ic] = False
        assert np.array_equal(emap.numpy()[mask], G["b_map"][mask])


@pytest.mark.parametrize("with_map", [False, True])
def test_four_channel_targets_are_refused_and_the_producers_named(with_map):
    from nerf.trainer import Trainer
    tr = Trainer(_student(), fp16=False)
    kw = {}
    if with_map:
        tr.error_map = torch.ones(1, 128 * 128)
        kw = dict(index=[0], inds_coarse=torch.arange(8).view(1, 8))
    with pytest.raises(ValueError, match="RGBA") as e:
        tr.train_step(torch.zeros(8, 3), torch.ones(8, 3), torch.zeros(8, 4), **kw)
    assert "rgba_targets" in str(e.value) and "sample" in str(e.value)


def test_restated_device_rng_is_uniform():
    """range [0, 1) and mean 0.5 within five standard errors of a uniform's mean, 5 / sqrt(12 n), on n = 3 * 2^16 draws"""
    n = 3 * 2 ** 16
    for seed, step in ((0, 0), (12345, 7)):
        u = bg_uniforms(seed, step, 2 ** 16)
        assert u.dtype == np.float32 and u.shape == (2 ** 16, 3)
        assert u.min() >= 0.0 and u.max() < 1.0
        print(seed, step, "mean", float(u.astype(np.float64).mean()))
        assert abs(float(u.astype(np.float64).mean()) - 0.5) <= 5.0 / np.sqrt(12.0 * n)
    assert not np.array_equal(bg_uniforms(0, 0, 64), bg_uniforms(0, 1, 64))
    assert not np.array_equal(bg_uniforms(0, 0, 64), bg_uniforms(1, 0, 64))
    assert int(pcg_hash(0)) == 129708002  # (the published PCG output permutation of the LCG step from 0)
