"""Error-map importance sampling, torch route (CPU): get_rays(error_map=...), the datasets' collate and the trainers' EMA update
against tests/golden/error_map.npz (written by tools/gen_error_map_golden.py from the reference's executed code)."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import REPO

GOLD = os.path.join(REPO, "tests", "golden", "error_map.npz")


def _gold():
    return np.load(GOLD)


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


@pytest.mark.parametrize("tag", ["a", "b"])
def test_get_rays_with_error_map_matches_reference(tag):
    from nerf import synthetic as syn
    d = _gold()
    H, W, N = (int(v) for v in d[f"{tag}_hw"])
    torch.manual_seed(int(d[f"{tag}_seed"]))
    r = syn.get_rays(torch.from_numpy(d[f"{tag}_poses"]), d[f"{tag}_intrinsics"], H, W, N, torch.from_numpy(d[f"{tag}_map"]))
    assert np.array_equal(r["inds_coarse"].numpy(), d[f"{tag}_inds_coarse"])
    assert np.array_equal(r["inds"].numpy(), d[f"{tag}_inds"])
    assert np.array_equal(r["rays_o"].numpy(), d[f"{tag}_rays_o"])
    assert np.array_equal(r["rays_d"].numpy(), d[f"{tag}_rays_d"])


def test_get_rays_without_error_map_is_unchanged():
    from nerf import synthetic as syn
    poses = syn.orbit_poses(1, seed=0)
    r = syn.get_rays(poses, syn.lego_intrinsics(), 800, 800, N=64, generator=torch.Generator().manual_seed(0))
    assert set(r) == {"rays_o", "rays_d", "inds"}
    assert torch.equal(r["inds"][0], torch.randint(0, 800 * 800, size=[64], generator=torch.Generator().manual_seed(0)))


def _student():
    from nerf import synthetic as syn
    from nerf.network import NeRFNetwork
    net = NeRFNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14, density_scale=1, min_near=0.2, density_thresh=10)
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    return net


@pytest.mark.parametrize("tag", ["ts_plain", "ts_depth"])
def test_train_step_error_map_update_matches_reference(oracle_wrappers, tag):
    """one step's loss on the oracle backends with the error map: the touched entries equal the reference's after its
    executed Trainer.train_step, every other entry is exactly unchanged"""
    from sealnerf import SealTrainer
    d = _gold()
    net = _student()
    net.mean_count = int(d["ts_mean_count"])
    tr = SealTrainer(net, net, lr=1e-2, fp16=False)
    emap = torch.from_numpy(d["ts_map"].copy())
    tr.error_map = emap
    inds = torch.from_numpy(d["ts_inds_coarse"])
    depth = torch.from_numpy(d["ts_depths"]) if tag == "ts_depth" else None
    net.train()
    torch.manual_seed(5)
    tr._em_batch = tr._error_map_batch([0], inds, None)
    loss, _ = tr.finetune_loss(torch.from_numpy(d["ts_rays_o"]), torch.from_numpy(d["ts_rays_d"]), torch.from_numpy(d["ts_images"]),
                               depth, bg_color=1)
    tr._em_batch = None
    assert abs(float(loss) - float(d[f"{tag}_loss"])) <= 1e-6 * float(d[f"{tag}_loss"])
    np.testing.assert_allclose(emap[0, inds[0]].numpy(), d[f"{tag}_touched"], rtol=0, atol=1e-6)
    before = d["ts_map"]
    mask = np.ones(before.shape, dtype=bool)
    mask[0, d["ts_inds_coarse"][0]] = False
    assert np.array_equal(emap.numpy()[mask], before[mask])
    rest = np.where(mask, emap.numpy().astype(np.float64), 0.0)
    assert rest.sum() == d[f"{tag}_rest_sum"] and (rest ** 2).sum() == d[f"{tag}_rest_sumsq"]


def test_collate_keys_and_shapes_match_reference():
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    from sealnerf.provider import SealDataset
    poses = syn.orbit_poses(3, seed=0)
    imgs = torch.rand(3, 40, 48, 3)
    ds = NeRFDataset(imgs, poses, syn.lego_intrinsics(40, 48), num_rays=256, error_map=True)
    assert ds.error_map.shape == (3, 128 * 128) and bool((ds.error_map == 1).all())
    b = ds.collate([1])
    assert {"H", "W", "rays_o", "rays_d", "images", "index", "inds_coarse"} <= set(b)
    assert b["rays_o"].shape == (1, 256, 3) and b["rays_d"].shape == (1, 256, 3) and b["images"].shape == (1, 256, 3)
    assert b["inds_coarse"].shape == (1, 256) and b["index"] == [1]
    assert len(set(b["inds_coarse"][0].tolist())) == 256
    assert torch.equal(b["images"][0], imgs[1].view(-1, 3)[b["inds"][0]])
    assert NeRFDataset(imgs, poses, syn.lego_intrinsics(40, 48), fp16=True).images.dtype == torch.half
    plain = NeRFDataset(imgs, poses, syn.lego_intrinsics(40, 48), num_rays=256)
    assert plain.error_map is None and "inds_coarse" not in plain.collate([0]) and "index" not in plain.collate([0])
    sd = SealDataset(poses, syn.lego_intrinsics(40, 48), 40, 48, num_rays=128, images=imgs, error_map=True)
    sd.depths = torch.rand(3, 40, 48, 1)
    s = sd.collate([2])
    assert s["inds_coarse"].shape == (1, 128) and s["index"] == [2] and s["depths"].shape == (1, 128, 1)
    assert {"H", "W", "rays_o", "rays_d", "skip_proxy", "data_index", "pixel_index", "images", "depths"} <= set(s)


def test_error_map_batches_refuse_data_parallelism_and_rgba():
    from nerf.trainer import Trainer
    net = _student()
    tr = Trainer(net, fp16=False)
    tr.error_map = torch.ones(1, 128 * 128)
    inds = torch.arange(8).view(1, 8)
    with pytest.raises(ValueError, match="RGBA"):
        tr.train_step(torch.zeros(8, 3), torch.ones(8, 3), torch.zeros(8, 4), index=[0], inds_coarse=inds)
    tr.dist = object()  # (any process group: the check comes first)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr.train_step(torch.zeros(8, 3), torch.ones(8, 3), torch.zeros(8, 3), index=[0], inds_coarse=inds)
