"""Host route of Seal-3D's custom-pose fine-tuning (`--custom_pose`): nerf/synthetic.py `rand_poses` against the reference's
`rand_poses` EXECUTED under torch.manual_seed (tests/golden/custom_pose.npz, tools/gen_custom_pose_golden.py) and against a
float64 witness (tests/custom_pose_witness.py), and sealnerf/provider.py `SealRandomDataset` (SealNeRF/provider.py:145-178):
frame arithmetic, what a batch holds, the torch route.  The GPU twin is tests/test_gpu_custom_pose.py."""
import math

import numpy as np
import pytest
import torch

import custom_pose_witness as cw


@pytest.fixture(scope="module")
def G():
    return cw.load()


def _case(G, tag, **kw):
    from nerf.synthetic import rand_poses
    torch.manual_seed(int(G[f"{tag}_seed"]))
    return rand_poses(G[f"{tag}_u"].shape[0], "cpu", radius=float(G[f"{tag}_radius"]), theta_range=tuple(G[f"{tag}_theta_range"]),
                      phi_range=tuple(G[f"{tag}_phi_range"]), **kw)


@pytest.mark.parametrize("tag", cw.POSE_CASES)
def test_rand_poses_equals_the_reference_bit_for_bit(G, tag):
    assert np.array_equal(_case(G, tag).numpy(), G[f"{tag}_poses"])
    g = torch.Generator().manual_seed(int(G[f"{tag}_seed"]))  # (a private generator seeded alike draws the same stream)
    assert np.array_equal(_case(G, tag, generator=g).numpy(), G[f"{tag}_poses"])


def test_rand_poses_defaults_are_the_references(G):
    from nerf.synthetic import rand_poses
    torch.manual_seed(int(G["a_seed"]))
    assert np.array_equal(rand_poses(1, "cpu").numpy(), G["a_poses"])


@pytest.mark.parametrize("tag", cw.POSE_CASES)
def test_look_at_translates_and_leaves_the_rotation(G, tag):
    look = torch.tensor([0.25, -0.4, 1.5])
    p0, p1 = _case(G, tag), _case(G, tag, look_at=look)
    assert torch.equal(p1[:, :3, :3], p0[:, :3, :3]) and torch.equal(p1[:, 3], p0[:, 3])
    assert torch.equal(p1[:, :3, 3], p0[:, :3, 3] + look)  # the fp32 sum
    # a 0-d tensor radius gives what the number gives
    from nerf.synthetic import rand_poses
    torch.manual_seed(3)
    a = rand_poses(4, "cpu", radius=2.5, look_at=look)
    torch.manual_seed(3)
    b = rand_poses(4, "cpu", radius=torch.tensor(2.5), look_at=look)
    assert torch.equal(a, b)


@pytest.mark.parametrize("tag", cw.POSE_CASES)
@pytest.mark.parametrize("look", [None, (0.25, -0.4, 1.5)])
def test_pose_geometry_against_the_float64_witness(G, tag, look):
    """|centre - look_at| = radius, forward points from the centre to look_at, R is orthonormal — within the reference's own
    fp32 deviation from the witness (a host result gets no more than the reference needs)"""
    tol = cw.reference_deviation(G)
    radius = float(G[f"{tag}_radius"])
    p = _case(G, tag, look_at=None if look is None else torch.tensor(look)).double().numpy()
    W = cw.witness_poses(G[f"{tag}_thetas"], G[f"{tag}_phis"], radius, look)
    scale = 1.0 + (0.0 if look is None else np.abs(look).max() / radius)  # (the sum's rounding grows with the translated centre)
    assert cw.scaled_pose_error(p, W, radius) <= tol * scale
    c = p[:, :3, 3] - (0.0 if look is None else np.asarray(look))
    assert np.abs(np.linalg.norm(c, axis=-1) / radius - 1.0).max() <= 4 * tol * scale
    fwd = p[:, :3, 2]
    assert np.abs(fwd + c / np.linalg.norm(c, axis=-1, keepdims=True)).max() <= 4 * tol * scale
    R = p[:, :3, :3]
    assert np.abs(np.transpose(R, (0, 2, 1)) @ R - np.eye(3)).max() <= 4 * tol


def test_the_witness_bounds_the_fixture_and_the_tolerance_is_the_floor(G):
    dev = cw.reference_deviation(G)
    assert 0 < dev < 5e-7 and cw.device_tolerance(G) == max(4 * dev, 2e-6) == 2e-6


MAP = {"pose_center": torch.tensor([0.1, 0.2, -0.3]), "pose_radius": 1.7}
INTR = (1111.0, 1100.0, 400.0, 300.0)


@pytest.mark.parametrize("H,W,num_rays,expect", [(800, 800, 4096, (64, 64)), (600, 800, 4096, None), (600, 800, -1, (600, 800)),
                                                 (16, 16, 64, (8, 8))])
def test_frame_arithmetic(H, W, num_rays, expect):
    from sealnerf import SealRandomDataset
    ds = SealRandomDataset(MAP, INTR, H, W, num_rays=num_rays)
    s = np.sqrt(H * W / num_rays) if num_rays > 0 else 1.0  # SealNeRF/provider.py:163-165
    assert (ds.H, ds.W) == (int(H / s), int(W / s)) and ds.rays_per_batch == ds.H * ds.W
    if expect is not None:
        assert (ds.H, ds.W) == expect
    assert np.array_equal(ds.intrinsics, np.asarray(INTR, dtype=np.float64) / s)
    val = SealRandomDataset(MAP, INTR, H, W, num_rays=num_rays, training=False, n_val=7)
    assert (val.H, val.W) == (H, W) and len(val) == 7 and len(SealRandomDataset(MAP, INTR, H, W, epoch_length=33)) == 33


def test_defaults_come_from_the_mapper_and_a_map_without_them_raises():
    from sealnerf import SealRandomDataset

    class Mapper:
        map_data = MAP
    ds = SealRandomDataset(Mapper(), INTR, 16, 16, num_rays=64)
    assert torch.equal(ds.look_at, MAP["pose_center"]) and ds.radius == 1.7
    ds = SealRandomDataset({"force_fill_bound": None}, INTR, 16, 16, num_rays=64, look_at=(0, 0, 1), radius=2.0)
    assert ds.radius == 2.0 and ds.look_at.tolist() == [0, 0, 1]
    for bad in ({"force_fill_bound": None}, {"pose_center": MAP["pose_center"]}, None):
        with pytest.raises(ValueError, match="pose_center.*pose_radius"):
            SealRandomDataset(bad, INTR, 16, 16)


@pytest.mark.parametrize("training", [True, False])
def test_collate_is_rand_poses_then_get_rays(training):
    from nerf.synthetic import get_rays, rand_poses
    from sealnerf import SealRandomDataset
    ds = SealRandomDataset(MAP, INTR, 24, 32, num_rays=48, training=training, theta_range=(0.4, 2.0), phi_range=(0.1, 3.0))
    b = ds.collate([0, 1, 2], generator=torch.Generator().manual_seed(5))
    poses = rand_poses(3, "cpu", radius=1.7, theta_range=(0.4, 2.0), phi_range=(0.1, 3.0), look_at=MAP["pose_center"],
                       generator=torch.Generator().manual_seed(5))
    r = get_rays(poses, ds.intrinsics, ds.H, ds.W, -1)
    assert b["H"] == ds.H and b["W"] == ds.W and b["rays_o"].shape == (3, ds.H * ds.W, 3)
    assert torch.equal(b["rays_o"], r["rays_o"]) and torch.equal(b["rays_d"], r["rays_d"])
    assert ("images_shape" in b) == (not training) and "images" not in b and not b.get("skip_proxy")
    if not training:
        assert b["images_shape"] == [3, 24, 32, 3] and (ds.H, ds.W) == (24, 32)
    torch.manual_seed(9)  # generator=None: torch's global stream
    c = ds.collate([0])
    torch.manual_seed(9)
    assert torch.equal(c["rays_d"], get_rays(rand_poses(1, "cpu", radius=1.7, theta_range=(0.4, 2.0), phi_range=(0.1, 3.0),
                                                        look_at=MAP["pose_center"]), ds.intrinsics, ds.H, ds.W, -1)["rays_d"])


def test_sample_needs_the_gpu():
    from sealnerf import SealRandomDataset
    with pytest.raises(RuntimeError, match="GPU"):
        SealRandomDataset(MAP, INTR, 16, 16, num_rays=64).sample([0])


def test_angles_of_the_fixture_stay_in_their_ranges(G):
    for tag in cw.POSE_CASES:
        tr, pr = G[f"{tag}_theta_range"], G[f"{tag}_phi_range"]
        assert np.all((G[f"{tag}_thetas"] >= tr[0]) & (G[f"{tag}_thetas"] <= tr[1]))
        assert np.all((G[f"{tag}_phis"] >= pr[0]) & (G[f"{tag}_phis"] <= pr[1]))
        assert math.isclose(float(G[f"{tag}_thetas"][0]), float(np.float32(G[f"{tag}_u"][0, 0]) * np.float32(tr[1] - tr[0]) + np.float32(tr[0])),
                            rel_tol=1e-6)
