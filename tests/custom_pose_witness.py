"""Float64 witness of the custom-pose batches (nerf/provider.py:57-91 `rand_poses` + look_at, nerf/utils.py:124-133 `get_rays`)
and the tolerance the device route is held to, shared by tests/test_custom_pose.py and tests/test_gpu_custom_pose.py.

The witness starts from the fp32 angles (tests/golden/custom_pose.npz `*_thetas`, `*_phis`) and does everything after them in
float64 with numpy, so the deviation of an fp32 result from it is that result's own rounding: trigonometry, three
normalisations, the rotation of the pixel direction.

Tolerance (derived, not picked): `reference_deviation(G)` is the largest absolute deviation of the REFERENCE's fp32 results in
the fixture from the witness — pose entries (translations divided by the radius) and ray directions — measured as 1.49e-07
(poses 8.4e-08, ray directions 1.49e-07: a little over one fp32 ulp below 1; rotation columns and directions are unit
vectors).  The device gets four times that (its sinf / cosf and reciprocal square root are within a couple of ulp where the
host's are within one, and the chain is three normalisations deep), but never less than the 2e-6 the project grants its
fp32 trigonometric kernels (frequency encoder, sph_from_ray; README "Parity"): TOL = max(4 x 1.49e-07, 2e-6) = 2e-6.  The
tests recompute the deviation from the fixture (`device_tolerance`), so the bound cannot drift from the data."""
import os

import numpy as np

from conftest import GOLDEN

POSE_CASES = ("a", "b")
FRAMES = (("a", 5, 7), ("a", 67, 131), ("b", 5, 7))
FLOOR = 2e-6  # README "Parity": fp32 trigonometric kernels


def load():
    return np.load(os.path.join(GOLDEN, "custom_pose.npz"))


def _normalize(v):
    return v / (np.linalg.norm(v, axis=-1, keepdims=True) + 1e-10)


def witness_poses(thetas, phis, radius, look_at=None):
    """[B, 4, 4] float64 from the (fp32) angles"""
    th, ph = np.asarray(thetas, dtype=np.float64), np.asarray(phis, dtype=np.float64)
    radius = float(radius)
    off = np.stack([radius * np.sin(th) * np.sin(ph), radius * np.cos(th), radius * np.sin(th) * np.cos(ph)], -1)
    fwd = -_normalize(off)
    up0 = np.broadcast_to(np.array([0.0, -1.0, 0.0]), fwd.shape)
    right = _normalize(np.cross(fwd, up0))
    up = _normalize(np.cross(right, fwd))
    poses = np.tile(np.eye(4), (th.shape[0], 1, 1))
    poses[:, :3, :3] = np.stack([right, up, fwd], -1)
    poses[:, :3, 3] = off + (0.0 if look_at is None else np.asarray(look_at, dtype=np.float64))
    return poses


def witness_rays_d(poses, intrinsics, rH, rW):
    """[B, rH * rW, 3] float64: the ray directions of every pixel, row-major; the intrinsics as fp32 (what both routes use)"""
    fx, fy, cx, cy = [np.float64(np.float32(v)) for v in intrinsics]
    pix = np.arange(rH * rW)
    i, j = (pix % rW) + 0.5, (pix // rW) + 0.5
    d = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones_like(i)], -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return d[None] @ np.transpose(np.asarray(poses, dtype=np.float64)[:, :3, :3], (0, 2, 1))


def scaled_pose_error(poses, witness, radius):
    """largest absolute deviation of [B, 4, 4] poses from the witness, translations divided by the radius"""
    d = np.abs(np.asarray(poses, dtype=np.float64) - witness)
    d[:, :3, 3] /= float(radius)
    return float(d.max())


def reference_deviation(G):
    """the reference's own fp32 error over the fixture (see the module docstring)"""
    dev = 0.0
    W = {}
    for tag in POSE_CASES:
        W[tag] = witness_poses(G[f"{tag}_thetas"], G[f"{tag}_phis"], G[f"{tag}_radius"])
        dev = max(dev, scaled_pose_error(G[f"{tag}_poses"], W[tag], G[f"{tag}_radius"]))
    for tag, rH, rW in FRAMES:
        key = f"{tag}_{rH}x{rW}"
        dev = max(dev, float(np.abs(G[f"{key}_rays_d"] - witness_rays_d(W[tag], G[f"{key}_intrinsics"], rH, rW)).max()))
    return dev


def device_tolerance(G):
    return max(4.0 * reference_deviation(G), FLOOR)
