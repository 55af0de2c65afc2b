"""Float64 / numpy witnesses of the interactive preview (nerf/preview.py, csrc/preview.hip) and the tolerances derived from them.

Camera.  `witness_camera` replays the fixture's script (tools/gen_preview_golden.py) with float64 rotation matrices (Rodrigues
for the rotation vectors, no quaternion, no scipy) and float64 translations.  The reference's float32 poses deviate from it by
`camera_reference_deviation(G)`: measured 2.19e-07 over the fixture (entries of the matrix; the translations are of order 1 to 3), which
is float32 rounding of a handful of products.  The bound the issue sets for the build's camera against the fixture is 1e-6.

sRGB.  `linear_to_srgb_f64` is the conversion in float64.  The `linear` route of s3d_preview_resolve is compared with the torch
fp32 sequence on the same inputs; its bound is the error that sequence itself has against this witness, times the margin the
project gives its fp32 transcendental kernels (tests/custom_pose_witness.py: four times the reference's own error, never less
than 2e-6): `linear_tolerance(x)`.  Measured on the CPU over the fixture's colours and a ramp of [0, 1.5] the torch sequence is within 1.48e-07 of the witness,
so the bound is the 2e-6 floor; the GPU test measures it again on its own inputs and prints it.

Frame preparation.  `prepare_numpy` / `accumulate_numpy` are the numpy expressions of NeRFGUI.prepare_buffer / test_step
themselves (float32 arrays, Python scalars): what the torch route and the kernel must reproduce bit for bit."""
import os

import numpy as np

from conftest import GOLDEN

MARGIN, FLOOR = 4.0, 2e-6  # tests/custom_pose_witness.py


def load():
    return np.load(os.path.join(GOLDEN, "preview.npz"))


def _rodrigues(v):
    v = np.asarray(v, dtype=np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def witness_camera(G):
    """poses [n + 1, 4, 4] and intrinsics [n + 1, 4] in float64 after each call of the fixture's script"""
    W, H, radius, fovy = G["cam_init"]
    R, center = np.diag([1.0, -1.0, -1.0]), np.zeros(3)
    up = np.array([0.0, 1.0, 0.0])

    def pose():
        m = np.eye(4)
        m[:3, :3] = R
        m[:3, 3] = R @ np.array([0.0, 0.0, -radius]) - center
        return m

    def intr():
        f = H / (2 * np.tan(np.radians(fovy) / 2))
        return np.array([f, f, W // 2, H // 2])
    poses, intrs = [pose()], [intr()]
    for op, args in zip(G["cam_ops"], G["cam_args"]):
        if op == "orbit":
            side = R[:, 0]
            R = _rodrigues(up * np.radians(-0.1 * args[0])) @ _rodrigues(side * np.radians(-0.1 * args[1])) @ R
        elif op == "scale":
            radius = radius * 1.1 ** (-args[0])
        elif op == "pan":
            center = center + 0.0005 * R @ args
        elif op == "set_pose":
            m = G["cam_set_pose"].astype(np.float64)
            u, _, vt = np.linalg.svd(m[:3, :3])  # (the nearest rotation of the float32 matrix)
            center = m[:3, :3] @ np.array([0.0, 0.0, -radius]) - m[:3, 3]
            R = u @ vt
        elif op == "set_intrinsics":
            fovy = 2 * np.degrees(np.arctan(H / (2 * G["cam_set_intrinsics"][0])))
        else:
            raise ValueError(op)
        poses.append(pose())
        intrs.append(intr())
    return np.stack(poses), np.stack(intrs)


def camera_reference_deviation(G):
    poses, intrs = witness_camera(G)
    return float(np.abs(G["cam_poses"] - poses).max()), float(np.abs(G["cam_intrinsics"] / intrs - 1).max())


def linear_to_srgb_f64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x < 0.0031308, 12.92 * x, 1.055 * np.abs(x) ** 0.41666 - 0.055)


def linear_tolerance(x_f32, torch_result):
    """bound of the device's `linear` route against the torch route on the colours x: MARGIN x the torch fp32 sequence's own
    error against the float64 witness, at least FLOOR.  Returns (bound, that error)."""
    own = float(np.abs(np.asarray(torch_result, dtype=np.float64) - linear_to_srgb_f64(x_f32)).max())
    return max(MARGIN * own, FLOOR), own


def mix_brush_numpy(img, masks, color, alpha=1.0):
    """SealNeRF/gui.py:221-223, masks [K, H, W] uint8"""
    mask = np.sum(masks[..., None], axis=0)
    return np.where(mask > 0, color[np.newaxis, np.newaxis, :] * alpha + img * (1 - alpha), img)


def prepare_numpy(image, depth, mode, masks, color, alpha=1.0):
    out = image if mode == "image" else np.expand_dims(depth / (depth.max() + 1e-6), -1).repeat(3, -1)
    return mix_brush_numpy(out, masks, color, alpha) if masks is not None and len(masks) else out


def accumulate_numpy(buffer, prepared, spp):
    return prepared if spp == 0 else (buffer * spp + prepared) / (spp + 1)


def nearest_index(out, inp):
    """source index of every destination index: torch's rule in float32"""
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)
