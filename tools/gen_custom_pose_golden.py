#!/usr/bin/env python3
"""Generate tests/golden/custom_pose.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the parts of the reference's custom-pose provider (SealNeRF/provider.py:145-178) that run — `rand_poses`
(nerf/provider.py:57-91, without `look_at`) and `get_rays(poses, intrinsics, rH, rW, -1)` (nerf/utils.py:54-139) — by
EXECUTING them on the CPU under torch.manual_seed:

  (a) B = 1, radius 1, default ranges;
  (b) B = 3, radius 2.5, theta_range (0.3, 2.6), phi_range (0.5, 4.0) — away from the poles, where forward || up0 degenerates;
  (c) the frames of (a)'s pose at 5 x 7 and at 67 x 131, intrinsics of an 800 x 800 frame scaled as the provider scales
      them, and the frames of (b)'s poses at 5 x 7;
  (d) the uniforms of each case (the same two torch.rand draws under the same seed) and the theta, phi they give.

    python tools/gen_custom_pose_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import _assert_reference, _install_reference_stack, _load_synthetic, _stub_training_imports  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "custom_pose.npz")

CASES = (("a", 1, 1.0, (np.pi / 3, 2 * np.pi / 3), (0, 2 * np.pi), 31),
         ("b", 3, 2.5, (0.3, 2.6), (0.5, 4.0), 32))
FRAMES = (("a", 5, 7), ("a", 67, 131), ("b", 5, 7))
FULL = 800  # the frames are down-scaled views of an 800 x 800 camera


def main():
    _install_reference_stack()
    _stub_training_imports()
    m = sys.modules.get("cv2") or types.ModuleType("cv2")
    if not hasattr(m, "transform"):
        m.transform = None
    sys.modules["cv2"] = m
    utils = importlib.import_module("nerf.utils")
    provider = importlib.import_module("nerf.provider")
    for m_ in (utils, provider):
        _assert_reference(m_)
    syn = _load_synthetic()
    out, poses = {}, {}
    for tag, B, radius, tr, pr, seed in CASES:
        torch.manual_seed(seed)
        p = provider.rand_poses(B, "cpu", radius=radius, theta_range=list(tr), phi_range=list(pr))
        torch.manual_seed(seed)  # (d): the two draws rand_poses made, in its order, and its two expressions
        u_t, u_p = torch.rand(B), torch.rand(B)
        thetas = u_t * (tr[1] - tr[0]) + tr[0]
        phis = u_p * (pr[1] - pr[0]) + pr[0]
        poses[tag] = p
        out.update({f"{tag}_poses": p.numpy(), f"{tag}_seed": np.int64(seed), f"{tag}_radius": np.float64(radius),
                    f"{tag}_theta_range": np.array(tr, dtype=np.float64), f"{tag}_phi_range": np.array(pr, dtype=np.float64),
                    f"{tag}_u": torch.stack([u_t, u_p], -1).numpy(), f"{tag}_thetas": thetas.numpy(), f"{tag}_phis": phis.numpy()})
    for tag, rH, rW in FRAMES:
        s = np.sqrt(FULL * FULL / (rH * rW))  # (any scale will do: the frame is rH x rW by construction)
        intr = syn.lego_intrinsics(FULL, FULL) / s
        r = utils.get_rays(poses[tag], intr, rH, rW, -1)
        key = f"{tag}_{rH}x{rW}"
        out.update({f"{key}_intrinsics": np.asarray(intr, dtype=np.float64), f"{key}_rays_o": r["rays_o"].contiguous().numpy(),
                    f"{key}_rays_d": r["rays_d"].contiguous().numpy()})
    # fixed zip timestamps: a re-run writes the same bytes
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, b.getvalue())
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("custom_pose: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
