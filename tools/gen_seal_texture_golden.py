#!/usr/bin/env python3
"""Generate tests/golden/seal_texture.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the brush tool's texture painting (`imageConfig`; SealNeRF/seal_utils.py:58-79 the `image` step of map_color, :753-769
modify_rgb with a per-sample target) the way tools/gen_seal_tools_golden.py pins the brush and anchor mappings: a reference
`SealBrushMapper` is created with `__new__` (its cv2 / skspatial constructor cannot run here), the build's float32 constants
are injected through the reference's own `map_data_conversion(force=True)`, and the reference's `SealMapper.map_color` is
EXECUTED on seeded points and colours.  The reference's texel indices are recorded by wrapping its `modify_rgb` for the call
(the per-sample target it receives is `image[idx_h, idx_w]`; the texture's texels are distinct, so the target names the texel).
What stays a restatement (not pinned): the plane fit of the quad's normal (skspatial), the decoding of an image file (cv2).

`floor` makes the lookup discontinuous: every point within MARGIN = 1e-4 texel of an integer texel coordinate on either axis
(computed in float64) is dropped, so the indices can be required to match exactly on any device.  That is about ten times the
float32 error of the coordinate (1e-7 in position x W / |ow| ~ 128 = 1e-5 texel).  The dropped share is printed and must not
exceed 0.5 % (expected for uniformly spread points: 2 axes x 2 MARGIN = 4e-4).

One set of 20,000 points and colours serves every case.  The reference's float32 outputs do not compress (12 bytes per row and
case), so only the first case (`image`) is run on all kept points; the three other option sets (`hsv`; `hsv` + `rgb` + light
offset; no alpha channel) are run on the first ROWS_MORE = 5,000 of them — the same quad and points, hence the same texels, and
every special colour row (they come first); their batch means are those of these 5,000 rows.  That keeps the file under the
size limit for a committed file (asserted).

    python tools/gen_seal_texture_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import _assert_reference, _install_reference_stack, _stub_training_imports  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "seal_texture.npz")
ROWS_MORE = 5000    # rows of the cases after the first
MARGIN = 1e-4       # texels
MAX_DROPPED = 0.005
H, W = 48, 64
N = 20000
QUAD = dict(o=[-0.2, 0.3, -0.1], w=[0.25, 0.32, -0.1], h=[-0.2, 0.28, 0.25])  # tilted: no edge along a coordinate axis


def _stroke():
    x = np.linspace(-0.25, 0.25, 24)
    return np.stack([x, 0.3 + 0.08 * x, 0.05 + 0.08 * np.sin(9 * x)], 1).round(4).tolist()


BRUSH = dict(type="brush", raw=_stroke(), normal=[0, 1, 0], brushType="line", brushDepth=1.0, brushPressure=0.05,
             attenuationDistance=0.08, attenuationMode="dry")


def texture(alpha=True):
    """seeded uint8 texels, all distinct in RGB; alpha rows 0..7 = 0, rows 8..15 = 1, the rest random"""
    g = np.random.default_rng(7)
    rgb = g.permutation(1 << 24)[:H * W]
    px = np.stack([rgb >> 16, (rgb >> 8) & 255, rgb & 255], -1).reshape(H, W, 3).astype(np.uint8)
    px[20, :8] = np.array([[90, 90, 90], [0, 0, 0], [255, 255, 255], [200, 0, 0], [0, 200, 0], [0, 0, 200], [180, 180, 40],
                           [40, 180, 180]], dtype=np.uint8)  # grey, black, white, pure channels, channel ties
    assert len({tuple(t) for t in px.reshape(-1, 3)}) == H * W
    if not alpha:
        return px
    a = g.integers(0, 256, (H, W)).astype(np.uint8)
    a[:8] = 0
    a[8:16] = 255
    return np.concatenate([px, a[..., None]], -1)


CASES = {
    "image": dict(alpha=True),
    "image_hsv": dict(alpha=True, hsv=[0.1, -0.05, 0.02]),
    "image_rgb_hsv_light": dict(alpha=True, hsv=[-0.07, 0.04, -0.03], rgb=[0.8, 0.2, 0.1], rgbLightOffset=0.05),
    "image_opaque": dict(alpha=False, rgbLightOffset=-0.02),
}


def _load_build():
    spec = importlib.util.spec_from_file_location("s3d_seal_utils", os.path.join(REPO, "seal-3d_amd", "sealnerf", "seal_utils.py"))
    mine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mine)
    return mine


def _inputs(seed):
    """points in a slab around the quad that is larger than it (about half project outside), colours with the special rows
    of seal_bbox.npz's colour cases: greys, black / white, pure channels, channel ties"""
    g = np.random.default_rng(seed)
    pts = np.stack([g.uniform(-0.29, 0.345, N), g.uniform(0.2, 0.4, N), g.uniform(-0.17, 0.325, N)], 1).astype(np.float32)
    cols = g.uniform(0, 1, (N, 3)).astype(np.float32)
    cols[:8] = np.array([[0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1], [0.7, 0, 0], [0, 0.7, 0], [0, 0, 0.7], [0.6, 0.6, 0.2], [0.2, 0.6, 0.6]],
                        dtype=np.float32)
    cols[8:200, 1] = cols[8:200, 0]          # r == g
    cols[200:400, 2] = cols[200:400, 1]      # g == b
    cols[400:600] = cols[400:600, :1]        # greys
    return pts, cols


def texel_coordinates(pts):
    """float64 texel coordinates (along w, along h) of float32 points"""
    o, w, h = (np.asarray(QUAD[k], dtype=np.float64) for k in "owh")
    n = np.cross(w - o, h - o)
    n /= np.linalg.norm(n)
    p = pts.astype(np.float64)
    vp = p - ((p - o) @ n)[:, None] * n - o
    return vp @ (w - o) / np.dot(w - o, w - o) * W, vp @ (h - o) / np.dot(h - o, h - o) * H


def main():
    _install_reference_stack()
    _stub_training_imports()
    su = importlib.import_module("SealNeRF.seal_utils")
    _assert_reference(su)
    mine = _load_build()
    out = {"quad": np.array(json.dumps(QUAD)), "brush": np.array(json.dumps(BRUSH)), "pixels_rgba": texture(True),
           "pixels_rgb": texture(False)}
    pts, cols = _inputs(2000)
    cw, ch = texel_coordinates(pts)
    near = (np.abs(cw - np.round(cw)) < MARGIN) | (np.abs(ch - np.round(ch)) < MARGIN)
    dropped = float(near.mean())
    inside = float(((cw > 0) & (cw < W) & (ch > 0) & (ch < H)).mean())
    print(f"{int((~near).sum())} of {N} points kept: dropped share {dropped:.5f} (cap {MAX_DROPPED}); inside the quad {inside:.3f}")
    assert dropped <= MAX_DROPPED, dropped
    pts, cols, cw, ch = pts[~near], cols[~near], cw[~near], ch[~near]
    out["points"], out["colors"] = pts, cols
    all_pts, all_cols, all_cw, all_ch = pts, cols, cw, ch
    for ci, (tag, case) in enumerate(CASES.items()):
        case = dict(case)
        rows = all_pts.shape[0] if ci == 0 else ROWS_MORE
        pts, cols, cw, ch = all_pts[:rows], all_cols[:rows], all_cw[:rows], all_ch[:rows]
        pixels = texture(case.pop("alpha"))
        mb = mine.get_seal_mapper(dict(BRUSH, imageConfig=dict(QUAD, pixels=pixels), **case))
        ref = su.SealBrushMapper.__new__(su.SealBrushMapper)  # no cv2 / skspatial constructor: constants from the build
        su.SealMapper.__init__(ref, mb.config)
        keys = ["image", "image_mask", "v_image_norm", "v_image_o", "v_image_w", "v_image_h", "rgb_light_offset"] + \
               [k for k in ("hsv", "rgb") if k in case]
        ref.map_data = {k: (mb.map_data[k].numpy().copy() if torch.is_tensor(mb.map_data[k]) else mb.map_data[k]) for k in keys}
        ref.map_data_conversion(force=True)
        for k in keys:
            if torch.is_tensor(mb.map_data[k]):  # the reference runs on the build's bits
                assert ref.map_data[k].dtype == torch.float32 and torch.equal(ref.map_data[k], mb.map_data[k]), k
        # the reference's texel indices: the per-sample target its modify_rgb receives for the `image` step
        seen = []
        real = su.modify_rgb

        def spy(rgb, modification, light_offset=0):
            seen.append(modification.clone())
            return real(rgb, modification, light_offset)
        su.modify_rgb = spy
        try:
            res = ref.map_color(torch.from_numpy(pts), None, torch.from_numpy(cols).clone())
        finally:
            su.modify_rgb = real
        target = seen[-1]
        assert target.shape == (pts.shape[0], 3) and len(seen) == (2 if "rgb" in case else 1)
        flat = ref.map_data["image"].reshape(-1, 3)
        lut = {tuple(t): i for i, t in enumerate(flat.numpy().view(np.uint32).tolist())}
        idx = np.array([lut[tuple(t)] for t in target.numpy().view(np.uint32).tolist()])
        idx_h, idx_w = (idx // W).astype(np.int16), (idx % W).astype(np.int16)
        # (float64 cross-check of the reference's float32 indices on the kept points)
        assert np.array_equal(idx_w, np.clip(np.floor(cw), 0, W - 1)) and np.array_equal(idx_h, np.clip(np.floor(ch), 0, H - 1)), tag
        if ci == 0:
            out["idx_h"], out["idx_w"] = idx_h, idx_w
        else:  # one quad, one set of points: the same texels in every case
            assert np.array_equal(out["idx_h"][:rows], idx_h) and np.array_equal(out["idx_w"][:rows], idx_w), tag
        out[f"{tag}_options"] = np.array(json.dumps(case))
        for k in keys:
            if k not in ("image", "image_mask"):
                out[f"{tag}_{k}"] = np.asarray(ref.map_data[k].numpy() if torch.is_tensor(ref.map_data[k]) else ref.map_data[k])
        out[f"{tag}_out"] = res.numpy()
        a = ref.map_data["image_mask"][idx_h.astype(np.int64), idx_w.astype(np.int64)]
        print(f"{tag}: {rows} rows, of alpha 0 / alpha 1: {int((a == 0).sum())} / {int((a == 1).sum())}; "
              f"mean |out - in| {float((res - torch.from_numpy(cols)).abs().mean()):.4f}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print(f"wrote {OUT} ({size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
