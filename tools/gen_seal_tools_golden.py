#!/usr/bin/env python3
"""Generate tests/golden/seal_tools.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the brush and anchor tools of SealNeRF/seal_utils.py the way oracle/gen_golden.py `seal` pins the bbox tool: the
reference mappers are created with `__new__` (their trimesh / pytorch3d / skspatial constructors cannot run here), the
build's float32 constants are injected, and the reference's own `map_to_origin` (with `map_mask`, `points_in_mesh`,
`moller_trumbore`, `project_points` and `torch.cdist` under it) is EXECUTED on seeded points.  The reference's
`mesh_surface_points_mask` is executed on the build's stroke triangles and projected stroke points, which pins the border
selection.  What stays a restatement (not pinned): the plane fit, the oriented box, the uv-sphere vertex set.

Every point whose float64 margin to a threshold of its tool (box faces and AABB, attenuation distance, cone and plane side)
is below 1e-5 is dropped, so the masks can be required to match exactly on any device.  Stored per case: the config (JSON),
the constants the reference ran on, the inputs, the mask and the mapped rows of the mask (the other rows are the inputs).

    python tools/gen_seal_tools_golden.py     (re-running reproduces the file bit for bit)
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

OUT = os.path.join(REPO, "tests", "golden", "seal_tools.npz")
MARGIN = 1e-5


def _stroke(n, x0, x1, y, z0, tilt, wave, seed):
    g = np.random.default_rng(seed)
    x = np.linspace(x0, x1, n)
    z = z0 + wave * np.sin(x * 9.0) + g.uniform(-0.01, 0.01, n)
    return np.stack([x, y + tilt * x + g.uniform(-0.002, 0.002, n), z], 1).round(4).tolist()


def _anchor_raw(c, r, seed):
    g = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, 8, endpoint=False)
    pts = np.stack([c[0] + r * np.cos(a), c[1] + 0.03 * np.cos(a) + g.uniform(-0.002, 0.002, 8), c[2] + r * np.sin(a)], 1)
    return pts.round(4)


_AX = _anchor_raw([0.0, 0.05, 0.12], 0.06, 3)
_AX[:, 0] = np.array([0.06, 0.0424, 0.0, -0.0424, -0.06, -0.0424, 0.0, 0.0424])  # symmetric in x: the anchor lies on x = 0

CASES = {
    "brush_linear1": dict(type="brush", raw=_stroke(24, -0.25, 0.25, 0.3, 0.05, 0.08, 0.08, 0), normal=[0, 1, 0],
                          brushType="line", brushDepth=1.0, brushPressure=0.05, attenuationDistance=0.08,
                          attenuationMode="linear"),
    "brush_linear2": dict(type="brush", raw=[_stroke(20, -0.3, 0.1, 0.2, -0.2, 0.05, 0.06, 1),
                                             _stroke(16, -0.1, 0.3, 0.22, 0.15, 0.05, 0.05, 2)],
                          normal=[0, 1, 0], brushType=["line", "line"], brushDepth=0.8, brushPressure=-0.04,
                          attenuationDistance=0.06, attenuationMode="linear"),
    "brush_dry": dict(type="brush", raw=_stroke(24, -0.2, 0.3, -0.1, 0.1, -0.1, 0.07, 4), normal=[0, -1, 0], brushType="line",
                      brushDepth=0.5, brushPressure=0.06, attenuationDistance=0.05, attenuationMode="dry",
                      hsv=[0.1, 0.0, -0.05]),
    "anchor_mixed": dict(type="anchor", raw=_anchor_raw([0.15, 0.1, -0.1], 0.07, 5).tolist(), translation=[0.04, 0.12, -0.03],
                         radius=0.1, scale=[1, 1, 1]),
    "anchor_scale": dict(type="anchor", raw=_anchor_raw([-0.2, -0.1, 0.2], 0.06, 6).tolist(), translation=[-0.02, 0.1, 0.03],
                         radius=0.09, scale=[1.2, 0.8, 1.1]),
    "anchor_axis": dict(type="anchor", raw=_AX.tolist(), translation=[0.03, 0.12, 0.0], radius=0.1, scale=[1, 1, 1]),
}


def _load_build():
    spec = importlib.util.spec_from_file_location("s3d_seal_utils", os.path.join(REPO, "seal-3d_amd", "sealnerf", "seal_utils.py"))
    mine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mine)
    return mine


def _box_margin(p, tris, bounds):
    """float64 distance of each point to the nearest triangle plane and AABB face (the inside test's and pre-test's edges)"""
    t = tris.astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    plane = np.abs(np.einsum("pfd,fd->pf", p[:, None, :] - t[None, :, 0], n))
    b = bounds.reshape(-1, 2, 3).astype(np.float64)
    face = np.abs(p[:, None, None, :] - b[None]).reshape(p.shape[0], -1)
    return np.minimum(plane.min(1), face.min(1))


def _brush_margin(p, mb):
    md = {k: (v.double().numpy() if torch.is_tensor(v) else v) for k, v in mb.map_data.items()}
    m = _box_margin(p, mb.map_triangles.numpy(), md["map_bound"])
    if md["attenuation_mode"] == "linear":
        ne, c = md["normal_expand"], md["center"]
        q = p - ((p - c) @ ne / (ne @ ne))[:, None] * ne
        d = np.sqrt(((q[:, None, :] - md["border_points"][None]) ** 2).sum(-1)).min(1)
        m = np.minimum(m, np.abs(d - float(md["attenuation_distance"])))
    return m


def _anchor_margin(p, mb):
    md = {k: (v.double().numpy() if torch.is_tensor(v) else v) for k, v in mb.map_data.items()}
    h, a, len_h, r = md["v_h"], md["v_anchor"], float(md["len_h"]), float(md["radius"])
    j = p - ((p - a) @ h / (h @ h))[:, None] * h
    tp = j - p
    dist = np.linalg.norm(tp, axis=1)
    q = j - (dist / len_h)[:, None] * md["v_offset"]
    ad = np.linalg.norm(q - a, axis=1)
    cone = np.abs(dist - len_h / r * 1.1 * (r - ad))
    return np.minimum.reduce([_box_margin(p, mb.map_triangles.numpy(), md["map_bound"]), np.abs(ad - r), cone,
                              np.abs(tp @ h) / np.linalg.norm(h)])


def _reference(su, mb, cls):
    ref = cls.__new__(cls)  # no trimesh / pytorch3d / skspatial constructor: constants from the build
    su.SealMapper.__init__(ref, mb.config)
    ref.map_data = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in mb.map_data.items()}
    ref.map_triangles = mb.map_triangles.clone()
    ref.map_test_dir = mb.map_test_dir.clone() if mb.map_test_dir is not None else None
    return ref


def _points(mb, seed, n=6000):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    b = mb.map_data["map_bound"].reshape(-1, 2, 3)
    lo, hi = b[:, 0].min(0).values - 0.03, b[:, 1].max(0).values + 0.03
    pts[n // 2:] = lo + (hi - lo) * torch.rand(n - n // 2, 3, generator=g)  # half of the points around the edit
    pts[:5] = 0.0
    pts[n // 2:n // 2 + 40, 1] = 0.0  # rows with a zero coordinate: outside the map mask whatever else holds
    pts[n // 2 + 40:n // 2 + 80, 2] = 0.0
    return pts


def main():
    _install_reference_stack()
    _stub_training_imports()
    su = importlib.import_module("SealNeRF.seal_utils")
    _assert_reference(su)
    mine = _load_build()
    out = {}
    for ci, (tag, cfg) in enumerate(CASES.items()):
        mb = mine.get_seal_mapper(cfg)
        brush = cfg["type"] == "brush"
        ref = _reference(su, mb, su.SealBrushMapper if brush else su.SealAnchorMapper)
        out[f"{tag}_config"] = np.array(json.dumps(cfg))
        out[f"{tag}_triangles"] = mb.map_triangles.numpy()
        out[f"{tag}_map_bound"] = mb.map_data["map_bound"].numpy()
        if brush:
            # the border selection: the reference's mesh_surface_points_mask on the build's stroke boxes and projected points
            strokes = cfg["raw"] if np.asarray(cfg["raw"][0]).ndim == 2 else [cfg["raw"]]
            border = []
            for s, stroke in enumerate(strokes):
                pts = np.asarray(stroke, dtype=np.float64)
                normal, point = mine.fit_plane(pts)
                if normal @ np.asarray(cfg["normal"], dtype=np.float64) < 0:
                    normal = -normal
                proj = su.project_points(torch.from_numpy(normal), torch.from_numpy(point), torch.from_numpy(pts))
                on = su.mesh_surface_points_mask(mb.map_triangles[12 * s:12 * s + 12].clone(), proj.float())
                out[f"{tag}_stroke{s}_projected"] = proj.numpy()
                out[f"{tag}_stroke{s}_border_mask"] = on.numpy()
                border.append(proj[on])
            border = torch.cat(border).float()
            assert torch.equal(border, mb.map_data["border_points"]), tag
            out[f"{tag}_border_points"] = border.numpy()
            out[f"{tag}_normal_expand"] = mb.map_data["normal_expand"].numpy()
            out[f"{tag}_center"] = mb.map_data["center"].numpy()
        else:
            for k in ("v_anchor", "v_offset", "v_h", "len_h", "radius", "scale"):
                out[f"{tag}_{k}"] = mb.map_data[k].numpy()
        pts = _points(mb, 1000 + ci)
        margin = (_brush_margin if brush else _anchor_margin)(pts.double().numpy(), mb)
        keep = torch.from_numpy(margin >= MARGIN)
        keep[:5] = True  # (the all-zero rows are outside whatever their margins)
        pts = pts[keep].contiguous()
        batches = [pts]
        if tag == "anchor_axis":
            # batch 0: cone points with x == 0 only -> no point passes `points.all(1)`, the reference returns the batch
            # unchanged with an all-false mask; batch 1: the same plus one point inside the box -> all of them are mapped
            cand = _points(mb, 77, 40000)[20000:]
            cand[:, 0] = 0.0
            cm = _anchor_margin(cand.double().numpy(), mb)
            inside = (mb.map_data["v_anchor"] + 0.5 * torch.tensor(cfg["translation"]))[None]  # halfway to the moved anchor
            assert bool(ref.map_mask(inside.clone())[0]) and _anchor_margin(inside.double().numpy(), mb)[0] >= MARGIN
            _, _, m_ = ref.map_to_origin(torch.cat([cand, inside]))
            sel = m_[:-1] & torch.from_numpy(cm >= MARGIN)
            cone = cand[sel][:64].contiguous()
            assert cone.shape[0] >= 32, cone.shape
            batches = [cone, torch.cat([cone, inside]), pts]
        for b, bp in enumerate(batches):
            key = f"{tag}_b{b}"
            p, d, m = ref.map_to_origin(bp.clone())
            dirs = torch.nn.functional.normalize(torch.randn(bp.shape[0], 3, generator=torch.Generator().manual_seed(b)), dim=-1)
            p2, d2, m2 = ref.map_to_origin(bp.clone(), dirs)
            assert torch.equal(m, m2) and torch.equal(p, p2) and d2 is dirs
            assert torch.equal(p[~m], bp[~m]), key
            out[f"{key}_points"] = bp.numpy()
            out[f"{key}_mask"] = m.numpy()
            out[f"{key}_mapped"] = p[m].numpy()
            print(f"{key}: {int(m.sum())} of {bp.shape[0]} points mapped")
        if tag == "anchor_axis":
            assert not out[f"{tag}_b0_mask"].any() and out[f"{tag}_b1_mask"][:-1].all()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
