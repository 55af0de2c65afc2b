"""CPU: the brush and anchor tools (sealnerf/seal_utils.py: SealBrushMapper, SealAnchorMapper, torch op sequence) against
tests/golden/seal_tools.npz — the outputs of the REFERENCE's `map_to_origin` (SealNeRF/seal_utils.py:408-453, 514-570, with
map_mask, points_in_mesh, project_points and torch.cdist under it) and `mesh_surface_points_mask` (:712-725) executed on the
build's constants (tools/gen_seal_tools_golden.py).  Not pinned, only restated: the plane fit (skspatial), the oriented box
and the uv-sphere vertices (trimesh); they are checked here by known answers."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN

BRUSH = ["brush_linear1", "brush_linear2", "brush_dry"]
ANCHOR = ["anchor_mixed", "anchor_scale", "anchor_axis"]


@pytest.fixture(scope="module")
def S():
    return np.load(os.path.join(GOLDEN, "seal_tools.npz"))


def config(S, tag):
    return json.loads(str(S[f"{tag}_config"]))


def batches(S, tag):
    return sorted(m.group(1) for m in (re.match(rf"{tag}_b(\d+)_points$", k) for k in S.files) if m)


@pytest.mark.parametrize("tag", BRUSH + ANCHOR)
def test_get_seal_mapper_builds_the_tool(S, tag):
    from sealnerf import SealAnchorMapper, SealBrushMapper, get_seal_mapper
    cfg = config(S, tag)
    m = get_seal_mapper(cfg)
    assert isinstance(m, SealBrushMapper if cfg["type"] == "brush" else SealAnchorMapper)
    # the constants the reference ran on are what the constructor builds
    assert np.array_equal(m.map_triangles.numpy(), S[f"{tag}_triangles"])
    assert np.array_equal(m.map_data["map_bound"].numpy(), S[f"{tag}_map_bound"])


def test_map_data_keys_and_shapes(S):
    from sealnerf import get_seal_mapper
    b = get_seal_mapper(config(S, "brush_linear2"))
    md = b.map_data
    assert set(md) == {"force_fill_bound", "map_bound", "normal_expand", "center", "border_points", "attenuation_distance",
                       "attenuation_mode"}
    assert md["force_fill_bound"].shape == (2, 2, 3) and md["map_bound"].shape == (2, 2, 3)
    assert md["force_fill_bound"].data_ptr() != md["map_bound"].data_ptr()  # (init_mapper clamps the fill bound in place)
    assert md["normal_expand"].shape == (3,) and md["center"].shape == (3,) and md["attenuation_distance"].shape == ()
    assert md["border_points"].ndim == 2 and md["border_points"].shape[1] == 3
    assert b.map_triangles.shape == (24, 3, 3) and torch.equal(b.map_test_dir, md["normal_expand"][None])
    # normal_expand and center are those of the LAST stroke
    last = np.asarray(config(S, "brush_linear2")["raw"][1])
    assert np.allclose(md["center"].numpy(), last.mean(0), atol=1e-7)
    a = get_seal_mapper(config(S, "anchor_mixed"))
    md = a.map_data
    assert {"force_fill_bound", "map_bound", "pose_center", "pose_radius", "v_anchor", "v_offset", "v_h", "len_h", "radius",
            "scale", "map_source"} <= set(md)
    assert md["map_bound"].shape == (2, 3) and md["map_source"] is True and a.map_test_dir is None
    assert a.map_triangles.shape == (12, 3, 3)


def test_plane_fit_and_oriented_box_known_answers():
    from sealnerf.seal_utils import SealBrushMapper, fit_plane, oriented_box_vertices, uv_sphere_vertices
    pts = np.array([[-0.2, 0.3, -0.05], [0.2, 0.3, -0.05], [0.2, 0.3, 0.2], [-0.2, 0.3, 0.2], [0.05, 0.3, 0.1]])  # y = 0.3
    n, c = fit_plane(pts)
    assert np.allclose(np.abs(n), [0, 1, 0]) and np.allclose(c, pts.mean(0))
    with pytest.raises(ValueError):
        fit_plane([[0, 0, 0], [1, 1, 1], [2, 2, 2]])
    for sign in (1, -1):
        m = SealBrushMapper(dict(type="brush", raw=pts.tolist(), normal=[0, sign, 0], brushType="line", brushDepth=2.0,
                                 brushPressure=0.1, attenuationDistance=0.05, attenuationMode="linear"))
        assert np.allclose(m.map_data["normal_expand"].numpy(), [0, 0.1 * sign, 0], atol=1e-7)
        # the box spans the stroke from 2 * pressure above the plane to brushDepth * pressure below it, along the normal
        lo, hi = m.map_data["map_bound"][0].numpy()
        assert np.allclose([lo[1], hi[1]], sorted([0.3 + 0.2 * sign, 0.3 - 0.2 * sign]), atol=1e-6)
        assert np.allclose([lo[0], hi[0], lo[2], hi[2]], [-0.2, 0.2, -0.05, 0.2], atol=1e-6)
    # a rotated box's corners come back as its corners
    R = np.array([[np.cos(0.5), -np.sin(0.5), 0], [np.sin(0.5), np.cos(0.5), 0], [0, 0, 1]])
    box = np.array([[x, y, z] for x in (0, 0.4) for y in (0, 0.2) for z in (0, 0.1)]) @ R.T
    v = oriented_box_vertices(box)
    assert np.abs(v[:, None] - box[None]).sum(-1).min(1).max() < 1e-9
    # uv sphere: 32 x 64 grid with the poles merged, every vertex on the sphere
    s = uv_sphere_vertices(0.5)
    assert s.shape == (30 * 64 + 2, 3) and np.allclose(np.linalg.norm(s, axis=1), 0.5)


@pytest.mark.parametrize("tag", BRUSH)
def test_border_points_match_reference_execution(S, tag):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(config(S, tag))
    ref = np.concatenate([S[f"{tag}_stroke{s}_projected"][S[f"{tag}_stroke{s}_border_mask"]]
                          for s in range(len([k for k in S.files if k.startswith(f"{tag}_stroke") and k.endswith("_projected")]))])
    assert np.array_equal(m.map_data["border_points"].numpy(), ref.astype(np.float32))
    assert np.array_equal(m.map_data["border_points"].numpy(), S[f"{tag}_border_points"])


@pytest.mark.parametrize("tag", BRUSH + ANCHOR)
def test_torch_mapper_matches_reference_execution(S, tag):
    """same torch op sequence on the same CPU: masks, mapped points and untouched rows bit-exact"""
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(config(S, tag))
    for b in batches(S, tag):
        pts = torch.from_numpy(S[f"{tag}_b{b}_points"])
        dirs = torch.nn.functional.normalize(torch.randn(pts.shape[0], 3), dim=-1)
        p, d, mask = m.map_to_origin(pts.clone(), dirs)
        assert d is dirs
        assert torch.equal(mask, torch.from_numpy(S[f"{tag}_b{b}_mask"]))
        assert np.array_equal(p[mask].numpy(), S[f"{tag}_b{b}_mapped"])
        assert torch.equal(p[~mask], pts[~mask])


def test_anchor_early_exit_batches(S):
    """the anchor's batch-wide quirk: cone points with x == 0 alone fail `points.all(1)` -> unchanged, mask all false; with one
    in-box point added, every one of them is mapped"""
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(config(S, "anchor_axis"))
    p0 = torch.from_numpy(S["anchor_axis_b0_points"])
    assert (p0[:, 0] == 0).all()
    out, _, mask = m.map_to_origin(p0)
    assert not mask.any() and torch.equal(out, p0)
    p1 = torch.from_numpy(S["anchor_axis_b1_points"])
    out, _, mask = m.map_to_origin(p1)
    assert mask[:-1].all() and not torch.equal(out[:-1], p0)


def test_colour_options_reach_map_color(S):
    from sealnerf import get_seal_mapper
    from sealnerf.seal_utils import modify_hsv, modify_rgb
    cfg = dict(config(S, "brush_linear1"), hsv=[0.1, -0.05, 0.02], rgb=[0.8, 0.2, 0.1], rgbLightOffset=0.05)
    m = get_seal_mapper(cfg)
    assert m.map_data["rgb_light_offset"] == 0.05
    cols = torch.rand(100, 3, generator=torch.Generator().manual_seed(0))
    want = modify_rgb(modify_hsv(cols, torch.tensor(cfg["hsv"])), torch.tensor(cfg["rgb"]), 0.05)
    assert torch.equal(m.map_color(None, None, cols), want)
    a = get_seal_mapper(dict(config(S, "anchor_mixed"), hsv=[0.2, 0, 0]))
    assert not torch.equal(a.map_color(None, None, cols), cols)


@pytest.mark.parametrize("change", [dict(brushType="curve"), dict(attenuationMode="ease-in"), dict(attenuationMode="ease-out"),
                                    dict(imageConfig={"path": "x.png", "o": [0, 0, 0], "w": [1, 0, 0], "h": [0, 1, 0]})])
def test_unsupported_options_raise(S, change):
    from sealnerf import get_seal_mapper
    with pytest.raises(NotImplementedError):
        get_seal_mapper(dict(config(S, "brush_linear1"), **change))
