"""CPU: the brush tool's texture painting (`imageConfig`; sealnerf/seal_utils.py: load_texture, SealBrushMapper, the `image`
step of SealMapper.map_color) against tests/golden/seal_texture.npz — the outputs and texel indices of
the REFERENCE's `map_color` (SealNeRF/seal_utils.py:48-81, with modify_rgb :753-769 under it) executed on the build's float32
constants (tools/gen_seal_texture_golden.py).  Not pinned, only restated: the plane fit of the quad's normal and the decoding
of an image file; they are checked here by known answers."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CASES = ["image", "image_hsv", "image_rgb_hsv_light", "image_opaque"]
IMAGE_KEYS = {"image", "image_mask", "v_image_norm", "v_image_o", "v_image_w", "v_image_h", "rgb_light_offset"}
BRUSH_KEYS = {"force_fill_bound", "map_bound", "normal_expand", "center", "border_points", "attenuation_distance", "attenuation_mode"}


@pytest.fixture(scope="module")
def T():
    return np.load(os.path.join(GOLDEN, "seal_texture.npz"))


def inputs(T, tag):
    """the case's rows: every kept point for `image`, the first 5,000 for the other option sets (same points, same texels)"""
    n = T[f"{tag}_out"].shape[0]
    return T["points"][:n], T["colors"][:n], T["idx_h"][:n], T["idx_w"][:n]


def texture_config(T, tag="image", **image_conf):
    """the golden case's brush config; `image_conf` replaces how the texels are given (default: inline `pixels`)"""
    opts = json.loads(str(T[f"{tag}_options"]))
    conf = dict(json.loads(str(T["quad"])))
    conf.update(image_conf or {"pixels": T["pixels_rgb" if tag == "image_opaque" else "pixels_rgba"]})
    return dict(json.loads(str(T["brush"])), imageConfig=conf, **opts)


def test_inline_pixels_build_the_reference_constants(T):
    from sealnerf import SealBrushMapper, get_seal_mapper
    m = get_seal_mapper(texture_config(T))
    assert isinstance(m, SealBrushMapper)
    md = m.map_data
    assert set(md) == BRUSH_KEYS | IMAGE_KEYS
    px = T["pixels_rgba"]
    H, W = px.shape[:2]
    assert md["image"].shape == (H, W, 3) and md["image"].dtype == torch.float32
    assert md["image_mask"].shape == (H, W) and md["image_mask"].dtype == torch.float32
    assert np.array_equal(md["image"].numpy(), px[:, :, :3].astype(np.float32) / 255)
    assert np.array_equal(md["image_mask"].numpy(), (px[:, :, 3] / 255).astype(np.float32))  # (the reference's float64 division)
    assert (md["image_mask"][:8] == 0).all() and (md["image_mask"][8:16] == 1).all()
    for k in ("v_image_norm", "v_image_o", "v_image_w", "v_image_h"):
        assert md[k].shape == (3,) and md[k].dtype == torch.float32
        assert np.array_equal(md[k].numpy(), T[f"image_{k}"])  # the constants the reference ran on
    assert md["rgb_light_offset"] == 0.0
    # the quad's normal by a known answer: unit, orthogonal to both edges (its sign does not matter)
    q = json.loads(str(T["quad"]))
    o, w, h = (np.asarray(q[k]) for k in "owh")
    n = md["v_image_norm"].double().numpy()
    assert abs(np.linalg.norm(n) - 1) < 1e-6 and abs(n @ (w - o)) < 1e-6 and abs(n @ (h - o)) < 1e-6
    assert get_seal_mapper(texture_config(T, "image_opaque")).map_data["rgb_light_offset"] == -0.02


def test_no_texture_keys_without_image_config(T):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(json.loads(str(T["brush"])))
    assert set(m.map_data) == BRUSH_KEYS


def test_uint8_float_list_and_npy_give_the_same_constants(T, tmp_path):
    from sealnerf import get_seal_mapper
    px = T["pixels_rgba"]
    want = get_seal_mapper(texture_config(T)).map_data
    as_float = px.astype(np.float32) / 255
    np.save(tmp_path / "tex_u8.npy", px)
    np.save(tmp_path / "tex_f32.npy", as_float)
    ways = [dict(pixels=as_float), dict(pixels=as_float.astype(np.float64)), dict(pixels=px.tolist()),
            dict(path=str(tmp_path / "tex_u8.npy")), dict(path=str(tmp_path / "tex_f32.npy"))]
    for way in ways:
        md = get_seal_mapper(texture_config(T, **way)).map_data
        assert set(md) == set(want)
        assert torch.equal(md["image"], want["image"]) and torch.equal(md["image_mask"], want["image_mask"]), list(way)
        assert md["image"].dtype == torch.float32 and md["image"].shape == want["image"].shape


def test_rgb_without_alpha_gives_a_ones_mask(T):
    from sealnerf import get_seal_mapper
    md = get_seal_mapper(texture_config(T, "image_opaque")).map_data
    assert md["image"].shape == T["pixels_rgb"].shape and md["image_mask"].shape == T["pixels_rgb"].shape[:2]
    assert md["image_mask"].dtype == torch.float32 and (md["image_mask"] == 1).all()


def test_grey_and_other_channel_counts_raise_value_error(T, tmp_path):
    from sealnerf import get_seal_mapper
    px = T["pixels_rgba"]
    np.save(tmp_path / "grey.npy", px[:, :, 0])
    for way in (dict(pixels=px[:, :, 0]), dict(pixels=px[:, :, :2]), dict(pixels=np.zeros((4, 4, 5), np.uint8)),
                dict(path=str(tmp_path / "grey.npy")), dict(path="grey.png")):
        with pytest.raises(ValueError):
            get_seal_mapper(texture_config(T, **way), image_loader=lambda path: px[:, :, 0])
    with pytest.raises(ValueError):
        get_seal_mapper(texture_config(T, pixels=np.zeros((4, 4, 3), dtype=bool)))
    for bad in (np.full((4, 4, 3), 256, dtype=np.uint16), np.full((4, 4, 3), -1, dtype=np.int32)):  # integers are 0..255
        with pytest.raises(ValueError):
            get_seal_mapper(texture_config(T, pixels=bad))


def test_encoded_file_needs_a_loader_and_a_missing_file_is_not_that(T, tmp_path):
    from sealnerf import get_seal_mapper
    with pytest.raises(NotImplementedError, match="image_loader") as e:
        get_seal_mapper(texture_config(T, path="stroke.png"))
    assert ".npy" in str(e.value)
    with pytest.raises(FileNotFoundError):  # (a missing file stays a missing file)
        get_seal_mapper(texture_config(T, path=str(tmp_path / "absent.npy")))
    for kind in ("bbox", "anchor"):  # only the brush tool reads imageConfig
        with pytest.raises(NotImplementedError, match="brush"):
            get_seal_mapper(dict(type=kind, imageConfig=texture_config(T)["imageConfig"]))


def test_image_loader_stub_and_pil(T, tmp_path):
    from sealnerf import get_seal_mapper, pil_image_loader
    px = T["pixels_rgba"]
    want = get_seal_mapper(texture_config(T)).map_data
    seen = []

    def stub(path):
        seen.append(path)
        return px
    md = get_seal_mapper(texture_config(T, path="anything.webp"), image_loader=stub).map_data
    assert seen == ["anything.webp"] and torch.equal(md["image"], want["image"]) and torch.equal(md["image_mask"], want["image_mask"])
    from PIL import Image
    Image.fromarray(px, "RGBA").save(tmp_path / "tex.png")
    Image.fromarray(T["pixels_rgb"], "RGB").save(tmp_path / "opaque.png")
    Image.fromarray(px[:, :, 0], "L").save(tmp_path / "grey.png")
    assert np.array_equal(pil_image_loader(str(tmp_path / "tex.png")), px)  # RGBA order, nothing swapped
    md = get_seal_mapper(texture_config(T, path=str(tmp_path / "tex.png")), image_loader=pil_image_loader).map_data
    assert torch.equal(md["image"], want["image"]) and torch.equal(md["image_mask"], want["image_mask"])
    md = get_seal_mapper(texture_config(T, "image_opaque", path=str(tmp_path / "opaque.png")), image_loader=pil_image_loader).map_data
    assert torch.equal(md["image"], want["image"]) and (md["image_mask"] == 1).all()
    with pytest.raises(ValueError):
        get_seal_mapper(texture_config(T, path=str(tmp_path / "grey.png")), image_loader=pil_image_loader)
    # four channels that are not RGBA (CMYK) and grey + alpha are refused by the loader itself
    Image.fromarray(px, "CMYK").save(tmp_path / "cmyk.tif")
    Image.fromarray(px[:, :, :2].copy(), "LA").save(tmp_path / "la.png")
    for name in ("cmyk.tif", "la.png"):
        with pytest.raises(ValueError, match="mode"):
            pil_image_loader(str(tmp_path / name))
    # a palette image is expanded
    Image.fromarray(T["pixels_rgb"], "RGB").quantize(16).save(tmp_path / "pal.png")
    assert pil_image_loader(str(tmp_path / "pal.png")).shape == T["pixels_rgb"].shape
    # a config file on disk, texels beside it as .npy
    np.save(tmp_path / "tex.npy", px)
    cfg = texture_config(T, path=str(tmp_path / "tex.npy"))
    (tmp_path / "seal.json").write_text(json.dumps(cfg))
    md = get_seal_mapper(config_file=str(tmp_path / "seal.json")).map_data
    assert torch.equal(md["image"], want["image"])


@pytest.mark.parametrize("tag", CASES)
def test_twin_matches_reference_execution(T, tag):
    """texel indices exact; colours within the twin tolerance for colour edits (tests/test_seal_golden.py: atol 2e-7)"""
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(texture_config(T, tag))
    pts, cols, want_h, want_w = inputs(T, tag)
    pts, cols = torch.from_numpy(pts), torch.from_numpy(cols)
    assert pts.shape[0] == (T["points"].shape[0] if tag == "image" else 5000) and T["points"].shape[0] > 19900
    idx_h, idx_w = m.texel_indices(pts)
    assert np.array_equal(idx_h.numpy(), want_h) and np.array_equal(idx_w.numpy(), want_w)
    H, W = m.map_data["image"].shape[:2]
    assert {int(idx_h.min()), int(idx_h.max())} == {0, H - 1} and {int(idx_w.min()), int(idx_w.max())} == {0, W - 1}
    keep = cols.clone()
    out = m.map_color(pts, None, cols)
    assert torch.equal(cols, keep)
    err = np.abs(out.numpy() - T[f"{tag}_out"]).max()
    print(tag, "max |twin - reference|", err)
    assert err <= 2e-7
    # alpha 0 leaves the colour of the steps before it, alpha 1 replaces it
    if tag == "image":
        a = m.map_data["image_mask"][idx_h, idx_w]
        assert torch.equal(out[a == 0], cols[a == 0]) and (a == 0).sum() > 1000 and (a == 1).sum() > 1000
        assert not torch.isclose(out[a == 1], cols[a == 1]).all(1).any()


def test_twin_in_float64_and_with_constants_on_another_dtype(T):
    """`map_color` on any dtype: float64 points and colours agree with the float32 reference run to float32 accuracy (the
    indices are those of the kept points: away from every texel edge)"""
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(texture_config(T, "image_hsv"))
    pts, cols, want_h, want_w = inputs(T, "image_hsv")
    pts, cols = torch.from_numpy(pts).double(), torch.from_numpy(cols).double()
    idx_h, idx_w = m.texel_indices(pts)
    assert np.array_equal(idx_h.numpy(), want_h) and np.array_equal(idx_w.numpy(), want_w)
    out = m.map_color(pts, None, cols)
    assert out.dtype == torch.float64
    # (a hue that lands within float32 rounding of a sextant border may take the other branch; both give the same colour)
    assert np.abs(out.numpy() - T["image_hsv_out"]).max() < 5e-6


def test_points_outside_the_quad_take_the_edge_texel(T):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(texture_config(T))
    q = json.loads(str(T["quad"]))
    o, w, h = (torch.tensor(q[k], dtype=torch.float32) for k in "owh")
    n = m.map_data["v_image_norm"]
    H, W = m.map_data["image"].shape[:2]
    uv = torch.tensor([[-0.5, -0.5], [1.5, -0.5], [-0.5, 1.5], [1.5, 1.5], [0.51, 0.51], [0.31, 3.0]])
    pts = o + uv[:, :1] * (w - o) + uv[:, 1:] * (h - o) + 0.3 * n  # (off the plane: the projection brings them back)
    idx_h, idx_w = m.texel_indices(pts)
    # (the quad's edges are 0.3 degrees off a right angle: 3 heights up moves the w coordinate by 0.4 texel)
    assert idx_w.tolist() == [0, W - 1, 0, W - 1, 32, 19] and idx_h.tolist() == [0, 0, H - 1, H - 1, 24, H - 1]


def test_modify_rgb_takes_per_sample_targets():
    from sealnerf.seal_utils import modify_rgb
    g = torch.Generator().manual_seed(0)
    cols, tgt = torch.rand(64, 3, generator=g), torch.rand(64, 3, generator=g)
    per_row = modify_rgb(cols, tgt, 0.03)
    # the batch mean is that of all rows: a row's result is what a single-target call over the same batch gives it
    for i in (0, 17, 63):
        assert torch.equal(per_row[i], modify_rgb(cols, tgt[i], 0.03)[i])


def test_rgb_and_image_together(T):
    """`rgb` then the texture: the second batch mean is taken over the first step's output"""
    from sealnerf import get_seal_mapper
    from sealnerf.seal_utils import modify_hsv, modify_rgb
    tag = "image_rgb_hsv_light"
    m = get_seal_mapper(texture_config(T, tag))
    opts = json.loads(str(T[f"{tag}_options"]))
    assert m.map_data["rgb_light_offset"] == opts["rgbLightOffset"]
    pts, cols = (torch.from_numpy(x) for x in inputs(T, tag)[:2])
    first = modify_rgb(modify_hsv(cols, torch.tensor(opts["hsv"])), torch.tensor(opts["rgb"]), opts["rgbLightOffset"])
    idx_h, idx_w = m.texel_indices(pts)
    a = m.map_data["image_mask"][idx_h, idx_w][:, None]
    want = a * modify_rgb(first, m.map_data["image"][idx_h, idx_w], opts["rgbLightOffset"]) + (1 - a) * first
    assert torch.equal(m.map_color(pts, None, cols), want)
    assert np.abs(want.numpy() - T[f"{tag}_out"]).max() <= 2e-7


@pytest.mark.parametrize("tag", ["image_hsv", "image_rgb_hsv_light"])
def test_map_color_masked_partial_and_empty_mask(T, tag):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(texture_config(T, tag))
    pts, cols = torch.from_numpy(T["points"]), torch.from_numpy(T["colors"])
    mask = torch.rand(pts.shape[0], generator=torch.Generator().manual_seed(5)) < 0.3
    keep = cols.clone()
    out = m.map_color_masked(pts, None, cols, mask)
    assert torch.equal(cols, keep)
    want = cols.clone()
    want[mask] = m.map_color(pts[mask], None, cols[mask])  # the batch mean is the masked rows' alone
    assert torch.equal(out, want) and not torch.equal(out[mask], cols[mask])
    assert not torch.equal(out[mask], m.map_color(pts, None, cols)[mask])
    none = torch.zeros_like(mask)
    assert torch.equal(m.map_color_masked(pts, None, cols, none), cols)
    half = m.map_color_masked(pts, None, cols.half(), mask)
    assert half.dtype == torch.float16 and (half.float() - want).abs().max() < 4e-3


def test_every_tool_has_the_per_device_cache():
    """the shared colour routes of SealMapper keep their per-device constants in `_dev`"""
    from sealnerf import SealBBoxMapper
    from test_seal import BBOX
    assert SealBBoxMapper(dict(BBOX))._dev == {}


def test_teacher_switches(T):
    """sealnerf/renderer.py: a texture alone re-colours (map_colors does not return early), pins the inference loop to the
    reference's batch shapes, and keeps the lean sample path on the native route — not together with `rgb`"""
    from sealnerf import get_seal_mapper
    from sealnerf.renderer import SealTeacherMixin

    class Host(SealTeacherMixin):
        pass
    pts, cols = torch.from_numpy(T["points"])[:512], torch.from_numpy(T["colors"])[:512]
    mask = torch.arange(512) % 3 == 0
    plain = get_seal_mapper(json.loads(str(T["brush"])))
    t = Host()
    t.seal_mapper = plain
    assert not t._batch_dependent_colors() and t._plain_sample_path() and t.map_colors(pts, None, cols, mask) is cols
    for tag, lean in (("image", True), ("image_hsv", True), ("image_rgb_hsv_light", False)):
        m = get_seal_mapper(texture_config(T, tag))
        t.seal_mapper = m
        assert t._batch_dependent_colors()
        assert t._plain_sample_path() is lean
        out = t.map_colors(pts, None, cols, mask)
        assert torch.equal(out, m.map_color_masked(pts, None, cols, mask)) and not torch.equal(out, cols)
        m.native = False
        assert t._plain_sample_path() is False
    t.proxy_enabled = False  # the student
    assert not t._batch_dependent_colors() and t._plain_sample_path()


def test_device_texture_layout(T):
    """what the kernel is handed: [H, W, 4] float32 texels of (h, s, v, alpha), hsv by the twin's rgb_to_hsv in float32, and
    the quad's 14 floats"""
    from sealnerf import get_seal_mapper
    from sealnerf.seal_utils import rgb_to_hsv
    m = get_seal_mapper(texture_config(T, "image_hsv"))
    k = m._image_native(torch.device("cpu"))
    md = m.map_data
    H, W = md["image"].shape[:2]
    assert k["texture"].shape == (H, W, 4) and k["texture"].dtype == torch.float32 and k["texture"].is_contiguous()
    assert torch.equal(k["texture"][..., :3].reshape(-1, 3), rgb_to_hsv(md["image"].reshape(-1, 3)))
    assert torch.equal(k["texture"][..., 3], md["image_mask"])
    ow, oh = md["v_image_w"] - md["v_image_o"], md["v_image_h"] - md["v_image_o"]
    assert k["quad"].dtype == np.float32 and k["quad"].shape == (14,)
    assert np.array_equal(k["quad"][:12], torch.cat([md["v_image_o"], ow, oh, md["v_image_norm"]]).numpy())
    assert k["quad"][12] == float(torch.norm(ow, 2) ** 2) and k["quad"][13] == float(torch.norm(oh, 2) ** 2)
    assert k["hsv"] == md["hsv"].tolist() and k["light"] == 0.0
    assert m._image_native(torch.device("cpu")) is k  # uploaded once per device


def test_new_entry_point_is_declared_bound_and_exported():
    import ctypes
    import s3d_hip
    from conftest import REPO
    name = "s3d_seal_map_color_image"
    assert name in s3d_hip.EXPORTS
    assert name in open(os.path.join(REPO, "include", "seal3d_hip.h")).read()
    if not os.path.exists(s3d_hip.LIB_PATH):
        s3d_hip.build()
    assert hasattr(ctypes.CDLL(s3d_hip.LIB_PATH), name)
    assert hasattr(s3d_hip.SealBackend, "map_color_image")
