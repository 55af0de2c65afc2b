"""Seal proxy functions (SealNeRF/seal_utils.py): map edited-space points back to the source space.

Three tools, each a `SealMapper` with a torch op sequence and device kernels (csrc/seal.hip):
  bbox    (`SealBBoxMapper`, seal_utils.py:155-279): `raw` (points spanning the source box), `transform` (4x4 source->target),
          `scale` (3), `boundType` ('to' | 'from' | 'both'), optional `mapSource`;
  brush   (`SealBrushMapper`, :282-453): `line` strokes pushed / pulled along their plane normal, `linear` or `dry`;
  anchor  (`SealAnchorMapper`, :456-570): a control point dragged by `translation`, its cone of influence carried along.
No trimesh / pytorch3d / skspatial: the box meshes are built directly (12 triangles per box), the plane fit and the uv-sphere
vertex set are restated, and the inside test is the reference's two-ray Moller-Trumbore parity test (seal_utils.py:630-685)
in plain torch.  Colour remapping: the `hsv` / `rgb` options (seal_utils.py:48-58, 739-769, color_utils.py:33-66) of every
tool, and the brush tool's texture painting (`imageConfig`, seal_utils.py:58-79, 382-404: texels inline, from a `.npy`, or
through an `image_loader`); `curve` strokes and the `ease-in` / `ease-out` attenuation are refused.
"""
import json

import numpy as np
import torch

_BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                       [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
# fixed test direction of the reference's inside test (seal_utils.py:676-678)
_TEST_DIR = (0.4395064455, 0.617598629942, 0.652231566745)


def _box_vertices(lo, hi):
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float64)


def _min_area_rect(p2):
    """minimum-area enclosing rectangle of 2-D points: (area, angle of the rectangle's first axis); one side of the optimum
    is collinear with a hull edge, so the hull edges are the only candidates, and the extents are those of the hull's vertices"""
    from scipy.spatial import ConvexHull
    hull = p2[ConvexHull(p2).vertices]
    best = (np.inf, 0.0)
    for a, b in zip(hull, np.roll(hull, -1, axis=0)):
        e = b - a
        n = np.linalg.norm(e)
        if n < 1e-12:
            continue
        e = e / n
        q = hull @ np.stack([e, [-e[1], e[0]]], axis=1)
        area = np.prod(q.max(0) - q.min(0))
        if area < best[0]:
            best = (area, np.arctan2(e[1], e[0]))
    return best


def oriented_box_vertices(points, snap=1e-9):
    """8 corners of the minimum-volume oriented bounding box of `points` — what the reference gets from
    `trimesh.PointCloud(raw).bounding_box_oriented` (seal_utils.py:587-588; trimesh.bounds.oriented_bounds: one face of
    the optimum is parallel to a convex-hull facet, so every facet normal is tried with the minimum-area rectangle of the
    projection).  Corner order is that of `_box_vertices` (index bits = side along the box's own x, y, z axes), so
    `_BOX_FACES` triangulates it.  A box whose axes are the coordinate axes (within `snap`) is returned as the exact
    min / max corners; coplanar or fewer than 4 points fall back to the axis-aligned box."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    aabb = _box_vertices(lo, hi)
    try:
        from scipy.spatial import ConvexHull
        hull = ConvexHull(pts)
    except Exception:  # degenerate input (QhullError) or no scipy: the axis-aligned box
        return aabb
    hp = pts[hull.vertices]
    best = None
    seen = []
    for eq in hull.equations:
        n = eq[:3] / np.linalg.norm(eq[:3])
        if n[np.argmax(np.abs(n))] < 0:
            n = -n  # a normal and its opposite give the same box
        if seen and np.any(np.abs(np.abs(np.array(seen) @ n) - 1) < 1e-12):
            continue
        seen.append(n)
        ref = np.eye(3)[np.argmin(np.abs(n))]
        u = np.cross(n, ref)
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        area, ang = _min_area_rect(hp @ np.stack([u, v], axis=1))
        h = hp @ n
        vol = area * (h.max() - h.min())
        if best is None or vol < best[0] * (1 - 1e-12):
            c, s_ = np.cos(ang), np.sin(ang)
            best = (vol, np.stack([c * u + s_ * v, -s_ * u + c * v, n]))  # rows = box axes
    vol_aabb = np.prod(hi - lo)
    R = best[1]
    # the box's axes up to order / sign are the coordinate axes -> the exact AABB (also when it is not smaller)
    if best[0] >= vol_aabb * (1 - 1e-12) or np.all(np.abs(np.abs(R).max(1) - 1) < snap):
        return aabb
    # canonical axis order / sign: each box axis is assigned to the coordinate axis it is closest to, pointing along +
    order = []
    for k in range(3):
        cand = [i for i in range(3) if i not in order]
        order.append(max(cand, key=lambda i: abs(R[i, k])))
    R = R[order]
    R = R * np.where(R[np.arange(3), np.arange(3)] < 0, -1.0, 1.0)[:, None]
    q = pts @ R.T
    qlo, qhi = q.min(0), q.max(0)
    return _box_vertices(qlo, qhi) @ R


def moller_trumbore_any(ray_o, ray_d, tris, eps=1e-8):
    """does ray i hit any triangle?  (n_rays, 3), (n_rays, 3), (n_faces, 3, 3)  — seal_utils.py:630-665"""
    E1 = tris[:, 1] - tris[:, 0]
    E2 = tris[:, 2] - tris[:, 0]
    N = torch.cross(E1, E2, dim=-1)
    invdet = 1.0 / -(torch.einsum("md,nd->mn", ray_d, N) + eps)
    A0 = ray_o[:, None] - tris[None, :, 0]
    DA0 = torch.cross(A0, ray_d[:, None].expand(*A0.shape), dim=-1)
    u = torch.einsum("mnd,nd->mn", DA0, E2) * invdet
    v = -torch.einsum("mnd,nd->mn", DA0, E1) * invdet
    t = torch.einsum("mnd,nd->mn", A0, N) * invdet
    return ((t >= 0.0) & (u >= 0.0) & (v >= 0.0) & ((u + v) <= 1.0)).any(1)


def points_in_mesh(points, triangles, rays_d=None):
    """a point is inside iff rays in BOTH directions of the test axis hit the mesh (seal_utils.py:668-685); `rays_d` [1, 3]
    replaces the fixed axis (the brush tool tests along its unnormalised `normal_expand`, seal_utils.py:379)"""
    if rays_d is None:
        rays_d = torch.tensor([_TEST_DIR], device=points.device, dtype=points.dtype)
    d = rays_d.repeat(points.shape[0], 1)
    hit = moller_trumbore_any(torch.cat([points, points]), torch.cat([d, -d]), triangles)
    return hit[:points.shape[0]] & hit[points.shape[0]:]


def rgb_to_hsv(rgb):
    """color_utils.py:33-46 (`rgb2hsv_torch`) on [N, 3], closed form instead of boolean-mask scatters: hue from the FIRST
    maximal channel (torch.max's tie rule), `%` = floored modulo, grey (delta == 0) -> hue 0; no host sync"""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    cmax, idx = torch.max(rgb, dim=1)
    cmin = torch.min(rgb, dim=1)[0]
    delta = cmax - cmin
    safe = torch.where(delta == 0, torch.ones_like(delta), delta)
    h0 = torch.remainder((g - b) / safe, 6.0)
    h1 = (b - r) / safe + 2.0
    h2 = (r - g) / safe + 4.0
    h = torch.where(idx == 0, h0, torch.where(idx == 1, h1, h2))
    h = torch.where(delta == 0, torch.zeros_like(h), h) / 6.0
    s = torch.where(cmax == 0, torch.zeros_like(cmax), delta / torch.where(cmax == 0, torch.ones_like(cmax), cmax))
    return torch.stack([h, s, cmax], dim=1)


def hsv_to_rgb(hsv):
    """color_utils.py:49-66 (`hsv2rgb_torch`) on [N, 3]; the sextant is `(h * 6)` cast to uint8, modulo 6, as there"""
    h, s, v = hsv[:, 0], hsv[:, 1], hsv[:, 2]
    c = v * s
    x = c * (-torch.abs(torch.remainder(h * 6.0, 2.0) - 1.0) + 1.0)
    m = v - c
    o = torch.zeros_like(c)
    idx = (h * 6.0).to(torch.uint8) % 6
    table = torch.stack([torch.stack([c, x, o], 1), torch.stack([x, c, o], 1), torch.stack([o, c, x], 1),
                         torch.stack([o, x, c], 1), torch.stack([x, o, c], 1), torch.stack([c, o, x], 1)], dim=1)  # [N, 6, 3]
    rgb = table.gather(1, idx.long()[:, None, None].expand(-1, 1, 3))[:, 0]
    return rgb + m[:, None]


def modify_hsv(rgb, modification):
    """seal_utils.py:739-750: rgb -> hsv, add the offsets, -> rgb"""
    if rgb.shape[0] == 0:
        return rgb
    hsv = rgb_to_hsv(rgb)
    mod = torch.as_tensor(modification, dtype=rgb.dtype, device=rgb.device)
    return hsv_to_rgb(hsv + mod[None, :3])


def modify_rgb(rgb, modification, light_offset=0):
    """seal_utils.py:753-769: hue and saturation of the target colour, value = the target's value + the sample's offset from
    the batch's mean value (+ light_offset), clamped to [0, 1]"""
    if rgb.shape[0] == 0:
        return rgb
    hsv = rgb_to_hsv(rgb)
    mod = rgb_to_hsv(torch.as_tensor(modification, dtype=rgb.dtype, device=rgb.device).view(-1, 3))
    raw = hsv[:, 2]
    val = torch.clamp(mod[:, 2] + (raw - raw.mean()) + light_offset, 0.0, 1.0)
    out = torch.stack([mod[:, 0].expand_as(val), mod[:, 1].expand_as(val), val], dim=1)
    return hsv_to_rgb(out)


def pil_image_loader(path):
    """a ready-made `image_loader` for get_seal_mapper: decode an image file with PIL (imported here only) to uint8
    [H, W, 3] RGB or [H, W, 4] RGBA — what the reference gets from cv2.imread(IMREAD_UNCHANGED) after its BGR(A) -> RGB
    swap.  A palette image is expanded (with its transparency); a grey image stays 2-D and is refused downstream; every
    other mode (CMYK, LA, 16-bit, ...) is refused here: its channels are not RGB(A)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == "P":
            im = im.convert("RGBA" if "transparency" in im.info else "RGB")
        if im.mode not in ("RGB", "RGBA", "L"):
            raise ValueError(f"pil_image_loader: `{path}` has mode {im.mode}; RGB, RGBA and palette images only")
        return np.asarray(im).copy()


def load_texture(image_conf, image_loader=None):
    """the texels of an `imageConfig` as float32 (image [H, W, 3], alpha [H, W]) — seal_utils.py:385-394.  `pixels`: a
    nested list / ndarray [H, W, 3 | 4] given inline; `path`: a `.npy` file of the same, or an encoded image file, which
    `image_loader` (path -> ndarray [H, W, 3 | 4], RGB(A) order) decodes.  uint8 (any integer type: 0..255) is divided by 255,
    floats are taken as they are; without an alpha channel alpha is 1."""
    if "pixels" in image_conf:
        arr = np.asarray(image_conf["pixels"])
    else:
        path = image_conf["path"]
        if str(path).lower().endswith(".npy"):
            arr = np.load(path)
        elif image_loader is None:
            raise NotImplementedError(f"imageConfig: `{path}` is an encoded image file and the core decodes none (torch and numpy "
                                      "only): pass get_seal_mapper(..., image_loader=) a callable path -> ndarray [H, W, 3 | 4] "
                                      "in RGB(A) order (sealnerf.pil_image_loader is one), or give the texels as a `.npy` file")
        else:
            arr = np.asarray(image_loader(path))
    if arr.ndim != 3 or arr.shape[2] not in (3, 4) or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"imageConfig: texels must be [H, W, 3] (RGB) or [H, W, 4] (RGBA), got {arr.shape}")
    if arr.dtype.kind in "ui":  # uint8, or the integers of a JSON list: 0..255
        if arr.min() < 0 or arr.max() > 255:
            raise ValueError(f"imageConfig: integer texels must lie in 0..255, got {int(arr.min())}..{int(arr.max())}")
        arr = arr.astype(np.float32) / np.float32(255)
    elif arr.dtype.kind != "f":
        raise ValueError(f"imageConfig: texels must be integers 0..255 or floating point, got {arr.dtype}")
    arr = arr.astype(np.float32)
    alpha = arr[:, :, 3] if arr.shape[2] == 4 else np.ones(arr.shape[:2], dtype=np.float32)
    return np.ascontiguousarray(arr[:, :, :3]), np.ascontiguousarray(alpha)


class SealMapper:
    """what every tool shares (seal_utils.py:18-153): the constants in `map_data` (float32 tensors) and `map_triangles`, their
    device, the `hsv` / `rgb` colour edit of the moved samples and the AABB + mesh `map_mask`.  `native = True`: GPU tensors go
    through the tool's device kernels (csrc/seal.hip); False = the reference's torch op sequence."""
    native = True
    map_test_dir = None  # [1, 3] ray direction of the inside test; None = the fixed axis

    def _color_options(self, seal_config):
        if "hsv" in seal_config:  # seal_utils.py:226-230, 389-393, 497-501
            self.map_data["hsv"] = torch.tensor(seal_config["hsv"], dtype=torch.float32)
        if "rgb" in seal_config:
            self.map_data["rgb"] = torch.tensor(seal_config["rgb"], dtype=torch.float32)
            self.map_data["rgb_light_offset"] = float(seal_config.get("rgbLightOffset", 0))

    def to(self, device):
        if device != self.device:
            self.map_data = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.map_data.items()}
            self.map_triangles = self.map_triangles.to(device)
            if self.map_test_dir is not None:
                self.map_test_dir = self.map_test_dir.to(device)
            self.device = device
        return self

    def map_mask(self, points):
        """AABB pre-test (incl. the reference's `points.all(1)` term) then the mesh inside test — seal_utils.py:132-153"""
        bounds = self.map_data["map_bound"]
        if bounds.ndim == 2:
            bounds = bounds[None]
        mask = None
        for i in range(bounds.shape[0]):
            cur = points.all(1) & ((bounds[i][1] > points) & (points > bounds[i][0])).all(1)
            mask = cur if mask is None else (mask | cur)
        if not mask.any():
            return mask
        inside = points_in_mesh(points[mask], self.map_triangles, self.map_test_dir)
        mask[mask.clone()] = inside
        return mask

    def map_color(self, points, dirs, colors):
        """seal_utils.py:48-81 (`hsv` / `rgb` of seal.json, :226-230, 389-393, 497-501): hue / saturation / value offsets, then
        re-colouring towards a target RGB that keeps each sample's brightness offset from the batch mean, then the brush
        tool's texture painting (`imageConfig`, :58-79): the same re-colouring towards the texel under each of `points` (the
        MAPPED sample points; the batch mean is that of all rows passed in), blended by the texel's alpha.  Torch ops on any
        device and dtype; the constants follow `points`."""
        if "hsv" in self.map_data:
            colors = modify_hsv(colors, self.map_data["hsv"])
        if "rgb" in self.map_data:
            colors = modify_rgb(colors, self.map_data["rgb"], self.map_data.get("rgb_light_offset", 0))
        if "image" in self.map_data:
            k = self._image_twin(points.device, points.dtype)
            idx_h, idx_w = self.texel_indices(points)
            alpha = k["image_mask"][idx_h, idx_w].to(colors.dtype)[None].T
            modified = modify_rgb(colors, k["image"][idx_h, idx_w].to(colors.dtype), self.map_data["rgb_light_offset"])
            colors = alpha * modified + (1 - alpha) * colors
        return colors

    def _image_twin(self, device, dtype):
        """the texture's constants on `device` in `dtype` (one copy per device and dtype; a caller that edits map_data in
        place clears `_dev`)"""
        key = ("twin", device, dtype)
        k = self._dev.get(key)
        if k is None:
            md = self.map_data
            k = {n: md[n].to(device, dtype) for n in ("image", "image_mask", "v_image_norm", "v_image_o", "v_image_w", "v_image_h")}
            self._dev[key] = k
        return k

    @torch.autocast("cuda", enabled=False)
    def texel_indices(self, points):
        """seal_utils.py:61-75: (idx_h, idx_w) of the texel under each point — the point projected onto the image plane, its
        coordinate along o->w (o->h) as a share of that edge times W (H), floored; outside the quad the edge texel.  Like
        map_to_origin it runs with autocast off: the dot products stay in the points' precision inside an fp16 render (half
        precision would move a point by texels)"""
        k = self._image_twin(points.device, points.dtype)
        H, W = k["image"].shape[:2]
        v_o = k["v_image_o"]
        v_op = project_points(k["v_image_norm"], v_o, points) - v_o
        v_ow, v_oh = k["v_image_w"] - v_o, k["v_image_h"] - v_o
        len_ow, len_oh = torch.norm(v_ow, 2), torch.norm(v_oh, 2)
        idx_w = torch.clamp(torch.floor(v_op @ v_ow / len_ow ** 2 * W), 0, W - 1).to(torch.long)
        idx_h = torch.clamp(torch.floor(v_op @ v_oh / len_oh ** 2 * H), 0, H - 1).to(torch.long)
        return idx_h, idx_w

    def _image_native(self, device):
        """what s3d_seal_map_color_image takes, uploaded once per device: the texture as [H, W, 4] float32 texels of
        (h, s, v, alpha) — `rgb_to_hsv` of the image in float32 on the host, the conversion modify_rgb applies to its target,
        so both routes see the same bits — and the quad's 14 host floats (o, ow, oh, normal, |ow|^2, |oh|^2).  The `hsv`
        offsets and the light offset are taken along as host values (no read-back inside a captured render): like the
        tensors they are those of the first call on the device until `_dev` is cleared"""
        key = ("image", device)
        k = self._dev.get(key)
        if k is None:
            md = {n: (v.detach().cpu() if torch.is_tensor(v) else v) for n, v in self.map_data.items()}
            image = md["image"].float()
            H, W = image.shape[:2]
            texels = torch.cat([rgb_to_hsv(image.reshape(-1, 3)), md["image_mask"].float().reshape(-1, 1)], dim=1)
            v_o = md["v_image_o"].float()
            v_ow, v_oh = md["v_image_w"].float() - v_o, md["v_image_h"].float() - v_o
            quad = torch.cat([v_o, v_ow, v_oh, md["v_image_norm"].float(),
                              (torch.norm(v_ow, 2) ** 2)[None], (torch.norm(v_oh, 2) ** 2)[None]]).numpy().copy()
            k = {"texture": texels.reshape(H, W, 4).contiguous().to(device), "quad": quad,
                 "hsv": md["hsv"].tolist() if "hsv" in md else None, "light": float(md["rgb_light_offset"])}
            self._dev[key] = k
        return k

    def map_color_masked(self, points, dirs, colors, mask):
        """the renderers' use of map_color (SealNeRF/renderer.py:316, 396-399): `colors[mask] = map_color(points[mask],
        dirs[mask], colors[mask])` — returns a new tensor, `colors` is left alone.  GPU tensors of a `native` mapper go through
        the device kernels: `hsv` / `rgb` through s3d_seal_map_color, a texture (with or without `hsv`) through
        s3d_seal_map_color_image; `rgb` together with a texture, and everything else, through map_color's torch ops."""
        md = self.map_data
        on_device = (self.native and colors.is_cuda and mask is not None and colors.dtype in (torch.float32, torch.float16)
                     and colors.dim() == 2 and colors.shape[1] == 3)
        if on_device and "image" in md and "rgb" not in md and points is not None and points.is_cuda and points.shape == colors.shape:
            # texture painting (with or without `hsv`): the batch mean, then one pass with one 16-byte texel load per moved
            # sample (csrc/seal.hip: s3d_seal_map_color_image).  With `rgb` as well the texture step's batch mean depends on
            # the `rgb` step's, a third pass: that combination takes the torch op sequence below, on the GPU.
            import s3d_hip
            k = self._image_native(colors.device)
            src = colors.contiguous()
            out = torch.empty_like(src)
            s3d_hip.SealBackend.map_color_image(src, points.float().contiguous(), mask.view(torch.uint8), k["hsv"], k["texture"], k["quad"],
                                                k["light"], out, n_valid=s3d_hip.active_row_limit(src.shape[0]))
            return out
        if on_device and "image" not in md and ("hsv" in md or "rgb" in md):
            # one or two passes on the device (csrc/seal.hip: s3d_seal_map_color) instead of a boolean gather (host sync), ~40
            # masked elementwise launches and a scatter back; the batch mean of the `rgb` edit is an order-independent sum
            import s3d_hip
            src = colors.contiguous()
            out = torch.empty_like(src)
            hsv = md["hsv"].tolist() if "hsv" in md else None
            tgt = md["rgb"].tolist() if "rgb" in md else None
            s3d_hip.SealBackend.map_color(src, mask.view(torch.uint8), hsv, tgt, md.get("rgb_light_offset", 0) if tgt is not None else 0.0,
                                          out, n_valid=s3d_hip.active_row_limit(src.shape[0]))
            return out
        out = colors.clone()
        if mask is None:
            return self.map_color(points, dirs, out)
        sel = colors[mask]
        if sel.shape[0]:
            out[mask] = self.map_color(points[mask] if points is not None else None, dirs[mask] if dirs is not None else None,
                                       sel.float()).to(colors.dtype)
        return out


class SealBBoxMapper(SealMapper):
    def __init__(self, seal_config):
        self.config = seal_config
        T = np.array(seal_config["transform"], dtype=np.float64)
        scale = np.array(seal_config["scale"], dtype=np.float64)
        raw = np.array(seal_config["raw"], dtype=np.float64)
        # the reference's `get_trimesh_box(raw)`: the ORIENTED bounding box of the raw points (seal_utils.py:186-188, 587-588)
        from_v = oriented_box_vertices(raw)
        center = from_v.mean(0)
        to_v = (from_v - center) * scale + center
        to_v = to_v @ T[:3, :3].T + T[:3, 3]
        to_center = to_v.mean(0)
        from_b = np.stack([from_v.min(0), from_v.max(0)])
        to_b = np.stack([to_v.min(0), to_v.max(0)])
        fill = np.stack([to_b, from_b])  # [2 boxes, (min,max), 3]  == force_fill_bound
        kind = seal_config.get("boundType", "to")
        if kind == "to":
            bounds, verts = to_b, [to_v]
        elif kind == "from":
            bounds, verts = from_b, [from_v]
        elif kind == "both":
            bounds, verts = fill, [to_v, from_v]
        else:
            raise ValueError(f"unknown boundType {kind}")
        tris = np.concatenate([v[_BOX_FACES] for v in verts])
        self.map_data = {
            "force_fill_bound": torch.tensor(fill, dtype=torch.float32),
            "map_bound": torch.tensor(bounds, dtype=torch.float32),
            "pose_center": torch.tensor((center + to_center) / 2, dtype=torch.float32),
            "pose_radius": float(np.linalg.norm(center - to_center) * 10),
            "transform": torch.tensor(np.linalg.inv(T), dtype=torch.float32),
            "rotation": torch.tensor(np.linalg.inv(T[:3, :3]), dtype=torch.float32),
            "scale": torch.tensor(1.0 / scale, dtype=torch.float32),
            "center": torch.tensor(center, dtype=torch.float32),
        }
        self._color_options(seal_config)
        if seal_config.get("mapSource"):
            self.map_data["empty_bound"] = torch.tensor(from_b, dtype=torch.float32)
            self.map_data["map_source"] = torch.tensor(seal_config["mapSource"], dtype=torch.float32)
        self.map_triangles = torch.tensor(tris, dtype=torch.float32)
        self.device = torch.device("cpu")
        self._dev = {}  # (per-device constants of the shared colour routes; every tool has one)
        # the same constants as float32 host arrays for the device kernel (csrc/seal.hip)
        md = self.map_data
        self._host = {"triangles": self.map_triangles.numpy().copy(),
                      "bounds": md["map_bound"].numpy().reshape(-1, 2, 3).copy(),
                      "inv_transform": md["transform"].numpy().copy(), "inv_rotation": md["rotation"].numpy().copy(),
                      "inv_scale": md["scale"].numpy().copy(), "center": md["center"].numpy().copy()}
        if "map_source" in md:
            self._host["empty_bound"] = md["empty_bound"].numpy().copy()
            self._host["map_source"] = md["map_source"].numpy().copy()

    def _map_native(self, points, dirs):
        import s3d_hip
        lead = points.shape
        p = points.reshape(-1, 3).contiguous()
        d = dirs.reshape(-1, 3).float().contiguous() if dirs is not None else None
        out_p = torch.empty_like(p)
        out_d = torch.empty_like(d) if d is not None else None
        mask = torch.empty(p.shape[0], dtype=torch.bool, device=p.device)
        # inside a renderer's announced padded batch (s3d_hip.row_limit) the rows behind the sample count are skipped, like
        # in every other per-sample kernel of that path
        s3d_hip.SealBackend.bbox_map(p, d, self._host, out_p, out_d, mask.view(torch.uint8), s3d_hip.active_row_limit(p.shape[0]))
        return out_p.view(lead), (out_d.view(dirs.shape) if dirs is not None else None), mask

    @torch.autocast("cuda", enabled=False)
    def map_to_origin(self, points, dirs=None):
        """seal_utils.py:237-279"""
        if self.native and points.is_cuda and points.dtype == torch.float32 and points.shape[-1] == 3 and points.numel() > 0:
            return self._map_native(points, dirs)
        self.to(points.device)
        mask = self.map_mask(points)
        if not mask.any():
            return points, dirs, mask
        inner = points[mask]
        hom = torch.vstack([inner.T, torch.ones([1, inner.shape[0]], device=inner.device)])
        moved = torch.matmul(self.map_data["transform"], hom).T[:, :3]
        origin = (moved - self.map_data["center"]) * self.map_data["scale"] + self.map_data["center"]
        out_p = points.clone()
        out_d = dirs.clone() if dirs is not None else None
        if "map_source" in self.map_data:
            sb = self.map_data["empty_bound"]
            out_p[((sb[1] > points) & (points > sb[0])).all(1)] = self.map_data["map_source"]
        out_p[mask] = origin
        if dirs is not None:
            out_d[mask] = torch.matmul(self.map_data["rotation"], dirs[mask].T).T
        return out_p, out_d, mask


def fit_plane(points):
    """skspatial's `Plane.best_fit` (what seal_utils.py:311, 476 call): the centroid, and the left singular vector of the
    centred points with the smallest singular value as the normal; collinear points raise as there"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    centroid = pts.mean(0)
    centered = pts - centroid
    if np.linalg.matrix_rank(centered) <= 1:
        raise ValueError("The points must not be collinear.")
    u, _, _ = np.linalg.svd(centered.T, full_matrices=False)
    return u[:, 2].copy(), centroid


def project_points(plane_norm, plane_point, target_points):
    """seal_utils.py:728-736: project points onto the plane (normal need not be unit)"""
    v = target_points - plane_point
    return target_points - (v @ plane_norm).unsqueeze(1) / (plane_norm @ plane_norm) * plane_norm


def mesh_surface_points_mask(triangles, points, offset=1e-4):
    """seal_utils.py:712-725: a point is on the border when one of its six +-offset neighbours is outside the mesh"""
    o = torch.tensor([[0, 0, offset], [0, 0, -offset], [0, offset, 0], [0, -offset, 0], [offset, 0, 0], [-offset, 0, 0]],
                     dtype=torch.float64).to(points.device, points.dtype)
    return torch.sum(torch.stack([~points_in_mesh(points + o[i], triangles) for i in range(6)]), 0) > 0


def uv_sphere_vertices(radius, count=(32, 32)):
    """the vertex set of `trimesh.creation.uv_sphere(radius)` (what seal_utils.py:485 builds the anchor box around), restated:
    count -> (c0 + c0 % 2, 2 (c1 + c1 % 2)) = (32, 64); theta_i = i pi / 31 (i = 0..31), phi_j = 2 pi j / 64 (j = 0..63);
    vertex = radius (sin theta_i cos phi_j, sin theta_i sin phi_j, cos theta_i), the poles once each.  Only the convex hull of
    the set matters here (the oriented box is built around it)."""
    c0 = count[0] + count[0] % 2
    c1 = 2 * (count[1] + count[1] % 2)
    theta = np.linspace(0.0, np.pi, c0)[1:-1]
    phi = np.linspace(0.0, 2.0 * np.pi, c1 + 1)[:-1]
    t, p = np.meshgrid(theta, phi, indexing="ij")
    ring = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], -1).reshape(-1, 3)
    return np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * radius


class SealBrushMapper(SealMapper):
    """brush tool (seal_utils.py:282-453): push (brushPressure > 0) or pull the surface under one or more `line` strokes along
    the strokes' plane normal.  Config keys: `raw` (one stroke [N, 3] or a list of strokes), `normal` (which side of the plane
    is positive), `brushType` ('line', or a list with one entry per stroke), `brushDepth`, `brushPressure`,
    `attenuationDistance`, `attenuationMode` ('linear' | 'dry'), optional `hsv` / `rgb` / `rgbLightOffset`, optional
    `imageConfig` (texture painting: `o`, `w`, `h` = origin, end of the width axis and end of the height axis of the image
    quad, and the texels as `pixels` or `path`, see load_texture).
    Each stroke's edit region is the oriented box of its points lifted by 2 * normal_expand and sunk by brushDepth *
    normal_expand (12 triangles); a sample inside is moved back by normal_expand, less the part that attenuates linearly with
    the distance of its projection on the plane to the nearest border point of the strokes."""

    def __init__(self, seal_config, image_loader=None):
        self.config = seal_config
        strokes = seal_config["raw"]
        if np.asarray(strokes[0]).ndim == 1:
            strokes = [strokes]
        brush_type = seal_config["brushType"]
        if isinstance(brush_type, str):
            brush_type = [brush_type] * len(strokes)
        pressure, depth = seal_config["brushPressure"], seal_config["brushDepth"]
        tris, bounds, border = [], [], []
        for i, stroke in enumerate(strokes):
            pts = np.asarray(stroke, dtype=np.float64)
            normal, point = fit_plane(pts)
            if "normal" in seal_config and normal @ np.asarray(seal_config["normal"], dtype=np.float64) < 0:
                normal = -normal
            normal_expand = normal * pressure
            projected = project_points(torch.from_numpy(normal), torch.from_numpy(point), torch.from_numpy(pts))
            if brush_type[i] != "line":
                raise NotImplementedError(f"brushType `{brush_type[i]}`: only `line` strokes (a `curve` stroke's mesh needs open3d's "
                                          "vertex clustering, seal_utils.py:606-624)")
            verts = oriented_box_vertices(np.vstack([pts + 2 * normal_expand, pts - depth * normal_expand]))
            t = verts[_BOX_FACES]
            tris.append(t)
            bounds.append(np.stack([verts.min(0), verts.max(0)]))
            # (the reference runs this test in the mapper's float32)
            on_border = mesh_surface_points_mask(torch.from_numpy(t).float(), projected.float())
            border.append(projected[on_border])
        mode = seal_config["attenuationMode"]
        if mode not in ("linear", "dry"):
            raise NotImplementedError(f"attenuationMode `{mode}`: the reference implements `linear` and `dry` only")
        bounds = np.stack(bounds)
        self.map_data = {
            "force_fill_bound": torch.tensor(bounds, dtype=torch.float32),
            "map_bound": torch.tensor(bounds, dtype=torch.float32),
            "normal_expand": torch.tensor(normal_expand, dtype=torch.float32),  # (of the LAST stroke, as in the reference)
            "center": torch.tensor(point, dtype=torch.float32),
            "border_points": torch.cat(border).float(),  # (of ALL strokes)
            "attenuation_distance": torch.tensor(float(seal_config["attenuationDistance"]), dtype=torch.float32),
            "attenuation_mode": mode,
        }
        self._color_options(seal_config)
        if "imageConfig" in seal_config:  # seal_utils.py:382-404
            conf = seal_config["imageConfig"]
            image, alpha = load_texture(conf, image_loader)
            quad = [np.asarray(conf[k], dtype=np.float64) for k in ("o", "w", "h")]
            self.map_data["rgb_light_offset"] = float(seal_config.get("rgbLightOffset", 0))
            self.map_data["image"] = torch.from_numpy(image)
            self.map_data["image_mask"] = torch.from_numpy(alpha)
            self.map_data["v_image_norm"] = torch.tensor(fit_plane(quad)[0], dtype=torch.float32)
            for k, v in zip(("v_image_o", "v_image_w", "v_image_h"), quad):
                self.map_data[k] = torch.tensor(v, dtype=torch.float32)
        self.map_triangles = torch.tensor(np.concatenate(tris), dtype=torch.float32)
        self.map_test_dir = self.map_data["normal_expand"][None].clone()  # the UNnormalised ray direction of the inside test
        self.device = torch.device("cpu")
        self._dev = {}

    def _device_constants(self, device):
        """triangles / bounds / border points as one device buffer per device (uploaded on the first native call there; a
        caller that edits map_data / map_triangles in place clears `_dev`)"""
        c = self._dev.get(device)
        if c is None:
            md = self.map_data
            parts = [self.map_triangles.reshape(-1), md["map_bound"].reshape(-1), md["border_points"].reshape(-1)]
            buf = torch.cat([x.detach().cpu().float() for x in parts]).to(device)
            n = [x.numel() for x in parts]
            c = {"triangles": buf[:n[0]], "bounds": buf[n[0]:n[0] + n[1]], "border": buf[n[0] + n[1]:],
                 "n_tris": n[0] // 9, "n_bounds": n[1] // 6, "n_border": n[2] // 3,
                 "normal_expand": md["normal_expand"].detach().cpu().numpy().astype(np.float32),
                 "center": md["center"].detach().cpu().numpy().astype(np.float32),
                 "attenuation_distance": float(md["attenuation_distance"]), "linear": md["attenuation_mode"] == "linear"}
            self._dev[device] = c
        return c

    def _map_native(self, points, dirs):
        import s3d_hip
        lead = points.shape
        p = points.reshape(-1, 3).contiguous()
        out_p = torch.empty_like(p)
        mask = torch.empty(p.shape[0], dtype=torch.bool, device=p.device)
        s3d_hip.SealBackend.brush_map(p, self._device_constants(p.device), out_p, mask.view(torch.uint8),
                                      s3d_hip.active_row_limit(p.shape[0]))
        return out_p.view(lead), dirs, mask

    @torch.autocast("cuda", enabled=False)
    def map_to_origin(self, points, dirs=None):
        """seal_utils.py:408-453; `dirs` come back unchanged"""
        if self.native and points.is_cuda and points.dtype == torch.float32 and points.shape[-1] == 3 and points.numel() > 0:
            return self._map_native(points, dirs)
        self.to(points.device)
        md = self.map_data
        mask = self.map_mask(points)
        if not mask.any():
            return points, dirs, mask
        inner = points[mask]
        if md["attenuation_mode"] == "linear":
            ne, att = md["normal_expand"], md["attenuation_distance"]
            projected = project_points(ne, md["center"], inner)
            dist = torch.cdist(projected, md["border_points"]).min(1)[0]
            mapped = inner - ne
            near = att > dist
            mapped[near] += (torch.abs(att - dist[near]) / att)[None].T @ ne[None]
        else:  # dry: no space mapping
            mapped = inner
        out_p = points.clone()
        out_p[mask] = mapped
        return out_p, dirs, mask


class SealAnchorMapper(SealMapper):
    """control point (anchor) tool (seal_utils.py:456-570): drag the surface around `mean(raw)` by `translation`; the samples in
    a cone from the anchor disc (`radius`) to the moved anchor are carried back towards the plane of `raw`, then scaled by
    `scale` about the anchor.  Config keys: `raw`, `translation`, `radius`, `scale`, optional `hsv` / `rgb` / `rgbLightOffset`.
    The edit region is the oriented box of a uv-sphere of 1.1 radius around the anchor, swept by -0.1 translation, and the
    moved anchor (1.1 translation)."""

    def __init__(self, seal_config):
        self.config = seal_config
        t = np.asarray(seal_config["translation"], dtype=np.float64)
        raw = np.asarray(seal_config["raw"], dtype=np.float64)
        anchor = raw.mean(0)
        radius = float(seal_config["radius"])
        normal, point = fit_plane(raw)
        moved = anchor + t
        projected_moved = moved + ((point - moved) @ normal) / (normal @ normal) * normal  # skspatial Plane.project_point
        v_offset = projected_moved - anchor
        v_h = projected_moved - moved
        sphere = uv_sphere_vertices(radius * 1.1) + anchor
        verts = oriented_box_vertices(np.vstack([sphere, anchor + 1.1 * t, sphere - 0.1 * t]))
        bounds = np.stack([verts.min(0), verts.max(0)])
        self.map_data = {
            "force_fill_bound": torch.tensor(bounds, dtype=torch.float32),
            "map_bound": torch.tensor(bounds, dtype=torch.float32),
            "pose_center": torch.tensor(verts.mean(0), dtype=torch.float32),
            "pose_radius": float(np.linalg.norm(t) * 10),
            "v_anchor": torch.tensor(anchor, dtype=torch.float32),
            "v_offset": torch.tensor(v_offset, dtype=torch.float32),
            "v_h": torch.tensor(v_h, dtype=torch.float32),
            "len_h": torch.tensor(float(np.linalg.norm(v_h)), dtype=torch.float32),
            "radius": torch.tensor(radius, dtype=torch.float32),
            "scale": torch.tensor(np.asarray(seal_config["scale"], dtype=np.float64) * np.ones(3), dtype=torch.float32),
        }
        self._color_options(seal_config)
        # keep every point of the local pretraining lattice (seal_utils.py:493-494); a flag here, unlike the bbox tool's point
        self.map_data["map_source"] = True
        self.map_triangles = torch.tensor(verts[_BOX_FACES], dtype=torch.float32)
        self.device = torch.device("cpu")
        self._dev = {}

    def _device_constants(self, device):
        c = self._dev.get(device)
        if c is None:
            md = self.map_data
            f32 = lambda k: md[k].detach().cpu().numpy().astype(np.float32).reshape(-1)
            c = {"triangles": self.map_triangles.detach().reshape(-1).float().to(device), "n_tris": self.map_triangles.shape[0],
                 "bounds": f32("map_bound"),
                 # [v_anchor 3 | v_offset 3 | v_h 3 | len_h | radius | scale 3]
                 "params": np.concatenate([f32("v_anchor"), f32("v_offset"), f32("v_h"), f32("len_h"), f32("radius"), f32("scale")])}
            self._dev[device] = c
        return c

    def _map_native(self, points, dirs):
        import s3d_hip
        lead = points.shape
        p = points.reshape(-1, 3).contiguous()
        out_p = torch.empty_like(p)
        mask = torch.empty(p.shape[0], dtype=torch.bool, device=p.device)
        flag = torch.empty(1, dtype=torch.int32, device=p.device)
        s3d_hip.SealBackend.anchor_map(p, self._device_constants(p.device), out_p, mask.view(torch.uint8), flag,
                                       s3d_hip.active_row_limit(p.shape[0]))
        return out_p.view(lead), dirs, mask

    @torch.autocast("cuda", enabled=False)
    def map_to_origin(self, points, dirs=None):
        """seal_utils.py:514-570, with its two quirks: when no point of the batch passes the map mask the batch comes back
        unchanged with that (all-false) mask; otherwise the cone mapping applies to EVERY point of the batch and the returned
        mask is cone AND plane side, not intersected with the box mask.  `dirs` come back unchanged."""
        if self.native and points.is_cuda and points.dtype == torch.float32 and points.shape[-1] == 3 and points.numel() > 0:
            return self._map_native(points, dirs)
        self.to(points.device)
        md = self.map_data
        mask = self.map_mask(points)
        if not mask.any():
            return points, dirs, mask
        v_h, anchor, len_h, radius = md["v_h"], md["v_anchor"], md["len_h"], md["radius"]
        projected = project_points(v_h, anchor, points)
        to_plane = projected - points
        plane_dist = torch.norm(to_plane, 2, 1)
        offset_points = projected - plane_dist.unsqueeze(1) / len_h * md["v_offset"]
        anchor_dist = torch.norm(offset_points - anchor, 2, 1)
        in_cone = torch.logical_and(anchor_dist <= radius, plane_dist / (radius - anchor_dist) < len_h / radius * 1.1)
        valid = torch.logical_and(in_cone, to_plane @ v_h > 0)
        v_map = -((len_h - plane_dist[valid]) / 10)[None].T @ v_h[None] / len_h
        mapped = (offset_points[valid] - v_map - anchor) * md["scale"] + anchor
        out_p = points.clone()
        out_p[valid] = mapped
        return out_p, dirs, valid


def get_seal_mapper(config_dict=None, config_file=None, image_loader=None):
    """seal_utils.py:573-584 (plain JSON instead of json5).  `image_loader`: decoder of a brush `imageConfig` whose `path`
    is an encoded image file, a callable path -> ndarray [H, W, 3 | 4] in RGB(A) order (e.g. pil_image_loader); inline
    `pixels` and `.npy` paths need none."""
    if config_dict is None:
        with open(config_file) as f:
            config_dict = json.load(f)
    kind = config_dict["type"]
    if "imageConfig" in config_dict and kind != "brush":
        raise NotImplementedError(f"imageConfig: only the brush tool paints a texture (seal_utils.py:382-404), not `{kind}`")
    if kind == "bbox":
        return SealBBoxMapper(config_dict)
    if kind == "brush":
        return SealBrushMapper(config_dict, image_loader)
    if kind == "anchor":
        return SealAnchorMapper(config_dict)
    raise NotImplementedError(f"unknown seal tool `{kind}` (bbox, brush, anchor)")


def generate_default_editing_tool_config(type):
    """scripts/mesh2config.py:11-29: the defaults of a tool's config, `raw` still empty"""
    obj = {"type": type, "raw": []}
    if type == "bbox":
        obj["transform"] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
        obj["scale"] = [1, 1, 1]
    elif type == "brush":
        obj.update(normal=[0, 1, 0], brushType="line", brushDepth=0.3, brushPressure=0.05, attenuationDistance=0.02,
                   attenuationMode="linear")
    elif type == "anchor":
        obj.update(translation=[0, 0.1, 0], radius=0.03)
    else:
        raise NotImplementedError(f"unknown seal tool `{type}` (bbox, brush, anchor)")
    return obj


def config_from_mesh(mesh_path, type, config=None):
    """scripts/mesh2config.py:32-43: the vertices of a mesh marked in a mesh tool (a PLY, e.g. cut from Trainer.save_mesh's
    export) become the `raw` points of a tool config — `config` when given (an existing config whose points are replaced),
    else the tool's defaults.  -> a dict for get_seal_mapper(config_dict=...)"""
    from nerf.mesh import read_ply
    vertices, _ = read_ply(mesh_path)
    obj = dict(config) if config is not None else generate_default_editing_tool_config(type)
    obj["raw"] = vertices.astype(np.float64).tolist()
    return obj
