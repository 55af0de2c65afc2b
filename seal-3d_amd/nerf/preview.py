"""The headless half of the reference's GUI (SealNeRF/gui.py, nerf/gui.py): the orbit camera, the two control rules, the
preview frame of `Trainer.test_gui` (nerf/utils.py:754-820) and the frame preparation of `NeRFGUI.prepare_buffer` /
`test_step` — everything behind the dearpygui window, which stays out of scope.

Two routes compute a frame.  The torch route is the reference's op sequence (get_rays, nan_to_num, two permutes around
F.interpolate, linear_to_srgb, the numpy overlay and accumulation written in torch); it runs on any device and is what the CPU
suite and the comparisons use.  The native route (CUDA tensors) is three launches around the render: s3d_frame_rays,
s3d_preview_resolve (csrc/preview.hip) and, for painted masks, the count / scan / emit of s3d_mask_positions_*; the frame never
leaves the device unless `PreviewSession.to_host()` is called.  Every operation of the tail except the sRGB power is individually
rounded fp32, so with `color_space="srgb"` the two routes give the same bits."""
import math
import time as _time

import numpy as np
import torch
import torch.nn.functional as F

from .synthetic import get_rays


# ---------------------------------------------------------------------- rotations (numpy; scipy is not a dependency)
def _quat_mul(a, b):
    """Hamilton product of two (x, y, z, w) quaternions: the rotation b followed by a"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=np.float64)


def _quat_from_rotvec(v):
    v = np.asarray(v, dtype=np.float64)
    angle = float(np.linalg.norm(v))
    if angle <= 1e-3:  # (the series of sin(angle / 2) / angle)
        scale = 0.5 - angle ** 2 / 48 + angle ** 4 / 3840
    else:
        scale = math.sin(angle / 2) / angle
    return np.array([scale * v[0], scale * v[1], scale * v[2], math.cos(angle / 2)], dtype=np.float64)


def _quat_to_matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _quat_from_matrix(m):
    """the unit quaternion of a (nearly) orthonormal 3 x 3 matrix: the largest of the four candidates is formed first"""
    m = np.asarray(m, dtype=np.float64)
    d = np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]])
    k = int(np.argmax(d))
    q = np.empty(4, dtype=np.float64)
    if k == 3:
        q[0], q[1], q[2], q[3] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + d[3]
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q[i] = 1 - d[3] + 2 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[l] = m[l, i] + m[i, l]
        q[3] = m[l, j] - m[j, l]
    return q / np.linalg.norm(q)


class OrbitCamera:
    """SealNeRF/gui.py:26-88.  The rotation is a unit quaternion (x, y, z, w) in float64, composed as the reference composes
    its scipy rotations; pose and intrinsics come out in the reference's dtypes (float32 matrix, float64 intrinsics)."""

    def __init__(self, W, H, r=2, fovy=60):
        self.W, self.H = W, H
        self.radius = r      # camera distance from the centre
        self.fovy = fovy     # degrees
        self.center = np.array([0, 0, 0], dtype=np.float32)
        self.rot = np.array([1.0, 0.0, 0.0, 0.0])  # from_quat([1, 0, 0, 0]): half a turn about x (the ngp convention)
        self.up = np.array([0, 1, 0], dtype=np.float32)

    def rotation(self):
        return _quat_to_matrix(self.rot)

    @property
    def pose(self):
        res = np.eye(4, dtype=np.float32)
        res[2, 3] -= self.radius
        rot = np.eye(4, dtype=np.float32)
        rot[:3, :3] = self.rotation()
        res = rot @ res
        res[:3, 3] -= self.center
        return res

    @pose.setter
    def pose(self, mat):
        mat = np.asarray(mat)
        rot = np.eye(4, dtype=np.float32)
        rot[:3, :3] = mat[:3, :3]
        res = np.eye(4, dtype=np.float32)
        res[2, 3] -= self.radius
        res = rot @ res
        self.rot = _quat_from_matrix(mat[:3, :3])
        self.center = res[:3, 3] - mat[:3, 3]

    @property
    def intrinsics(self):
        focal = self.H / (2 * np.tan(np.radians(self.fovy) / 2))
        return np.array([focal, focal, self.W // 2, self.H // 2])

    @intrinsics.setter
    def intrinsics(self, intr):
        self.fovy = 2 * np.degrees(np.arctan(self.H / (2 * intr[0])))

    def orbit(self, dx, dy):
        side = self.rotation()[:3, 0]
        rotvec_x = self.up * np.radians(-0.1 * dx)
        rotvec_y = side * np.radians(-0.1 * dy)
        q = _quat_mul(_quat_from_rotvec(rotvec_x), _quat_mul(_quat_from_rotvec(rotvec_y), self.rot))
        self.rot = q / np.linalg.norm(q)

    def scale(self, delta):
        self.radius *= 1.1 ** (-delta)

    def pan(self, dx, dy, dz=0):
        self.center += 0.0005 * self.rotation() @ np.array([dx, dy, dz])


# ---------------------------------------------------------------------- control rules (SealNeRF/gui.py:212-217, 347-353)
def next_downscale(t_ms, downscale):
    """dynamic resolution: a full-resolution frame may take 200 ms.  `t_ms`: the time of a frame rendered at `downscale`; the
    new value replaces the current one only when it differs by more than 20 %"""
    full_t = t_ms / (downscale ** 2)
    new = min(1, max(1 / 4, math.sqrt(200 / full_t)))
    return new if (new > downscale * 1.2 or new < downscale * 0.8) else downscale


def next_train_steps(t_ms, steps):
    """dynamic train steps: 16 steps may take 500 ms.  `t_ms`: the time `steps` steps took (the reference scales it to 16 steps
    first); 20 % hysteresis like next_downscale"""
    full_t = t_ms / steps * 16
    new = min(16, max(4, int(16 * 500 / full_t)))
    return new if (new > steps * 1.2 or new < steps * 0.8) else steps


# ---------------------------------------------------------------------- the torch route of the tail
def linear_to_srgb(x):
    return torch.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055)


def resolve_torch(image, depth, H, W, to_srgb=False, rays_o=None, rays_d=None, return_pos=False):
    """nerf/utils.py:782-799 on one frame: image [rH, rW, 3], depth [rH, rW] -> (image [H, W, 3], depth [H, W], pos or None)"""
    preds, preds_depth = image[None], torch.nan_to_num(depth)[None]
    if tuple(depth.shape) != (H, W):
        preds = F.interpolate(preds.permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1).contiguous()
        preds_depth = F.interpolate(preds_depth.unsqueeze(1), size=(H, W), mode="nearest").squeeze(1)
    if to_srgb:
        preds = linear_to_srgb(preds)
    pos = None
    if return_pos:
        pos = rays_o.view(H, W, 3) + preds_depth.view(H, W, 1) * rays_d.view(H, W, 3)
    return preds[0], preds_depth[0], pos


def mix_brush(img, masks, color, alpha=1.0):
    """`mix_brush` of NeRFGUI.prepare_buffer: img [H, W, 3], masks [K, H, W] uint8, color [3] fp32"""
    painted = (masks.sum(dim=0, dtype=torch.int64) > 0)[..., None]
    return torch.where(painted, color[None, None, :] * alpha + img * (1 - alpha), img)


def prepare_torch(frame_image, frame_depth, mode="image", masks=None, color=None, alpha=1.0):
    """NeRFGUI.prepare_buffer (SealNeRF/gui.py:219-289) without the window's drawing aids"""
    if mode == "image":
        out = frame_image
    else:
        out = (frame_depth / (frame_depth.max() + 1e-6))[..., None].repeat(1, 1, 3)
    if masks is not None and masks.shape[0] > 0:
        out = mix_brush(out, masks, torch.as_tensor(color, dtype=torch.float32, device=out.device), alpha)
    return out


def accumulate_torch(buffer, prepared, spp):
    """the accumulation of NeRFGUI.test_step: `spp` frames are in the buffer already.  The division is a true one, as numpy's
    (torch on the GPU would multiply by the reciprocal of a Python number)"""
    if spp == 0:
        return prepared.clone()
    return (buffer * spp + prepared) / torch.full((), float(spp + 1), dtype=buffer.dtype, device=buffer.device)


# ---------------------------------------------------------------------- one preview frame
def frame_rays(pose, intrinsics, rH, rW, device, native):
    """the rays of one camera for a whole frame: rays_o, rays_d [1, rH * rW, 3]"""
    pose = np.asarray(pose, dtype=np.float32)
    if native:
        import s3d_hip
        rays_o = torch.empty(1, rH * rW, 3, dtype=torch.float32, device=device)
        rays_d = torch.empty(1, rH * rW, 3, dtype=torch.float32, device=device)
        s3d_hip.RaySampleBackend.frame_rays(pose.reshape(-1).tolist(), intrinsics, rH, rW, rays_o, rays_d)
        return rays_o, rays_d
    rays = get_rays(torch.from_numpy(pose).unsqueeze(0).to(device), intrinsics, rH, rW, -1)
    return rays["rays_o"].contiguous(), rays["rays_d"].contiguous()


def resolve_frame(image, depth, H, W, to_srgb, rays_o, rays_d, return_pos, native, display=None):
    """the tail behind the render: -> dict(image, depth[, pos]); `display` (a PreviewSession's state: buffer, spp, mode, masks,
    color, alpha) has its buffer updated — in the same launch on the native route"""
    image, depth = image.float().contiguous(), depth.float().contiguous()
    if native:
        import s3d_hip
        kw = {}
        if display is not None:
            kw = dict(buffer=display["buffer"], mode=display["mode"], masks=display.get("masks"), color=display["color"],
                      alpha=display.get("alpha", 1.0), spp=display["spp"])
        fi, fd, pos = s3d_hip.PreviewBackend.resolve(image, depth, H, W, to_srgb, rays_o, rays_d, return_pos, **kw)
    else:
        fi, fd, pos = resolve_torch(image, depth, H, W, to_srgb, rays_o, rays_d, return_pos)
        if display is not None:
            prepared = prepare_torch(fi, fd, display["mode"], display.get("masks"), display["color"], display.get("alpha", 1.0))
            display["buffer"].copy_(accumulate_torch(display["buffer"], prepared, display["spp"]))
    out = {"image": fi, "depth": fd}
    if return_pos:
        out["pos"] = pos
    return out


def preview_frame(trainer, pose, intrinsics, W, H, bg_color=None, spp=1, downscale=1, return_pos=False, color_space="srgb",
                  native=None, display=None, perturb=None, **render_kw):
    """`Trainer.test_gui` (nerf/utils.py:754-820): see nerf/trainer.py"""
    if return_pos and downscale != 1:
        raise ValueError("test_gui: return_pos needs downscale == 1 (the position map is rays_o + depth * rays_d of the full frame)")
    if color_space not in ("srgb", "linear"):
        raise ValueError(f"test_gui: color_space is 'srgb' or 'linear', got {color_space!r}")
    device = next(trainer.model.parameters()).device
    if native is None:
        native = device.type == "cuda"
    elif native and device.type != "cuda":
        raise RuntimeError("test_gui: the native route needs the model on the GPU")
    rH, rW = int(H * downscale), int(W * downscale)
    if rH < 1 or rW < 1:
        raise ValueError(f"test_gui: downscale {downscale} leaves no pixel of a {H} x {W} frame")
    intrinsics = np.asarray(intrinsics, dtype=np.float64) * downscale
    rays_o, rays_d = frame_rays(pose, intrinsics, rH, rW, device, native)
    if torch.is_tensor(bg_color):
        bg_color = bg_color.to(device)
    if perturb is None:
        perturb = False if spp == 1 else spp  # (spp doubles as the jitter switch; the first sample is not perturbed)
    out = trainer._preview_render(rays_o, rays_d, bg_color, perturb, **render_kw)
    return resolve_frame(out["image"].reshape(rH, rW, 3), out["depth"].reshape(rH, rW), H, W, color_space == "linear",
                         rays_o, rays_d, return_pos, native, display)


def mask_positions(pos, masks, native):
    """`get_mask_pos`: [pos[m > 0] for m in masks] as device tensors"""
    if masks.shape[0] == 0:
        return []
    if native:
        import s3d_hip
        rows, offs = s3d_hip.PreviewBackend.mask_positions(masks.contiguous(), pos.contiguous())
        return [rows[a:b] for a, b in zip(offs[:-1], offs[1:])]
    return [pos[m > 0] for m in masks]


def stroke_mask(H, W, p0, p1, thickness, device="cpu"):
    """a painted line as a capsule: the pixels within thickness / 2 of the segment p0 -> p1 ((x, y) pixel coordinates), uint8
    [H, W].  cv2.line's exact pixel set is not claimed."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device), torch.arange(W, dtype=torch.float32, device=device),
                            indexing="ij")
    ax, ay, bx, by = float(p0[0]), float(p0[1]), float(p1[0]), float(p1[1])
    dx, dy = bx - ax, by - ay
    t = ((xs - ax) * dx + (ys - ay) * dy) / max(dx * dx + dy * dy, 1e-12)
    t = t.clamp(0, 1)
    dist2 = (xs - (ax + t * dx)) ** 2 + (ys - (ay + t * dy)) ** 2
    return (dist2 <= (max(float(thickness), 1.0) / 2) ** 2).to(torch.uint8)


class PreviewSession:
    """`NeRFGUI` without the window: camera, display buffer (on the trainer's device), accumulation state, view mode and the
    painted strokes.  `step()` is `NeRFGUI.test_step`."""

    def __init__(self, trainer, W, H, max_spp=64, radius=2, fovy=60, bg_color=None, color_space="srgb", dynamic_resolution=True,
                 native=None, time=None):
        self.trainer, self.W, self.H, self.max_spp = trainer, int(W), int(H), max_spp
        self.cam = OrbitCamera(W, H, r=radius, fovy=fovy)
        self.device = next(trainer.model.parameters()).device
        self.native = (self.device.type == "cuda") if native is None else native
        self.bg_color = torch.ones(3, dtype=torch.float32) if bg_color is None else bg_color
        self.color_space = color_space
        self.render_trainer = trainer
        self.buffer = torch.zeros(self.H, self.W, 3, dtype=torch.float32, device=self.device)
        self.need_update = True   # the camera moved: restart the accumulation
        self.spp = 1
        self.mode = "image"
        self.dynamic_resolution = dynamic_resolution
        self.downscale = 1
        self.brush_masks = []
        self._stacked = None
        self.brush_color = np.array([1.0, 0.0, 0.0], dtype=np.float32)
        self.brush_alpha = 1.0
        self.show_strokes = True
        self.time = time  # a D-NeRF trainer previews at this time
        self.last_frame, self.last_ms = None, None

    # -- strokes
    def add_stroke(self, mask):
        mask = torch.as_tensor(mask)
        if tuple(mask.shape[:2]) != (self.H, self.W):
            raise ValueError(f"add_stroke: a mask is [{self.H}, {self.W}], got {tuple(mask.shape)}")
        self.brush_masks.append((mask.reshape(self.H, self.W) != 0).to(torch.uint8).to(self.device))
        self._stacked = None
        self.need_update = True

    def stroke(self, p0, p1, thickness=10, add=True):
        mask = stroke_mask(self.H, self.W, p0, p1, thickness, self.device)
        if add:
            self.add_stroke(mask)
        return mask

    def clear_strokes(self):
        self.brush_masks, self._stacked = [], None
        self.need_update = True

    def masks(self):
        """[K, H, W] uint8 on the device (K may be 0)"""
        if self._stacked is None:
            self._stacked = torch.stack(self.brush_masks) if self.brush_masks else \
                torch.zeros(0, self.H, self.W, dtype=torch.uint8, device=self.device)
        return self._stacked

    def set_mode(self, mode):
        if mode not in ("image", "depth"):
            raise ValueError(f"mode is 'image' or 'depth', got {mode!r}")
        self.mode, self.need_update = mode, True

    # -- frames
    def _test_gui(self, trainer, spp, downscale, return_pos=False, display=None):
        kw = {} if self.time is None else {"time": self.time}
        if return_pos:
            kw["return_pos"] = True
        return trainer.test_gui(self.cam.pose, self.cam.intrinsics, self.W, self.H, bg_color=self.bg_color, spp=spp,
                                downscale=downscale, color_space=self.color_space, native=self.native, display=display, **kw)

    def step(self):
        """render one frame into the buffer if the view changed or the accumulation is not full; returns whether it did"""
        if not (self.need_update or self.spp < self.max_spp):
            return False
        on_gpu = self.device.type == "cuda"
        if on_gpu:
            starter, ender = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            starter.record()
        else:
            t0 = _time.perf_counter()
        display = dict(buffer=self.buffer, spp=0 if self.need_update else self.spp, mode=self.mode,
                       masks=self.masks() if self.show_strokes else None, color=self.brush_color, alpha=self.brush_alpha)
        self.last_frame = self._test_gui(self.render_trainer, self.spp, self.downscale, display=display)
        if on_gpu:
            ender.record()
            ender.synchronize()
            t = starter.elapsed_time(ender)
        else:
            t = (_time.perf_counter() - t0) * 1000
        self.last_ms = t
        if self.dynamic_resolution and t > 0:
            self.downscale = next_downscale(t, self.downscale)
        if self.need_update:
            self.spp, self.need_update = 1, False
        else:
            self.spp += 1
        return True

    def mask_positions(self, cluster=True, trainer=None):
        """`get_mask_pos`: the 3-D points under the painted masks (one tensor per stroke), or with cluster=False the whole
        position map [H, W, 3]; rendered at full resolution by `trainer` (default: the session's)"""
        pos = self._test_gui(trainer or self.trainer, 1, 1, return_pos=True)["pos"]
        if not cluster:
            return pos
        return mask_positions(pos, self.masks(), self.native)

    def to_host(self):
        return self.buffer.detach().cpu().numpy()
