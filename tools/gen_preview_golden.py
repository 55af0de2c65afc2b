#!/usr/bin/env python3
"""Generate tests/golden/preview.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the headless half of the reference's GUI by EXECUTING it on the CPU: `SealNeRF/gui.py` is imported with `dearpygui` and
`cv2` replaced by stubs (every window call is a no-op that remembers the callbacks it is handed), and a real `NeRFGUI` is built
over a stand-in trainer whose `test_gui` / `test_step` are the reference's `nerf.utils.Trainer` methods on a tiny NGP model on
the CPU oracle.

  camera      `OrbitCamera(131, 67, r=2.5, fovy=50)` through a fixed script of orbit / scale / pan calls and both setters; pose
              and intrinsics after every call.
  rays        `get_rays(pose, intrinsics, rH, rW, -1)` for three of those poses at 5 x 7 and 20 x 39, the last at 67 x 131 too.
  tail        `Trainer.test_gui` at (H, W, downscale) = (5, 7, 1), (67, 131, 0.3), (67, 131, 0.5) with color_space srgb and
              linear, and (5, 7, 1), (20, 39, 1) with return_pos.  `test_step` is wrapped: it plants NaN, +inf and -inf in the
              depth and its results are recorded, so the tail can be replayed on exactly the renderer output the reference saw.
  prepare     `NeRFGUI.prepare_buffer` in image and depth mode with 0, 1 and 3 masks; the accumulation line of `test_step`.
  positions   `NeRFGUI.get_mask_pos`, and the config `callback_config_brush` builds from it.

    python tools/gen_preview_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import io
import os
import sys
import types
import zipfile
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import (SEAL_LOOP_NET, SEAL_LOOP_OPT, _assert_reference, _install_reference_stack, _load_synthetic,  # noqa: E402
                               _seed_params, _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "preview.npz")

CAM = dict(W=131, H=67, r=2.5, fovy=50)
SCRIPT = (("orbit", (35.0, -12.0, 0.0)), ("scale", (2.0, 0.0, 0.0)), ("pan", (40.0, -25.0, 10.0)), ("orbit", (-140.0, 260.0, 0.0)),
          ("set_pose", None), ("orbit", (7.0, 3.0, 0.0)), ("set_intrinsics", None), ("scale", (-1.5, 0.0, 0.0)), ("pan", (-8.0, 3.0, 0.0)))
RAY_POSES = (0, 4, len(SCRIPT))          # index into the recorded poses (0: the initial camera)
RAY_FRAMES = ((5, 7), (20, 39), (67, 131))
TAIL = ((5, 7, 1), (67, 131, 0.3), (67, 131, 0.5))
POS = ((5, 7), (20, 39))
PLANT = ((0, float("nan")), (3, float("inf")), (-2, float("-inf")))  # flat pixel of the rendered depth <- value


class _Anything:
    """a dearpygui call: returns itself, works as a context manager"""

    def __call__(self, *a, **k):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getattr__(self, name):
        return self


def _stub_window(callbacks):
    dpg = types.ModuleType("dearpygui.dearpygui")

    def attr(name):
        def call(*a, **k):
            if "callback" in k and ("tag" in k or "label" in k):
                callbacks[k.get("tag") or k.get("label")] = k["callback"]
            return False if name.startswith("is_") else _Anything()
        return call
    dpg.__getattr__ = attr
    pkg = types.ModuleType("dearpygui")
    pkg.dearpygui = dpg
    sys.modules["dearpygui"], sys.modules["dearpygui.dearpygui"] = pkg, dpg
    cv2 = sys.modules.get("cv2") or types.ModuleType("cv2")
    if not hasattr(cv2, "transform"):
        cv2.transform = None
    sys.modules["cv2"] = cv2

    class Event:  # torch.cuda.Event of a machine without a GPU
        def __init__(self, *a, **k):
            pass

        def record(self):
            pass

        def elapsed_time(self, other):
            return 100.0
    torch.cuda.Event = Event
    torch.cuda.synchronize = lambda *a, **k: None


def _masks(H, W, K, seed):
    rng = np.random.RandomState(seed)
    out = []
    for k in range(K):
        m = np.zeros((H, W, 1), dtype=np.uint8)
        y0, x0 = rng.randint(0, max(H - 2, 1)), rng.randint(0, max(W - 3, 1))
        m[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 4, 2)] = 1 + k  # (any non-zero value paints)
        m[rng.rand(H, W, 1) < 0.05] = 255
        out.append(m)
    return out


def main():
    _install_reference_stack()
    _stub_training_imports()
    callbacks = {}
    _stub_window(callbacks)
    import warnings
    warnings.simplefilter("ignore")
    utils = importlib.import_module("nerf.utils")
    net_mod = importlib.import_module("nerf.network")
    gui = importlib.import_module("SealNeRF.gui")
    for m_ in (utils, net_mod, gui):
        _assert_reference(m_)
    syn = _load_synthetic()
    out = {}

    # ---- camera
    cam = gui.OrbitCamera(**CAM)
    poses, intrs = [cam.pose.copy()], [cam.intrinsics.copy()]
    other = gui.OrbitCamera(10, 10, r=1.7)  # (the pose handed to the setter: a proper rotation, off-centre)
    other.orbit(200.0, -75.0)
    other.pan(100.0, 50.0)
    set_pose = other.pose.copy()
    set_intr = np.array([88.0, 88.0, 65.0, 33.0])
    for op, args in SCRIPT:
        if op == "set_pose":
            cam.pose = set_pose
        elif op == "set_intrinsics":
            cam.intrinsics = set_intr
        elif op == "scale":
            cam.scale(args[0])
        else:
            getattr(cam, op)(*(args[:2] if op == "orbit" else args))
        poses.append(cam.pose.copy())
        intrs.append(cam.intrinsics.copy())
    out.update(cam_init=np.array([CAM["W"], CAM["H"], CAM["r"], CAM["fovy"]], dtype=np.float64),
               cam_ops=np.array([op for op, _ in SCRIPT]), cam_args=np.array([a if a is not None else (np.nan,) * 3 for _, a in SCRIPT]),
               cam_set_pose=set_pose, cam_set_intrinsics=set_intr, cam_poses=np.stack(poses), cam_intrinsics=np.stack(intrs),
               cam_radius=np.float64(cam.radius), cam_fovy=np.float64(cam.fovy), cam_center=cam.center.copy())
    assert np.stack(poses).dtype == np.float32

    # ---- rays
    out["ray_poses"] = np.array(RAY_POSES)
    for pi in RAY_POSES:
        for rH, rW in RAY_FRAMES:
            if (rH, rW) == (67, 131) and pi != RAY_POSES[-1]:
                continue
            intr = intrs[pi] * (rH / CAM["H"])
            r = utils.get_rays(torch.from_numpy(poses[pi]).unsqueeze(0), intr, rH, rW, -1)
            key = f"rays_{pi}_{rH}x{rW}"
            out.update({f"{key}_intrinsics": np.asarray(intr, dtype=np.float64), f"{key}_rays_o": r["rays_o"][0].contiguous().numpy(),
                        f"{key}_rays_d": r["rays_d"][0].contiguous().numpy()})

    # ---- the stand-in trainer: a tiny NGP model on the CPU oracle, the reference's test_step / test_gui
    torch.manual_seed(3)
    net = net_mod.NeRFNetwork(**SEAL_LOOP_NET)
    _seed_params(net)
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    raw = {}

    def test_step(data, bg_color=None, perturb=False):
        rgb, depth = utils.Trainer.test_step(trainer, data, bg_color=bg_color, perturb=perturb)
        depth = depth.clone()
        flat = depth.view(-1)
        for i, v in PLANT:
            flat[i] = v
        raw["image"], raw["depth"] = rgb[0].clone().numpy(), depth[0].clone().numpy()
        return rgb, depth
    trainer = types.SimpleNamespace(model=net, ema=None, fp16=False, device=torch.device("cpu"), opt=types.SimpleNamespace(**SEAL_LOOP_OPT),
                                    test_step=test_step, log=lambda *a, **k: None)
    trainer.test_gui = lambda *a, **k: utils.Trainer.test_gui(trainer, *a, **k)
    view_pose, view_intr = syn.orbit_poses(1, seed=0)[0].numpy(), syn.lego_intrinsics(67, 131)
    out.update(view_pose=view_pose, view_intrinsics=np.asarray(view_intr, dtype=np.float64), bg_color=np.ones(3, dtype=np.float32),
               plant_index=np.array([i for i, _ in PLANT]), plant_value=np.array([v for _, v in PLANT], dtype=np.float32))
    bg = torch.ones(3)
    frames = {}
    for H, W, ds in TAIL:
        intr = view_intr * (H / 67)
        for cs in ("srgb", "linear"):
            trainer.opt.color_space = cs
            o = trainer.test_gui(view_pose, intr, W, H, bg, 1, ds)
            key = f"tail_{H}x{W}_{ds}_{cs}"
            out.update({f"{key}_raw_image": raw["image"], f"{key}_raw_depth": raw["depth"], f"{key}_image": o["image"], f"{key}_depth": o["depth"]})
            frames[(H, W, ds, cs)] = o
    trainer.opt.color_space = "srgb"
    out["tail_cases"] = np.array(TAIL, dtype=np.float64)
    for H, W in POS:
        o = trainer.test_gui(view_pose, view_intr * (H / 67), W, H, bg, 1, 1, True)
        key = f"pos_{H}x{W}"
        out.update({f"{key}_raw_image": raw["image"], f"{key}_raw_depth": raw["depth"], f"{key}_image": o["image"], f"{key}_depth": o["depth"],
                    f"{key}_pos": o["pos"]})

    # ---- a real NeRFGUI behind the stubbed window
    opt = types.SimpleNamespace(W=131, H=67, radius=2.5, fovy=50, test=False, max_spp=4, dt_gamma=0, max_steps=1024, bound=1,
                                workspace="/nonexistent", pretraining_epochs=0)
    g = gui.NeRFGUI(opt, trainer, trainer, train_loader=None, debug=False)
    g.dynamic_resolution = False
    for (H, W, ds) in ((67, 131, 0.5), (5, 7, 1)):
        o = frames[(H, W, ds, "srgb")]
        g.H, g.W = H, W
        for mode in ("image", "depth"):
            for K in (0, 1, 3):
                g.mode = mode
                g.state = gui.STATE_BRUSH if K else gui.STATE_PREVIEW
                ms = _masks(H, W, K, seed=10 * H + K)
                g.brush_mask, g.active_mask = ms[:-1], (ms[-1] if K else np.zeros((H, W, 1), dtype=np.uint8))
                p = g.prepare_buffer({"image": o["image"].copy(), "depth": o["depth"].copy()})
                key = f"prep_{H}x{W}_{mode}_k{K}"
                out[key] = np.ascontiguousarray(p, dtype=np.float32)
                assert p.dtype == np.float32, p.dtype
                if K:
                    out[f"prep_{H}x{W}_k{K}_masks"] = np.stack([m[:, :, 0] for m in ms])
    out["brush_color"] = g.brush_color.copy()
    # the accumulation line of test_step: three frames of the (67, 131) camera, jittered by spp
    g.H, g.W, g.mode, g.state = 67, 131, "image", gui.STATE_PREVIEW
    g.cam = types.SimpleNamespace(pose=view_pose, intrinsics=view_intr)  # (a dataset-style pose: not one OrbitCamera's setter takes)
    g.downscale, g.need_update, g.spp = 0.3, True, 1
    for n in range(3):
        torch.manual_seed(100 + n)
        g.test_step()
        out[f"accum_{n}_raw_image"], out[f"accum_{n}_raw_depth"] = raw["image"], raw["depth"]
        out[f"accum_{n}_buffer"] = np.ascontiguousarray(g.render_buffer, dtype=np.float32)
        assert g.render_buffer.dtype == np.float32 and g.spp == n + 1
    out["accum_camera_pose"], out["accum_camera_intrinsics"] = g.cam.pose.copy(), g.cam.intrinsics.copy()

    # ---- mask positions and the brush config
    g.H = g.W = None
    for H, W in POS:
        g.H, g.W = H, W
        g.cam = types.SimpleNamespace(pose=view_pose, intrinsics=view_intr * (H / 67))
        ms = _masks(H, W, 3, seed=77 + H)
        ms[1][:] = 0  # (an empty stroke in the middle)
        g.brush_mask = ms
        got = g.get_mask_pos(True)
        key = f"maskpos_{H}x{W}"
        out.update({f"{key}_masks": np.stack([m[:, :, 0] for m in ms]), f"{key}_rows": np.concatenate(got).astype(np.float32),
                    f"{key}_offsets": np.cumsum([0] + [len(p) for p in got]), f"{key}_pose": g.cam.pose.copy(),
                    f"{key}_intrinsics": g.cam.intrinsics.copy()})
    g.state = gui.STATE_BRUSH
    g.brush_config["brushType"] = ["line", "curve", "line"]
    g.brush_config["normal"] = [1.0, 2.0, -2.0]
    callbacks["_button_brush_config"](None, None)
    cfg = g.config
    out.update(cfg_raw_rows=np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in cfg["raw"]]),
               cfg_raw_offsets=np.cumsum([0] + [len(p) for p in cfg["raw"]]), cfg_rgb=np.asarray(cfg["rgb"], dtype=np.float64),
               cfg_normal=np.asarray(cfg["normal"], dtype=np.float64), cfg_brushType=np.array(cfg["brushType"]),
               cfg_strings=np.array([f"{k}={cfg[k]}" for k in ("type", "attenuationMode")]),
               cfg_numbers=np.array([cfg[k] for k in ("brushDepth", "brushPressure", "attenuationDistance", "simplifyVoxel")], dtype=np.float64),
               cfg_keys=np.array(sorted(cfg)))

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
    print("preview: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes, crc", zlib.crc32(buf.getvalue()))


if __name__ == "__main__":
    main()
