"""CPU: the headless preview (nerf/preview.py, sealnerf/preview.py) against tests/golden/preview.npz — outputs of the REFERENCE's
OrbitCamera, get_rays, Trainer.test_gui, NeRFGUI.prepare_buffer / test_step / get_mask_pos and callback_config_brush, executed by
tools/gen_preview_golden.py — and against the numpy / float64 witnesses of tests/preview_witness.py."""
import types

import numpy as np
import pytest
import torch

import preview_witness as pw


@pytest.fixture(scope="module")
def G():
    return pw.load()


def _run_script(G):
    from nerf.preview import OrbitCamera
    W, H, r, fovy = G["cam_init"]
    cam = OrbitCamera(int(W), int(H), r=float(r), fovy=float(fovy))
    poses, intrs = [cam.pose], [cam.intrinsics]
    for op, args in zip(G["cam_ops"], G["cam_args"]):
        if op == "set_pose":
            cam.pose = G["cam_set_pose"]
        elif op == "set_intrinsics":
            cam.intrinsics = G["cam_set_intrinsics"]
        elif op == "scale":
            cam.scale(args[0])
        elif op == "orbit":
            cam.orbit(args[0], args[1])
        else:
            cam.pan(*args)
        poses.append(cam.pose)
        intrs.append(cam.intrinsics)
    return cam, np.stack(poses), np.stack(intrs)


def test_camera_against_the_reference_and_the_witness(G):
    cam, poses, intrs = _run_script(G)
    assert poses.dtype == np.float32 and intrs.dtype == np.float64
    dev_pose, dev_intr = pw.camera_reference_deviation(G)
    e_ref = float(np.abs(poses - G["cam_poses"]).max())
    e_wit = float(np.abs(poses - pw.witness_camera(G)[0]).max())
    print(f"camera: reference vs float64 witness {dev_pose:.3e} (intrinsics, relative: {dev_intr:.3e}); build vs reference {e_ref:.3e}, "
          f"vs witness {e_wit:.3e}")
    assert dev_pose <= 1e-6, "the witness describes the reference"
    assert e_ref <= 1e-6 and e_wit <= 1e-6
    assert np.abs(intrs / G["cam_intrinsics"] - 1).max() <= 1e-12
    assert abs(cam.radius - float(G["cam_radius"])) <= 1e-12 and abs(cam.fovy - float(G["cam_fovy"])) <= 1e-9
    assert np.abs(cam.center - G["cam_center"]).max() <= 1e-6
    assert np.array_equal(poses[0, :3, :3], np.diag([1, -1, -1]).astype(np.float32)), "from_quat([1, 0, 0, 0])"


def test_camera_does_not_need_scipy():
    import nerf.preview as pv
    src = open(pv.__file__).read()
    assert "import scipy" not in src and "from scipy" not in src


@pytest.mark.parametrize("t, cur, want", [(800, 1, 0.5), (50, 0.5, 1), (180, 1, 1), (100000, 0.5, 0.25), (1, 1, 1), (1, 0.25, 1),
                                          (200 / 1.2 ** 2, 1, 1), (200 / 1.21 ** 2, 0.5, 0.5 * 1.21), (200 / 1.19 ** 2, 0.5, 0.5),
                                          (200 / 0.79 ** 2, 1, 0.79), (200 / 0.81 ** 2, 1, 1)])
def test_next_downscale(t, cur, want):
    """sqrt(200 / (t / d^2)) clamped to [1/4, 1]; taken only beyond 1.2 x or below 0.8 x the current value"""
    from nerf.preview import next_downscale
    assert next_downscale(t, cur) == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("t, cur, want", [(500, 16, 16), (1000, 16, 8), (10000, 16, 4), (10, 4, 16), (500 * 16 / 13.5, 16, 16),
                                          (500 * 16 / 12.5, 16, 12), (500 * 10 / 12.5, 10, 10), (500 * 10 / 13.5, 10, 13), (250, 8, 16),
                                          (500 * 10 / 8.5, 10, 10), (500 * 10 / 7.5, 10, 7)])
def test_next_train_steps(t, cur, want):
    """int(16 * 500 / (t / steps * 16)) = int(500 steps / t) clamped to [4, 16], with the same hysteresis"""
    from nerf.preview import next_train_steps
    assert next_train_steps(t, cur) == want


def test_frame_rays_torch_route_against_the_reference(G):
    from nerf.preview import frame_rays
    for pi in G["ray_poses"]:
        for rH, rW in ((5, 7), (20, 39), (67, 131)):
            key = f"rays_{pi}_{rH}x{rW}"
            if f"{key}_rays_d" not in G.files:
                continue
            ro, rd = frame_rays(G["cam_poses"][pi], G[f"{key}_intrinsics"], rH, rW, torch.device("cpu"), native=False)
            assert np.array_equal(ro[0].numpy(), G[f"{key}_rays_o"]) and np.array_equal(rd[0].numpy(), G[f"{key}_rays_d"]), key


class _Replay:
    """a trainer whose render returns the renderer output the reference's test_gui saw (recorded in the fixture)"""

    def __init__(self, G, key):
        self.image, self.depth = torch.from_numpy(G[f"{key}_raw_image"]), torch.from_numpy(G[f"{key}_raw_depth"])
        self.model = torch.nn.Linear(1, 1)
        self.calls = []

    def _preview_render(self, rays_o, rays_d, bg_color, perturb):
        self.calls.append((tuple(rays_o.shape), perturb))
        return {"image": self.image.reshape(1, -1, 3), "depth": self.depth.reshape(1, -1)}

    def test_gui(self, *a, **k):
        from nerf.trainer import Trainer
        return Trainer.test_gui(self, *a, **k)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("cs", ["srgb", "linear"])
def test_test_gui_torch_route_reproduces_the_reference_bit_for_bit(G, cs):
    for H, W, ds in G["tail_cases"]:
        H, W, ds = int(H), int(W), (int(ds) if ds == 1 else float(ds))
        key = f"tail_{H}x{W}_{ds}_{cs}"
        tr = _Replay(G, key)
        out = tr.test_gui(G["view_pose"], G["view_intrinsics"] * (H / 67), W, H, torch.ones(3), 1, ds, color_space=cs)
        assert tr.calls == [((1, int(H * ds) * int(W * ds), 3), False)]
        assert out["image"].shape == (H, W, 3) and out["depth"].shape == (H, W) and "pos" not in out
        assert _same(out["image"], G[f"{key}_image"]) and _same(out["depth"], G[f"{key}_depth"]), key
        assert np.isfinite(out["depth"].numpy()).all() and not np.isfinite(G[f"{key}_raw_depth"]).all()


def test_return_pos_and_its_guard(G):
    for H, W in ((5, 7), (20, 39)):
        key = f"pos_{H}x{W}"
        tr = _Replay(G, key)
        out = tr.test_gui(G["view_pose"], G["view_intrinsics"] * (H / 67), W, H, torch.ones(3), 1, 1, True)
        assert all(_same(out[k], G[f"{key}_{k}"]) for k in ("image", "depth", "pos")), key
    with pytest.raises(ValueError, match="downscale"):
        tr.test_gui(G["view_pose"], G["view_intrinsics"], 39, 20, None, 1, 0.5, True)
    with pytest.raises(ValueError, match="color_space"):
        tr.test_gui(G["view_pose"], G["view_intrinsics"], 39, 20, color_space="hsv")
    # spp is the jitter switch
    tr.calls.clear()
    tr.test_gui(G["view_pose"], G["view_intrinsics"], 39, 20, spp=5)
    assert tr.calls[0][1] == 5


def test_nearest_rule_against_interpolate():
    """min((int)floorf(dst * fl(in / out)), in - 1) is F.interpolate(mode='nearest') — the rule s3d_preview_resolve implements"""
    import torch.nn.functional as F
    for out in (4, 6, 64, 67, 128, 131, 800, 1080, 1920):
        for ds in (0.25, 0.3, 0.37, 0.5, 0.61, 0.8, 0.99, 1):
            inp = max(int(out * ds), 1)
            src = torch.arange(inp, dtype=torch.float32).view(1, 1, 1, inp)
            got = F.interpolate(src, size=(1, out), mode="nearest").view(-1).long().numpy()
            assert np.array_equal(got, pw.nearest_index(out, inp)), (out, inp)


def test_frame_preparation_reproduces_the_reference_bit_for_bit(G):
    from nerf.preview import prepare_torch
    color = G["brush_color"]
    for H, W, ds in ((67, 131, 0.5), (5, 7, 1)):
        img, dep = G[f"tail_{H}x{W}_{ds}_srgb_image"], G[f"tail_{H}x{W}_{ds}_srgb_depth"]
        for mode in ("image", "depth"):
            for K in (0, 1, 3):
                masks = G[f"prep_{H}x{W}_k{K}_masks"] if K else None
                got = prepare_torch(torch.from_numpy(img), torch.from_numpy(dep), mode, None if masks is None else torch.from_numpy(masks), color)
                want = G[f"prep_{H}x{W}_{mode}_k{K}"]
                assert got.dtype == torch.float32 and _same(got, want), (H, W, mode, K)
                assert _same(pw.prepare_numpy(img, dep, mode, masks, color), want), "the witness is the reference's expression"


@pytest.mark.parametrize("alpha", [1.0, 0.35])
def test_mix_brush_and_accumulate_against_numpy(alpha):
    from nerf.preview import accumulate_torch, mix_brush
    rng = np.random.RandomState(0)
    img = rng.rand(9, 13, 3).astype(np.float32) * 3 - 1
    masks = (rng.rand(3, 9, 13) < 0.3).astype(np.uint8) * rng.randint(1, 256, size=(3, 9, 13)).astype(np.uint8)
    masks[:, 0, 0] = (128, 128, 0)  # (a uint8 sum would wrap to 0 here; numpy sums in a wider type)
    color = np.array([0.9, 0.1, 0.3], dtype=np.float32)
    got = mix_brush(torch.from_numpy(img), torch.from_numpy(masks), torch.from_numpy(color), alpha)
    assert _same(got, pw.mix_brush_numpy(img, masks, color, alpha)) and got.dtype == torch.float32
    buf = rng.rand(9, 13, 3).astype(np.float32)
    for spp in (0, 1, 5, 63):
        acc = accumulate_torch(torch.from_numpy(buf), torch.from_numpy(img), spp)
        want = pw.accumulate_numpy(buf, img, spp)
        assert want.dtype == np.float32 and _same(acc, want), spp


def test_accumulation_of_test_step_against_the_reference(G):
    """three frames of NeRFGUI.test_step replayed: buffer after each"""
    from nerf.preview import PreviewSession
    tr = _Replay(G, "accum_0")
    s = PreviewSession(tr, 131, 67, max_spp=4, dynamic_resolution=False)
    s.cam = types.SimpleNamespace(pose=G["accum_camera_pose"], intrinsics=G["accum_camera_intrinsics"])
    s.downscale = 0.3
    for n in range(3):
        tr.image, tr.depth = torch.from_numpy(G[f"accum_{n}_raw_image"]), torch.from_numpy(G[f"accum_{n}_raw_depth"])
        assert s.step() and s.spp == n + 1
        assert _same(s.to_host(), G[f"accum_{n}_buffer"]), n
    assert [c[1] for c in tr.calls] == [False, False, 2], "perturb = False if spp == 1 else spp, with spp as it was BEFORE the frame"


def test_session_state_machine():
    from nerf.preview import PreviewSession

    class Flat(_Replay):
        def __init__(self):
            self.model, self.calls, self.value = torch.nn.Linear(1, 1), [], 0.0

        def _preview_render(self, rays_o, rays_d, bg_color, perturb):
            self.calls.append(perturb)
            n = rays_o.shape[1]
            return {"image": torch.full((1, n, 3), self.value), "depth": torch.full((1, n), 2.0)}
    tr = Flat()
    s = PreviewSession(tr, 12, 8, max_spp=3, dynamic_resolution=False)
    assert s.need_update and s.spp == 1 and s.buffer.shape == (8, 12, 3) and s.masks().shape == (0, 8, 12)
    tr.value = 1.0
    assert s.step() and not s.need_update and s.spp == 1 and float(s.buffer.mean()) == 1.0
    tr.value = 0.0
    assert s.step() and s.spp == 2 and float(s.buffer.mean()) == 0.5          # (1 * 1 + 0) / 2
    assert s.step() and s.spp == 3 and float(s.buffer.mean()) == pytest.approx(1 / 3, rel=1e-6)
    assert not s.step() and len(tr.calls) == 3, "the accumulation is full"
    m = s.stroke((2, 2), (9, 5), thickness=3)
    assert m.dtype == torch.uint8 and m.shape == (8, 12) and 0 < int(m.sum()) < 8 * 12 and m[2, 2] and m[5, 9] and not m[7, 0]
    assert s.need_update and len(s.brush_masks) == 1 and s.masks().shape == (1, 8, 12)
    tr.value = 0.25
    assert s.step() and s.spp == 1
    red = torch.tensor([1.0, 0.0, 0.0])
    assert torch.equal(s.buffer[m.bool()], red.expand(int(m.sum()), 3)) and float(s.buffer[~m.bool()].mean()) == 0.25
    s.set_mode("depth")
    assert s.need_update and s.step()
    assert float(s.buffer[~m.bool()].min()) == pytest.approx(2.0 / (2.0 + 1e-6), rel=1e-6)
    s.clear_strokes()
    assert s.need_update and not s.brush_masks and s.step() and float(s.buffer.min()) > 0.99
    with pytest.raises(ValueError):
        s.add_stroke(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        s.set_mode("normals")
    # dynamic resolution follows the measured time through next_downscale
    s2 = PreviewSession(tr, 12, 8, dynamic_resolution=True)
    s2.step()
    assert s2.downscale == 1 and s2.last_ms is not None  # (a frame this small never takes 200 ms / 1.2^2)


def test_mask_positions_torch_route_against_the_reference(G):
    from nerf.preview import mask_positions
    for H, W in ((5, 7), (20, 39)):
        key = f"maskpos_{H}x{W}"
        pos, masks = torch.from_numpy(G[f"pos_{H}x{W}_pos"]), torch.from_numpy(G[f"{key}_masks"])
        got = mask_positions(pos, masks, native=False)
        offs = G[f"{key}_offsets"]
        assert [len(p) for p in got] == np.diff(offs).tolist() and len(got[1]) == 0
        assert _same(torch.cat(got), G[f"{key}_rows"])


def test_brush_config_against_the_reference(G):
    from sealnerf.preview import BRUSH_DEFAULTS, SealSession
    H, W = 20, 39
    tr = _Replay(G, f"pos_{H}x{W}")
    s = SealSession(tr, W, H, dynamic_resolution=False)
    s.cam = types.SimpleNamespace(pose=G[f"maskpos_{H}x{W}_pose"], intrinsics=G[f"maskpos_{H}x{W}_intrinsics"])
    assert s.brush_config() is None
    for m, kind in zip(G[f"maskpos_{H}x{W}_masks"], G["cfg_brushType"]):
        s.add_stroke(m, brush_type=str(kind))
    cfg = s.brush_config(normal=[1.0, 2.0, -2.0])
    assert sorted(cfg) == G["cfg_keys"].tolist()
    offs = G["cfg_raw_offsets"]
    assert [len(p) for p in cfg["raw"]] == np.diff(offs).tolist()
    rows = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in cfg["raw"]])
    assert np.array_equal(rows, G["cfg_raw_rows"])
    assert cfg["rgb"] == G["cfg_rgb"].tolist() and np.array_equal(np.asarray(cfg["normal"]), G["cfg_normal"])
    assert cfg["brushType"] == G["cfg_brushType"].tolist()
    assert [f"{k}={cfg[k]}" for k in ("type", "attenuationMode")] == G["cfg_strings"].tolist()
    assert [cfg[k] for k in ("brushDepth", "brushPressure", "attenuationDistance", "simplifyVoxel")] == G["cfg_numbers"].tolist()
    assert BRUSH_DEFAULTS["normal"] == [1, 0, 0] and BRUSH_DEFAULTS["brushType"] == [], "the defaults are not written to"


def test_test_gui_renders_the_reference_frame_on_the_oracle(oracle_wrappers, G):
    """the whole method on the fixture's network (CPU oracle): the rendered frame is the reference's to summation-order noise
    (the bar of tests/test_seal_loop_golden.py), then the tail's bits follow from the tests above"""
    import zlib
    from nerf import network, synthetic as syn
    from nerf.trainer import Trainer
    from test_seal_loop_golden import NET, OPT, _seeded, relmax
    net = network.NeRFNetwork(**NET)
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    tr = Trainer(net, fp16=False)
    tr.render_kwargs.update(OPT)
    before = [p.detach().clone() for p in net.parameters()]
    out = tr.test_gui(G["view_pose"], G["view_intrinsics"], 131, 67, torch.ones(3), 1, 0.3)
    key = "tail_67x131_0.3_srgb"
    clean = np.isfinite(G[f"{key}_raw_depth"])  # (the fixture planted NaN / inf in three pixels of the rendered depth)
    src = np.ix_(pw.nearest_index(67, 20), pw.nearest_index(131, 39))
    ok = clean[src]
    assert relmax(out["image"].numpy(), G[f"{key}_image"]) < 1e-6
    assert relmax(out["depth"].numpy()[ok], G[f"{key}_depth"][ok]) < 1e-6
    assert all(torch.equal(a, b) for a, b in zip(before, net.parameters())) and not net.training
