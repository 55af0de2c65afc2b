"""GPU: the interactive preview on the HIP path — s3d_frame_rays (csrc/raysample.hip), s3d_preview_resolve and
s3d_mask_positions_* (csrc/preview.hip) against the reference's outputs (tests/golden/preview.npz) and against the torch route
of nerf/preview.py on the same inputs; Trainer.test_gui / train_gui on a tiny NGP model, the D-NeRF trainers, and a SealSession.

Bounds.  Frame rays: the bound tests/test_gpu_custom_pose.py derives for frame rays (its TOL = max(4 x the reference's own
deviation from the float64 witness, 2e-6) = 2e-6).  Resolve, `srgb` route: bit for bit (copies and individually rounded
operations).  Resolve, `linear` route: tests/preview_witness.py `linear_tolerance` — four times the error the torch fp32
sequence has against the float64 witness on the test's own colours, at least 2e-6; measured and printed by the test.
Mask positions: index for index."""
import types
import zlib

import numpy as np
import pytest
import torch

import custom_pose_witness as cw
import preview_witness as pw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return pw.load()


@pytest.fixture(scope="module")
def TOL():
    return cw.device_tolerance(cw.load())


def _rays(hip, pose, intr, rH, rW):
    ro = torch.full((rH * rW, 3), float("nan"), device="cuda")
    rd = torch.full((rH * rW, 3), float("nan"), device="cuda")
    hip.RaySampleBackend.frame_rays(np.asarray(pose, dtype=np.float32).reshape(-1).tolist(), intr, rH, rW, ro, rd)
    return ro, rd


# ---------------------------------------------------------------------------------------------------------------- frame rays
@pytest.mark.parametrize("frame", [(1, 1), (5, 7), (20, 39), (67, 131)], ids=lambda f: f"{f[0]}x{f[1]}")
def test_frame_rays_against_the_reference(hip, G, TOL, frame):
    rH, rW = frame
    for pi in G["ray_poses"]:
        pose = G["cam_poses"][pi]
        key = f"rays_{pi}_{rH}x{rW}"
        have = f"{key}_rays_d" in G.files
        intr = G[f"{key}_intrinsics"] if have else G["cam_intrinsics"][pi] * (rH / 67)
        ro, rd = _rays(hip, pose, intr, rH, rW)
        assert torch.equal(ro, torch.from_numpy(pose[:3, 3]).cuda().expand_as(ro)), "origins are the pose's translation"
        e_wit = float(np.abs(rd.cpu().numpy() - cw.witness_rays_d(pose[None].astype(np.float64), intr, rH, rW)[0]).max())
        print(f"{key}: rays_d vs float64 witness {e_wit:.3e} (bound {TOL:.1e})")
        assert e_wit <= TOL
        if have:
            e_d = float(np.abs(rd.cpu().numpy() - G[f"{key}_rays_d"]).max())
            e_o = float(np.abs(ro.cpu().numpy() - G[f"{key}_rays_o"]).max())
            print(f"{key}: rays_d vs reference {e_d:.3e}, rays_o {e_o:.3e}")
            assert e_d <= TOL and e_o == 0.0


def test_frame_rays_past_one_workgroups_share_and_the_orbit_kernels_bits(hip, TOL):
    """701 x 1003 pixels: 3 rH rW / 4 = 527,328 items, more than the 2,048 workgroups x 256 lanes of one pass (the item loop goes
    round), and 3 rH rW = 1 (mod 4): the last item is partial.  The rays are s3d_orbit_rays' for the same pose, bit for bit."""
    rH, rW = 701, 1003
    assert (3 * rH * rW) % 4 == 1 and (3 * rH * rW + 3) // 4 > 2048 * 256
    intr = np.array([900.0, 890.0, rW / 2, rH / 2])
    ro_o, rd_o = torch.empty(1, rH * rW, 3, device="cuda"), torch.empty(1, rH * rW, 3, device="cuda")
    poses = torch.empty(1, 4, 4, device="cuda")
    hip.RaySampleBackend.orbit_rays(1, rH, rW, intr, ro_o, rd_o, poses, radius=3.0, look_at=(0.25, -0.4, 1.5),
                                    u_pose=torch.tensor([[0.3, 0.8]], device="cuda"))
    guard = torch.full((rH * rW * 3 + 8,), 7.0, device="cuda")
    ro, rd = guard[:rH * rW * 3].view(-1, 3), torch.empty(rH * rW, 3, device="cuda")
    hip.RaySampleBackend.frame_rays(poses[0].cpu().numpy().reshape(-1).tolist(), intr, rH, rW, ro, rd)
    assert torch.equal(rd, rd_o[0]) and torch.equal(ro, ro_o[0])
    assert torch.equal(guard[rH * rW * 3:], torch.full((8,), 7.0, device="cuda")), "nothing is written past the frame"
    with pytest.raises(RuntimeError, match="must hold"):
        hip.RaySampleBackend.frame_rays([0.0] * 16, intr, 4, 4, ro, rd)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        hip.RaySampleBackend.frame_rays([0.0] * 16, intr, 4, 4, torch.zeros(49, device="cuda")[1:], torch.zeros(48, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- resolve
SHAPES = [((5, 7), (5, 7)), ((1, 1), (4, 6)), ((20, 39), (67, 131)), ((33, 65), (67, 131)), ((16, 32), (64, 128))]


def _inputs(src, dst, seed, depth_case="mixed"):
    g = torch.Generator().manual_seed(seed)
    (rH, rW), (H, W) = src, dst
    image = (torch.rand(rH, rW, 3, generator=g) * 1.4 - 0.1)
    image.view(-1)[:4] = torch.tensor([0.0031308, 0.0031307, 0.0, 1.0])[:min(4, image.numel())]
    depth = torch.rand(rH, rW, generator=g) * 5
    flat = depth.view(-1)
    if depth_case == "mixed" and flat.numel() >= 6:
        flat[0], flat[1], flat[2], flat[4] = float("nan"), float("inf"), float("-inf"), -0.0
    elif depth_case == "mixed":
        flat[0] = float("nan")
    elif depth_case == "max_last":
        flat[-1] = 9.5
    elif depth_case == "zero":
        depth.zero_()
    buffer = torch.rand(H, W, 3, generator=g)
    masks = (torch.rand(3, H, W, generator=g) < 0.3).to(torch.uint8) * 200
    masks[1].zero_()
    masks[0, -1, -1] = 1
    rays_o, rays_d = torch.rand(H * W, 3, generator=g) - 0.5, torch.rand(H * W, 3, generator=g) - 0.5
    return [t.cuda() for t in (image, depth, buffer, masks, rays_o, rays_d)]


def _both(hip, src, dst, to_srgb, mode, K, alpha, spp, depth_case="mixed", seed=0):
    from nerf.preview import resolve_frame
    (rH, rW), (H, W) = src, dst
    image, depth, buffer, masks, rays_o, rays_d = _inputs(src, dst, seed, depth_case)
    with_pos = (rH, rW) == (H, W)
    color = np.array([0.9, 0.2, 0.4], dtype=np.float32)
    outs = []
    for native in (True, False):
        buf = buffer.clone()
        display = dict(buffer=buf, spp=spp, mode=mode, masks=masks[:K].contiguous(), color=color, alpha=alpha)
        o = resolve_frame(image, depth, H, W, to_srgb, rays_o, rays_d, with_pos, native, display)
        o["buffer"] = buf
        outs.append(o)
    return outs, image


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resolve_srgb_route_is_the_torch_route_bit_for_bit(hip, shape):
    src, dst = shape
    n = 0
    for mode in ("image", "depth"):
        for K in (0, 1, 3):
            for alpha in (1.0, 0.35):
                for spp in (0, 1, 5):
                    if K == 0 and alpha != 1.0:
                        continue
                    (a, b), _ = _both(hip, src, dst, False, mode, K, alpha, spp, seed=n)
                    for k in a:
                        # (-0 and +0 are told apart: the comparison is on the bits, NaN never survives nan_to_num)
                        assert _bits(a[k], b[k]), (k, mode, K, alpha, spp)
                    assert torch.isfinite(a["depth"]).all() and ("pos" in a) == (src == dst)
                    n += 1


@pytest.mark.parametrize("depth_case", ["max_last", "zero"])
@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resolve_depth_mode_maximum(hip, shape, depth_case):
    """the maximum sits in the LAST source pixel (the last workgroup's last lane), or the frame is all zero (divisor 1e-6)"""
    src, dst = shape
    for K, spp in ((0, 0), (3, 5)):
        (a, b), _ = _both(hip, src, dst, False, "depth", K, 0.35, spp, depth_case)
        assert all(_bits(a[k], b[k]) for k in a)
        if depth_case == "max_last" and (K, spp) == (0, 0):
            assert float(a["buffer"].max()) == pytest.approx(9.5 / (9.5 + 1e-6), rel=1e-6)
        if depth_case == "zero" and (K, spp) == (0, 0):
            assert float(a["buffer"].abs().max()) == 0.0


def test_resolve_guards(hip):
    image, depth = torch.rand(3, 3, 3, device="cuda"), torch.rand(3, 3, device="cuda")
    with pytest.raises(RuntimeError, match="must fit"):
        hip.PreviewBackend.resolve(image, depth, 2, 2)
    with pytest.raises(RuntimeError, match="full resolution"):
        hip.PreviewBackend.resolve(image, depth, 6, 6, rays_o=torch.rand(36, 3, device="cuda"), rays_d=torch.rand(36, 3, device="cuda"),
                                   return_pos=True)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.PreviewBackend.resolve(image.cpu(), depth.cpu(), 3, 3)
    with pytest.raises(RuntimeError, match="mode"):
        hip.PreviewBackend.resolve(image, depth, 3, 3, buffer=torch.zeros(3, 3, 3, device="cuda"), mode="normals")
    fi, fd, pos = hip.PreviewBackend.resolve(image, depth, 3, 3)
    assert fi is image and torch.equal(fd, depth) and pos is None, "no upsampling, no conversion: the renderer's image is handed back"
    fi, _, _ = hip.PreviewBackend.resolve(image, depth, 3, 3, to_srgb=True)
    assert fi is not image and not torch.equal(fi, image)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resolve_linear_route_within_the_measured_bound(hip, shape):
    src, dst = shape
    for mode, K, alpha, spp in (("image", 0, 1.0, 0), ("image", 3, 0.35, 5), ("depth", 1, 1.0, 1)):
        (a, b), image = _both(hip, src, dst, True, mode, K, alpha, spp)
        from nerf.preview import linear_to_srgb
        tol, own = pw.linear_tolerance(image.cpu().numpy(), linear_to_srgb(image).cpu().numpy())
        e_img = float((a["image"] - b["image"]).abs().max())
        e_buf = float((a["buffer"] - b["buffer"]).abs().max())
        print(f"{src}->{dst} {mode} K={K}: torch fp32 vs float64 witness {own:.3e}, bound {tol:.3e}; device vs torch image {e_img:.3e}, "
              f"buffer {e_buf:.3e}")
        assert e_img <= tol and e_buf <= tol
        assert _bits(a["depth"], b["depth"]) and ("pos" not in a or _bits(a["pos"], b["pos"]))
        if mode == "depth":
            assert _bits(a["buffer"], b["buffer"]), "the depth view has no power in it"


def test_resolve_reproduces_the_reference_frames(hip, G):
    """the fixture's renderer outputs through the kernel: the reference's test_gui frames, prepare_buffer results and the
    three accumulated buffers of test_step, bit for bit (srgb)"""
    from nerf.preview import resolve_frame
    for H, W, ds in ((5, 7, 1), (67, 131, 0.3), (67, 131, 0.5)):
        key = f"tail_{H}x{W}_{ds}_srgb"
        raw_i, raw_d = torch.from_numpy(G[f"{key}_raw_image"]).cuda(), torch.from_numpy(G[f"{key}_raw_depth"]).cuda()
        o = resolve_frame(raw_i, raw_d, H, W, False, None, None, False, True)
        assert np.array_equal(o["image"].cpu().numpy(), G[f"{key}_image"]) and np.array_equal(o["depth"].cpu().numpy(), G[f"{key}_depth"])
        if (H, W, ds) in ((5, 7, 1), (67, 131, 0.5)):  # (the frames tools/gen_preview_golden.py hands to prepare_buffer)
            for mode in ("image", "depth"):
                for K in (0, 1, 3):
                    buf = torch.zeros(H, W, 3, device="cuda")
                    masks = torch.from_numpy(G[f"prep_{H}x{W}_k{K}_masks"]).cuda() if K else None
                    resolve_frame(raw_i, raw_d, H, W, False, None, None, False, True,
                                  dict(buffer=buf, spp=0, mode=mode, masks=masks, color=G["brush_color"]))
                    assert np.array_equal(buf.cpu().numpy(), G[f"prep_{H}x{W}_{mode}_k{K}"]), (H, W, mode, K)
    buf = torch.zeros(67, 131, 3, device="cuda")
    for n in range(3):
        resolve_frame(torch.from_numpy(G[f"accum_{n}_raw_image"]).cuda(), torch.from_numpy(G[f"accum_{n}_raw_depth"]).cuda(), 67, 131,
                      False, None, None, False, True, dict(buffer=buf, spp=n, mode="image", masks=None, color=G["brush_color"]))
        assert np.array_equal(buf.cpu().numpy(), G[f"accum_{n}_buffer"]), n
    for H, W in ((5, 7), (20, 39)):
        key = f"pos_{H}x{W}"
        ro, rd = _rays(hip, G["view_pose"], G["view_intrinsics"] * (H / 67), H, W)
        o = resolve_frame(torch.from_numpy(G[f"{key}_raw_image"]).cuda(), torch.from_numpy(G[f"{key}_raw_depth"]).cuda(), H, W, False,
                          ro, rd, True, True)
        want = ro.view(H, W, 3) + o["depth"].view(H, W, 1) * rd.view(H, W, 3)
        assert _bits(o["pos"], want)


# ---------------------------------------------------------------------------------------------------------------- mask positions
def _mask_cases(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    empty, full = torch.zeros(H, W, dtype=torch.uint8), torch.full((H, W), 255, dtype=torch.uint8)
    last = torch.zeros(H, W, dtype=torch.uint8)
    last[-1, -1] = 1
    rnd = (torch.rand(H, W, generator=g) < 0.3).to(torch.uint8) * 7
    rnd2 = (torch.rand(H, W, generator=g) < 0.3).to(torch.uint8)
    return {"empty": empty[None], "full": full[None], "last": last[None], "random": rnd[None], "three": torch.stack([rnd, empty, rnd2])}


# 1,200 x 1,200 x 3 masks = 3 x 352 workgroups of 4,096 pixels: more than one workgroup per mask in the count and emit launches
# (a mask's rows continue across workgroup sums), and 1,056 workgroup sums > the 1,024 the single scan workgroup takes per
# pass — that size is there for the SCAN phase's second pass.  67 x 131 = 8,777 pixels is three count / emit workgroups a mask
# with H W odd: masks 1 and 2 start off a 4-byte boundary (the byte path).
@pytest.mark.parametrize("size", [(5, 7), (67, 131), (1200, 1200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_positions_equal_numpy_boolean_indexing(hip, size):
    H, W = size
    g = torch.Generator().manual_seed(H)
    pos = torch.rand(H, W, 3, generator=g)
    pos_np, pos_d = pos.numpy(), pos.cuda()
    cases = _mask_cases(H, W, seed=W)
    if H * W > 100000:
        cases = {"three": cases["three"], "last": cases["last"]}
    for name, masks in cases.items():
        rows, offs = hip.PreviewBackend.mask_positions(masks.cuda(), pos_d)
        want = [pos_np[m.numpy() > 0] for m in masks]
        assert offs == np.cumsum([0] + [len(w) for w in want]).tolist(), name
        assert np.array_equal(rows.cpu().numpy(), np.concatenate(want)), name
        if name == "three":
            assert offs[1] == offs[2] and 0.25 * H * W < offs[1] < 0.35 * H * W or H * W < 100
    with pytest.raises(RuntimeError, match="masks"):
        hip.PreviewBackend.mask_positions(torch.zeros(0, H, W, dtype=torch.uint8, device="cuda"), pos_d)


def test_mask_positions_of_the_reference(hip, G):
    from nerf.preview import mask_positions
    for H, W in ((5, 7), (20, 39)):
        key = f"maskpos_{H}x{W}"
        got = mask_positions(torch.from_numpy(G[f"pos_{H}x{W}_pos"]).cuda(), torch.from_numpy(G[f"{key}_masks"]).cuda(), native=True)
        assert [len(p) for p in got] == np.diff(G[f"{key}_offsets"]).tolist()
        assert np.array_equal(torch.cat(got).cpu().numpy(), G[f"{key}_rows"])


# ---------------------------------------------------------------------------------------------------------------- end to end
def _ngp(seed_offset=0):
    """the tiny NGP model of tests/test_gpu_seal_loop.py (parameters seeded by name, lego-like occupancy), without a mapper"""
    from nerf import network, synthetic as syn
    from test_seal_loop_golden import NET, _seeded
    net = network.NeRFNetwork(**NET).cuda()
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000 + seed_offset, -0.5, 0.5))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    return net


def _view(H, W):
    from nerf import synthetic as syn
    return syn.orbit_poses(1, seed=0)[0].numpy(), syn.lego_intrinsics(H, W)


@pytest.mark.parametrize("downscale", [1, 0.5])
def test_test_gui_is_render_image_on_frame_rays_plus_the_torch_tail(hip, downscale):
    from nerf.preview import resolve_torch
    from nerf.trainer import Trainer
    from test_seal_loop_golden import OPT
    H, W = 48, 64
    net = _ngp()
    tr = Trainer(net, fp16=True)
    tr.render_kwargs.update(OPT)
    pose, intr = _view(H, W)
    params = [p.detach().clone() for p in net.parameters()]
    bits = net.density_bitfield.clone()
    out = tr.test_gui(pose, intr, W, H, downscale=downscale, return_pos=downscale == 1)
    rH, rW = int(H * downscale), int(W * downscale)
    ro, rd = _rays(hip, pose, intr * downscale, rH, rW)
    ref = tr.render_image(ro[None], rd[None])
    img, dep, pos = resolve_torch(ref["image"].reshape(rH, rW, 3).float(), ref["depth"].reshape(rH, rW).float(), H, W, False,
                                  ro, rd, downscale == 1)
    assert _bits(out["image"], img) and _bits(out["depth"], dep) and (downscale != 1 or _bits(out["pos"], pos))
    assert 0.05 < float((out["image"] < 0.99).float().mean()), "the view shows the scene, not only the background"
    assert all(torch.equal(a, b) for a, b in zip(params, net.parameters())) and torch.equal(bits, net.density_bitfield)
    with pytest.raises(ValueError, match="downscale"):
        tr.test_gui(pose, intr, W, H, downscale=0.5, return_pos=True)
    t = tr.test_gui(pose, intr, W, H, downscale=downscale, native=False)
    assert float((t["image"] - out["image"]).abs().max()) < 2e-2, "the torch route renders the same frame (its own rays: fp16 render noise)"


def _batches(net_device, n, num_rays):
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    poses = syn.orbit_poses(n, seed=1)
    g = torch.Generator().manual_seed(0)
    images = torch.rand(n, 32, 32, 3, generator=g)
    return NeRFDataset(images, poses, syn.lego_intrinsics(32, 32), num_rays=num_rays, device=net_device)


def test_graphed_trainer_trains_previews_and_trains_again_without_recapture(hip):
    from nerf.trainer import GraphedTrainer
    from test_seal_loop_golden import OPT
    net = _ngp()
    tr = GraphedTrainer(net, 256, fp16=True)
    tr.render_kwargs.update(OPT)
    ds = _batches("cuda", 3, 256)
    out = tr.train_gui(ds, step=20)
    assert np.isfinite(out["loss"]) and out["lr"] == tr.optimizer.param_groups[0]["lr"] and tr.global_step == 20
    assert tr.n_captures == 1 and tr.graph is not None
    pose, intr = _view(24, 32)
    a = tr.test_gui(pose, intr, 32, 24)
    assert not net.training and torch.isfinite(a["image"]).all()
    out = tr.train_gui(ds, step=6)
    assert tr.n_captures == 1 and tr.global_step == 26 and np.isfinite(out["loss"]), "the captured step replays unchanged"
    b = tr.test_gui(pose, intr, 32, 24)
    assert not torch.equal(a["image"], b["image"]), "six more steps moved the frame"


def test_spp_jitters_the_frame_and_the_buffer_follows_the_accumulate_rule(hip):
    from nerf.preview import PreviewSession
    from nerf.trainer import Trainer
    from test_seal_loop_golden import OPT
    net = _ngp()
    tr = Trainer(net, fp16=True)
    tr.render_kwargs.update(OPT)
    pose, intr = _view(24, 32)
    torch.manual_seed(0)
    f1 = tr.test_gui(pose, intr, 32, 24, spp=1)["image"]
    f2 = tr.test_gui(pose, intr, 32, 24, spp=2)["image"]
    assert torch.equal(f1, tr.test_gui(pose, intr, 32, 24, spp=1)["image"]) and not torch.equal(f1, f2)
    s = PreviewSession(tr, 32, 24, max_spp=4, dynamic_resolution=False)
    s.cam = types.SimpleNamespace(pose=pose, intrinsics=intr)
    want = None
    for n in range(4):
        assert s.step()
        frame = s.last_frame["image"]
        want = frame.clone() if n == 0 else (want * n + frame) / torch.full((), float(n + 1), device="cuda")
        assert _bits(s.buffer, want) and s.spp == n + 1
    assert not s.step() and torch.equal(s.last_frame["image"], frame)
    assert float((s.buffer - f1).abs().max()) < 0.5 and isinstance(s.to_host(), np.ndarray) and s.to_host().shape == (24, 32, 3)
    s.dynamic_resolution, s.need_update = True, True
    assert s.step() and s.downscale == 1 and s.last_ms > 0


# ---------------------------------------------------------------------------------------------------------------- D-NeRF
@pytest.mark.parametrize("backbone", ["deform", "basis", "hyper"])
def test_dnerf_test_gui_runs_and_depends_on_time(hip, backbone):
    from dnerf.utils import Trainer
    if backbone == "deform":
        from test_gpu_dnerf import _model
    elif backbone == "basis":
        from test_gpu_dnerf_basis import _model
    else:
        from test_gpu_dnerf_hyper import _model
    from nerf import synthetic as syn
    net = _model()
    net.density_bitfield.copy_(torch.from_numpy(syn.lego_like_density_grid(seed=0)[1]).cuda().expand_as(net.density_bitfield))
    tr = Trainer(net, fp16=True)
    pose, intr = _view(16, 24)
    params = [p.detach().clone() for p in net.parameters()]
    torch.manual_seed(0)
    a = tr.test_gui(pose, intr, 24, 16, time=0.1)
    torch.manual_seed(0)
    b = tr.test_gui(pose, intr, 24, 16, time=0.9, downscale=1)
    torch.manual_seed(0)
    a2 = tr.test_gui(pose, intr, 24, 16, time=0.1)
    assert a["image"].shape == (16, 24, 3) and a["depth"].shape == (16, 24) and "pos" not in a
    assert torch.isfinite(a["image"]).all() and torch.isfinite(a["depth"]).all()
    assert torch.equal(a["image"], a2["image"]) and not torch.equal(a["image"], b["image"]), "two times, two frames"
    assert all(torch.equal(p, q) for p, q in zip(params, net.parameters()))
    with pytest.raises(TypeError):
        tr.test_gui(pose, intr, 24, 16, return_pos=True)


# ---------------------------------------------------------------------------------------------------------------- SealSession
def test_seal_session_paint_distil_look_reset(hip):
    from nerf.trainer import Trainer
    from sealnerf import SealDataset, SealSession, SealTrainer, make_student, make_teacher
    from test_seal_loop_golden import NET, OPT, _seeded
    from nerf import network, synthetic as syn

    def net(make):
        m = make(network.NeRFNetwork, **NET).cuda()
        for k, p in m.named_parameters():
            p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
        dens, bits = syn.lego_like_density_grid(seed=0)
        m.density_grid.copy_(torch.from_numpy(dens))
        m.density_bitfield.copy_(torch.from_numpy(bits))
        return m
    teacher, student = net(make_teacher), net(make_student)
    teacher.eval()
    tr = SealTrainer(student, teacher, lr=1e-2, fp16=True)
    tr.render_kwargs.update(OPT)
    teacher_tr = Trainer(teacher, fp16=True)
    teacher_tr.render_kwargs.update(OPT)
    H, W = 32, 40
    ds = SealDataset(syn.orbit_poses(2, seed=0).cuda(), syn.lego_intrinsics(H, W), H, W, num_rays=128, render_kwargs=OPT)
    s = SealSession(tr, W, H, dataset=ds, teacher_trainer=teacher_tr, dynamic_resolution=False, max_spp=1)
    s.cam = types.SimpleNamespace(pose=syn.orbit_poses(1, seed=0)[0].numpy(), intrinsics=syn.lego_intrinsics(H, W))
    assert s.step()
    before = s.last_frame
    # 1. paint where the view shows the scene
    hit = (before["image"] < 0.95).any(-1)
    ys, xs = torch.nonzero(hit, as_tuple=True)
    cy, cx = int(ys.float().median()), int(xs.float().median())
    mask = s.stroke((cx - 5, cy), (cx + 5, cy), thickness=6)
    painted = mask.bool() & hit
    assert int(painted.sum()) > 10
    assert s.step() and torch.equal(s.buffer[mask.bool()], torch.tensor([1.0, 0, 0], device="cuda").expand(int(mask.sum()), 3))
    # 2. positions -> config -> mapper + pretraining sets
    pts = s.mask_positions(cluster=True)
    assert len(pts) == 1 and pts[0].shape == (int(mask.sum()), 3) and torch.isfinite(pts[0]).all()
    cfg = s.brush_config(brushDepth=0.1, brushPressure=0.05, simplifyVoxel=8)
    assert cfg["type"] == "brush" and len(cfg["raw"]) == 1 and cfg["rgb"] == [1.0, 0.0, 0.0] and cfg["brushType"] == ["line"]
    s.begin_edit(epochs=2, batch_size=1 << 20, lr=0.05, local_point_step=0.02, local_angle_step=90, seed=0)
    assert student.seal_mapper is teacher.seal_mapper is not None and s.is_pretraining and not s.brush_masks
    assert "local" in tr.pretraining_data and tr.pretraining_data["local"]["points"].shape[0] > 0
    # 3. two pretraining epochs, then four fine-tuning steps
    o = s.train(2)
    assert np.isfinite(o["loss"]) and not s.is_pretraining and s.trained_steps == 2 and tr.global_step == 0
    o = s.train(4)
    assert np.isfinite(o["loss"]) and tr.global_step == 4 and s.need_update
    # 4. the student's frame differs inside the painted region from the teacher's — the teacher's weights without the edit's
    #    proxy: the scene as it was (with the proxy on, the teacher trainer shows the target the student is distilled towards)
    assert s.step()
    after = s.last_frame["image"]
    s.render_trainer, s.need_update = teacher_tr, True
    assert s.step()
    target = s.last_frame["image"]
    teacher.proxy_enabled = False
    s.need_update = True
    assert s.step()
    t_frame = s.last_frame["image"]
    d_in = float((after - t_frame).abs()[painted].mean())
    print(f"seal session: mean |student - teacher| inside the stroke {d_in:.4f}; target vs teacher {float((target - t_frame).abs()[painted].mean()):.4f}")
    assert d_in > 1e-3 and not torch.equal(target, t_frame)
    # 5. reset: the student is the teacher again, and renders its frame
    s.render_trainer = tr
    s.reset()
    assert all(torch.equal(p, q) for p, q in zip(student.parameters(), teacher.parameters())) and s.need_update
    assert s.step() and torch.equal(s.last_frame["image"], t_frame)
    teacher.proxy_enabled = True
    s.commit()
    assert teacher.seal_mapper is None and student.seal_mapper is None and not teacher.density_bitfield_hacked
