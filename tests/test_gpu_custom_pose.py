"""GPU: Seal-3D's custom-pose fine-tuning (`--custom_pose`) on the HIP path — `s3d_orbit_rays` (csrc/raysample.hip) against
the reference's `rand_poses` / `get_rays` outputs (tests/golden/custom_pose.npz), the float64 witness and the sampler's own ray
code; the counter-hash draw; graph capture; `SealRandomDataset.sample` feeding both Seal trainers.

Tolerance of poses and rays (tests/custom_pose_witness.py: measured, not picked): the reference's fp32 results deviate from
the float64 witness by at most 1.49e-07 over the fixture (translations divided by the radius); the device gets four times
that, never less than the 2e-6 of the project's fp32 trigonometric kernels: TOL = max(4 x 1.49e-07, 2e-6) = 2e-6."""
import math

import numpy as np
import pytest
import torch

import custom_pose_witness as cw

pytestmark = pytest.mark.gpu

LOOK = (0.25, -0.4, 1.5)


@pytest.fixture(scope="module")
def G():
    return cw.load()


@pytest.fixture(scope="module")
def TOL(G):
    return cw.device_tolerance(G)


def _intrinsics(G, rH, rW):
    for tag in cw.POSE_CASES:
        if f"{tag}_{rH}x{rW}_intrinsics" in G.files:
            return G[f"{tag}_{rH}x{rW}_intrinsics"]
    return np.array([1.3, 1.1, 0.5, 0.5]) * max(rH, rW)


def _orbit(hip, B, rH, rW, intr, **kw):
    dev = "cuda"
    ro, rd = torch.full((B, rH * rW, 3), float("nan"), device=dev), torch.full((B, rH * rW, 3), float("nan"), device=dev)
    poses = torch.full((B, 4, 4), float("nan"), device=dev)
    hip.RaySampleBackend.orbit_rays(B, rH, rW, intr, ro, rd, poses, **kw)
    return poses, ro, rd


def _sampler_rays(hip, poses, rH, rW, intr, N):
    """the sampler's uniform-pixel draw on `poses` as its pose set: rays and the pixels they belong to"""
    B = poses.shape[0]
    ro, rd = torch.empty(B, N, 3, device="cuda"), torch.empty(B, N, 3, device="cuda")
    inds = torch.empty(B, N, dtype=torch.int64, device="cuda")
    hip.RaySampleBackend.sample_train_rays(None, torch.arange(B, device="cuda"), N, rH, rW, poses.contiguous(), intr, ro, rd, inds,
                                           seed=7, ctl=torch.zeros(2, dtype=torch.int32, device="cuda"))
    return ro, rd, inds


@pytest.mark.parametrize("frame", [(1, 1), (5, 7), (67, 131)], ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tag", cw.POSE_CASES)
def test_explicit_uniforms_against_golden_witness_and_sampler(hip, G, TOL, tag, frame):
    rH, rW = frame
    radius, B = float(G[f"{tag}_radius"]), G[f"{tag}_u"].shape[0]
    intr = _intrinsics(G, rH, rW)
    ctl = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    poses, ro, rd = _orbit(hip, B, rH, rW, intr, radius=radius, theta_range=tuple(G[f"{tag}_theta_range"]),
                           phi_range=tuple(G[f"{tag}_phi_range"]), u_pose=torch.from_numpy(G[f"{tag}_u"]).cuda(), ctl=ctl)
    assert ctl.tolist() == [5, 5], "explicit uniforms leave ctl alone"
    # poses: the reference's, and the witness
    W = cw.witness_poses(G[f"{tag}_thetas"], G[f"{tag}_phis"], radius)
    e_ref = cw.scaled_pose_error(poses.cpu().numpy(), G[f"{tag}_poses"].astype(np.float64), radius)
    e_wit = cw.scaled_pose_error(poses.cpu().numpy(), W, radius)
    print(f"{tag} {rH}x{rW}: pose error vs reference {e_ref:.3e}, vs witness {e_wit:.3e} (bound {TOL:.1e})")
    assert e_ref <= TOL and e_wit <= TOL
    assert torch.equal(poses[:, 3], torch.tensor([0.0, 0, 0, 1], device="cuda").expand(B, 4))
    # origins: exactly the written translation
    assert torch.equal(ro, poses[:, None, :3, 3].expand_as(ro))
    # directions: bit for bit what the sampler forms for the same pose, intrinsics and pixel
    N = min(4 * rH * rW, 16384)
    s_ro, s_rd, inds = _sampler_rays(hip, poses, rH, rW, intr, N)
    assert int(inds.min()) >= 0 and int(inds.max()) < rH * rW
    if rH * rW > 1:
        assert inds.unique().numel() > 0.7 * rH * rW  # (4 draws a pixel, 16,384 at the most: 1 - e^-1.87 = 0.85 of the frame)
    pick = inds[..., None].expand(B, N, 3)
    assert torch.equal(s_rd, rd.gather(1, pick)) and torch.equal(s_ro, ro.gather(1, pick))
    # directions: the witness's, and — where the fixture holds the frame — the reference's get_rays
    e_wit = float(np.abs(rd.cpu().numpy() - cw.witness_rays_d(poses.cpu().numpy(), intr, rH, rW)).max())
    e_chain = float(np.abs(rd.cpu().numpy() - cw.witness_rays_d(W, intr, rH, rW)).max())
    print(f"{tag} {rH}x{rW}: rays_d vs witness on the written pose {e_wit:.3e}, on the witness pose {e_chain:.3e}")
    assert e_wit <= TOL and e_chain <= TOL
    key = f"{tag}_{rH}x{rW}"
    if f"{key}_rays_d" in G.files:
        e_d = float(np.abs(rd.cpu().numpy() - G[f"{key}_rays_d"]).max())
        e_o = float(np.abs(ro.cpu().numpy() - G[f"{key}_rays_o"]).max()) / radius
        print(f"{key}: rays_d vs reference {e_d:.3e}, rays_o / radius {e_o:.3e}")
        assert e_d <= TOL and e_o <= TOL


def test_look_at_moves_the_origin_only(hip, G, TOL):
    u = torch.from_numpy(G["b_u"]).cuda()
    kw = dict(radius=2.5, theta_range=tuple(G["b_theta_range"]), phi_range=tuple(G["b_phi_range"]), u_pose=u)
    intr = _intrinsics(G, 5, 7)
    p0, ro0, rd0 = _orbit(hip, 3, 5, 7, intr, **kw)
    p1, ro1, rd1 = _orbit(hip, 3, 5, 7, intr, look_at=LOOK, **kw)
    assert torch.equal(rd0, rd1) and torch.equal(p0[:, :3, :3], p1[:, :3, :3])
    assert torch.equal(p1[:, :3, 3], p0[:, :3, 3] + torch.tensor(LOOK, device="cuda"))  # the fp32 sum
    assert torch.equal(ro1, p1[:, None, :3, 3].expand_as(ro1))
    from nerf.synthetic import rand_poses
    torch.manual_seed(int(G["b_seed"]))
    host = rand_poses(3, "cpu", radius=2.5, theta_range=tuple(G["b_theta_range"]), phi_range=tuple(G["b_phi_range"]), look_at=torch.tensor(LOOK))
    assert cw.scaled_pose_error(p1.cpu().numpy(), host.double().numpy(), 2.5) <= TOL


def test_a_frame_past_the_workgroup_cap_and_unaligned_poses(hip, TOL):
    """297 x 295 pixels: more groups of four floats than 256 workgroups x 256 lanes (the item loop goes round), and
    3 rH rW = 1 (mod 4), so the second and third pose start off a 16-byte boundary (their first and last items are partial)"""
    from nerf.synthetic import get_rays
    rH, rW, B = 297, 295, 3
    assert (3 * rH * rW) % 4 == 1 and 3 * rH * rW // 4 > 256 * 256
    intr = np.array([410.0, 405.0, rW / 2, rH / 2])
    u = torch.tensor([[0.1, 0.7], [0.5, 0.2], [0.9, 0.95]], device="cuda")
    poses, ro, rd = _orbit(hip, B, rH, rW, intr, radius=3.0, look_at=LOOK, u_pose=u)
    assert torch.equal(ro, poses[:, None, :3, 3].expand_as(ro))
    ref = get_rays(poses, intr, rH, rW, -1)["rays_d"]  # torch on the device: same expressions, its own rounding
    assert float((rd - ref).abs().max()) <= TOL
    s_ro, s_rd, inds = _sampler_rays(hip, poses, rH, rW, intr, 16384)
    edge = torch.tensor([0, 1, 2, rH * rW - 3, rH * rW - 2, rH * rW - 1], device="cuda")  # + the pixels of the partial items
    pick = inds[..., None].expand(B, -1, 3)
    assert torch.equal(s_rd, rd.gather(1, pick))
    assert float((rd[:, edge] - ref[:, edge]).abs().max()) <= TOL


def _recover(poses, radius, look=(0.0, 0.0, 0.0)):
    c = (poses[:, :3, 3].double().cpu().numpy() - np.asarray(look)) / radius
    return np.arccos(np.clip(c[:, 1], -1, 1)), np.mod(np.arctan2(c[:, 0], c[:, 2]), 2 * math.pi)


@pytest.mark.parametrize("ranges", [((math.pi / 3, 2 * math.pi / 3), (0.0, 2 * math.pi)), ((0.3, 2.6), (0.5, 4.0))], ids=["default", "b"])
def test_hash_route_draws(hip, TOL, ranges):
    B, (tr, pr) = 4096, ranges
    kw = dict(radius=2.0, theta_range=tr, phi_range=pr, look_at=LOOK, seed=11)
    ctl = torch.zeros(2, dtype=torch.int32, device="cuda")
    p0, ro0, rd0 = _orbit(hip, B, 1, 1, (1.0, 1.0, 0.5, 0.5), ctl=ctl, **kw)
    assert ctl.tolist() == [1, 0], "one launch advances the step by one"
    p1, _, _ = _orbit(hip, B, 1, 1, (1.0, 1.0, 0.5, 0.5), ctl=ctl, **kw)
    assert ctl.tolist() == [2, 0]
    assert torch.isfinite(p0).all() and torch.isfinite(rd0).all() and torch.equal(ro0[:, 0], p0[:, :3, 3])
    # angles recovered from the centre: arccos and arctan2 magnify an error of the centre by 1 / sin(theta) <= 1 / sin(0.3) < 4
    th, ph = _recover(p0, 2.0, LOOK)
    slack = 4 * TOL
    assert th.min() >= tr[0] - slack and th.max() <= tr[1] + slack
    assert ph.min() >= pr[0] - slack and ph.max() <= pr[1] + slack
    assert np.unique(p0.cpu().numpy().reshape(B, -1), axis=0).shape[0] == B, "no two poses are equal"
    # five standard deviations of the mean of 4,096 uniforms: 5 / sqrt(12 x 4096) = 0.0226
    bound = 5 / math.sqrt(12 * B)
    u_t, u_p = (th - tr[0]) / (tr[1] - tr[0]), (ph - pr[0]) / (pr[1] - pr[0])
    print(f"mean u_theta {u_t.mean():.4f}, mean u_phi {u_p.mean():.4f} (0.5 +- {bound:.4f})")
    assert abs(u_t.mean() - 0.5) <= bound and abs(u_p.mean() - 0.5) <= bound
    assert abs(np.corrcoef(u_t, u_p)[0, 1]) <= 5 / math.sqrt(B), "theta and phi are keyed apart"
    assert not torch.equal(p0, p1), "two consecutive launches differ"
    # the same seed and step: the same poses; another seed: others
    again, _, _ = _orbit(hip, B, 1, 1, (1.0, 1.0, 0.5, 0.5), ctl=torch.zeros(2, dtype=torch.int32, device="cuda"), **kw)
    assert torch.equal(again, p0)
    step1, _, _ = _orbit(hip, B, 1, 1, (1.0, 1.0, 0.5, 0.5), ctl=torch.tensor([1, 0], dtype=torch.int32, device="cuda"), **kw)
    assert torch.equal(step1, p1)
    other, _, _ = _orbit(hip, B, 1, 1, (1.0, 1.0, 0.5, 0.5), ctl=torch.zeros(2, dtype=torch.int32, device="cuda"), **dict(kw, seed=12))
    assert not torch.equal(other, p0)


def test_many_workgroups_advance_the_step_once(hip):
    """67 x 131 x 3 poses = 78 workgroups: the last one to finish advances ctl[0], and every one drew at the same step"""
    ctl = torch.tensor([40, 0], dtype=torch.int32, device="cuda")
    intr = (120.0, 118.0, 65.5, 33.5)
    for k in range(3):
        poses, ro, rd = _orbit(hip, 3, 67, 131, intr, radius=1.5, seed=3, ctl=ctl)
        assert ctl.tolist() == [41 + k, 0]
        one, _, _ = _orbit(hip, 3, 1, 1, intr, radius=1.5, seed=3, ctl=torch.tensor([40 + k, 0], dtype=torch.int32, device="cuda"))
        assert torch.equal(one, poses) and torch.equal(ro, poses[:, None, :3, 3].expand_as(ro)) and torch.isfinite(rd).all()


def test_captured_launch_draws_a_fresh_pose_on_every_replay(hip):
    rH, rW, intr = 8, 8, (11.0, 11.0, 4.0, 4.0)
    kw = dict(radius=1.2, look_at=LOOK, seed=21)
    ctl = torch.tensor([7, 0], dtype=torch.int32, device="cuda")
    poses, ro, rd = (torch.zeros(1, 4, 4, device="cuda"), torch.zeros(1, 64, 3, device="cuda"), torch.zeros(1, 64, 3, device="cuda"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.RaySampleBackend.orbit_rays(1, rH, rW, intr, ro, rd, poses, ctl=ctl, **kw)
    assert ctl.tolist() == [7, 0], "a capture does not execute"
    replayed = []
    for _ in range(3):
        g.replay()
        replayed.append((poses.clone(), ro.clone(), rd.clone()))
    assert ctl.tolist() == [10, 0]
    ctl2 = torch.tensor([7, 0], dtype=torch.int32, device="cuda")
    for k in range(3):
        e = _orbit(hip, 1, rH, rW, intr, ctl=ctl2, **kw)
        assert all(torch.equal(a, b) for a, b in zip(replayed[k], e)), k
    assert not torch.equal(replayed[0][0], replayed[1][0]) and not torch.equal(replayed[1][0], replayed[2][0]) \
        and not torch.equal(replayed[0][0], replayed[2][0])


def test_guards(hip):
    ctl = torch.zeros(2, dtype=torch.int32, device="cuda")
    e3 = torch.empty(0, 3, device="cuda")
    hip.RaySampleBackend.orbit_rays(0, 4, 4, (1, 1, 2, 2), e3, e3, None, ctl=ctl)      # B = 0
    hip.RaySampleBackend.orbit_rays(2, 0, 4, (1, 1, 2, 2), e3, e3, None, ctl=ctl)      # an empty frame
    assert ctl.tolist() == [0, 0], "nothing was launched"
    ro, rd = torch.zeros(1, 16, 3, device="cuda"), torch.zeros(1, 16, 3, device="cuda")
    with pytest.raises(RuntimeError, match="ctl or the explicit uniforms"):
        hip.RaySampleBackend.orbit_rays(1, 4, 4, (1, 1, 2, 2), ro, rd)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        hip.RaySampleBackend.orbit_rays(1, 4, 4, (1, 1, 2, 2), torch.zeros(49, device="cuda")[1:], rd, ctl=ctl)
    with pytest.raises(RuntimeError, match="finite"):
        hip.RaySampleBackend.orbit_rays(1, 4, 4, (1, 1, 2, 2), ro, rd, ctl=ctl, radius=float("nan"))
    with pytest.raises(RuntimeError, match="must hold"):
        hip.RaySampleBackend.orbit_rays(2, 4, 4, (1, 1, 2, 2), ro, rd, ctl=ctl)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.RaySampleBackend.orbit_rays(1, 4, 4, (1, 1, 2, 2), ro.cpu(), rd, ctl=ctl)
    assert ctl.tolist() == [0, 0] and float(ro.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- trainers
def _pair():
    """tiny NGP teacher + student and a bbox mapper, built as tests/test_gpu_seal_loop.py builds them"""
    from sealnerf import make_student, make_teacher
    from test_gpu_seal_loop import case_mapper, golden_network
    mapper = case_mapper("both_color")
    teacher = golden_network(make_teacher, mapper, "cuda")
    student = golden_network(make_student, teacher.seal_mapper, "cuda")
    teacher.train()  # (the one-march proxy branch: the one GraphedSealTrainer replays from its graph)
    return teacher, student, mapper


def _dataset(mapper, **kw):
    from nerf import synthetic as syn
    from sealnerf import SealRandomDataset
    ds = SealRandomDataset(mapper, syn.lego_intrinsics(16, 16), 16, 16, num_rays=64, device="cuda", **kw)
    assert (ds.H, ds.W, ds.rays_per_batch) == ((8, 8, 64) if ds.training else (16, 16, 256))
    return ds


def test_sample_matches_collate_on_its_own_poses(hip, TOL):
    from nerf.synthetic import get_rays
    _, _, mapper = _pair()
    ds = _dataset(mapper, seed=4)
    b = ds.sample([0, 1])
    assert b["H"] == 8 and b["W"] == 8 and b["rays_o"].shape == (2, 64, 3) and b["poses"].shape == (2, 4, 4) and "images_shape" not in b
    r = get_rays(b["poses"], ds.intrinsics, 8, 8, -1)
    assert torch.equal(b["rays_o"], r["rays_o"]) and float((b["rays_d"] - r["rays_d"]).abs().max()) <= TOL
    c = (b["poses"][:, :3, 3] - ds.look_at).norm(dim=-1) / ds.radius
    assert float((c - 1).abs().max()) <= 4 * TOL
    assert not torch.equal(ds.sample([0, 1])["poses"], b["poses"]) and ds._ctl.tolist() == [2, 0]
    val = _dataset(mapper, training=False)
    v = val.sample([0])
    assert (v["H"], v["W"]) == (16, 16) and v["images_shape"] == [1, 16, 16, 3] and v["rays_d"].shape == (1, 256, 3)


@pytest.mark.parametrize("route", ["sample", "collate"])
def test_eager_seal_trainer_trains_on_a_custom_pose_batch(hip, route):
    from sealnerf import SealTrainer
    from test_gpu_seal_loop import OPT
    teacher, student, mapper = _pair()
    tr = SealTrainer(student, teacher, lr=1e-2, fp16=True)
    tr.render_kwargs.update(OPT)
    ds = _dataset(mapper)
    before = student.encoder.embeddings.detach().clone()
    b = ds.sample([0]) if route == "sample" else ds.collate([0])
    assert b["rays_o"].shape == (1, 64, 3)
    loss = float(tr.train_step(b["rays_o"].contiguous(), b["rays_d"].contiguous()))
    assert np.isfinite(loss) and not torch.equal(before, student.encoder.embeddings)


def test_graphed_custom_pose_steps_match_the_eager_trainer(hip):
    """three train_step_random steps: three different poses, and the losses of an eager SealTrainer stepped on the same three
    ray batches (read back from s_ro / s_rd after each step).  Tolerance: the project's bar for graphed-against-eager Seal
    fine-tuning steps, rtol = 0.5 (tests/test_gpu_configs.py:114, `np.testing.assert_allclose(hist, hist_e, rtol=0.5)`)."""
    from sealnerf import GraphedSealTrainer, SealTrainer
    from test_gpu_seal_loop import OPT
    teacher, student, mapper = _pair()
    tr = GraphedSealTrainer(student, teacher, 64, lr=1e-2, fp16=True)
    tr.render_kwargs.update(OPT)
    ds = _dataset(mapper)
    torch.manual_seed(0)
    hist, batches, poses = [], [], []
    for _ in range(3):
        hist.append(float(tr.train_step_random(ds)))
        batches.append((tr.s_ro.clone(), tr.s_rd.clone(), tr.s_gt.clone(), tr.s_depth.clone()))
        poses.append(tr.s_poses.clone())
    assert tr.proxy_graph is not None, "the teacher's proxy render was replayed from its graph"
    assert not any(torch.equal(poses[i], poses[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    for (ro, rd, _, _), p in zip(batches, poses):
        assert torch.equal(ro, p[0, :3, 3].expand_as(ro)) and float((rd.norm(dim=-1) - 1).abs().max()) < 1e-5
    teacher_e, student_e, _ = _pair()
    tr_e = SealTrainer(student_e, teacher_e, lr=1e-2, fp16=True)
    tr_e.render_kwargs.update(OPT)
    torch.manual_seed(0)
    hist_e = []
    for ro, rd, gt, dep in batches:
        rgb_e, dep_e = tr_e.proxy_truth(ro, rd)
        # (the proxy is deterministic, perturb=False: the graphed targets are the eager ones)
        assert float((rgb_e.reshape(-1, 3) - gt).abs().max()) <= 1e-4 and float((dep_e.reshape(-1) - dep).abs().max()) <= 1e-4 * max(1.0, float(dep.abs().max()))
        hist_e.append(float(tr_e.train_step(ro, rd)))
    print("graphed", hist, "eager", hist_e)
    assert np.isfinite(hist).all() and np.isfinite(hist_e).all()
    np.testing.assert_allclose(hist, hist_e, rtol=0.5)


def test_graphed_custom_pose_steps_replay_without_host_copies(hip, monkeypatch):
    """past the 16 eager steps that gather sample statistics the student's step is captured: from then on a step is the
    sampler launch and two replays, with no staging copy in between"""
    from sealnerf import GraphedSealTrainer
    from test_gpu_seal_loop import OPT
    teacher, student, mapper = _pair()
    tr = GraphedSealTrainer(student, teacher, 64, lr=1e-2, fp16=True)
    tr.render_kwargs.update(OPT)
    ds = _dataset(mapper)
    hist = [float(tr.train_step_random(ds)) for _ in range(20)]
    assert tr.n_captures >= 1 and tr.proxy_graph is not None and np.isfinite(hist).all()
    calls, orig = [], torch._foreach_copy_
    monkeypatch.setattr(torch, "_foreach_copy_", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    seen = []
    for _ in range(4):
        hist.append(float(tr.train_step_random(ds)))
        seen.append(tr.s_poses.clone())
    monkeypatch.undo()
    assert not calls and np.isfinite(hist).all() and ds._ctl.tolist() == [24, 0]
    assert len({tuple(p.flatten().tolist()) for p in seen}) == 4


def test_eager_proxy_fallback_and_ray_count_mismatch(hip):
    from sealnerf import GraphedSealTrainer
    from test_gpu_seal_loop import OPT
    teacher, student, mapper = _pair()
    teacher.eval()  # (main_SealNeRF.py:210: the inference-loop proxy has data-dependent extents — rendered eagerly)
    tr = GraphedSealTrainer(student, teacher, 64, lr=1e-2, fp16=True)
    tr.render_kwargs.update(OPT)
    ds = _dataset(mapper)
    loss = float(tr.train_step_random(ds))
    assert np.isfinite(loss) and tr.proxy_graph is None and not teacher.training
    assert torch.equal(tr.s_ro, tr.s_poses[0, :3, 3].expand_as(tr.s_ro))
    teacher2, student2, _ = _pair()
    tr128 = GraphedSealTrainer(student2, teacher2, 128, lr=1e-2, fp16=True)
    tr128.render_kwargs.update(OPT)
    with pytest.raises(ValueError, match="64 rays per pose.*num_rays = 128"):
        tr128.train_step_random(ds)
    assert float(tr128.s_ro.abs().sum()) == 0.0 and ds._ctl.tolist() == [1, 0], "a refused step draws nothing"
    # two poses a step fill a trainer of 2 x 64 rays
    assert np.isfinite(float(tr128.train_step_random(ds, index=(0, 1)))) and tr128.s_poses.shape == (2, 4, 4)
    assert torch.equal(tr128.s_ro[64:], tr128.s_poses[1, :3, 3].expand(64, 3)) and not torch.equal(tr128.s_poses[0], tr128.s_poses[1])
