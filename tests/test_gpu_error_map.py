"""Error-map importance sampling on the GPU: s3d_sample_train_rays (explicit uniforms against torch, the device RNG against
torch.multinomial), s3d_error_map_update against the torch restatement, the trainers' routes, graph replay, Seal and TensoRF
steps with the map, and learning: the sampler concentrates on what the model has not learnt."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from test_seal_tools import S, config  # noqa: F401

pytestmark = pytest.mark.gpu


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _peaked_map(B, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(128.0), torch.arange(128.0), indexing="ij")
    m = torch.rand(B, 128, 128, generator=g) * 0.05
    for b in range(B):
        cx, cy = torch.rand(2, generator=g) * 128
        m[b] += 4 * torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 200.0)
    return m.reshape(B, -1).contiguous()


def _explicit(hip, emap, B, H, W, N, img_dtype=torch.float32, seed=0):
    """one explicit-uniform sampler launch and the torch expectation of every output"""
    from nerf import synthetic as syn
    poses = syn.orbit_poses(B, seed=seed).cuda()
    intr = syn.lego_intrinsics(H, W)
    images = _seeded((B, H, W, 3), seed + 1).to(img_dtype).cuda()
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    u_keys = (1.0 - _seeded((B, 128 * 128), seed + 2)).cuda()  # (0, 1]
    u_fine = _seeded((B, N, 2), seed + 3).cuda()
    emap = emap.cuda()
    o = {k: torch.full((B, N, 3), -7.0, device="cuda") for k in ("rays_o", "rays_d", "gt")}
    inds, coarse = (torch.full((B, N), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    hip.RaySampleBackend.sample_train_rays(emap, idx, N, H, W, poses, intr, o["rays_o"], o["rays_d"], inds, coarse, images=images,
                                           gt=o["gt"], u_keys=u_keys, u_fine=u_fine)
    torch.cuda.synchronize()
    # expectation: keys w / -log(u) (0 where w <= 0), the N largest, at equal keys the lower cell (stable sort), ascending order
    keys = torch.where(emap > 0, emap / (0.0 - torch.log(u_keys)), torch.zeros_like(emap))
    order = torch.sort(keys, dim=1, descending=True, stable=True).indices[:, :N]
    exp_coarse = torch.sort(order, dim=1).values
    sx, sy = H / 128, W / 128
    ix = ((exp_coarse // 128) * sx + u_fine[..., 0] * sx).long().clamp(max=H - 1)
    iy = ((exp_coarse % 128) * sy + u_fine[..., 1] * sy).long().clamp(max=W - 1)
    exp_inds = ix * W + iy
    i = (exp_inds % W).float() + 0.5
    j = (exp_inds // W).float() + 0.5
    fx, fy, cx, cy = [float(v) for v in intr]
    dirs = torch.stack(((i - cx) / fx, (j - cy) / fy, torch.ones_like(i)), dim=-1)
    dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
    exp_rd = dirs @ poses[:, :3, :3].transpose(-1, -2)
    exp_gt = torch.gather(images.view(B, -1, 3), 1, torch.stack(3 * [exp_inds], -1)).float()
    return dict(coarse=coarse, inds=inds, o=o, exp_coarse=exp_coarse, exp_inds=exp_inds, exp_rd=exp_rd, exp_gt=exp_gt,
                exp_ro=poses[:, None, :3, 3].expand(B, N, 3))


CASES = {
    "800x800": (1, 800, 800, 4096, lambda: _peaked_map(1, 1)),
    "600x800_B2": (2, 600, 800, 4096, lambda: _peaked_map(2, 2)),
    "N16384": (1, 800, 800, 16384, lambda: _peaked_map(1, 3)),
    "few_positive": (1, 800, 800, 4096, lambda: torch.zeros(1, 16384).index_fill_(1, torch.arange(0, 16384, 173), 0.5)),
    "single_hot": (1, 800, 800, 256, lambda: torch.zeros(1, 16384).index_fill_(1, torch.tensor([5000]), 1.0)),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("img_dtype", [torch.float32, torch.float16])
def test_sampler_with_explicit_uniforms_matches_torch(hip, case, img_dtype):
    B, H, W, N, mk = CASES[case]
    r = _explicit(hip, mk(), B, H, W, N, img_dtype)
    assert torch.equal(r["coarse"], r["exp_coarse"])  # the set of torch's top N keys, ascending (zero-weight fill: by index)
    assert torch.equal(r["inds"], r["exp_inds"])
    assert torch.equal(r["o"]["rays_o"], r["exp_ro"])
    assert torch.equal(r["o"]["gt"], r["exp_gt"])
    assert (r["o"]["rays_d"] - r["exp_rd"]).abs().max().item() <= 1e-6


def _dataset(error_map=True, n=2, H=800, W=800, N=256, seed=0):
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    imgs = _seeded((n, H, W, 3), 5)
    return NeRFDataset(imgs, syn.orbit_poses(n, seed=0), syn.lego_intrinsics(H, W), num_rays=N, error_map=error_map,
                       device="cuda", seed=seed)


def test_device_rng_draws_like_torch_multinomial(hip):
    """2,000 draws of N = 256 cells from a peaked map: no duplicates in a row, and the inclusion counts per 8 x 8 block of
    cells agree with torch.multinomial(replacement=False) on the GPU within 6 sqrt(a + b) (a, b: the two counts; both are sums
    of independent Bernoulli-like draws, so the difference has a standard deviation below sqrt(a + b))"""
    ds = _dataset(N=256)
    ds.error_map.copy_(_peaked_map(2, 7))
    hits = torch.zeros(16384, device="cuda")
    ref = torch.zeros(16384, device="cuda")
    draws = 2000
    for _ in range(draws):
        b = ds.sample([1])
        c = b["inds_coarse"][0]
        hits.index_add_(0, c, torch.ones(256, device="cuda"))
        ref.index_add_(0, torch.multinomial(ds.error_map[1], 256, replacement=False), torch.ones(256, device="cuda"))
        if _ < 20:
            assert c.unique().numel() == 256 and bool((c[1:] > c[:-1]).all())
    assert float(hits.sum()) == draws * 256
    a = hits.view(16, 8, 16, 8).sum((1, 3))
    r = ref.view(16, 8, 16, 8).sum((1, 3))
    bound = 6 * torch.sqrt(torch.clamp(a + r, min=1))
    assert bool(((a - r).abs() <= bound).all()), float(((a - r).abs() / bound).max())


def test_uniform_mode_in_range_and_fresh_cells_on_graph_replay(hip):
    ds = _dataset(error_map=False, N=4096)
    b = ds.sample([0])
    assert int(b["inds"].min()) >= 0 and int(b["inds"].max()) < 800 * 800
    assert b["inds"].unique().numel() > 4000  # (randint: duplicates possible, rare)
    assert torch.equal(b["images"][0], ds.images[0].view(-1, 3)[b["inds"][0]])
    dm = _dataset(N=1024)
    out = {"rays_o": torch.zeros(1, 1024, 3, device="cuda"), "rays_d": torch.zeros(1, 1024, 3, device="cuda"),
           "images": torch.zeros(1, 1024, 3, device="cuda"), "inds": torch.zeros(1, 1024, dtype=torch.int64, device="cuda"),
           "inds_coarse": torch.zeros(1, 1024, dtype=torch.int64, device="cuda"), "index": torch.zeros(1, dtype=torch.int64, device="cuda")}
    dm.sample([1], out=out)  # warm-up
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            dm.sample([1], out=out)
    torch.cuda.current_stream().wait_stream(s)
    seen = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append(out["inds_coarse"].clone())
        assert int(out["index"][0]) == 1 and out["inds_coarse"][0].unique().numel() == 1024
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def _torch_update(emap, index, inds, image, ws, gt, bg, depth=None, gt_depth=None, dw=1.0):
    """the kernel's float expressions in torch"""
    B, N = inds.shape
    bgt = bg if torch.is_tensor(bg) else torch.tensor(bg, device=image.device).expand(B * N, 3)
    p = image + (1 - ws).unsqueeze(-1) * bgt
    d = p - gt
    sq = d * d
    e = (sq[:, 0] + sq[:, 1] + sq[:, 2]) * (1.0 / 3.0)
    if depth is not None:
        e = e + dw * (torch.nan_to_num(depth, nan=0.0) - gt_depth).abs().double().mean().float()
    e = e.view(B, N)
    out = emap.clone()
    old = out[index[:, None], inds]
    new = 0.1 * old + 0.9 * e
    out[index[:, None], inds] = torch.where(torch.isfinite(e), new, old)
    return out


@pytest.mark.parametrize("kind", ["const", "per_ray", "depth"])
def test_update_kernel_matches_torch_restatement(hip, kind):
    B, N = 2, 2048
    emap = _peaked_map(3, 11).cuda()
    index = torch.tensor([2, 0], dtype=torch.int64, device="cuda")
    inds = torch.stack([torch.randperm(16384, generator=torch.Generator().manual_seed(b))[:N] for b in range(B)]).cuda()
    image, gt = _seeded((B * N, 3), 12).cuda(), _seeded((B * N, 3), 13).cuda()
    ws = _seeded((B * N,), 14).cuda()
    bg = _seeded((B * N, 3), 15).cuda() if kind == "per_ray" else (1.0, 0.5, 0.25)
    depth = gt_depth = None
    if kind == "depth":
        depth, gt_depth = _seeded((B * N,), 16, 0, 4).cuda(), _seeded((B * N,), 17, 0, 4).cuda()
        depth[5] = float("nan")
    image[7, 1] = float("nan")  # a non-finite error keeps the old value
    exp = _torch_update(emap, index, inds, image, ws, gt, bg, depth, gt_depth, 0.5)
    got = emap.clone()
    hip.RaySampleBackend.error_map_update(got, index, inds, image, gt, ws, bg, depth, gt_depth, 0.5)
    torch.cuda.synchronize()
    assert got[index[0], inds[0, 7]] == emap[index[0], inds[0, 7]]
    if kind == "depth":  # (the batch mean of the depth term: reduced in the launch's fixed order)
        torch.testing.assert_close(got, exp, rtol=1e-6, atol=1e-7)
    else:
        assert torch.equal(got, exp)
    untouched = torch.ones_like(emap, dtype=torch.bool)
    untouched[index[:, None], inds] = False
    assert torch.equal(got[untouched], emap[untouched])


def _ngp(seed=0):
    from nerf import synthetic as syn
    from nerf.network import NeRFNetwork
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, log2_hashmap_size=15).cuda()
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens).cuda())
    net.density_bitfield.copy_(torch.from_numpy(bits).cuda())
    net.iter_density = 100
    return net


@pytest.mark.parametrize("route", ["fused", "bgmse", "torch_scaler"])
def test_trainer_routes_update_the_map_like_the_torch_restatement(hip, monkeypatch, route):
    import nerf.trainer as T
    net = _ngp()
    tr = T.Trainer(net, lr=1e-2, fp16=True, update_extra_interval=10 ** 9, native_optim=route != "torch_scaler")
    if route == "bgmse":
        tr.fused_losses = False
    tr.global_step = 1
    net.mean_count = 4096 * 40
    ds = _dataset(N=4096)
    tr.error_map = ds.error_map
    ds.error_map.copy_(_peaked_map(2, 21))
    seen = {}
    orig = T.update_error_map

    def spy(out, gt, em, gt_depth=None, dw=1.0):
        emap, index, inds = em
        o = dict(out)
        if not o.get("premultiplied", False):  # (torch route: image already composited)
            o = dict(o, weights_sum=torch.ones_like(o["weights_sum"]), bg_color=0.0)
        bg = o["bg_color"]
        bg = (float(bg),) * 3 if not torch.is_tensor(bg) else bg.float().reshape(-1, 3)
        seen["exp"] = _torch_update(emap, torch.as_tensor(index, device="cuda").reshape(-1), inds.reshape(1, -1),
                                    o["image"].detach().float().reshape(-1, 3), o["weights_sum"].detach().float().reshape(-1),
                                    gt.float().reshape(-1, 3), bg)
        seen["premultiplied"] = out.get("premultiplied", False)
        return orig(out, gt, em, gt_depth, dw)

    monkeypatch.setattr(T, "update_error_map", spy)
    for _ in range(2):
        b = ds.sample([1])
        tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], index=b["index"], inds_coarse=b["inds_coarse"])
        torch.cuda.synchronize()
        if route == "torch_scaler":
            assert not seen["premultiplied"]
            torch.testing.assert_close(ds.error_map, seen["exp"], rtol=1e-6, atol=1e-7)
        else:
            assert seen["premultiplied"]
            assert torch.equal(ds.error_map, seen["exp"])
    assert not torch.equal(ds.error_map[1], _peaked_map(2, 21)[1].cuda())
    assert torch.equal(ds.error_map[0], _peaked_map(2, 21)[0].cuda())


def _graphed_em_run(recapture, batches, steps=20):
    from nerf.trainer import GraphedTrainer
    net = _ngp()
    tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
    tr.global_step = 1
    net.mean_count = 4096 * 40
    emap = _peaked_map(2, 31).cuda()
    tr.error_map = emap
    for k in range(steps):
        if recapture:
            tr.graph = None
        ro, rd, gt, idx, inds = batches[k]
        tr.train_step(ro, rd, gt, index=idx, inds_coarse=inds)
    torch.cuda.synchronize()
    return tr, emap


def test_graphed_replay_and_eager_twin_end_with_the_same_map(hip):
    ds = _dataset(N=4096)
    batches = []
    for k in range(20):
        b = ds.sample([k % 2])
        batches.append((b["rays_o"][0].clone(), b["rays_d"][0].clone(), b["images"][0].clone(), b["index"].clone(),
                        b["inds_coarse"].clone()))
    tr_r, m_r = _graphed_em_run(False, batches)
    assert tr_r.n_captures == 1
    tr_e, m_e = _graphed_em_run(True, batches)
    assert tr_e.n_captures == 20
    assert torch.isfinite(m_r).all()
    assert not torch.equal(m_r, _peaked_map(2, 31).cuda())
    # (tolerance of test_graphed_replay_equals_the_eager_step_with_background: the renders of the two runs agree to fp16 atomics)
    torch.testing.assert_close(m_r, m_e, rtol=1e-3, atol=1e-3)


def test_graphed_step_reads_the_sampler_s_static_batch(hip, monkeypatch):
    """sample(out=trainer.static_batch()) writes the captured step's inputs: no staging copy, the map still moves"""
    from nerf.trainer import GraphedTrainer
    net = _ngp()
    tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
    tr.global_step = 1
    net.mean_count = 4096 * 40
    ds = _dataset(N=4096)
    tr.error_map = ds.error_map
    calls = []
    orig = torch._foreach_copy_
    monkeypatch.setattr(torch, "_foreach_copy_", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    for k in range(4):
        b = ds.sample([k % 2], out=tr.static_batch())
        tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], index=b["index"], inds_coarse=b["inds_coarse"])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert not calls and tr.n_captures == 1
    assert int(tr.s_index[0]) == 1 and float((ds.error_map != 1).sum()) > 0


def _seal_pair():
    from nerf import network, synthetic as syn
    from sealnerf import get_seal_mapper, make_student, make_teacher
    from test_seal_golden import case_config
    torch.manual_seed(0)
    kw = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, log2_hashmap_size=15)
    teacher = make_teacher(network.NeRFNetwork, **kw).cuda()
    student = make_student(network.NeRFNetwork, **kw).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    for net in (teacher, student):
        net.density_grid.copy_(torch.from_numpy(grid))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.iter_density = 100
    student.load_state_dict(teacher.state_dict())
    m = get_seal_mapper(case_config("both", np.load(os.path.join(REPO, "tests", "golden", "seal_bbox.npz"))))
    teacher.init_mapper(m)
    student.init_mapper(m)
    return teacher, student


@pytest.mark.parametrize("graphed", [False, True])
def test_seal_bbox_finetune_with_the_map(hip, S, graphed):
    from nerf import synthetic as syn
    from sealnerf import GraphedSealTrainer, SealTrainer
    from sealnerf.provider import SealDataset
    teacher, student = _seal_pair()
    tr = GraphedSealTrainer(student, teacher, 1024, lr=1e-2, fp16=True) if graphed else SealTrainer(student, teacher, lr=1e-2, fp16=True)
    ds = SealDataset(syn.orbit_poses(2, seed=0), syn.lego_intrinsics(), 800, 800, num_rays=1024, device="cuda", error_map=True)
    tr.error_map = ds.error_map
    hist = []
    for k in range(20):
        b = ds.sample([k % 2])  # (no frames: the targets are the teacher's proxy renders)
        hist.append(float(tr.train_step(b["rays_o"][0], b["rays_d"][0], index=b["index"], inds_coarse=b["inds_coarse"])))
    torch.cuda.synchronize()
    assert np.isfinite(hist).all() and torch.isfinite(ds.error_map).all()
    assert float((ds.error_map != 1).sum()) > 0 and float((ds.error_map[0] != 1).sum()) <= 10 * 1024
    if graphed:
        assert tr.n_captures >= 1


def test_tensorf_eager_step_with_the_map(hip):
    from nerf import synthetic as syn
    from tensoRF import network as trf
    from tensoRF.utils import Trainer
    torch.manual_seed(0)
    net = trf.NeRFNetwork(resolution=[64] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(grid))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net.iter_density = 100
    tr = Trainer(net, lr0=2e-2, fp16=True, update_extra_interval=10 ** 9)
    tr.global_step = 1
    ds = _dataset(N=4096)
    tr.error_map = ds.error_map
    b = ds.sample([0])
    loss = float(tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], index=b["index"], inds_coarse=b["inds_coarse"]))
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    changed = ds.error_map[0].ne(1)
    assert 0 < int(changed.sum()) <= 4096 and bool(changed[b["inds_coarse"][0]].any())


def test_sampler_learns_to_concentrate_on_the_unlearnt_quadrant(hip):
    """two frames of one pose: the same smooth colour everywhere but in the top-left quadrant, which carries a 1-pixel
    checkerboard, inverted between the frames — high-frequency texture the model cannot reconcile.  After 300 steps with the
    map the share of sampled rays in that quadrant is at least 1.5 x its area share.  (The sample budget covers every ray: a ray
    dropped by the budget renders as background, and the sampler's ascending cell order would make those the last cells.)"""
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    from nerf.trainer import GraphedTrainer
    H = W = 256
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.stack([0.3 + 0.4 * xx / W, 0.5 + 0.3 * yy / H, torch.full_like(xx, 0.4)], -1)
    q = (yy < H // 2) & (xx < W // 2)
    chk = ((yy + xx) % 2).unsqueeze(-1)
    imgs = torch.stack([torch.where(q.unsqueeze(-1), c.expand(H, W, 3), img) for c in (chk, 1 - chk)])
    ds = NeRFDataset(imgs, syn.orbit_poses(1, seed=0).expand(2, 4, 4), syn.lego_intrinsics(H, W), num_rays=4096, error_map=True,
                     device="cuda")
    net = _ngp()
    net.density_grid.fill_(50.0)  # (every ray hits matter: every pixel's colour is learnable)
    net.density_bitfield.fill_(255)
    tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
    tr.global_step = 1
    net.mean_count = 4096 * 512  # (~465 samples per ray through the occupied cube)
    tr.error_map = ds.error_map
    share = []
    for k in range(300):
        b = ds.sample([k % 2], out=tr.static_batch())
        if k >= 250:
            inds = b["inds"][0]
            share.append(float(((inds // W < H // 2) & (inds % W < W // 2)).float().mean()))
        tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], index=b["index"], inds_coarse=b["inds_coarse"])
    torch.cuda.synchronize()
    assert np.mean(share) >= 1.5 * 0.25, np.mean(share)
