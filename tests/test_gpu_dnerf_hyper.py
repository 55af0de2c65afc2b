"""D-NeRF hyper backbone on the GPU: the two kernels of csrc/dnerf_hyper.hip against the contract of include/seal3d_hip.h (bit for
bit against s3d_grid_encode_forward with D = 4 where it says so, within a bound derived from the documented order of additions for
grad_ambient), that D = 4 call itself against the CPU oracle, the fused route of the model against its own torch routes under both
interpolations, the renderer's slot selection with this model, a budgeted step, a training smoke and the armed fused Adam update
of the 4-D table."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import dnerf_hyper_witness as hw

pytestmark = pytest.mark.gpu

# the bits of grad_ambient recorded before the sum moved into csrc/ordered_sum.hpp (whose order tests/ordered_sum_witness.py pins
# through the kernels whose terms numpy can restate)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordered_sum_bits.json")) as _f:
    RECORDED = json.load(_f)["hyper_grad_ambient"]

SENT = 1024.0  # sentinel the output buffers are pre-filled with (exact in fp16)
BOUND = 1.0
# one row (a lone lane), nine chunks of 256 + 1 (several workgroups, a ragged last one), 512 x 256 + 257 (a second row per lane of
# the backward's sum; the size at which a one-rounding fp16 conversion showed in csrc/dnerf.hip)
SIZES = [1, 2305, 131329]
AMBIENTS = [-1.0, 0.3, 1.0, 1.5]  # -bound, inside, +bound, outside: all-zero rows


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _nv(n_valid):
    return None if n_valid is None else torch.tensor([n_valid, 0], dtype=torch.int32, device="cuda")


def _live(B, n_valid):
    return B if n_valid is None else min(B, (max(n_valid, 0) + 127) // 128 * 128)


_ENC = {}


def _encoder(L, gridtype, align, interp, dtype):
    """input_dim 4, base resolution 2, 2^10 rows, desired resolution 256: with 16 levels it holds all four level classes.  The
    table is seeded in [-1, 1] (fp32) / [-0.5, 0.5] (fp16) once per geometry and shared."""
    from gridencoder import GridEncoder
    key = (L, gridtype, align, interp, dtype)
    if key not in _ENC:
        enc = GridEncoder(input_dim=4, num_levels=L, level_dim=2, base_resolution=2, log2_hashmap_size=10, desired_resolution=256,
                          gridtype=gridtype, align_corners=align, interpolation=interp)
        r = 1.0 if dtype == torch.float32 else 0.5
        table = _seeded(tuple(enc.embeddings.shape), 11, -r, r).to(dtype).cuda()
        _ENC[key] = (enc, table, enc.offsets.cuda(), float(np.log2(enc.per_level_scale)))
    return _ENC[key]


def _level_classes(enc):
    """per level, how the index treats the four coordinates (gridencoder.cu:66-84: a coordinate enters while stride <= size)"""
    off = enc.offsets.numpy()
    out = []
    for level in range(enc.num_levels):
        size = int(off[level + 1] - off[level])
        scale = np.float32(np.exp2(np.float32(level * np.log2(enc.per_level_scale))) * enc.base_resolution - 1)
        res = int(np.ceil(scale)) + 1
        stride, entered = 1, 0
        for _ in range(4):
            if stride <= size:
                entered += 1
                stride *= res if enc.align_corners else res + 1
        out.append("dense" if stride <= size else {4: "wrap", 3: "no ambient", 2: "no z", 1: "no y"}[entered])
    return out


_PTS = {}


def _points(B):
    """[B, 3] in [-bound, bound] with rows on exact +-bound and a few outside (shared, never written)"""
    if B not in _PTS:
        x = _seeded((B, 3), 70 + B, -BOUND, BOUND)
        if B >= 64:
            x[0], x[1], x[2] = -BOUND, BOUND, 0.0
            x[3, 0], x[4, 1], x[5, 2] = BOUND, -BOUND, BOUND
            x[6, 0], x[7, 2], x[8, 1] = -1.01 * BOUND, 1.001 * BOUND, 3.0 * BOUND  # outside: zero rows
        _PTS[B] = x.cuda().contiguous()
    return _PTS[B]


def _reference(hip, enc, table, offsets, S, x4, want_jac=True, **kw):
    """s3d_grid_encode_forward with D = 4 on the concatenated input -> (feat [B, 2 L] in the table's dtype, dy_dx [B, L, 4, 2]).
    That call produces the Jacobian for pre-normalised inputs only: x01 as it forms it itself — one add, one multiplication by the
    exact reciprocal of a power of two"""
    B, L = x4.shape[0], enc.num_levels
    x01 = ((x4 + BOUND) * (1.0 / (2.0 * BOUND))).contiguous()
    out = torch.empty(L, B, 2, dtype=table.dtype, device="cuda")
    jac = torch.empty(B, L * 8, dtype=table.dtype, device="cuda") if want_jac else None
    hip.GridBackend.grid_encode_forward(x01, table, offsets, out, B, 4, 2, L, S, enc.base_resolution, jac, enc.gridtype_id,
                                        enc.align_corners, enc.interp_id, **kw)
    return out.permute(1, 0, 2).reshape(B, 2 * L), (jac.view(B, L, 4, 2) if want_jac else None)


def _forward(hip, enc, table, offsets, S, x, ambient, n_valid=None, want_x4=True, want_jac=True):
    B, L = x.shape[0], enc.num_levels
    feat = torch.full((B, 2 * L), SENT, dtype=torch.float16, device="cuda")
    x4 = torch.full((B, 4), SENT, device="cuda") if want_x4 else None
    dy_da = torch.full((B, L, 2), SENT, dtype=table.dtype, device="cuda") if want_jac else None
    hip.DnerfHyperBackend.grid_forward(x, ambient, table, offsets, S, enc.base_resolution, enc.gridtype_id, enc.align_corners,
                                       enc.interp_id, BOUND, feat, x4, dy_da, _nv(n_valid))
    return feat, x4, dy_da


# ---- forward --------------------------------------------------------------------------------------------------------------------
def test_the_small_encoder_holds_all_four_level_classes():
    enc = _encoder(16, "tiled", False, "linear", torch.float32)[0]
    classes = _level_classes(enc)
    assert {"dense", "wrap", "no ambient", "no z"} <= set(classes), classes
    assert classes == ["dense"] * 3 + ["wrap"] * 2 + ["no ambient"] * 4 + ["no z"] * 7, classes


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("interp", ["linear", "smoothstep"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("gridtype", ["tiled", "hash"])
@pytest.mark.parametrize("L", [16, 6])
def test_grid_forward_equals_the_4d_grid_call_bit_for_bit(hip, L, gridtype, dtype, interp, align):
    """feat, dy_da and x4 against s3d_grid_encode_forward (D = 4, with dy_dx) on the torch-built [x | ambient] in the same process"""
    enc, table, offsets, S = _encoder(L, gridtype, align, interp, dtype)
    classes = _level_classes(enc)
    for B in SIZES:
        x = _points(B)
        for a in AMBIENTS:
            ambient = torch.tensor([a * BOUND], device="cuda")
            x4_ref = torch.cat([x, ambient.reshape(1, 1).repeat(B, 1)], dim=1).contiguous()
            ref, jac = _reference(hip, enc, table, offsets, S, x4_ref)
            feat, x4, dy_da = _forward(hip, enc, table, offsets, S, x, ambient)
            tag = f"B {B} ambient {a}"
            assert torch.equal(_bits(x4), _bits(x4_ref)), tag
            assert torch.equal(_bits(feat), _bits(ref.to(torch.float16))), tag  # (an fp32 sum: one rounding to binary16)
            assert torch.equal(_bits(dy_da), _bits(jac[:, :, 3, :])), tag
            if a > 1.0:
                assert not feat.any() and not dy_da.any(), tag
                continue
            if B >= 64:
                assert not feat[6:9].any() and not dy_da[6:9].any() and bool(feat[:6].abs().sum() > 0), tag
                assert bool((feat.float().abs().sum(1) > 0).sum() >= B - 3), tag
            if interp == "linear":
                assert not dy_da.any(), tag  # (`pos_deriv[D] = {1.0f}`: the reference's quirk, kept)
            elif B >= 64:
                live = [l for l, c in enumerate(classes) if c in ("dense", "wrap") or gridtype == "hash"]
                shared = [l for l, c in enumerate(classes) if c in ("no ambient", "no z") and gridtype == "tiled"]
                # (at +-bound the smoothstep slope 6 p (1 - p) can vanish: p = 0 with align_corners)
                assert a != 0.3 or (all(bool(dy_da[:, l].abs().sum() > 0) for l in live) and live), tag
                assert not dy_da[:, shared].any(), tag  # (both ambient corners are the same row: a zero difference)
            # the optional outputs change nothing
            only, none_x4, none_j = _forward(hip, enc, table, offsets, S, x, ambient, want_x4=False, want_jac=False)
            assert torch.equal(_bits(only), _bits(feat)) and none_x4 is None and none_j is None


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("n_valid", [0, 100, 300, 2304, 5000])
def test_grid_forward_leaves_rows_behind_the_count_untouched(hip, dtype, n_valid):
    B = 2305
    enc, table, offsets, S = _encoder(16, "tiled", False, "smoothstep", dtype)
    x, ambient = _points(B), torch.tensor([0.3], device="cuda")
    full = _forward(hip, enc, table, offsets, S, x, ambient)
    part = _forward(hip, enc, table, offsets, S, x, ambient, n_valid=n_valid)
    live = _live(B, n_valid)
    for got, want in zip(part, full):
        assert torch.equal(_bits(got[:live]), _bits(want[:live]))
        assert bool((got[live:] == SENT).all())
    assert live in (0, 128, 384, 2304, 2305)


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("gridtype", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_the_4d_grid_call_itself_follows_the_oracle(oracle, hip, dtype, gridtype, interp):
    """s3d_grid_encode_forward with D = 4 at B = 2,305 held to what tests/test_gpu_gridencoder.py holds the D = 3 call to: every
    corner row and every output bit for bit, the fp32 Jacobian at rtol 1e-6 / atol 1e-7 (that file compares no fp16 Jacobian)"""
    B = 2305
    enc, table, offsets, S = _encoder(16, "tiled" if gridtype else "hash", False, "smoothstep" if interp else "linear", dtype)
    L, H = 16, enc.base_resolution
    x01 = ((torch.cat([_points(B), torch.full((B, 1), 0.3, device="cuda")], dim=1) + BOUND) * (1.0 / (2.0 * BOUND))).contiguous()
    xc, ec, oc = x01.cpu(), table.cpu(), enc.offsets
    want_jac = dtype == torch.float32
    out_c = torch.empty(L, B, 2, dtype=dtype)
    jac_c = torch.empty(B, L * 8, dtype=dtype) if want_jac else None
    cidx_c = torch.empty(B, L, 16, dtype=torch.int32)
    oracle.GridBackend.grid_encode_forward(xc, ec, oc, out_c, B, 4, 2, L, S, H, jac_c, gridtype, False, interp, corner_idx=cidx_c)
    out_g = torch.empty(L, B, 2, dtype=dtype, device="cuda")
    jac_g = torch.empty(B, L * 8, dtype=dtype, device="cuda") if want_jac else None
    hip.GridBackend.grid_encode_forward(x01, table, offsets, out_g, B, 4, 2, L, S, H, jac_g, gridtype, False, interp)
    cidx_g = torch.empty(B, L, 16, dtype=torch.int32, device="cuda")
    hip.GridBackend.grid_corner_indices(x01, offsets, cidx_g, B, 4, 2, L, S, H, gridtype, False)
    assert torch.equal(cidx_c, cidx_g.cpu()), "hash / dense indexing differs"
    assert torch.equal(_bits(out_c), _bits(out_g.cpu())), float((out_c.float() - out_g.cpu().float()).abs().max())
    assert not out_c[:, 6:9].any() and bool(out_c.float().abs().sum() > 0)
    if want_jac:
        torch.testing.assert_close(jac_g.cpu(), jac_c, rtol=1e-6, atol=1e-7)
        assert bool(jac_c.view(B, L, 4, 2)[:, :, 3].abs().sum() > 0) == bool(interp)


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _backward(hip, g, j, scale, dtype, n_valid=None, want_sum=True):
    B, L = g.shape[0], g.shape[1] // 2
    levels = torch.full((L, B, 2), SENT, dtype=dtype, device="cuda")
    g_amb = torch.full((1,), SENT, device="cuda") if want_sum else None
    hip.DnerfHyperBackend.grid_backward(g, j, scale, levels, g_amb, _nv(n_valid))
    return levels, g_amb


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("L", [16, 6])
@pytest.mark.parametrize("B,n_valid", [(B, None) for B in SIZES] + [(2305, 0), (2305, 100), (2305, 2200), (2305, 5000)])
def test_grid_backward(hip, B, n_valid, L, dtype):
    g = _seeded((B, 2 * L), B + L, -1, 1).half().cuda()
    j = _seeded((B, L, 2), B + L + 1, -1, 1).to(dtype).cuda()
    live = _live(B, n_valid)
    scale = 1.0 / (2.0 * BOUND)
    levels, g_amb = _backward(hip, g, j, scale, dtype, n_valid)
    again = _backward(hip, g, j, scale, dtype, n_valid)
    want, exact, abs_sum = hw.grid_backward(g.cpu().numpy(), j.cpu().numpy(), scale, rows=live)
    # the transposition: exact (fp16 -> fp32 is exact), rows behind the count untouched
    assert np.array_equal(levels[:, :live].double().cpu().numpy(), want[:, :live])
    assert bool((levels[:, live:] == SENT).all())
    # grad_ambient: any fp32 evaluation of n chained additions of these terms stays within n 2^-24 sum |term| of the exact sum
    n = hw.longest_chain(B, L)
    bound = n * 2.0 ** -24 * abs_sum
    err = abs(float(g_amb.double()) - exact)
    print(f"[hyper grid backward] B {B} n_valid {n_valid} L {L} {dtype}: |err| {err:.3e} bound {bound:.3e} (n {n}, exact {exact:.6e})")
    assert err <= bound
    assert live == 0 or float(g_amb.abs()) > 0
    assert live != 0 or float(g_amb) == 0.0
    assert torch.equal(_bits(g_amb), _bits(again[1])) and torch.equal(_bits(levels), _bits(again[0]))  # the same bits in two runs
    assert int(_bits(g_amb)) == RECORDED[f"B{B}-nv{n_valid}-L{L}-{'f16' if dtype == torch.float16 else 'f32'}"]
    # without dy_da or without the output word: the transposition alone, nothing else written
    only, word = _backward(hip, g, None, scale, dtype, n_valid)
    assert torch.equal(_bits(only), _bits(levels)) and float(word) == SENT
    only, _ = _backward(hip, g, j, scale, dtype, n_valid, want_sum=False)
    assert torch.equal(_bits(only), _bits(levels))
    # grad_scale 1 (a lookup that did not normalise): twice the value, exactly
    assert float(_backward(hip, g, j, 1.0, dtype, n_valid)[1]) == 2.0 * float(g_amb)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("gridtype", ["tiled", "hash"])
def test_table_gradients_through_x4_equal_those_of_the_torch_built_input(hip, gridtype, dtype):
    """the same call on the same bits: s3d_grid_encode_backward (binned: deterministic) with the kernel's x4 and its transposed
    gradient against the torch-built [x | ambient] and the permuted gradient"""
    B, L = 2305, 16
    enc, table, offsets, S = _encoder(L, gridtype, False, "smoothstep", dtype)
    x, ambient = _points(B), torch.tensor([0.3], device="cuda")
    _, x4, _ = _forward(hip, enc, table, offsets, S, x, ambient)
    g = (_seeded((B, 2 * L), 5, -1, 1) * 1e-2).half().cuda()
    levels = _backward(hip, g, None, 0.5, dtype, want_sum=False)[0]
    x4_ref = torch.cat([x, ambient.reshape(1, 1).repeat(B, 1)], dim=1).contiguous()
    levels_ref = g.view(B, L, 2).permute(1, 0, 2).contiguous().to(dtype)
    out = []
    try:
        hip.GridBackend.set_backward_path(2)
        for inp, grad in ((x4, levels), (x4_ref, levels_ref)):
            ge = torch.zeros_like(table)
            hip.GridBackend.grid_encode_backward(grad, inp, table, offsets, ge, B, 4, 2, L, S, enc.base_resolution, None, None,
                                                 enc.gridtype_id, False, enc.interp_id, bound=BOUND)
            out.append(ge)
    finally:
        hip.GridBackend.set_backward_path(0)
    assert torch.equal(_bits(out[0]), _bits(out[1])) and bool(out[0].float().abs().sum() > 0)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(seed_range=0.25, time_size=2, interpolation="linear", **kw):
    from dnerf.network_hyper import NeRFNetwork
    from gridencoder import GridEncoder
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, time_size=time_size,
                      interpolation=interpolation, **kw)
    if net.ambient_dim == 1:
        net.encoder = GridEncoder(input_dim=4, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=14,
                                  desired_resolution=256, gridtype="tiled", interpolation=interpolation)
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -seed_range, seed_range))
    return net.cuda()


def _marched_points(net, M):
    import raymarching
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=128, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    nears, fars = raymarching.near_far_from_aabb(ro, rd, net.aabb_train, net.min_near)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, _, _ = raymarching.march_rays_train(ro, rd, 1, torch.from_numpy(bits).cuda(), 1, 128, nears, fars, counter, 0, False, 128,
                                                    True, 0, 1024)
    assert xyzs.shape[0] >= M
    return xyzs[:M].contiguous(), dirs[:M].contiguous()


def _route(net, x, d, t, mode):
    """(outputs, parameter gradients) of one route: 'fp32' (torch ops, no autocast), 'autocast' (torch ops), 'fused'"""
    net.zero_grad()
    net.fused_mlp = mode == "fused"
    net.train()
    calls = []
    mid = net._color_fused
    net._color_fused = lambda *a: (calls.append(1), mid(*a))[1]
    try:
        with torch.autocast("cuda", dtype=torch.float16, enabled=mode != "fp32"):
            sigma, rgbs, deform = net(x, d, t)
            loss = (sigma.float() * 0.01).sum() + rgbs.float().sum() * 0.1
        loss.backward()
    finally:
        del net._color_fused
    assert deform is None and bool(calls) == (mode == "fused")
    out = dict(sigma=sigma.detach().float(), rgbs=rgbs.detach().float())
    for k, p in net.named_parameters():
        out["grad " + k] = p.grad.detach().float().clone()
    return out


@pytest.mark.parametrize("interpolation", ["linear", "smoothstep"])
def test_fused_route_against_the_models_own_torch_routes(hip, capsys, interpolation):
    """the three-route criterion of tests/test_gpu_dnerf_basis.py: for every output and parameter gradient the fused route's maximum
    error against the fp32 torch route is at most twice the autocast torch route's own, plus 2e-3 max|ref|.  1,500 marched points
    (no multiple of 128: padding rows), t = 0.37.  Under linear interpolation every route hands ambient_net an exactly zero
    gradient; under smoothstep every route a non-zero one.  Figures: profiles/dnerf_hyper.md."""
    net = _model(interpolation=interpolation)
    assert net._glue_ok()
    x, d = _marched_points(net, 1500)
    t = torch.tensor([[0.37]], device="cuda")
    ref = _route(net, x, d, t, "fp32")
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert 1e-3 < float(ref["sigma"].median()) < 1e3 and float(ref["sigma"].std()) > 1e-3  # (seeding: a live sigma)
    auto = _route(net, x, d, t, "autocast")
    fused = _route(net, x, d, t, "fused")
    for k, v in ref.items():
        if k.startswith("grad ambient_net") and interpolation == "linear":
            assert not v.any() and not auto[k].any() and not fused[k].any(), k
        else:
            assert float(v.abs().max()) > 0 and float(fused[k].abs().max()) > 0, k
    lines, bad = [], []
    for k, r in ref.items():
        scale = float(r.abs().max())
        ea, ef = float((auto[k] - r).abs().max()), float((fused[k] - r).abs().max())
        lines.append(f"{k:28s} max|ref| {scale:.3e}  autocast err {ea:.3e}  fused err {ef:.3e}")
        if not ef <= 2 * ea + 2e-3 * scale:
            bad.append(lines[-1])
    with capsys.disabled():
        print(f"\n[dnerf hyper routes, {interpolation}] " + f"\n[dnerf hyper routes, {interpolation}] ".join(lines))
    assert not bad, "\n".join(bad)


def test_a_two_dimensional_ambient_stays_on_the_torch_route(hip):
    net = _model(ambient_dim=2).eval()
    x, d = _marched_points(net, 300)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert not net._can_fuse(x)
        sigma, rgbs, deform = net(x, d, torch.tensor([[0.37]], device="cuda"))
    assert deform is None and sigma.shape == (300,) and rgbs.shape == (300, 3) and torch.isfinite(sigma).all()


def test_density_on_the_fused_route(hip):
    net = _model(interpolation="smoothstep").eval()
    x, _ = _marched_points(net, 300)
    t = torch.tensor([[0.37]], device="cuda")
    with torch.no_grad():
        ref = net.density(x, t)
        with torch.autocast("cuda", dtype=torch.float16):
            assert net._can_fuse(x)
            got = net.density(x, t)
    assert got["sigma"].shape == (300,) and got["geo_feat"].shape == (300, 32) and got["sigma"].dtype == torch.float32
    torch.testing.assert_close(got["sigma"], ref["sigma"], rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(got["geo_feat"].float(), ref["geo_feat"], rtol=2e-2, atol=2e-3)


# ---- renderer, trainer ------------------------------------------------------------------------------------------------------------
def _box_bits(lo, hi):
    import raymarching
    H = 128
    c = torch.arange(H, device="cuda")
    xx, yy, zz = torch.meshgrid(c, c, c, indexing="ij")
    coords = torch.stack([xx, yy, zz], -1).reshape(-1, 3).int()
    w = 2 * coords.float() / (H - 1) - 1
    inside = ((w >= torch.tensor(lo, device="cuda")) & (w <= torch.tensor(hi, device="cuda"))).all(-1)
    grid = torch.zeros(1, H ** 3, device="cuda")
    grid[0, raymarching.morton3D(coords).long()] = inside.float()
    return raymarching.packbits(grid, 0.5)


@pytest.mark.parametrize("train", [True, False])
def test_run_cuda_marches_the_slot_of_its_time(hip, train):
    """two slots holding two different boxes: a rendering at t = 0.2 / 0.8 equals, bit for bit, the rendering of a one-slot model with
    the same parameters whose only slot holds that time's box"""
    from nerf import synthetic as syn
    model = _model(time_size=2)
    boxes = (_box_bits([-0.6, -0.6, -0.6], [-0.1, 0.6, 0.6]), _box_bits([0.1, -0.6, -0.6], [0.6, 0.6, 0.6]))
    model.density_bitfield[0].copy_(boxes[0])
    model.density_bitfield[1].copy_(boxes[1])
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=512, generator=torch.Generator().manual_seed(3))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    images = []
    for time, slot in ((0.2, 0), (0.8, 1)):
        base = _model(time_size=1)
        base.density_bitfield[0].copy_(boxes[slot])
        model.train(train)
        base.train(train)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            got = model.run_cuda(ro, rd, time, bg_color=1, perturb=False, max_steps=256)
            want = base.run_cuda(ro, rd, time, bg_color=1, perturb=False, max_steps=256)
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["depth"], want["depth"])
        assert ("deform" in got) == train and got.get("deform") is None
        assert model.density_bitfield.shape == (2, 128 ** 3 // 8)
        images.append(got["image"])
    assert not torch.equal(images[0], images[1]) and float((images[0] - 1).abs().max()) > 0.05


def test_a_budgeted_step_equals_the_trimmed_one(hip):
    """mean_count > 0: the marcher hands back zero-padded buffers, forward reads the count back once and runs on the live rows — the
    rows the marcher keeps when it trims (mean_count 0): the same samples through the same kernels."""
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    gt = _seeded((256, 3), 82).cuda()
    runs = {}
    for budget in (0, 32768):
        net = _model(interpolation="smoothstep")
        net.density_bitfield[0].copy_(torch.from_numpy(bits))
        net.mean_count = budget
        tr = Trainer(net, fp16=True, native_optim=False, update_extra_interval=10 ** 9)
        tr.global_step = 1
        seen, shapes, ran = {}, [], []
        tr._reduce_and_step = lambda seen=seen, net=net: seen.update({k: p.grad.clone() for k, p in net.named_parameters()})
        fwd, dens_of = net.forward, net._density_fused
        net.forward = lambda x, d, t=None, fwd=fwd, shapes=shapes: (shapes.append(x.shape[0]), fwd(x, d, t))[1]
        net._density_fused = lambda x, t, dens_of=dens_of, ran=ran: (ran.append(x.shape[0]), dens_of(x, t))[1]
        torch.manual_seed(5)  # (the marcher's per-ray jitter: the same samples in both steps)
        loss = tr.train_step(ro, rd, gt, 0.2)
        runs[budget] = (loss.float(), seen, shapes[0], ran[0], int(net.step_counter[0, 0]))
    count = runs[0][4]
    live = (count + 127) // 128 * 128
    assert runs[32768][4] == count and 0 < live < 32768
    assert runs[0][2] == live and runs[32768][2] == 32768 + 128 - 32768 % 128  # (what the marcher handed over)
    assert runs[0][3] == runs[32768][3] == live  # (what the networks ran on)
    torch.testing.assert_close(runs[32768][0], runs[0][0], rtol=1e-6, atol=0)
    for k, g in runs[0][1].items():
        other = runs[32768][1][k]
        assert torch.isfinite(other).all() and bool(other.abs().sum() > 0), k
        if k == "encoder.embeddings":
            # (the fp16 table gradient of a batch this small is summed by atomics: tests/test_gpu_dnerf.py, the same step)
            assert torch.equal((other != 0).any(1).view(-1)[:4096], (g != 0).any(1).view(-1)[:4096])
            continue
        # the same rows through the same kernels; the Linear layers' GEMMs may add in another order from run to run, which moves an
        # fp16 result by an ulp of its size: 2^-10 of the largest entry
        torch.testing.assert_close(other, g, rtol=0, atol=2.0 ** -10 * float(g.abs().max()), msg=k)


def test_training_smoke_on_two_flat_colours(hip):
    """64 x 64 frames at eight times, one flat colour before t = 0.5 and another from there on: 30 eager steps of 1,024 rays; the loss
    stays finite and the mean of the last 8 steps (every frame once) lies below the mean of the first 8 (a direction, not a magnitude)"""
    from dnerf.network_hyper import NeRFNetwork
    from dnerf.provider import DNeRFDataset
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    torch.manual_seed(0)
    times = (torch.arange(8, dtype=torch.float32) + 0.5) / 8
    colours = torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.3, 0.9]])
    images = colours[(times >= 0.5).long()].view(8, 1, 1, 3).expand(8, 64, 64, 3).contiguous()
    poses = syn.orbit_poses(8, seed=0)
    f = 64 / 800
    fx, fy, cx, cy = syn.lego_intrinsics()
    ds = DNeRFDataset(images, poses, (fx * f, fy * f, cx * f, cy * f), times, num_rays=1024, device="cuda")
    net = NeRFNetwork(bound=1, cuda_ray=True, time_size=2, density_thresh=0.01, interpolation="smoothstep").cuda()
    tr = Trainer(net, fp16=True, update_extra_interval=16)
    fused = []
    mid = net._color_fused
    net._color_fused = lambda *a: (fused.append(1), mid(*a))[1]
    losses = []
    for step in range(30):
        batch = ds.collate([step % 8])
        losses.append(tr.train_step(batch["rays_o"][0], batch["rays_d"][0], batch["images"][0], batch["time"]))
    losses = torch.stack(losses).float().cpu()
    assert torch.isfinite(losses).all() and fused
    first, last = float(losses[:8].mean()), float(losses[-8:].mean())
    print(f"[dnerf hyper smoke] first 8: {first:.5f}  last 8: {last:.5f}")
    assert last < first


def test_an_armed_fused_adam_update_runs_inside_the_4d_tables_backward(hip):
    """the fused route's table backward carries no dy_dx, so an update the native optimizer armed for the 4-D table is applied by
    the accumulate kernel (gridencoder.grid._table_backward: `fused_done`), under smoothstep as well, where the torch route's
    backward — with dy_dx — cannot.  32,768 points (a size the binned backward takes); the table is armed by hand, as a trainer
    whose every other gradient is checked where it is produced would arm it."""
    from dnerf.utils import Trainer
    for fused_route in (True, False):
        net = _model(interpolation="smoothstep")
        net.fused_mlp = fused_route
        tr = Trainer(net, fp16=True, update_extra_interval=10 ** 9)
        assert tr.native_optim
        net.train()
        table = net.encoder.embeddings
        before = table.detach().clone()
        x = _seeded((32768, 3), 7, -1, 1).cuda()
        d = torch.nn.functional.normalize(_seeded((32768, 3), 8, -1, 1), dim=-1).cuda()
        tr.optimizer.zero_grad()
        assert tr.optimizer.arm_fused_tables(grad_scale=tr.scaler._scale) == 1
        with torch.autocast("cuda", dtype=torch.float16):
            sigma, rgbs, _ = net(x, d, torch.tensor([[0.37]], device="cuda"))
            loss = (sigma.float() * 0.01).mean() + rgbs.float().mean()
        tr.scaler.backward(loss)
        h = table._s3d
        assert h.arm is None and bool(h.fused_done) == fused_route
        assert torch.equal(before, table.detach()) != fused_route  # (updated in its backward, or not yet)
        assert torch.isfinite(table).all() and float(net.ambient_net[0].weight.grad.abs().max()) > 0
        tr.optimizer.disarm_fused_tables()
