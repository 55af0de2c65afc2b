"""GPU parity of the fused MLP kernels (csrc/ffmlp.hip, csrc/ffmlp_generic.hip) and of the stand-alone NGP head kernels
(csrc/ngp_head.hip) against the float64 witness of tests/mlp_witness.py.

(a) exact cases — integer data for which every fp16 rounding and every fp32 sum is exact (tests/test_mlp_witness.py checks the
    conditions on the CPU): outputs, grad_inputs and grad_weights BIT FOR BIT on every path of the dispatch;
(b) rounding and accumulation probes: ties to even at the layer boundaries, fp32 accumulation;
(c) every activation as hidden and as output activation, within bounds the witness computes from one-ulp flips of the stored
    activations (nothing measured on the kernels);
(d) the stand-alone head kernels against their float64 statements.
The `[ffmlp parity]` lines (c) prints are recorded in profiles/ffmlp_parity.md."""
import os

import numpy as np
import pytest
import torch

import mlp_witness as mw

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float16))).cuda()


def bits(a):
    """binary16 bit patterns of a witness array (-0 of a float64 product counts as the +0 a sum starting at +0 gives)"""
    return torch.from_numpy(np.ascontiguousarray((np.asarray(a, np.float64) + 0.0).astype(np.float16))).view(torch.int16)


def same(t, ref):
    return torch.equal(t.detach().cpu().contiguous().view(torch.int16).reshape(-1), bits(ref).reshape(-1))


def level_major(t, B, in_dim):
    return t.view(B, in_dim // 2, 2).permute(1, 0, 2).contiguous()


def row_major(t, B, in_dim):
    return t.permute(1, 0, 2).reshape(B, in_dim).contiguous()


class Net:
    """one witness case on the device"""

    def __init__(self, hip, case, rows=None):
        self.F, self.case = hip.FFMLPBackend, case
        self.in_dim, self.W, self.n, self.act = case["in_dim"], case["W"], case["n"], case["act"]
        self.x, self.grad, self.w = dev16(case["x"][:rows]), dev16(case["grad"][:rows]), dev16(mw.flat(case["mats"]))
        self.B = self.x.shape[0]
        self.shape = (self.in_dim, self.W, self.n)

    def filled(self, *shape):
        return torch.full(shape, SENTINEL, dtype=torch.half, device="cuda")

    def forward(self, train, out_act=6, layout=0, n_valid=None):
        """-> (outputs, forward_buffer or None)"""
        x = level_major(self.x, self.B, self.in_dim) if layout else self.x
        out = self.filled(self.B, 16)
        if train:
            fb = torch.empty(self.n, self.B, self.W, dtype=torch.half, device="cuda")
            self.F.ffmlp_forward(x, self.w, self.B, self.in_dim, 16, self.W, self.n, self.act, out_act, fb, out, input_layout=layout, n_valid=n_valid)
            return out, fb
        scratch = torch.empty(2, self.B, self.W, dtype=torch.half, device="cuda")
        self.F.ffmlp_inference(x, self.w, self.B, self.in_dim, 16, self.W, self.n, self.act, out_act, scratch, out, input_layout=layout, n_valid=n_valid)
        return out, None

    def backward(self, fb, calc=True, layout=0, prefill=None, n_valid=None, **kw):
        """stored (fb given) or fused (fb None) backward -> (grad_inputs row-major or None, grad_weights, found_inf)"""
        x = level_major(self.x, self.B, self.in_dim) if layout else self.x
        bb = torch.zeros(self.n, self.B, self.W, dtype=torch.half, device="cuda") if fb is not None else None
        gi = self.filled(*x.shape) if calc else None
        gw = prefill.clone() if prefill is not None else self.filled(self.w.numel())
        found = torch.zeros(1, device="cuda")
        self.F.ffmlp_backward(self.grad, x, self.w, fb, self.B, self.in_dim, 16, self.W, self.n, self.act, 6, calc, bb, gi, gw,
                              input_layout=layout, accumulate=prefill is not None, n_valid=n_valid, found_inf=found, **kw)
        if calc and layout:
            gi = row_major(gi, self.B, self.in_dim)
        return gi, gw, found


def check_exact(hip, case, rows, with_n_valid):
    """every path the shape has against the witness on the case's first `rows` rows"""
    net = Net(hip, case, rows)
    ref = mw.run_case(case, rows)
    shape, B = net.shape, net.B
    native = shape in mw.NATIVE_SHAPES
    fused = net.F.fused_backward_supported(net.in_dim, 16, net.W, net.n, net.act)
    assert fused == (shape in mw.FUSED_SHAPES)
    gw_ref = mw.h16(ref["gw"])
    rng = np.random.default_rng(rows)
    pre = rng.integers(-3, 4, net.w.numel()).astype(np.float64)
    gw_acc = mw.h16(pre + ref["gw"])  # an accumulating call adds in fp32 and rounds once
    assert np.abs(pre + ref["gw"]).max() <= 65504

    out, fb = net.forward(True)
    assert same(out, ref["outputs"]), "training forward"
    assert same(net.forward(False)[0], ref["outputs"]), "inference forward"
    backs = [("stored", fb)] + ([("fused", None)] if fused else [])
    for name, buf in backs:
        gi, gw, found = net.backward(buf)
        assert same(gi, ref["grad_inputs"]), f"{name} backward: grad_inputs"
        assert same(gw, gw_ref), f"{name} backward: grad_weights"
        gi, gw2, found2 = net.backward(buf, prefill=dev16(pre))
        assert same(gi, ref["grad_inputs"]) and same(gw2, gw_acc), f"{name} backward, accumulate"
        assert float(found) == 0 and float(found2) == 0
    if fused:
        _, gw, _ = net.backward(None, calc=False)
        assert same(gw, gw_ref), "fused backward without grad_inputs"
        gi, gw, _ = net.backward(None, layout=1)
        assert same(gi, ref["grad_inputs"]) and same(gw, gw_ref), "fused backward, level-major inputs"
    if native:
        assert same(net.forward(True, layout=1)[0], ref["outputs"]), "training forward, level-major inputs"
        assert same(net.forward(False, layout=1)[0], ref["outputs"]), "inference forward, level-major inputs"
    if with_n_valid and native:
        for count in (77, B - 300):
            nv = torch.tensor([count], dtype=torch.int32, device="cuda")
            v = min(B, (count + 127) // 128 * 128)
            part = mw.run_case(case, v)
            out_ref = np.concatenate([part["outputs"], np.full((B - v, 16), SENTINEL)])
            gi_ref = np.concatenate([part["grad_inputs"], np.full((B - v, net.in_dim), SENTINEL)])
            assert same(net.forward(True, n_valid=nv)[0], out_ref) and same(net.forward(False, n_valid=nv)[0], out_ref), f"n_valid {count}"
            for name, buf in backs:
                gi, gw, _ = net.backward(buf, n_valid=nv)
                assert same(gi, gi_ref), f"{name} backward, n_valid {count}: grad_inputs"
                assert same(gw, mw.h16(part["gw"])), f"{name} backward, n_valid {count}: grad_weights"


# ------------------------------------------------------------------------------------------------------------ (a) exact parity
def test_fused_backward_accepts_the_expected_shapes(hip):
    F = hip.FFMLPBackend
    for act in (0, 1, 3, 4, 5, 6):
        assert [s for s in mw.NATIVE_SHAPES + mw.GENERIC_SHAPES if F.fused_backward_supported(s[0], 16, s[1], s[2], act)] == mw.FUSED_SHAPES
    assert not any(F.fused_backward_supported(s[0], 16, s[1], s[2], 2) for s in mw.NATIVE_SHAPES + mw.GENERIC_SHAPES)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("act", [0, 6])
@pytest.mark.parametrize("shape", mw.NATIVE_SHAPES + mw.GENERIC_SHAPES, ids=ids)
def test_exact_parity(hip, shape, act, kind):
    case = mw.exact_case(kind, shape, act, mw.BATCHES[-1])
    for rows in mw.BATCHES:
        check_exact(hip, case, rows, with_n_valid=rows == mw.BATCHES[-1])


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("act", [0, 6])
@pytest.mark.parametrize("shape", mw.BIG_SHAPES, ids=ids)
def test_exact_parity_above_every_grid_cap(hip, shape, act, kind):
    """131,200 rows = 4,100 tiles: more than 4 x 768 / 4 x 256 forward, 4 x 1,024 data-gradient and 4 x 256 / 4 x 128 weight-gradient
    tiles per launch — every several-tiles-per-workgroup loop runs and every partial plane is written"""
    check_exact(hip, mw.exact_case(kind, shape, act, mw.BIG_BATCH), None, with_n_valid=False)


@pytest.mark.parametrize("B", [384, mw.BIG_BATCH])
def test_deferred_reduce_of_a_pair_equals_the_two_plain_calls(hip, B):
    F = hip.FFMLPBackend
    # (384: the leading rows of the 4,736-row case, as in test_exact_parity)
    nets = [Net(hip, mw.exact_case("dense", s, 0, max(B, mw.BATCHES[-1])), B) for s in ((32, 64, 2), (32, 64, 3))]
    refs = [mw.run_case(n.case, B) for n in nets]
    jobs, outs = [], []
    for net in nets:
        ws = torch.empty(F.backward_workspace_bytes(net.in_dim, 16, net.W, net.n), dtype=torch.uint8, device="cuda")
        gi, gw, found = net.backward(None, workspace=ws, defer_reduce=True)
        assert same(gw, np.full(net.w.numel(), SENTINEL)), "a deferred call leaves grad_weights alone"
        jobs.append((ws, B, net.in_dim, net.W, net.n, gw, False, found))
        outs.append((gi, gw, found))
    F.wgrad_reduce_pair(*jobs)
    for (gi, gw, found), ref, net in zip(outs, refs, nets):
        plain = net.backward(None)
        assert same(gi, ref["grad_inputs"]) and same(gw, mw.h16(ref["gw"])) and float(found) == 0
        assert torch.equal(gw.view(torch.int16), plain[1].view(torch.int16)) and torch.equal(gi.view(torch.int16), plain[0].view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ (b) probes
@pytest.mark.parametrize("act", [0, 6])
def test_ties_to_even_at_the_layer_boundaries_and_fp32_accumulation(hip, act):
    case, hidden, outs = mw.probe_case(act)
    net = Net(hip, case)
    ref = mw.run_case(case)["outputs"]
    assert list(ref[0, :7]) == list(outs) and list(ref[0, :4]) == list(hidden)  # (+ row: the first layer's probes arrive unchanged)
    for train in (True, False):
        out = net.forward(train)[0]
        assert out[0, :7].tolist() == list(outs), "2,049 / 2,050 / 2,051 -> 2,048 / 2,050 / 2,052; 2,048 + 16 x 1 - 2,048 = 16"
        assert same(out, ref)


# ------------------------------------------------------------------------------------------------------------ (c) activations
CHAIN_SHAPES = [(32, 64), (32, 128), (32, 16)]  # register-resident (stored + fused), W = 128, layer-by-layer


def report(label, got, ref, bound):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    err = np.abs(got - ref)
    print(f"[ffmlp parity] {label}: worst error / bound {float((err / bound).max()):.3f}, {int((err != 0).sum())} of {err.size} elements differ")
    assert np.isfinite(got).all() and (err <= bound).all(), label


@pytest.mark.parametrize("act", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("in_dim,W", CHAIN_SHAPES, ids=ids)
def test_hidden_activation_within_the_witness_bounds(hip, in_dim, W, act):
    case = mw.chain_case(in_dim, W, act)
    ref = mw.chain_bounds(case)
    assert np.isfinite(ref["out"]).all() and float((ref["out"] != 0).mean()) > 0.5
    net = Net(hip, case)
    tag = f"hidden {mw.ACT_NAMES[act]} W {W}"
    out, fb = net.forward(True)
    report(f"{tag} forward", out, ref["out"], ref["out_bound"])
    report(f"{tag} inference", net.forward(False)[0], ref["out"], ref["out_bound"])
    if act == mw.SINE:
        with pytest.raises(RuntimeError, match="sine needs pre-activations"):
            net.backward(fb)
        return
    assert np.abs(ref["gw"]).max() < 65504 and float((ref["grad_inputs"] != 0).mean()) > 0.2
    fused = net.F.fused_backward_supported(in_dim, 16, W, 2, act)
    assert fused == (W == 64)
    for name, buf in [("stored", fb)] + ([("fused", None)] if fused else []):
        gi, gw, found = net.backward(buf)
        report(f"{tag} {name} backward grad_inputs", gi, ref["grad_inputs"], ref["grad_inputs_bound"])
        report(f"{tag} {name} backward grad_weights", gw, ref["gw"], ref["gw_bound"])
        assert float(found) == 0


@pytest.mark.parametrize("out_act", range(7))
@pytest.mark.parametrize("in_dim,W", CHAIN_SHAPES, ids=ids)
def test_output_activation_within_the_witness_bounds(hip, in_dim, W, out_act):
    for act in (mw.SIGMOID, mw.RELU):
        case = mw.chain_case(in_dim, W, act)
        ref = mw.chain_bounds(case, out_act=out_act)
        net = Net(hip, case)
        tag = f"output {mw.ACT_NAMES[out_act]} after {mw.ACT_NAMES[act]} W {W}"
        report(f"{tag} forward", net.forward(True, out_act=out_act)[0], ref["out"], ref["out_bound"])
        report(f"{tag} inference", net.forward(False, out_act=out_act)[0], ref["out"], ref["out_bound"])


# ------------------------------------------------------------------------------------------------------------ (d) head kernels
def within_one_ulp(got, ref):
    """|got - half(ref)| <= one binary16 ulp of ref"""
    got = got.detach().cpu().double().numpy()
    return bool((np.abs(got - mw.h16(ref)) <= mw.ulp16(ref)).all())


def head_inputs(B, seed):
    rng = np.random.default_rng(seed)
    from conftest import GOLDEN
    sh = np.load(os.path.join(GOLDEN, "sh_deg8.npz"))
    reps = -(-B // len(sh["inputs"]))
    dirs = np.tile(sh["inputs"], (reps, 1))[:B].astype(np.float32)
    sh16 = np.tile(sh["outputs"][:, :16], (reps, 1))[:B].astype(np.float64)
    h = rng.integers(-4, 5, (B, 16)).astype(np.float64)
    edges = np.array([15.0, -15.0, 16.0, -16.0, 20.0, -20.0, 14.5, -0.25])
    h[:, 0] = np.where(np.arange(B) % 3 == 0, edges[(np.arange(B) // 3) % len(edges)], h[:, 0] / 2)
    return rng, dirs, sh16, h


def valid_count(B, masked):
    """-> (n_valid tensor or None, rows the kernels touch)"""
    if not masked:
        return None, B
    count = max(B - 300, 77)
    return torch.tensor([count], dtype=torch.int32, device="cuda"), min(B, (count + 127) // 128 * 128)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [1, 127, 128, 4096])
@pytest.mark.parametrize("two", [False, True], ids=["mid", "mid2"])
def test_density_head_kernels_against_the_witness(hip, two, B, masked):
    H = hip.NgpHeadBackend
    rng, dirs, sh16, h = head_inputs(B, B + two)
    nv, v = valid_count(B, masked)
    enc = rng.integers(-8, 9, (16, B, 2)).astype(np.float64) / 4
    width = 64 if two else 32
    hd, dd = dev16(h), torch.from_numpy(dirs).cuda()
    sigma = torch.full((B,), SENTINEL, device="cuda")
    cin = torch.full((B, width), SENTINEL, dtype=torch.half, device="cuda")
    if two:
        H.mid2_forward(hd, dd, dev16(enc), sigma, cin, n_valid=nv)
        cin_ref = mw.mid2_cin(h, sh16, enc)
    else:
        H.mid_forward(hd, dd, sigma, cin, n_valid=nv)
        cin_ref = mw.mid_cin(h, sh16)
    s_ref, rtol = mw.sigma_with_tolerance(h[:, 0])
    s = sigma.cpu().double().numpy()
    assert (np.abs(s[:v] - s_ref[:v]) <= rtol * s_ref[:v]).all() and (s[v:] == SENTINEL).all()
    assert same(cin[:v, 16:], cin_ref[:v, 16:]), "geometry features, second encoder's features, zero pad"
    assert within_one_ulp(cin[:v, :16], cin_ref[:v, :16]), "SH columns"
    assert same(cin[v:], np.full((B - v, width), SENTINEL))

    # backward
    d_cin = rng.integers(-16, 17, (B, width)).astype(np.float64) / 8
    target = rng.uniform(0.5, 100.0, B) * rng.choice([-1.0, 1.0], B)
    d_sigma = (target * np.exp(-np.clip(h[:, 0], -15, 15))).astype(np.float32)  # keeps d_sigma exp(clamp(h0)) inside binary16
    g0 = mw.mid_grad_h0(d_sigma, h[:, 0])
    for hs in ((16, 1) if two else (16,)):
        h_in = hd if hs == 16 else hd[:, 0].contiguous()
        for ds in (torch.from_numpy(d_sigma).cuda(), None):
            d_h = torch.full((B, 16), SENTINEL, dtype=torch.half, device="cuda")
            if two:
                d_enc = torch.full((16, B, 2), SENTINEL, dtype=torch.half, device="cuda")
                H.mid2_backward(dev16(d_cin), ds, h_in, d_h, d_enc, n_valid=nv)
                enc_ref = mw.mid2_grad_enc(d_cin)
                enc_ref[:, v:] = SENTINEL
                assert same(d_enc, enc_ref), "d_enc"
            else:
                H.mid_backward(dev16(d_cin), ds, h_in, d_h, n_valid=nv)
            assert same(d_h[:v, 1:], mw.mid_grad_routed(d_cin)[:v]) and same(d_h[v:], np.full((B - v, 16), SENTINEL))
            if ds is None:
                assert same(d_h[:v, 0], np.zeros(v))
            else:
                assert within_one_ulp(d_h[:v, 0], g0[:v]), "d_sigma exp(clamp(h0, -15, 15))"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [1, 127, 128, 4096])
def test_colour_head_kernels_against_the_witness(hip, B, masked):
    H = hip.NgpHeadBackend
    rng = np.random.default_rng(B)
    nv, v = valid_count(B, masked)
    out = mw.h16(rng.normal(0, 3, (B, 16)))
    out[:: 5, 0] = rng.choice([-12.0, 12.0, -17.0, 17.0, 0.0], len(out[:: 5]))
    rgb = torch.full((B, 3), SENTINEL, device="cuda")
    H.rgb_forward(dev16(out), rgb, n_valid=nv)
    assert within_one_ulp(rgb[:v], mw.rgb_forward(out)[:v]) and bool((rgb[v:] == SENTINEL).all())
    assert torch.equal(rgb[:v], rgb[:v].half().float()), "the head's values are binary16 values"
    y = rgb.clone()
    y[v:] = 0.5
    d_rgb = rng.normal(0, 1, (B, 3)).astype(np.float32)
    d_out = torch.full((B, 16), SENTINEL, dtype=torch.half, device="cuda")
    H.rgb_backward(torch.from_numpy(d_rgb).cuda(), y, d_out, n_valid=nv)
    assert within_one_ulp(d_out[:v, :3], mw.rgb_backward(d_rgb, y.cpu().double().numpy())[:v])
    assert same(d_out[:v, 3:], np.zeros((v, 13))) and same(d_out[v:], np.full((B - v, 16), SENTINEL))
