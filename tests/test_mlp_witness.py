"""The float64 MLP witness (tests/mlp_witness.py) checked before it judges the GPU kernels: against a torch float64 autograd twin,
its exact cases against the conditions that make them exact, and against the CPU oracle bit for bit — the construction and the
flat weight layout are proven here, without a GPU."""
import numpy as np
import pytest
import torch

import mlp_witness as mw

ALL_SHAPES = mw.NATIVE_SHAPES + mw.GENERIC_SHAPES


@pytest.mark.parametrize("act", range(7))
@pytest.mark.parametrize("in_dim,W,n", [(16, 32, 2), (48, 16, 3)])
def test_witness_is_the_torch_float64_autograd_twin(act, in_dim, W, n):
    """rounding off: the forward formulas, and the backward formulas that work from the STORED activation, against autograd of an
    independent statement of each activation, to 1e-12 relative (sine: forward only — it has no backward from the stored value)"""
    rng = np.random.default_rng(act + 10 * n)
    B, out_act = 24, (act + 3) % 7
    mats = [rng.uniform(-1, 1, s) * (3.0 / s[1]) ** 0.5 for s in [(W, in_dim)] + [(W, W)] * (n - 1) + [(16, W)]]
    x, grad = rng.normal(0, 0.5, (B, in_dim)), rng.normal(0, 1, (B, 16))
    twin = {
        mw.RELU: torch.relu, mw.EXP: torch.exp, mw.SINE: torch.sin, mw.SIGMOID: torch.sigmoid,
        mw.SQUAREPLUS: lambda v: (v + torch.sqrt(v * v + 4.0 / mw.K_ACT ** 2)) / 2,
        mw.SOFTPLUS: lambda v: torch.nn.functional.softplus(v, beta=mw.K_ACT, threshold=1e9), mw.NONE: lambda v: v,
    }
    xt = torch.from_numpy(x).requires_grad_(True)
    mt = [torch.from_numpy(m).requires_grad_(True) for m in mats]
    h = xt
    for m in mt[:-1]:
        h = twin[act](h @ m.t())
    pre_out = h @ mt[-1].t()
    f = mw.forward(x, mats, act, out_act, rounding=False)

    def close(a, b):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()

    close(f["out_pre"], pre_out.detach().numpy())
    close(f["out"], twin[out_act](pre_out).detach().numpy())
    if act == mw.SINE:
        with pytest.raises(ValueError):
            mw.backward(grad, x, mats, f["acts"], act, rounding=False)
        return
    pre_out.backward(torch.from_numpy(grad))  # the backward pass takes the gradient of the pre-activation output
    b = mw.backward(grad, x, mats, f["acts"], act, rounding=False)
    close(b["grad_inputs"], xt.grad.numpy())
    for got, m in zip(b["gw"], mt):
        close(got, m.grad.numpy())
    assert np.array_equal(mw.flat(mw.split(mw.flat(mats), in_dim, W, n)), mw.flat(mats))


def test_rounding_helpers():
    assert list(mw.h16([2049.0, 2050.0, 2051.0, 65520.0 - 1e-9, 2.0 ** -25])) == [2048.0, 2050.0, 2052.0, 65504.0, 0.0]
    assert list(mw.ulp16([1.0, 1.5, 2.0, 2047.0, 2048.0, 2.0 ** -14, 2.0 ** -20, 0.0])) == [
        2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 1.0, 2.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("act", [0, 6])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_conditions_hold_for_every_gpu_case(shape, act, kind):
    case = mw.exact_case(kind, shape, act, mw.BATCHES[-1])
    for rows in mw.BATCHES + (mw.BATCHES[-1] - 300 + 44,):  # (the row counts of the n_valid runs round up to 128: 77 -> 128)
        assert rows % 128 == 0
        mw.assert_exact(case, rows)
    if shape in mw.BIG_SHAPES:
        mw.assert_exact(mw.exact_case(kind, shape, act, mw.BIG_BATCH))


def test_probe_case_holds_its_ties_and_its_cancellation():
    for act in (0, 6):
        case, hidden, outs = mw.probe_case(act)
        f = mw.forward(case["x"], case["mats"], act)
        exact = mw.forward(case["x"], case["mats"], act, rounding=False)
        assert list(exact["pre"][0][0, :4]) == [2049.0, 2050.0, 2051.0, 16.0] and list(f["acts"][0][0, :4]) == list(hidden)
        assert list(f["out"][0, :7]) == list(outs)
        assert list(f["out"][1, :7]) == ([0.0] * 7 if act == 0 else list(-outs))
        # a binary16 accumulator (rounding after every addition, in index order) loses the sixteen ones
        acc = np.float16(0)
        for v, w in zip(case["x"][0], case["mats"][0][3]):
            acc = np.float16(acc + np.float16(v * w))
        assert float(acc) < 16.0


def _t16(a):
    return torch.from_numpy(np.asarray(a, np.float64).astype(np.float16))


def oracle_run(oracle, case, rows=None, out_act=6):
    """the CPU oracle on a witness case -> (outputs, grad_inputs, grad_weights fp32 sums)"""
    in_dim, W, n, act = case["in_dim"], case["W"], case["n"], case["act"]
    x, grad, w = _t16(case["x"][:rows]), _t16(case["grad"][:rows]), _t16(mw.flat(case["mats"]))
    B = x.shape[0]
    fb, out = torch.empty(n, B, W, dtype=torch.half), torch.empty(B, 16, dtype=torch.half)
    oracle.FFMLPBackend.ffmlp_forward(x, w, B, in_dim, 16, W, n, act, out_act, fb, out)
    if act == mw.SINE:
        return out.double().numpy(), None, None
    bb, gi, gw = torch.zeros(n, B, W, dtype=torch.half), torch.zeros(B, in_dim, dtype=torch.half), torch.zeros_like(w)
    gw32 = oracle.FFMLPBackend.ffmlp_backward(grad, x, w, fb, B, in_dim, 16, W, n, act, out_act, True, bb, gi, gw)
    return out.double().numpy(), gi.double().numpy(), gw32.double().numpy()


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("act", [0, 6])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_equals_the_witness_bit_for_bit_on_the_exact_cases(oracle, shape, act, kind):
    case = mw.exact_case(kind, shape, act, mw.BATCHES[-1])
    rows = mw.BATCHES[-1] if shape in mw.BIG_SHAPES else 384
    ref = mw.run_case(case, rows)
    out, gi, gw = oracle_run(oracle, case, rows)
    assert np.array_equal(out, ref["outputs"]) and np.array_equal(gi, ref["grad_inputs"])
    assert np.array_equal(gw, ref["gw"])  # (fp32 sums of integers below 2^24: exact before the rounding to binary16)


def test_oracle_equals_the_witness_on_the_probes(oracle):
    for act in (0, 6):
        case, _, _ = mw.probe_case(act)
        assert np.array_equal(oracle_run(oracle, case)[0], mw.run_case(case)["outputs"])


@pytest.mark.parametrize("act", [1, 2, 3, 4, 5])
def test_oracle_stays_inside_the_witness_bounds_on_the_chains(oracle, act):
    """the oracle evaluates the activations in fp32, as the kernels do: it must lie within the bounds the witness computes"""
    case = mw.chain_case(32, 64, act)
    ref = mw.chain_bounds(case)
    out, gi, gw = oracle_run(oracle, case)
    assert (np.abs(out - ref["out"]) <= ref["out_bound"]).all()
    assert float((ref["out"] != 0).mean()) > 0.5 and np.isfinite(ref["out"]).all()
    if act != mw.SINE:
        assert (np.abs(gi - ref["grad_inputs"]) <= ref["grad_inputs_bound"]).all()
        assert (np.abs(mw.h16(gw) - ref["gw"]) <= ref["gw_bound"]).all()
        assert np.abs(ref["gw"]).max() < 65504 and float((ref["grad_inputs"] != 0).mean()) > 0.2


@pytest.mark.parametrize("out_act", range(7))
def test_oracle_stays_inside_the_witness_bounds_with_an_output_activation(oracle, out_act):
    for act in (mw.SIGMOID, mw.RELU):
        case = mw.chain_case(32, 64, act)
        ref = mw.chain_bounds(case, out_act=out_act)
        assert (np.abs(oracle_run(oracle, case, out_act=out_act)[0] - ref["out"]) <= ref["out_bound"]).all()


def test_a_wrong_constant_leaves_the_chain_bounds_by_far():
    """the bounds are tight enough to see what they are for: squareplus / softplus evaluated with the scale 9 instead of 10"""
    for act in (mw.SQUAREPLUS, mw.SOFTPLUS):
        case = mw.chain_case(32, 64, act)
        ref = mw.chain_bounds(case)
        k, mw.K_ACT = mw.K_ACT, 9.0
        try:
            wrong = mw.run_case(case)
        finally:
            mw.K_ACT = k
        assert (np.abs(wrong["outputs"] - ref["out"]) / ref["out_bound"]).max() > 10
        assert (np.abs(wrong["grad_inputs"] - ref["grad_inputs"]) / ref["grad_inputs_bound"]).max() > 10
