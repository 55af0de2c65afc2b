"""The sampling path without the occupancy grid, without a GPU: the float64 witness (tests/hier_witness.py) against the project's own
torch route on the CPU and against float64 autograd, the provenance of the tolerances the GPU tests use (tests/hier_cases.py), and
the binding's refusals."""
import numpy as np
import pytest
import torch

import hier_cases as C
import hier_witness as W

from hier_cases import analytic_color_np, gauss_density_np, gauss_renderer


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_witness_matches_the_torch_route_on_cpu(oracle_wrappers, train):
    """The project's `run` on CPU tensors (the torch route, always) against the witness on the semi-transparent scene, which keeps
    every ray below weights_sum = 0.9: no pdf bin falls under the 1e-5 rule, so fp32 and float64 draw the same samples up to
    rounding and every pixel agrees to 1e-4 of the value range.  Training: the jitter and the pdf's uniforms are the same draws."""
    N, S, U = 300, 64, 48
    o, d = C.rays(N, "mixed")
    R = gauss_renderer()
    R.train(train)
    torch.manual_seed(5)
    with torch.no_grad():
        got = R.run(torch.tensor(o), torch.tensor(d), num_steps=S, upsample_steps=U, bg_color=1, perturb=train)
    assert R.last_sampling_route == "torch"
    noise = u = None
    if train:
        torch.manual_seed(5)
        noise, u = torch.rand((N, S)).numpy(), torch.rand([N, U]).numpy()
    image, depth, ws = W.render(o, d, C.AABB, C.MIN_NEAR, S, U, C.SCALE, gauss_density_np, analytic_color_np, noise, u)
    assert 0.5 < float(ws.max()) <= 0.9, float(ws.max())  # (the scene's bound, and a real picture)
    assert np.isnan(depth[0]) and np.isfinite(depth[1:]).all()  # (ray 0 misses the box)
    for key, ref in (("image", image), ("depth", depth), ("weights_sum", ws)):
        err = C.err_abs(got[key].numpy(), ref)
        print(f"{key}: max |torch fp32 - witness| = {err:.3e}")
        assert err <= 1e-4 * float(np.nanmax(np.abs(ref))), key


@pytest.mark.parametrize("case", [(1, 3, 1, "miss"), (1, 3, 1, "inside"), (63, 65, 63, "mixed"), (65, 64, 0, "mixed")], ids=C.case_id)
def test_witness_backward_matches_float64_autograd(case):
    """the hand-derived backward of the witness against torch.autograd over the reference's op sequence in float64, sigma from
    empty to opaque; forward values too"""
    N, S, U, kind = case
    inp = C.composite_inputs(N, S, U, kind)
    ref, got = C.witness_composite(inp, S), C.torch_composite(inp, S, dtype=torch.float64)
    for k in ("weights", "weights_sum", "depth", "image"):
        assert C.err_abs(got[k].numpy(), ref[k]) <= 1e-12, k
    for k in ("grad_sigma", "grad_rgbs"):
        assert C.err_rel(got[k].numpy(), ref[k]) <= 1e-10, k
    hit = inp["nears"] < C.FLT_MAX
    assert np.isfinite(ref["grad_sigma"][hit]).all() and np.isnan(ref["grad_sigma"][~hit]).all()
    assert float(inp["sigma_cat"].max()) > 1e3 or N == 1


def test_witness_upsampling_matches_the_torch_ops_in_float64():
    for case in [(63, 64, 48, "mixed"), (65, 65, 63, "mixed"), (1, 3, 1, "inside")]:
        N, S, U, kind = case
        inp = C.upsample_inputs(N, S, U, kind)
        for u in (None, inp["u"]):
            new_z, _, z_sorted, order = W.upsample(inp["z"], inp["sigma"], inp["nears"], inp["fars"], C.SCALE, u, U, inp["rays_o"],
                                                   inp["rays_d"], C.AABB)
            # (the deterministic row is torch.linspace's fp32 values there and exact here: half an fp32 ulp of u, times the
            #  inverse CDF's slope of at most 4 (S - 2) bins of 1 / (S - 1) each)
            assert C.err_new_z(C.torch_upsample(inp, u, dtype=torch.float64).numpy(), new_z, inp) <= (4 * 2.0 ** -24 if u is None else 1e-12)
            both = np.concatenate([inp["z"].astype(np.float64), new_z], axis=1)
            assert np.array_equal(np.take_along_axis(both, order, axis=1), z_sorted) and (np.diff(z_sorted, axis=1) >= 0).all()


def test_recorded_torch_errors_are_what_the_torch_ops_give():
    """TORCH_ERROR (tests/hier_cases.py) is a measurement: the torch fp32 op sequence against the witness on the cases the GPU
    tests run.  Re-measured here; torch's CPU kernels may sum in another order on another machine, hence the factor."""
    measured = C.measure_torch_errors()
    for k, v in measured.items():
        print(f"{k}: measured {v:.3e}, recorded {C.TORCH_ERROR[k]:.3e}, kernels allowed {C.bound(k):.3e}")
        assert C.TORCH_ERROR[k] / 3 <= v <= C.TORCH_ERROR[k] * 1.5, k
    # (well-conditioned, as the upsampling cases promise: no pdf bin below 1 / (4 (S - 2)))
    for (N, S, U, kind) in C.UPSAMPLE_CASES:
        inp = C.upsample_inputs(N, S, U, kind)
        hit = inp["nears"] < C.FLT_MAX
        if hit.any():
            w = W.alpha_weights(inp["z"][hit], inp["sigma"][hit], inp["nears"][hit], inp["fars"][hit], C.SCALE, S)[4][:, 1:-1] + 1e-5
            assert float((w / w.sum(axis=1, keepdims=True)).min()) >= 1 / (4 * (S - 2))


def test_binding_refuses_cpu_tensors_and_rows_above_the_cap():
    import s3d_hip
    H = s3d_hip.HierBackend
    cap = H.max_samples()
    assert cap >= 2048 and H.supports(3, 0) and H.supports(cap - 1, 1) and not H.supports(2, 0) and not H.supports(cap, 1)
    f = torch.zeros
    N, S, U = 2, 4, 2
    aabb = torch.tensor(C.AABB)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        H.coarse_samples(f(N, 3), f(N, 3), aabb, 0.2, S, f(N), f(N), f(N, S), f(N, S, 3))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        H.upsample(f(N, S), f(N, S), f(N), f(N), 1.0, None, f(N, 3), f(N, 3), aabb, U, f(N, U), f(N, U, 3), f(N, S + U),
                   f(N, S + U, dtype=torch.int32))
    order = f(N, S + U, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        H.weights(f(N, S + U), order, f(N, S + U), f(N), f(N), 1.0, S, f(N, S + U), f(N, S + U, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        H.composite_forward(f(N, S + U), f(N, S + U, 3), f(N, S + U), order, f(N), f(N), S, f(N), f(N), f(N, 3))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        H.composite_backward(f(N, 3), None, None, f(N, S + U), f(N, S + U, 3), f(N, S + U), order, f(N), f(N), 1.0, S, f(N, S + U),
                             f(N, S + U, 3))
    K = cap + 1
    with pytest.raises(RuntimeError, match="exceeds the cap"):
        H.coarse_samples(f(1, 3), f(1, 3), aabb, 0.2, K, f(1), f(1), f(1, K), f(1, K, 3))
    with pytest.raises(RuntimeError, match="exceeds the cap"):
        H.upsample(f(1, cap), f(1, cap), f(1), f(1), 1.0, None, f(1, 3), f(1, 3), aabb, 1, f(1, 1), f(1, 1, 3), f(1, K),
                   f(1, K, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="exceeds the cap"):
        H.weights(f(1, K), f(1, K, dtype=torch.int32), f(1, K), f(1), f(1), 1.0, cap, f(1, K), f(1, K, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="num_steps >= 3"):
        H.coarse_samples(f(1, 3), f(1, 3), aabb, 0.2, 2, f(1), f(1), f(1, 2), f(1, 2, 3))
    with pytest.raises(RuntimeError, match="order may be omitted"):
        H.composite_forward(f(N, S + U), f(N, S + U, 3), f(N, S + U), None, f(N), f(N), S, f(N), f(N), f(N, 3))
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        H.weights(f(N, S + U), order, f(N, S + U, dtype=torch.float16), f(N), f(N), 1.0, S, f(N, S + U), f(N, S + U, dtype=torch.bool))
