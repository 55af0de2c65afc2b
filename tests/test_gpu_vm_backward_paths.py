"""The two TensoRF factor-backward entry points (s3d_vm_features_backward / s3d_vm_color_backward, csrc/tensorf.hip) share one
host path: its checks, in their order and with each entry point's own prefix, and every arm of its launch ladder at the
smallest shape that reaches it, against oracle/vm_features.py."""
import functools
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAT_IDS, VEC_IDS = ((0, 1), (0, 2), (1, 2)), (2, 1, 0)


def _factors(ranks, res, g, scale=1.0):
    planes = [torch.randn(1, ranks[i], res[MAT_IDS[i][1]], res[MAT_IDS[i][0]], generator=g) * scale for i in range(3)]
    lines = [torch.randn(1, ranks[i], res[VEC_IDS[i]], 1, generator=g) * scale for i in range(3)]
    return planes, lines


# ---- (a) the host-side checks: all of them return before any launch

def _call(V, kind, ranks, res, N=64, n_bounds=None):
    g = torch.Generator().manual_seed(1)
    planes, lines = _factors(ranks, res, g)
    pd, ld = [p.cuda() for p in planes], [l.cuda() for l in lines]
    x = (torch.rand(N, 3, generator=g) * 2 - 1).cuda()
    rows = sum(ranks)
    bins = None
    if n_bounds is not None:
        bins = (torch.zeros(6, N, dtype=torch.int32, device="cuda"), torch.zeros(6, n_bounds, dtype=torch.int32, device="cuda"), n_bounds)
    if kind == "features":
        return V.features_backward(x, pd, ld, res, False, torch.zeros(N, rows, device="cuda"), bins)
    basis = torch.zeros(27, rows, dtype=torch.float16, device="cuda")
    return V.color_backward(x, pd, ld, res, basis, torch.zeros(N, 27, dtype=torch.float16, device="cuda"), bins)


@pytest.mark.parametrize("kind", ["features", "color"])
def test_factor_backward_refuses_ranks_above_64_under_its_own_name(hip, kind):
    msg = {"features": "vm_features_backward: rank 80 > 64 not supported", "color": "vm_color_backward: rank 80 > 64"}[kind]
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _call(hip.VmBackend, kind, [80, 80, 80], [4, 4, 4])


@pytest.mark.parametrize("kind", ["features", "color"])
def test_factor_backward_refuses_a_start_table_with_too_few_columns(hip, kind):
    with pytest.raises(RuntimeError, match=re.escape(f"vm_{kind}_backward: `start` needs more than")):
        _call(hip.VmBackend, kind, [4, 4, 4], [24, 24, 24], n_bounds=2)


@pytest.mark.parametrize("kind", ["features", "color"])
def test_factor_backward_checks_the_rank_before_the_start_table(hip, kind):
    with pytest.raises(RuntimeError, match=re.escape(f"vm_{kind}_backward: rank 80 > 64")):
        _call(hip.VmBackend, kind, [80, 80, 80], [24, 24, 24], n_bounds=2)


# ---- (b) the launch ladder.  Resolution [9, 70, 10]: several 8 x 8 tiles per plane (shared window borders) and two 64-cell line
# chunks along one axis; a third of the points lies partly outside.

RES = [9, 70, 10]
N_POINTS = 700


@functools.lru_cache(maxsize=None)
def _inputs(ranks):
    """(x, planes, lines, grad [N], grad [N, rows], g_out fp16 [N, 27], basis fp16 [27, rows]) on the CPU, seeded per rank set"""
    g = torch.Generator().manual_seed(100 + sum(ranks))
    planes, lines = _factors(ranks, RES, g)
    x = torch.rand(N_POINTS, 3, generator=g) * 2.4 - 1.2
    rows = sum(ranks)
    gs, gc = torch.randn(N_POINTS, generator=g), torch.randn(N_POINTS, rows, generator=g)
    g_out = (torch.randn(N_POINTS, 27, generator=g) * 0.05).half()
    basis = (torch.randn(27, rows, generator=g) * 0.3).half()
    return x, planes, lines, gs, gc, g_out, basis


# (ranks, points, which arm of the ladder the call takes)
LADDER = [
    ((2, 1, 3), 700, "lane kernels at 16 ranks per point"),
    ((16, 16, 16), 700, "equal ranks below the matrix-core threshold"),
    ((32, 32, 16), 700, "matrix-core arm refused: 64-lane kernels"),
    ((32, 32, 32), 700, "matrix-core arm, two ranges"),
    ((32, 32, 32), 300, "matrix-core arm, one partial range"),
]
MODES = {(2, 1, 3): ("reduce",), (16, 16, 16): ("rows",)}
CASES = [(r, n, m) for r, n, _ in LADDER for m in MODES.get(r, ("reduce", "rows", "color"))]


@pytest.mark.parametrize("ranks,N,mode", CASES, ids=[f"{'-'.join(map(str, r))}/{n}/{m}" for r, n, m in CASES])
def test_factor_backward_ladder_matches_the_cpu_oracle(hip, ranks, N, mode):
    from oracle import vm_features as vo
    V = hip.VmBackend
    x, planes, lines, gs, gc, g_out, basis = _inputs(ranks)
    x, gs, gc, g_out = x[:N].contiguous(), gs[:N].contiguous(), gc[:N].contiguous(), g_out[:N].contiguous()
    xn, pn, ln = x.numpy(), [p[0].numpy() for p in planes], [l[0, :, :, 0].numpy() for l in lines]
    pd, ld, xd = [p.cuda() for p in planes], [l.cuda() for l in lines], x.cuda()
    rows = sum(ranks)
    if mode == "color":
        gp, gl, gb = V.color_backward(xd, pd, ld, RES, basis.cuda(), g_out.cuda())
        # the products' gradient (g_out . W)^T and the basis gradient g_out^T . products, in float64 from the fp16 operands
        grad_rows = (g_out.double() @ basis.double()).numpy().T
        ref_b = g_out.double().numpy().T @ vo.color_products(xn, pn, ln).astype(np.float64).T
        rp, rl = vo.factor_grads(xn, pn, ln, grad_rows)
        got, ref = gp + gl + [gb], rp + rl + [ref_b]
        rtol, atol = 2e-2, 2e-3  # (test_tensorf_color_features_with_basis_mat_in_the_kernel, the same quantities)
    else:
        reduce = mode == "reduce"
        gp, gl = V.features_backward(xd, pd, ld, RES, reduce, (gs if reduce else gc).cuda())
        grad_rows = np.tile(gs.numpy()[None], (rows, 1)) if reduce else gc.numpy().T
        rp, rl = vo.factor_grads(xn, pn, ln, grad_rows)
        got, ref = gp + gl, rp + rl
        rtol, atol = 1e-4, 2e-5  # (test_tensorf_vm_kernels_match_cpu_oracle)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert float(np.abs(b).max()) > 0
        np.testing.assert_allclose(a.cpu().numpy().reshape(b.shape), b, rtol=rtol, atol=atol * float(np.abs(b).max()))
