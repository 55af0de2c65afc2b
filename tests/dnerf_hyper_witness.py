"""Float64 numpy statement of the backward of the D-NeRF hyper grid lookup (csrc/dnerf_hyper.hip; DESIGN.md "D-NeRF, hyper") and of
the padded density head.  Written from the contract of include/seal3d_hip.h, not from the kernels: real arithmetic on the same fp16
/ fp32 inputs, without the kernel's fp32 roundings, which the GPU tests bound term by term."""
import numpy as np

BLOCK, MAX_BLOCKS = 256, 512  # the launch of s3d_dnerf_hyper_grid_backward: min(512, ceil(B / 256)) workgroups of 256 lanes


def grid_backward(grad_feat, dy_da, grad_scale, rows=None):
    """grad_feat [B, 2 L], dy_da [B, L, 2] or None -> (grad_levels [L, B, 2] — the transposition, exact — , grad_ambient, abs_sum):
    grad_ambient = grad_scale * sum over the rows in front of `rows` and the columns of g_bk j_bk; abs_sum the same sum of
    |g_bk j_bk| (what the error bound of the fp32 sum scales with)"""
    g = np.asarray(grad_feat, dtype=np.float64)
    B, L = g.shape[0], g.shape[1] // 2
    levels = np.ascontiguousarray(g.reshape(B, L, 2).transpose(1, 0, 2))
    if dy_da is None:
        return levels, 0.0, 0.0
    live = B if rows is None else min(rows, B)
    terms = g[:live] * np.asarray(dy_da, dtype=np.float64).reshape(B, 2 * L)[:live]
    return levels, float(terms.sum() * grad_scale), float(np.abs(terms).sum() * abs(grad_scale))


def longest_chain(B, L):
    """the longest chain of fp32 additions behind grad_ambient in the documented order: a row's 2 L fused multiply-adds, a lane's
    rows, the exchange tree of a wave (6), the waves of a workgroup (4), then in the last workgroup a lane's partials, the tree, the
    waves; + 1 for the product with grad_scale"""
    G = min(MAX_BLOCKS, max(1, -(-B // BLOCK)))
    rows_per_lane = -(-B // (G * BLOCK))
    partials_per_lane = -(-G // BLOCK)
    return 2 * L + rows_per_lane + 6 + 4 + partials_per_lane + 6 + 4 + 1


def padded_head_weight(w):
    """the density net's last matrix [33, H] as the 64 rows the density-head kernel reads: row 0 sigma, rows 1..31 zero, rows
    32..63 the 32 feature rows"""
    w = np.asarray(w, dtype=np.float64)
    return np.concatenate([w[:1], np.zeros((31, w.shape[1])), w[1:]], axis=0)


E0 = np.eye(32, dtype=np.float64)[0]  # the constant basis of the head
