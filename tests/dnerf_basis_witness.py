"""Float64 numpy statement of the D-NeRF temporal-basis density head (csrc/dnerf_basis.hip; DESIGN.md "D-NeRF, temporal basis")
and of the colour fold.  Written from the contract of include/seal3d_hip.h, not from the kernels: real arithmetic without the
contract's rounding points (the half roundings of `pre`, `gh` and the outputs), which the GPU tests bound term by term."""
import numpy as np

ROW, CIN, BASIS = 64, 48, 32


def mid_forward(h, sh, sigma_basis):
    """h [B, 64], sh [B, 16] (SH_4 of the directions), sigma_basis [32] -> sigma [B] = exp(h[:, :32] . sigma_basis), colour-net
    input [B, 48] = [sh | h[:, 32:]]"""
    h = np.asarray(h, dtype=np.float64)
    pre = h[:, :BASIS] @ np.asarray(sigma_basis, dtype=np.float64)
    return np.exp(pre), np.concatenate([np.asarray(sh, dtype=np.float64), h[:, BASIS:]], axis=1)


def mid_backward(g_cin, g_sigma, h, sigma_basis, rows=None):
    """-> (grad_h [B, 64], grad_sigma_basis [32]).  g = grad_sigma * exp(clamp(pre, -15, 15)); grad_h[:, :32] = g sb,
    grad_h[:, 32:] = g_cin[:, 16:]; grad_sigma_basis = sum over the rows in front of `rows` of g_b h_b[:32].  g_sigma None: zeros."""
    h = np.asarray(h, dtype=np.float64)
    sb = np.asarray(sigma_basis, dtype=np.float64)
    B = h.shape[0]
    out = np.zeros((B, ROW))
    out[:, BASIS:] = np.asarray(g_cin, dtype=np.float64)[:, CIN - (ROW - BASIS):]
    if g_sigma is None:
        return out, np.zeros(BASIS)
    pre = h[:, :BASIS] @ sb
    g = np.asarray(g_sigma, dtype=np.float64) * np.exp(np.clip(pre, -15.0, 15.0))
    out[:, :BASIS] = g[:, None] * sb[None, :]
    live = B if rows is None else min(rows, B)
    return out, (g[:live, None] * h[:live, :BASIS]).sum(axis=0)


def fold(w2, color_basis):
    """W_eff [3, H]: W_eff[c] = sum_k color_basis[k] w2[K c + k]"""
    w2 = np.asarray(w2, dtype=np.float64)
    cb = np.asarray(color_basis, dtype=np.float64)
    return np.einsum("k,ckj->cj", cb, w2.reshape(3, cb.shape[0], w2.shape[1]))


def contraction(hidden, w2, color_basis):
    """the reference's explicit form: (hidden @ w2.T).view(-1, 3, K) @ color_basis  -> [B, 3] (before the sigmoid)"""
    out = np.asarray(hidden, dtype=np.float64) @ np.asarray(w2, dtype=np.float64).T
    return out.reshape(out.shape[0], 3, -1) @ np.asarray(color_basis, dtype=np.float64)
