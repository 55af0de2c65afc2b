"""Float64 numpy witness of the CP line-factor contract (include/seal3d_hip.h: s3d_cp_*; tensoRF/network_cp.py:78-111 of the
reference), for the tests of the fused kernels.

Line i is `[R, D_i]` along coordinate VEC_IDS[i] and is sampled at u = x[n][VEC_IDS[i]] the way grid_sample samples the fake-2D
`[1, R, D, 1]` tensor (bilinear, zeros padding, align_corners=True):

    p = ((u + 1) / 2) * (D - 1)          in fp32, like the sampler (it decides the cell)
    i0 = floor(p), w = p - i0
    value = v[i0] * (1 - w) + v[i0 + 1] * w      a tap outside [0, D - 1] counts as zero

and the product is f[r][n] = l0[r] * l1[r] * l2[r].  Everything after `p` is float64.  Besides values and gradients the
gradient functions return, per gradient cell, the number of terms `n_cell` and `sum |term|` — what a bound on an fp32 sum in
any order is made of."""
import numpy as np

VEC_IDS = (2, 1, 0)


def locate(u, D):
    """(i0, w0, w1, b0, b1) of coordinates u [N] on a line of D cells"""
    u = np.asarray(u, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = ((u + np.float32(1)) / np.float32(2)) * np.float32(D - 1)
        ok = np.abs(p) < 1e9  # (non-finite: both taps out of range)
    fl = np.floor(np.where(ok, p, 0)).astype(np.float64)
    i0 = np.where(ok, fl, -2).astype(np.int64)
    w1 = np.where(ok, p.astype(np.float64) - fl, 0.0)
    w0 = 1.0 - w1
    b0 = (i0 >= 0) & (i0 < D)
    b1 = (i0 + 1 >= 0) & (i0 + 1 < D)
    return i0, w0, w1, b0, b1


def line_values(x, lines):
    """l[i] [R, N] float64 for the three lines `lines[i]` [R, D_i] at points x [N, 3], and the taps"""
    x = np.asarray(x)
    vals, taps = [], []
    for i, a in enumerate(VEC_IDS):
        v = np.asarray(lines[i], dtype=np.float64)
        D = v.shape[1]
        i0, w0, w1, b0, b1 = locate(x[:, a], D)
        v0 = np.where(b0[None], v[:, np.clip(i0, 0, D - 1)], 0.0)
        v1 = np.where(b1[None], v[:, np.clip(i0 + 1, 0, D - 1)], 0.0)
        vals.append(v0 * w0[None] + v1 * w1[None])
        taps.append((i0, w0, w1, b0, b1))
    return vals, taps


def products(x, lines):
    """f [R, N]"""
    l, _ = line_values(x, lines)
    return l[0] * l[1] * l[2]


def features(x, lines):
    """sigma_feat [N] = sum_r f[r][n]"""
    return products(x, lines).sum(0)


def line_grads(x, lines, g):
    """gradients of sum(g * out) w.r.t. the lines.  g: [N] (out = features) or [R, N] (out = products).
    Returns (grads [R, D_i] x 3, n_cell [D_i] x 3, abs_sum [R, D_i] x 3)."""
    l, taps = line_values(x, lines)
    R = l[0].shape[0]
    g = np.asarray(g, dtype=np.float64)
    g = np.broadcast_to(g[None], (R, g.shape[0])) if g.ndim == 1 else g
    grads, counts, sums = [], [], []
    for i in range(3):
        j, k = [a for a in range(3) if a != i]
        gl = g * l[j] * l[k]  # [R, N]
        D = np.asarray(lines[i]).shape[1]
        i0, w0, w1, b0, b1 = taps[i]
        gr, sa, nc = np.zeros((R, D)), np.zeros((R, D)), np.zeros(D, dtype=np.int64)
        for idx, w, b in ((i0, w0, b0), (i0 + 1, w1, b1)):
            sel = np.nonzero(b)[0]
            term = gl[:, sel] * w[sel][None]
            for r in range(R):
                np.add.at(gr[r], idx[sel], term[r])
                np.add.at(sa[r], idx[sel], np.abs(term[r]))
            np.add.at(nc, idx[sel], 1)
        grads.append(gr)
        counts.append(nc)
        sums.append(sa)
    return grads, counts, sums


def basis_features(x, lines, W):
    """basis_mat(f.T) [N, C] in float64 (no binary16 rounding), W [C, R]"""
    return products(x, lines).T @ np.asarray(W, dtype=np.float64).T


def basis_grads(x, lines, W, go):
    """gradients of sum(go * basis_features) w.r.t. the lines and W: (line grads, n_cell, abs_sum, grad_W [C, R])"""
    W, go = np.asarray(W, dtype=np.float64), np.asarray(go, dtype=np.float64)
    gl, nc, sa = line_grads(x, lines, W.T @ go.T)
    return gl, nc, sa, go.T @ products(x, lines).T
