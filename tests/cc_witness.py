"""Float64 numpy witness of the CCNeRF contract (include/seal3d_hip.h: s3d_cc_*; tensoRF/network_cc.py:128-250, :287-291 of the
reference), for the tests of the fused kernels.

A group is a dict: `lines` (three [R, D_i] along coordinate VEC_IDS[i]) + `s_vec` [C, R] and / or `planes` (three [R, H_i, W_i],
plane i spans the coordinates MAT_IDS[i] = (m0, m1): m0 along the last axis) + `s_mat` [C, R]; an absent component is None.
Every axis is sampled the way grid_sample does with bilinear, zeros padding and align_corners=FALSE:

    p = ((u + 1) * D - 1) / 2            in fp32, like the sampler (it decides the cell)
    i0 = floor(p), w = p - i0
    value = v[i0] * (1 - w) + v[i0 + 1] * w      a tap outside [0, D - 1] counts as zero

so a point up to one cell outside [-1, 1] still reads a value.  The vector product is l0[r] * l1[r] * l2[r], the matrix product
p0[r] * p1[r] * p2[r]; level k is the sum over groups g <= k of S_vec_g @ f_vec_g + S_mat_g @ f_mat_g; the colour head contracts
the 3 * degree^2 rows of a level with the SH basis of the direction.  Everything after `p` is float64."""
import numpy as np

VEC_IDS = (2, 1, 0)
MAT_IDS = ((0, 1), (0, 2), (1, 2))


def locate(u, D):
    """(i0, w0, w1, b0, b1) of coordinates u [N] on an axis of D cells"""
    u = np.asarray(u, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = ((u + np.float32(1)) * np.float32(D) - np.float32(1)) / np.float32(2)
        ok = np.abs(p) < 1e9  # (non-finite: both taps out of range)
    fl = np.floor(np.where(ok, p, 0)).astype(np.float64)
    i0 = np.where(ok, fl, -2).astype(np.int64)
    w1 = np.where(ok, p.astype(np.float64) - fl, 0.0)
    w0 = 1.0 - w1
    return i0, w0, w1, (i0 >= 0) & (i0 < D), (i0 + 1 >= 0) & (i0 + 1 < D)


def _line_taps(x, v, a):
    """[(cell index [N], weight [N], in range [N])] x 2 of line v [R, D] along coordinate a"""
    i0, w0, w1, b0, b1 = locate(np.asarray(x)[:, a], v.shape[1])
    return [(i0, w0, b0), (i0 + 1, w1, b1)]


def _plane_taps(x, v, m0, m1):
    """the four taps of plane v [R, H, W] as flat cell indices into [H * W]"""
    H, W = v.shape[1:]
    ix, wx0, wx1, bx0, bx1 = locate(np.asarray(x)[:, m0], W)
    iy, wy0, wy1, by0, by1 = locate(np.asarray(x)[:, m1], H)
    taps = []
    for dy, wy, by in ((0, wy0, by0), (1, wy1, by1)):
        for dx, wx, bx in ((0, wx0, bx0), (1, wx1, bx1)):
            taps.append(((iy + dy) * W + ix + dx, wx * wy, bx & by))
    return taps


def _sample(v2, taps):
    """sum over taps of v2[:, cell] * weight, v2 [R, cells] -> [R, N]"""
    out = np.zeros((v2.shape[0], taps[0][0].shape[0]))
    for idx, w, b in taps:
        out += np.where(b[None], v2[:, np.clip(idx, 0, v2.shape[1] - 1)], 0.0) * w[None]
    return out


def line_values(x, lines):
    """l[i] [R, N] of the three lines"""
    return [_sample(np.asarray(v, dtype=np.float64), _line_taps(x, np.asarray(v), a)) for v, a in zip(lines, VEC_IDS)]


def plane_values(x, planes):
    """p[i] [R, N] of the three planes"""
    return [_sample(np.asarray(v, dtype=np.float64).reshape(v.shape[0], -1), _plane_taps(x, np.asarray(v), m0, m1))
            for v, (m0, m1) in zip(planes, MAT_IDS)]


def group_products(x, group):
    """(f_vec [R_vec, N] or None, f_mat [R_mat, N] or None)"""
    fv = fm = None
    if group.get("lines") is not None:
        l = line_values(x, group["lines"])
        fv = l[0] * l[1] * l[2]
    if group.get("planes") is not None:
        p = plane_values(x, group["planes"])
        fm = p[0] * p[1] * p[2]
    return fv, fm


def levels(x, groups, residual=True):
    """the cumulative per-level rows [K_out, C, N]"""
    out, last = [], 0.0
    for g in groups:
        fv, fm = group_products(x, g)
        y = last
        if fv is not None:
            y = y + np.asarray(g["s_vec"], dtype=np.float64) @ fv
        if fm is not None:
            y = y + np.asarray(g["s_mat"], dtype=np.float64) @ fm
        out.append(y)
        last = y
    return np.stack(out) if residual else np.stack(out[-1:])


def sh_basis(dirs, degree):
    """real spherical harmonics of degree <= 4 [N, degree^2] (the polynomial form of shencoder, unit directions)"""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    cols = [0.28209479177387814 * np.ones_like(x),
            -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
            1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * zz - 0.31539156525251999,
            -1.0925484305920792 * xz, 0.54627421529603959 * (xx - yy),
            0.59004358992664352 * y * (-3.0 * xx + yy), 2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * zz),
            0.3731763325901154 * z * (5.0 * zz - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * zz),
            1.4453057213202769 * z * (xx - yy), 0.59004358992664352 * x * (-xx + 3.0 * yy)]
    assert 1 <= degree <= 4
    return np.stack(cols[:degree * degree], axis=1)


def features(x, groups, residual=True):
    """the density head [K_out, N]"""
    return levels(x, groups, residual)[:, 0]


def color(x, dirs, groups, degree, residual=True):
    """the colour head's logits [K_out, N, 3]"""
    y = levels(x, groups, residual)  # [K, 3 B, N]
    K, _, N = y.shape
    return np.einsum("kcbn,nb->knc", y.reshape(K, 3, degree * degree, N), sh_basis(dirs, degree))


def row_grads(g, groups_n, residual, dirs=None, degree=0):
    """the gradient that reaches every group's rows, [n_groups][C, N]: the suffix sum over the levels (group g receives every
    level >= g) of g [K_out, N] (density) or of g [K_out, N, 3] spread over the SH basis"""
    g = np.asarray(g, dtype=np.float64)
    if degree:
        g = np.einsum("knc,nb->kcbn", g, sh_basis(dirs, degree)).reshape(g.shape[0], 3 * degree * degree, g.shape[1])
    else:
        g = g[:, None, :]
    if not residual:
        return [g[0]] * groups_n
    suffix = np.cumsum(g[::-1], axis=0)[::-1]
    return [suffix[k] for k in range(groups_n)]


def _scatter(gl, taps, cells):
    """gl [R, N] scattered to [R, cells] through the taps"""
    out = np.zeros((gl.shape[0], cells))
    for idx, w, b in taps:
        sel = np.nonzero(b)[0]
        term = gl[:, sel] * w[sel][None]
        for r in range(gl.shape[0]):
            np.add.at(out[r], idx[sel], term[r])
    return out


def grads(x, groups, g, residual=True, dirs=None, degree=0):
    """gradients of sum(g * head) w.r.t. every factor and S: a list of dicts shaped like `groups`"""
    dys = row_grads(g, len(groups), residual, dirs, degree)
    out = []
    for grp, dy in zip(groups, dys):
        res = dict(lines=None, planes=None, s_vec=None, s_mat=None)
        if grp.get("lines") is not None:
            l = line_values(x, grp["lines"])
            df = np.asarray(grp["s_vec"], dtype=np.float64).T @ dy  # [R, N]
            res["s_vec"] = dy @ (l[0] * l[1] * l[2]).T
            res["lines"] = []
            for i, a in enumerate(VEC_IDS):
                j, k = [q for q in range(3) if q != i]
                v = np.asarray(grp["lines"][i])
                res["lines"].append(_scatter(df * l[j] * l[k], _line_taps(x, v, a), v.shape[1]))
        if grp.get("planes") is not None:
            p = plane_values(x, grp["planes"])
            df = np.asarray(grp["s_mat"], dtype=np.float64).T @ dy
            res["s_mat"] = dy @ (p[0] * p[1] * p[2]).T
            res["planes"] = []
            for i, (m0, m1) in enumerate(MAT_IDS):
                j, k = [q for q in range(3) if q != i]
                v = np.asarray(grp["planes"][i])
                res["planes"].append(_scatter(df * p[j] * p[k], _plane_taps(x, v, m0, m1), v.shape[1] * v.shape[2]).reshape(v.shape))
        out.append(res)
    return out
