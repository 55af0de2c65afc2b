"""Float64 numpy statement of the D-NeRF glue (csrc/dnerf.hip; DESIGN.md "D-NeRF"): the two input rows, the warp, the
regulariser's sum and the warp's backward.  Written from the contracts of include/seal3d_hip.h, not from the kernels."""
import numpy as np

DIN, SIN, GRID_COLS = 80, 112, 32


def freq(x, degree):
    """[x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) | ...]: blocks of D columns (s3d_freq_encode_forward's column order)"""
    # the encoder's contract is sin(fl32(2^f x + phase)) with phase 0 or fl32(pi / 2): the scaling by a power of two is exact, the
    # phase is added in fp32 (at 2^9 x the rounding of that sum is 6e-5 of argument, far above fp32 sine error), the sine is exact here
    x32 = np.asarray(x, dtype=np.float32)
    cols = [x32.astype(np.float64)]
    for f in range(degree):
        a = x32 * np.float32(2.0 ** f)
        cols += [np.sin(a.astype(np.float64)), np.sin((a + np.float32(np.pi / 2)).astype(np.float64))]
    return np.concatenate(cols, axis=1)


def times_of(t, B):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    return np.repeat(t, B, axis=0) if t.shape[0] == 1 else t


def din_row(x, t):
    """[B, 80] = [freq_10(x) (63) | freq_6(t) (13) | 0 (4)]"""
    B = x.shape[0]
    row = np.zeros((B, DIN))
    row[:, :63] = freq(x, 10)
    row[:, 63:76] = freq(times_of(t, B), 6)
    return row


def sin_row(grid_features, x, t):
    """[B, 112] = [grid(x') (2 L <= 32, zero behind) | freq_10(x) | freq_6(t) | 0 (4)]"""
    B = x.shape[0]
    row = np.zeros((B, SIN))
    g = np.asarray(grid_features, dtype=np.float64)
    row[:, :g.shape[1]] = g
    row[:, GRID_COLS:] = din_row(x, t)
    return row


def warp(x, dout):
    """x' = x + dout[:, :3] and the deformation itself"""
    deform = np.asarray(dout, dtype=np.float64)[:, :3]
    return np.asarray(x, dtype=np.float64) + deform, deform


def reg_sum(deform, rows=None):
    d = np.asarray(deform, dtype=np.float64)
    return np.abs(d if rows is None else d[:rows]).sum()


def regulariser(deform, weight=1e-3, rows=None):
    """weight * mean |deform| over the live rows and three columns"""
    n = deform.shape[0] if rows is None else rows
    return weight * reg_sum(deform, rows) / (3.0 * n)


def warp_backward(g_xw, deform, coef=None, scale=1.0, rows=None):
    """[B, 16]: columns 0..2 = coef * sign(deform) + g_xw * scale (sign(0) = 0; rows at or behind `rows` take no coef), rest zero"""
    g = np.asarray(g_xw, dtype=np.float64) * scale
    if coef is not None:
        s = np.sign(np.asarray(deform, dtype=np.float64))
        if rows is not None:
            s[rows:] = 0.0
        g = g + coef * s
    out = np.zeros((g.shape[0], 16))
    out[:, :3] = g
    return out


def split_grad(g_sin, L):
    """columns 0..2L-1 of [B, 112] as level-major [L, B, 2]"""
    g = np.asarray(g_sin)
    return np.ascontiguousarray(g[:, :2 * L].reshape(g.shape[0], L, 2).transpose(1, 0, 2))
