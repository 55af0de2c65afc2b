"""The order of additions of csrc/ordered_sum.hpp in numpy float32, written from the header's comment (not from the kernels):

    a lane         its own terms in index order
    a wave         shfl_down by 32, 16, 8, 4, 2, 1: lane 0 holds the sum
    a workgroup    its four waves in index order, ((p0 + p1) + p2) + p3: one partial per workgroup
    the launch     lane i of the last workgroup adds the partials i, i + 256, ... in index order from 0, then the same wave and
                   workgroup steps

Every addition is one float32 addition, so the result is the kernel's bit for bit when the terms are."""
import numpy as np

BLOCK = 256


def _wave_tree(v):
    """[..., 64] -> [...]: what lane 0 holds behind v += shfl_down(v, o) for o = 32 .. 1 (lane i < o reads lane i + o)"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(v, block):
    """[..., block] -> [...]: the waves' trees, then the waves in index order"""
    p = _wave_tree(v.reshape(v.shape[:-1] + (block // 64, 64)))
    r = p[..., 0]
    for w in range(1, block // 64):
        r = r + p[..., w]
    return r


def _lane_sums(terms, stride):
    """running sums from 0 of terms[i], terms[i + stride], ... -> [stride]"""
    n = len(terms)
    rows = -(-n // stride) if n else 0
    padded = np.zeros(max(rows, 1) * stride, np.float32)  # (s + 0 == s: a lane without a row adds nothing)
    padded[:n] = terms
    s = np.zeros(stride, np.float32)
    for r in padded.reshape(-1, stride):
        s = s + r
    return s


def ordered_sum(terms, groups, block=BLOCK, strided=True):
    """terms: the per-row fp32 terms in row order.  `strided`: lane i of workgroup g owns the rows g block + i + k groups block
    (a grid of fixed size); else one row per lane, one chunk of `block` rows per workgroup.  -> np.float32"""
    terms = np.asarray(terms)
    assert terms.dtype == np.float32 and terms.ndim == 1 and block % 64 == 0 and groups >= 1
    assert strided or groups == max(1, -(-len(terms) // block)), "one row per lane: one workgroup per chunk"
    partials = _block_sum(_lane_sums(terms, groups * block).reshape(groups, block), block)
    assert partials.dtype == np.float32
    return np.float32(_block_sum(_lane_sums(partials, block), block))
