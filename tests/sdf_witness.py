"""Witness of the SDF data path's contracts (include/seal3d_hip.h "SDF"), written from the header in numpy: the exact
point-triangle distance by region, the generalised winding number, the signed distance, the MAPE criterion with its gradient, the
dataset's normalisation and its watertight check, the random stream (hash_u32) and two closed meshes to test on.  Everything runs
in the dtype of its inputs (float64 unless a test restates the formula in float32 to measure that format's own error)."""
import numpy as np


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def icosphere(level=0, radius=1.0):
    """(vertices [V, 3] float64, faces [20 * 4^level, 3] int64), outward-facing, vertices on the sphere"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        verts, cache, out = list(v), {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                cache[k] = len(verts) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(verts), np.array(out, dtype=np.int64)
    return v * radius, f


def box(lo=(-0.5, -0.5, -0.5), hi=(0.5, 0.5, 0.5)):
    """axis-aligned box, 8 vertices and 12 outward-facing triangles"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[lo[0] if not i & 1 else hi[0], lo[1] if not i & 2 else hi[1], lo[2] if not i & 4 else hi[2]] for i in range(8)])
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                  [1, 3, 7], [1, 7, 5]], dtype=np.int64)
    return v, f


def box_sdf(p, lo, hi):
    """closed form: negative inside"""
    p = np.asarray(p, np.float64)
    c, h = (np.asarray(lo, np.float64) + hi) / 2, (np.asarray(hi, np.float64) - lo) / 2
    q = np.abs(p - c) - h
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)


# ---- distance, winding, sign -----------------------------------------------------------------------------------------------
TINY = 1e-30


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _seg2(p, e):
    """squared distance of p [..., 3] (relative to the segment's start) to the segment along e"""
    ee = _dot(e, e)
    ok = ee > TINY
    t = np.clip(np.where(ok, _dot(p, e) / np.where(ok, ee, 1), 0), 0, 1).astype(p.dtype)
    v = p - t[..., None] * e
    return _dot(v, v)


def point_triangle(points, tri, want_region=True):
    """(squared distance [N], region [N]) of points [N, 3] to ONE triangle [3, 3]; region: 0 the face, 1 2 3 the edges AB BC CA,
    4 5 6 the vertices A B C (-1: a triangle without area, or not asked for)"""
    p = np.asarray(points)
    A, B, C = (np.asarray(tri)[k].astype(p.dtype) for k in range(3))
    ab, ac, bc = B - A, C - A, C - B
    ap, bp = p - A, p - B
    d_ab, d_bc, d_ca = _seg2(ap, ab), _seg2(bp, bc), _seg2(ap, ac)
    d2 = np.minimum(np.minimum(d_ab, d_bc), d_ca)
    n = np.cross(ab, ac)
    nn = _dot(n, n)
    region = np.full(p.shape[0], -1)
    if nn > TINY:
        # barycentric coordinates of the foot of the perpendicular
        d00, d01, d11, d20, d21 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac), _dot(ap, ab), _dot(ap, ac)
        v, w = d11 * d20 - d01 * d21, d00 * d21 - d01 * d20
        den = d00 * d11 - d01 * d01
        inside = (v >= 0) & (w >= 0) & (v + w <= den)
        plane = _dot(ap, n) ** 2 / nn
        d2 = np.where(inside, np.minimum(d2, plane), d2)
        if not want_region:
            return d2, region
        # the region, for the tests that place points: by the clamped parameters of the nearest edge
        t_ab, t_bc, t_ca = _dot(ap, ab) / d00, _dot(bp, bc) / _dot(bc, bc), _dot(p - C, -ac) / d11
        edge = np.argmin(np.stack([d_ab, d_bc, d_ca]), axis=0)
        t = np.choose(edge, [t_ab, t_bc, t_ca])
        region = np.where(inside, 0, np.where(t <= 0, 4 + edge, np.where(t >= 1, 4 + (edge + 1) % 3, 1 + edge)))
    return d2, region


def solid_angle(points, tri):
    """Omega_f [N] of one triangle (van Oosterom and Strackee); 0 for a face without area and for a point in its plane"""
    p = np.asarray(points)
    A, B, C = (np.asarray(tri)[k].astype(p.dtype) for k in range(3))
    n = np.cross(B - A, C - A)
    if _dot(n, n) <= TINY:
        return np.zeros(p.shape[0], p.dtype)
    a, b, c = A - p, B - p, C - p
    la, lb, lc = (np.sqrt(_dot(x, x)) for x in (a, b, c))
    num = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return np.where(num == 0, 0, 2 * np.arctan2(num, den)).astype(p.dtype)


def mesh_sdf(points, triangles):
    """-> (sdf [N], winding [N], nearest_face [N], dist [N]) of points [N, 3] against triangles [F, 3, 3], in points' dtype"""
    p = np.asarray(points)
    tris = np.asarray(triangles)
    best = np.full(p.shape[0], np.inf, p.dtype)
    face = np.zeros(p.shape[0], np.int64)
    omega = np.zeros(p.shape[0], p.dtype)
    for f in range(tris.shape[0]):
        d2, _ = point_triangle(p, tris[f], want_region=False)
        closer = d2 < best  # (strict: ties stay with the lowest face)
        best, face = np.where(closer, d2, best), np.where(closer, f, face)
        omega = omega + solid_angle(p, tris[f])
    w = omega * p.dtype.type(1 / (4 * np.pi))
    dist = np.sqrt(best)
    return np.where(w > 0.5, -dist, dist), w, face, dist


# ---- the criterion -----------------------------------------------------------------------------------------------------------
def mape(pred, target, clip=None, grad_scale=1.0):
    """-> (loss, grad [B]) of include/seal3d_hip.h's s3d_sdf_mape_forward_backward, in pred's dtype"""
    pred, t = np.asarray(pred).reshape(-1), np.asarray(target).reshape(-1).astype(np.asarray(pred).dtype)
    ft = pred.dtype.type
    p = np.clip(pred, -clip, clip) if clip else pred
    scale = np.abs(t) + ft(1e-2)
    loss = (np.abs(p - t) / scale).mean()
    g = ft(grad_scale) * np.sign(p - t) / (scale * ft(pred.shape[0]))
    if clip:
        g = np.where(np.abs(pred) > clip, ft(0), g)
    return loss, g.astype(pred.dtype)


# ---- the dataset's host side ---------------------------------------------------------------------------------------------
def normalise(vertices):
    """sdf/provider.py:37-43 of the reference: the bounding box's centre to the origin, its diagonal to 2 * 0.95"""
    v = np.asarray(vertices, np.float64)
    lo, hi = v.min(0), v.max(0)
    return (v - (lo + hi) / 2) * (2 / np.sqrt(np.sum((hi - lo) ** 2)) * 0.95)


def watertight(faces):
    """every directed edge occurs once and its reverse occurs once"""
    f = np.asarray(faces)
    edges = {}
    for a, b, c in f:
        for e in ((a, b), (b, c), (c, a)):
            edges[e] = edges.get(e, 0) + 1
    return all(n == 1 and edges.get((b, a), 0) == 1 for (a, b), n in edges.items())


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return float(_dot(a, np.cross(b, c)).sum() / 6)


def face_cdf(triangles):
    t = np.asarray(triangles, np.float64)
    area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) / 2
    return np.cumsum(area) / area.sum()


# ---- the random stream -------------------------------------------------------------------------------------------------------
def _pcg(v):
    v = (v * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    w = (((v >> ((v >> np.uint64(28)) + np.uint64(4))) ^ v) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    return ((w >> np.uint64(22)) ^ w) & np.uint64(0xFFFFFFFF)


def hash_u32(key, step, n):
    """csrc/s3d_common.hpp: pcg_hash(pcg_hash(key ^ step * 0x9E3779B9) + n), n an array"""
    n = np.asarray(n, np.uint64)
    seed = np.uint64((int(key) ^ (int(step) * 0x9E3779B9)) & 0xFFFFFFFF)
    return _pcg((_pcg(seed) + n) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def unit24(w):
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float64) / 2.0 ** 24
