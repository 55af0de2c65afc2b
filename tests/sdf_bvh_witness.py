"""Witness of the mesh BVH's contract (include/seal3d_hip.h "SDF: BVH query"), written from the header in numpy: the tree (Morton
order, implicit heap, per-node record) node by node from the faces it covers, and the two walks (nearest face with box pruning,
hierarchical winding number) over ANY tree arrays of that layout.  The walks read the pair quantities from tables that
tests/sdf_witness.py fills (d^2 and solid angle of every point against every face), so a walk's minimum is made of the very numbers
sdf_witness.mesh_sdf takes its minimum of; they run in the dtype of the points (float64, or float32 to restate the kernel's own
decisions: the far test and the dipole term are written in the kernel's operation order)."""
import numpy as np

import sdf_witness as sw

LEAF = 4
SLACK = 1e-4  # the distance walk's pruning slack (csrc/sdf_pair.hpp derives it)


# ---- meshes beyond sdf_witness's two -----------------------------------------------------------------------------------------
def open_box():
    """the box without its lid (the two triangles of the +z side): an open mesh"""
    v, f = sw.box()
    return v, f[[k for k in range(12) if k not in (2, 3)]]


def with_degenerates(v, f):
    """the mesh plus faces that add no area and no volume, some in front of and some behind the mesh's own: a face with a
    repeated corner, a face that is one point, and copies of two existing faces each with its reversed twin (such a pair cancels
    in the winding number, and a copy ties with its original in the distance)"""
    head = [[f[0][0], f[0][0], f[0][1]], list(f[7]), list(f[7][::-1])]
    tail = [[f[1][0], f[1][0], f[1][0]], list(f[2]), list(f[2][::-1])]
    return v, np.concatenate([np.asarray(head, np.int64), f, np.asarray(tail, np.int64)])


def shell_of(F, seed=0):
    """exactly F triangles: closed icospheres of different radii and centres, then triangles of a further one, then faces without
    area — a tree's padding and ragged last leaf at any F"""
    rng = np.random.default_rng(seed)
    tris = []
    while len(tris) < F:
        v, f = sw.icosphere(1 if F - len(tris) >= 80 else 0, rng.uniform(0.2, 0.5))
        t = (v + rng.uniform(-0.4, 0.4, 3))[f]
        tris += list(t[:F - len(tris)])
    tris = np.asarray(tris)
    if F >= 3:
        tris[-1, 2] = tris[-1, 1]  # one face without area at the very end
    return tris


def cases():
    """name -> (triangles [F, 3, 3] float64 of fp32-exact values, closed: winding numbers are 0 or 1 off the surface)"""
    out = {}
    for level, name in ((0, "icosphere 20"), (2, "icosphere 320"), (3, "icosphere 1280")):
        v, f = sw.icosphere(level, 0.8)
        out[name] = (v[f], True)
    v, f = sw.box()
    out["box 12"] = (v[f], True)
    v, f = with_degenerates(*sw.icosphere(1, 0.7))
    out["degenerate 86"] = (v[f], True)
    v, f = open_box()
    out["open box 10"] = (v[f], False)
    for F in (1, 3, 4, 5, 255, 257, 515):
        out[f"shells {F}"] = (shell_of(F, seed=F), False)
    return {k: (t.astype(np.float32).astype(np.float64), closed) for k, (t, closed) in out.items()}


def query_points(triangles, n_near, n_uniform, seed=0, noise=0.01):
    """float32 points: n_near on faces drawn by area plus normal noise, then n_uniform in [-1, 1)^3"""
    rng = np.random.default_rng(seed)
    t = np.asarray(triangles, np.float64)
    area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    pick = rng.choice(len(t), n_near, p=area / area.sum()) if area.sum() > 0 else rng.integers(0, len(t), n_near)
    s, u = np.sqrt(rng.random(n_near))[:, None], rng.random(n_near)[:, None]
    near = (1 - s) * t[pick, 0] + s * (1 - u) * t[pick, 1] + s * u * t[pick, 2] + noise * rng.standard_normal((n_near, 3))
    return np.concatenate([near, rng.random((n_uniform, 3)) * 2 - 1]).astype(np.float32)


def surface_points(triangles, limit=64):
    """float32 points placed on the mesh by construction: vertices (exact), edge midpoints and centroids of the first faces"""
    t = np.asarray(triangles, np.float32)[:limit]
    mids = (t + np.roll(t, 1, axis=1)) * np.float32(0.5)
    return np.concatenate([t.reshape(-1, 3), mids.reshape(-1, 3), t.mean(axis=1, dtype=np.float32)])


# ---- the tree ----------------------------------------------------------------------------------------------------------------
def morton30(c, lo, hi):
    code = 0
    for axis in range(3):
        ext = hi[axis] - lo[axis]
        q = int(min(max(np.floor((c[axis] - lo[axis]) / (ext if ext > 0 else 1.0) * 1024.0), 0), 1023))
        for bit in range(10):
            code |= ((q >> bit) & 1) << (3 * bit + axis)
    return code


def leaves_for(F, leaf=LEAF):
    L = 1
    while L * leaf < F:
        L *= 2
    return L


def node_range(i, F, L, leaf=LEAF):
    d = int(np.floor(np.log2(i + 1)))
    span = (L >> d) * leaf
    k = i + 1 - (1 << d)
    return min(k * span, F), min((k + 1) * span, F)


def build(triangles, leaf=LEAF):
    """-> dict(perm [F], L, nodes float64 [2L-1, 16] in the header's layout but unrounded, radius about the unrounded centroid)"""
    t = np.asarray(triangles, np.float32).astype(np.float64)
    F = len(t)
    flat = t.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    codes = [morton30(t[f].mean(0), lo, hi) for f in range(F)]
    perm = np.asarray(sorted(range(F), key=lambda f: (codes[f], f)), np.int64)
    L = leaves_for(F, leaf)
    nodes = np.zeros((2 * L - 1, 16))
    for i in range(2 * L - 1):
        a, b = node_range(i, F, L, leaf)
        if a == b:
            nodes[i, 0:3], nodes[i, 4:7], nodes[i, 11] = np.inf, -np.inf, -1.0
            continue
        tt = t[perm[a:b]]
        vv = tt.reshape(-1, 3)
        nvec = 0.5 * np.cross(tt[:, 1] - tt[:, 0], tt[:, 2] - tt[:, 0])
        area = np.linalg.norm(nvec, axis=1)
        c = (area[:, None] * tt.mean(1)).sum(0) / area.sum() if area.sum() > 0 else vv.mean(0)
        nodes[i, 0:3], nodes[i, 4:7], nodes[i, 8:11] = vv.min(0), vv.max(0), c
        nodes[i, 11] = np.linalg.norm(vv - c, axis=1).max()
        nodes[i, 12:15] = nvec.sum(0)
    return {"perm": perm, "L": L, "F": F, "leaf": leaf, "nodes": nodes}


# ---- the walks ---------------------------------------------------------------------------------------------------------------
def pair_tables(points, triangles):
    """(D2 [N, F], Omega [N, F]) by sdf_witness's own functions, in points' dtype, faces in their ORIGINAL order"""
    p = np.asarray(points)
    D2 = np.stack([sw.point_triangle(p, tri, want_region=False)[0] for tri in triangles], axis=1)
    Om = np.stack([sw.solid_angle(p, tri) for tri in triangles], axis=1)
    return D2, Om


def _trailing_ones(v):
    k, m = np.zeros_like(v), v.copy()
    while True:
        sel = (m & 1) == 1
        if not sel.any():
            return k
        k[sel] += 1
        m[sel] >>= 1


def _box_d2(nodes, j, p):
    nd = nodes[j - 1]
    q = np.maximum(np.maximum(nd[:, 0:3] - p, 0), p - nd[:, 4:7])
    return q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]


def walk_nearest(points, nodes, perm, F, L, D2, leaf=LEAF, slack=SLACK):
    """-> (best d^2 [N], nearest original face [N], visited faces per point [N]); asserts that no walk reaches the cap"""
    p = np.asarray(points)
    ft = p.dtype.type
    nodes = np.asarray(nodes).astype(p.dtype)
    N = len(p)
    best, face = np.full(N, np.inf, p.dtype), np.full(N, np.iinfo(np.int64).max, np.int64)
    j, trail, visited = np.ones(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    active, steps, cap = np.ones(N, bool), 0, 2 * (2 * L - 1)
    while active.any():
        assert steps < cap, "the distance walk reached its iteration cap"
        steps += 1
        idx = np.nonzero(active)[0]
        jj, pp = j[idx], p[idx]
        reach = np.sqrt(best[idx]) + ft(slack)
        with np.errstate(invalid="ignore", over="ignore"):
            visit = ~(_box_d2(nodes, jj, pp) > reach * reach)
        inner = visit & (jj < L)
        for k in range(leaf):
            f = (jj - L) * leaf + k
            ok = visit & (jj >= L) & (f < F)
            rows, orig = idx[ok], perm[np.where(ok, f, 0)][ok]
            d2 = D2[rows, orig]
            better = (d2 < best[rows]) | ((d2 == best[rows]) & (orig < face[rows]))
            best[rows[better]], face[rows[better]] = d2[better], orig[better]
            visited[rows] += 1
        if inner.any():
            ji, pi = jj[inner], pp[inner]
            right_first = (_box_d2(nodes, 2 * ji + 1, pi) < _box_d2(nodes, 2 * ji, pi)).astype(np.int64)
            j[idx[inner]], trail[idx[inner]] = 2 * ji + right_first, trail[idx[inner]] * 2 + right_first
        out = idx[~inner]
        up = _trailing_ones(j[out] ^ trail[out])
        j[out], trail[out] = j[out] >> up, trail[out] >> up
        done = j[out] == 0
        active[out[done]] = False
        j[out[~done]] ^= 1
    return best, face, visited


def walk_winding(points, nodes, perm, F, L, Om, beta=3.0, leaf=LEAF):
    """-> (w [N], nodes and faces tested per point [N]); the far test and the dipole term in the kernel's operation order"""
    p = np.asarray(points)
    ft = p.dtype.type
    nodes = np.asarray(nodes).astype(p.dtype)
    N = len(p)
    omega, j, tests = np.zeros(N, p.dtype), np.ones(N, np.int64), np.zeros(N, np.int64)
    active, steps, cap = np.ones(N, bool), 0, 2 * (2 * L - 1)
    while active.any():
        assert steps < cap, "the winding walk reached its iteration cap"
        steps += 1
        idx = np.nonzero(active)[0]
        jj, nd = j[idx], nodes[j[idx] - 1]
        tests[idx] += 1
        d = nd[:, 8:11] - p[idx]
        dist2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        br = ft(beta) * nd[:, 11]
        full = nd[:, 11] >= 0
        far = full & (dist2 > br * br)
        with np.errstate(invalid="ignore", divide="ignore"):
            dipole = (nd[:, 12] * d[:, 0] + nd[:, 13] * d[:, 1] + nd[:, 14] * d[:, 2]) / (dist2 * np.sqrt(dist2))
        omega[idx[far]] += dipole[far]
        inner = full & ~far & (jj < L)
        near_leaf = full & ~far & (jj >= L)
        for k in range(leaf):
            f = (jj - L) * leaf + k
            ok = near_leaf & (f < F)
            rows = idx[ok]
            omega[rows] += Om[rows, perm[np.where(ok, f, 0)][ok]]
            tests[rows] += 1
        j[idx[inner]] = 2 * jj[inner]
        out = idx[~inner]
        nxt = j[out] + 1
        nxt = nxt >> (_trailing_ones(~nxt & (2 ** 40 - 1)))  # (strip the trailing zeros of j + 1)
        j[out] = nxt
        active[out[nxt == 1]] = False
    return omega * ft(1 / (4 * np.pi)), tests
