"""Plain numpy marching cubes: the CPU yardstick of the mesh export (a support module, not a test).

It follows the contract of DESIGN.md §8 (mesh export) statement by statement, in fp32, with the tables of
tools/gen_mc_tables.py:
  * the field is read with NaN as 0 and +-inf as +-FLT_MAX; a grid point is solid iff u > iso;
  * grid point p owns its +x, +y, +z edges; a crossing edge (exactly one solid end) gives one vertex at lo + t along the
    axis, t = (iso - f_lo) / (f_hi - f_lo), lo the owning point; t is kept inside [0, 1] (a no-op unless iso - f_lo overflows);
  * vertices are ordered by the owner's linear index (x ny + y) nz + z, then x-, y-, z-edge;
  * world = v / (n_axis - 1) * (bmax - bmin) + bmin per axis;
  * triangles are ordered by cell linear index over the (nx-1)(ny-1)(nz-1) cells, table order inside a cell.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from tools import gen_mc_tables as mct  # noqa: E402

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def sanitise(u):
    f = np.array(u, dtype=np.float32, copy=True)
    f[np.isnan(f)] = 0.0
    f[f == np.inf] = FLT_MAX
    f[f == -np.inf] = -FLT_MAX
    return f


def cell_cases(u, iso):
    """case index of every cell, [nx-1, ny-1, nz-1]"""
    solid = sanitise(u) > F32(iso)
    nx, ny, nz = solid.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = mct.corner_xyz(c)
        case |= solid[dx:dx + nx - 1, dy:dy + ny - 1, dz:dz + nz - 1].astype(np.int64) << c
    return case


def marching_cubes(u, iso, bounds=None):
    """-> (vertices [V,3] float32 in world coordinates, triangles [T,3] int32); bounds = (min xyz, max xyz), default [0, n-1]"""
    u = np.asarray(u, dtype=np.float32)
    nx, ny, nz = u.shape
    assert min(u.shape) >= 2
    n = np.array([nx, ny, nz])
    if bounds is None:
        bounds = np.concatenate([np.zeros(3), n - 1.0])
    bounds = np.asarray(bounds, dtype=np.float32).reshape(6)
    bmin, bmax = bounds[:3], bounds[3:]
    iso = F32(iso)
    f = sanitise(u)
    solid = f > iso
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = solid[:-1] != solid[1:]
    cross[:, :-1, :, 1] = solid[:, :-1] != solid[:, 1:]
    cross[:, :, :-1, 2] = solid[:, :, :-1] != solid[:, :, 1:]
    flat = cross.reshape(-1)  # index = 3 * linear point index + axis: the vertex order
    vid = np.cumsum(flat) - flat  # exclusive prefix = the vertex id of a crossing edge
    hit = np.flatnonzero(flat)
    lin, ax = hit // 3, hit % 3
    p = np.stack(np.unravel_index(lin, (nx, ny, nz)), axis=1)
    q = p.copy()
    q[np.arange(len(hit)), ax] += 1
    f_lo, f_hi = f[p[:, 0], p[:, 1], p[:, 2]], f[q[:, 0], q[:, 1], q[:, 2]]
    with np.errstate(all="ignore"):
        t = ((iso - f_lo) / (f_hi - f_lo)).astype(np.float32)
    t = np.fmin(np.fmax(t, F32(0)), F32(1))
    v = p.astype(np.float32)
    v[np.arange(len(hit)), ax] = v[np.arange(len(hit)), ax] + t
    with np.errstate(all="ignore"):
        world = (v / (n - 1).astype(np.float32)[None] * (bmax - bmin)[None] + bmin[None]).astype(np.float32)

    case = cell_cases(u, iso).reshape(-1)
    count = np.asarray(mct.TRI_COUNT)[case]
    cells = np.flatnonzero(count)
    cp = np.stack(np.unravel_index(cells, (nx - 1, ny - 1, nz - 1)), axis=1)
    table = np.asarray(mct.TRI_TABLE)[case[cells]]  # [cells, 3 width]
    owner = np.asarray([mct.corner_xyz(c) for c in mct.EDGE_OWNER])
    axis = np.asarray(mct.EDGE_AXIS)
    e = np.where(table >= 0, table, 0)
    op = cp[:, None, :] + owner[e]  # [cells, 3 width, 3]
    ids = vid[3 * ((op[..., 0] * ny + op[..., 1]) * nz + op[..., 2]) + axis[e]]
    assert flat[3 * ((op[..., 0] * ny + op[..., 1]) * nz + op[..., 2]) + axis[e]][table >= 0].all()
    tris = ids[table >= 0].reshape(-1, 3).astype(np.int32)
    return world.reshape(-1, 3), tris


# ------------------------------------------------------------------------------------------------ mesh checks
def edge_use(tris):
    """directed edges of a triangle list -> (undirected edge keys [E], uses forward [E], uses backward [E])"""
    t = np.asarray(tris, dtype=np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * (int(t.max()) + 1 if len(t) else 1) + hi
    uniq, inv = np.unique(key, return_inverse=True)
    fwd = np.bincount(inv, weights=(a < b), minlength=len(uniq)).astype(np.int64)
    bwd = np.bincount(inv, weights=(a > b), minlength=len(uniq)).astype(np.int64)
    first = np.zeros(len(uniq), dtype=np.int64)
    first[inv] = np.arange(len(key))
    return np.stack([lo[first], hi[first]], axis=1), fwd, bwd


def is_closed(tris):
    """every edge in exactly two triangles that traverse it in opposite directions"""
    _, fwd, bwd = edge_use(tris)
    return bool(np.all(fwd == 1) and np.all(bwd == 1))


def euler(verts, tris):
    e, _, _ = edge_use(tris)
    return len(verts) - len(e) + len(tris)


def signed_volume(verts, tris):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
