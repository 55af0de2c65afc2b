"""The mesh BVH of the SDF dataset's distance query (include/seal3d_hip.h "SDF: BVH query"): built once per mesh on the host, in
numpy, and walked on the device by s3d_mesh_sdf_bvh.  Faces sorted by the Morton code of their centroid, an implicit balanced tree
in heap order over leaves of LEAF faces; a node's bounds, centroid, radius and summed area normal come from the fp32 vertices the
kernel reads, in float64, rounded as the header states.  MeshBVH is the only producer of these arrays and checks them before it
uploads them: the kernel finds nodes and face ranges by arithmetic and trusts nothing but the sizes."""
import numpy as np
import torch

import s3d_hip

MAX_FACES = 1 << 26  # (at most 2^24 leaves: depth 24, within the walk's 32-bit trail)


def _spread10(q):
    """bits 0..9 of q to positions 0, 3, .., 27"""
    q = q.astype(np.uint32) & np.uint32(0x3FF)
    q = (q | (q << np.uint32(16))) & np.uint32(0x030000FF)
    q = (q | (q << np.uint32(8))) & np.uint32(0x0300F00F)
    q = (q | (q << np.uint32(4))) & np.uint32(0x030C30C3)
    q = (q | (q << np.uint32(2))) & np.uint32(0x09249249)
    return q


def morton30(centroids, lo, hi):
    """30-bit Morton code of points within the box [lo, hi]: 10 bits per axis, x in the lowest position"""
    ext = np.where(hi > lo, hi - lo, 1.0)
    q = np.clip(np.floor((centroids - lo) / ext * 1024.0), 0, 1023).astype(np.uint32)
    return _spread10(q[:, 0]) | (_spread10(q[:, 1]) << np.uint32(1)) | (_spread10(q[:, 2]) << np.uint32(2))


def _round_up32(x64):
    """the smallest fp32 that is not below x64"""
    x32 = x64.astype(np.float32)
    low = x32.astype(np.float64) < x64
    return np.where(low, np.nextafter(x32, np.float32(np.inf)), x32).astype(np.float32)


class MeshBVH:
    """triangles [F, 3, 3] (numpy or torch; taken as fp32, the kernel's view of the mesh) ->
    perm [F] int32 (sorted face k is original face perm[k]), triangles_sorted [F, 3, 3] fp32, nodes [2L - 1, 16] fp32, F, L, depth"""

    def __init__(self, triangles):
        tri = triangles.detach().cpu().numpy() if torch.is_tensor(triangles) else np.asarray(triangles)
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)
        F = tri.shape[0]
        if F == 0:
            raise ValueError("MeshBVH: the mesh has no faces")
        if F > MAX_FACES:
            raise ValueError(f"MeshBVH: at most 2^26 faces, got {F}")
        self.leaf = s3d_hip.SdfBackend.bvh_leaf()
        t64 = tri.astype(np.float64)
        flat = t64.reshape(-1, 3)
        code = morton30(t64.mean(axis=1), flat.min(axis=0), flat.max(axis=0))
        perm = np.argsort(code, kind="stable")
        L = 1
        while L * self.leaf < F:
            L *= 2
        self.F, self.L, self.depth = F, L, L.bit_length() - 1
        self.perm = perm.astype(np.int32)
        self.triangles_sorted = np.ascontiguousarray(tri[perm])
        self.nodes = self._nodes(t64[perm])
        self.check()
        self._device = {}

    def _nodes(self, ts):
        """ts: the sorted faces [F, 3, 3] in float64 -> nodes [2L - 1, 16] fp32, level by level over the padded face slots"""
        F, L, P = self.F, self.L, self.L * self.leaf
        A, B, C = ts[:, 0], ts[:, 1], ts[:, 2]
        nvec = 0.5 * np.cross(B - A, C - A)
        area = np.sqrt((nvec * nvec).sum(axis=1))

        def padded(x, fill):
            out = np.full((P,) + x.shape[1:], fill, np.float64)
            out[:F] = x
            return out
        vmin, vmax = padded(ts.min(axis=1), np.inf), padded(ts.max(axis=1), -np.inf)
        s_n, s_a, s_ac = padded(nvec, 0.0), padded(area, 0.0), padded(area[:, None] * ts.mean(axis=1), 0.0)
        s_v, count = padded(ts.sum(axis=1), 0.0), padded(np.ones(F), 0.0)
        verts = padded(ts, 0.0)
        nodes = np.zeros((2 * L - 1, 16), np.float32)
        for d in range(self.depth + 1):
            n, span = 1 << d, P >> d
            cnt = count.reshape(n, span).sum(axis=1)
            full = cnt > 0
            a = s_a.reshape(n, span).sum(axis=1)
            c = np.where((a > 0)[:, None], s_ac.reshape(n, span, 3).sum(axis=1) / np.where(a > 0, a, 1.0)[:, None],
                         s_v.reshape(n, span, 3).sum(axis=1) / np.where(full, 3.0 * cnt, 1.0)[:, None])
            c32 = np.where(full[:, None], c, 0.0).astype(np.float32)
            # the radius about the centroid as stored
            dv = verts.reshape(n, span, 3, 3) - c32.astype(np.float64)[:, None, None, :]
            dist = np.sqrt((dv * dv).sum(axis=-1)).max(axis=-1)  # [n, span]
            dist = np.where(count.reshape(n, span) > 0, dist, -np.inf).max(axis=1)
            rec = nodes[n - 1:2 * n - 1]
            rec[:, 0:3] = np.nextafter(vmin.reshape(n, span, 3).min(axis=1).astype(np.float32), np.float32(-np.inf))
            rec[:, 4:7] = np.nextafter(vmax.reshape(n, span, 3).max(axis=1).astype(np.float32), np.float32(np.inf))
            rec[:, 8:11] = c32
            rec[:, 11] = np.where(full, _round_up32(np.where(full, dist, 0.0)), np.float32(-1.0))
            rec[:, 12:15] = s_n.reshape(n, span, 3).sum(axis=1).astype(np.float32)
            rec[~full, 0:3], rec[~full, 4:7] = np.inf, -np.inf
        return nodes

    def node_range(self, i):
        """the sorted faces [first, last) that node i (heap order, from 0) covers"""
        d = (i + 1).bit_length() - 1
        span = (self.L >> d) * self.leaf
        k = i + 1 - (1 << d)
        return min(k * span, self.F), min((k + 1) * span, self.F)

    def check(self):
        F, L = self.F, self.L
        assert 0 < F <= MAX_FACES and L >= 1 and L & (L - 1) == 0 and L * self.leaf >= F and (L == 1 or (L // 2) * self.leaf < F)
        assert self.perm.shape == (F,) and self.perm.dtype == np.int32
        assert np.array_equal(np.sort(self.perm), np.arange(F, dtype=np.int32)), "perm is not a permutation"
        assert self.triangles_sorted.shape == (F, 3, 3) and self.triangles_sorted.dtype == np.float32
        assert self.nodes.shape == (2 * L - 1, 16) and self.nodes.dtype == np.float32 and not np.isnan(self.nodes).any()
        empty = self.nodes[:, 11] < 0
        assert not empty[0] and self.node_range(0) == (0, F)
        assert int((~empty[L - 1:]).sum()) == -(-F // self.leaf), "the leaves that hold faces are the first ceil(F / LEAF)"
        assert np.isposinf(self.nodes[empty, 0:3]).all() and np.isneginf(self.nodes[empty, 4:7]).all()
        assert (self.nodes[empty, 12:15] == 0).all() and np.isfinite(self.nodes[~empty]).all()

    def device_arrays(self, device):
        """(nodes [2L-1, 16], staged [F, 20], perm [F] int32) on `device`, uploaded and staged at the first call"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self.check()
            tri = torch.from_numpy(self.triangles_sorted).to(device)
            self._device[device] = (torch.from_numpy(self.nodes).to(device), s3d_hip.SdfBackend.bvh_stage(tri),
                                    torch.from_numpy(self.perm).to(device))
        return self._device[device]
