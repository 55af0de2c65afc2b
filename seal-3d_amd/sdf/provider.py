"""SDF dataset (sdf/provider.py of the reference) with the sampling and the distance query on the device: an item is two launches,
s3d_sdf_sample_points (surface | perturbed surface | uniform rows) and s3d_mesh_sdf — or, from BVH_AUTO_MIN_FACES faces on,
s3d_mesh_sdf_bvh over a tree built once (sdf/bvh.py) — over the rows that are not on the surface.
The reference draws with trimesh and queries pysdf on the CPU; here the mesh is loaded, normalised, checked and oriented once on
the host, and an item is a pure function of (seed, item number)."""
import os
import warnings

import numpy as np
import torch

import s3d_hip
from nerf.mesh import read_ply
from sdf.bvh import MeshBVH

# accel="auto" takes the BVH from this many faces on: the smallest size of the sweep in profiles/sdf_bvh.md (N = 2^17 points, UV
# spheres and tori of 1,280 faces and upwards in steps of 4x) at which the BVH's median was below brute force's in the same run,
# on both meshes and both point sets (3.1 against 4.4 ms on the sphere; at 1,280 faces 1.5 against 1.1 ms)
BVH_AUTO_MIN_FACES = 5120


def read_obj(path_or_lines):
    """-> (vertices [V, 3] float64, faces [T, 3] int64) of a Wavefront .obj: `v x y z` and `f` lines only; an index may be `a`,
    `a/b`, `a//c` or `a/b/c` (the first number counts), negative indices count back from the vertices read so far, polygons
    are fan-triangulated around their first corner"""
    lines = open(path_or_lines).read().splitlines() if isinstance(path_or_lines, (str, os.PathLike)) else list(path_or_lines)
    vertices, faces = [], []
    for line in lines:
        w = line.split("#", 1)[0].split()
        if not w:
            continue
        if w[0] == "v":
            vertices.append([float(c) for c in w[1:4]])
        elif w[0] == "f":
            idx = []
            for corner in w[1:]:
                i = int(corner.split("/")[0])
                if i == 0 or abs(i) > len(vertices):
                    raise ValueError(f"obj: face index {i} out of range ({len(vertices)} vertices so far)")
                idx.append(i - 1 if i > 0 else len(vertices) + i)
            if len(idx) < 3:
                raise ValueError(f"obj: a face needs three corners, got `{line.strip()}`")
            faces += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    return np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)


def load_mesh(path_or_mesh):
    if isinstance(path_or_mesh, (tuple, list)) and len(path_or_mesh) == 2:
        v, f = path_or_mesh
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else v
        f = f.detach().cpu().numpy() if torch.is_tensor(f) else f
        return np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    ext = os.path.splitext(str(path_or_mesh))[1].lower()
    if ext == ".ply":
        v, f = read_ply(path_or_mesh)
        return np.asarray(v, np.float64), np.asarray(f, np.int64)
    if ext == ".obj":
        return read_obj(path_or_mesh)
    raise NotImplementedError(f"SDFDataset reads .ply and .obj meshes or a (vertices, faces) pair, not `{path_or_mesh}`")


def normalize_vertices(vertices):
    """sdf/provider.py:37-43: into [-1, 1] — the bounding box's centre to the origin, its diagonal to 2 * 0.95"""
    v = np.asarray(vertices, np.float64)
    vmin, vmax = v.min(0), v.max(0)
    return (v - ((vmin + vmax) / 2)[None, :]) * (2 / np.sqrt(np.sum((vmax - vmin) ** 2)) * 0.95)


def is_watertight(faces):
    """every edge is shared by exactly two faces that run through it in opposite directions"""
    f = np.asarray(faces, np.int64)
    if f.size == 0:
        return False
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    directed = e[:, 0] * n + e[:, 1]
    uniq, counts = np.unique(directed, return_counts=True)
    if (counts != 1).any():
        return False
    return bool(np.isin(e[:, 1] * n + e[:, 0], uniq).all())


def signed_volume(vertices, faces):
    a, b, c = (np.asarray(vertices, np.float64)[np.asarray(faces)[:, k]] for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


class SDFDataset(torch.utils.data.Dataset):
    def __init__(self, path_or_mesh, size=100, num_samples=2 ** 18, clip_sdf=None, seed=0, device=None, noise_std=0.01,
                 accel="auto"):
        super().__init__()
        vertices, faces = load_mesh(path_or_mesh)
        if len(faces) == 0:
            raise ValueError("SDFDataset: the mesh has no faces")
        vertices = normalize_vertices(vertices)
        print(f"[INFO] mesh: {vertices.shape} {faces.shape}")
        self.watertight = is_watertight(faces)
        if not self.watertight:
            warnings.warn("[WARN] mesh is not watertight! SDF maybe incorrect.")
        # the winding number's sign rule takes outward-facing triangles
        self.flipped = signed_volume(vertices, faces) < 0
        if self.flipped:
            faces = faces[:, ::-1].copy()
        self.vertices, self.faces = vertices, faces
        assert num_samples % 8 == 0, "num_samples must be divisible by 8."
        self.num_samples, self.clip_sdf, self.size, self.seed, self.noise_std = num_samples, clip_sdf, size, int(seed), noise_std
        self.epoch = 0
        self.device = torch.device(device if device is not None else "cuda")
        tri = vertices[faces]  # [F, 3, 3]
        area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) / 2
        if not area.sum() > 0:
            raise ValueError("SDFDataset: the mesh has no area")
        cdf = (np.cumsum(area) / area.sum()).astype(np.float32)
        cdf[int(np.nonzero(area)[0][-1]):] = 1.0  # (the last face with an area closes the range, whatever the rounding)
        self.triangles = torch.from_numpy(tri.astype(np.float32)).contiguous().to(self.device)
        self.cdf = torch.from_numpy(cdf).to(self.device)
        # the distance query: brute force over all faces, or the BVH (the same distance bit for bit, the sign through a hierarchical
        # winding number with far-field terms); the tree is built here, once
        if accel not in ("brute", "bvh", "auto"):
            raise ValueError(f"SDFDataset: accel is 'brute', 'bvh' or 'auto', not `{accel}`")
        self.accel = accel if accel != "auto" else ("bvh" if len(faces) >= BVH_AUTO_MIN_FACES else "brute")
        self.bvh = MeshBVH(tri.astype(np.float32)) if self.accel == "bvh" else None

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        N = self.num_samples
        # (the reference draws afresh whenever an item is asked for: the trainer counts `epoch` up, so item i of another epoch differs)
        points = s3d_hip.SdfBackend.sample_points(self.triangles, self.cdf, N, self.seed, self.epoch * self.size + int(i), self.noise_std)
        sdfs = torch.zeros(N, 1, dtype=torch.float32, device=self.device)  # (rows [0, N / 2) lie on the surface)
        if self.bvh is not None:
            sdfs[N // 2:, 0] = s3d_hip.SdfBackend.mesh_sdf_bvh(points[N // 2:], self.bvh)
        else:
            sdfs[N // 2:, 0] = s3d_hip.SdfBackend.mesh_sdf(points[N // 2:], self.triangles)
        if self.clip_sdf is not None:
            sdfs = sdfs.clamp(-self.clip_sdf, self.clip_sdf)
        return {"sdfs": sdfs, "points": points}

    def dataloader(self, shuffle=True):
        """items with the reference's batch axis of 1 (its DataLoader(batch_size=1) on host arrays); the tensors stay on the device"""
        return torch.utils.data.DataLoader(self, batch_size=1, shuffle=shuffle, num_workers=0)
