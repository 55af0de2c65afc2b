"""Mesh export: density field -> iso-surface -> PLY (nerf/utils.py:175-205 and :583-603 of the reference).

The reference samples the field in chunks to the host, runs PyMCubes there and writes the file with trimesh.  Here the
volume stays on the query's device, the iso-surface comes from the HIP marching cubes (s3d_hip.MeshBackend, csrc/mesh.hip)
and the PLY reader / writer are a few lines of numpy.  The surface's definition — vertex = linear interpolation along a
crossing grid edge, world = v / (n - 1) * (max - min) + min — is the reference's; vertex and triangle ORDER are this
project's, fixed so that a mesh can be compared index for index.
"""
import os

import numpy as np
import torch


def extract_fields(bound_min, bound_max, resolution, query_func, S=128, device=None):
    """nerf/utils.py:175-190: the field on the resolution^3 lattice of [bound_min, bound_max], queried in S^3 chunks in
    meshgrid(indexing="ij") point order.  -> u [resolution]*3 float32, on the device query_func answers on.  The three
    axes are made on the host as in the reference (so the lattice has the reference's bits); `device`: the chunks' points
    are built there instead of on the host."""
    X, Y, Z = (torch.linspace(float(bound_min[k]), float(bound_max[k]), resolution).to(device).split(S) for k in range(3))
    u = None
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = query_func(pts).reshape(len(xs), len(ys), len(zs)).detach()
                    if u is None:
                        u = torch.zeros(resolution, resolution, resolution, dtype=torch.float32, device=val.device)
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, device=None):
    """nerf/utils.py:193-205 -> (vertices [V, 3] float32 in world coordinates, triangles [T, 3] int32), device tensors"""
    from s3d_hip import MeshBackend
    u = extract_fields(bound_min, bound_max, resolution, query_func, device=device)
    bounds = torch.cat([torch.as_tensor(bound_min).detach().float().reshape(3).cpu(),
                        torch.as_tensor(bound_max).detach().float().reshape(3).cpu()])
    return MeshBackend.marching_cubes(u, threshold, bounds)


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _need_ply(path):
    if os.path.splitext(str(path))[1].lower() != ".ply":
        raise NotImplementedError(f"mesh files are read and written as .ply only, not `{path}`")


def write_ply(path, vertices, triangles):
    """binary little-endian PLY: vertex float x y z, face list uchar int vertex_indices"""
    _need_ply(path)
    v = _host(vertices, "<f4").reshape(-1, 3)
    t = _host(triangles, "<i4").reshape(-1, 3)
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"], faces["i"] = 3, t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """-> (vertices [V, 3] float32, triangles [T, 3] int32) of an ASCII or binary PLY: float or double x / y / z (other
    vertex properties are skipped), faces as a list property of any count / index type, triangles only"""
    _need_ply(path)
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []  # elements: [name, count, [(property name, type) | (name, count type, item type)]]
    for line in data[:end].decode("ascii").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property":
            elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]) if w[1] == "list" else (w[2], _PLY_TYPES[w[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: unknown PLY format `{fmt}`")
    order = ">" if fmt == "binary_big_endian" else "<"
    tokens, pos = (iter(data[body:].split()) if fmt == "ascii" else None), body
    vertices, triangles = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for name, count, props in elements:
        lists = [p for p in props if len(p) == 3]
        if not lists:  # fixed-size rows
            dt = np.dtype([(p[0], order + p[1]) for p in props])
            if fmt == "ascii":
                rows = np.array([[float(next(tokens)) for _ in props] for _ in range(count)], dtype=np.float64).reshape(count, len(props))
                cols = {p[0]: rows[:, k] for k, p in enumerate(props)}
            else:
                rows = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                pos += dt.itemsize * count
                cols = {p[0]: rows[p[0]] for p in props}
            if name == "vertex":
                vertices = np.stack([cols["x"], cols["y"], cols["z"]], axis=1).astype(np.float32)
            continue
        if name == "face" and fmt != "ascii" and len(props) == 1:
            fast = _read_faces_fast(data, pos, count, order, props[0])
            if fast is not None:
                triangles = fast
                pos += (np.dtype(props[0][1]).itemsize + 3 * np.dtype(props[0][2]).itemsize) * count
                continue
        rows = []  # rows with a list: walked one by one
        for _ in range(count):
            row = None
            for p in props:
                if len(p) == 2:
                    if fmt == "ascii":
                        next(tokens)
                    else:
                        pos += np.dtype(p[1]).itemsize
                    continue
                if fmt == "ascii":
                    n = int(next(tokens))
                    items = [int(float(next(tokens))) for _ in range(n)]
                else:
                    n = int(np.frombuffer(data, dtype=order + p[1], count=1, offset=pos)[0])
                    pos += np.dtype(p[1]).itemsize
                    items = np.frombuffer(data, dtype=order + p[2], count=n, offset=pos).tolist()
                    pos += np.dtype(p[2]).itemsize * n
                if p[0] in ("vertex_indices", "vertex_index"):
                    row = items
            if name == "face":
                if row is None or len(row) != 3:
                    raise ValueError(f"{path}: faces must be triangles")
                rows.append(row)
        if name == "face":
            triangles = np.asarray(rows, dtype=np.int64).reshape(-1, 3).astype(np.int32)
    return vertices, triangles


def _read_faces_fast(data, pos, count, order, p):
    """binary faces that are all triangles with one list property: one structured read"""
    dt = np.dtype([("n", order + p[1]), ("i", order + p[2], (3,))])
    if pos + dt.itemsize * count > len(data):
        return None
    rows = np.frombuffer(data, dtype=dt, count=count, offset=pos)
    return rows["i"].astype(np.int32) if np.all(rows["n"] == 3) else None


def save_mesh(model, save_path, resolution=256, threshold=10, fp16=True):
    """nerf/utils.py:583-603 for any model with `density` and `aabb_infer` (a Seal teacher's density goes through its
    proxy, so its mesh shows the edit).  Nothing of the model is written: parameters, buffers and the binding's cached
    scratch only — a captured training step replays unchanged afterwards."""
    os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
    _need_ply(save_path)
    device = model.aabb_infer.device

    def query_func(pts):
        with torch.no_grad():
            with torch.autocast(device.type, dtype=torch.float16, enabled=fp16 and device.type == "cuda"):
                return model.density(pts.to(device))["sigma"]

    aabb = model.aabb_infer.detach().float().cpu()
    vertices, triangles = extract_geometry(aabb[:3], aabb[3:], resolution, threshold, query_func, device=device)
    write_ply(save_path, vertices, triangles)
    return vertices, triangles
