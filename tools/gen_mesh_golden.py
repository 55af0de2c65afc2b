#!/usr/bin/env python3
"""Generate tests/golden/mesh_fields.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the reference's `extract_fields` (nerf/utils.py:175-190) by EXECUTING it: an analytic query on a resolution-20
lattice in chunks of S = 8 (the last chunk of every axis is partial: 8 + 8 + 4) over bounds that are not symmetric.  The
query uses +, - and * on fp32 only, one rounding per operation, so the CPU and the GPU give the same bits.  Stored: the
call's inputs, the points of the last (partial) chunk as the query saw them, and u.

    python tools/gen_mesh_golden.py     (re-running reproduces the file bit for bit)
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "mesh_fields.npz")

BOUND_MIN, BOUND_MAX, RESOLUTION, S = (-1.0, -0.5, 0.25), (0.75, 1.5, 2.0), 20, 8


def golden_query(pts):
    """an fp32 polynomial of the point, exact on every device: ((x x + 0.5 y y) - z x) + 0.25 y"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return ((x * x + (y * y) * 0.5) - z * x) + y * 0.25


def main():
    sys.path.insert(0, REPO)
    import importlib
    from oracle.gen_golden import _assert_reference, _install_reference_stack, _stub_training_imports
    _install_reference_stack()
    _stub_training_imports()
    utils = importlib.import_module("nerf.utils")
    _assert_reference(utils)
    seen = []

    def query(pts):
        seen.append(pts.clone())
        return golden_query(pts)

    bmin, bmax = torch.tensor(BOUND_MIN), torch.tensor(BOUND_MAX)
    u = utils.extract_fields(bmin, bmax, RESOLUTION, query, S=S)
    out = dict(bound_min=bmin.numpy(), bound_max=bmax.numpy(), resolution=np.int64(RESOLUTION), S=np.int64(S),
               n_chunks=np.int64(len(seen)), pts_last=seen[-1].numpy(), u=np.asarray(u, dtype=np.float32))
    buf = io.BytesIO()  # fixed zip timestamps: a re-run writes the same bytes
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, b.getvalue())
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("mesh_fields: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
