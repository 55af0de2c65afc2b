#!/usr/bin/env python3
"""Generate tests/golden/error_map.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the reference's error-map importance sampling by EXECUTING it on the CPU oracle:

  (a) `get_rays(poses, intrinsics, 800, 800, N=4096, error_map)` (nerf/utils.py:92-114) with a seeded non-uniform map, B = 1,
      under torch.manual_seed: inds_coarse, inds, rays_o, rays_d;
  (b) the same at B = 2, 600 x 800 (not square: an x / y swap shows);
  (c) one reference `Trainer.train_step` (nerf/utils.py:436-537) with `error_map` set, on oracle.gen_golden's `train` scene
      (same network settings, seeded parameters, density grid and jitter seed), its 512 rays drawn by (a)'s sampler: the map
      entries the step touched after the update, and a checksum of the rest;
  (d) the same step with Seal `depths` (the depth term broadcast to every ray).

    python tools/gen_error_map_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import (TRAIN_NET, _assert_reference, _install_reference_stack, _load_synthetic,  # noqa: E402
                               _seed_params, _seeded, _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "error_map.npz")


def _map(B, seed):
    """a non-uniform map: smooth bumps plus noise, a dead (zero) band"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, 128, 128, generator=g) * 0.2
    yy, xx = torch.meshgrid(torch.arange(128.0), torch.arange(128.0), indexing="ij")
    for b in range(B):
        cx, cy = torch.rand(2, generator=g) * 128
        m[b] += torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 300.0)
    m[:, 60:64, :] = 0.0
    return m.reshape(B, -1).contiguous()


def main():
    _install_reference_stack()
    _stub_training_imports()
    utils = importlib.import_module("nerf.utils")
    network = importlib.import_module("nerf.network")
    strainer = importlib.import_module("SealNeRF.trainer")
    for m_ in (utils, network, strainer):
        _assert_reference(m_)
    syn = _load_synthetic()
    out = {}
    # (a), (b) get_rays with an error map
    for tag, B, H, W, N, seed in (("a", 1, 800, 800, 4096, 21), ("b", 2, 600, 800, 4096, 22)):
        poses = syn.orbit_poses(B, seed=seed)
        intr = syn.lego_intrinsics(H, W)
        emap = _map(B, seed + 100)
        torch.manual_seed(seed + 200)
        r = utils.get_rays(poses, intr, H, W, N, emap)
        out.update({f"{tag}_poses": poses.numpy(), f"{tag}_intrinsics": np.asarray(intr), f"{tag}_hw": np.array([H, W, N]),
                    f"{tag}_map": emap.numpy(), f"{tag}_seed": np.int64(seed + 200),
                    f"{tag}_inds_coarse": r["inds_coarse"].numpy(), f"{tag}_inds": r["inds"].numpy(),
                    f"{tag}_rays_o": r["rays_o"].numpy(), f"{tag}_rays_d": r["rays_d"].numpy()})
    # (c), (d) one executed train step with the map, plain and with Seal depths
    poses = syn.orbit_poses(2, seed=0)
    emap0 = _map(2, 300)
    torch.manual_seed(41)
    r = utils.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, 512, emap0[[0]])
    ro, rd, inds_coarse = r["rays_o"].contiguous(), r["rays_d"].contiguous(), r["inds_coarse"]
    images = _seeded((1, 512, 3), 42)
    depths = _seeded((1, 512), 43, 1.0, 4.0)
    out.update(ts_rays_o=ro.numpy(), ts_rays_d=rd.numpy(), ts_images=images.numpy(), ts_depths=depths.numpy(),
               ts_inds_coarse=inds_coarse.numpy(), ts_map=emap0.numpy(), ts_mean_count=np.int64(32768))
    for tag, extra in (("ts_plain", {}), ("ts_depth", {"depths": depths})):
        torch.manual_seed(3)
        net = network.NeRFNetwork(**TRAIN_NET)
        _seed_params(net)
        dens, bits = syn.lego_like_density_grid(seed=0)
        net.density_grid.copy_(torch.from_numpy(dens))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.mean_count = 32768
        emap = emap0.clone()
        opt = types.SimpleNamespace(color_space="srgb", patch_size=1, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
        me = types.SimpleNamespace(model=net, opt=opt, _backbone=strainer.BackBoneTypes.NGP,
                                   criterion=torch.nn.MSELoss(reduction="none"), criterion_depth=torch.nn.L1Loss(), error_map=emap)
        net.train()
        torch.manual_seed(5)
        _, _, loss = utils.Trainer.train_step(me, dict({"rays_o": ro, "rays_d": rd, "images": images.clone(), "index": [0],
                                                        "inds_coarse": inds_coarse}, **extra))
        touched = np.zeros(emap.shape, dtype=bool)
        touched[0, inds_coarse[0].numpy()] = True
        after = emap.numpy()
        rest = np.where(touched, 0.0, after.astype(np.float64))
        out.update({f"{tag}_loss": np.float64(loss.item()), f"{tag}_touched": after[0, inds_coarse[0].numpy()],
                    f"{tag}_rest_sum": np.float64(rest.sum()), f"{tag}_rest_sumsq": np.float64((rest ** 2).sum())})
    # fixed zip timestamps: a re-run writes the same bytes
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, b.getvalue())
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("error_map: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
