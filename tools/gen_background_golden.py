#!/usr/bin/env python3
"""Generate tests/golden/background.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the NGP background model of the reference (nerf/network.py:74-96 construction, :149-163 `background`, :208-210
`get_params`) by EXECUTING it on the CPU oracle:

  (a) `NeRFNetwork(bg_radius=32).background(sph, d)` forward and backward on seeded rays, `sph` from the reference's own
      `raymarching.sph_from_ray`; parameters seeded by name (oracle.gen_golden._seed_params), gradients recorded with
      oracle.gen_golden._grad_record (table: norm, sum and 2,048 seeded rows);
  (b) one reference `Trainer.train_step` (nerf/utils.py:436-537) with bg_radius = 32 on oracle.gen_golden's `train` scene (same
      network settings, seeded parameters, density grid, rays, targets and jitter seed): loss, prediction, sample counter and
      the gradient records of `encoder_bg.embeddings` and `bg_net.*` (+ the norms of every other gradient);
  (c) parameter names, shapes, `get_params` group sizes and per-parameter checksums right after `torch.manual_seed(s)`
      construction, which pin the registration order and the order of the RNG draws.

Tables are not stored.

    python tools/gen_background_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import (TRAIN_NET, _assert_reference, _grad_record, _install_reference_stack,  # noqa: E402
                               _load_synthetic, _seed_params, _seeded, _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "background.npz")
NET = dict(bound=1, cuda_ray=True, log2_hashmap_size=14, bg_radius=32)
INIT_SEED = 11
N_RAYS = 1024


def main():
    _install_reference_stack()
    _stub_training_imports()
    network = importlib.import_module("nerf.network")
    utils = importlib.import_module("nerf.utils")
    strainer = importlib.import_module("SealNeRF.trainer")
    raymarching = importlib.import_module("raymarching")
    for m_ in (network, utils, strainer):
        _assert_reference(m_)
    out = {}
    # (c) construction: names, shapes, checksums of the initial values
    torch.manual_seed(INIT_SEED)
    net = network.NeRFNetwork(**NET)
    names = [k for k, _ in net.named_parameters()]
    out["init_names"] = np.array(names)
    out["init_shapes"] = np.array([list(p.shape) + [0] * (2 - p.dim()) for _, p in net.named_parameters()], dtype=np.int64)
    out["init_sum"] = np.array([p.detach().double().sum().item() for _, p in net.named_parameters()])
    out["init_sumsq"] = np.array([(p.detach().double() ** 2).sum().item() for _, p in net.named_parameters()])
    out["init_seed"] = np.int64(INIT_SEED)
    out["get_params_sizes"] = np.array([sum(p.numel() for p in g["params"]) for g in net.get_params(1e-2)], dtype=np.int64)
    # (a) background forward + backward on seeded rays
    _seed_params(net)
    ro = _seeded((N_RAYS, 3), 71, -1.5, 1.5)
    rd = torch.nn.functional.normalize(_seeded((N_RAYS, 3), 72, -1, 1), dim=-1)
    sph = raymarching.sph_from_ray(ro, rd, NET["bg_radius"])
    grad = _seeded((N_RAYS, 3), 73, -1, 1)
    net.zero_grad()
    rgb = net.background(sph, rd)
    rgb.backward(grad)
    out.update(bg_rays_o=ro.numpy(), bg_rays_d=rd.numpy(), bg_sph=sph.numpy(), bg_grad_rgb=grad.numpy(), bg_rgb=rgb.detach().numpy())
    rec = {}
    _grad_record(net, "bg_grad", rec)
    out.update({k: v for k, v in rec.items() if "_bg" in k})
    # (b) one executed Trainer.train_step with the background model (gen_train's scene and seeds)
    import types
    syn = _load_synthetic()
    torch.manual_seed(3)
    net = network.NeRFNetwork(**dict(TRAIN_NET, bg_radius=NET["bg_radius"]))
    _seed_params(net)
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net.mean_count = 32768
    poses = syn.orbit_poses(2, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=512, generator=torch.Generator().manual_seed(41))
    ro, rd = r["rays_o"].contiguous(), r["rays_d"].contiguous()
    images = _seeded((1, 512, 3), 42)
    depths = _seeded((1, 512), 43, 1.0, 4.0)
    opt = types.SimpleNamespace(color_space="srgb", patch_size=1, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    me = types.SimpleNamespace(model=net, opt=opt, _backbone=strainer.BackBoneTypes.NGP, criterion=torch.nn.MSELoss(reduction="none"),
                               criterion_depth=torch.nn.L1Loss(), error_map=None)
    net.train()
    torch.manual_seed(5)
    pred, _, loss = utils.Trainer.train_step(me, {"rays_o": ro, "rays_d": rd, "images": images.clone(), "depths": depths})
    net.zero_grad()
    loss.backward()
    out.update(ts_rays_o=ro.numpy(), ts_rays_d=rd.numpy(), ts_images=images.numpy(), ts_depths=depths.numpy(),
               ts_loss=np.float64(loss.item()), ts_pred=pred.detach().numpy(), ts_counter=net.step_counter[0].numpy().copy(),
               ts_mean_count=np.int64(32768))
    rec = {}
    _grad_record(net, "ts_grad", rec)
    out.update({k: v for k, v in rec.items() if "_bg" in k or k.endswith("_norm")})
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
    print("background: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes; rgb mean", float(rgb.detach().mean()), "train loss", loss.item())


if __name__ == "__main__":
    main()
