#!/usr/bin/env python3
"""Generate tests/golden/tensorf_background.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the TensoRF background model of the reference (tensoRF/network.py:69-96 construction, :201-218 `background`, :331-333
`get_params`) by EXECUTING it on the CPU oracle:

  (a) `NeRFNetwork(bg_radius=32, bg_resolution=[20, 12]).background(sph, d)` forward and backward: 1,024 seeded rays with `sph`
      from the reference's own `raymarching.sph_from_ray`, then 16 rows whose coordinates are set by hand to +-1, 0 and +-1.05
      (the plane's border, its centre, and outside: zeros padding).  The plane is not square, so a swap of H and W shows.
      Parameters seeded by name (oracle.gen_golden._seed_params); the whole `bg_mat` gradient (1,920 values) and both weight
      gradients are stored;
  (b) one reference `Trainer.train_step` (tensoRF/utils.py:42-49) with bg_radius = 32 on oracle.gen_golden's `tensorf` scene
      (same network settings, seeded parameters, density grid, rays, targets and jitter seed): loss, prediction, sample counter,
      the gradients of `bg_mat` and `bg_net.*` and the norms of every other gradient;
  (c) parameter names, shapes, `get_params` group sizes and per-parameter checksums right after `torch.manual_seed(s)`
      construction, which pin the registration order and the order of the RNG draws.

    python tools/gen_tensorf_background_golden.py     (re-running reproduces the file bit for bit)
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
from oracle.gen_golden import (TENSORF_NET, _assert_reference, _grad_record_flat, _install_reference_stack,  # noqa: E402
                               _load_synthetic, _seed_params, _seeded, _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "tensorf_background.npz")
BG = dict(bg_radius=32, bg_resolution=[20, 12])
TS_BG = dict(bg_radius=32, bg_resolution=[32, 32])
INIT_SEED = 11
N_RAYS = 1024
# sphere coordinates set by hand: the border exactly, the centre, and just outside (one axis, both axes)
EDGE_SPH = [[-1, -1], [1, 1], [-1, 1], [1, -1], [0, 0], [1, 0], [0, -1], [1.05, 0], [0, -1.05], [1.05, 1.05], [-1.05, -1.05],
            [-1.05, 1], [1, 1.05], [1.05, -1.05], [0.5, 1], [-1, 0.25]]


def main():
    _install_reference_stack()
    _stub_training_imports()
    trf = importlib.import_module("tensoRF.network")
    tu = importlib.import_module("tensoRF.utils")
    strainer = importlib.import_module("SealNeRF.trainer")
    raymarching = importlib.import_module("raymarching")
    for m_ in (trf, tu, strainer):
        _assert_reference(m_)
    trf.NeRFNetwork._self = trf.NeRFNetwork
    out = {}
    # (c) construction: names, shapes, checksums of the initial values
    torch.manual_seed(INIT_SEED)
    net = trf.NeRFNetwork(**dict(TENSORF_NET, **BG))
    out["init_names"] = np.array([k for k, _ in net.named_parameters()])
    out["init_shapes"] = np.array([str(tuple(p.shape)) for _, p in net.named_parameters()])
    out["init_sum"] = np.array([p.detach().double().sum().item() for _, p in net.named_parameters()])
    out["init_sumsq"] = np.array([(p.detach().double() ** 2).sum().item() for _, p in net.named_parameters()])
    out["init_seed"] = np.int64(INIT_SEED)
    groups = net.get_params(2e-2, 1e-3)
    out["get_params_sizes"] = np.array([sum(p.numel() for p in g["params"]) for g in groups], dtype=np.int64)
    out["get_params_lrs"] = np.array([g["lr"] for g in groups])
    # (a) background forward + backward
    _seed_params(net)
    ro = _seeded((N_RAYS + len(EDGE_SPH), 3), 71, -1.5, 1.5)
    rd = torch.nn.functional.normalize(_seeded((N_RAYS + len(EDGE_SPH), 3), 72, -1, 1), dim=-1)
    sph = raymarching.sph_from_ray(ro, rd, BG["bg_radius"])
    sph[N_RAYS:] = torch.tensor(EDGE_SPH, dtype=torch.float32)
    grad = _seeded((N_RAYS + len(EDGE_SPH), 3), 73, -1, 1)
    net.zero_grad()
    rgb = net.background(sph, rd)
    rgb.backward(grad)
    out.update(bg_rays_o=ro.numpy(), bg_rays_d=rd.numpy(), bg_sph=sph.numpy(), bg_n_marched=np.int64(N_RAYS), bg_grad_rgb=grad.numpy(),
               bg_rgb=rgb.detach().numpy(), bg_grad_bg_mat=net.bg_mat.grad.numpy().copy(),
               bg_grad_bg_net_0_weight=net.bg_net[0].weight.grad.numpy().copy(),
               bg_grad_bg_net_1_weight=net.bg_net[1].weight.grad.numpy().copy())
    # (b) one executed Trainer.train_step with the background model (gen_tensorf's scene and seeds)
    syn = _load_synthetic()
    torch.manual_seed(3)
    net = trf.NeRFNetwork(**dict(TENSORF_NET, **TS_BG))
    _seed_params(net)
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net.mean_count = 32768
    poses = syn.orbit_poses(1, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"].contiguous(), r["rays_d"].contiguous()
    images = _seeded((1, 256, 3), 82)
    opt = types.SimpleNamespace(color_space="srgb", patch_size=1, dt_gamma=0, max_steps=1024, T_thresh=1e-4, l1_reg_weight=1e-4)
    me = object.__new__(tu.Trainer)
    me.model, me.opt, me.criterion, me.error_map = net, opt, torch.nn.MSELoss(reduction="none"), None
    me._backbone, me.log_ptr = strainer.BackBoneTypes.TensoRF, None
    net.train()
    torch.manual_seed(5)
    pred, _, loss = tu.Trainer.train_step(me, {"rays_o": ro, "rays_d": rd, "images": images.clone()})
    net.zero_grad()
    loss.backward()
    out.update(ts_rays_o=ro.numpy(), ts_rays_d=rd.numpy(), ts_images=images.numpy(), ts_loss=np.float64(loss.item()),
               ts_pred=pred.detach().numpy(), ts_counter=net.step_counter[0].numpy().copy(), ts_l1_weight=np.float64(opt.l1_reg_weight),
               ts_mean_count=np.int64(32768))
    rec = {}
    _grad_record_flat(net, "ts_grad", rec)
    out.update({k: v for k, v in rec.items() if "_bg_" in k or k.endswith("_norm")})
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
    print("tensorf_background: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes; rgb mean", float(rgb.detach().mean()),
          "train loss", loss.item())


if __name__ == "__main__":
    main()
