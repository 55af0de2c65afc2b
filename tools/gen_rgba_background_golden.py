#!/usr/bin/env python3
"""Generate tests/golden/rgba_background.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the reference's training on RGBA frames — the per-pixel random background of nerf/utils.py:465-474 and the compositing
of the prediction on the same colours (nerf/renderer.py:316) — by EXECUTING it on the CPU oracle:

  (a) one reference `Trainer.train_step` (nerf/utils.py:436-537) on oracle.gen_golden's `train` scene (same network settings,
      seeded parameters, density grid and jitter seed) with fp32 `images [1, 512, 4]`, `bg_radius` 0, under torch.manual_seed:
      the drawn `bg_color` (what the step hands to `render`), `gt_rgb`, `pred_rgb`, the loss and every parameter gradient;
  (b) the same step with the error map set, its rays drawn by `get_rays(error_map=...)`: the map entries the step touched;
  (c) `eval_step`'s blend of a small `[1, 16, 16, 4]` frame onto white (nerf/utils.py:549-554): `gt_rgb`;
  (d) the train step on fp16 frames (the `-O` preload): `bg_color` and `gt_rgb`, both half.

Alphas hold exact 0, exact 1 and values between.

    python tools/gen_rgba_background_golden.py     (re-running reproduces the file bit for bit)
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
from oracle.gen_golden import (TRAIN_NET, _assert_reference, _grad_record, _install_reference_stack, _load_synthetic,  # noqa: E402
                               _seed_params, _seeded, _stub_training_imports)
from tools.gen_error_map_golden import _map  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "rgba_background.npz")


def _rgba(shape, seed):
    """seeded RGBA in [0, 1); every fourth alpha exactly 0, every fourth exactly 1, the rest between"""
    img = _seeded(tuple(shape) + (4,), seed)
    a = img[..., 3].reshape(-1)
    a[0::4] = 0.0
    a[1::4] = 1.0
    return img.contiguous()


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
    poses = syn.orbit_poses(2, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=512, generator=torch.Generator().manual_seed(41))
    ro, rd = r["rays_o"].contiguous(), r["rays_d"].contiguous()
    emap0 = _map(2, 300)
    torch.manual_seed(41)
    rm = utils.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, 512, emap0[[0]])
    images = _rgba((1, 512), 42)
    opt = types.SimpleNamespace(color_space="srgb", patch_size=1, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    out.update(seed=np.int64(5), mean_count=np.int64(32768), images=images.numpy(), a_rays_o=ro.numpy(), a_rays_d=rd.numpy(),
               b_rays_o=rm["rays_o"].numpy(), b_rays_d=rm["rays_d"].numpy(), b_inds_coarse=rm["inds_coarse"].numpy(),
               b_map=emap0.numpy())

    def step(tag, rays_o, rays_d, imgs, emap=None, extra=None, record_gt=False):
        torch.manual_seed(3)
        net = network.NeRFNetwork(**TRAIN_NET)
        _seed_params(net)
        dens, bits = syn.lego_like_density_grid(seed=0)
        net.density_grid.copy_(torch.from_numpy(dens))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.mean_count = 32768
        seen = {}
        render = net.render

        def spy(*a, **k):  # (what the step hands to the renderer)
            seen["bg_color"] = k["bg_color"]
            return render(*a, **k)
        net.render = spy
        mse = torch.nn.MSELoss(reduction="none")

        def criterion(pred, gt):  # (the half targets of (d): recorded as formed, widened for the criterion)
            seen["gt_rgb"] = gt
            return mse(pred, gt.float())
        me = types.SimpleNamespace(model=net, opt=opt, _backbone=strainer.BackBoneTypes.NGP,
                                   criterion=criterion if record_gt else mse, criterion_depth=torch.nn.L1Loss(), error_map=emap)
        net.train()
        torch.manual_seed(5)
        pred, gt, loss = utils.Trainer.train_step(me, dict({"rays_o": rays_o, "rays_d": rays_d, "images": imgs.clone()}, **(extra or {})))
        return net, seen, pred, gt, loss

    # (a) fp32 RGBA frames, no background model
    net, seen, pred, gt, loss = step("a", ro, rd, images)
    assert torch.is_tensor(seen["bg_color"]) and seen["bg_color"].shape == (1, 512, 3) and gt.dtype == torch.float32
    net.zero_grad()
    loss.backward()
    out.update(a_bg_color=seen["bg_color"].numpy(), a_gt_rgb=gt.numpy(), a_pred_rgb=pred.detach().numpy(),
               a_loss=np.float64(loss.item()), a_counter=net.step_counter[0].numpy().copy())
    _grad_record(net, "a_grad", out)
    # (b) the same with the error map
    emap = emap0.clone()
    net, seen, pred, gt, loss = step("b", rm["rays_o"].contiguous(), rm["rays_d"].contiguous(), images, emap=emap,
                                     extra={"index": [0], "inds_coarse": rm["inds_coarse"]})
    ic = rm["inds_coarse"][0].numpy()
    touched = np.zeros(emap.shape, dtype=bool)
    touched[0, ic] = True
    assert np.array_equal(emap.numpy()[~touched], emap0.numpy()[~touched])
    out.update(b_bg_color=seen["bg_color"].numpy(), b_gt_rgb=gt.numpy(), b_loss=np.float64(loss.item()), b_touched=emap.numpy()[0, ic])
    # (c) eval_step's white blend
    frame = _rgba((1, 16, 16), 45)
    r16 = syn.get_rays(poses[1:2], syn.lego_intrinsics(16, 16), 16, 16)
    net.eval()
    net.render = types.MethodType(type(net).render, net)
    me = types.SimpleNamespace(model=net, opt=opt, criterion=torch.nn.MSELoss(reduction="none"))
    with torch.no_grad():
        _, _, gt_eval, _ = utils.Trainer.eval_step(me, {"rays_o": r16["rays_o"].contiguous(), "rays_d": r16["rays_d"].contiguous(),
                                                        "images": frame.clone()})
    out.update(c_images=frame.numpy(), c_gt_rgb=gt_eval.numpy())
    # (d) fp16 frames
    half = images.half()
    net, seen, pred, gt, loss = step("d", ro, rd, half, record_gt=True)
    assert seen["bg_color"].dtype == torch.half and seen["gt_rgb"].dtype == torch.half
    out.update(d_images=half.numpy(), d_bg_color=seen["bg_color"].numpy(), d_gt_rgb=seen["gt_rgb"].numpy())
    a = images[..., 3]
    assert bool((a == 0).any()) and bool((a == 1).any()) and bool(((a > 0) & (a < 1)).any())
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
    print("rgba_background: wrote", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes; loss", out["a_loss"], out["b_loss"])


if __name__ == "__main__":
    main()
