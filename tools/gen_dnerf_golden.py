#!/usr/bin/env python3
"""Generate tests/golden/dnerf.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the D-NeRF backbone the way tools/gen_ccnerf_golden.py pins the CCNeRF one: the reference's dnerf/network.py `NeRFNetwork`
(deformation MLP in front of the NGP heads) with seeded parameters is EXECUTED on the CPU oracle stack — parameter names and
shapes, the `get_params` group layout, `forward` and `density` on seeded points (some of them on +-bound) at t = 0, 0.37 and 1,
`run_cuda` in train and eval mode and the sampling path `run` at 256 rays, and dnerf/utils.py `Trainer.train_step` with the
deformation regulariser and every parameter gradient.  Only recorded arrays are stored.

`time_size` is the reference's hard-coded 64.  The occupancy grid is analytic and seeded: the slot of t = 0.37 (slot 23) holds the
synthetic scene's grid, every other slot is empty, packed per slot — the reference's own sweep (64 x 128^3 CPU queries) is not run.
With `mean_count` 0 the marcher trims its buffers, so the regulariser's mean runs over the rows that hold a sample.

    python tools/gen_dnerf_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import (_assert_reference, _grad_record_flat, _install_reference_stack, _load_synthetic, _seed_params,  # noqa: E402
                               _seeded, _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "dnerf.npz")
NET = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
TIMES = (0.0, 0.37, 1.0)
SLOT = 23  # floor(0.37 * 64)
SEED_RANGE = 0.1


def _points():
    x = _seeded((300, 3), 71, -1.0, 1.0)
    edge = torch.tensor([-1.0, 1.0, 0.0, -1.0, 1.0])
    for a in range(3):
        x[5 * a:5 * a + 5, a] = edge
    x[15:18] = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    return x


def main():
    _install_reference_stack()
    _stub_training_imports()
    dn = importlib.import_module("dnerf.network")
    du = importlib.import_module("dnerf.utils")
    for m_ in (dn, du):
        _assert_reference(m_)
    syn = _load_synthetic()
    out = {}

    def make(**over):
        torch.manual_seed(3)
        net = dn.NeRFNetwork(**dict(NET, **over))
        _seed_params(net, -SEED_RANGE, SEED_RANGE)
        return net
    net = make()
    assert net.time_size == 64
    out.update(param_names=np.array([k for k, _ in net.named_parameters()]),
               param_shapes=np.array([str(tuple(p.shape)) for _, p in net.named_parameters()]),
               buffer_names=np.array([k for k, _ in net.named_buffers()]),
               buffer_shapes=np.array([str(tuple(b.shape)) for _, b in net.named_buffers()]),
               seed_range=np.float64(SEED_RANGE), slot=np.int64(SLOT))
    groups = net.get_params(1e-2, 1e-3)
    names = {id(p): k for k, p in net.named_parameters()}
    out["group_lrs"] = np.array([g["lr"] for g in groups])
    out["group_members"] = np.array([",".join(names[id(p)] for p in g["params"]) for g in groups])
    x = _points()
    d = torch.nn.functional.normalize(_seeded((300, 3), 72, -1, 1), dim=-1)
    out.update(fw_x=x.numpy(), fw_d=d.numpy(), fw_t=np.array(TIMES))
    net.eval()
    with torch.no_grad():
        for k, tv in enumerate(TIMES):
            t = torch.tensor([[tv]], dtype=torch.float32)
            sg, cl, df = net(x, d, t)
            dens = net.density(x, t)
            out.update({f"fw{k}_sigma": sg.numpy(), f"fw{k}_rgb": cl.numpy(), f"fw{k}_deform": df.numpy(),
                        f"dn{k}_sigma": dens["sigma"].numpy(), f"dn{k}_geo": dens["geo_feat"].numpy(), f"dn{k}_deform": dens["deform"].numpy()})
    # -- the occupancy grid: one analytic slot, packed per slot
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid[SLOT].copy_(torch.from_numpy(dens))
    net.density_bitfield[SLOT].copy_(torch.from_numpy(bits))
    poses = syn.orbit_poses(1, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"].contiguous(), r["rays_d"].contiguous()
    time = torch.tensor([[0.37]], dtype=torch.float32)
    out.update(rays_o=ro.numpy(), rays_d=rd.numpy(), time=time.numpy())
    with torch.no_grad():
        net.eval()
        res = net.run_cuda(ro, rd, time, bg_color=1, perturb=False, max_steps=1024, dt_gamma=0)
        out.update(eval_image=res["image"].numpy(), eval_depth=res["depth"].numpy())
        empty = net.run_cuda(ro, rd, torch.tensor([[0.9]]), bg_color=1, perturb=False, max_steps=1024, dt_gamma=0)
        out.update(eval_empty_image=empty["image"].numpy())
        net.train()
        net.mean_count, net.local_step = 0, 0
        res = net.run_cuda(ro, rd, time, bg_color=1, perturb=False, force_all_rays=False, max_steps=1024, dt_gamma=0)
        out.update(train_image=res["image"].numpy(), train_depth=res["depth"].numpy(), train_deform_rows=np.int64(res["deform"].shape[0]),
                   train_deform_absmean=np.float64(res["deform"].abs().double().mean()), train_counter=net.step_counter[0].numpy().copy())
        # -- the sampling path `run` (no occupancy grid), eval mode: deterministic upsampling
        plain = make(cuda_ray=False).eval()
        res = plain.run(ro[:, :64], rd[:, :64], time, num_steps=16, upsample_steps=16, bg_color=1, perturb=False)
        out.update(run_image=res["image"].numpy(), run_depth=res["depth"].numpy(), run_deform=res["deform"].numpy())
    # -- Trainer.train_step (dnerf/utils.py:38-121) on an instance made without __init__
    images = _seeded((1, 256, 3), 82)
    opt = types.SimpleNamespace(color_space="srgb", dt_gamma=0, max_steps=1024)
    me = object.__new__(du.Trainer)
    me.model, me.opt, me.criterion, me.error_map, me.log_ptr = net, opt, torch.nn.MSELoss(reduction="none"), None, None
    net.train()
    net.mean_count, net.local_step = 0, 0
    net.step_counter.zero_()
    torch.manual_seed(5)
    pred, gt, loss = du.Trainer.train_step(me, {"rays_o": ro, "rays_d": rd, "time": time, "images": images.clone()})
    net.zero_grad()
    loss.backward()
    out.update(ts_images=images.numpy(), ts_loss=np.float64(loss.item()), ts_pred=pred.detach().numpy(),
               ts_counter=net.step_counter[0].numpy().copy(),
               ts_mse=np.float64(torch.nn.functional.mse_loss(pred.detach(), gt).item()))
    _grad_record_flat(net, "ts_grad", out, n=512)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays); train loss {loss.item()} "
          f"|deform| max {float(np.abs(out['fw1_deform']).max())} sigma max {float(out['fw1_sigma'].max())}")


if __name__ == "__main__":
    main()
