#!/usr/bin/env python3
"""Generate tests/golden/dnerf_hyper.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the D-NeRF hyper backbone the way tools/gen_dnerf_basis_golden.py pins the temporal-basis one: the reference's
dnerf/network_hyper.py `NeRFNetwork` with seeded parameters is EXECUTED on the CPU oracle stack — parameter and buffer names and
shapes, the `get_params` group layout, `forward` and `density` on the 300 seeded points (some of them on +-bound) at t = 0, 0.37 and
1, `run_cuda` in train and eval mode at 256 rays, and dnerf/utils.py `Trainer.train_step` (no regulariser term: this model's
`deform` is None) with every parameter gradient.  Only recorded arrays are stored.  The sampling path `run` is not recorded: the
reference's raises KeyError for this model (dnerf/renderer.py:257 reads `density_outputs['deform']`).

`train_step` is recorded twice: as constructed (linear interpolation: every `ambient_net` gradient is EXACTLY zero, because the grid
kernel's `pos_deriv[D] = {1.0f}` zeroes the Jacobian of every dimension but 0 — asserted here), and with the executed model's
`encoder.interp_id` set to smoothstep (the gradients are not zero — asserted here).

`time_size` is the reference's hard-coded 64.  The occupancy grid is analytic and seeded: the slot of t = 0.37 (slot 23) holds the
synthetic scene's grid, every other slot is empty, packed per slot.

    python tools/gen_dnerf_hyper_golden.py     (re-running reproduces the file bit for bit)
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
sys.path.insert(0, HERE)
from oracle.gen_golden import (_assert_reference, _grad_record_flat, _install_reference_stack, _load_synthetic, _seed_params,  # noqa: E402
                               _seeded, _stub_training_imports)
from gen_dnerf_golden import NET, SLOT, TIMES, _points  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "dnerf_hyper.npz")
# (0.1, the deformation fixture's range, leaves the ambient near zero behind five layers and sigma = 1, rgb = 0.5 to four digits:
#  the trap tools/gen_dnerf_basis_golden.py describes)
SEED_RANGE = 0.25


def main():
    _install_reference_stack()
    _stub_training_imports()
    nh = importlib.import_module("dnerf.network_hyper")
    du = importlib.import_module("dnerf.utils")
    for m_ in (nh, du):
        _assert_reference(m_)
    syn = _load_synthetic()
    out = {}
    torch.manual_seed(3)
    net = nh.NeRFNetwork(**NET)
    _seed_params(net, -SEED_RANGE, SEED_RANGE)
    assert net.time_size == 64 and net.encoder.interp_id == 0 and net.encoder.input_dim == 4
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
            assert df is None
            dens = net.density(x, t)
            out.update({f"fw{k}_sigma": sg.numpy(), f"fw{k}_rgb": cl.numpy(),
                        f"dn{k}_sigma": dens["sigma"].numpy(), f"dn{k}_geo": dens["geo_feat"].numpy()})
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
        assert res["deform"] is None
        out.update(train_image=res["image"].numpy(), train_depth=res["depth"].numpy(), train_counter=net.step_counter[0].numpy().copy())
    # -- Trainer.train_step (dnerf/utils.py:38-121) on an instance made without __init__: linear, then smoothstep
    images = _seeded((1, 256, 3), 82)
    opt = types.SimpleNamespace(color_space="srgb", dt_gamma=0, max_steps=1024)
    me = object.__new__(du.Trainer)
    me.model, me.opt, me.criterion, me.error_map, me.log_ptr = net, opt, torch.nn.MSELoss(reduction="none"), None, None
    out["ts_images"] = images.numpy()
    for prefix, interp_id in (("ts", 0), ("tss", 1)):
        net.encoder.interp_id = interp_id
        net.train()
        net.mean_count, net.local_step = 0, 0
        net.step_counter.zero_()
        torch.manual_seed(5)
        pred, gt, loss = du.Trainer.train_step(me, {"rays_o": ro, "rays_d": rd, "time": time, "images": images.clone()})
        net.zero_grad()
        loss.backward()
        out.update({f"{prefix}_loss": np.float64(loss.item()), f"{prefix}_pred": pred.detach().numpy(),
                    f"{prefix}_counter": net.step_counter[0].numpy().copy(),
                    f"{prefix}_mse": np.float64(torch.nn.functional.mse_loss(pred.detach(), gt).item())})
        _grad_record_flat(net, f"{prefix}_grad", out, n=512)
        amb = [float(l.weight.grad.abs().max()) for l in net.ambient_net]
        if interp_id == 0:
            assert all(a == 0.0 for a in amb), amb  # (exactly: the Jacobian column is a sum of products with the constant 0)
        else:
            assert all(a > 0.0 for a in amb), amb
        print(f"[{prefix}] loss {loss.item()} max |grad ambient_net| {amb}")
    net.encoder.interp_id = 0
    ambient = [float(torch.tanh(_run(net, tv))) for tv in TIMES]
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays); ambient at {TIMES}: {ambient}; "
          f"sigma {float(out['fw1_sigma'].min())}..{float(out['fw1_sigma'].max())} "
          f"rgb {float(out['fw1_rgb'].min())}..{float(out['fw1_rgb'].max())}")


def _run(net, tv):
    """the ambient net's pre-activation at time tv (printed only: the seed range must leave tanh unsaturated and time-dependent)"""
    with torch.no_grad():
        h = net.encoder_time(torch.tensor([[tv]], dtype=torch.float32))
        for k, layer in enumerate(net.ambient_net):
            h = layer(h)
            if k != len(net.ambient_net) - 1:
                h = torch.relu(h)
    return h.reshape(())


if __name__ == "__main__":
    main()
