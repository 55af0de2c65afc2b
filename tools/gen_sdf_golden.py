#!/usr/bin/env python3
"""Generate tests/golden/sdf.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the SDF backbone the way tools/gen_dnerf_golden.py pins the D-NeRF one: the reference's sdf/netowrk.py `SDFNetwork` with seeded
parameters is EXECUTED on the CPU oracle stack — parameter names and shapes, the forward at 300 seeded points (some of them on
+-1), and sdf/utils.py `Trainer.train_step` with loss.py `mape_loss`, the loss and every parameter gradient, with and without
`clip_sdf = 0.1`.  Only recorded arrays are stored.  sdf/provider.py cannot be executed (trimesh, pysdf): the dataset's contracts
are covered by tests/sdf_witness.py.

    python tools/gen_sdf_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import (_assert_reference, _grad_record_flat, _install_reference_stack, _seed_params, _seeded,  # noqa: E402
                               _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "sdf.npz")
SEED_RANGE = 0.5
CLIP = 0.1


def _points():
    x = _seeded((300, 3), 91, -1.0, 1.0)
    edge = torch.tensor([-1.0, 1.0, 0.0, -1.0, 1.0])
    for a in range(3):
        x[5 * a:5 * a + 5, a] = edge
    x[15:18] = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    return x


def main():
    _install_reference_stack()
    _stub_training_imports()
    sn = importlib.import_module("sdf.netowrk")
    su = importlib.import_module("sdf.utils")
    ls = importlib.import_module("loss")
    for m_ in (sn, su, ls):
        _assert_reference(m_)
    out = {}

    def make(**over):
        torch.manual_seed(3)
        net = sn.SDFNetwork(encoding="hashgrid", **over)
        _seed_params(net, -SEED_RANGE, SEED_RANGE)
        return net
    net = make()
    out.update(param_names=np.array([k for k, _ in net.named_parameters()]),
               param_shapes=np.array([str(tuple(p.shape)) for _, p in net.named_parameters()]),
               state_names=np.array(list(net.state_dict())), seed_range=np.float64(SEED_RANGE), clip=np.float64(CLIP))
    x = _points()
    y = _seeded((300, 1), 92, -0.3, 0.3)
    y[20:24] = 0.0  # (targets on the surface: the floor of the scale)
    out.update(x=x.numpy(), y=y.numpy())
    for tag, over in (("plain", {}), ("clip", dict(clip_sdf=CLIP))):
        net = make(**over)
        net.eval()
        with torch.no_grad():
            out[f"{tag}_forward"] = net(x).numpy()
        me = object.__new__(su.Trainer)
        me.model, me.criterion, me.log_ptr = net, ls.mape_loss, None
        net.train()
        pred, truth, loss = su.Trainer.train_step(me, {"points": x[None], "sdfs": y[None]})
        net.zero_grad()
        loss.backward()
        out.update({f"{tag}_loss": np.float64(loss.item()), f"{tag}_pred": pred.detach().numpy(),
                    f"{tag}_mape_rows": ls.mape_loss(pred.detach(), truth, reduction="none").numpy()})
        _grad_record_flat(net, f"{tag}_grad", out, n=512)
    assert (np.abs(out["plain_forward"]) > CLIP).any() and (np.abs(out["plain_forward"]) < CLIP).any()  # (the clamp is live, not total)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays); loss {out['plain_loss']} / clipped {out['clip_loss']}; "
          f"|sdf| max {float(np.abs(out['plain_forward']).max())}")


if __name__ == "__main__":
    main()
