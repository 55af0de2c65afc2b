"""SDF network (sdf/netowrk.py of the reference): sdf = MLP([grid(x)]), a hash grid in front of `num_layers` bias-free Linear layers
with ReLU between them, optional skip connections that re-append the encoding, and an optional clamp of the output.

Two routes (DESIGN.md "SDF"), chosen as dnerf/network.py chooses: the reference's torch op sequence (CPU, fp32, any shape, skips),
and under fp16 autocast on the GPU the grid encoder's level-major output straight into the fully fused 32 -> 64 -> 64 -> 1 MLP —
the existing entry points, no kernel of its own.  `forward_padded` hands the MLP's [Bp, 16] fp16 rows to the fused criterion
(s3d_sdf_mape_forward_backward), which clamps by `clip_sdf` itself."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import s3d_hip
from encoding import get_encoder
from ffmlp.ffmlp import ffmlp_forward


class SDFNetwork(nn.Module):
    cuda_ray = False  # (nerf/checkpoint.py asks every model: there is no occupancy state to store)

    def __init__(self, encoding="hashgrid", num_layers=3, skips=[], hidden_dim=64, clip_sdf=None):
        super().__init__()
        self.num_layers, self.skips, self.hidden_dim, self.clip_sdf = num_layers, list(skips), hidden_dim, clip_sdf
        self.encoder, self.in_dim = get_encoder(encoding)
        dims = []
        for l in range(num_layers):
            fan_in = self.in_dim if l == 0 else hidden_dim + (self.in_dim if l in self.skips else 0)
            dims.append((fan_in, 1 if l == num_layers - 1 else hidden_dim))
        self.backbone = nn.ModuleList([nn.Linear(i, o, bias=False) for i, o in dims])

    # ---- the fused route ---------------------------------------------------------------------------------------------------
    fused_mlp = True  # False (test reference): the torch op sequence everywhere

    def _shape_ok(self):
        """what the fused MLP entry points take: 16 levels x 2 features of a 3-D grid in front of 64 -> 64 -> 1, no skips"""
        e = self.encoder
        return (not self.skips and self.num_layers == 3 and self.hidden_dim == 64 and getattr(e, "level_dim", 0) == 2
                and getattr(e, "num_levels", 0) == 16 and getattr(e, "input_dim", 0) == 3
                and s3d_hip.FFMLPBackend.fused_backward_supported(32, 16, 64, 2, 0))

    def can_fuse(self, x):
        return (self.fused_mlp and x.is_cuda and x.dim() == 2 and x.shape[-1] == 3 and x.shape[0] > 0 and x.dtype == torch.float32
                and not x.requires_grad and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16
                and self._shape_ok())

    def _pack(self):
        """[64 x 32 | 64 x 64 | 16 x 64]: the last matrix padded from 1 to 16 rows (their products are exact zeros)"""
        w0, w1, w2 = (l.weight for l in self.backbone)
        return torch.cat([w0.reshape(-1), w1.reshape(-1), F.pad(w2, (0, 0, 0, 16 - w2.shape[0])).reshape(-1)])

    def forward_padded(self, x):
        """x fp32 [B, 3] on the GPU under fp16 autocast -> the MLP's rows [Bp, 16] fp16, Bp = B rounded up to 128 (the padding rows
        sit at x = 0), column 0 the unclamped distance"""
        if not self.can_fuse(x):
            raise RuntimeError("SDFNetwork.forward_padded: the fused route needs fp32 [B, 3] GPU input under fp16 autocast and the "
                               "32 -> 64 -> 64 -> 1 shape without skips; call forward()")
        B = x.shape[0]
        pad = (-B) % 128
        if pad:
            x = torch.cat([x, x.new_zeros(pad, 3)], dim=0)
        e = self.encoder(x.contiguous(), level_major=True)
        infer = not torch.is_grad_enabled()
        return ffmlp_forward(e, self._pack(), 32, 16, 64, 2, 0, 6, infer, e.requires_grad, None, None, 1, None)

    # ---- the reference's op sequence -------------------------------------------------------------------------------------------
    def _forward_torch(self, x):
        x = self.encoder(x)
        h = x
        for l, layer in enumerate(self.backbone):
            if l in self.skips:
                h = torch.cat([h, x], dim=-1)
            h = layer(h)
            if l != self.num_layers - 1:
                h = F.relu(h, inplace=True)
        return h

    def forward(self, x):
        """x [B, 3] in [-1, 1] -> sdf [B, 1]"""
        if self.can_fuse(x):
            h = self.forward_padded(x)[:x.shape[0], :1]
        else:
            h = self._forward_torch(x)
        if self.clip_sdf is not None:
            h = h.clamp(-self.clip_sdf, self.clip_sdf)
        return h
