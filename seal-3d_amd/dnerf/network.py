"""D-NeRF network (dnerf/network.py of the reference): a time-conditioned deformation MLP in front of the NGP density and colour
heads.  deform = MLP_5x128([freq_10(x) | freq_6(t)]), x' = x + deform, h = MLP_2x64([grid(x') | freq_10(x) | freq_6(t)]),
sigma = trunc_exp(h0), rgb = sigmoid(MLP_3x64([SH_4(d) | h1..15])).

Two routes (DESIGN.md "D-NeRF"): the reference's torch op sequence (CPU, fp32, any shape), and under fp16 autocast on the GPU
the kernels of csrc/dnerf.hip around the fused MLP entry points — the gradient of the density reaches the deformation network
through the grid's input Jacobian `dy_dx`."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

import s3d_hip
from activation import trunc_exp
from encoding import get_encoder
from ffmlp.ffmlp import ffmlp_forward
from gridencoder.grid import _table_backward, _table_for_kernels, note_table_use
from nerf.network import _Background, _mlp, _run_mlp
from nerf.network_ff import _NgpMid, _NgpRgb

from .renderer import NeRFRenderer

_dn = s3d_hip.DnerfBackend
DIN, SIN = 80, 112


class _Rows:
    """the two input rows of one call (not tensors of the autograd graph: _WarpGrid fills `sin` and hands it out)"""
    __slots__ = ("din", "sin", "B")


def _encode_rows(x, t):
    """din [Bp, 80] and sin [Bp, 112] (Bp = B rounded up to the MLP kernels' 128 rows, the padding rows zero) with everything but
    the grid columns of `sin` filled"""
    B = x.shape[0]
    Bp = (B + 127) // 128 * 128
    rows = _Rows()
    rows.B = B
    rows.din = torch.empty(Bp, DIN, dtype=torch.float16, device=x.device)
    rows.sin = torch.empty(Bp, SIN, dtype=torch.float16, device=x.device)
    if Bp != B:  # (fewer than 128 padding rows: only they are cleared)
        rows.din[B:].zero_()
        rows.sin[B:].zero_()
    _dn.encode_forward(x, t, rows.din[:B], rows.sin[:B])
    return rows


class _WarpGrid(Function):
    """x' = x + deform and the grid encoding of x' into the density network's row (s3d_dnerf_warp_grid_forward); backward:
    split_grad -> the table backward with dy_dx (gridencoder.grid._table_backward: the table gradient takes the optimizer's
    hand-over like every other table's) -> warp_backward.  Returns (sin, deform fp32 [B, 3], reg_sum or None)."""

    @staticmethod
    def forward(ctx, x, dout, table_param, enc, bound, rows, want_reg):
        B = rows.B
        # (grad mode is off inside a Function's forward: what the call needs is asked of autograd)
        table = _table_for_kernels(table_param, not any(ctx.needs_input_grad))
        L = enc.num_levels
        S = float(np.log2(enc.per_level_scale))
        dev = x.device
        xw = torch.empty(B, 3, dtype=torch.float32, device=dev)
        deform = torch.empty(B, 3, dtype=torch.float32, device=dev)
        dy_dx = torch.empty(B, L * 6, dtype=table.dtype, device=dev) if ctx.needs_input_grad[1] else None
        reg = torch.empty((), dtype=torch.float32, device=dev) if want_reg else None
        sin = rows.sin
        _dn.warp_grid_forward(x, dout[:B], table, enc.offsets, S, enc.base_resolution, enc.gridtype_id, enc.align_corners,
                              enc.interp_id, bound, sin[:B], xw, deform, dy_dx, reg)
        ctx.save_for_backward(xw, table, enc.offsets, dy_dx, deform)
        ctx.geometry = (B, 3, 2, L, S, enc.base_resolution, enc.gridtype_id, enc.align_corners, enc.interp_id)
        ctx.param, ctx.bound, ctx.rows_padded = table_param, bound, sin.shape[0]
        ctx.mark_non_differentiable(deform)
        ctx.set_materialize_grads(False)
        return sin, deform, reg

    @staticmethod
    def backward(ctx, g_sin, g_deform, g_reg):
        xw, table, offsets, dy_dx, deform = ctx.saved_tensors
        B, L = ctx.geometry[0], ctx.geometry[3]
        dev = xw.device
        g_x = None
        g_table = None
        if g_sin is not None:
            g_sin = g_sin.to(torch.float16).contiguous()
            g_levels = torch.empty(L, B, 2, dtype=table.dtype, device=dev)
            _dn.split_grad(g_sin[:B], g_levels)
            # (the grid backward takes an input Jacobian with normalised inputs only: x01 as load_point forms it — a multiplication
            #  by the exact reciprocal of a power of two — on the [B, 3] tensor the forward kept)
            x01 = xw.add(ctx.bound).mul_(1.0 / (2.0 * ctx.bound)) if dy_dx is not None else xw
            g_x, g_table = _table_backward(ctx.param, table, g_levels, x01, offsets, ctx.geometry,
                                           {} if dy_dx is not None else {"bound": ctx.bound}, dy_dx=dy_dx)
        g_dout = None
        if ctx.needs_input_grad[1]:
            if g_x is None:
                g_x = torch.zeros(B, 3, dtype=table.dtype, device=dev)
            Bp = ctx.rows_padded
            g_dout = (torch.empty if Bp == B else torch.zeros)(Bp, 16, dtype=torch.float16, device=dev)
            coef = None if g_reg is None else g_reg.float().reshape(1).contiguous()
            _dn.warp_backward(g_x, 1.0 / (2.0 * ctx.bound), deform, coef, g_dout[:B])
        return None, g_dout, (g_table if ctx.needs_input_grad[2] else None), None, None, None, None


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="tiledgrid", encoding_dir="sphere_harmonics", encoding_time="frequency", encoding_deform="frequency",
                 encoding_bg="hashgrid", num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                 num_layers_bg=2, hidden_dim_bg=64, num_layers_deform=5, hidden_dim_deform=128, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        # deformation network (dnerf/network.py:31-52)
        self.num_layers_deform, self.hidden_dim_deform = num_layers_deform, hidden_dim_deform
        self.encoder_deform, self.in_dim_deform = get_encoder(encoding_deform, multires=10)
        self.encoder_time, self.in_dim_time = get_encoder(encoding_time, input_dim=1, multires=6)
        self.deform_net = _mlp([self.in_dim_deform + self.in_dim_time] + [hidden_dim_deform] * (num_layers_deform - 1) + [3])
        # density network on [grid(x') | enc(x) | enc(t)] (:55-75)
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.encoder, self.in_dim = get_encoder(encoding, desired_resolution=2048 * bound)
        self.sigma_net = _mlp([self.in_dim + self.in_dim_time + self.in_dim_deform] + [hidden_dim] * (num_layers - 1) + [1 + geo_feat_dim])
        # colour network (:77-96)
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        self.encoder_dir, self.in_dim_dir = get_encoder(encoding_dir)
        self.color_net = _mlp([self.in_dim_dir + geo_feat_dim] + [hidden_dim_color] * (num_layers_color - 1) + [3])
        if self.bg_radius > 0:
            self.num_layers_bg, self.hidden_dim_bg = num_layers_bg, hidden_dim_bg
            self.encoder_bg, self.in_dim_bg = get_encoder(encoding_bg, input_dim=2, num_levels=4, log2_hashmap_size=19,
                                                          desired_resolution=2048)
            self.bg_net = _mlp([self.in_dim_bg + self.in_dim_dir] + [hidden_dim_bg] * (num_layers_bg - 1) + [3])
        else:
            self.bg_net = None
        self.register_buffer("_eye_hidden", torch.eye(hidden_dim), persistent=False)  # (not a checkpoint key)

    # ---- the fused route -------------------------------------------------------------------------------------------------
    fused_mlp = True  # False (test reference): the torch op sequence everywhere

    def _glue_ok(self):
        """the row layouts of csrc/dnerf.hip fit this model: freq_10(x), freq_6(t), a 3-D grid of 16 levels x 2 features (the kernels
        take fewer levels, but the packed density weights put freq_10(x) behind column 2 L, the row at column 32), and a bound whose
        normalisation is exact as a multiplication"""
        e, ex, et = self.encoder, self.encoder_deform, self.encoder_time
        return (getattr(ex, "degree", None) == 10 and getattr(ex, "input_dim", 0) == 3 and type(ex).__name__ == "FreqEncoder"
                and getattr(et, "degree", None) == 6 and getattr(et, "input_dim", 0) == 1 and type(et).__name__ == "FreqEncoder"
                and getattr(e, "level_dim", 0) == 2 and getattr(e, "input_dim", 0) == 3 and getattr(e, "num_levels", 0) == 16
                and self.bound > 0 and math.frexp(2.0 * self.bound)[0] == 0.5)

    def _can_fuse(self, x):
        return (self.fused_mlp and x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and x.dtype == torch.float32
                and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16 and self._glue_ok())

    # which of the three networks the fused MLP entry points take; another shape keeps THAT network on torch's Linear
    def _deform_fusable(self):
        return self.num_layers_deform == 5 and self.hidden_dim_deform == 128

    def _sigma_fusable(self):
        return self.num_layers == 2 and self.hidden_dim == 64 and self.geo_feat_dim == 15

    def _color_fusable(self):
        return (self.geo_feat_dim == 15 and self.num_layers_color == 3 and self.hidden_dim_color == 64
                and getattr(self.encoder_dir, "degree", None) == 4)

    def _pack_deform(self):
        """[128 x 80 | 3 x (128 x 128) | 16 x 128]: the first matrix padded from 76 to 80 columns, the last from 3 to 16 rows"""
        w = [l.weight for l in self.deform_net]
        return torch.cat([F.pad(w[0], (0, DIN - w[0].shape[1])).reshape(-1)] + [m.reshape(-1) for m in w[1:-1]]
                         + [F.pad(w[-1], (0, 0, 0, 16 - w[-1].shape[0])).reshape(-1)])

    def _pack_sigma(self):
        """[64 x 112 | I_64 | 16 x 64]: relu(I relu(a)) == relu(a) exactly, so the identity layer that makes the two-matrix network
        a shape the MLP entry points take changes neither values nor gradients (nerf/network.py does the same)"""
        w0, w1 = self.sigma_net[0].weight, self.sigma_net[1].weight
        return torch.cat([F.pad(w0, (0, SIN - w0.shape[1])).reshape(-1), self._eye_hidden.reshape(-1), w1.reshape(-1)])

    def _pack_color(self):
        c0, c1, c2 = (l.weight for l in self.color_net)
        return torch.cat([F.pad(c0, (0, 1)).reshape(-1), c1.reshape(-1), F.pad(c2, (0, 0, 0, 13)).reshape(-1)])

    def _time_tensor(self, t, dev):
        if t is None:
            t = self._bound_time
            if t is None:
                raise ValueError("dnerf: forward / density need a time `t` (or run inside NeRFRenderer.run_cuda / run)")
        if not torch.is_tensor(t):
            t = torch.tensor([[float(t)]], dtype=torch.float32)
        return t.to(device=dev, dtype=torch.float32)

    def _density_fused(self, x, t, want_reg):
        """-> (h [Bp, 16] fp16 or [B, 1 + geo] on the torch density net, deform fp32 [B, 3], reg_sum or None, Bp)"""
        B = x.shape[0]
        infer = not torch.is_grad_enabled()
        x = x.contiguous()
        rows = _encode_rows(x, t.reshape(-1).contiguous())
        Bp = rows.din.shape[0]
        if self._deform_fusable():
            dout = ffmlp_forward(rows.din, self._pack_deform(), DIN, 16, 128, 4, 0, 6, infer, False, None, None, 0, None)
        else:
            dout = F.pad(_run_mlp(self.deform_net, rows.din[:, :self.in_dim_deform + self.in_dim_time]).to(torch.float16), (0, 13))
        note_table_use(self.encoder.embeddings)
        sin, deform, reg = _WarpGrid.apply(x, dout.contiguous(), self.encoder.embeddings, self.encoder, float(self.bound), rows, want_reg)
        if self._sigma_fusable():
            h = ffmlp_forward(sin, self._pack_sigma(), SIN, 16, 64, 2, 0, 6, infer, sin.requires_grad, None, None, 0, None)
        else:
            h = _run_mlp(self.sigma_net, sin[:, :self.in_dim + self.in_dim_deform + self.in_dim_time])
        return h, deform, reg, Bp

    def _color_fused(self, h, d, B, Bp):
        d = d.float().contiguous()
        if Bp != B:
            d = torch.cat([d, torch.zeros(Bp - B, 3, dtype=d.dtype, device=d.device)], dim=0)
        infer = not torch.is_grad_enabled()
        sigma, cin = _NgpMid.apply(h.contiguous(), d)
        if s3d_hip.FFMLPBackend.fused_backward_supported(32, 16, 64, 2, 0):
            rgb = ffmlp_forward(cin, self._pack_color(), 32, 16, 64, 2, 0, 6, infer, cin.requires_grad, None, None, 0, None, True)
        else:
            rgb = _NgpRgb.apply(ffmlp_forward(cin, self._pack_color(), 32, 16, 64, 2, 0, 6, infer, cin.requires_grad, None, None, 0,
                                              None).contiguous())
        return sigma[:B], rgb[:B]

    # ---- the reference's op sequence ---------------------------------------------------------------------------------------
    def _deform_torch(self, x, t):
        enc_x = self.encoder_deform(x, bound=self.bound)
        enc_t = self.encoder_time(t)
        if enc_t.shape[0] == 1:
            enc_t = enc_t.repeat(x.shape[0], 1)
        deform = _run_mlp(self.deform_net, torch.cat([enc_x, enc_t], dim=1))
        return deform, enc_x, enc_t

    def _density_torch(self, x, t):
        deform, enc_x, enc_t = self._deform_torch(x, t)
        h = _run_mlp(self.sigma_net, torch.cat([self.encoder(x + deform, bound=self.bound), enc_x, enc_t], dim=1))
        return trunc_exp(h[..., 0]), h[..., 1:], deform

    def _rgb(self, d, geo_feat):
        return torch.sigmoid(_run_mlp(self.color_net, torch.cat([self.encoder_dir(d), geo_feat], dim=-1)))

    # ---- the model's surface -------------------------------------------------------------------------------------------------
    def forward(self, x, d, t=None):
        """x [N, 3] in [-bound, bound], d [N, 3], t [1, 1] in [0, 1] -> (sigma, rgbs, deform).  Without `t` (the base renderer's
        two-argument call inside run_cuda): the time the renderer bound for this rendering, the result is (sigma, rgbs) and
        `deform` is kept for the renderer."""
        bound_call = t is None
        t = self._time_tensor(t, x.device)
        self._deform_reg = None
        # A training render under a sample budget (mean_count > 0) hands over the marcher's padded buffers and announces the
        # device-side sample count (s3d_hip.row_limit).  The 112-wide density MLP runs on kernels that take no row limit, so the
        # count is read back here (one host read) and the networks run on the live rows — the count rounded up to 128, the
        # project's row-limit convention and exactly the rows the marcher keeps when it trims; sigma and rgb go back as rows of
        # the padded extent, `deform` keeps the live rows only — what the regulariser averages over.
        rows_all = x.shape[0]
        nv = s3d_hip.active_row_limit(rows_all) if self.training else None
        live = rows_all if nv is None else min((max(int(nv.reshape(-1)[0]), 0) + 127) // 128 * 128, rows_all)
        if live < rows_all:
            if live == 0:
                sigma, rgbs, deform = x.new_zeros(rows_all), x.new_zeros(rows_all, 3), x.new_zeros(0, 3)
                if bound_call:
                    self._deform_out = deform
                    return sigma, rgbs
                return sigma, rgbs, deform
            x, d = x[:live], d[:live]
        if self._can_fuse(x):
            want_reg = self.training and torch.is_grad_enabled()
            h, deform, reg, Bp = self._density_fused(x, t, want_reg)
            B = x.shape[0]
            if self._sigma_fusable() and self._color_fusable():
                sigma, rgbs = self._color_fused(h, d, B, Bp)
            else:
                h = h[:B]
                sigma, rgbs = trunc_exp(h[..., 0]), self._rgb(d, h[..., 1:])
            if reg is not None:
                self._deform_reg = (reg, B)  # (dnerf/utils.py: the regulariser's value and the route of its gradient)
        else:
            sigma, geo_feat, deform = self._density_torch(x, t)
            rgbs = self._rgb(d, geo_feat)
        if live < rows_all:
            sigma, rgbs = F.pad(sigma, (0, rows_all - live)), F.pad(rgbs, (0, 0, 0, rows_all - live))
        if bound_call:
            self._deform_out = deform
            return sigma, rgbs
        return sigma, rgbs, deform

    def density(self, x, t=None):
        t = self._time_tensor(t, x.device)
        if self._can_fuse(x):
            h, deform, _, _ = self._density_fused(x, t, False)
            h = h[:x.shape[0]]
            return {"sigma": trunc_exp(h[..., 0]), "geo_feat": h[..., 1:], "deform": deform}
        sigma, geo_feat, deform = self._density_torch(x, t)
        return {"sigma": sigma, "geo_feat": geo_feat, "deform": deform}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        if mask is None:
            return self._rgb(d, geo_feat)
        rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
        if mask.any():
            rgbs[mask] = self._rgb(d[mask], geo_feat[mask]).to(rgbs.dtype)
        return rgbs

    fused_background = True

    def background(self, x, d):
        """the NGP background head, unchanged (nerf/network.py: _Background)"""
        from nerf.network import NeRFNetwork as _Ngp
        if _Ngp._can_fuse_bg(self, x):
            return _Background.apply(x, d, self.encoder_bg.embeddings, self.bg_net[0].weight, self.bg_net[1].weight, self.encoder_bg)
        h = torch.cat([self.encoder_dir(d), self.encoder_bg(x)], dim=-1)
        return torch.sigmoid(_run_mlp(self.bg_net, h))

    def get_params(self, lr, lr_net):
        groups = [(self.encoder, lr), (self.sigma_net, lr_net), (self.encoder_dir, lr), (self.color_net, lr_net),
                  (self.encoder_deform, lr), (self.encoder_time, lr), (self.deform_net, lr_net)]
        if self.bg_radius > 0:
            groups += [(self.encoder_bg, lr), (self.bg_net, lr_net)]
        return [{"params": g.parameters(), "lr": r} for g, r in groups]
