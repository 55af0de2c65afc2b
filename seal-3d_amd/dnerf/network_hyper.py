"""D-NeRF hyper network (dnerf/network_hyper.py of the reference, `main_dnerf.py --hyper`): an NGP whose grid is 4-dimensional — the
fourth coordinate is an "ambient" scalar from a 5 x 128 MLP on freq_6(t), evaluated on ONE row per call because `t` is [1, 1]:
ambient = tanh(ambient_net(freq_6(t))) * bound, h = MLP_2x64(grid_4D([x | ambient])) [33], sigma = trunc_exp(h[:, 0]),
rgb = sigmoid(MLP_3x64([SH_4(d) | h[:, 1:]])).

Two routes (DESIGN.md "D-NeRF, hyper"): the reference's torch op sequence (CPU, fp32, any shape, ambient_dim != 1), and under fp16
autocast on the GPU the lookup of csrc/dnerf_hyper.hip — features, the 4-D input row and the ambient column of the Jacobian from 16
gathers per level, no [N, 4] cat, no dy_dx tensor, and a table backward without dy_dx that keeps the optimizer's hand-over — between
torch's Linear (ambient net, density net), the basis model's density-head kernel with the constant basis e_0, and the fused MLP
entry points (colour net).

`interpolation` is a build extension: under the reference's only setting, "linear", the ambient net receives an exactly zero
gradient (the grid kernel's `pos_deriv[D] = {1.0f}` zeroes the Jacobian of every dimension but 0); "smoothstep" is the setting under
which it learns."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Function

import s3d_hip
from activation import trunc_exp
from encoding import get_encoder
from ffmlp.ffmlp import ffmlp_forward
from gridencoder.grid import _table_backward, _table_for_kernels, note_table_use
from nerf.network import _Background, _mlp, _run_mlp

from .network_basis import BASIS, CIN, ROW, _BasisMid
from .renderer import NeRFRenderer

_hy = s3d_hip.DnerfHyperBackend


class _HyperGrid(Function):
    """feat [B, 2 L] fp16 = grid_4D([x | ambient]) (s3d_dnerf_hyper_grid_forward); backward: s3d_dnerf_hyper_grid_backward (the
    level-major gradient and grad_ambient, a fixed-order fp32 sum) -> the table backward WITHOUT dy_dx on the [B, 4] row the forward
    wrote (gridencoder.grid._table_backward: the optimizer's fp16 hand-over and an armed fused Adam update apply).  Under linear
    interpolation the ambient column of the Jacobian is identically zero: it is neither produced nor stored, and grad_ambient is
    zeros without a launch."""

    @staticmethod
    def forward(ctx, x, ambient, table_param, enc, bound):
        B, L = x.shape[0], enc.num_levels
        # (grad mode is off inside a Function's forward: what the call needs is asked of autograd)
        table = _table_for_kernels(table_param, not any(ctx.needs_input_grad))
        S = float(np.log2(enc.per_level_scale))
        dev = x.device
        feat = torch.empty(B, 2 * L, dtype=torch.float16, device=dev)
        x4 = torch.empty(B, 4, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        dy_da = (torch.empty(B, L, 2, dtype=table.dtype, device=dev)
                 if ctx.needs_input_grad[1] and enc.interp_id != 0 else None)
        _hy.grid_forward(x, ambient.detach().float().reshape(1).contiguous(), table, enc.offsets, S, enc.base_resolution,
                         enc.gridtype_id, enc.align_corners, enc.interp_id, bound, feat, x4, dy_da)
        ctx.save_for_backward(x4, table, enc.offsets, dy_da)
        ctx.geometry = (B, 4, 2, L, S, enc.base_resolution, enc.gridtype_id, enc.align_corners, enc.interp_id)
        ctx.param, ctx.bound, ctx.ambient_shape = table_param, bound, ambient.shape
        return feat

    @staticmethod
    def backward(ctx, g_feat):
        x4, table, offsets, dy_da = ctx.saved_tensors
        B, L = ctx.geometry[0], ctx.geometry[3]
        dev = g_feat.device
        g_amb = g_table = None
        if ctx.needs_input_grad[1]:
            g_amb = (torch.empty if dy_da is not None else torch.zeros)(1, dtype=torch.float32, device=dev)
        if x4 is not None or dy_da is not None:
            g_levels = torch.empty(L, B, 2, dtype=table.dtype, device=dev)
            _hy.grid_backward(g_feat.to(torch.float16).contiguous(), dy_da, 1.0 / (2.0 * ctx.bound), g_levels,
                              g_amb if dy_da is not None else None)
            if x4 is not None:
                g_table = _table_backward(ctx.param, table, g_levels, x4, offsets, ctx.geometry, {"bound": ctx.bound})[1]
        return None, (None if g_amb is None else g_amb.view(ctx.ambient_shape)), g_table, None, None


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="tiledgrid", encoding_dir="sphere_harmonics", encoding_time="frequency", encoding_bg="hashgrid",
                 num_layers=2, hidden_dim=64, geo_feat_dim=32, num_layers_color=3, hidden_dim_color=64, num_layers_bg=2,
                 hidden_dim_bg=64, num_layers_ambient=5, hidden_dim_ambient=128, ambient_dim=1, bound=1, interpolation="linear",
                 **kwargs):
        super().__init__(bound, **kwargs)
        # ambient network (dnerf/network_hyper.py:31-51)
        self.num_layers_ambient, self.hidden_dim_ambient, self.ambient_dim = num_layers_ambient, hidden_dim_ambient, ambient_dim
        self.encoder_time, self.in_dim_time = get_encoder(encoding_time, input_dim=1, multires=6)
        self.ambient_net = _mlp([self.in_dim_time] + [hidden_dim_ambient] * (num_layers_ambient - 1) + [ambient_dim])
        # density network on the (3 + ambient_dim)-dimensional grid (:53-73)
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.encoder, self.in_dim = get_encoder(encoding, input_dim=3 + ambient_dim, desired_resolution=2048 * bound,
                                                interpolation=interpolation)
        self.sigma_net = _mlp([self.in_dim] + [hidden_dim] * (num_layers - 1) + [1 + geo_feat_dim])
        # colour network (:75-94)
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
        # the constant basis e_0 of the density head (not a checkpoint key)
        self.register_buffer("_e0", F.one_hot(torch.tensor(0), BASIS).to(torch.float16), persistent=False)

    # ---- the fused route -------------------------------------------------------------------------------------------------
    fused_mlp = True  # False (test reference): the torch op sequence everywhere

    def _glue_ok(self):
        """the kernels fit this model: one ambient coordinate on a 4-D grid of 16 levels x 2 features, a 33-column density output
        (sigma + 32 features: the 64-column row of csrc/dnerf_basis.hip with 31 zero columns), SH_4 directions, a colour net the
        fused MLP entry points take, and a bound whose normalisation is exact as a multiplication"""
        e = self.encoder
        return (self.ambient_dim == 1 and type(e).__name__ == "GridEncoder" and e.input_dim == 4 and e.num_levels == 16
                and e.level_dim == 2 and self.num_layers == 2 and self.geo_feat_dim == ROW - BASIS
                and getattr(self.encoder_dir, "degree", None) == 4 and self.in_dim_dir + self.geo_feat_dim == CIN
                and self.num_layers_color == 3 and self.hidden_dim_color == 64
                and self.bound > 0 and math.frexp(2.0 * self.bound)[0] == 0.5)

    def _can_fuse(self, x):
        return (self.fused_mlp and x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and x.dtype == torch.float32
                and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16 and self._glue_ok())

    def _head_weight(self):
        """the density net's last matrix as the 64 rows the density-head kernel reads: row 0 sigma, rows 1..31 zero, rows 32..63 the
        32 feature rows.  With the basis e_0 the head's dot is fmaf(h_0, 1, 0) = h_0: sigma = exp(h_0), and the gradient of column
        0 is half(d_sigma exp(clamp(h_0))) — the reference's trunc_exp on an fp16 column"""
        w = self.sigma_net[-1].weight
        return torch.cat([w[:1], w.new_zeros(BASIS - 1, w.shape[1]), w[1:]], dim=0)

    def _pack_color(self):
        """[64 x 48 | 64 x 64 | 16 x 64]: the last matrix padded from 3 to 16 rows"""
        c0, c1, c2 = (l.weight for l in self.color_net)
        return torch.cat([c0.reshape(-1), c1.reshape(-1), F.pad(c2, (0, 0, 0, 13)).reshape(-1)])

    def _time_tensor(self, t, dev):
        if t is None:
            t = self._bound_time
            if t is None:
                raise ValueError("dnerf: forward / density need a time `t` (or run inside NeRFRenderer.run_cuda / run)")
        if not torch.is_tensor(t):
            t = torch.tensor([[float(t)]], dtype=torch.float32)
        return t.to(device=dev, dtype=torch.float32)

    def _ambient(self, t):
        """[1, ambient_dim] of the call's one time (:126-136); under autocast a half, as the reference's is"""
        return torch.tanh(_run_mlp(self.ambient_net, self.encoder_time(t.reshape(1, 1)))) * self.bound

    def _density_fused(self, x, t):
        """-> (h [Bp, 64] fp16 = [h_0 | 0 (31) | features (32)] with Bp = B rounded up to the MLP kernels' 128 rows, Bp).  The
        padding rows are points at the origin: they cost fewer than 128 rows of work and take zero gradients from the sliced
        outputs."""
        B = x.shape[0]
        Bp = (B + 127) // 128 * 128
        x = x.contiguous()
        if Bp != B:
            x = torch.cat([x, x.new_zeros(Bp - B, 3)], dim=0)
        ambient = self._ambient(t).float()  # float(half(tanh(.)) * bound): what the reference's cat promotes; stays on the device
        note_table_use(self.encoder.embeddings)
        feat = _HyperGrid.apply(x, ambient, self.encoder.embeddings, self.encoder, float(self.bound))
        hidden = F.relu(self.sigma_net[0](feat), inplace=True)
        return F.linear(hidden, self._head_weight()).to(torch.float16).contiguous(), Bp

    def _color_fused(self, h, d, B, Bp):
        d = d.float().contiguous()
        if Bp != B:
            d = torch.cat([d, d.new_zeros(Bp - B, 3)], dim=0)
        infer = not torch.is_grad_enabled()
        sigma, cin = _BasisMid.apply(h, d, self._e0)
        # 48 -> 64 -> 64 -> 16 with the rgb head: fp32 sigmoid(out[:, :3]) straight from the last layer (seal3d_hip.h: rgb_head)
        rgb = ffmlp_forward(cin, self._pack_color(), CIN, 16, 64, 2, 0, 6, infer, cin.requires_grad, None, None, 0, None, True)
        return sigma[:B], rgb[:B]

    # ---- the reference's op sequence ---------------------------------------------------------------------------------------
    def _density_torch(self, x, t):
        ambient = self._ambient(t)
        x = torch.cat([x, ambient.repeat(x.shape[0], 1)], dim=1)
        h = _run_mlp(self.sigma_net, self.encoder(x, bound=self.bound))
        return trunc_exp(h[..., 0]), h[..., 1:]

    def _rgb(self, d, geo_feat):
        return torch.sigmoid(_run_mlp(self.color_net, torch.cat([self.encoder_dir(d), geo_feat], dim=-1)))

    # ---- the model's surface -------------------------------------------------------------------------------------------------
    def forward(self, x, d, t=None):
        """x [N, 3] in [-bound, bound], d [N, 3], t [1, 1] in [0, 1] -> (sigma, rgbs, None): this model deforms nothing.  Without `t`
        (the base renderer's two-argument call inside run_cuda): the time the renderer bound for this rendering, the result is
        (sigma, rgbs), and the renderer is told that there is no deformation to regularise."""
        bound_call = t is None
        t = self._time_tensor(t, x.device)
        self._deform_reg = None
        if bound_call:
            self._deform_out = None
        # A training render under a sample budget (mean_count > 0) hands over the marcher's padded buffers and announces the
        # device-side sample count (s3d_hip.row_limit).  The density net runs on torch's Linear, which takes no row limit, so the
        # count is read back here (one host read) and the networks run on the live rows — the count rounded up to 128, exactly the
        # rows the marcher keeps when it trims; sigma and rgb go back as rows of the padded extent (dnerf/network.py does the same).
        rows_all = x.shape[0]
        nv = s3d_hip.active_row_limit(rows_all) if self.training else None
        live = rows_all if nv is None else min((max(int(nv.reshape(-1)[0]), 0) + 127) // 128 * 128, rows_all)
        if live < rows_all:
            if live == 0:
                sigma, rgbs = x.new_zeros(rows_all), x.new_zeros(rows_all, 3)
                return (sigma, rgbs) if bound_call else (sigma, rgbs, None)
            x, d = x[:live], d[:live]
        if self._can_fuse(x):
            h, Bp = self._density_fused(x, t)
            sigma, rgbs = self._color_fused(h, d, x.shape[0], Bp)
        else:
            sigma, geo_feat = self._density_torch(x, t)
            rgbs = self._rgb(d, geo_feat)
        if live < rows_all:
            sigma, rgbs = F.pad(sigma, (0, rows_all - live)), F.pad(rgbs, (0, 0, 0, rows_all - live))
        return (sigma, rgbs) if bound_call else (sigma, rgbs, None)

    def density(self, x, t=None):
        t = self._time_tensor(t, x.device)
        if self._can_fuse(x):
            h, _ = self._density_fused(x, t)
            B = x.shape[0]
            return {"sigma": _BasisMid.apply(h, None, self._e0)[:B], "geo_feat": h[:B, BASIS:]}
        sigma, geo_feat = self._density_torch(x, t)
        return {"sigma": sigma, "geo_feat": geo_feat}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        """:215-244 — `geo_feat` suffices for this model, so the sampling path (`run`) works with it"""
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
                  (self.encoder_time, lr), (self.ambient_net, lr_net)]
        if self.bg_radius > 0:
            groups += [(self.encoder_bg, lr), (self.bg_net, lr_net)]
        return [{"params": g.parameters(), "lr": r} for g, r in groups]
