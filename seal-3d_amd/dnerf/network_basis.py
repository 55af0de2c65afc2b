"""D-NeRF temporal-basis network (dnerf/network_basis.py of the reference, `main_dnerf.py --basis`): no deformation field — the
time enters through two bases from a 5 x 128 MLP on freq_6(t), evaluated on ONE row per call because `t` is [1, 1]:
(sigma_basis [32] | color_basis [8]) = basis_net(freq_6(t)), h = MLP_2x64(grid(x)) [64], sigma = trunc_exp(h[:, :32] @ sigma_basis),
rgb = sigmoid(MLP_3x64([SH_4(d) | h[:, 32:]]).view(-1, 3, 8) @ color_basis).

Two routes (DESIGN.md "D-NeRF, temporal basis"): the reference's torch op sequence (CPU, fp32, any shape), and under fp16 autocast
on the GPU the density head of csrc/dnerf_basis.hip between torch's Linear (basis net, density net) and the fused MLP entry points
(colour net).  The colour contraction costs no kernel there: one call has one time, so `color_basis` is folded into the colour
net's last weight matrix — W_eff[c] = sum_k color_basis[k] W2[8 c + k] — and the network runs as 48 -> 64 -> 64 -> 16 with the rgb
head.  Autograd through the fold carries the gradient to `color_net[2].weight` and, through `color_basis`, to `basis_net`."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

import s3d_hip
from activation import trunc_exp
from encoding import get_encoder
from ffmlp.ffmlp import ffmlp_forward
from nerf.network import _Background, _mlp, _run_mlp

from .renderer import NeRFRenderer

_bs = s3d_hip.DnerfBasisBackend
ROW, CIN, BASIS = _bs.ROW, _bs.CIN, _bs.BASIS


class _BasisMid(Function):
    """sigma = exp(half(h[:, :32] . sigma_basis)) and the colour net's input [half(SH_4(d)) | h[:, 32:]] in one kernel per direction
    (s3d_dnerf_basis_mid_forward / _backward); the backward hands `grad_sigma_basis` — a fixed-order fp32 sum over the rows — to
    autograd for the sigma_basis slice of basis_net's output.  `dirs` None: sigma alone (density())."""

    @staticmethod
    def forward(ctx, h, dirs, sigma_basis):
        B = h.shape[0]
        sb = sigma_basis.detach().to(torch.float16).reshape(-1).contiguous()
        if sb.data_ptr() % 16:
            sb = sb.clone()
        sigma = torch.empty(B, dtype=torch.float32, device=h.device)
        cin = None if dirs is None else torch.empty(B, CIN, dtype=torch.float16, device=h.device)
        _bs.mid_forward(h, dirs, sb, sigma, cin)
        ctx.save_for_backward(h, sb)
        ctx.set_materialize_grads(False)
        if cin is None:
            return sigma
        return sigma, cin

    @staticmethod
    def backward(ctx, g_sigma, g_cin=None):
        h, sb = ctx.saved_tensors
        B = h.shape[0]
        if g_cin is None:
            g_cin = torch.zeros(B, CIN, dtype=torch.float16, device=h.device)
        g_h = torch.empty_like(h)
        g_sb = torch.empty(BASIS, dtype=torch.float32, device=h.device) if ctx.needs_input_grad[2] else None
        _bs.mid_backward(g_cin.to(torch.float16).contiguous(), None if g_sigma is None else g_sigma.float().contiguous(), h, sb, g_h,
                         g_sb)
        return g_h, None, g_sb


def fold_color_basis(w2, color_basis):
    """W_eff [3, H]: W_eff[c, :] = sum_k color_basis[k] * w2[K c + k, :] — `(h @ w2.T).view(-1, 3, K) @ color_basis == h @ W_eff.T`
    exactly in real arithmetic, because one call has one time"""
    K = color_basis.shape[0]
    return torch.einsum("k,ckj->cj", color_basis, w2.view(3, K, w2.shape[1]))


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="tiledgrid", encoding_dir="sphere_harmonics", encoding_time="frequency", encoding_bg="hashgrid",
                 num_layers=2, hidden_dim=64, geo_feat_dim=32, num_layers_color=3, hidden_dim_color=64, num_layers_bg=2,
                 hidden_dim_bg=64, sigma_basis_dim=32, color_basis_dim=8, num_layers_basis=5, hidden_dim_basis=128, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        # basis network (dnerf/network_basis.py:32-53)
        self.num_layers_basis, self.hidden_dim_basis = num_layers_basis, hidden_dim_basis
        self.sigma_basis_dim, self.color_basis_dim = sigma_basis_dim, color_basis_dim
        self.encoder_time, self.in_dim_time = get_encoder(encoding_time, input_dim=1, multires=6)
        self.basis_net = _mlp([self.in_dim_time] + [hidden_dim_basis] * (num_layers_basis - 1) + [sigma_basis_dim + color_basis_dim])
        # density network (:55-75)
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.encoder, self.in_dim = get_encoder(encoding, desired_resolution=2048 * bound)
        self.sigma_net = _mlp([self.in_dim] + [hidden_dim] * (num_layers - 1) + [sigma_basis_dim + geo_feat_dim])
        # colour network (:77-96)
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        self.encoder_dir, self.in_dim_dir = get_encoder(encoding_dir)
        self.color_net = _mlp([self.in_dim_dir + geo_feat_dim] + [hidden_dim_color] * (num_layers_color - 1) + [3 * color_basis_dim])
        if self.bg_radius > 0:
            self.num_layers_bg, self.hidden_dim_bg = num_layers_bg, hidden_dim_bg
            self.encoder_bg, self.in_dim_bg = get_encoder(encoding_bg, input_dim=2, num_levels=4, log2_hashmap_size=19,
                                                          desired_resolution=2048)
            self.bg_net = _mlp([self.in_dim_bg + self.in_dim_dir] + [hidden_dim_bg] * (num_layers_bg - 1) + [3])
        else:
            self.bg_net = None

    # ---- the fused route -------------------------------------------------------------------------------------------------
    fused_mlp = True  # False (test reference): the torch op sequence everywhere

    def _glue_ok(self):
        """the row layouts of csrc/dnerf_basis.hip fit this model: a 64-column density output of 32 basis and 32 feature columns,
        SH_4 directions"""
        return (self.sigma_basis_dim == BASIS and self.sigma_basis_dim + self.geo_feat_dim == ROW
                and getattr(self.encoder_dir, "degree", None) == 4 and self.in_dim_dir + self.geo_feat_dim == CIN)

    def _can_fuse(self, x):
        return (self.fused_mlp and x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and x.dtype == torch.float32
                and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16 and self._glue_ok())

    def _color_fusable(self):
        """the colour net with the folded last matrix is a shape the fused MLP entry points take; another shape keeps the network
        on torch's Linear and the explicit contraction"""
        return self.num_layers_color == 3 and self.hidden_dim_color == 64

    def _pack_color(self, color_basis):
        """[64 x 48 | 64 x 64 | 16 x 64]: the last matrix is the fold of color_basis into color_net[2], computed in fp32 and padded
        from 3 to 16 rows"""
        c0, c1, c2 = (l.weight for l in self.color_net)
        w_eff = fold_color_basis(c2.float(), color_basis.float())
        return torch.cat([c0.reshape(-1), c1.reshape(-1), F.pad(w_eff, (0, 0, 0, 13)).reshape(-1)])

    def _time_tensor(self, t, dev):
        if t is None:
            t = self._bound_time
            if t is None:
                raise ValueError("dnerf: forward / density need a time `t` (or run inside NeRFRenderer.run_cuda / run)")
        if not torch.is_tensor(t):
            t = torch.tensor([[float(t)]], dtype=torch.float32)
        return t.to(device=dev, dtype=torch.float32)

    def _bases(self, t):
        """(sigma_basis [32], color_basis [8]) of the call's one time (:128-137)"""
        hb = _run_mlp(self.basis_net, self.encoder_time(t.reshape(1, 1)))
        return hb[0, :self.sigma_basis_dim], hb[0, self.sigma_basis_dim:]

    def _density_fused(self, x, t):
        """-> (h [Bp, 64] fp16 with Bp = B rounded up to the MLP kernels' 128 rows, sigma_basis, color_basis, Bp).  The padding rows
        are points at the origin: they cost fewer than 128 rows of work and take zero gradients from the sliced outputs."""
        B = x.shape[0]
        Bp = (B + 127) // 128 * 128
        x = x.contiguous()
        if Bp != B:
            x = torch.cat([x, x.new_zeros(Bp - B, 3)], dim=0)
        sigma_basis, color_basis = self._bases(t)
        h = _run_mlp(self.sigma_net, self.encoder(x, bound=self.bound)).to(torch.float16).contiguous()
        return h, sigma_basis, color_basis, Bp

    def _color_fused(self, h, d, sigma_basis, color_basis, B, Bp):
        d = d.float().contiguous()
        if Bp != B:
            d = torch.cat([d, d.new_zeros(Bp - B, 3)], dim=0)
        infer = not torch.is_grad_enabled()
        sigma, cin = _BasisMid.apply(h, d, sigma_basis.float())
        if self._color_fusable():
            # 48 -> 64 -> 64 -> 16 with the rgb head: fp32 sigmoid(out[:, :3]) straight from the last layer (seal3d_hip.h: rgb_head)
            rgb = ffmlp_forward(cin, self._pack_color(color_basis), CIN, 16, 64, 2, 0, 6, infer, cin.requires_grad, None, None, 0, None,
                                True)
        else:
            out = _run_mlp(self.color_net, cin)
            rgb = torch.sigmoid(out.view(-1, 3, self.color_basis_dim) @ color_basis.to(out.dtype))
        return sigma[:B], rgb[:B]

    # ---- the reference's op sequence ---------------------------------------------------------------------------------------
    def _density_torch(self, x, t):
        sigma_basis, color_basis = self._bases(t)
        h = _run_mlp(self.sigma_net, self.encoder(x, bound=self.bound))
        sigma = trunc_exp(h[..., :self.sigma_basis_dim] @ sigma_basis)
        return sigma, h[..., self.sigma_basis_dim:], color_basis

    def _rgb(self, d, geo_feat, color_basis):
        h = _run_mlp(self.color_net, torch.cat([self.encoder_dir(d), geo_feat], dim=-1))
        return torch.sigmoid(h.view(-1, 3, self.color_basis_dim) @ color_basis)

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
            h, sigma_basis, color_basis, Bp = self._density_fused(x, t)
            sigma, rgbs = self._color_fused(h, d, sigma_basis, color_basis, x.shape[0], Bp)
        else:
            sigma, geo_feat, color_basis = self._density_torch(x, t)
            rgbs = self._rgb(d, geo_feat, color_basis)
        if live < rows_all:
            sigma, rgbs = F.pad(sigma, (0, rows_all - live)), F.pad(rgbs, (0, 0, 0, rows_all - live))
        return (sigma, rgbs) if bound_call else (sigma, rgbs, None)

    def density(self, x, t=None):
        t = self._time_tensor(t, x.device)
        if self._can_fuse(x):
            h, sigma_basis, _, _ = self._density_fused(x, t)
            sigma = _BasisMid.apply(h, None, sigma_basis.float())
            B = x.shape[0]
            return {"sigma": sigma[:B], "geo_feat": h[:B, self.sigma_basis_dim:]}
        sigma, geo_feat, _ = self._density_torch(x, t)
        return {"sigma": sigma, "geo_feat": geo_feat}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        raise NotImplementedError("dnerf.network_basis: color() has no way to receive color_basis — the reference's sampling path is "
                                  "broken for this model (network_basis.py:214, asserted in main_dnerf.py:81); render with cuda_ray=True")

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
                  (self.encoder_time, lr), (self.basis_net, lr_net)]
        if self.bg_radius > 0:
            groups += [(self.encoder_bg, lr), (self.bg_net, lr_net)]
        return [{"params": g.parameters(), "lr": r} for g, r in groups]
