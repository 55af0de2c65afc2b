"""TensoRF CP (CANDECOMP/PARAFAC) backbone — counterpart of tensoRF/network_cp.py of the reference (`main_tensoRF.py --cp`).

Three line factors per component and no planes: density rank 96, colour rank 288, `basis_mat` 288 -> 27 and the colour MLP of
the vector-matrix network (FreqEncoder(27, deg 2) + FreqEncoder(3, deg 2) = 150 -> 128 -> 128 -> 3).  About 1.4 MB of factors
at resolution 300 against the VM-48 model's 69 MB.  Parameter names and shapes follow the reference (sigma_vec / color_vec
[1, R, D, 1], basis_mat, color_net), so its checkpoints load key for key.

On the GPU the three grid_sample calls + two products + sum (or basis_mat) of `get_sigma_feat` / `get_color_feat` run as one
kernel per call (`s3d_cp_features_forward` / `s3d_cp_color_forward`, csrc/tensorf_cp.hip) and their parameter gradients as one
(`s3d_cp_features_backward` / `s3d_cp_color_backward`: points sorted by 64-row line chunk, fp32 sums per cell in LDS, one global
atomic per cell and workgroup instead of one per (point, rank, tap)).  The factor gradients are NOT marked as checked: a
GradScaler reads their 1.4 MB itself.  A gradient w.r.t. the coordinates falls back to the grid_sample sequence."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import s3d_hip
from activation import trunc_exp
from encoding import get_encoder
from nerf.renderer import NeRFRenderer
from tensoRF.network import TensoRFCommon, _linear, _MeanAbsSum


def _shadows(net, lines):
    """rank-fastest shadows of a line set (CpBackend.transpose_lines), taken afresh at every forward (the native optimizer
    rewrites the parameters without touching `_version`); the forward and the backward of one step share them"""
    if not getattr(net, "fused_shadows", True):
        return None
    return s3d_hip.CpBackend.transpose_lines([v.detach() for v in lines], net.resolution)


def _bins(net, x, n_valid=None):
    """the points of x sorted by line chunk (CpBackend.backward_bins): x and the resolution decide it, so the density and the
    colour features of one forward share the sort.  Kept on the network, keyed by the storage of x, dropped after two uses or at
    the next forward (tensoRF/network.py: _bins)."""
    cache = net.__dict__.setdefault("_cp_bins", {})
    key = (x.data_ptr(), x._version, x.shape[0], tuple(net.resolution), None if n_valid is None else n_valid.data_ptr())
    if key not in cache:
        if len(cache) >= 4:
            cache.clear()
        cache[key] = [x, s3d_hip.CpBackend.backward_bins(x, net.resolution, n_valid), 2]
    ent = cache[key]
    ent[2] -= 1
    if ent[2] <= 0:
        del cache[key]
    return ent[1]


def _torch_backward(ctx, fn, x, lines, g, reduce, extra=()):
    """the reference's op sequence re-run under autograd (a gradient for the coordinates was asked for)"""
    if ctx.nv is not None:  # (the torch route sums over every row: the absent ones hold anything)
        live = torch.arange(x.shape[0], device=x.device) < (ctx.nv.reshape(-1)[:1] + 127) // 128 * 128
        g = torch.where(live if reduce else live.unsqueeze(0), g, torch.zeros((), dtype=g.dtype, device=g.device))
    with torch.enable_grad():
        leaves = [v.detach().requires_grad_(True) for v in lines]
        xin = x.detach().requires_grad_(True)
        out = fn(xin, leaves)
        grads = torch.autograd.grad(out, [xin] + leaves, g.contiguous())
    return grads[0], grads[1:]


class _CpFeatures(torch.autograd.Function):
    """forward: one HIP kernel; backward: the chunk-binned HIP kernel for the line gradients"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)  # grid_sample is an fp32 op under autocast too
    def forward(ctx, x, net, reduce, *lines):
        x = x.contiguous()
        N = x.shape[0]
        out = torch.empty((N,) if reduce else (lines[0].shape[1], N), dtype=torch.float32, device=x.device)
        nv = s3d_hip.active_row_limit(N)  # (padded sample batch: rows behind the device-side count are absent)
        sh = _shadows(net, lines)
        s3d_hip.CpBackend.features_forward(x, [v.contiguous() for v in lines], net.resolution, reduce, out, n_valid=nv, shadows=sh)
        ctx.save_for_backward(x, *lines)
        ctx.net, ctx.reduce, ctx.nv, ctx.sh = net, reduce, nv, sh
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, *lines = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            g = g if ctx.reduce else g.t()  # [R, N] gradient of the `.T` consumer: point-major underneath
            gl = s3d_hip.CpBackend.features_backward(x, [v.contiguous() for v in lines], ctx.net.resolution, ctx.reduce,
                                                     g.float().contiguous(), _bins(ctx.net, x, ctx.nv), None, n_valid=ctx.nv,
                                                     shadows=ctx.sh)
            return (None, None, None) + tuple(gl)
        fn = ctx.net._sigma_feat_torch if ctx.reduce else ctx.net._color_prod_torch
        gx, gl = _torch_backward(ctx, fn, x, lines, g, ctx.reduce)
        return (gx, None, None) + tuple(gl)


class _CpColorBasis(torch.autograd.Function):
    """basis_mat(vec_feat.T) of tensoRF/network_cp.py:105-109 in ONE kernel per direction (s3d_cp_color_forward / _backward): the
    [288, N] products never leave the chip.  Arithmetic of the fp16 autocast Linear: operands rounded to binary16, fp32
    accumulation, binary16 output."""

    @staticmethod
    def forward(ctx, x, net, weight, *lines):
        x = x.float().contiguous()
        lines_c = [v.float().contiguous() for v in lines]
        w16 = weight.detach().to(torch.float16).contiguous()
        out = torch.empty(x.shape[0], w16.shape[0], dtype=torch.float16, device=x.device)
        nv = s3d_hip.active_row_limit(x.shape[0])
        sh = _shadows(net, lines_c)
        s3d_hip.CpBackend.color_forward(x, lines_c, net.resolution, w16, out, n_valid=nv, shadows=sh)
        ctx.save_for_backward(x, w16, *lines)
        ctx.net, ctx.nv, ctx.sh = net, nv, sh
        return out

    @staticmethod
    def backward(ctx, g):
        x, w16, *lines = ctx.saved_tensors
        # (g as it arrives: a [:, :27] view of _MlpInput's zero-padded [N, 32] gradient is used in place, anything else is padded)
        gl, gw = s3d_hip.CpBackend.color_backward(x, [v.float().contiguous() for v in lines], ctx.net.resolution, w16,
                                                  g.to(torch.float16), _bins(ctx.net, x, ctx.nv), None, n_valid=ctx.nv, shadows=ctx.sh)
        return (None, None, gw) + tuple(gl)


class NeRFNetwork(TensoRFCommon, NeRFRenderer):
    def __init__(self, resolution=(128, 128, 128), sigma_rank=(96, 96, 96), color_rank=(288, 288, 288), color_feat_dim=27,
                 num_layers=3, hidden_dim=128, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        # (main_tensoRF.py:86 of the reference asserts the same before it builds the model)
        assert self.bg_radius <= 0, "background model is not implemented for --cp"
        self.resolution = list(resolution)
        self.sigma_rank, self.color_rank, self.color_feat_dim = list(sigma_rank), list(color_rank), color_feat_dim
        for name, rank in (("sigma_rank", self.sigma_rank), ("color_rank", self.color_rank)):
            if len(set(rank)) != 1:  # (the reference multiplies [R, N] tensors and sizes basis_mat by color_rank[0])
                raise ValueError(f"CP backbone: the three entries of {name} must be equal, got {rank}")
        self.mat_ids = [[0, 1], [0, 2], [1, 2]]
        self.vec_ids = [2, 1, 0]
        self.sigma_vec = self.init_one_svd(self.sigma_rank, self.resolution)
        self.color_vec = self.init_one_svd(self.color_rank, self.resolution)
        self.basis_mat = nn.Linear(self.color_rank[0], color_feat_dim, bias=False)
        self.num_layers, self.hidden_dim = num_layers, hidden_dim
        self.encoder, enc_dim = get_encoder("frequency", input_dim=color_feat_dim, multires=2)
        self.encoder_dir, enc_dim_dir = get_encoder("frequency", input_dim=3, multires=2)
        self.in_dim = enc_dim + enc_dim_dir
        dims = [self.in_dim] + [hidden_dim] * (num_layers - 1) + [3]
        self.color_net = nn.ModuleList([nn.Linear(i, o, bias=False) for i, o in zip(dims[:-1], dims[1:])])

    def __getstate__(self):
        """copy.deepcopy and pickling leave the backward's sorted-point cache behind"""
        state = self.__dict__.copy()
        state.pop("_cp_bins", None)
        state.pop("_l1_inv", None)
        state.pop("_s3d_found_inf", None)
        return state

    def init_one_svd(self, n_component, resolution, scale=0.2):
        return nn.ParameterList([nn.Parameter(scale * torch.randn((1, n_component[i], resolution[vec_id], 1)))  # [1, R, D, 1]
                                 for i, vec_id in enumerate(self.vec_ids)])

    fused_cp = True  # tests / A-B runs: False = the reference's grid_sample sequence on the GPU too

    def _line_feats(self, x, vecs):
        N = x.shape[0]
        coord = torch.stack([x[..., i] for i in self.vec_ids])
        coord = torch.stack((torch.zeros_like(coord), coord), dim=-1).view(3, -1, 1, 2)  # fake 2-D coordinates
        # (coord[i:i + 1], not the reference's coord[[i]]: the same rows without an index tensor copied from the host, which a
        #  graph capture does not permit)
        return [F.grid_sample(vecs[i], coord[i:i + 1], align_corners=True).view(-1, N) for i in range(3)]

    def _color_prod_torch(self, x, vecs):
        a, b, c = self._line_feats(x, vecs)
        return a * b * c  # [R, N]

    def _sigma_feat_torch(self, x, vecs):
        return torch.sum(self._color_prod_torch(x, vecs), dim=0)

    def _use_native(self, x):
        return self.fused_cp and x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and all(v.dtype == torch.float32 for v in self.sigma_vec)

    def get_sigma_feat(self, x):
        if self._use_native(x):
            return _CpFeatures.apply(x, self, True, *self.sigma_vec)
        return self._sigma_feat_torch(x, self.sigma_vec)

    fused_basis = True  # A-B runs: False = the products through HBM and basis_mat as an nn.Linear

    def get_color_feat(self, x):
        if self._use_native(x):
            if (self.fused_basis and not x.requires_grad and self.basis_mat.bias is None and self.basis_mat.out_features <= 32
                    and self.color_rank[0] <= 512 and torch.is_autocast_enabled("cuda")
                    and torch.get_autocast_dtype("cuda") == torch.float16):
                return _CpColorBasis.apply(x, self, self.basis_mat.weight, *self.color_vec)
            return _linear(self.basis_mat, _CpFeatures.apply(x, self, False, *self.color_vec).T)
        return _linear(self.basis_mat, self._color_prod_torch(x, self.color_vec).T)

    def _normalize(self, x):
        if (self.fused_cp and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and not x.requires_grad
                and self.aabb_train.is_cuda and self.aabb_train.dtype == torch.float32):
            out = torch.empty_like(x)  # (one launch instead of five, the same operations in the same order)
            s3d_hip.VmBackend.aabb_normalize(x, self.aabb_train.contiguous(), out)
            return out
        return 2 * (x - self.aabb_train[:3]) / (self.aabb_train[3:] - self.aabb_train[:3]) - 1

    def _colors(self, cf, d):
        if self._fused_mlp_ok(cf, d.requires_grad):
            return self._color_mlp_fused(cf, d)
        h = torch.cat([self.encoder(cf), self.encoder_dir(d)], dim=-1)
        for k, layer in enumerate(self.color_net):
            h = _linear(layer, h)
            if k != self.num_layers - 1:
                h = F.relu(h, inplace=True)
        return torch.sigmoid(h)

    def forward(self, x, d):
        x = self._normalize(x)
        self.__dict__["_cp_bins"] = {}  # (the previous forward's sorted points)
        sigma = trunc_exp(self.get_sigma_feat(x))
        return sigma, self._colors(self.get_color_feat(x), d)

    def density(self, x):
        return {"sigma": trunc_exp(self.get_sigma_feat(self._normalize(x)))}

    def color(self, x, d, mask=None, **kwargs):
        """masked inference (tensoRF/network_cp.py:156-189): colours where `mask` is set, zeros elsewhere"""
        x = self._normalize(x)
        if mask is not None:
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            x, d = x[mask], d[mask]
        h = self._colors(self.get_color_feat(x), d)
        if mask is None:
            return h
        rgbs[mask] = h.to(rgbs.dtype)
        return rgbs

    def density_factors(self):
        """the density factors the L1 term covers (tensoRF/utils.py: _regularizer)"""
        return list(self.sigma_vec)

    fused_l1 = True  # tests / A-B runs: False = the reference's op-by-op expression

    def density_loss(self):
        """L1 penalty on the density lines (tensoRF/network_cp.py:193-197): sum_i mean|sigma_vec[i]|"""
        if self.fused_l1:
            return _MeanAbsSum.apply(*self.sigma_vec)
        loss = 0
        for v in self.sigma_vec:
            loss = loss + torch.mean(torch.abs(v))
        return loss

    def get_params(self, lr1, lr2=None):
        lr2 = lr1 if lr2 is None else lr2
        return [{"params": self.sigma_vec, "lr": lr1}, {"params": self.color_vec, "lr": lr1},
                {"params": self.basis_mat.parameters(), "lr": lr2}, {"params": self.color_net.parameters(), "lr": lr2}]

    @torch.no_grad()
    def upsample_model(self, resolution):
        """linear re-sampling of all lines to a new resolution (tensoRF/network_cp.py:200-212)"""
        for vecs in (self.sigma_vec, self.color_vec):
            for i, vec_id in enumerate(self.vec_ids):
                vecs[i] = nn.Parameter(F.interpolate(vecs[i].data, size=(resolution[vec_id], 1), mode="bilinear", align_corners=True))
        self.resolution = list(resolution)

    @torch.no_grad()
    def shrink_model(self):
        """crop aabb_train and every line to the bounding box of the occupied cells of the coarsest density grid
        (tensoRF/network_cp.py:214-246).  Returns (tl, br): the kept index range per axis.  The parameter set changes:
        re-create the optimizer afterwards (Trainer.rebuild_optimizer), as after upsample_model."""
        import raymarching
        hgs = self.bound / self.grid_size
        thresh = min(self.density_thresh, self.mean_density)
        occupied = self.density_grid[self.cascade - 1] > thresh
        pos = raymarching.morton3D_invert(torch.nonzero(occupied).squeeze(-1))
        if pos.shape[0] == 0:
            raise RuntimeError("shrink_model: no cell of the coarsest cascade is above the density threshold")
        pos = (2 * pos / (self.grid_size - 1) - 1) * (self.bound - hgs)
        min_pos, max_pos = pos.amin(0) - hgs, pos.amax(0) + hgs
        reso = torch.tensor(self.resolution, dtype=torch.long, device=self.aabb_train.device)
        units = (self.aabb_train[3:] - self.aabb_train[:3]) / reso
        tl = torch.round((min_pos - self.aabb_train[:3]) / units).long().clamp(min=0)
        br = torch.minimum(torch.round((max_pos - self.aabb_train[:3]) / units).long(), reso)
        tl_h, br_h = tl.tolist(), br.tolist()
        for i, vec_id in enumerate(self.vec_ids):
            for vecs in (self.sigma_vec, self.color_vec):
                vecs[i] = nn.Parameter(vecs[i].data[..., tl_h[vec_id]:br_h[vec_id], :].contiguous())
        self.aabb_train = torch.cat([min_pos, max_pos], dim=0).to(self.aabb_train.dtype)
        # (the reference leaves `self.resolution` stale after the crop; the fused kernels take the line extents from it)
        self.resolution = [b - a for a, b in zip(tl_h, br_h)]
        return tl_h, br_h
