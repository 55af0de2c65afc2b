"""TensoRF CP (CANDECOMP/PARAFAC) backbone — counterpart of tensoRF/network_cp.py of the reference (`main_tensoRF.py --cp`).

Three line factors per component and no planes: density rank 96, colour rank 288, `basis_mat` 288 -> 27 and the colour MLP of
the vector-matrix network (FreqEncoder(27, deg 2) + FreqEncoder(3, deg 2) = 150 -> 128 -> 128 -> 3).  About 1.4 MB of factors
at resolution 300 against the VM-48 model's 69 MB.  Parameter names and shapes follow the reference (sigma_vec / color_vec
[1, R, D, 1], basis_mat, color_net), so its checkpoints load key for key.

On the GPU the three grid_sample calls + two products + sum (or basis_mat) of `get_sigma_feat` / `get_color_feat` run as one
kernel per call (`s3d_cp_features_forward` / `s3d_cp_color_forward`, csrc/tensorf_cp.hip) and their parameter gradients as one
(`s3d_cp_features_backward` / `s3d_cp_color_backward`: points sorted by 64-row line chunk, fp32 sums per cell in LDS, one global
atomic per cell and workgroup instead of one per (point, rank, tap)).  The factor gradients are NOT marked as checked: a
GradScaler reads their 1.4 MB itself.  A gradient w.r.t. the coordinates falls back to the grid_sample sequence.

The host path that drives these kernels (the two autograd Functions, the sorted-point cache, `forward` / `density`, the dispatch
of `get_sigma_feat` / `get_color_feat`) is the vector-matrix network's: tensoRF/network.py, `TensoRFCommon`.  This file holds
the parameters, the grid_sample route, the line crop / resample loops and what the shared path asks of a backbone."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import s3d_hip
from encoding import get_encoder
from nerf.renderer import NeRFRenderer
from tensoRF.network import TensoRFCommon, _ColorBasis, _Features, _MeanAbsSum


class _CpFeatures(_Features):
    pass


class _CpColorBasis(_ColorBasis):
    pass


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

    # what the shared host path (tensoRF/network.py: TensoRFCommon) asks of a backbone
    _backend, _Features, _ColorBasis = s3d_hip.CpBackend, _CpFeatures, _CpColorBasis
    _fused = property(lambda self: self.fused_cp)

    def _found_inf(self, factors, *more):
        return None  # (the line gradients are not marked as checked: a GradScaler reads their 1.4 MB itself)

    def _color_factors(self):
        return list(self.color_vec)

    @staticmethod
    def _split(factors):
        return (factors,)

    @staticmethod
    def _product_rows(lead):
        return lead[0][0].shape[1]

    def _basis_rank_ok(self):
        return self.color_rank[0] <= 512

    def _shadows(self, lines):
        """rank-fastest shadows of a line set (CpBackend.transpose_lines), taken afresh at every forward (the native optimizer
        rewrites the parameters without touching `_version`); the forward and the backward of one step share them"""
        if not getattr(self, "fused_shadows", True):
            return None
        return s3d_hip.CpBackend.transpose_lines([v.detach() for v in lines], self.resolution)

    def _use_native(self, x):
        return super()._use_native(x) and all(v.dtype == torch.float32 for v in self.sigma_vec)

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
        tl_h, br_h, min_pos, max_pos = self._occupied_box()
        for i, vec_id in enumerate(self.vec_ids):
            for vecs in (self.sigma_vec, self.color_vec):
                vecs[i] = nn.Parameter(vecs[i].data[..., tl_h[vec_id]:br_h[vec_id], :].contiguous())
        return self._cropped_to(tl_h, br_h, min_pos, max_pos)
