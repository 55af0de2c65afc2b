"""CCNeRF backbone (rank-residual TensoRF) — counterpart of tensoRF/network_cc.py of the reference (`main_CCNeRF.py`).

The radiance field is a sum of vector components (three lines with one rank index, `l0[r] * l1[r] * l2[r]`) and matrix
components (three planes with one rank index, `P01[r] * P02[r] * P12[r]`), each behind a matrix S: one row for the density head,
3 * degree^2 rows — the SH coefficients of the three colour channels — for the colour head.  The components are cut into K groups
(the rank lists are cumulative: `np.diff` gives the group sizes, an empty group owns no parameters), and in training the network
returns the output of every prefix of groups: sigma [K, M], rgb [K, M, 3].  The renderer composites each level and the loss is the
mean over levels (nerf/renderer.py, nerf/trainer.py), so that the trained model can be cut to any prefix afterwards
(`finalize`, `compress`) and trained objects can be placed together in one scene (`compose`, inference only).

Unlike the vector-matrix and CP backbones every factor is sampled with `align_corners=False`: the cell is
p = ((u + 1) * D - 1) / 2, a point up to one cell outside [-1, 1] still reads a value.

Parameter names and shapes follow the reference (U_vec_density / S_vec_density / U_mat_density / S_mat_density / U_vec / S_vec /
U_mat / S_mat), so its state dicts load strictly.

On the GPU the grid_sample calls, the products, the S matmuls, the level sums and the SH contraction of one head run as one
kernel per direction (`s3d_cc_features_*` / `s3d_cc_color_*`, csrc/tensorf_cc.hip; the contract is in include/seal3d_hip.h).  A
gradient w.r.t. the coordinates or directions, a degree above 4, ranks the kernels do not cover and CPU tensors take the
grid_sample sequence.  From TensoRFCommon (tensoRF/network.py) come the normalisation, the occupied box of shrink_model, the
value of the L1 term for the trainer whose optimizer forms its gradient, and the copy / pickle rules.

One extension: in eval mode `forward(x, d, K=k)` / `density(x, K=k)` with k > 0 return the first k groups' output (the reference
raises there) — the preview of a compression level without `compress()`."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import s3d_hip
from activation import trunc_exp
from encoding import get_encoder
from nerf.renderer import NeRFRenderer
from tensoRF.network import TensoRFCommon, _MeanAbsSum

MAT_IDS = [[0, 1], [0, 2], [1, 2]]
VEC_IDS = [2, 1, 0]


def _flatten(groups):
    """(flat tensor list, layout) of a group list; layout[k] = (has vector component, has matrix component)"""
    flat, layout = [], []
    for lines, planes, s_vec, s_mat in groups:
        layout.append((lines is not None, planes is not None))
        if lines is not None:
            flat += list(lines) + [s_vec]
        if planes is not None:
            flat += list(planes) + [s_mat]
    return flat, tuple(layout)


def _unflatten(flat, layout):
    groups, it = [], iter(flat)
    for has_vec, has_mat in layout:
        lines = [next(it) for _ in range(3)] if has_vec else None
        s_vec = next(it) if has_vec else None
        planes = [next(it) for _ in range(3)] if has_mat else None
        s_mat = next(it) if has_mat else None
        groups.append((lines, planes, s_vec, s_mat))
    return groups


def _resolution_of(groups):
    """the factor extents per axis, read off the factors themselves (a composed object brings its own)"""
    res = [None] * 3
    for lines, planes, _, _ in groups:
        if lines is not None:
            for i, vec_id in enumerate(VEC_IDS):
                res[vec_id] = lines[i].shape[2]
        if planes is not None:
            for i, (m0, m1) in enumerate(MAT_IDS):
                res[m0], res[m1] = planes[i].shape[3], planes[i].shape[2]
    return res


class _CcHead(torch.autograd.Function):
    """one head of the network (density: dirs None, degree 0; colour: SH-contracted logits) on the fused kernels: forward one
    launch, parameter gradients one launch"""

    @staticmethod
    def forward(ctx, x, dirs, degree, residual, half, layout, *flat):
        x = x.float().contiguous()
        dirs = None if dirs is None else dirs.float().contiguous()
        groups = _unflatten([t.detach().contiguous() for t in flat], layout)
        res = _resolution_of(groups)
        N = x.shape[0]
        shape = (len(groups) if residual else 1, N) + ((3,) if degree else ())
        nv = s3d_hip.active_row_limit(N)
        # (rows behind a device-side count are not written: they are zero here, since torch ops downstream read whole tensors)
        out = torch.empty(shape, dtype=torch.float32, device=x.device) if nv is None else torch.zeros(shape, dtype=torch.float32, device=x.device)
        s3d_hip.CcBackend.forward(x, dirs, groups, res, degree, residual, half, out, n_valid=nv)
        ctx.save_for_backward(x, dirs, *flat)
        ctx.spec = (degree, residual, half, layout, res, nv)
        return out

    @staticmethod
    def backward(ctx, g):
        x, dirs, *flat = ctx.saved_tensors
        degree, residual, half, layout, res, nv = ctx.spec
        groups = _unflatten([t.detach().contiguous() for t in flat], layout)
        grads = s3d_hip.CcBackend.backward(x, dirs, groups, res, degree, residual, half, g.float().contiguous(), None, n_valid=nv)
        return (None,) * 6 + tuple(_flatten(grads)[0])


class NeRFNetwork(TensoRFCommon, NeRFRenderer):
    rank_residual = True  # (what a trainer asks: the training output has a leading level axis)

    def __init__(self, resolution=(128, 128, 128), degree=4, rank_vec_density=(64, 64, 64, 64, 64), rank_mat_density=(0, 4, 8, 12, 16),
                 rank_vec=(64, 64, 64, 64, 64), rank_mat=(0, 4, 16, 32, 64), bg_resolution=(512, 512), bg_rank=8, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        self.resolution = list(resolution)
        self.degree = degree
        self.encoder_dir, self.enc_dir_dim = get_encoder("sphere_harmonics", degree=degree)
        self.out_dim = 3 * self.enc_dir_dim
        ranks = [list(int(r) for r in v) for v in (rank_vec_density, rank_mat_density, rank_vec, rank_mat)]
        if len({len(v) for v in ranks}) != 1:
            raise ValueError("CCNeRF: the four rank lists must have one entry per group")
        # one entry per object: a composed scene appends the other objects' lists (compose)
        self.rank_vec_density, self.rank_mat_density, self.rank_vec, self.rank_mat = ([v] for v in ranks)
        self.K = [len(ranks[0])]
        self.group_vec_density, self.group_mat_density, self.group_vec, self.group_mat = ([np.diff(v, prepend=0)] for v in ranks)
        self.mat_ids, self.vec_ids = MAT_IDS, VEC_IDS
        self.U_vec_density, self.S_vec_density = self._new_component(self.group_vec_density[0], 1, lines=True)
        self.U_mat_density, self.S_mat_density = self._new_component(self.group_mat_density[0], 1, lines=False)
        self.U_vec, self.S_vec = self._new_component(self.group_vec[0], self.out_dim, lines=True)
        self.U_mat, self.S_mat = self._new_component(self.group_mat[0], self.out_dim, lines=False)
        self.finalized = self.K[0] == 1
        if self.bg_radius > 0:
            self.bg_resolution, self.bg_rank = list(bg_resolution), bg_rank
            self.bg_mat = nn.Parameter(0.2 * torch.randn((1, bg_rank, bg_resolution[0], bg_resolution[1])))  # [1, R, H, W]
            self.bg_S = nn.Parameter(nn.init.kaiming_normal_(torch.ones(self.out_dim, bg_rank)))

    def _new_component(self, group_sizes, rows, lines, scale=0.2):
        """(U, S) of one component: per non-empty group three factors [1, r, D, 1] / [1, r, H, W] and S [rows, r]"""
        U, S = nn.ParameterList(), nn.ParameterList()
        res = self.resolution
        for r in group_sizes:
            r = int(r)
            if r <= 0:
                continue
            for i in range(3):
                shape = (1, r, res[VEC_IDS[i]], 1) if lines else (1, r, res[MAT_IDS[i][1]], res[MAT_IDS[i][0]])
                U.append(nn.Parameter(scale * torch.randn(shape)))
            S.append(nn.Parameter(nn.init.kaiming_normal_(torch.ones(rows, r))))
        return U, S

    # ------------------------------------------------------------------ the groups of one head
    def _groups(self, density, K=-1, oid=0):
        """the first K groups (all: K <= 0) of object `oid` as (lines, planes, s_vec, s_mat) tuples; in a composed scene every
        object is finalized and owns entry `oid` of each list (tensoRF/network_cc.py:150-173 of the reference)"""
        if density:
            Uv, Sv, Um, Sm, gv, gm = self.U_vec_density, self.S_vec_density, self.U_mat_density, self.S_mat_density, self.group_vec_density, self.group_mat_density
        else:
            Uv, Sv, Um, Sm, gv, gm = self.U_vec, self.S_vec, self.U_mat, self.S_mat, self.group_vec, self.group_mat
        K = self.K[oid] if K <= 0 else min(K, self.K[oid])
        ov = om = oid
        groups = []
        for k in range(K):
            lines = planes = s_vec = s_mat = None
            if gv[oid][k]:
                lines, s_vec = [Uv[3 * ov + i] for i in range(3)], Sv[ov]
                ov += 1
            if gm[oid][k]:
                planes, s_mat = [Um[3 * om + i] for i in range(3)], Sm[om]
                om += 1
            groups.append((lines, planes, s_vec, s_mat))
        return groups

    @staticmethod
    def _levels_torch(x, groups, residual):
        """the grid_sample sequence (tensoRF/network_cc.py:128-250): [K, N, rows] (residual) or [N, rows]"""
        N = x.shape[0]
        vec_coord = torch.stack([x[..., i] for i in VEC_IDS])
        vec_coord = torch.stack((torch.zeros_like(vec_coord), vec_coord), dim=-1).view(3, -1, 1, 2)
        mat_coord = torch.stack([x[..., ids] for ids in MAT_IDS]).view(3, -1, 1, 2)
        levels, last = [], None
        for lines, planes, s_vec, s_mat in groups:
            y = 0
            if lines is not None:
                a, b, c = (F.grid_sample(lines[i], vec_coord[i:i + 1], align_corners=False).view(-1, N) for i in range(3))
                y = y + s_vec @ (a * b * c)
            if planes is not None:
                a, b, c = (F.grid_sample(planes[i], mat_coord[i:i + 1], align_corners=False).view(-1, N) for i in range(3))
                y = y + s_mat @ (a * b * c)
            if last is not None:
                y = y + last
            levels.append(y)
            last = y
        if residual:
            return torch.stack(levels, dim=0).permute(0, 2, 1).contiguous()
        return last.permute(1, 0).contiguous()

    fused_cc = True  # tests / A-B runs: False = the reference's grid_sample sequence on the GPU too
    _fused = property(lambda self: self.fused_cc)

    def _head(self, x, d, groups, residual):
        """density (d None): the levels' features [K_out, N]; colour: the SH-contracted logits [K_out, N, 3].  K_out = the
        number of groups (residual) or 1."""
        degree = 0 if d is None else self.degree
        if (self._use_native(x) and not x.requires_grad and (d is None or (d.is_cuda and not d.requires_grad))
                and s3d_hip.CcBackend.refusal(groups, degree) is None):
            half = torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16
            flat, layout = _flatten(groups)
            with torch.autocast("cuda", enabled=False):
                return _CcHead.apply(x, d, degree, bool(residual), bool(half), layout, *flat)
        h = self._levels_torch(x, groups, residual)
        if not residual:
            h = h.unsqueeze(0)
        if d is None:
            return h.squeeze(-1)
        N = x.shape[0]
        enc_d = self.encoder_dir(d)  # [N, degree^2]
        return (h.view(h.shape[0], N, 3, self.degree ** 2) * enc_d.unsqueeze(1)).sum(-1)

    # ------------------------------------------------------------------ forward / density
    def normalize_coord(self, x, oid=0):
        if oid == 0:
            return self._normalize(x)
        tr = getattr(self, f"T_{oid}")  # [4, 4]: world -> the object's frame
        x = (torch.cat([x, torch.ones_like(x[:, :1])], dim=1) @ tr.T)[:, :3]
        aabb = getattr(self, f"aabb_{oid}")
        return 2 * (x - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1

    def normalize_dir(self, d, oid=0):
        return d if oid == 0 else d @ getattr(self, f"R_{oid}").T

    def forward(self, x, d, K=-1):
        """x [N, 3] in [-bound, bound], d [N, 3] unit.  Training: sigma [K, N], rgb [K, N, 3] (every prefix of the first K
        groups); eval: sigma [N], rgb [1, N, 3] (all groups, or the first K)."""
        if len(self.K) == 1:
            xm = self.normalize_coord(x)
            sigma = trunc_exp(self._head(xm, None, self._groups(True, K), self.training))
            rgb = torch.sigmoid(self._head(xm, d, self._groups(False, K), self.training))
            return (sigma if self.training else sigma[0]), rgb
        # a composed scene (inference only): object by object, the logits blended by the softmax of the detached densities
        sigmas, logits, sigma_all = [], [], 0
        for oid in range(1, len(self.K)):
            xm = self.normalize_coord(x, oid)
            sigma = trunc_exp(self._head(xm, None, self._groups(True, -1, oid), False))[0]
            sigmas.append(sigma.detach().clone())
            sigma_all = sigma_all + sigma
            logits.append(self._head(xm, self.normalize_dir(d, oid).contiguous(), self._groups(False, -1, oid), False)[0])
        ws = F.softmax(torch.stack(sigmas, dim=0), dim=0)  # [O, N]
        rgb = 0
        for w, h in zip(ws, logits):
            rgb = rgb + h * w.unsqueeze(-1)
        return sigma_all, torch.sigmoid(rgb)

    def density(self, x, K=-1):
        if len(self.K) == 1:
            return {"sigma": trunc_exp(self._head(self.normalize_coord(x), None, self._groups(True, K), False))[0]}
        sigma_all = 0
        for oid in range(1, len(self.K)):
            sigma_all = sigma_all + trunc_exp(self._head(self.normalize_coord(x, oid), None, self._groups(True, -1, oid), False))[0]
        return {"sigma": sigma_all}

    def background(self, x, d):
        """x [N, 2]: the ray's sphere coordinates in [-1, 1]; the torch sequence (no kernel for this backbone's background)"""
        N = x.shape[0]
        h = F.grid_sample(self.bg_mat, x.view(1, N, 1, 2), align_corners=False).view(-1, N)  # [R, N]
        h = (self.bg_S @ h).T.contiguous().view(N, 3, -1)
        return torch.sigmoid((h * self.encoder_dir(d).unsqueeze(1)).sum(-1))

    # ------------------------------------------------------------------ regulariser, optimizer groups
    def density_factors(self):
        """the density factors the L1 term covers (tensoRF/utils.py: _regularizer)"""
        return list(self.U_vec_density) + list(self.U_mat_density)

    fused_l1 = True  # tests / A-B runs: False = the reference's op-by-op expression

    def density_loss(self):
        """L1 penalty (tensoRF/network_cc.py:384-390): sum over the density lines and planes of mean|U|"""
        if self.fused_l1:
            return _MeanAbsSum.apply(*self.density_factors())
        loss = 0
        for u in self.density_factors():
            loss = loss + torch.mean(torch.abs(u))
        return loss

    def get_params(self, lr1, lr2=None):
        lr2 = lr1 if lr2 is None else lr2
        params = [{"params": self.U_vec_density, "lr": lr1}, {"params": self.S_vec_density, "lr": lr2},
                  {"params": self.U_mat_density, "lr": lr1}, {"params": self.S_mat_density, "lr": lr2},
                  {"params": self.U_vec, "lr": lr1}, {"params": self.S_vec, "lr": lr2},
                  {"params": self.U_mat, "lr": lr1}, {"params": self.S_mat, "lr": lr2}]
        if self.bg_radius > 0:
            params += [{"params": self.bg_mat, "lr": lr1}, {"params": self.bg_S, "lr": lr2}]
        return params

    # ------------------------------------------------------------------ resolution schedule
    def _line_lists(self):
        return (self.U_vec_density, self.U_vec)

    def _plane_lists(self):
        return (self.U_mat_density, self.U_mat)

    @torch.no_grad()
    def upsample_model(self, resolution):
        """bilinear re-sampling of all factors (align_corners=False) to a new resolution (tensoRF/network_cc.py:394-415)"""
        for U in self._line_lists():
            for i in range(len(U)):
                U[i] = nn.Parameter(F.interpolate(U[i].data, size=(resolution[VEC_IDS[i % 3]], 1), mode="bilinear", align_corners=False))
        for U in self._plane_lists():
            for i in range(len(U)):
                m0, m1 = MAT_IDS[i % 3]
                U[i] = nn.Parameter(F.interpolate(U[i].data, size=(resolution[m1], resolution[m0]), mode="bilinear", align_corners=False))
        self.resolution = list(resolution)

    @torch.no_grad()
    def shrink_model(self):
        """crop aabb_train and every factor to the bounding box of the occupied cells of the coarsest density grid
        (tensoRF/network_cc.py:417-459).  Returns (tl, br).  The parameter set changes: re-create the optimizer afterwards."""
        tl, br, min_pos, max_pos = self._occupied_box()
        for U in self._line_lists():
            for i in range(len(U)):
                a = VEC_IDS[i % 3]
                U[i] = nn.Parameter(U[i].data[..., tl[a]:br[a], :].contiguous())
        for U in self._plane_lists():
            for i in range(len(U)):
                m0, m1 = MAT_IDS[i % 3]
                U[i] = nn.Parameter(U[i].data[..., tl[m1]:br[m1], tl[m0]:br[m0]].contiguous())
        return self._cropped_to(tl, br, min_pos, max_pos)

    # ------------------------------------------------------------------ finalize / compress / compose
    @staticmethod
    @torch.no_grad()
    def _fuse_groups(U, S):
        """the ranks of every group sorted by importance (|S| column sum times the three factors' norms, most important first),
        then all groups concatenated along the rank axis: one group"""
        if len(U) == 0 or len(S) == 0:
            return nn.ParameterList(), nn.ParameterList()
        Us, Ss = [[], [], []], []
        for k in range(len(S)):
            importance = S[k].abs().sum(0)
            for j in range(3):
                importance = importance * U[3 * k + j].view(importance.shape[0], -1).norm(dim=-1)
            order = torch.argsort(importance, descending=True)
            Ss.append(S[k].data[:, order])
            for j in range(3):
                Us[j].append(U[3 * k + j].data[:, order])
        return (nn.ParameterList([nn.Parameter(torch.cat(u, dim=1)) for u in Us]),
                nn.ParameterList([nn.Parameter(torch.cat(Ss, dim=1))]))

    def _components(self):
        return (("U_vec_density", "S_vec_density", "rank_vec_density", "group_vec_density"),
                ("U_mat_density", "S_mat_density", "rank_mat_density", "group_mat_density"),
                ("U_vec", "S_vec", "rank_vec", "group_vec"), ("U_mat", "S_mat", "rank_mat", "group_mat"))

    @torch.no_grad()
    def finalize(self):
        """fuse all groups into one (faster inference, the precondition of compress / compose); rank-residual training ends"""
        for u, s, rank, group in self._components():
            U, S = self._fuse_groups(getattr(self, u), getattr(self, s))
            setattr(self, u, U)
            setattr(self, s, S)
            getattr(self, rank)[0] = [getattr(self, rank)[0][-1]]
            getattr(self, group)[0] = getattr(self, rank)[0]
        self.K[0] = 1
        self.finalized = True

    @torch.no_grad()
    def compress(self, ranks):
        """keep the `ranks` = (density vec, density mat, colour vec, colour mat) most important ranks of a finalized model"""
        if not self.finalized:
            self.finalize()
        for (u, s, rank, group), r in zip(self._components(), ranks):
            r = int(r)
            U, S = getattr(self, u), getattr(self, s)
            if r == 0:
                setattr(self, u, nn.ParameterList())
                setattr(self, s, nn.ParameterList())
            else:
                # (clone: a slice would keep the whole storage alive, and a saved checkpoint its full size)
                S[0] = nn.Parameter(S[0].data[:, :r].clone())
                for i in range(3):
                    U[i] = nn.Parameter(U[i].data[:, :r].clone())
            getattr(self, rank)[0] = [r]
            getattr(self, group)[0] = getattr(self, rank)[0]

    @torch.no_grad()
    def compose(self, other, R=None, s=None, t=None):
        """place `other` into this scene, rotated by R [3, 3], scaled by s and translated by t [3] (first scale and rotate, then
        translate).  Both models are finalized; the scene becomes inference-only and evaluates object by object."""
        if not self.finalized:
            self.finalize()
        if not other.finalized:
            other.finalize()
        for u, sname, rank, group in self._components():
            getattr(self, u).extend(getattr(other, u))
            getattr(self, sname).extend(getattr(other, sname))
            getattr(self, rank).extend(getattr(other, rank))
            getattr(self, group).extend(getattr(other, group))
        self.K.extend(other.K)
        oid = len(self.K) - 1

        def as_tensor(v, default):
            if v is None:
                return default
            return torch.from_numpy(v.astype(np.float32)) if isinstance(v, np.ndarray) else v.float()
        R = as_tensor(R, torch.eye(3, dtype=torch.float32))
        t = as_tensor(t, torch.zeros(3, dtype=torch.float32))
        T = torch.eye(4, dtype=torch.float32)
        T[:3, :3] = R.cpu() * (1 if s is None else s)
        T[:3, 3] = t.cpu()
        dev = self.aabb_train.device
        # (T is the model matrix; the samples go the other way)
        self.register_buffer(f"T_{oid}", torch.inverse(T).to(dev))
        self.register_buffer(f"R_{oid}", R.cpu().T.contiguous().to(dev))
        self.register_buffer(f"aabb_{oid}", other.aabb_train.detach().clone().to(dev))
        for _ in range(3):  # (several passes: the grid is an EMA-max of jittered samples)
            self.update_extra_state()
