"""Minimal NGP training step (the hot-path part of nerf/utils.py `Trainer`): rays -> render -> MSE -> backward ->
Adam, with fp16 autocast + GradScaler (`-O`), `update_extra_state` every 16 steps (nerf/utils.py:845-848),
Adam(betas=(0.9, 0.99), eps=1e-15) and lr 1e-2 (main_SealNeRF.py:283-288), PSNR as in nerf/utils.py:226-233.
Optional data parallelism over rays: gradients are all-reduced through one flat bucket (parallel/dist.py)."""
import contextlib
import gc
import math
import os

import torch
import torch.nn.functional as F

from gridencoder.grid import bump_weights_epoch


def psnr(pred, target):
    return -10 * math.log10(float(torch.mean((pred.float() - target.float()) ** 2)) + 1e-20)


class _BgMse(torch.autograd.Function):
    """loss = mean((image + (1 - weights_sum) * bg - gt)^2): background compositing (nerf/renderer.py:316) and the MSE
    criterion (nerf/utils.py:484) in one kernel per direction (csrc/ngp_head.hip) instead of ~14 tiny launches.  With
    `depth` / `gt_depth`: + depth_weight * L1Loss(nan_to_num(depth), gt_depth), Seal-3D's depth term (nerf/utils.py:486-489)
    — a value only: the reference's composite backward drops the depth gradient (raymarching.py:274)."""

    @staticmethod
    def forward(ctx, image, weights_sum, gt, bg, expected_grad=None, depth=None, gt_depth=None, depth_weight=1.0):
        """`expected_grad`: the (device scalar) upstream gradient the loss WILL receive — the loss scale under GradScaler; the
        forward launch then writes the backward's result as well and backward() launches nothing when it is handed that tensor"""
        import s3d_hip
        image, weights_sum, gt = image.float().contiguous(), weights_sum.float().contiguous(), gt.float().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=image.device)
        ctx.pre = None
        extra = {}
        if depth is not None:
            extra = dict(depth=depth.detach().float().contiguous().reshape(-1), gt_depth=gt_depth.float().contiguous().reshape(-1),
                         depth_weight=float(depth_weight))
        if expected_grad is not None and expected_grad.dtype == torch.float32 and expected_grad.numel() == 1:
            g_image, g_ws = torch.empty_like(image), torch.empty_like(weights_sum)
            s3d_hip.NgpHeadBackend.bg_mse_forward(image, weights_sum, gt, bg, loss, expected_grad, g_image, g_ws, **extra)
            ctx.pre = (g_image, g_ws, expected_grad.data_ptr(), expected_grad._version)
        else:
            s3d_hip.NgpHeadBackend.bg_mse_forward(image, weights_sum, gt, bg, loss, **extra)
        ctx.save_for_backward(image, weights_sum, gt)
        ctx.bg = bg
        return loss

    @staticmethod
    def backward(ctx, g):
        import s3d_hip
        if ctx.pre is not None and g.dtype == torch.float32 and g.data_ptr() == ctx.pre[2] and g._version == ctx.pre[3]:
            return (ctx.pre[0], ctx.pre[1]) + (None,) * 6  # (the announced upstream gradient: already computed)
        image, weights_sum, gt = ctx.saved_tensors
        g_image, g_ws = torch.empty_like(image), torch.empty_like(weights_sum)
        s3d_hip.NgpHeadBackend.bg_mse_backward(image, weights_sum, gt, ctx.bg, g.float().contiguous(), g_image, g_ws)
        return (g_image, g_ws) + (None,) * 6


def rgba_targets(images, random_bg=True, generator=None, seed=None, ctl=None):
    """Training targets of RGBA frames (nerf/utils.py:465-474): `images` [..., 4] -> (gt_rgb [..., 3], bg_color), with
    gt_rgb = rgb * a + bg_color * (1 - a) and bg_color a per-pixel random colour [..., 3] (`random_bg`) or the number 1 (a model
    with bg_radius > 0, and evaluation: nerf/utils.py:549-554).  Three-channel frames pass through with bg_color 1.
    Torch route (CPU tensors, or no `seed`): the reference's lines in the frames' dtype — `torch.rand_like`, so that
    torch.manual_seed reproduces the reference's draw (`generator`: torch.rand from it instead).  Native route (CUDA tensors
    and a `seed`): one launch of s3d_rgba_targets, fp32 results; `ctl` is the device int32 {step, 0} the launch advances, so a
    captured launch draws a fresh background on every replay.  Under data parallelism every rank passes its own seed."""
    if images.shape[-1] == 3:
        return images, 1
    if images.shape[-1] != 4:
        raise ValueError(f"rgba_targets: frames have 3 or 4 channels, got {images.shape[-1]}")
    if images.is_cuda and seed is not None:
        import s3d_hip
        if random_bg and ctl is None:
            raise ValueError("rgba_targets: the native route draws the background at step ctl[0] (a device int32 tensor {step, 0})")
        images = images.contiguous()
        gt = torch.empty(*images.shape[:-1], 3, dtype=torch.float32, device=images.device)
        bg = torch.empty_like(gt) if random_bg else None
        s3d_hip.RaySampleBackend.rgba_targets(images, gt, bg, random_bg=random_bg, seed=seed, ctl=ctl if random_bg else None)
        return gt, (bg if random_bg else 1)
    rgb, a = images[..., :3], images[..., 3:]
    if not random_bg:
        bg = 1
    elif generator is None:
        bg = torch.rand_like(rgb)
    else:
        bg = torch.rand(rgb.shape, generator=generator, dtype=rgb.dtype, device=rgb.device)
    return rgb * a + bg * (1 - a), bg


def update_error_map(out, gt_rgb, error_map, gt_depth=None, depth_weight=1.0, per_ray_error=None):
    """nerf/utils.py:506-528: fold the step's per-ray error into the error map as 0.1 old + 0.9 err.  `error_map` =
    (map [n, 128*128], index [B], inds_coarse [B, N]); err = mean_c((pred - gt)^2) (+ depth_weight * the batch's mean L1 depth
    error, added to every ray as `loss += criterion_depth(...)` does).  A renderer output that defers its background (the GPU's
    native route) is folded in by one launch of s3d_error_map_update, which composites the background itself; otherwise the
    reference's gather / scatter sequence runs.  `per_ray_error`: the error itself, where the caller has formed it (the mean over
    the levels of a rank-residual rendering)."""
    emap, index, inds = error_map
    index = torch.as_tensor(index, dtype=torch.int64, device=emap.device).reshape(-1)
    inds = inds.to(emap.device).reshape(index.numel(), -1)
    B, N = inds.shape
    depth = None
    if gt_depth is not None:
        depth = torch.nan_to_num(out["depth"].detach().float(), nan=0.0).reshape(-1)
    if out.get("premultiplied", False) and emap.is_cuda:
        import s3d_hip
        bg = out["bg_color"]
        bg = bg.detach().float().reshape(-1, 3).contiguous() if torch.is_tensor(bg) else \
            ((float(bg),) * 3 if not isinstance(bg, (tuple, list)) else tuple(float(v) for v in bg))
        s3d_hip.RaySampleBackend.error_map_update(
            emap, index, inds.contiguous(), out["image"].detach().float().reshape(-1, 3).contiguous(),
            gt_rgb.detach().float().reshape(-1, 3).contiguous(), out["weights_sum"].detach().float().reshape(-1).contiguous(), bg,
            depth.contiguous() if depth is not None else None,
            gt_depth.detach().float().reshape(-1).contiguous() if gt_depth is not None else None, depth_weight)
        return
    pred = out["image"]
    if out.get("premultiplied", False):
        bg = out["bg_color"]
        bg = bg.view(pred.shape) if torch.is_tensor(bg) else (bg if not isinstance(bg, (tuple, list)) else torch.tensor(bg, device=pred.device))
        pred = pred + (1 - out["weights_sum"]).unsqueeze(-1) * bg
    with torch.no_grad():
        if per_ray_error is not None:
            error = per_ray_error.float().view(B, N)
        else:
            error = F.mse_loss(pred.detach().float(), gt_rgb.detach().float().view(pred.shape), reduction="none").mean(-1).view(B, N)
        if gt_depth is not None:
            error = error + depth_weight * F.l1_loss(depth.view(gt_depth.shape), gt_depth.float())
        em = emap[index]  # [B, 128*128] (advanced indexing: a copy)
        ema = 0.1 * em.gather(1, inds) + 0.9 * error.to(em.device)
        em.scatter_(1, inds, ema)
        emap[index] = em


def render_loss(out, gt_rgb, expected_grad=None, gt_depth=None, depth_weight=1.0, error_map=None):
    """MSE between the rendered batch and the targets (+ Seal-3D's L1 depth term when `gt_depth` is given); uses the fused
    kernel when the renderer deferred the background (`expected_grad`: see _BgMse.forward).  `error_map`: (map, index,
    inds_coarse) of an error-map batch — the step's per-ray errors are folded into the map (update_error_map)."""
    if "levels" in out:
        # CCNeRF's rank-residual training (nerf/renderer.py marks it): image [K, ..., 3], one rendering per prefix of groups.  The per-ray criterion
        # [K, ...] is averaged over the levels before the error-map update and the final mean (nerf/utils.py:502-530)
        if gt_depth is not None:
            raise NotImplementedError("render_loss: a depth target with a rank-residual (CCNeRF) rendering")
        per_ray = F.mse_loss(out["image"], gt_rgb.unsqueeze(0).expand_as(out["image"]), reduction="none").mean(-1).mean(0)
        if error_map is not None:
            update_error_map(out, gt_rgb, error_map, per_ray_error=per_ray.detach())
        return per_ray.mean()
    if error_map is not None:
        update_error_map(out, gt_rgb, error_map, gt_depth, depth_weight)
    if "loss" in out:  # the renderer's compositing launch formed the criterion itself (Trainer._fused_loss -> render(fused_loss=...))
        return out["loss"]
    if out.get("premultiplied", False) and torch.is_tensor(out["bg_color"]):  # (a background model's colours, unfused criterion)
        out = dict(out, image=out["image"] + (1 - out["weights_sum"]).unsqueeze(-1) * out["bg_color"].view(out["image"].shape))
    elif out.get("premultiplied", False):
        bg = out["bg_color"]
        bg = (float(bg),) * 3 if not isinstance(bg, (tuple, list)) else tuple(float(v) for v in bg)
        if gt_depth is not None:
            return _BgMse.apply(out["image"].reshape(-1, 3), out["weights_sum"].reshape(-1), gt_rgb.reshape(-1, 3), bg, expected_grad,
                                out["depth"], gt_depth, depth_weight)
        return _BgMse.apply(out["image"].reshape(-1, 3), out["weights_sum"].reshape(-1), gt_rgb.reshape(-1, 3), bg, expected_grad)
    loss = F.mse_loss(out["image"], gt_rgb)
    if gt_depth is not None:
        loss = loss + depth_weight * F.l1_loss(torch.nan_to_num(out["depth"], nan=0.0).view(gt_depth.shape), gt_depth)
    return loss


class Trainer:
    def __init__(self, model, lr=1e-2, fp16=True, update_extra_interval=16, dist=None, max_steps=1024, dt_gamma=0,
                 T_thresh=1e-4, capturable=False, native_optim=None, optimizer=None, scaler=None, lr_scheduler=None, ema_decay=None):
        self.model = model
        # `ema_decay` (the reference's NGP / D-NeRF / Seal entry points pass 0.95, nerf/utils.py:356-357): an exponential moving
        # average of ALL parameters (nerf/ema.py), updated behind every optimizer step; evaluation and the `best` checkpoint use
        # the averaged weights.  None: no object, no launch
        self.ema_decay = ema_decay
        self.ema = None
        # `lr_scheduler(optimizer)` -> a torch scheduler, stepped after every optimizer step (nerf/utils.py:411-414 with
        # `scheduler_update_every_step=True`, main_SealNeRF.py:283-300: LambdaLR 0.1 ** min(iter / iters, 1)); a replayed step
        # follows it through the optimizer's device-side lr factor (nerf/optim.py: follow_lr_schedule)
        self._lr_scheduler_factory = lr_scheduler
        self.lr_scheduler = None
        self.lr = lr
        self.fp16 = fp16
        self.update_extra_interval = update_extra_interval
        self.dist = dist
        self.render_kwargs = dict(max_steps=max_steps, dt_gamma=dt_gamma, T_thresh=T_thresh)
        on_gpu = next(model.parameters()).is_cuda
        # GPU default: Adam + loss scaling straight from the (fp16) gradients of the HIP kernels (nerf/optim.py);
        # native_optim=False keeps the reference's torch.optim.Adam + GradScaler (the only choice on CPU)
        self.native_optim = on_gpu if native_optim is None else (native_optim and on_gpu)
        self._capturable = capturable and on_gpu
        if optimizer is not None:  # share an existing optimizer / scaler (e.g. an eager twin of a graphed trainer)
            self.optimizer, self.scaler = optimizer, scaler
            if lr_scheduler is not None:
                self.lr_scheduler = lr_scheduler(self.optimizer)
            self._rebuild_ema()
        else:
            self.scaler = None
            self.rebuild_optimizer()
        self.global_step = 0
        self.epoch = 0
        self.workspace, self.name = None, "ngp"  # where save_mesh puts a file it is given no path for
        # the training set's error map (nerf/utils.py:616 `self.error_map = train_loader._data.error_map`): with it, steps that
        # are handed `index` / `inds_coarse` fold their per-ray errors into it (update_error_map)
        self.error_map = None
        self._em_batch = None
        self.stats = {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
        if dist is not None:
            dist.register(model)  # broadcasts rank 0's parameters through `.data` (no version bump) ...
            resync = getattr(self.optimizer, "resync_half", None)
            if resync is not None:
                resync()  # ... so the optimizer's fp16 copies are re-made from the adopted values
            bump_weights_epoch()
            if self.ema is not None:
                self.ema.reseed()  # ... and the average starts from them: every rank holds the same shadows from here on

    def _param_groups(self):
        """the optimizer's parameter groups (a backbone's trainer may use several learning rates: tensoRF/utils.py)"""
        return self.model.get_params(self.lr)

    def rebuild_optimizer(self):
        """(re-)create optimizer (and, the first time, the loss scaler) over the model's CURRENT parameters — needed after
        the parameter set changes (TensoRF upsample_model, tensoRF/utils.py:137-140 / :347-352)"""
        model, lr, fp16 = self.model, self.lr, self.fp16
        on_gpu = next(model.parameters()).is_cuda
        if self.native_optim:
            from .optim import NativeAdam, NativeGradScaler
            self.optimizer = NativeAdam(self._param_groups(), lr=lr, betas=(0.9, 0.99), eps=1e-15)
            if self.scaler is None:
                self.scaler = NativeGradScaler(next(model.parameters()).device, enabled=fp16)
            if self.dist is None:
                self.scaler.attach(self.optimizer)
        else:
            self.optimizer = torch.optim.Adam(self._param_groups(), betas=(0.9, 0.99), eps=1e-15, fused=on_gpu,
                                              capturable=self._capturable)
            if self.scaler is None:
                self.scaler = torch.amp.GradScaler("cuda", enabled=fp16)
        if self._lr_scheduler_factory is not None:
            self.lr_scheduler = self._lr_scheduler_factory(self.optimizer)
        self._rebuild_ema()

    def _rebuild_ema(self):
        """the average over the model's CURRENT parameters, started from their current values with the update count at 0 (a
        changed parameter set — TensoRF upsampling, a CCNeRF structure change — starts it over: the old shadows fit nothing)"""
        if self.ema_decay is None:
            return
        if self.ema is None:
            from .ema import NativeEMA, weights_changed
            self.ema = NativeEMA(self.model.parameters(), decay=self.ema_decay,
                                 on_weights_changed=lambda: weights_changed(self.optimizer))
        else:
            self.ema.reseed(self.model.parameters())

    def _averaged(self):
        """context of evaluation: the model holds the averaged weights inside it (nerf/utils.py:774-785, 919-1011), its own after it"""
        return self.ema.average_parameters() if self.ema is not None else contextlib.nullcontext()

    def _sched_step(self):
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()

    def save_checkpoint(self, workspace, name="ngp", full=False, best=False, remove_old=True, max_keep_ckpt=2):
        """reference on-disk format (nerf/utils.py:1015-1076); see nerf/checkpoint.py"""
        from .checkpoint import save_checkpoint
        return save_checkpoint(self, workspace, name, full=full, best=best, remove_old=remove_old, max_keep_ckpt=max_keep_ckpt,
                               ema=self.ema)

    def load_checkpoint(self, checkpoint, model_only=False):
        """reference on-disk format (nerf/utils.py:1078-1137); a file written by the reference's Trainer loads as is"""
        from .checkpoint import load_checkpoint
        return load_checkpoint(self, checkpoint, model_only=model_only, ema=self.ema)

    def _maybe_update_extra_state(self):
        model = self.model
        if model.cuda_ray and self.global_step % self.update_extra_interval == 0:
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                model.update_extra_state()
            if self.dist is not None:
                # replicas draw different random cells: adopt rank 0's grid / bitfield / mean_count so that every rank
                # marches the same occupancy and takes the same (re-)capture decisions below
                self.dist.sync_extra_state(model)
            return True
        return False

    def _error_map_batch(self, index, inds_coarse, gt_rgb):
        """(map, index, inds_coarse) of this step's update, or None (no map, or the batch was not drawn from it).  Targets
        arrive blended: RGBA frames go through one of the two producers first, with or without a map."""
        if gt_rgb is not None and not isinstance(gt_rgb, tuple) and gt_rgb.shape[-1] != 3:
            raise ValueError("train_step takes blended targets [N, 3]: RGBA frames (the reference's per-pixel random background) are "
                             "blended by NeRFDataset.sample() or nerf.trainer.rgba_targets(), which return gt_rgb and bg_color")
        if self.error_map is None or inds_coarse is None or index is None:
            return None
        if self.dist is not None:
            raise NotImplementedError("error map: not supported with data parallelism (the ranks' rays update one map; "
                                      "keeping it consistent across ranks is not implemented)")
        return (self.error_map, index, inds_coarse)

    def _eager_step(self, rays_o, rays_d, gt_rgb, bg_color=1):
        model = self.model
        # without data parallelism the gradients are simply replaced each step (no 49 MB zero fill + 147 MB accumulate);
        # with it they live in the flat all-reduce bucket and are cleared in place
        self.optimizer.zero_grad(set_to_none=self.dist is None)
        self._open_step_tail()
        try:
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                out = model.render(rays_o, rays_d, bg_color=bg_color, perturb=True, force_all_rays=False,
                                   defer_background=self.native_optim, fused_loss=self._fused_loss(gt_rgb), **self.render_kwargs)
                loss = self._regularized(render_loss(out, gt_rgb, self._expected_grad(), error_map=self._em_batch))
        except BaseException:
            self._drop_step_tail()
            raise
        self._backward(loss)
        self._reduce_and_step()
        return loss.detach()

    fused_losses = True  # GPU + native optimizer: one-launch criteria (False: the unfused sequences, A/B runs and parity tests)

    def _fused_loss(self, gt_rgb, gt_depth=None, depth_weight=1.0):
        """`fused_loss=` of NeRFRenderer.run_cuda: targets and the loss's announced upstream gradient for
        raymarching.composite_rays_train_loss — compositing, criterion and compositing backward as one launch.
        None where the step has no announced gradient (torch's GradScaler) or the fusion is switched off."""
        g = self._expected_grad()
        if g is None or not self.fused_losses or not self.native_optim or not gt_rgb.is_cuda:
            return None
        return dict(gt=gt_rgb, expected_grad=g, gt_depth=gt_depth, depth_weight=depth_weight)

    def _regularizer(self):
        """extra loss term of a backbone's trainer (TensoRF: `density_loss() * l1_reg_weight`, tensoRF/utils.py:42-49); None: none"""
        return None

    def _regularized(self, loss):
        reg = self._regularizer()
        return loss if reg is None else loss + reg.to(loss.dtype)

    def _reduce_and_step(self):
        """gradient all-reduce (data parallelism) + optimizer step.  Native optimizer: the reduction is issued in pieces and
        pipelined with the per-parameter updates (NativeGradScaler.step); torch optimizer: one reduction, then the step."""
        if self.dist is not None and self.native_optim:
            self.scaler.step(self.optimizer, dist=self.dist)
        else:
            if self.dist is not None:
                self.dist.allreduce_grads(self.scaler)
            self.scaler.step(self.optimizer)
        self.scaler.update()
        self._ema_update()

    def _ema_update(self):
        """behind the optimizer step and the scaler's update of EVERY step, skipped ones included (nerf/utils.py:733: the
        reference calls `ema.update()` unconditionally).  Stream order puts it behind a table update that ran inside the grid
        backward too."""
        if self.ema is not None:
            self.ema.update()

    def _expected_grad(self):
        """the upstream gradient `_backward` will hand to the loss (NativeGradScaler: its scale tensor), if known in advance"""
        sc = self.scaler
        return sc._scale.reshape(()) if (hasattr(sc, "backward") and getattr(sc, "enabled", False)) else None

    # the hash tables' Adam inside their backward's accumulate kernel (nerf/optim.py: arm_fused_tables); S3D_FUSE_TABLE_ADAM=0: A/B
    fuse_table_updates = __import__("os").environ.get("S3D_FUSE_TABLE_ADAM", "1") != "0"

    def _fused_tables_allowed(self):
        opt, sc = self.optimizer, self.scaler
        if getattr(self.model, "bg_radius", 0) > 0:
            return False  # (the background model's backward is not ordered behind the tables': their updates stay in step())
        if not (self.fuse_table_updates and self.native_optim and self.dist is None and hasattr(opt, "arm_fused_tables")
                and hasattr(sc, "_checked_at_source")):
            return False
        params = [p for g in opt.param_groups for p in g["params"]]
        return all(getattr(p, "_s3d", None) is not None for p in params) and sc._checked_at_source(opt)

    def _arm_fused_tables(self):
        """single replica, native optimizer + scaler, every gradient of the step a hand-over buffer whose producer raises the
        scaler's flag itself: the step's skip decision is complete when the tables' backward — the last node of the graph —
        starts, so their update can be applied there.  (Seal's nn.Linear `.grad`s without a pack, TensoRF's factors, data
        parallelism: the separate update as before.)"""
        if not self._fused_tables_allowed():
            return 0
        sc = self.scaler
        return self.optimizer.arm_fused_tables(grad_scale=sc._scale if sc.enabled else None)

    # The step's small closing launches — the MLPs' weight-gradient reduce and Adam, the criterion's sum, the scaler's update with
    # the ring push — inside the hash table's backward (s3d_hip.StepTail, NativeAdam.arm_step_tail).  False: the separate
    # launches (A/B runs, parity tests)
    fuse_step_tail = True
    _tail = None

    def _open_step_tail(self):
        """Before the step's render: a holder for the closing launches, where the tables' update may ride at all (one replica, no
        background model, ...: `_fused_tables_allowed`).  The criterion's sum is filed in it when nothing reads the loss value
        before the backward pass (no regularizer is added to it)."""
        import s3d_hip
        if s3d_hip.StepTail.current is not None:
            s3d_hip.StepTail.current.close()  # (a step that ended in an exception)
        self._tail = None
        if not (self.fuse_step_tail and getattr(self.scaler, "enabled", False) and self._fused_tables_allowed()
                and hasattr(self.optimizer, "arm_step_tail")):
            return
        self._tail = s3d_hip.StepTail.current = s3d_hip.StepTail()
        self._tail.accept_loss = type(self)._regularizer is Trainer._regularizer and type(self)._regularized is Trainer._regularized

    def _drop_step_tail(self):
        """the step failed before its backward pass: nobody may find its holder (nothing it holds is launched)"""
        import s3d_hip
        if self._tail is not None and s3d_hip.StepTail.current is self._tail:
            s3d_hip.StepTail.current = None
        self._tail = None

    def _backward(self, loss):
        """the step's ONE backward pass (every caller follows it with `_reduce_and_step`)"""
        n = self._arm_fused_tables()
        tail, self._tail = self._tail, None
        if tail is not None and not (n == 1 and self.optimizer.arm_step_tail(tail, self.scaler, getattr(self, "_ring_args", None))):
            tail.close()  # (no table, or two of them: a filed criterion sum is launched now, everything else as always)
            tail = None
        try:
            if hasattr(self.scaler, "backward"):  # NativeGradScaler: the scale is passed as the root gradient
                self.scaler.backward(loss)
            else:
                self.scaler.scale(loss).backward()
        finally:
            if tail is not None:
                tail.close()  # (whatever was filed and not taken by the table's backward — it did not run — is launched here)

    def train_step(self, rays_o, rays_d, gt_rgb, bg_color=1, index=None, inds_coarse=None):
        """rays_o/d [N,3], gt_rgb [N,3].  Returns the (detached) loss tensor; no host sync.  `index` / `inds_coarse` (a batch
        of NeRFDataset.collate / sample with the error map on): the step updates `self.error_map`.  `bg_color`: a number, three
        numbers, or the per-ray background [N,3] fp32 the targets were blended onto (NeRFDataset.sample / rgba_targets)."""
        self._em_batch = self._error_map_batch(index, inds_coarse, gt_rgb)
        try:
            self.model.train()
            self._maybe_update_extra_state()
            self.global_step += 1
            loss = self._eager_step(rays_o, rays_d, gt_rgb, bg_color)
            self._sched_step()
        finally:
            self._em_batch = None
        return loss

    def save_mesh(self, save_path=None, resolution=256, threshold=10):
        """nerf/utils.py:583-603: the model's density > threshold surface on the resolution^3 lattice of aabb_infer, as a PLY
        (default <workspace>/meshes/<name>_<epoch>.ply).  Field and marching cubes stay on the device (nerf/mesh.py); the
        model is only read, so a captured step replays unchanged afterwards."""
        from .mesh import save_mesh
        if save_path is None:
            if self.workspace is None:
                raise ValueError("save_mesh: no save_path, and the trainer has no `workspace` to derive one from")
            save_path = os.path.join(self.workspace, "meshes", f"{self.name}_{self.epoch}.ply")
        save_mesh(self.model, save_path, resolution=resolution, threshold=threshold, fp16=self.fp16)
        return save_path

    @torch.no_grad()
    def render_image(self, rays_o, rays_d, bg_color=1):
        self.model.eval()
        with self._averaged(), torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            return self.model.render(rays_o, rays_d, bg_color=bg_color, perturb=False, **self.render_kwargs)

    # ------------------------------------------------------------------ interactive preview (nerf/preview.py)
    def _preview_render(self, rays_o, rays_d, bg_color, perturb):
        """the render of a preview frame: eval mode, averaged weights, autocast (nerf/utils.py:772-785)"""
        self.model.eval()
        with self._averaged(), torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            return self.model.render(rays_o, rays_d, staged=True, bg_color=bg_color, perturb=perturb, **self.render_kwargs)

    @torch.no_grad()
    def test_gui(self, pose, intrinsics, W, H, bg_color=None, spp=1, downscale=1, return_pos=False, color_space="srgb", native=None,
                 display=None):
        """nerf/utils.py:754-820: one preview frame from a free camera.  `pose`: 4 x 4 cam2world (numpy), `intrinsics`: fx, fy,
        cx, cy of the W x H frame.  The frame is rendered at int(H * downscale) x int(W * downscale) with the intrinsics scaled,
        `perturb = False if spp == 1 else spp`, and brought back to H x W by nearest-neighbour upsampling; `color_space="linear"`
        converts the colours to sRGB.  Returns device tensors {"image" [H, W, 3], "depth" [H, W]} and, with `return_pos`
        (downscale 1 only: ValueError otherwise), "pos" [H, W, 3] = rays_o + depth * rays_d.
        On the GPU the frame's rays and the whole tail are one launch each (s3d_frame_rays, s3d_preview_resolve); on CPU tensors,
        or with `native=False`, the reference's torch op sequence runs.  `display`: the display state of a
        nerf.preview.PreviewSession, whose buffer the tail then updates as well.  The model is only read: a captured training
        step replays unchanged afterwards."""
        from .preview import preview_frame
        return preview_frame(self, pose, intrinsics, W, H, bg_color=bg_color, spp=spp, downscale=downscale, return_pos=return_pos,
                             color_space=color_space, native=native, display=display)

    def _gui_batch(self, dataset, i):
        """batch i of train_gui: drawn on the device where the dataset lives there (`sample`), else by `collate`"""
        index = [i % len(dataset)]
        dev = getattr(dataset, "device", None)
        if hasattr(dataset, "sample") and dev is not None and torch.device(dev).type == "cuda":
            return dataset.sample(index)
        return dataset.collate(index)

    def _gui_train_step(self, data):
        gt, bg = data["images"], data.get("bg_color", 1)
        if gt.shape[-1] == 4:
            gt, bg = rgba_targets(gt)
        return self.train_step(data["rays_o"].reshape(-1, 3), data["rays_d"].reshape(-1, 3), gt.reshape(-1, 3),
                               bg_color=bg.reshape(-1, 3) if torch.is_tensor(bg) else bg, index=data.get("index"),
                               inds_coarse=data.get("inds_coarse"))

    def train_gui(self, dataset, step=16):
        """nerf/utils.py:690-749: `step` training steps between two preview frames, on batches of `dataset` (its `sample` on
        the device, else `collate`), cycling through its images.  Nothing is read back before the one read of the summed loss.
        The parameter average keeps this trainer's cadence (every step).  Returns {"loss": the mean, "lr": the first group's}."""
        total = None
        for k in range(step):
            loss = self._gui_train_step(self._gui_batch(dataset, self._gui_cursor + k)).detach().float().reshape(())
            total = loss.clone() if total is None else total + loss
        self._gui_cursor += step
        return {"loss": float(total) / step if step else 0.0, "lr": self.optimizer.param_groups[0]["lr"]}

    _gui_cursor = 0



# Stream capture restricts HIP calls of the CAPTURING thread only: with a process group alive, torch's RCCL watchdog thread
# polls its work events (hipEventQuery) at any time, and under the default "global" mode such a poll during one of the
# captures below aborts the process ("operation not permitted when stream is capturing").
_CAPTURE_MODE = "thread_local"


@contextlib.contextmanager
def _capturing(graph, pool=None):
    """`torch.cuda.graph` under _CAPTURE_MODE with Python's cycle collector held off.  A collection that starts inside a capture
    runs, on the capturing thread, the destructors of whatever dead cycle it finds — an earlier trainer with its CUDAGraph and
    that graph's private memory pool among them (a trainer is part of a cycle: tests that need one gone call gc.collect()) — and
    a HIP call that stream capture does not permit aborts the process.  When a collection falls is a matter of allocation counts,
    so it moves with any change of host code.  Garbage waits until the capture has ended."""
    held = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode=_CAPTURE_MODE, **({} if pool is None else {"pool": pool})):
            yield
    finally:
        if held:
            gc.enable()
_RING_PUSH = __import__("os").environ.get("S3D_RING_PUSH", "1") != "0"  # A/B switch: 0 = host-side ring bookkeeping


class GraphedTrainer(Trainer):
    """The same training step replayed from a HIP graph (torch.cuda.CUDAGraph): the step issues ~115 kernels whose
    launch cost (~0.3 ms of a 2.5 ms step, rocprof: GPU 79 % busy) is paid once at capture.

    What makes the step capturable: no host sync inside it (the sample budget M is a *static* allocation instead of the
    16-step running mean — rays that do not fit are dropped exactly as in the reference, raymarching.cu:416 — fused
    Adam + GradScaler keep found_inf on the device), static input buffers, libseal3d_hip launches on the capture
    stream.  `update_extra_state` (data-dependent shapes, `.item()`) stays eager every 16 steps; the graph is
    re-captured only when the budget has to grow.

    The budget is generous (`budget_factor` x the running mean at capture): every per-sample kernel of the step takes the
    march's device-side sample count (`n_valid`, seal3d_hip.h) and skips the unused tail of the buffers, so a larger M
    costs two fills, not compute — fewer dropped rays than the reference's M = running mean, and re-captures only when
    the mean outgrows the headroom."""

    def __init__(self, model, num_rays, budget_factor=1.3, graph_extra_state=True, capture_collectives=True, **kw):
        super().__init__(model, capturable=True, **kw)
        self.capture_collectives = capture_collectives  # False: two graphs with the all-reduce issued eagerly between them
        self.collectives_in_graph = False
        dev = next(model.parameters()).device
        self.s_ro = torch.zeros(num_rays, 3, device=dev)
        self.s_rd = torch.zeros(num_rays, 3, device=dev)
        self.s_gt = torch.zeros(num_rays, 3, device=dev)
        self.s_bg = torch.ones(num_rays, 3, device=dev)  # per-ray background of RGBA batches (nerf/utils.py:471)
        self.budget_factor = budget_factor
        self.graph_extra_state = graph_extra_state
        self.ues_graph, self.ues_mean, self.ues_warm = None, None, False
        self.graph = None
        self.graph_opt = None
        self.n_captures = 0
        self.budget = 0
        self._budget_check_due = False  # an update's sample mean is still to be set against the budget (_maybe_update_extra_state)
        self.s_loss = None
        self.s_counter = torch.zeros(2, dtype=torch.int32, device=dev)
        # the graph itself files each step's loss and sample counter in 16-slot rings (seal3d_hip.h: s3d_step_ring_push)
        # (the loss history is longer than the counter ring: the tensor train_step() hands out for step k is a view of slot
        #  k % 1024 and stays valid for the next 1,023 steps — a caller that keeps loss tensors longer clones them)
        self.loss_ring = torch.zeros(1024, dtype=torch.float32, device=dev)
        self._pushes = 0  # ring pushes executed so far = the device's running step number (s_cursor[1])
        self.s_cursor = torch.zeros(2, dtype=torch.int32, device=dev)  # {ring slot, running step number}
        self.noise_key = (torch.initial_seed() * 0x9E3779B1 + (self.dist.rank if self.dist is not None else 0) * 0x85EBCA6B) & 0xFFFFFFFF
        self._counter_ring = None
        self._ring_args = None
        # error-map batches: the captured step reads the batch's image index and cells from static buffers too (written by
        # NeRFDataset.sample(out=static_batch()) or staged), and its update launch is part of the graph
        self.s_index = torch.zeros(1, dtype=torch.int64, device=dev)
        self.s_inds_coarse = torch.zeros(1, num_rays, dtype=torch.int64, device=dev)
        self._graph_em = None
        self._graph_bg = False  # the step on hand / captured composites on s_bg (True) or on the constant 1

    def static_batch(self):
        """the step's static input buffers as a `sample(out=...)` target (one image of num_rays rays): the sampler's launch
        writes the batch where the captured step reads it"""
        n = self.s_ro.shape[0]
        return {"rays_o": self.s_ro.view(1, n, 3), "rays_d": self.s_rd.view(1, n, 3), "images": self.s_gt.view(1, n, 3),
                "bg_color": self.s_bg.view(1, n, 3), "inds_coarse": self.s_inds_coarse, "index": self.s_index}

    def _static_loss(self):
        """the step's loss on the static input buffers (subclasses: other criteria, e.g. Seal's depth term)"""
        self._open_step_tail()
        try:
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                out = self.model.render(self.s_ro, self.s_rd, bg_color=self.s_bg if self._graph_bg else 1, perturb=True,
                                        force_all_rays=False, defer_background=self.native_optim,
                                        fused_loss=self._fused_loss(self.s_gt), **self.render_kwargs)
                return self._regularized(render_loss(out, self.s_gt, self._expected_grad(), error_map=self._em_batch))
        except BaseException:
            self._drop_step_tail()
            raise

    def _body_fb(self):
        """zero grads -> render -> loss -> scaled backward"""
        # without data parallelism the gradients are simply replaced each step (no 49 MB zero fill + 147 MB accumulate);
        # with it they live in the flat all-reduce bucket and are cleared in place
        self.optimizer.zero_grad(set_to_none=self.dist is None)
        loss = self._static_loss()
        self._ring_args = None
        if self._counter_ring is not None and self.native_optim:
            # rides in the scaler update's launch (_body_opt), or with it in the hash table's backward (Trainer.fuse_step_tail)
            self._ring_args = (loss.detach().float().reshape(()), self.s_counter, self.loss_ring, self._counter_ring, self.s_cursor)
        self._backward(loss)
        loss = loss.detach()
        if self._counter_ring is not None and not self.native_optim:
            import s3d_hip
            s3d_hip.OptimBackend.step_ring_push(loss.float().reshape(()), self.s_counter, self.loss_ring, self._counter_ring, self.s_cursor)
        return loss

    def _body_opt(self):
        self.scaler.step(self.optimizer)
        if self._ring_args is not None:
            self.scaler.update(ring_push=self._ring_args)
            self._ring_args = None
        else:
            self.scaler.update()
        self._ema_update()  # (part of the captured optimizer body: a step stays one replay — the second one of the two-graph split)

    def _capture(self):
        """One graph for the whole step — with data parallelism too when the process group's collectives can be captured
        (RCCL; probed once, parallel/dist.py: capture_supported).  Otherwise (gloo, `capture_collectives=False`) the step
        is captured as TWO graphs (forward+backward | check+Adam+scaler update) and the gradient all-reduce is issued eagerly
        between the two replays."""
        model = self.model
        model.train()
        self.n_captures += 1
        if hasattr(self.optimizer, "capture_lr"):
            self.optimizer.capture_lr()  # (this lr becomes a launch argument; later values reach the replay through lr_scale)
        self._graph_lr_epoch = getattr(self.optimizer, "lr_epoch", 0)
        self.budget = int(max(model.mean_count, 1) * self.budget_factor)
        saved = (model.mean_count, model.local_step)
        model.mean_count = self.budget
        # the marcher always counts in a private buffer; the last kernel of the step files it in the ring slot of a device
        # cursor (which follows `local_step % 16`), and leaves the private counter cleared for the next replay
        ring = model.step_counter
        self._counter_ring = ring if ring.is_contiguous() and ring.dtype == torch.int32 and _RING_PUSH else None
        self.s_counter.zero_()
        self.s_cursor[0].fill_(saved[1] % 16)
        model.step_counter = self.s_counter.view(1, 2).expand(16, 2)
        model._counter_prezeroed = self._counter_ring is not None
        if self._counter_ring is not None:  # per-ray jitter drawn from the device-side step number instead of torch.rand
            model._noise_step, model._noise_key = self.s_cursor[1:], self.noise_key
        model.local_step = 0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            # ONE real step on the current batch, launched eagerly on a side stream: it is this call's training step (the
            # capture below records without executing, and train_step does not replay after a capture), and it warms the
            # allocator pools the capture will draw from (the eager steps before the first capture did the rest); every
            # rank runs the same number of all-reduces
            model.local_step = 0
            self.s_warm_loss = self._body_fb().clone()
            if self.dist is not None:
                self.dist.allreduce_grads(self.scaler)
            self._body_opt()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        model.local_step = 0
        if self.dist is None:
            with _capturing(self.graph):
                self.s_loss = self._body_fb()
                self._body_opt()
            self.graph_opt = None
        elif self.capture_collectives and self.dist.capture_supported():
            # data parallelism, ONE graph: forward + backward, the gradient all-reduce (RCCL records into the capture: its
            # kernels run on the process group's stream, forked from and joined back into the step's stream by event edges),
            # check + Adam + scale update.  One collective per gradient buffer — every fork / join edge costs ~9 us here.
            saved_chunk = self.dist.chunk_bytes
            self.dist.chunk_bytes = 1 << 40
            try:
                with _capturing(self.graph):
                    self.s_loss = self._body_fb()
                    self.dist.allreduce_grads(self.scaler)
                    self._body_opt()
            finally:
                self.dist.chunk_bytes = saved_chunk
            self.graph_opt = None
            self.collectives_in_graph = True
        else:
            with _capturing(self.graph):
                self.s_loss = self._body_fb()
            self.graph_opt = torch.cuda.CUDAGraph()
            with _capturing(self.graph_opt, pool=self.graph.pool()):
                self._body_opt()
            self.collectives_in_graph = False
        model.step_counter = ring
        model._counter_prezeroed = False
        model._noise_step = None
        model.mean_count, model.local_step = saved

    def load_checkpoint(self, checkpoint, model_only=False):
        out = super().load_checkpoint(checkpoint, model_only=model_only)
        self._counter_ring = None
        self.graph = self.graph_opt = None  # optimizer state tensors were replaced, mean_count may have moved: re-capture
        return out

    def _check_budget(self):
        """drop the captured step when the running mean sample count left the static budget's useful range: re-capture"""
        mean = self.model.mean_count
        if self.graph is not None and (mean * 1.1 > self.budget or mean * 2 < self.budget):
            self.graph = None

    def _maybe_update_extra_state(self):
        """steady state: the partial occupancy update replayed from its own HIP graph, with NO host read.  Per cascade: the
        two sorted streams (torch), three launches for the draw, the density query, two for the scatter / EMA-max; then one
        tail launch and the bitfield re-pack.  The update's mean density and sample count travel to pinned host memory behind
        an event (NeRFRenderer.finish_extra_state), so the host keeps running ahead of the device across the update.
        The sample-budget check that follows an update is therefore put off to the top of the NEXT update, when that event
        has long completed: a re-capture decision lags by one update interval (16 steps).  The budget is 1.3 x the running
        mean, and the check fires once 1.1 x the mean exceeds it or 2 x the mean falls below it, which leaves room for that
        lag; a step whose samples exceed the budget drops the overflowing rays, as it always did.
        First sweeps, models that extend `update_extra_state`, and `graph_extra_state=False` keep the eager reference
        sequence."""
        from .renderer import NeRFRenderer
        model = self.model
        if not (model.cuda_ray and self.global_step % self.update_extra_interval == 0):
            return False
        # (a model may extend update_extra_state by a pure epilogue — the Seal renderers re-mark the edit region in the
        #  bitfield, SealNeRF/renderer.py:50-66 — and say so: `after_extra_state`)
        epilogue = getattr(model, "after_extra_state", None) if getattr(type(model), "extra_state_epilogue_only", False) else None
        plain = type(model).update_extra_state is NeRFRenderer.update_extra_state or epilogue is not None
        if not (self.graph_extra_state and plain and model.iter_density >= 16) or getattr(model, "dist_shard", None) is not None:
            return super()._maybe_update_extra_state()  # (sharded over the ranks: density queries split + all-gather)
        if self._budget_check_due:
            self._budget_check_due = False
            self._check_budget()  # (the previous update's numbers: their event completed many steps ago)
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            if self.ues_graph is None and not self.ues_warm:
                mean = model.partial_grid_update_device()  # first time: eager (lazy initialisations, allocator warm-up)
                self.ues_warm = True
            else:
                if self.ues_graph is None:
                    self.ues_graph = torch.cuda.CUDAGraph()
                    with _capturing(self.ues_graph):
                        self.ues_mean = model.partial_grid_update_device()
                model.stage_extra_state()
                self.ues_graph.replay()
                mean = self.ues_mean
            model.finish_extra_state(mean)
            if epilogue is not None:
                epilogue()
        if self.dist is not None:
            self.dist.sync_extra_state(model)
        return True

    def _stage_inputs(self, rays_o, rays_d, gt_rgb, bg=None):
        dst, src = [self.s_ro, self.s_rd, self.s_gt], [rays_o, rays_d, gt_rgb]
        if bg is not None:
            dst.append(self.s_bg)
            src.append(bg)
        if all(a.data_ptr() == b.data_ptr() for a, b in zip(dst, src)):
            return  # (drawn into the static buffers by the sampler: static_batch)
        torch._foreach_copy_(dst, [t.reshape(-1, 3) for t in src])  # one launch

    def _stage_error_map(self, em):
        """the static (map, index, inds_coarse) of the captured step; the batch's are copied in unless the sampler wrote them
        there"""
        emap, index, inds = em
        index = torch.as_tensor(index, dtype=torch.int64).reshape(-1)
        if index.numel() != 1 or inds.numel() != self.s_inds_coarse.numel():
            raise ValueError("GraphedTrainer: an error-map batch is one image of num_rays rays")
        if index.data_ptr() != self.s_index.data_ptr():
            self.s_index.copy_(index, non_blocking=True)
        if inds.data_ptr() != self.s_inds_coarse.data_ptr():
            self.s_inds_coarse.copy_(inds.reshape(1, -1))
        return (emap, self.s_index, self.s_inds_coarse)

    def _replay(self):
        # an eager backward without a step since the last replay left gradients in the hand-over buffer that the captured
        # step (recorded with a clean buffer: no fill) would accumulate onto: clear them first (host-side flags, no sync)
        dirty = getattr(self.optimizer, "clear_unconsumed", None)
        if dirty is not None:
            dirty()
        self.graph.replay()
        if self.graph_opt is not None:
            self.dist.allreduce_grads(self.scaler)
            self.graph_opt.replay()
        # the replay files its loss at slot s_cursor[1] % loss_slots and advances the device cursor: the host count moves HERE,
        # next to the launch, so that any caller of _replay() keeps the two in step
        slot = self._pushes % self.loss_ring.numel()
        if self._counter_ring is not None:
            self._pushes += 1
        return slot

    def train_step(self, rays_o, rays_d, gt_rgb, bg_color=1, index=None, inds_coarse=None):
        self._em_batch = self._error_map_batch(index, inds_coarse, gt_rgb)
        try:
            return self._graphed_step(rays_o, rays_d, gt_rgb, bg_color)
        finally:
            self._em_batch = None

    def _graphed_step(self, rays_o, rays_d, gt_rgb, bg_color):
        model = self.model
        model.train()
        if self._maybe_update_extra_state():
            self.s_cursor[0].zero_()  # (update_extra_state restarts the counter ring: local_step = 0)
            pending = getattr(model, "extra_state_pending", None)
            if pending is not None and pending():
                self._budget_check_due = True  # (a native update's numbers are checked at the top of the next update)
            else:
                self._check_budget()
        self.global_step += 1
        if self.graph is None and model.mean_count <= 0:
            # no sample statistics yet (first 16 steps): eager step with the wrapper's host sync
            loss = self._eager_step(rays_o, rays_d, gt_rgb, bg_color)
            self._sched_step()
            return loss
        per_ray = torch.is_tensor(bg_color)
        if per_ray:
            if type(self)._static_loss is not GraphedTrainer._static_loss:
                raise ValueError("GraphedTrainer: this trainer's captured criterion composites on bg_color=1")
            if not (bg_color.is_cuda and bg_color.dtype == torch.float32 and bg_color.numel() == self.s_bg.numel()):
                raise ValueError("GraphedTrainer: a per-ray background is an fp32 device tensor [num_rays, 3]")
            self._stage_inputs(rays_o, rays_d, gt_rgb, bg_color.detach())
        elif bg_color != 1:
            raise ValueError("GraphedTrainer: the captured step composites on the white background (bg_color=1) of the "
                             "BASELINE configs or on a per-ray background tensor; use Trainer for other background colours")
        else:
            self._stage_inputs(rays_o, rays_d, gt_rgb)
        if self.graph is not None and per_ray != self._graph_bg:
            self.graph = None  # (captured for the other kind of background: re-capture)
        self._graph_bg = per_ray
        if self._em_batch is not None:
            self._em_batch = self._stage_error_map(self._em_batch)
        em_key = None if self._em_batch is None else self._em_batch[0].data_ptr()
        if self.graph is not None and em_key != self._graph_em:
            self.graph = None  # (the captured step updates another map, or none: re-capture)
        if self.graph is not None and hasattr(self.optimizer, "follow_lr_schedule") and not self.optimizer.follow_lr_schedule():
            self.graph = None  # (parameter groups moved by different factors: the captured lr arguments no longer fit)
        if self.graph is not None and getattr(self.optimizer, "lr_epoch", 0) != getattr(self, "_graph_lr_epoch", 0):
            self.graph = None  # (somebody rebased the captured lrs since — another graph's capture, an eager step: re-capture)
        if self.graph is None:
            self._graph_em = em_key
            self._capture()  # runs this step eagerly (one optimizer update), then records the graph
            loss = self.s_warm_loss
            filed = self._counter_ring is not None
            self._pushes += 1 if filed else 0  # (the warm-up step filed its loss too)
        else:
            slot = self._replay()
            filed = self._counter_ring is not None
            # the static loss buffer is overwritten by the next replay; the graph files each step's loss in a 1,024-slot
            # history (no extra launch per step): the caller gets the VIEW of this step's slot, untouched for 1,023 more steps
            # — a caller that keeps loss tensors longer than that (statistics over an epoch) clones or reads them
            loss = self.loss_ring[slot] if filed else self.s_loss.clone()
        bump_weights_epoch()  # replays update the parameters without touching Tensor._version
        if not filed:
            model.step_counter[model.local_step % 16].copy_(self.s_counter)
        model.local_step += 1
        self._sched_step()
        return loss
