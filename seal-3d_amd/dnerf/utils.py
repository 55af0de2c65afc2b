"""D-NeRF trainer (dnerf/utils.py:73-122 of the reference): the NGP training step at one time per batch, two learning rates
(encoders `lr`, networks `lr_net`: dnerf/network.py:255-270) and the deformation regulariser `1e-3 * |deform|.mean()`."""
import torch

from nerf.trainer import GraphedTrainer as _GraphedTrainer
from nerf.trainer import Trainer as _Trainer


class Trainer(_Trainer):
    def __init__(self, model, lr=1e-2, lr_net=1e-3, deform_reg_weight=1e-3, **kw):
        self.lr_net = lr_net
        self.deform_reg_weight = deform_reg_weight
        super().__init__(model, lr=lr, **kw)

    def _param_groups(self):
        return self.model.get_params(self.lr, self.lr_net)

    def _regularizer(self):
        """`deform_reg_weight * |deform|.mean()` of the step's rendering (dnerf/utils.py:117-119).  On the fused route the value is
        weight * reg_sum / (3 * rows) with reg_sum from the warp kernel, and its gradient reaches the deformation network as the
        `coef` of s3d_dnerf_warp_backward — the upstream gradient of reg_sum, i.e. the scaler's scale times weight / (3 * rows) —
        not through torch's abs / mean backward.  The mean runs over the rows that hold a sample (the one divergence
        from the reference, which also averages the marcher's zero-padded rows)."""
        if not self.deform_reg_weight:
            return None
        model = self.model
        fused = getattr(model, "_deform_reg", None)
        if fused is not None:
            reg_sum, rows = fused
            return reg_sum * (self.deform_reg_weight / (3.0 * max(rows, 1)))
        deform = getattr(model, "_last_deform", None)
        if deform is None or deform.numel() == 0:  # (no rendering yet, or a step whose rays marched no sample)
            return None
        return self.deform_reg_weight * deform.abs().mean()

    def train_step(self, rays_o, rays_d, gt_rgb, time, bg_color=1, index=None, inds_coarse=None):
        """rays_o / rays_d [N, 3] of ONE frame, gt_rgb [N, 3], time: that frame's time in [0, 1] (a number or a [1, 1] tensor)"""
        self.render_kwargs["time"] = time
        try:
            return super().train_step(rays_o, rays_d, gt_rgb, bg_color, index=index, inds_coarse=inds_coarse)
        finally:
            self.render_kwargs.pop("time", None)
            self.model._last_deform = None
            self.model._deform_reg = None

    @torch.no_grad()
    def render_image(self, rays_o, rays_d, time, bg_color=1):
        """the eval / test rendering at `time`"""
        self.model.eval()
        with self._averaged(), torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            return self.model.render(rays_o, rays_d, time, bg_color=bg_color, perturb=False, **self.render_kwargs)

    eval_step = test_step = render_image

    def _preview_render(self, rays_o, rays_d, bg_color, perturb, time=0):
        self.model.eval()
        with self._averaged(), torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            return self.model.render(rays_o, rays_d, time, staged=True, bg_color=bg_color, perturb=perturb, **self.render_kwargs)

    @torch.no_grad()
    def test_gui(self, pose, intrinsics, W, H, time=0, bg_color=None, spp=1, downscale=1, color_space="srgb", native=None,
                 display=None):
        """dnerf/utils.py:169-219: the preview frame of nerf.trainer.Trainer.test_gui at `time` in [0, 1].  As in the reference
        `perturb=spp` is passed ALWAYS, so a D-NeRF preview jitters its first sample at spp 1 as well (the static trainers do
        not), and there is no `return_pos`."""
        from nerf.preview import preview_frame
        return preview_frame(self, pose, intrinsics, W, H, bg_color=bg_color, spp=spp, downscale=downscale, color_space=color_space,
                             native=native, display=display, perturb=spp, time=time)


class GraphedTrainer(_GraphedTrainer):
    def __init__(self, model, *args, **kw):
        raise NotImplementedError("GraphedTrainer: the D-NeRF backbone's step is not captured — the occupancy slot is chosen on the "
                                  "host from the batch's time and the network reads the marcher's sample count back in every step, "
                                  "neither of which a replayed graph can follow; use dnerf.utils.Trainer")
