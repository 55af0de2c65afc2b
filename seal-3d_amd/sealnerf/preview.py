"""The headless edit loop of the reference's GUI (SealNeRF/gui.py: `callback_config_brush`, `callback_train`, `train_step`,
`callback_override`, `callback_ckpt_reset`): paint strokes on a preview, turn them into a brush config, distil, look again."""
import time as _time

import numpy as np
import torch

from nerf.preview import PreviewSession, next_train_steps

from .seal_utils import get_seal_mapper

# the brush options the window starts with (SealNeRF/gui.py:109-118)
BRUSH_DEFAULTS = {
    "type": "brush",
    "normal": [1, 0, 0],
    "brushType": [],
    "brushDepth": 0.6,
    "brushPressure": 0.02,
    "attenuationDistance": 0.02,
    "attenuationMode": "dry",
    "simplifyVoxel": 16,
}


class SealSession(PreviewSession):
    """A PreviewSession over a Seal student trainer (its `teacher` is the model being edited).  Frames are rendered by the
    student; `render_trainer` may be pointed at a trainer of the teacher to look at the unedited scene."""

    def __init__(self, trainer, W, H, dataset=None, teacher_trainer=None, **kw):
        super().__init__(trainer, W, H, **kw)
        self.dataset = dataset
        self.teacher_trainer = teacher_trainer
        self.brush_options = {k: (list(v) if isinstance(v, list) else v) for k, v in BRUSH_DEFAULTS.items()}
        self.brush_type = "line"
        self.config = None
        self.train_steps = 16
        self.trained_steps = 0  # `self.step` of the reference's window
        self.is_pretraining = False

    def add_stroke(self, mask, brush_type=None):
        super().add_stroke(mask)
        self.brush_options["brushType"].append(brush_type or self.brush_type)

    def clear_strokes(self):
        super().clear_strokes()
        self.brush_options["brushType"] = []

    def brush_config(self, **options):
        """`callback_config_brush`: the painted strokes as a brush config — raw: per stroke the list of 3-D points under it,
        rgb: the brush colour, the normal normalised, the remaining options as set (`options` overrides them).  None when
        nothing is painted."""
        self.brush_options.update(options)
        if not self.brush_masks:
            return None
        raw = [p.cpu().numpy().tolist() for p in self.mask_positions(cluster=True)]
        norm = np.linalg.norm(self.brush_options["normal"], axis=0)
        self.brush_options["normal"] = [x / norm for x in self.brush_options["normal"]]
        self.config = dict(raw=raw, rgb=self.brush_color.tolist(), **self.brush_options)
        return self.config

    def begin_edit(self, config=None, **pretraining):
        """`callback_train`: the mapper of `config` (default: the last brush_config) goes to teacher and student, the
        pretraining sets are built (`pretraining`: the arguments of init_pretraining), and the strokes are cleared"""
        config = config if config is not None else self.config
        if config is None:
            raise ValueError("begin_edit: no edit config (paint strokes and call brush_config, or pass one)")
        self.config = config
        mapper = get_seal_mapper(config)
        self.trainer.teacher.init_mapper(mapper)
        self.trainer.model.init_mapper(mapper)
        self.trainer.invalidate_graphs()
        self.trainer.init_pretraining(**pretraining)
        self.trained_steps = 0
        self.is_pretraining = self.trainer.pretraining_epochs > 0
        self.clear_strokes()
        self.need_update = True
        return mapper

    def train(self, step=None):
        """the window's `train_step`: `step` (default: the adaptive train_steps) pretraining epochs or fine-tuning steps.  A
        call never runs past the last pretraining epoch, and the call that reaches `pretraining_epochs` switches to
        fine-tuning (the window runs whole batches of epochs and switches once it has passed the count).  With the default
        step the measured time adapts train_steps (next_train_steps)."""
        n = self.train_steps if step is None else int(step)
        if self.is_pretraining:
            n = min(n, max(self.trainer.pretraining_epochs - self.trained_steps, 1))
        on_gpu = self.device.type == "cuda"
        if on_gpu:
            starter, ender = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            starter.record()
        else:
            t0 = _time.perf_counter()
        out = self.trainer.train_gui(self.dataset, step=n, is_pretraining=self.is_pretraining)
        if on_gpu:
            ender.record()
            ender.synchronize()
            t = starter.elapsed_time(ender)
        else:
            t = (_time.perf_counter() - t0) * 1000
        self.trained_steps += n
        if self.is_pretraining and self.trained_steps >= self.trainer.pretraining_epochs:
            self.is_pretraining = False
        self.need_update = True
        if step is None and t > 0:
            self.train_steps = next_train_steps(t, n)
        return out

    @torch.no_grad()
    def commit(self):
        """`callback_override`: the student becomes the teacher; both mappers are cleared and the teacher's bitfield restored"""
        tr = self.trainer
        tr.teacher.load_state_dict(tr.model.state_dict())
        tt = self.teacher_trainer
        if tr.ema is not None and tt is not None and tt.ema is not None:
            tt.ema.load_state_dict(tr.ema.state_dict())
        if tr.teacher.density_bitfield_hacked:
            tr.teacher.restore_bitfield()
        tr.teacher.seal_mapper = None
        tr.model.seal_mapper = None
        tr.invalidate_graphs()
        self._weights_replaced(tt)
        self.trained_steps, self.need_update = 0, True

    @torch.no_grad()
    def reset(self):
        """`callback_ckpt_reset`: the teacher's weights go back over the student's"""
        tr = self.trainer
        tr.model.load_state_dict(tr.teacher.state_dict())
        tt = self.teacher_trainer
        if tr.ema is not None and tt is not None and tt.ema is not None:
            tr.ema.load_state_dict(tt.ema.state_dict())
        tr.invalidate_graphs()
        self._weights_replaced(tr)
        self.trained_steps, self.need_update = 0, True

    @staticmethod
    def _weights_replaced(trainer):
        """parameters were overwritten in place: cached fp16 copies are stale"""
        from gridencoder.grid import bump_weights_epoch
        bump_weights_epoch()
        resync = getattr(getattr(trainer, "optimizer", None), "resync_half", None)
        if resync is not None:
            resync()
