"""SDF trainer (sdf/utils.py of the reference): train_step / eval_step / test_step on one dataset item, epochs of items,
evaluation, checkpoints in the project's format and `save_mesh` through the device marching cubes.

The criterion is the reference's `mape_loss` (loss.py:7-16).  Where the model's fused route runs, loss and gradient come from one
launch on the MLP's padded rows (s3d_sdf_mape_forward_backward); anywhere else the torch restatement below is used.  The parameter
average of `torch_ema` (main_sdf.py:58 `ema_decay=0.95`) is nerf/ema.py's; tensorboard and `rich` are left out, as in the other
trainers here."""
import contextlib
import os

import torch
from torch.autograd import Function

import s3d_hip
from nerf import checkpoint as ckpt
from nerf.mesh import extract_geometry, write_ply


def mape_loss(pred, target, reduction="mean"):
    """mean absolute percentage error with the reference's floor of 1e-2 on |target|; pred, target [B, 1]"""
    loss = (pred - target).abs() / (target.abs() + 1e-2)
    return loss.mean() if reduction == "mean" else loss


class _FusedMape(Function):
    """mape_loss(clamp(rows[:B, 0]), target) on the MLP's rows [Bp, 16] fp16.  The forward launch writes the gradient too, multiplied
    by B so that it is sign / (|t| + 1e-2) — in fp16's normal range whatever the batch size; backward scales it by the upstream
    gradient (the loss scale) / B."""

    @staticmethod
    def forward(ctx, rows, target, B, clip):
        loss, grad = s3d_hip.SdfBackend.mape_forward_backward(rows[:B], target.reshape(-1).contiguous(), clip, float(B))
        if rows.shape[0] != B:
            grad = torch.cat([grad, grad.new_zeros(rows.shape[0] - B, grad.shape[1])], dim=0)
        ctx.save_for_backward(grad)
        ctx.B = B
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * (g.float() / ctx.B).to(grad.dtype), None, None, None


def fused_mape(rows, target, clip=None):
    return _FusedMape.apply(rows, target, target.numel(), clip)


def default_optimizer(model, lr=1e-4):
    """main_sdf.py:51-54: Adam over two groups, weight decay on the MLP only.  (torch's Adam: nerf/optim.py's native one has no weight
    decay yet — DESIGN.md "SDF", open items)"""
    return torch.optim.Adam([{"name": "encoding", "params": model.encoder.parameters()},
                             {"name": "net", "params": model.backbone.parameters(), "weight_decay": 1e-6}],
                            lr=lr, betas=(0.9, 0.99), eps=1e-15)


class Trainer:
    def __init__(self, name, model, criterion=mape_loss, optimizer=None, lr_scheduler=None, device=None, mute=False, fp16=False,
                 eval_interval=1, max_keep_ckpt=2, workspace=None, use_checkpoint="latest", scheduler_update_every_step=False,
                 ema_decay=None):
        """optimizer / lr_scheduler: factories `model -> optimizer`, `optimizer -> scheduler` as in the reference (None: main_sdf.py's
        Adam, and its StepLR(10, 0.1)).  ema_decay: keep nerf.ema.NativeEMA over the parameters, updated after every optimizer step;
        evaluation and the `best` checkpoint use the averaged weights (sdf/utils.py:148-149, 349-350, 414-422, 503-511 of the reference)"""
        self.name, self.mute, self.fp16, self.workspace = name, mute, fp16, workspace
        self.eval_interval, self.max_keep_ckpt, self.scheduler_update_every_step = eval_interval, max_keep_ckpt, scheduler_update_every_step
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.model = model.to(self.device)
        self.criterion = criterion
        self.optimizer = optimizer(self.model) if optimizer is not None else default_optimizer(self.model)
        self.lr_scheduler = (lr_scheduler(self.optimizer) if lr_scheduler is not None
                             else torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=10, gamma=0.1))
        self.scaler = torch.amp.GradScaler(self.device.type, enabled=self.fp16 and self.device.type == "cuda")
        self.ema = None
        if ema_decay is not None:
            from nerf.ema import NativeEMA, weights_changed
            self.ema = NativeEMA(self.model.parameters(), decay=ema_decay, on_weights_changed=lambda: weights_changed(self.optimizer))
        self.epoch = self.global_step = self.local_step = 0
        self.stats = {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
        self.step_losses = []  # the last epoch's loss per step
        if workspace is not None:
            os.makedirs(workspace, exist_ok=True)
            if use_checkpoint == "latest":
                path = ckpt.latest_checkpoint(workspace, name)
                if path is not None:
                    self.load_checkpoint(path)
            elif use_checkpoint == "best":
                best = os.path.join(workspace, "checkpoints", f"{name}.pth")
                path = best if os.path.exists(best) else ckpt.latest_checkpoint(workspace, name)
                if path is not None:
                    self.load_checkpoint(path, model_only=path == best)
            elif use_checkpoint != "scratch":
                self.load_checkpoint(use_checkpoint)

    def log(self, *args):
        if not self.mute:
            print(*args)

    def _autocast(self):
        return torch.autocast(self.device.type, dtype=torch.float16, enabled=self.fp16 and self.device.type == "cuda")

    # ---- one item --------------------------------------------------------------------------------------------------------------
    def train_step(self, data):
        """data: points [1, B, 3], sdfs [1, B, 1] -> (pred [B, 1], truth [B, 1], loss)"""
        X, y = data["points"][0], data["sdfs"][0]
        model = self.model
        if self.criterion is mape_loss and model.can_fuse(X):
            rows = model.forward_padded(X)
            loss = fused_mape(rows, y, model.clip_sdf)
            pred = rows[:X.shape[0], :1]
            if model.clip_sdf is not None:
                pred = pred.clamp(-model.clip_sdf, model.clip_sdf)
            return pred, y, loss
        pred = model(X)
        return pred, y, self.criterion(pred, y)

    def eval_step(self, data):
        return self.train_step(data)

    def test_step(self, data):
        return self.model(data["points"][0])

    def prepare_data(self, data):
        return {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in data.items()}

    # ---- epochs ----------------------------------------------------------------------------------------------------------------
    def train_one_epoch(self, loader):
        self.log(f"==> Start Training Epoch {self.epoch}, lr={self.optimizer.param_groups[0]['lr']:.6f} ...")
        self.model.train()
        if hasattr(loader.dataset, "epoch"):
            loader.dataset.epoch = self.epoch
        losses = []
        self.local_step = 0
        for data in loader:
            self.local_step += 1
            self.global_step += 1
            data = self.prepare_data(data)
            self.optimizer.zero_grad(set_to_none=True)
            with self._autocast():
                _, _, loss = self.train_step(data)
            self.scaler.scale(loss).backward()
            self.scaler.step(self.optimizer)
            self.scaler.update()
            if self.ema is not None:
                self.ema.update()
            if self.scheduler_update_every_step:
                self.lr_scheduler.step()
            losses.append(loss.detach().float())  # (read once, after the epoch)
        self.step_losses = torch.stack(losses).tolist() if losses else []
        average = sum(self.step_losses) / max(len(self.step_losses), 1)
        self.stats["loss"].append(average)
        if not self.scheduler_update_every_step:
            if isinstance(self.lr_scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                self.lr_scheduler.step(average)
            else:
                self.lr_scheduler.step()
        self.log(f"==> Finished Epoch {self.epoch}, loss={average:.4f}.")
        return average

    @torch.no_grad()
    def evaluate_one_epoch(self, loader):
        self.log(f"++> Evaluate at epoch {self.epoch} ...")
        self.model.eval()
        losses = []
        with self.ema.average_parameters() if self.ema is not None else contextlib.nullcontext():
            for data in loader:
                with self._autocast():
                    _, _, loss = self.eval_step(self.prepare_data(data))
                losses.append(loss.detach().float())
        average = float(torch.stack(losses).mean()) if losses else float("nan")
        self.stats["valid_loss"].append(average)
        self.stats["results"].append(average)  # (no metrics: the best checkpoint is the one of the lowest loss)
        self.log(f"++> Evaluate epoch {self.epoch} Finished, loss={average:.4f}.")
        return average

    def train(self, train_loader, valid_loader, max_epochs):
        for epoch in range(self.epoch + 1, max_epochs + 1):
            self.epoch = epoch
            self.train_one_epoch(train_loader)
            if self.workspace is not None:
                self.save_checkpoint(full=True, best=False)
            if self.epoch % self.eval_interval == 0:
                self.evaluate_one_epoch(valid_loader)
                if self.workspace is not None:
                    self.save_mesh()
                    self.save_checkpoint(full=False, best=True)

    def evaluate(self, loader):
        return self.evaluate_one_epoch(loader)

    # ---- files -----------------------------------------------------------------------------------------------------------------
    def save_mesh(self, save_path=None, resolution=256):
        """the zero level set over [-1, 1]^3 as a PLY"""
        if save_path is None:
            save_path = os.path.join(self.workspace, "validation", f"{self.name}_{self.epoch}.ply")
        self.log(f"==> Saving mesh to {save_path}")
        os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
        was_training = self.model.training
        self.model.eval()

        def query_func(pts):
            with torch.no_grad(), self._autocast():
                return self.model(pts.to(self.device).float().contiguous()).float()

        vertices, triangles = extract_geometry(torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]), resolution, 0,
                                               query_func, device=self.device)
        self.model.train(was_training)
        write_ply(save_path, vertices, triangles)
        self.log("==> Finished saving mesh.")
        return save_path

    def save_checkpoint(self, full=False, best=False):
        return ckpt.save_checkpoint(self, self.workspace, name=self.name, full=full, best=best, max_keep_ckpt=self.max_keep_ckpt,
                                    lr_scheduler=self.lr_scheduler, ema=self.ema)

    def load_checkpoint(self, checkpoint, model_only=False):
        missing, unexpected = ckpt.load_checkpoint(self, checkpoint, model_only=model_only, lr_scheduler=self.lr_scheduler,
                                                      ema=self.ema)
        self.log(f"[INFO] loaded {checkpoint}" + (f", missing {missing}" if missing else "") + (f", unexpected {unexpected}" if unexpected else ""))
        return missing, unexpected
