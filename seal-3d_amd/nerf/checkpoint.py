"""Checkpoints in the reference's on-disk format (nerf/utils.py:1015-1137 of the reference): a plain `torch.save` dict

    {epoch, global_step, stats, [mean_count, mean_density], model: state_dict, [optimizer, lr_scheduler, scaler, ema]}

written to `{workspace}/checkpoints/{name}_ep{epoch:04d}.pth`.  The model's state-dict keys are the reference's
(`encoder.embeddings`, `encoder.offsets`, `sigma_net.weights` / `sigma_net.{i}.weight`, `color_net.*`, `density_grid`,
`density_bitfield`, `step_counter`, `aabb_train`, `aabb_infer`), so a file written by the reference's Trainer loads
here and the other way round; the Seal student starts from the teacher's file the same way (`--ckpt`).

`optimizer` holds torch.optim.Adam's layout (per-parameter `step`, `exp_avg`, `exp_avg_sq`) and `scaler`
torch.amp.GradScaler's (`scale`, `growth_factor`, `backoff_factor`, `growth_interval`, `_growth_tracker`) whichever
optimizer/scaler implementation the trainer runs (nerf/optim.py translates).
"""
import glob
import os

import torch

from .ema import weights_changed


def checkpoint_path(workspace, name, epoch):
    return os.path.join(workspace, "checkpoints", f"{name}_ep{epoch:04d}.pth")


def save_checkpoint(trainer, workspace, name="ngp", full=False, best=False, remove_old=True, max_keep_ckpt=2,
                    lr_scheduler=None, ema=None):
    """Write the trainer's state; returns the file path (None when `best` has nothing to compare)."""
    model = trainer.model
    stats = trainer.stats
    state = {"epoch": trainer.epoch, "global_step": trainer.global_step, "stats": stats}
    if model.cuda_ray:
        state["mean_count"] = model.mean_count
        state["mean_density"] = model.mean_density
    if hasattr(model, "time_size"):
        state["time_size"] = int(model.time_size)  # D-NeRF: the time axis of density_grid / density_bitfield / times
    if hasattr(model, "upsample_model") and hasattr(model, "resolution"):
        state["resolution"] = list(model.resolution)  # TensoRF: factor resolution at save time (tensoRF/utils.py:236)
    if getattr(model, "rank_residual", False):  # CCNeRF: the model's structure (tensoRF/utils.py:251-256)
        _refuse_composed(model, "save")
        for key in _CC_RANKS:
            state[key] = [int(r) for r in getattr(model, key)[0]]
    if full:
        state["optimizer"] = trainer.optimizer.state_dict()
        if lr_scheduler is not None:
            state["lr_scheduler"] = lr_scheduler.state_dict()
        state["scaler"] = trainer.scaler.state_dict()
        if ema is not None:
            state["ema"] = ema.state_dict()
    ckpt_dir = os.path.join(workspace, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    if not best:
        state["model"] = model.state_dict()
        path = checkpoint_path(workspace, name, trainer.epoch)
        if remove_old:
            stats["checkpoints"].append(path)
            if len(stats["checkpoints"]) > max_keep_ckpt:
                old = stats["checkpoints"].pop(0)
                if os.path.exists(old):
                    os.remove(old)
        torch.save(state, path)
        return path
    # "best": only when the last evaluation improved; drops density_grid (not needed to render, :1067-1068)
    if not stats["results"]:
        return None
    if stats["best_result"] is not None and stats["results"][-1] >= stats["best_result"]:
        return None
    stats["best_result"] = stats["results"][-1]
    path = os.path.join(ckpt_dir, f"{name}.pth")
    if ema is not None:
        ema.store()
        ema.copy_to()
    try:
        state["model"] = dict(model.state_dict())
        state["model"].pop("density_grid", None)
        # written BEFORE the restore: a state-dict's tensors are the parameters' own storage, so a file written behind it (as
        # the reference does, nerf/utils.py:1064-1073) would hold the restored values, not the averaged ones
        torch.save(state, path)
    finally:
        if ema is not None:
            ema.restore()
            ema.collected_params = None
    return path


def latest_checkpoint(workspace, name="ngp"):
    files = sorted(glob.glob(os.path.join(workspace, "checkpoints", f"{name}_ep*.pth")))
    return files[-1] if files else None


def load_checkpoint(trainer, checkpoint, model_only=False, lr_scheduler=None, ema=None):
    """Load a reference-format file into the trainer; returns (missing_keys, unexpected_keys).

    A bare state-dict (no 'model' key) is accepted like the reference does (:1081-1084)."""
    model = trainer.model
    device = next(model.parameters()).device
    ckpt = torch.load(checkpoint, map_location=device, weights_only=False)
    _check_time_size(model, ckpt)
    if "model" not in ckpt:
        model.load_state_dict(ckpt)
        weights_changed(trainer.optimizer)
        _reseed(ema, model)
        return [], []
    if getattr(model, "rank_residual", False) and all(k in ckpt for k in _CC_RANKS):
        _refuse_composed(model, "load")
        model = _match_cc_structure(trainer, ckpt)
    elif "resolution" in ckpt and hasattr(model, "upsample_model") and list(ckpt["resolution"]) != list(model.resolution):
        # TensoRF: bring the factors to the checkpoint's resolution before loading them, then re-create the optimizer
        # over the new Parameters (tensoRF/utils.py:347-352)
        model.upsample_model(ckpt["resolution"])
        trainer.rebuild_optimizer()
    missing, unexpected = model.load_state_dict(ckpt["model"], strict=False)
    weights_changed(trainer.optimizer)
    if ema is not None and "ema" in ckpt:
        ema.load_state_dict(ckpt["ema"])
    else:
        _reseed(ema, model)
    if model.cuda_ray:
        if "mean_count" in ckpt:
            model.mean_count = ckpt["mean_count"]
        if "mean_density" in ckpt:
            model.mean_density = ckpt["mean_density"]
    if model_only:
        return list(missing), list(unexpected)
    trainer.stats = ckpt["stats"]
    trainer.epoch = ckpt["epoch"]
    trainer.global_step = ckpt["global_step"]
    if trainer.optimizer is not None and "optimizer" in ckpt:
        trainer.optimizer.load_state_dict(ckpt["optimizer"])
    if lr_scheduler is not None and "lr_scheduler" in ckpt:
        lr_scheduler.load_state_dict(ckpt["lr_scheduler"])
    if trainer.scaler is not None and "scaler" in ckpt and ckpt["scaler"]:
        trainer.scaler.load_state_dict(ckpt["scaler"])
    return list(missing), list(unexpected)


def _check_time_size(model, ckpt):
    """D-NeRF: the occupancy buffers carry a time axis of `time_size` slots; a file of another size does not fit the model"""
    if not hasattr(model, "time_size"):
        return
    sd = ckpt.get("model", ckpt)
    have = ckpt.get("time_size")
    if have is None and torch.is_tensor(sd.get("times")):
        have = sd["times"].shape[0]
    if have is not None and int(have) != int(model.time_size):
        raise ValueError(f"checkpoint: written with time_size={int(have)}, the model has time_size={int(model.time_size)}; "
                         "create the model with the checkpoint's time_size")


_CC_RANKS = ("rank_vec_density", "rank_mat_density", "rank_vec", "rank_mat")


def _refuse_composed(model, what):
    """the checkpoint format carries ONE object's rank lists (the reference's does too): a composed scene — several objects with
    their `T_i` / `R_i` / `aabb_i` buffers — would be written with the host object's structure and come back with the other
    objects' tensors as unexpected keys.  Save the objects' own checkpoints and compose them again after loading."""
    if len(model.K) > 1:
        raise ValueError(f"checkpoint: cannot {what} a composed CCNeRF scene ({len(model.K) - 1} composed objects): the format "
                         "holds one object's rank lists; keep the objects' own checkpoints and call compose() after loading them")


def _match_cc_structure(trainer, ckpt):
    """CCNeRF: a checkpoint fits only a model of its own structure — the rank lists decide how many parameters there are, and a
    finalized or compressed model has other lists than the one it was trained as.  A model of another structure is re-created
    from the checkpoint's lists at the checkpoint's resolution, and the optimizer over its parameters (tensoRF/utils.py:327-356
    of the reference)."""
    model = trainer.model
    same = (all([int(r) for r in ckpt[k]] == [int(r) for r in getattr(model, k)[0]] for k in _CC_RANKS) and len(model.K) == 1
            and list(ckpt["resolution"]) == list(model.resolution))
    if same:
        return model
    device = next(model.parameters()).device
    extra = dict(bg_resolution=model.bg_resolution, bg_rank=model.bg_rank) if model.bg_radius > 0 else {}
    new = type(model)(resolution=[int(r) for r in ckpt["resolution"]], degree=model.degree, bound=model.bound, cuda_ray=model.cuda_ray,
                      density_scale=model.density_scale, min_near=model.min_near, density_thresh=model.density_thresh,
                      bg_radius=model.bg_radius, **{k: [int(r) for r in ckpt[k]] for k in _CC_RANKS}, **extra).to(device)
    new.train(model.training)
    trainer.model = new
    trainer.rebuild_optimizer()
    return new


def _reseed(ema, model):
    """A file without an `ema` entry (model-only, `best`, written without an EMA) loaded into a trainer that keeps one: the
    average starts over from the loaded weights, update count 0.  (The reference leaves the shadows at the values they had —
    after construction the random initial weights — and then evaluates those; DESIGN.md lists the divergence.)"""
    if ema is not None and hasattr(ema, "reseed"):
        ema.reseed(model.parameters())
