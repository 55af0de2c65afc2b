"""The Seal data provider's distillation half (SealNeRF/provider.py:13-136): a pose set whose images are REPLACED by the
teacher's renders through the proxy (`proxy_dataset`), and the per-step batch that gathers colour + depth targets of random
pixels from them (`collate`).  The disk loader under it (nerf/provider.py: transforms.json, image decoding) is outside the
hot path — poses, intrinsics and the frame size are handed in.  `SealRandomDataset` is the provider of `--custom_pose`
(:145-178): batches from generated orbit cameras around the edit."""
import math

import numpy as np
import torch

from nerf.provider import MAP_CELLS, DeviceSampling
from nerf.synthetic import get_rays, rand_poses


class SealDataset(DeviceSampling):
    """`error_map=True` (training only): the reference's per-image map of recent per-pixel loss, torch.ones(n, 128*128) on the
    device (nerf/provider.py:234-256, inherited by SealNeRF/provider.py); `collate` then draws error-weighted pixels and hands
    out `index` / `inds_coarse`, and `sample()` (nerf/provider.py: DeviceSampling) draws the batch on the GPU."""

    def __init__(self, poses, intrinsics, H, W, num_rays=4096, images=None, device=None, training=True, render_kwargs=None,
                 fp16=False, error_map=False, seed=0):
        self.device = torch.device(device) if device is not None else poses.device
        self.poses = poses.to(self.device)
        self.intrinsics, self.H, self.W = intrinsics, H, W
        self.training = training
        self.num_rays = num_rays if training else -1
        self.images = images  # [B, H, W, 3] or None (the reference's ground truth: only its shape is used by proxy_dataset)
        self.depths = None
        self.proxy_flag = False
        self.fp16 = fp16
        self.render_kwargs = dict(render_kwargs or {})
        self.error_map = torch.ones(len(self.poses), MAP_CELLS, dtype=torch.float, device=self.device) \
            if (training and error_map) else None
        self._init_sampling(seed)

    def __len__(self):
        return self.poses.shape[0]

    @torch.no_grad()
    def proxy_dataset(self, model, n_batch=1):
        """SealNeRF/provider.py:19-70: every pose rendered by the teacher (`render(..., staged=True, bg_color=None,
        perturb=False, force_all_rays=True)` in the mode the teacher is in, in `n_batch` pieces — like the reference's loop,
        a remainder piece makes `n_batch` one larger FOR EVERY LATER POSE too), NaNs zeroed; the frames become `images`
        [B, H, W, 3] and `depths` [B, H, W, 1] and batches are marked `skip_proxy`."""
        images, depths = [], []
        if not getattr(model, "density_bitfield_hacked", True):
            model.hack_bitfield()  # (SealNeRF/trainer.py:268-269, before the provider is asked)
        for i in range(len(self)):
            rays = get_rays(self.poses[i:i + 1], self.intrinsics, self.H, self.W, -1)
            rays_o, rays_d = rays["rays_o"].contiguous(), rays["rays_d"].contiguous()
            total = rays_o.shape[1]
            size = total // n_batch
            if total % n_batch:
                n_batch += 1
            img, dep = [], []
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16 and rays_o.is_cuda):
                for k in range(n_batch):
                    out = model.render(rays_o[:, k * size:(k + 1) * size], rays_d[:, k * size:(k + 1) * size], staged=True,
                                       bg_color=None, perturb=False, force_all_rays=True, **self.render_kwargs)
                    img.append(out["image"])
                    dep.append(out["depth"])
            img = torch.nan_to_num(torch.cat(img, 1), nan=0.0)
            dep = torch.nan_to_num(torch.cat(dep, 1), nan=0.0)
            images.append(img.float().view(self.H, self.W, -1))
            depths.append(dep.float().view(self.H, self.W, -1))
        self.images = torch.stack(images, dim=0)
        self.depths = torch.stack(depths, dim=0)
        self.proxy_flag = True

    def collate(self, index, generator=None):
        """SealNeRF/provider.py:72-131 for a dataset pose: `num_rays` random pixels of pose `index[0]` (error-map weighted when
        the map is on), their rays and the targets gathered from `images` / `depths`; with the map also `index` and
        `inds_coarse` (the trainer's update)"""
        B = len(index)
        poses = self.poses[index]
        error_map = None if self.error_map is None else self.error_map[index]
        rays = get_rays(poses, self.intrinsics, self.H, self.W, self.num_rays, error_map, generator=generator)
        out = {"H": self.H, "W": self.W, "rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "skip_proxy": self.proxy_flag,
               "data_index": torch.tensor(index), "pixel_index": rays["inds"] if self.num_rays > 0 else None}
        for name, frames in (("images", self.images), ("depths", self.depths)):
            if frames is None:
                continue
            v = frames[index].to(self.device)
            if self.training:
                C = v.shape[-1]
                v = torch.gather(v.view(B, -1, C), 1, torch.stack(C * [rays["inds"]], -1))
            out[name] = v
        if error_map is not None:
            out["index"] = index
            out["inds_coarse"] = rays["inds_coarse"]
        return out


class SealRandomDataset(DeviceSampling):
    """`--custom_pose` (main_SealNeRF.py:113-118, 316-340; SealNeRF/provider.py:145-178): fine-tuning batches from generated
    orbit cameras around the edit instead of dataset poses.  Every batch is the full frame of a random pose looking at
    `look_at` from distance `radius` (default: the mapper's `pose_center` / `pose_radius`), at the low resolution whose pixel
    count is about `num_rays`; the targets are the teacher's proxy render (no `images`, `skip_proxy` unset).  As shipped, the
    reference's collate passes `look_at=` to a `rand_poses` without that parameter; here it means: the orbit's centre
    (nerf/synthetic.py: rand_poses).

    Frame size (SealNeRF/provider.py:163-166): s = sqrt(H W / num_rays) in float64 (1 when num_rays <= 0 or not training),
    rH, rW = int(H / s), int(W / s), intrinsics / s; `rays_per_batch` = rH rW is what a trainer's `num_rays` has to be.
    `len()` is `n_val` for validation and `epoch_length` for training (the poses are generated: an epoch is as long as the
    caller says)."""

    poses = None
    images = None
    error_map = None

    def __init__(self, mapper_or_map_data, intrinsics, H, W, num_rays=4096, device=None, training=True, n_val=10, look_at=None,
                 radius=None, theta_range=(math.pi / 3, 2 * math.pi / 3), phi_range=(0, 2 * math.pi), seed=0, epoch_length=100):
        map_data = getattr(mapper_or_map_data, "map_data", mapper_or_map_data) or {}
        if look_at is None:
            look_at = map_data.get("pose_center")
        if radius is None:
            radius = map_data.get("pose_radius")
        if look_at is None or radius is None:
            raise ValueError("SealRandomDataset: the mapper's map_data has no 'pose_center' / 'pose_radius' (the brush mapper "
                             "provides none): pass look_at= and radius=")
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.look_at = torch.as_tensor(look_at, dtype=torch.float32).reshape(3).to(self.device)
        self.radius = float(radius)
        self._look_host = tuple(float(v) for v in self.look_at.cpu())
        self.theta_range, self.phi_range = tuple(theta_range), tuple(phi_range)
        self.training = training
        self.num_rays = num_rays if training else -1
        self.full_H, self.full_W = int(H), int(W)
        s = 1.0
        if self.num_rays > 0:
            s = float(np.nan_to_num(np.sqrt(self.full_H * self.full_W / self.num_rays), nan=1.0))
        self.H, self.W = int(self.full_H / s), int(self.full_W / s)
        self.intrinsics = np.asarray([float(v) for v in intrinsics], dtype=np.float64) / s
        self.rays_per_batch = self.H * self.W
        self.n_val, self.epoch_length = int(n_val), int(epoch_length)
        self._init_sampling(seed)

    def __len__(self):
        return self.epoch_length if self.training else self.n_val

    def collate(self, index, generator=None):
        """SealNeRF/provider.py:154-178, the torch route: len(index) random poses (`rand_poses`) and the rays of their whole
        rH x rW frames (`get_rays`); not training: + `images_shape`, so that proxy_truth_data reshapes the targets to frames"""
        B = len(index)
        poses = rand_poses(B, self.device, radius=self.radius, theta_range=self.theta_range, phi_range=self.phi_range,
                           look_at=self.look_at, generator=generator)
        rays = get_rays(poses, self.intrinsics, self.H, self.W, -1)
        out = {"H": self.H, "W": self.W, "rays_o": rays["rays_o"], "rays_d": rays["rays_d"]}
        if not self.training:
            out["images_shape"] = [B, self.H, self.W, 3]
        return out

    def sample(self, index, out=None):
        """the batch of `collate(index)` drawn on the GPU in one launch (s3d_orbit_rays): len(index) poses keyed by (`seed`,
        the dataset's device-side step number, slot) and their frames' rays written into `out` (rays_o, rays_d
        [B, rH rW, 3], poses [B, 4, 4] fp32; missing entries are allocated) — the static inputs of a graph-replayed step
        (GraphedSealTrainer.train_step_random).  Also returns `poses`.  Ranks of a data-parallel run use different seeds."""
        import s3d_hip
        if self.device.type != "cuda":
            raise RuntimeError("sample() runs on the GPU: the dataset's device must be one (use collate() on the CPU)")
        B, n, dev = len(index), self.rays_per_batch, self.device
        if self._ctl is None:
            self._ctl = torch.zeros(2, dtype=torch.int32, device=dev)
        out = dict(out or {})
        for name, shape in (("rays_o", (B, n, 3)), ("rays_d", (B, n, 3)), ("poses", (B, 4, 4))):
            if out.get(name) is None:
                out[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        s3d_hip.RaySampleBackend.orbit_rays(B, self.H, self.W, self.intrinsics, out["rays_o"], out["rays_d"], out["poses"],
                                            look_at=self._look_host, radius=self.radius, theta_range=self.theta_range,
                                            phi_range=self.phi_range, seed=self.seed, ctl=self._ctl)
        res = {"H": self.H, "W": self.W, "rays_o": out["rays_o"], "rays_d": out["rays_d"], "poses": out["poses"]}
        if not self.training:
            res["images_shape"] = [B, self.H, self.W, 3]
        return res
