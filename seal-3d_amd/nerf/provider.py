"""In-memory training data of nerf/provider.py (reference): preloaded images, poses and intrinsics, the per-image error map
(nerf/provider.py:234-256) and the per-step batch (`collate`, :283-327).  Loading from disk (transforms.json, image decoding)
is outside the hot path: the frames are handed in.

Two ways to draw a batch:
  * `collate(index)`: the reference's torch sequence (nerf/synthetic.get_rays, error-map weighted when the map is on), CPU or GPU;
  * `sample(index, out=...)`: one launch of s3d_sample_train_rays on the GPU (csrc/raysample.hip) — cells drawn from the map by
    a device-side RNG whose step number advances on the device, rays formed and targets gathered straight into the caller's
    buffers (the static inputs of a graph-replayed step: GraphedTrainer.static_batch); RGBA frames are blended onto their
    per-pixel random background in the same launch."""
import torch

from .synthetic import get_rays

MAP_CELLS = 128 * 128


class DeviceSampling:
    """`sample()` over `poses`, `intrinsics`, `H`, `W`, `num_rays`, `images`, `depths` and `error_map` of the dataset"""

    depths = None

    def _init_sampling(self, seed):
        self.seed = int(seed) & 0xFFFFFFFF
        self._ctl = None
        self._arange = None

    def _index_tensor(self, index):
        """index -> int64 device tensor [B]; a single image or a contiguous run is a view of a cached arange (no copy)"""
        dev = self.poses.device
        if torch.is_tensor(index):
            return index.to(dev, torch.int64).reshape(-1)
        index = [int(i) for i in index] if isinstance(index, (list, tuple)) else [int(index)]
        if self._arange is None:
            self._arange = torch.arange(len(self.poses), dtype=torch.int64, device=dev)
        if index == list(range(index[0], index[0] + len(index))):
            return self._arange[index[0]:index[0] + len(index)]
        return torch.tensor(index, dtype=torch.int64, device=dev)

    def sample(self, index, out=None):
        """the batch of `collate(index)` drawn on the GPU in one launch (s3d_sample_train_rays).  `out`: dict of caller buffers
        to fill (rays_o, rays_d [B,N,3], images [B,N,3] fp32, inds, inds_coarse [B,N] int64, index [B] int64, depths [B,N]);
        missing entries are allocated.  With the map on, cells are drawn from it (exponential race: the distribution of
        torch.multinomial without replacement, winners in ascending cell order); otherwise pixels are uniform.  RGBA frames
        (nerf/utils.py:465-474) are blended in the same launch: `images` is the target on a per-pixel random background, which
        is returned as `bg_color` [B,N,3] (the dataset's `random_bg=False`, for a model with bg_radius > 0: blended onto 1, no
        `bg_color`).  The background's draws are keyed by `seed`: ranks of a data-parallel run use different seeds (so do the
        poses of sealnerf.provider.SealRandomDataset.sample, which replaces this method with one s3d_orbit_rays launch)."""
        import s3d_hip
        if not self.poses.is_cuda:
            raise RuntimeError("sample() runs on the GPU: the dataset's poses must live there (use collate() on the CPU)")
        if self.num_rays <= 0:
            raise RuntimeError("sample() draws training batches: num_rays must be > 0")
        rgba = self.images is not None and self.images.shape[-1] == 4
        random_bg = rgba and getattr(self, "random_bg", True)
        idx = self._index_tensor(index)
        B, N, dev = idx.numel(), self.num_rays, self.poses.device
        if self.error_map is not None and N > MAP_CELLS:
            raise ValueError(f"sample(): {N} rays exceed the {MAP_CELLS} cells of the error map")
        if self._ctl is None:
            self._ctl = torch.zeros(2, dtype=torch.int32, device=dev)
        out = dict(out or {})
        new = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
        out.setdefault("rays_o", new(B, N, 3))
        out.setdefault("rays_d", new(B, N, 3))
        out.setdefault("inds", new(B, N, dtype=torch.int64))
        if self.images is not None:
            out.setdefault("images", new(B, N, 3))
        if random_bg:
            out.setdefault("bg_color", new(B, N, 3))
        if self.depths is not None:
            out.setdefault("depths", new(B, N, 1))
        if self.error_map is not None:
            out.setdefault("inds_coarse", new(B, N, dtype=torch.int64))
            out.setdefault("index", idx)
        images = self.images.contiguous() if self.images is not None else None
        depths = self.depths.float().contiguous() if self.depths is not None else None
        out_index = out.get("index")
        s3d_hip.RaySampleBackend.sample_train_rays(
            self.error_map, idx, N, self.H, self.W, self.poses.float().contiguous(), self.intrinsics, out["rays_o"], out["rays_d"],
            out["inds"], out.get("inds_coarse"), images, depths, out.get("images"), out.get("depths"), self.seed, self._ctl,
            out_index=out_index if out_index is not None and out_index.data_ptr() != idx.data_ptr() else None,
            **(dict(rgba=True, random_bg=random_bg, out_bg=out["bg_color"] if random_bg else None) if rgba else {}))
        res = {"H": self.H, "W": self.W, "rays_o": out["rays_o"], "rays_d": out["rays_d"], "inds": out["inds"]}
        if self.images is not None:
            res["images"] = out["images"]
        if random_bg:
            res["bg_color"] = out["bg_color"]
        if self.depths is not None:
            res["depths"] = out["depths"]
        if self.error_map is not None:
            res["index"] = out["index"]
            res["inds_coarse"] = out["inds_coarse"]
        return res


class NeRFDataset(DeviceSampling):
    """images [n, H, W, 3|4] (fp32; held as fp16 with `fp16=True`, as the reference preloads them under `-O`), poses
    [n, 4, 4] cam2world, intrinsics (fx, fy, cx, cy).  `error_map=True` (training only): torch.ones(n, 128*128) on the
    device, the reference's per-image map of recent per-pixel loss (nerf/provider.py:234-256)."""

    def __init__(self, images, poses, intrinsics, num_rays=4096, error_map=False, device=None, training=True, fp16=False, seed=0,
                 random_bg=True):
        self.device = torch.device(device) if device is not None else poses.device
        self.training = training
        self.poses = poses.to(self.device).float()
        self.intrinsics = intrinsics
        self.images = None
        if images is not None:
            self.H, self.W = int(images.shape[1]), int(images.shape[2])
            self.images = images.to(torch.half if fp16 else torch.float).to(self.device)
        self.random_bg = random_bg  # RGBA frames: sample() blends onto a per-pixel random background (False: onto 1)
        self.num_rays = num_rays if training else -1
        self.error_map = torch.ones(len(self.poses), MAP_CELLS, dtype=torch.float, device=self.device) \
            if (training and error_map) else None
        self._init_sampling(seed)

    def __len__(self):
        return self.poses.shape[0]

    def collate(self, index, generator=None):
        """nerf/provider.py:283-327 for dataset poses: rays of `num_rays` pixels of images `index` (error-map weighted when the
        map is on), their colours, and — with the map — `index` and `inds_coarse` for the trainer's update.  RGBA frames come
        back with four channels: the caller blends them with nerf.trainer.rgba_targets"""
        B = len(index)
        poses = self.poses[index].to(self.device)
        error_map = None if self.error_map is None else self.error_map[index]
        rays = get_rays(poses, self.intrinsics, self.H, self.W, self.num_rays, error_map, generator=generator)
        results = {"H": self.H, "W": self.W, "rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "inds": rays["inds"]}
        if self.images is not None:
            images = self.images[index].to(self.device)
            if self.training:
                C = images.shape[-1]
                images = torch.gather(images.view(B, -1, C), 1, torch.stack(C * [rays["inds"]], -1))
            results["images"] = images
        if error_map is not None:
            results["index"] = index
            results["inds_coarse"] = rays["inds_coarse"]
        return results
