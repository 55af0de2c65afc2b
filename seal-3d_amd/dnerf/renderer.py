"""D-NeRF renderer (dnerf/renderer.py of the reference): the NGP renderer with a time axis on the occupancy grid.

`density_grid` [T, cascade, H^3], `density_bitfield` [T, cascade H^3 / 8] and `times` [T, 1, 1] = (arange(T) + 0.5) / T are the
reference's buffers (checkpoint keys); T = `time_size`, the reference's constant 64 by default.  A rendering at `time` marches
slot floor(time T) (clamped) of the bitfield through the base class's `run_cuda` / `run`: the slot's bitfield — a contiguous
view — stands in for `density_bitfield` and the time is bound for the network's calls while the base method runs, so the
marchers, the compositing and the inference loop are the NGP backbone's own code."""
import contextlib
import math

import numpy as np
import torch

import raymarching
from nerf.renderer import NeRFRenderer as _NgpRenderer
from nerf.renderer import _meshgrid


class NeRFRenderer(_NgpRenderer):
    _bound_time = None
    _deform_out = None
    _deform_reg = None
    _last_deform = None

    def __init__(self, bound=1, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1, time_size=64,
                 **kwargs):
        super().__init__(bound, cuda_ray=False, density_scale=density_scale, min_near=min_near, density_thresh=density_thresh,
                         bg_radius=bg_radius, **kwargs)
        self.time_size = int(time_size)
        self.cuda_ray = cuda_ray
        if cuda_ray:
            T, H3 = self.time_size, self.grid_size ** 3
            self.register_buffer("density_grid", torch.zeros(T, self.cascade, H3))
            self.register_buffer("density_bitfield", torch.zeros(T, self.cascade * H3 // 8, dtype=torch.uint8))
            self.mean_density = 0
            self.iter_density = 0
            self.register_buffer("times", ((torch.arange(T, dtype=torch.float32) + 0.5) / T).view(-1, 1, 1))
            self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
            self.mean_count = 0
            self.local_step = 0
        # the occupancy update's random draws (cell jitter, time jitter, the partial update's cells): a generator of the
        # model's own, so that two models seeded alike end with identical grids whatever else drew from torch's global stream
        self.sweep_seed = 0x5EA13D
        self._sweep_gen = None

    def forward(self, x, d, t=None):
        raise NotImplementedError()

    def density(self, x, t=None):
        raise NotImplementedError()

    def slot_of(self, time):
        """the occupancy slot of `time`: floor(time T) clamped to [0, T - 1] (dnerf/renderer.py:285).  A Python number or a CPU
        tensor is resolved on the host; a GPU tensor costs the one read-back the reference's `density_bitfield[t]` costs."""
        if torch.is_tensor(time):
            time = float(time.reshape(-1)[0])
        return int(min(max(math.floor(np.float32(time) * np.float32(self.time_size)), 0), self.time_size - 1))

    @contextlib.contextmanager
    def _at_time(self, time, slot):
        """the base renderer's view of this model at one time: the slot's bitfield as `density_bitfield`, the time bound for
        forward / density calls that do not name one"""
        full = self._buffers["density_bitfield"] if self.cuda_ray else None
        prev = self._bound_time
        self._bound_time = time
        if full is not None:
            self._buffers["density_bitfield"] = full[slot]
        try:
            yield
        finally:
            self._bound_time = prev
            if full is not None:
                self._buffers["density_bitfield"] = full

    def _time_value(self, time):
        """`time` as the [1, 1] fp32 tensor the network encodes (the reference passes the batch's [B, 1] with B == 1)"""
        if torch.is_tensor(time):
            return time.reshape(-1)[:1].reshape(1, 1).float()
        return torch.tensor([[float(time)]], dtype=torch.float32)

    def run_cuda(self, rays_o, rays_d, time, **kwargs):
        """dnerf/renderer.py:261-386: the base run_cuda on the bitfield of `time`'s slot; the training result carries `deform`"""
        t = self._time_value(time)
        self._deform_out = None
        with self._at_time(t.to(rays_o.device), self.slot_of(t if not t.is_cuda else time)):
            results = super().run_cuda(rays_o, rays_d, **kwargs)
        if self.training:
            results["deform"] = self._last_deform = self._deform_out  # (_last_deform: what dnerf/utils.py regularises)
        self._deform_out = None
        return results

    def run(self, rays_o, rays_d, time, **kwargs):
        """dnerf/renderer.py:129-258: the base sampling path with `time` passed to `density`; the result carries `deform`"""
        t = self._time_value(time).to(rays_o.device)
        kept = {}
        color = self.color

        def color_keeping_deform(x, d, mask=None, **dens):
            kept["deform"] = dens.get("deform")  # (the base method hands over every density output of the merged row: depth-sorted on its torch route, [coarse | fine] on its native one)
            return color(x, d, mask=mask, **dens)
        self.color = color_keeping_deform  # (an instance attribute in front of the class's method, for the base method's call)
        try:
            with self._at_time(t, 0):
                results = super().run(rays_o, rays_d, **kwargs)
        finally:
            del self.color
        results["deform"] = kept.get("deform")
        if self.training:
            self._last_deform = results["deform"]
        return results

    def render(self, rays_o, rays_d, time, staged=False, max_ray_batch=4096, **kwargs):
        """dnerf/renderer.py:558-591"""
        if self.cuda_ray:
            return self.run_cuda(rays_o, rays_d, time, **kwargs)
        if not staged:
            return self.run(rays_o, rays_d, time, **kwargs)
        B, N = rays_o.shape[:2]
        depth = torch.empty((B, N), device=rays_o.device)
        image = torch.empty((B, N, 3), device=rays_o.device)
        for b in range(B):
            for head in range(0, N, max_ray_batch):
                tail = min(head + max_ray_batch, N)
                part = self.run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], time[b:b + 1] if torch.is_tensor(time) else time,
                                **kwargs)
                depth[b:b + 1, head:tail] = part["depth"]
                image[b:b + 1, head:tail] = part["image"]
        return {"depth": depth, "image": image}

    # ------------------------------------------------------------------ occupancy grid with a time axis
    def reset_extra_state(self):
        super().reset_extra_state()
        self._sweep_gen = None

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """cells no training camera sees get density -1 in every time slot (dnerf/renderer.py:389-451)"""
        if not self.cuda_ray:
            return
        if isinstance(poses, np.ndarray):
            poses = torch.from_numpy(poses)
        B = poses.shape[0]
        fx, fy, cx, cy = intrinsic
        dev = self.density_grid.device
        axis = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
        count = torch.zeros_like(self.density_grid[0])
        poses = poses.to(dev)
        for xs in axis:
            for ys in axis:
                for zs in axis:
                    xx, yy, zz = _meshgrid(xs, ys, zs)
                    coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    indices = raymarching.morton3D(coords).long()
                    world = (2 * coords.float() / (self.grid_size - 1) - 1).unsqueeze(0)
                    for cas in range(self.cascade):
                        bound, hgs = self._cascade_geometry(cas)
                        cas_world = world * (bound - hgs)
                        for head in range(0, B, S):
                            tail = min(head + S, B)
                            cam = cas_world - poses[head:tail, :3, 3].unsqueeze(1)
                            cam = cam @ poses[head:tail, :3, :3]
                            mask = ((cam[:, :, 2] > 0)
                                    & (torch.abs(cam[:, :, 0]) < cx / fx * cam[:, :, 2] + hgs * 2)
                                    & (torch.abs(cam[:, :, 1]) < cy / fy * cam[:, :, 2] + hgs * 2)).sum(0).reshape(-1)
                            count[cas, indices] += mask
        self.density_grid[count.unsqueeze(0).expand_as(self.density_grid) == 0] = -1

    def _generator(self):
        dev = self.density_grid.device
        if self._sweep_gen is None or self._sweep_gen.device != dev:
            self._sweep_gen = torch.Generator(device=dev)
            self._sweep_gen.manual_seed(int(self.sweep_seed))
        return self._sweep_gen

    @torch.no_grad()
    def _query_cells_at(self, coords, cas, time, gen):
        """jittered cell centres of cascade `cas` at a time jittered by +- 0.5 / T -> density (dnerf/renderer.py:483-497)"""
        bound, hgs = self._cascade_geometry(cas)
        xyzs = 2 * coords.float() / (self.grid_size - 1) - 1
        cas_xyzs = xyzs * (bound - hgs)
        cas_xyzs += (self._rand(cas_xyzs.shape, gen, cas_xyzs) * 2 - 1) * hgs
        t = time + (self._rand(time.shape, gen, time) * 2 - 1) * (0.5 / self.time_size)
        return self.density(cas_xyzs, t)["sigma"].reshape(-1).detach() * self.density_scale

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128):
        """dnerf/renderer.py:453-555: all T slots in full for the first 16 updates, then H^3/4 uniform + H^3/4 occupied cells per
        slot and cascade until the 100th, then nothing but the decay-free re-pack; EMA-max, one bitfield per slot.  A host loop
        over the native calls of the NGP update."""
        if not self.cuda_ray:
            return
        dev = self.density_grid.device
        gen = self._generator()
        tmp_grid = -torch.ones_like(self.density_grid)
        if self.iter_density < 16:
            axis = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
            for t, time in enumerate(self.times):
                for xs in axis:
                    for ys in axis:
                        for zs in axis:
                            xx, yy, zz = _meshgrid(xs, ys, zs)
                            coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                            indices = raymarching.morton3D(coords).long()
                            for cas in range(self.cascade):
                                tmp_grid[t, cas, indices] = self._query_cells_at(coords, cas, time, gen).to(tmp_grid.dtype)
        elif self.iter_density < 100:
            N = self.grid_size ** 3 // 4
            for t, time in enumerate(self.times):
                for cas in range(self.cascade):
                    coords = self._randint(self.grid_size, (N, 3), gen, dev)
                    indices = raymarching.morton3D(coords).long()
                    occ = torch.nonzero(self.density_grid[t, cas] > 0).squeeze(-1)
                    pick = self._randint(occ.shape[0], [N], gen, dev, torch.long)
                    occ = occ[pick]
                    occ_coords = raymarching.morton3D_invert(occ)
                    indices = torch.cat([indices, occ], dim=0)
                    coords = torch.cat([coords, occ_coords], dim=0)
                    tmp_grid[t, cas, indices] = self._query_cells_at(coords, cas, time, gen).to(tmp_grid.dtype)
        valid = (self.density_grid >= 0) & (tmp_grid >= 0)
        self.density_grid[valid] = torch.maximum(self.density_grid[valid] * decay, tmp_grid[valid])
        self.mean_density = torch.mean(self.density_grid.clamp(min=0)).item()
        self.iter_density += 1
        thresh = min(self.mean_density, self.density_thresh)
        for t in range(self.time_size):
            raymarching.packbits(self.density_grid[t], thresh, self.density_bitfield[t])
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0
