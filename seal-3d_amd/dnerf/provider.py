"""In-memory D-NeRF training data (dnerf/provider.py of the reference): nerf.provider.NeRFDataset plus one time per frame."""
import torch

from nerf.provider import NeRFDataset


class DNeRFDataset(NeRFDataset):
    """`times` [n] or [n, 1]: a frame's time as given; the whole set is divided by `max + 1e-8` when its maximum exceeds 1
    (dnerf/provider.py:237-254).  A batch comes from ONE frame and carries that frame's time [1, 1]."""

    def __init__(self, images, poses, intrinsics, times, **kw):
        super().__init__(images, poses, intrinsics, **kw)
        times = torch.as_tensor(times, dtype=torch.float32).reshape(-1, 1)
        if times.shape[0] != len(self.poses):
            raise ValueError(f"DNeRFDataset: {times.shape[0]} times for {len(self.poses)} frames")
        if times.max() > 1:
            times = times / (times.max() + 1e-8)
        self.times = times.to(self.device)

    def _one_frame(self, index):
        idx = index.reshape(-1).tolist() if torch.is_tensor(index) else ([int(i) for i in index] if isinstance(index, (list, tuple)) else [int(index)])
        if len(idx) != 1:
            raise ValueError(f"DNeRFDataset: a batch comes from one frame (one time per rendering), got frames {idx}")
        return idx

    def collate(self, index, generator=None):
        idx = self._one_frame(index)
        out = super().collate(idx, generator=generator)
        out["time"] = self.times[idx]
        return out

    def sample(self, index, out=None):
        idx = self._one_frame(index)
        res = super().sample(idx, out=out)
        res["time"] = self.times[idx]
        return res
