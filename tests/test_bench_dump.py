"""`bench.py --dump-outputs DIR` (host side): the last timed step's results as float32 / float64 .npy files, at most 64 MB,
large tensors as the same seeded sample in every run; `--full` is off by default."""
import os
import sys

import numpy as np
import torch


def test_plain_run_is_the_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    args = bench.parse()
    assert args.steps == 7 and args.full is False and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "out"


def test_dump_outputs_writes_float_arrays_with_a_fixed_sample(tmp_path):
    import bench
    from nerf import network
    torch.manual_seed(0)
    model = network.NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
    model.step_counter[2] = torch.tensor([1234, 96], dtype=torch.int32)
    model.local_step = 3
    loss = torch.tensor(0.25)
    bench.dump_outputs(str(tmp_path / "a"), loss, model)
    bench.dump_outputs(str(tmp_path / "b"), loss, model)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    state = model.state_dict()
    assert set(names) == {"loss.npy", "step_counter_last.npy"} | {f"state.{k}.npy" for k in state}
    arrays = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for n in names:
        assert np.array_equal(arrays[n[:-4]], np.load(tmp_path / "b" / n))
    assert arrays["loss"] == np.float32(0.25)
    assert arrays["step_counter_last"].tolist() == [1234.0, 96.0]
    emb = state["encoder.embeddings"]
    assert emb.numel() > bench.DUMP_FULL_MAX
    idx = torch.randint(0, emb.numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0))
    assert np.array_equal(arrays["state.encoder.embeddings"], emb.reshape(-1)[idx].numpy())
    assert np.array_equal(arrays["state.sigma_net.0.weight"], state["sigma_net.0.weight"].numpy())
    assert np.array_equal(arrays["state.density_bitfield"], state["density_bitfield"].numpy().astype(np.float64))
