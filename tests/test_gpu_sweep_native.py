"""GPU: the occupancy-grid update in native launches without a host round trip (csrc/raymarching.hip: k_sweep_partials,
k_sweep_scan, k_sweep_draw_native, k_sweep_tail, k_packbits_record; NeRFRenderer.partial_grid_update_device /
finish_extra_state; GraphedTrainer._maybe_update_extra_state).

Grid sizes H = 16 and 32, i.e. N = H^3 / 4 = 1,024 and 8,192 draws per stream and 4 and 32 cell blocks of 1,024: the first
draw is one full workgroup, the second eight.  Cascade 0 and 1 (the jitter key and the geometry change with the cascade)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEV = "cuda"
KEY = 0x5EA1


def _grid(H, kind):
    H3 = H ** 3
    g = torch.Generator(device=DEV).manual_seed(H)
    if kind == "random":  # ~7 % of the cells > 0, some never-seen cells (-1), exact zeros
        grid = torch.rand(H3, device=DEV, generator=g)
        grid[grid < 0.93] = 0
        grid[5:40] = -1
    elif kind == "one":
        grid = torch.zeros(H3, device=DEV)
        grid[:9] = -1
        grid[H3 // 3 + 5] = 0.5
    elif kind == "none":
        grid = torch.zeros(H3, device=DEV)
        grid[::7] = -1
    else:
        grid = torch.full((H3,), 2.0, device=DEV)
    return grid


def _streams(N, seed):
    """two sorted streams as NeRFRenderer._sorted_uniform makes them"""
    from nerf.renderer import NeRFRenderer
    torch.manual_seed(seed)
    return NeRFRenderer._sorted_uniform(N, torch.device(DEV)), NeRFRenderer._sorted_uniform(N, torch.device(DEV))


def _draw(hip, grid, H, cas, step=5):
    bound = float(2 ** cas)
    tmp = torch.zeros(H ** 3, device=DEV)
    step_t = torch.full((1,), step, dtype=torch.int32, device=DEV)
    su, so = _streams(H ** 3 // 4, 100 * H + cas)
    cells, xyzs = hip.RaymarchingBackend.sweep_draw_native(su, so, grid, H, bound, bound / H, tmp, KEY + cas, step_t)
    return cells, xyzs, su, so, tmp, step_t, bound


@pytest.mark.parametrize("cas", [0, 1])
@pytest.mark.parametrize("kind", ["random", "one", "none", "all"])
@pytest.mark.parametrize("H", [16, 32])
def test_occupied_picks_equal_searchsorted_and_the_rest_equals_the_stream_fed_draw(hip, H, kind, cas):
    """occupied half: the cells equal searchsorted(cumsum(grid > 0), pick, right=True) clamped, for the same pick (no occupied
    cell: the last cell); uniform half, cells and jittered positions: exactly what k_sweep_draw gives for the same streams;
    the launch also leaves tmp = -1"""
    H3, N = H ** 3, H ** 3 // 4
    grid = _grid(H, kind)
    cells, xyzs, su, so, tmp, step_t, bound = _draw(hip, grid, H, cas)
    assert bool((tmp == -1).all())
    csum = torch.cumsum(grid > 0, dim=0, dtype=torch.int32)
    pick = (so * csum[-1]).to(torch.int32)
    want = torch.searchsorted(csum, pick, right=True).clamp(max=H3 - 1)
    assert torch.equal(cells[N:].long(), want)
    if kind == "none":
        assert bool((cells[N:] == H3 - 1).all())
    elif kind == "one":
        assert bool((cells[N:] == H3 // 3 + 5).all())
    else:
        assert bool((grid[cells[N:].long()] > 0).all())
    old_cells, old_xyzs = hip.RaymarchingBackend.sweep_draw(su, so, csum, H, bound, bound / H, KEY + cas, step_t)
    assert torch.equal(cells, old_cells) and torch.equal(xyzs, old_xyzs)


@pytest.mark.parametrize("total_step", [0, 1, 16])
@pytest.mark.parametrize("C", [1, 2, 3])  # (3: the cell count is no power of two)
@pytest.mark.parametrize("H", [16, 32])
def test_tail_record_and_bitfield_equal_the_separate_launches(hip, H, C, total_step):
    """same grid, samples and counter ring through both routes: scatter / EMA-max / k_sweep_mean per cascade, `total / numel`,
    host min(), packbits, host sum  ==  scatter_update per cascade, ONE tail launch, packbits from the record — bit for bit"""
    R = hip.RaymarchingBackend
    H3, N = H ** 3, H ** 3 // 4
    g = torch.Generator(device=DEV).manual_seed(7 * H + C)
    grid0 = torch.stack([_grid(H, "random") * (1 + c) for c in range(C)])
    ring = torch.randint(1000, 400000, (16, 2), dtype=torch.int32, device=DEV, generator=g)
    sigma_block = (torch.rand(2 * N, 3, device=DEV, generator=g) * 3).half()  # the samples are a strided fp16 column
    sigma_block[::5] = 0
    for density_thresh in (0.01, 10.0):  # threshold = density_thresh / = mean
        old, new = grid0.clone(), grid0.clone()
        tmp = torch.empty(H3, device=DEV)
        partial = torch.zeros(C, R.sweep_partial_stride(), device=DEV)
        total = None
        for cas in range(C):
            su, so = _streams(N, H + cas)
            cells, _ = R.sweep_draw_native(su, so, new[cas], H, 1.0, 1.0 / H, tmp, KEY + cas, None)
            sigma = sigma_block[:, cas]
            part = R.sweep_update(old[cas], cells, sigma.contiguous(), 1.5, 0.95, None)
            total = part if total is None else total + part
            R.sweep_scatter_update(new[cas], cells, sigma, 1.5, 0.95, tmp, partial[cas])
        mean_old = total / old.numel()
        thresh_old = min(float(mean_old), density_thresh)
        bits_old = torch.zeros(C * H3 // 8, dtype=torch.uint8, device=DEV)
        R.packbits(old, C * H3 // 8, thresh_old, bits_old)
        count_old = int(ring[:total_step, 0].sum()) if total_step else 0

        record = torch.zeros(4, dtype=torch.int32, device=DEV)
        local_step = torch.full((1,), total_step, dtype=torch.int32, device=DEV)
        sweep_step = torch.full((1,), 41, dtype=torch.int32, device=DEV)
        bits_new = torch.zeros_like(bits_old)
        R.sweep_tail(partial, H3, density_thresh, ring, local_step, sweep_step, record)
        R.packbits_record(new, C * H3 // 8, record, bits_new)
        rec = record.cpu().numpy()
        assert torch.equal(old, new)
        assert rec.view(np.float32)[0].tobytes() == mean_old.cpu().numpy().tobytes()
        assert rec.view(np.float32)[1] == np.float32(thresh_old)
        assert int(rec.view(np.uint32)[2]) | (int(rec.view(np.uint32)[3]) << 32) == count_old
        assert torch.equal(bits_old, bits_new) and int(sweep_step) == 42
        assert 0 < int(np.unpackbits(bits_new.cpu().numpy()).sum()) < C * H3


def _trainer_setup():
    import bench
    import s3d_hip
    from nerf import network_ff, synthetic as syn
    from nerf.trainer import GraphedTrainer
    torch.manual_seed(0)
    model = network_ff.NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    _, bits = syn.lego_like_density_grid(seed=0)
    batches, _ = bench.make_batches(8, 2048, 0, torch.device("cuda"), s3d_hip.RaymarchingBackend, torch.from_numpy(bits).cuda(),
                                    syn.lego_like_boxes(0))
    return model, GraphedTrainer(model, 2048, lr=1e-2, fp16=True), batches


def test_trainer_updates_without_a_host_read_and_rechecks_its_budget_one_update_later(hip, monkeypatch):
    """48 steps across three updates (eager native, captured, replayed) with Tensor.item / Tensor.tolist /
    torch.cuda.synchronize raising inside _maybe_update_extra_state; mean_count / mean_density read afterwards equal a host
    recomputation from the ring and the grid of that update; a sample mean forced beyond the budget at one update re-captures
    the step at the next one"""
    model, tr, batches = _trainer_setup()
    state = {"inside": False, "updates": 0, "force": False}

    def guarded(name, fn):
        def wrapper(*a, **k):
            # (the one update that CAPTURES the graph enters torch.cuda.graph, which synchronizes by itself: the synchronize
            #  guard covers the eager and the replayed updates, the item / tolist guards all of them)
            capturing = name == "torch.cuda.synchronize" and tr.ues_warm and tr.ues_graph is not None and state["updates"] == 1
            if state["inside"] and not capturing:
                raise AssertionError(f"{name} inside _maybe_update_extra_state")
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(torch.Tensor, "item", guarded("Tensor.item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "tolist", guarded("Tensor.tolist", torch.Tensor.tolist))
    monkeypatch.setattr(torch.cuda, "synchronize", guarded("torch.cuda.synchronize", torch.cuda.synchronize))
    inner = tr._maybe_update_extra_state
    seen = {}

    def update():
        if not (model.cuda_ray and tr.global_step % tr.update_extra_interval == 0 and model.iter_density >= 16):
            return inner()
        if state["force"]:
            model.step_counter[:, 0] = 4 * tr.budget
        seen["ring"], seen["rows"] = model.step_counter.clone(), min(16, model.local_step)
        state["inside"] = True
        try:
            done = inner()
        finally:
            state["inside"] = False
        assert done
        seen["grid"] = model.density_grid.clone()
        seen["bits"] = model.density_bitfield.clone()
        state["updates"] += 1
        return done
    tr._maybe_update_extra_state = update

    def run(steps):
        for _ in range(steps):
            tr.train_step(*batches[tr.global_step % len(batches)])

    run(17)                   # two full sweeps (steps 0 and 16), eager
    model.iter_density = 16   # steady state from here on
    run(48)                   # updates at 32 (eager native), 48 (captured), 64 (replayed)
    assert state["updates"] == 3 and tr.ues_graph is not None and model.iter_density == 19
    assert model.extra_state_pending()
    mean_count, mean_density = model.mean_count, model.mean_density
    assert not model.extra_state_pending()
    assert seen["rows"] == 16 and mean_count == int(int(seen["ring"][:16, 0].sum()) / 16) and mean_count > 0
    want = float(seen["grid"].clamp(min=0).double().mean())
    assert abs(mean_density - want) <= 1e-5 * want and want > 0  # (fp32 block sums of 2 M cells against an fp64 mean)
    thresh = np.float32(min(mean_density, model.density_thresh))
    assert np.array_equal(np.unpackbits(seen["bits"].cpu().numpy(), bitorder="little"),
                          (seen["grid"].reshape(-1).cpu().numpy() > thresh).astype(np.uint8))

    # a jump of the sample mean beyond the budget, seen by the update at step 80, re-captures at the update of step 96
    run(15)
    assert not model.extra_state_pending() and tr.graph is not None
    state["force"] = True
    run(1)                    # the update at 80 checks the numbers of step 64 (read above already: the check is the trainer's
                              # own flag, not the record's) and files the forced mean; nobody reads it yet
    state["force"] = False
    captures = tr.n_captures
    run(15)
    assert tr.n_captures == captures and model.extra_state_pending()
    assert model.mean_count > tr.budget and not model.extra_state_pending()  # (a read in between, as a logger's: the check stays due)
    run(1)                    # top of the update at 96: sets the forced mean against the budget, drops the graph; the step re-captures
    assert tr.n_captures == captures + 1 and tr.graph is not None
    assert tr.budget == int(max(model.mean_count, 1) * tr.budget_factor) and model.mean_count < 4 * tr.budget
