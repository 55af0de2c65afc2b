"""Ray/point-sharded data parallelism for the distillation / training step.

The reference has no live multi-GPU path (dead DDP hooks only, nerf/utils.py:330-333).  The path shards
naturally: every rank holds a full replica (tables 49 MB fp16, MLPs, bitfield), marches and shades its own
slice of the rays (or pretraining points), and the only exchange is ONE sum all-reduce per step over a flat
fp32 gradient bucket (hash-table + MLP grads, 98 MB for the Seal NGP net) — RCCL over xGMI on the GPU box
(backend "nccl"), gloo in the CPU tests.  Parameter `.grad`s are views into the bucket, so backward writes
straight into it and no gather/scatter copies are needed.  GradScaler consistency: gradients are reduced
BEFORE `unscale_`, so an overflow on any rank makes the reduced gradient non-finite on every rank and all
replicas skip the step together.
"""
import os

import torch
import torch.distributed as dist


def init_from_env(backend=None):
    """Initialise torch.distributed from torchrun's environment; returns (rank, world, local_rank)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def launched_by_torchrun():
    return "WORLD_SIZE" in os.environ and "RANK" in os.environ


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n, script, argv, need_gpus=True):
    """`python script --gpus n` typed WITHOUT torchrun: replace this process by
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node n ... script argv` (one rank per GPU, rendezvous on
    127.0.0.1 at a free port).  Refuses — non-zero exit, a sentence on stderr — when the node shows fewer than n GPUs:
    a run that quietly measured one GPU would be read as an n-GPU number.  Does not return."""
    import sys
    if need_gpus:
        seen = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if seen < n:
            sys.stderr.write(f"{os.path.basename(script)}: {n} GPUs requested, {seen} visible\n")
            sys.exit(2)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), script] + list(argv)
    sys.stdout.flush()
    sys.stderr.flush()
    os.execv(sys.executable, cmd)


def shard_slice(n, rank, world):
    """contiguous shard [lo, hi) of n units for `rank` (remainder spread over the first ranks)"""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class RayShardedDP:
    def __init__(self, group=None, average=True, force_collective=False, shard_occupancy=True):
        self.shard_occupancy = shard_occupancy  # False: every rank sweeps the whole grid, rank 0's result is broadcast
        self.group = group
        self.force_collective = force_collective  # issue the collectives even for world == 1 (single-GPU test of the path)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.average = average
        self._avg_ok = None
        self.flat = None
        self.params = []
        self.half_grads = []

    def register(self, model):
        """broadcast rank 0's replica and re-home every parameter gradient inside one flat bucket"""
        # tables whose gradient is handed over as an fp16 buffer (nerf/optim.py) are reduced in that buffer — half the
        # bytes on the wire; everything else is re-homed inside the flat fp32 bucket
        self.half_grads, seen = [], set()
        for p in model.parameters():
            h = getattr(p, "_s3d", None)
            if p.requires_grad and h is not None:
                buf = h.flat  # the optimizer's single flat buffer
                if buf.data_ptr() not in seen:
                    seen.add(buf.data_ptr())
                    self.half_grads.append(buf)
        self.params = [p for p in model.parameters() if p.requires_grad and getattr(p, "_s3d", None) is None]
        if self.world > 1:
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, src=0, group=self.group)
        total = sum(p.numel() for p in self.params)
        dev = next(model.parameters()).device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.flat[off:off + n].view_as(p)
            off += n
        if self.average and (self.world > 1 or self.force_collective):
            self._avg_supported()  # probe now (host read-back): never inside a graph capture
        if self.shard_occupancy and hasattr(model, "dist_shard"):
            model.dist_shard = self  # the occupancy sweep is split over the ranks (nerf/renderer.py)
        return self

    def _avg_supported(self):
        """ReduceOp.AVG on this group, probed once with a real (tiny) fp16 collective: every rank takes part, so every rank
        reaches the same verdict; anything but the exact mean falls back to SUM + divide"""
        if self._avg_ok is None:
            ok = False
            if dist.get_backend(self.group) == "nccl":
                try:
                    probe = torch.full((8,), 3.0, dtype=torch.float16, device="cuda")
                    dist.all_reduce(probe, op=dist.ReduceOp.AVG, group=self.group)
                    ok = bool((probe == 3.0).all().item())
                except RuntimeError:
                    ok = False
            self._avg_ok = ok
        return self._avg_ok

    # ---- chunked, asynchronous reduction ---------------------------------------------------------------------
    # One collective over the whole flat fp16 buffer finishes before the first parameter can be updated.  `grad_chunks()`
    # cuts the buffers at parameter boundaries into pieces of about `chunk_bytes`; `allreduce_grads_async()` issues one
    # collective per piece (async_op: they queue on the process group's communication stream, in order) and returns the
    # handles; the optimizer waits for piece k, updates the parameters inside it, and lets pieces k+1.. travel meanwhile
    # (nerf/optim.py: NativeGradScaler.step(chunks=...)).  xGMI is point to point (7 links per GPU): pieces of a few MB
    # keep every link busy while the update kernels of the previous piece run; tiny pieces would be latency bound.
    chunk_bytes = 8 << 20

    def grad_chunks(self):
        """[(buffer, start, stop)] element ranges of the registered gradient buffers, cut at parameter boundaries"""
        out = []
        for h in self.half_grads:
            cuts = sorted(set(getattr(h, "_s3d_param_cuts", [])) | {0, h.numel()})
            per = max(self.chunk_bytes // h.element_size(), 1)
            start = 0
            for c in cuts[1:]:
                if c - start >= per or c == h.numel():
                    # a parameter larger than the piece size is itself split evenly (a hash table is 24 MB)
                    n = max((c - start + per - 1) // per, 1)
                    step = ((c - start + n - 1) // n + 7) // 8 * 8
                    a = start
                    while a < c:
                        out.append((h, a, min(a + step, c)))
                        a = min(a + step, c)
                    start = c
        if self.flat is not None and self.flat.numel():
            out.append((self.flat, 0, self.flat.numel()))
        return out

    def allreduce_grads_async(self):
        """issue the reduction piece by piece; returns [(buffer, start, stop, work)] in issue order (work.wait() before use)"""
        if self.world == 1 and not self.force_collective:
            return []
        self._rehome_grads()
        fused_avg = self.average and self._avg_supported()
        op = dist.ReduceOp.AVG if fused_avg else dist.ReduceOp.SUM
        handles = []
        for buf, a, b in self.grad_chunks():
            view = buf[a:b]
            work = dist.all_reduce(view, op=op, group=self.group, async_op=True)
            handles.append((buf, a, b, work, not fused_avg and self.average and self.world > 1))
        return handles

    def capture_supported(self):
        """Can this group's all-reduce be recorded into a HIP graph and replayed?  Probed once with a throw-away graph holding
        one tiny collective (every rank runs the probe at the same point of its program, so every rank reaches the same
        verdict): RCCL supports stream capture, gloo does not."""
        if getattr(self, "_capture_ok", None) is None:
            ok = False
            if dist.is_initialized() and dist.get_backend(self.group) == "nccl" and torch.cuda.is_available():
                try:
                    probe = torch.full((256,), 2.0, dtype=torch.float16, device="cuda")
                    dist.all_reduce(probe, op=dist.ReduceOp.SUM, group=self.group)  # (communicator warm before the capture)
                    probe.fill_(2.0)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        dist.all_reduce(probe, op=dist.ReduceOp.SUM, group=self.group)
                        probe.add_(0.0)  # (a one-rank all-reduce records nothing: the probe graph is never an EMPTY graph)
                    probe.fill_(2.0)
                    g.replay()
                    torch.cuda.synchronize()
                    ok = bool((probe == 2.0 * self.world).all().item())
                    del g
                except Exception:  # noqa: BLE001  (any failure = not supported; the two-graph path is taken)
                    ok = False
            self._capture_ok = ok
        return self._capture_ok

    def fused_avg(self):
        """True when the mean over the ranks comes out of the collective itself (RCCL AVG: a pre-multiplied sum that cannot
        overflow on the wire); False on the SUM + divide fallback (gloo, or AVG not available)"""
        return bool(self.average and self._avg_supported())

    def allreduce_flag(self, flag):
        """a device-side overflow flag: non-zero on any rank -> non-zero everywhere"""
        if self.world > 1 or self.force_collective:
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.group)

    def finish_chunk(self, handle):
        buf, a, b, work, divide = handle
        work.wait()
        if divide:
            buf[a:b].div_(self.world)

    def _rehome_grads(self):
        # safety: a grad that autograd re-allocated is copied back into its bucket slot
        off = 0
        for p in self.params:
            n = p.numel()
            slot = self.flat[off:off + n]
            if p.grad is None:
                slot.zero_()
                p.grad = slot.view_as(p)
            elif p.grad.data_ptr() != slot.data_ptr():
                slot.copy_(p.grad.reshape(-1))
                p.grad = slot.view_as(p)
            off += n

    # ---- sharded evaluation with an all-gather ------------------------------------------------------------------
    def shard_rows(self, n):
        """this rank's contiguous slice [lo, hi) of n rows"""
        return shard_slice(n, self.rank, self.world)

    def all_gather_rows(self, local, n):
        """rows [lo, hi) computed by every rank -> the full [n, ...] tensor on every rank (ranks hold unequal slices:
        padded to the largest, gathered, trimmed)"""
        if self.world == 1 and not self.force_collective:
            return local
        per = (n + self.world - 1) // self.world
        pad = torch.zeros((per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        pad[:local.shape[0]] = local
        parts = [torch.empty_like(pad) for _ in range(self.world)]
        dist.all_gather(parts, pad, group=self.group)
        out = []
        for r, part in enumerate(parts):
            lo, hi = shard_slice(n, r, self.world)
            out.append(part[:hi - lo])
        return torch.cat(out, dim=0)

    def sharded_map(self, fn, *tensors):
        """fn on this rank's row slice of every tensor, results all-gathered: the full result on every rank.  fn may return a
        tensor or a tuple of tensors (first dimension = rows)."""
        n = tensors[0].shape[0]
        lo, hi = self.shard_rows(n)
        res = fn(*[t[lo:hi] for t in tensors])
        if isinstance(res, (tuple, list)):
            return tuple(self.all_gather_rows(r.contiguous(), n) for r in res)
        return self.all_gather_rows(res.contiguous(), n)

    def sharded_render(self, model, rays_o, rays_d, **kwargs):
        """a full frame (teacher proxy render, evaluation) split into contiguous pixel ranges, one per rank;
        image + depth all-gathered (640,000 rays x 16 B = 10 MB per frame)"""
        ro, rd = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)

        def part(o, d):
            out = model.render(o.contiguous(), d.contiguous(), **kwargs)
            return out["image"].reshape(-1, 3), out["depth"].reshape(-1)
        image, depth = self.sharded_map(part, ro, rd)
        return {"image": image.view(*rays_o.shape[:-1], 3), "depth": depth.view(*rays_o.shape[:-1])}

    def allreduce_grads(self, scaler=None):
        """blocking form: every piece issued, then awaited (RCCL averages inside the collective — pre-multiplied sum: no
        divide pass, and the fp16 bucket of loss-scaled gradients cannot overflow in the sum of `world` ranks; gloo (CPU
        tests) has no AVG: SUM + divide)"""
        for h in self.allreduce_grads_async():
            self.finish_chunk(h)

    def sync_extra_state(self, model):
        """keep the occupancy state identical on all replicas after `update_extra_state` (RNG differs per rank).  A model
        whose occupancy sweep is itself sharded (`model.dist_shard`, nerf/renderer.py) already holds identical grids: only
        the sample budget is agreed on."""
        if (self.world == 1 and not self.force_collective) or not getattr(model, "cuda_ray", False):
            return
        if getattr(model, "dist_shard", None) is self:
            t = torch.tensor([float(model.mean_count)], device=model.density_grid.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            model.mean_count = int(t[0].item())
            return
        dist.broadcast(model.density_grid, src=0, group=self.group)
        dist.broadcast(model.density_bitfield, src=0, group=self.group)
        # sample budget: the largest running mean over the ranks (each rank marches its own rays), density: rank 0's
        t = torch.tensor([float(model.mean_count), float(model.mean_density) if self.rank == 0 else float("-inf")],
                         device=model.density_grid.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        model.mean_count, model.mean_density = int(t[0].item()), float(t[1].item())

    def all_reduce_scalar(self, value, op="sum"):
        if self.world == 1:
            return value
        t = torch.tensor([float(value)], dtype=torch.float64, device=self.flat.device if self.flat is not None else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM, group=self.group)
        return float(t.item())
