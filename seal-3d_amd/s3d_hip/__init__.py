"""s3d_hip — ctypes binding of libseal3d_hip.so (the MI355X product path).

This is the only module that touches the native library.  It exposes five
backend objects whose methods have the names and argument order of the
reference's pybind ``_backend`` modules (raymarching/src/bindings.cpp:6-17,
gridencoder/src/bindings.cpp:6-8, shencoder/src/bindings.cpp:6-7,
freqencoder/src/bindings.cpp:6-7, ffmlp/src/bindings.cpp:6-10), taking torch
tensors that live on the GPU, launching on torch's *current* HIP stream, and
raising ``RuntimeError`` on any non-zero return code.

There is NO CPU fallback: if the library is missing or a tensor is not on the
GPU the call fails loudly.
"""
import ctypes as C
import math
import os
import subprocess
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("S3D_HIP_LIB") or os.path.join(_HERE, "libseal3d_hip.so")  # override: kernel-tuning experiments
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

F32, F16 = 0, 1

# every symbol include/seal3d_hip.h declares
EXPORTS = [
    "s3d_last_error", "s3d_version",
    "s3d_near_far_from_aabb", "s3d_sph_from_ray", "s3d_morton3D", "s3d_morton3D_invert", "s3d_mip_levels", "s3d_packbits",
    "s3d_march_rays_train_workspace_size", "s3d_march_rays_train",
    "s3d_sweep_draw", "s3d_sweep_update_workspace_size", "s3d_sweep_update",
    "s3d_sweep_draw_native_workspace_size", "s3d_sweep_draw_native", "s3d_sweep_partial_stride", "s3d_sweep_scatter_update",
    "s3d_sweep_tail", "s3d_packbits_record",
    "s3d_composite_rays_train_forward", "s3d_composite_rays_train_backward", "s3d_composite_rays_train_loss",
    "s3d_march_rays", "s3d_composite_rays", "s3d_compact_alive_workspace_size", "s3d_compact_alive",
    "s3d_grid_level_scales", "s3d_grid_encode_forward", "s3d_grid_encode_forward_pair", "s3d_grid_corner_indices", "s3d_grid_encode_backward",
    "s3d_grid_encode_backward_workspace_size", "s3d_grid_encode_backward_control_size",
    "s3d_grad_total_variation",
    "s3d_sh_encode_forward", "s3d_sh_encode_backward", "s3d_freq_encode_forward", "s3d_freq_encode_backward", "s3d_freq_encode_pack_forward", "s3d_freq_encode_pack_backward",
    "s3d_ffmlp_forward", "s3d_ffmlp_inference", "s3d_ffmlp_ngp_pair_inference", "s3d_ffmlp_wgrad_reduce_pair", "s3d_ffmlp_backward_workspace_size", "s3d_ffmlp_backward",
    "s3d_ffmlp_fused_backward_supported",
    "s3d_ffmlp_allocate_splitk", "s3d_ffmlp_free_splitk",
    "s3d_grads_nonfinite", "s3d_adam_step", "s3d_adam_step_multi", "s3d_adam_advance", "s3d_scaler_update", "s3d_step_ring_push", "s3d_step_epilogue",
    "s3d_ngp_mid_forward", "s3d_ngp_mid_backward", "s3d_ngp_mid2_forward", "s3d_ngp_mid2_backward", "s3d_ngp_rgb_forward", "s3d_ngp_rgb_backward",
    "s3d_bg_mse_forward", "s3d_bg_mse_backward", "s3d_bg_targets", "s3d_l1_pair_workspace_size", "s3d_l1_pair_loss",
    "s3d_seal_bbox_map", "s3d_seal_map_color", "s3d_seal_map_color_image", "s3d_seal_brush_map", "s3d_seal_anchor_map", "s3d_grid_encode_backward_adam", "s3d_grid_encode_backward_adam_tail", "s3d_loss_terms_reduce", "s3d_vm_features_forward",
    "s3d_aabb_normalize", "s3d_weighted_abs_sum_workspace_size", "s3d_weighted_abs_sum", "s3d_pack_linear_chain", "s3d_unpack_linear_chain",
    "s3d_vm_backward_max_bins", "s3d_vm_backward_keys", "s3d_vm_backward_bins_workspace_size", "s3d_vm_backward_bins",
    "s3d_vm_backward_stage_bytes", "s3d_vm_transpose_factors",
    "s3d_vm_features_backward", "s3d_vm_color_forward", "s3d_vm_color_backward",
    "s3d_cp_transpose_lines", "s3d_cp_features_forward", "s3d_cp_color_forward", "s3d_cp_features_backward", "s3d_cp_color_backward",
    "s3d_cc_features_forward", "s3d_cc_color_forward", "s3d_cc_features_backward", "s3d_cc_color_backward",
    "s3d_composite_rays_train_loss_bg", "s3d_bg_targets_rays",
    "s3d_background_forward", "s3d_background_backward_workspace_size", "s3d_background_backward",
    "s3d_vm_background_forward", "s3d_vm_background_backward_workspace_size", "s3d_vm_background_backward",
    "s3d_sample_train_rays", "s3d_error_map_update", "s3d_sample_train_rays_rgba", "s3d_rgba_targets", "s3d_orbit_rays",
    "s3d_mc_workspace_bytes", "s3d_mc_count", "s3d_mc_emit",
    "s3d_dnerf_encode_forward", "s3d_dnerf_warp_grid_workspace_size", "s3d_dnerf_warp_grid_forward", "s3d_dnerf_split_grad",
    "s3d_dnerf_warp_backward",
    "s3d_dnerf_basis_mid_forward", "s3d_dnerf_basis_mid_workspace_size", "s3d_dnerf_basis_mid_backward",
    "s3d_dnerf_hyper_grid_forward", "s3d_dnerf_hyper_backward_workspace_size", "s3d_dnerf_hyper_grid_backward",
    "s3d_hier_max_samples", "s3d_hier_coarse_samples", "s3d_hier_upsample", "s3d_hier_weights", "s3d_hier_composite_forward",
    "s3d_hier_composite_backward",
    "s3d_mesh_sdf_tile", "s3d_mesh_sdf", "s3d_sdf_sample_points", "s3d_sdf_mape_workspace_size", "s3d_sdf_mape_forward_backward",
    "s3d_ema_update_multi", "s3d_ema_exchange_multi",
    "s3d_mesh_bvh_leaf", "s3d_mesh_bvh_stage", "s3d_mesh_sdf_bvh",
    "s3d_frame_rays", "s3d_preview_resolve", "s3d_mask_positions_workspace_bytes", "s3d_mask_positions_count", "s3d_mask_positions_emit",
]


def build(force=False, jobs=8):
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-s", f"-j{jobs}"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"seal3d HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (needs hipcc). There is no CPU fallback for the product path.")
        l = C.CDLL(LIB_PATH)
        l.s3d_last_error.restype = C.c_char_p
        l.s3d_version.restype = C.c_char_p
        for name in ("s3d_march_rays_train_workspace_size", "s3d_compact_alive_workspace_size",
                     "s3d_ffmlp_backward_workspace_size", "s3d_grid_encode_backward_workspace_size",
                     "s3d_grid_encode_backward_control_size", "s3d_l1_pair_workspace_size",
                     "s3d_sweep_update_workspace_size", "s3d_sweep_draw_native_workspace_size", "s3d_vm_backward_bins_workspace_size", "s3d_vm_backward_stage_bytes",
                     "s3d_weighted_abs_sum_workspace_size", "s3d_background_backward_workspace_size",
                     "s3d_vm_background_backward_workspace_size", "s3d_mc_workspace_bytes",
                     "s3d_dnerf_warp_grid_workspace_size", "s3d_dnerf_basis_mid_workspace_size", "s3d_dnerf_hyper_backward_workspace_size",
                     "s3d_sdf_mape_workspace_size", "s3d_mask_positions_workspace_bytes"):
            getattr(l, name).restype = C.c_size_t
        l.s3d_vm_backward_max_bins.restype = C.c_uint32
        l.s3d_grid_level_scales.restype = None
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = lib().s3d_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError("seal3d HIP backend needs GPU tensors (no CPU fallback in the product path)")
    if not t.is_contiguous():
        raise RuntimeError("seal3d HIP backend needs contiguous tensors")
    return C.c_void_p(t.data_ptr())


def _u(x):
    return C.c_uint32(int(x))


def _nv(t):
    """`n_valid` of seal3d_hip.h: None, or an int32 GPU tensor whose first element is the sample count"""
    if t is None:
        return C.c_void_p(0)
    if t.dtype != torch.int32 or not t.is_cuda:
        raise RuntimeError("n_valid must be an int32 GPU tensor (the ray marcher's counter)")
    return C.c_void_p(t.data_ptr())


def _live(t, B):
    """`live` of s3d_grid_encode_forward: None, or an fp32 GPU tensor [B, ...] whose first column marks live rows"""
    if t is None:
        return C.c_void_p(0), C.c_uint32(0)
    if t.dtype != torch.float32 or not t.is_cuda or t.shape[0] != B:
        raise RuntimeError("live must be an fp32 GPU tensor with one row per input row")
    return C.c_void_p(t.data_ptr()), C.c_uint32(t.stride(0) if t.dim() > 1 else 1)


# Inference counterpart of row_limit: the deltas tensor of the current march_rays chunk (zero rows = unused slots)
_LIVE_ROWS = None


class live_rows:
    def __init__(self, deltas):
        self.value = deltas

    def __enter__(self):
        global _LIVE_ROWS
        self.saved, _LIVE_ROWS = _LIVE_ROWS, self.value
        return self

    def __exit__(self, *exc):
        global _LIVE_ROWS
        _LIVE_ROWS = self.saved
        return False


def active_live_rows(B):
    t = _LIVE_ROWS
    if t is not None and t.shape[0] == int(B) and t.dtype == torch.float32 and t.is_cuda:
        return t
    return None


# The padded sample batch of the current training render: (counter tensor, rows of the padded buffers).  The renderer
# announces it around the network call; a network whose whole sample path is native picks it up with
# `active_row_limit(B)` and hands it to every kernel explicitly (forward AND backward), so the work follows the samples.
_ROW_LIMIT = None


class row_limit:
    def __init__(self, counter, rows):
        self.value = (counter, int(rows))

    def __enter__(self):
        global _ROW_LIMIT
        self.saved, _ROW_LIMIT = _ROW_LIMIT, self.value
        return self

    def __exit__(self, *exc):
        global _ROW_LIMIT
        _ROW_LIMIT = self.saved
        return False


def active_row_limit(B):
    """the announced counter when it describes a batch of exactly B rows, else None"""
    if _ROW_LIMIT is not None and _ROW_LIMIT[1] == int(B):
        return _ROW_LIMIT[0]
    return None


class StepTail:
    """The small launches that end a training step, collected while the step is issued so that the hash table's backward — the
    last node of the step — can run them inside its own two launches (GridBackend.grid_encode_backward_adam_tail).  A trainer
    opens one per step (nerf/trainer.py: Trainer.fuse_step_tail); producers file their part instead of launching it:
      loss     raymarching: the sum of the criterion's per-ray terms          (workspace, N, with_depth, depth_weight, loss)
      reduce   ffmlp: the weight-gradient reduce of the two networks           (a, b) of FFMLPBackend.wgrad_reduce_pair
      adam     nerf/optim.py: the update of the parameters in `adam_params`    built by `adam_items` when the table's backward runs
      epilogue nerf/optim.py: the scaler's update (+ the trainer's ring push)  arguments of scaler_update / step_epilogue
    `armed`: a table's backward will take the tail (set by the trainer once exactly one table is armed); until then only the loss
    may be filed.  `flush()` issues whatever was filed and not taken as its ordinary launches.  The holder keeps every tensor it
    was handed alive until then: under graph capture a freed block would be handed to the next allocation."""
    current = None

    def __init__(self):
        self.loss = self.reduce = self.epilogue = None
        self.adam_params, self.adam_items, self.on_applied = [], None, None
        self.armed = False
        self.accept_loss = False  # the step reads the loss value only after the table's backward (no regularizer is added to it)
        self.applied = 0  # TAIL_* bits of the parts that ran inside the table's backward

    def take(self):
        """the `tail` dict of grid_encode_backward_adam_tail; what it names is issued by that call, one way or the other"""
        t = dict(loss=self.loss, reduce=self.reduce)
        items = self.adam_items(self.adam_params) if (self.adam_items is not None and self.adam_params) else None
        if items:
            t["adam"] = items
        if self.epilogue is not None and (items or not self.adam_params) and self.epilogue[0](self.adam_params):
            t["epilogue"] = self.epilogue[1]
        self.loss = self.reduce = None
        return t

    def done(self, parts):
        self.applied = parts
        if self.on_applied is not None:
            self.on_applied(self, parts)

    def flush(self):
        if self.reduce is not None:
            FFMLPBackend.wgrad_reduce_pair(*self.reduce)
        if self.loss is not None:
            RaymarchingBackend.loss_terms_reduce(*self.loss)
        self.loss = self.reduce = None

    def close(self):
        self.flush()
        if StepTail.current is self:
            StepTail.current = None


class Handover:
    """What a parameter carries because a nerf.optim.NativeAdam adopted it: `p._s3d` is one of these, or p is not adopted.  Made
    whole by the adoption (NativeAdam.__init__, PackedWeights.adopt), so nothing of an earlier optimizer or scaler survives one.
      grad, flat, flat_range    the fp16 gradient the backward kernels write, the optimizer's flat buffer and p's elements of it
      half, half_version        the fp16 copy the update launch maintains and the `p._version` it was made for
      touched, consumed         written since the last clear / read (and cleared) by a step since: host-side flags
      unchecked                 a torch op wrote `grad`: the scaler checks the buffer itself
      found_inf                 the attached scaler's flag, raised by the kernels that write `grad` (NativeGradScaler.attach)
      arm, fused_done           arguments of the update a table's backward applies itself (arm_fused_tables) / it did so
      pending                   forward passes that took this table into an autograd graph and whose backward has not run yet
                                (gridencoder.grid: note_table_use / _table_backward; the optimizer's zero_grad() and step() start it over)"""
    __slots__ = ("grad", "flat", "flat_range", "half", "half_version", "touched", "consumed", "unchecked", "found_inf", "arm",
                 "fused_done", "pending")

    def __init__(self, grad=None, flat=None, flat_range=None, half=None, half_version=None):
        self.grad, self.flat, self.flat_range, self.half, self.half_version = grad, flat, flat_range, half, half_version
        self.touched = self.consumed = self.unchecked = self.fused_done = False
        self.found_inf = self.arm = None
        self.pending = 0

    def fresh_half(self, p):
        """the fp16 copy while it is p's current value, else None (somebody wrote the parameter through torch)"""
        return self.half if self.half_version == p._version else None

    @property
    def dirty(self):
        """written since the last clear and not consumed by a step"""
        return self.touched and not self.consumed


def _shadow2(shadows):
    """(planes_t, lines_t) pointer arrays of VmBackend.transpose_factors()' result, or two NULLs"""
    if shadows is None:
        return None, None
    ptr3 = C.c_void_p * 3
    return ptr3(*[t.data_ptr() for t in shadows[0]]), ptr3(*[t.data_ptr() for t in shadows[1]])


def _shadow1(shadows):
    """planes_t pointer array of VmBackend.transpose_factors()' result, or NULL"""
    return (_shadow2(shadows)[0],)


def _f(x):
    return C.c_float(float(x))


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise RuntimeError(f"seal3d HIP backend: unsupported dtype {t.dtype} (float32/float16 only)")


def _need(t, dtype, name):
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")


# The four parts of a step's tail (StepTail), each validated in one place: its stand-alone entry point passes the result on as C
# arguments, GridBackend.grid_encode_backward_adam_tail files it in the s3d_step_tail.  `who`: the caller, for the messages.

def _reduce_job_args(job, who):
    """one job of FFMLPBackend.wgrad_reduce_pair: (workspace, B, input_dim, hidden_dim, num_layers, grad_weights, accumulate, found_inf)"""
    ws, B, input_dim, hidden_dim, num_layers, grad_weights, accumulate, found_inf = job
    _need(grad_weights, torch.float16, f"{who}: grad_weights")
    return (_p(ws), _u(B), _u(input_dim), _u(hidden_dim), _u(num_layers), _p(grad_weights), C.c_int(int(bool(accumulate))),
            _p(found_inf))


def _loss_terms_args(workspace, N, with_depth, depth_weight, loss, who):
    """the arguments of RaymarchingBackend.loss_terms_reduce"""
    _need(workspace, torch.float32, f"{who}: workspace"); _need(loss, torch.float32, f"{who}: loss")
    if workspace.numel() < 4 * N:
        raise RuntimeError(f"{who}: the loss workspace holds 4N floats")
    return _p(workspace), _u(N), C.c_int(int(bool(with_depth))), _f(depth_weight), _p(loss)


def _scaler_update_args(scale, growth_tracker, found_inf, growth_factor, backoff_factor, growth_interval, adam_step, who):
    """the arguments of OptimBackend.scaler_update"""
    _need(scale, torch.float32, f"{who}: scale"); _need(growth_tracker, torch.int32, f"{who}: growth_tracker")
    if adam_step is not None:
        _need(adam_step, torch.float32, f"{who}: adam_step")
    return (_p(scale), _p(growth_tracker), _p(found_inf), _f(growth_factor), _f(backoff_factor), C.c_int32(int(growth_interval)),
            _p(adam_step))


def _ring_push_args(loss, counter, loss_ring, counter_ring, cursor, who):
    """the arguments of OptimBackend.step_ring_push, with the rings' sizes (ring, loss_slots) behind them"""
    _need(counter, torch.int32, f"{who}: counter"); _need(counter_ring, torch.int32, f"{who}: counter_ring")
    _need(cursor, torch.int32, f"{who}: cursor")
    if cursor.numel() < 2:
        raise RuntimeError(f"{who}: cursor is int32[2] = {{slot, running step number}}")
    if loss is not None:
        _need(loss, torch.float32, f"{who}: loss"); _need(loss_ring, torch.float32, f"{who}: loss_ring")
    ring = counter_ring.shape[0]
    if not counter_ring.is_contiguous() or counter_ring.numel() != 2 * ring or (loss is not None and loss_ring.numel() < 1):
        raise RuntimeError(f"{who}: rings must be contiguous [ring, 2] / [loss_slots]")
    slots = 0 if loss is None or loss_ring.numel() == ring else loss_ring.numel()
    return (_p(loss), _p(counter), _p(loss_ring if loss is not None else None), _p(counter_ring), _p(cursor), C.c_int32(ring),
            C.c_int32(slots))


def _background_workspace(size_fn, N, device, found_inf):
    """both background backward bindings: found_inf's dtype check, the workspace query -> (uint8 workspace on `device`, its c_size_t size)"""
    if found_inf is not None:
        _need(found_inf, torch.float32, "found_inf")
    nb = int(size_fn(_u(N)))
    return torch.empty(max(nb, 1), dtype=torch.uint8, device=device), C.c_size_t(nb)


class _Workspace:
    """Per-device, per-stream scratch owned by the binding (grown on demand, reused).  While the stream is being captured
    into a HIP graph the scratch is a plain temporary instead: a cached tensor would come out of THAT graph's private memory
    pool and dangle for every later caller once the graph is destroyed (torch captures every graph on the same stream)."""

    def __init__(self):
        self.buf = {}

    def get(self, nbytes, device):
        n = max(int(nbytes), 1 << 16)
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(n, dtype=torch.uint8, device=device)
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            if b is None and len(self.buf) >= 16:  # (streams come and go: drop the oldest entries)
                for k in list(self.buf)[:8]:
                    del self.buf[k]
            b = torch.empty(n, dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b


_ws = _Workspace()


class _ControlBlocks:
    """Zero-filled, self-cleaning control blocks of the binned grid backward (include/seal3d_hip.h: `control`), one per
    device, allocated OUTSIDE graph captures only: a block first requested while the stream is capturing would live in
    that graph's private pool (see _Workspace), so the call then runs without one (the library clears its control words
    with a launch of its own, as it does for any caller that passes none).  One block per device, not per stream: a
    captured step replays on whatever stream its owner picks, and the binding's callers issue their grid backwards in
    stream order (two of them running concurrently on different streams of one device would have to bring their own)."""

    def __init__(self):
        self.buf = {}
        self.retired = []  # smaller blocks that were replaced: never freed — a captured graph may still hold their address

    def get(self, nbytes, device):
        if nbytes <= 0:
            return None
        b = self.buf.get(device.index)
        if b is not None and b.numel() >= nbytes:
            return b
        if torch.cuda.is_current_stream_capturing():
            return None
        if b is not None:
            self.retired.append(b)  # (all-zero between calls like every control block; a few hundred KB)
        b = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
        self.buf[device.index] = b
        return b


_ctl = _ControlBlocks()


def level_scales(L, S, H):
    out = (C.c_float * int(L))()
    lib().s3d_grid_level_scales(_u(L), _f(S), _u(H), out)
    return list(out)


class RaymarchingBackend:
    """raymarching/src/raymarching.h:7-18"""

    @staticmethod
    def near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars, noises=None, noise_step=None, noise_key=0):
        _need(rays_o, torch.float32, "rays_o")
        if noises is not None:
            _need(noises, torch.float32, "noises")
            if noise_step is not None:
                _need(noise_step, torch.int32, "noise_step")
        _check(lib().s3d_near_far_from_aabb(_p(rays_o), _p(rays_d), _p(aabb), _u(N), _f(min_near), _p(nears),
                                            _p(fars), _p(noises), _p(noise_step), _u(int(noise_key) & 0xFFFFFFFF), _stream()),
               "near_far_from_aabb")

    @staticmethod
    def sweep_draw(u_uniform, u_occupied, occ_csum, H, bound, half_cell, noise_key=0, noise_step=None):
        """cells [2N] int32 + jittered positions [2N, 3] of one cascade's occupancy sweep (seal3d_hip.h)"""
        _need(u_uniform, torch.float64, "u_uniform"); _need(u_occupied, torch.float64, "u_occupied")
        _need(occ_csum, torch.int32, "occ_csum")
        N = u_uniform.numel()
        if u_occupied.numel() != N or occ_csum.numel() != H ** 3:
            raise RuntimeError("sweep_draw: u_uniform / u_occupied are [N], occ_csum is [H^3]")
        if noise_step is not None:
            _need(noise_step, torch.int32, "noise_step")
        cells = torch.empty(2 * N, dtype=torch.int32, device=u_uniform.device)
        xyzs = torch.empty(2 * N, 3, dtype=torch.float32, device=u_uniform.device)
        _check(lib().s3d_sweep_draw(_p(u_uniform), _p(u_occupied), _p(occ_csum), _u(N), _u(H), _f(bound), _f(half_cell),
                                    _u(int(noise_key) & 0xFFFFFFFF), _p(noise_step), _p(cells), _p(xyzs), _stream()), "sweep_draw")
        return cells, xyzs

    @staticmethod
    def sweep_update(density_grid, cells, sigma, density_scale, decay, step_counter=None):
        """EMA-max update of one cascade's density grid [H^3] (a contiguous fp32 view, in place) from the samples; returns the
        device scalar sum(max(grid, 0)) (seal3d_hip.h)"""
        _need(density_grid, torch.float32, "density_grid"); _need(cells, torch.int32, "cells")
        if sigma.dtype not in (torch.float16, torch.float32) or sigma.numel() != cells.numel():
            raise RuntimeError("sweep_update: sigma must be fp16 / fp32, one per cell sample")
        if step_counter is not None:
            _need(step_counter, torch.int32, "step_counter")
        n_cells = density_grid.numel()
        ws = _ws.get(lib().s3d_sweep_update_workspace_size(_u(n_cells)), density_grid.device)
        out = torch.empty((), dtype=torch.float32, device=density_grid.device)
        _check(lib().s3d_sweep_update(_p(density_grid), _u(n_cells), _p(cells), _p(sigma), C.c_int(_dt(sigma)), _u(cells.numel()),
                                      _f(density_scale), _f(decay), _p(ws), C.c_size_t(ws.numel()), _p(out), _p(step_counter),
                                      _stream()), "sweep_update")
        return out

    @staticmethod
    def sweep_draw_native(u_uniform, u_occupied, density_grid, H, bound, half_cell, tmp, noise_key=0, noise_step=None):
        """sweep_draw with the occupied cells found in per-block counts + bit masks of density_grid > 0 instead of a prefix array;
        also leaves tmp [H^3] = -1 (seal3d_hip.h).  Returns cells [2N] int32 and xyzs [2N, 3]."""
        _need(u_uniform, torch.float64, "u_uniform"); _need(u_occupied, torch.float64, "u_occupied")
        _need(density_grid, torch.float32, "density_grid"); _need(tmp, torch.float32, "tmp")
        H3, dev = int(H) ** 3, density_grid.device
        N = u_uniform.numel()
        if u_occupied.numel() != N or density_grid.numel() != H3 or tmp.numel() != H3:
            raise RuntimeError("sweep_draw_native: u_uniform / u_occupied are [N], density_grid and tmp [H^3]")
        if noise_step is not None:
            _need(noise_step, torch.int32, "noise_step")
        ws = _ws.get(lib().s3d_sweep_draw_native_workspace_size(_u(H)), dev)
        cells = torch.empty(2 * N, dtype=torch.int32, device=dev)
        xyzs = torch.empty(2 * N, 3, dtype=torch.float32, device=dev)
        _check(lib().s3d_sweep_draw_native(_p(u_uniform), _p(u_occupied), _p(density_grid), _u(N), _u(H), _f(bound), _f(half_cell),
                                           _u(int(noise_key) & 0xFFFFFFFF), _p(noise_step), _p(tmp), _p(cells), _p(xyzs), _p(ws),
                                           C.c_size_t(ws.numel()), _stream()), "sweep_draw_native")
        return cells, xyzs

    @staticmethod
    def sweep_partial_stride():
        return int(lib().s3d_sweep_partial_stride())

    @staticmethod
    def sweep_scatter_update(density_grid, cells, sigma, density_scale, decay, tmp, partial):
        """EMA-max update of one cascade's grid from (cells, sigma) through tmp (which the draw left at -1); sigma is a 1-D fp16 /
        fp32 tensor of any stride; partial [sweep_partial_stride()] receives the block sums of max(grid, 0) (seal3d_hip.h)"""
        _need(density_grid, torch.float32, "density_grid"); _need(cells, torch.int32, "cells")
        _need(tmp, torch.float32, "tmp"); _need(partial, torch.float32, "partial")
        if sigma.dtype not in (torch.float16, torch.float32) or sigma.dim() != 1 or sigma.numel() != cells.numel() or not sigma.is_cuda:
            raise RuntimeError("sweep_scatter_update: sigma must be a 1-D fp16 / fp32 GPU tensor, one per cell sample")
        if tmp.numel() != density_grid.numel() or partial.numel() < RaymarchingBackend.sweep_partial_stride():
            raise RuntimeError("sweep_scatter_update: tmp is [n_cells], partial [sweep_partial_stride()]")
        stride = sigma.stride(0) if sigma.numel() > 1 else 1
        if stride < 1:
            raise RuntimeError("sweep_scatter_update: sigma must have a positive stride")
        _check(lib().s3d_sweep_scatter_update(_p(density_grid), _u(density_grid.numel()), _p(cells), C.c_void_p(sigma.data_ptr()),
                                              C.c_int(_dt(sigma)), _u(stride), _u(cells.numel()), _f(density_scale), _f(decay),
                                              _p(tmp), _p(partial), _stream()), "sweep_scatter_update")

    @staticmethod
    def sweep_tail(partial, n_cells, density_thresh, step_ring, local_step, sweep_step, record):
        """mean / threshold / sample count of an update into `record` (int32 [4], 16 bytes; seal3d_hip.h)"""
        _need(partial, torch.float32, "partial"); _need(step_ring, torch.int32, "step_ring")
        _need(local_step, torch.int32, "local_step"); _need(record, torch.int32, "record")
        if partial.dim() != 2 or partial.shape[1] != RaymarchingBackend.sweep_partial_stride() or step_ring.shape != (16, 2) \
                or record.numel() != 4:
            raise RuntimeError("sweep_tail: partial is [cascades, sweep_partial_stride()], step_ring [16, 2], record int32 [4]")
        if sweep_step is not None:
            _need(sweep_step, torch.int32, "sweep_step")
        _check(lib().s3d_sweep_tail(_p(partial), _u(partial.shape[0]), _u(n_cells), _f(density_thresh), _p(step_ring),
                                    _p(local_step), _p(sweep_step), _p(record), _stream()), "sweep_tail")

    @staticmethod
    def packbits_record(grid, N, record, bitfield):
        """packbits with the threshold of a sweep_tail record (no host value in between)"""
        _need(grid, torch.float32, "grid"); _need(record, torch.int32, "record"); _need(bitfield, torch.uint8, "bitfield")
        if grid.numel() != 8 * int(N) or bitfield.numel() < int(N) or record.numel() != 4:
            raise RuntimeError("packbits_record: grid holds 8 N cells, bitfield N bytes, record int32 [4]")
        _check(lib().s3d_packbits_record(_p(grid), _u(N), _p(record), _p(bitfield), _stream()), "packbits_record")

    @staticmethod
    def sph_from_ray(rays_o, rays_d, radius, N, coords):
        _need(rays_o, torch.float32, "rays_o")
        _check(lib().s3d_sph_from_ray(_p(rays_o), _p(rays_d), _f(radius), _u(N), _p(coords), _stream()),
               "sph_from_ray")

    @staticmethod
    def morton3D(coords, N, indices):
        _need(coords, torch.int32, "coords")
        _check(lib().s3d_morton3D(_p(coords), _u(N), _p(indices), _stream()), "morton3D")

    @staticmethod
    def morton3D_invert(indices, N, coords):
        _need(indices, torch.int32, "indices")
        _check(lib().s3d_morton3D_invert(_p(indices), _u(N), _p(coords), _stream()), "morton3D_invert")

    @staticmethod
    def mip_levels(xyz, dt, H, Cc):
        """Test hook: (mip_from_pos [N], mip_from_dt [N]) of the marching kernels' cascade selection (raymarching.cu:42-54)."""
        _need(xyz, torch.float32, "xyz")
        _need(dt, torch.float32, "dt")
        N = xyz.shape[0]
        assert dt.shape[0] == N
        mp = torch.empty(N, dtype=torch.int32, device=xyz.device)
        md = torch.empty(N, dtype=torch.int32, device=xyz.device)
        _check(lib().s3d_mip_levels(_p(xyz), _p(dt), _u(N), _u(H), _u(Cc), _p(mp), _p(md), _stream()), "mip_levels")
        return mp, md

    @staticmethod
    def packbits(grid, N, density_thresh, bitfield):
        _need(grid, torch.float32, "grid")
        _check(lib().s3d_packbits(_p(grid), _u(N), _f(density_thresh), _p(bitfield), _stream()), "packbits")

    @staticmethod
    def march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, Cc, H, M, nears, fars, xyzs, dirs,
                         deltas, rays, counter, noises, aabb=None, min_near=0.0, noise_step=None, noise_key=0):
        """`aabb` (build extension): near_far_from_aabb is part of the call — nears / fars (and noises, with `noise_step`) are
        outputs (seal3d_hip.h)"""
        _need(rays_o, torch.float32, "rays_o")
        if aabb is not None:
            _need(aabb, torch.float32, "aabb"); _need(nears, torch.float32, "nears"); _need(fars, torch.float32, "fars")
        if noise_step is not None:
            _need(noise_step, torch.int32, "noise_step")
        nbytes = lib().s3d_march_rays_train_workspace_size(_u(N), _u(max_steps))
        ws = _ws.get(nbytes, rays_o.device)
        _check(lib().s3d_march_rays_train(_p(rays_o), _p(rays_d), _p(grid), _f(bound), _f(dt_gamma), _u(max_steps),
                                          _u(N), _u(Cc), _u(H), _u(M), _p(nears), _p(fars), _p(xyzs), _p(dirs),
                                          _p(deltas), _p(rays), _p(counter), _p(noises), _p(ws),
                                          C.c_size_t(ws.numel()), C.c_int(RaymarchingBackend._march_path), _p(aabb),
                                          _f(min_near), _p(noise_step), _u(int(noise_key) & 0xFFFFFFFF), _stream()),
               "march_rays_train")

    @staticmethod
    def composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image):
        for t, n in ((sigmas, "sigmas"), (rgbs, "rgbs"), (deltas, "deltas")):
            _need(t, torch.float32, n)
        _check(lib().s3d_composite_rays_train_forward(_p(sigmas), _p(rgbs), _p(deltas), _p(rays), _u(M), _u(N),
                                                      _f(T_thresh), _p(weights_sum), _p(depth), _p(image),
                                                      C.c_int(RaymarchingBackend._composite_path), _stream()),
               "composite_rays_train_forward")

    @staticmethod
    def composite_rays_train_backward(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image,
                                      M, N, T_thresh, grad_sigmas, grad_rgbs):
        for t, n in ((grad_image, "grad_image"), (grad_weights_sum, "grad_weights_sum"), (sigmas, "sigmas"), (rgbs, "rgbs"),
                     (deltas, "deltas")):
            _need(t, torch.float32, n)
        _check(lib().s3d_composite_rays_train_backward(_p(grad_weights_sum), _p(grad_image), _p(sigmas), _p(rgbs),
                                                       _p(deltas), _p(rays), _p(weights_sum), _p(image), _u(M),
                                                       _u(N), _f(T_thresh), _p(grad_sigmas), _p(grad_rgbs),
                                                       C.c_int(RaymarchingBackend._composite_path), _stream()),
               "composite_rays_train_backward")

    @staticmethod
    def _check_train_loss(name, M, N, gt_depth, grad_image, grad_weights_sum, exact, **tensors):
        """argument checks of composite_rays_train_loss / _loss_bg (`name`, for the messages): fp32 `tensors`, the `exact` ones [N,3]"""
        for n, t in tensors.items():
            _need(t, torch.float32, n)
        if (any(tensors[n].numel() != 3 * N for n in exact) or tensors["workspace"].numel() < 4 * N
                or tensors["grad_sigmas"].numel() < M or tensors["grad_rgbs"].numel() < 3 * M):
            raise RuntimeError(f"{name}: {' / '.join(exact)} [N,3], workspace >= 4N floats, grad_sigmas [M], grad_rgbs [M,3]")
        if gt_depth is not None:
            _need(gt_depth, torch.float32, "gt_depth")
            if gt_depth.numel() != N:
                raise RuntimeError(f"{name}: gt_depth holds one value per ray")
        if (grad_image is None) != (grad_weights_sum is None):
            raise RuntimeError(f"{name}: grad_image and grad_weights_sum come together")
        if RaymarchingBackend._composite_path != 0:
            raise RuntimeError(f"{name}: the fused launch exists for the wave-per-ray path only")

    @staticmethod
    def composite_rays_train_loss(sigmas, rgbs, deltas, rays, M, N, T_thresh, gt, bg_rgb, grad_loss, weights_sum, depth, image,
                                  grad_sigmas, grad_rgbs, loss, workspace, gt_depth=None, depth_weight=1.0, grad_image=None,
                                  grad_weights_sum=None, defer_reduce=False):
        """composite forward + background / MSE loss (announced upstream gradient `grad_loss`) + composite backward of one ray batch
        in one launch + a one-workgroup sum of the loss terms (seal3d_hip.h); workspace: 4N floats of scratch.  `defer_reduce`:
        the sum is left to a later loss_terms_reduce / step tail on the same workspace (`loss` is not written by this call)"""
        RaymarchingBackend._check_train_loss(
            "composite_rays_train_loss", M, N, gt_depth, grad_image, grad_weights_sum, ("gt",), sigmas=sigmas, rgbs=rgbs, deltas=deltas,
            gt=gt, grad_loss=grad_loss, loss=loss, workspace=workspace, grad_sigmas=grad_sigmas, grad_rgbs=grad_rgbs)
        bg = (C.c_float * 3)(*[float(v) for v in bg_rgb])
        _check(lib().s3d_composite_rays_train_loss(_p(sigmas), _p(rgbs), _p(deltas), _p(rays), _u(M), _u(N), _f(T_thresh), _p(gt), bg,
                                                   _p(grad_loss), _p(gt_depth), _f(depth_weight), _p(weights_sum), _p(depth), _p(image),
                                                   _p(grad_sigmas), _p(grad_rgbs), _p(grad_image), _p(grad_weights_sum),
                                                   _p(None if defer_reduce else loss), _p(workspace), _stream()), "composite_rays_train_loss")

    @staticmethod
    def loss_terms_reduce(workspace, N, with_depth, depth_weight, loss):
        """the one-workgroup sum a composite_rays_train_loss(defer_reduce=True) call left out (seal3d_hip.h)"""
        _check(lib().s3d_loss_terms_reduce(*_loss_terms_args(workspace, N, with_depth, depth_weight, loss, "loss_terms_reduce"), _stream()),
               "loss_terms_reduce")

    @staticmethod
    def composite_rays_train_loss_bg(sigmas, rgbs, deltas, rays, M, N, T_thresh, gt, bg, grad_loss, weights_sum, depth, image,
                                     grad_sigmas, grad_rgbs, grad_bg, loss, workspace, gt_depth=None, depth_weight=1.0,
                                     grad_image=None, grad_weights_sum=None, defer_reduce=False):
        """composite_rays_train_loss with a per-ray background bg [N,3] (device) and its gradient grad_bg [N,3] (seal3d_hip.h);
        grad_bg None: a background that needs no gradient (the random background of RGBA frames)"""
        with_grad = {} if grad_bg is None else {"grad_bg": grad_bg}
        RaymarchingBackend._check_train_loss(
            "composite_rays_train_loss_bg", M, N, gt_depth, grad_image, grad_weights_sum, ("gt", "bg") + tuple(with_grad), sigmas=sigmas,
            rgbs=rgbs, deltas=deltas, gt=gt, bg=bg, grad_loss=grad_loss, loss=loss, workspace=workspace,
            grad_sigmas=grad_sigmas, grad_rgbs=grad_rgbs, **with_grad)
        _check(lib().s3d_composite_rays_train_loss_bg(_p(sigmas), _p(rgbs), _p(deltas), _p(rays), _u(M), _u(N), _f(T_thresh), _p(gt),
                                                      _p(bg), _p(grad_loss), _p(gt_depth), _f(depth_weight), _p(weights_sum), _p(depth),
                                                      _p(image), _p(grad_sigmas), _p(grad_rgbs), _p(grad_image), _p(grad_weights_sum),
                                                      _p(grad_bg), _p(None if defer_reduce else loss), _p(workspace), _stream()),
               "composite_rays_train_loss_bg")

    zero_fills_march_rays = True  # march_rays(zero_unfilled=True): the kernel writes the zeros of the unfilled slots itself

    @staticmethod
    def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, Cc, H, grid,
                   nears, fars, xyzs, dirs, deltas, noises, n_alive_dev=None, n_rows_out=None, zero_unfilled=False):
        """n_alive_dev / n_rows_out (build extension): device-side alive count and the sample-row count it implies;
        zero_unfilled: xyzs / dirs / deltas arrive uninitialised, the kernel zeroes what it does not fill; noises may be None"""
        _need(rays_o, torch.float32, "rays_o")
        _check(lib().s3d_march_rays(_u(n_alive), _u(n_step), _p(rays_alive), _p(rays_t), _p(rays_o), _p(rays_d),
                                    _f(bound), _f(dt_gamma), _u(max_steps), _u(Cc), _u(H), _p(grid), _p(nears),
                                    _p(fars), _p(xyzs), _p(dirs), _p(deltas), _p(noises), _nv(n_alive_dev), _nv(n_rows_out),
                                    _u(xyzs.shape[0]), C.c_int(int(zero_unfilled)), _stream()), "march_rays")

    @staticmethod
    def composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth,
                       image, n_alive_dev=None):
        for t, n in ((image, "image"), (deltas, "deltas"), (weights_sum, "weights_sum"), (depth, "depth"), (rays_t, "rays_t")):
            _need(t, torch.float32, n)
        _check(lib().s3d_composite_rays(_u(n_alive), _u(n_step), _f(T_thresh), _p(rays_alive), _p(rays_t),
                                        _p(sigmas), _p(rgbs), _p(deltas), _p(weights_sum), _p(depth), _p(image),
                                        _nv(n_alive_dev), C.c_int(_dt(sigmas)), C.c_int(_dt(rgbs)), _stream()), "composite_rays")

    # kernel choice handed to the library with every call (`path` arguments of seal3d_hip.h); binding-side state for
    # tests / experiments — the library itself keeps no process-wide switches
    _march_path = 0
    _composite_path = 0

    @staticmethod
    def set_composite_path(path):
        """0 = wave-per-ray compositing, 1 = lane-per-ray (tests / experiments)"""
        RaymarchingBackend._composite_path = int(path)

    @staticmethod
    def set_march_path(path):
        """0 = auto, 1 = lane-per-ray kernels, 2 = wave-per-ray kernels, 3 = wave-per-ray without the single-cascade fast path (tests / experiments)"""
        RaymarchingBackend._march_path = int(path)

    # --- build extension (not in the reference's native surface) ---
    @staticmethod
    def compact_alive(rays_alive, n, out, n_out, n_in_dev=None):
        nbytes = lib().s3d_compact_alive_workspace_size(_u(n))
        ws = _ws.get(nbytes, rays_alive.device)
        _check(lib().s3d_compact_alive(_p(rays_alive), _u(n), _p(out), _p(n_out), _p(ws), C.c_size_t(ws.numel()),
                                       _nv(n_in_dev), _stream()), "compact_alive")


_level_rows_cache = {}  # id(tensor) -> (weakref, version, rows)


def _max_level_rows(offsets):
    """max rows of one level.  `offsets` is the module's registered buffer (built on the host, grid.py:104-112); the
    one-time read-back happens on the first backward, before any graph capture, and is cached per tensor object."""
    hit = _level_rows_cache.get(id(offsets))
    if hit is not None and hit[0]() is offsets and hit[1] == offsets._version:
        return hit[2]
    if torch.cuda.is_current_stream_capturing():
        return 0  # unknown: the library falls back to direct atomics
    o = offsets.detach().cpu()
    v = int((o[1:] - o[:-1]).max().item()) if o.numel() > 1 else 0
    if len(_level_rows_cache) > 256:
        for k in [k for k, h in _level_rows_cache.items() if h[0]() is None]:
            del _level_rows_cache[k]
    _level_rows_cache[id(offsets)] = (weakref.ref(offsets), offsets._version, v)
    return v


# the runs of C arguments that s3d_grid_encode_backward, _adam and _adam_tail have in common (seal3d_hip.h), in their order
def _bwd_tables(grad, inputs, embeddings, offsets, grad_embeddings, max_level_rows, B, D, Cc, L, S, H):
    return (_p(grad), _p(inputs), _p(embeddings), _p(offsets), _p(grad_embeddings), _u(max_level_rows), _u(B), _u(D), _u(Cc), _u(L),
            _f(S), _u(H))


def _bwd_options(gridtype, align_corners, interp, grad, ws, bound, n_valid):
    return (_u(gridtype), C.c_int(int(align_corners)), _u(interp), C.c_int(_dt(grad)), _p(ws), C.c_size_t(ws.numel()), _f(bound),
            _nv(n_valid))


def _bwd_flags(found_inf, ctl):
    return _p(found_inf), _p(ctl), C.c_size_t(ctl.numel() if ctl is not None else 0)


class GridBackend:
    """gridencoder/src/gridencoder.h:12-15"""

    supports_bound = True  # forward/backward accept raw coordinates + `bound` (normalisation fused into the kernels)

    @staticmethod
    def grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, Cc, L, S, H, dy_dx, gridtype, align_corners,
                            interp, bound=0.0, n_valid=None, live=None):
        _need(inputs, torch.float32, "inputs")
        _need(offsets, torch.int32, "offsets")
        if outputs.dtype != embeddings.dtype:
            raise RuntimeError("outputs must have the dtype of embeddings")
        _check(lib().s3d_grid_encode_forward(_p(inputs), _p(embeddings), _p(offsets), _p(outputs), _u(B), _u(D),
                                             _u(Cc), _u(L), _f(S), _u(H), _p(dy_dx), _u(gridtype),
                                             C.c_int(int(align_corners)), _u(interp), C.c_int(_dt(embeddings)),
                                             _f(bound), _nv(n_valid), *_live(live, B), _stream()), "grid_encode_forward")

    @staticmethod
    def grid_encode_forward_pair(inputs, emb_a, emb_b, offsets, out_a, out_b, B, D, Cc, L, S, H, gridtype, align_corners,
                                 interp, bound=0.0, n_valid=None, live=None):
        """two tables of one geometry on the same points in one launch (seal3d_hip.h: s3d_grid_encode_forward_pair)"""
        _need(inputs, torch.float32, "inputs")
        _need(offsets, torch.int32, "offsets")
        if not (out_a.dtype == emb_a.dtype == emb_b.dtype == out_b.dtype) or emb_a.shape != emb_b.shape:
            raise RuntimeError("grid_encode_forward_pair: both tables and both outputs share dtype and shape")
        _check(lib().s3d_grid_encode_forward_pair(_p(inputs), _p(emb_a), _p(emb_b), _p(offsets), _p(out_a), _p(out_b), _u(B), _u(D),
                                                  _u(Cc), _u(L), _f(S), _u(H), _u(gridtype), C.c_int(int(align_corners)),
                                                  _u(interp), C.c_int(_dt(emb_a)), _f(bound), _nv(n_valid), *_live(live, B),
                                                  _stream()), "grid_encode_forward_pair")

    @staticmethod
    def grid_corner_indices(inputs, offsets, corner_idx, B, D, Cc, L, S, H, gridtype, align_corners):
        _check(lib().s3d_grid_corner_indices(_p(inputs), _p(offsets), _p(corner_idx), _u(B), _u(D), _u(Cc), _u(L),
                                             _f(S), _u(H), _u(gridtype), C.c_int(int(align_corners)), _stream()),
               "grid_corner_indices")

    @staticmethod
    def _backward_buffers(grad, offsets, B, D, Cc, L):
        """(max_level_rows, workspace, control block or None) of a backward call; the control block from 8,192 points on"""
        mlr = _max_level_rows(offsets)
        ws = _ws.get(lib().s3d_grid_encode_backward_workspace_size(_u(B), _u(D), _u(Cc), _u(L), _u(mlr),
                                                                   C.c_int(_dt(grad))), grad.device)
        ctl = _ctl.get(lib().s3d_grid_encode_backward_control_size(_u(D), _u(Cc), _u(L), _u(mlr), C.c_int(_dt(grad))),
                       grad.device) if B >= 8192 else None
        return mlr, ws, ctl

    @staticmethod
    def _backward_call(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, found_inf, adam=None):
        """what the three backward methods do in front of their library call: the argument check, with `adam` that of the
        optimizer state -> (max_level_rows, workspace, control block or None, s3d_grid_adam or None)"""
        _need(inputs, torch.float32, "inputs")
        if found_inf is not None:
            _need(found_inf, torch.float32, "found_inf")
        if grad_embeddings.dtype != grad.dtype:
            raise RuntimeError("grad_embeddings must have the dtype of grad")
        for k in ("param", "exp_avg", "exp_avg_sq") if adam is not None else ():
            _need(adam[k], torch.float32, k)
            if adam[k].shape != embeddings.shape or not adam[k].is_contiguous():
                raise RuntimeError(f"adam[{k!r}] must be a contiguous fp32 tensor of the table's shape")
        return GridBackend._backward_buffers(grad, offsets, B, D, Cc, L) + (GridBackend._grid_adam(adam) if adam is not None else None,)

    @staticmethod
    def grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, S, H, dy_dx,
                             grad_inputs, gridtype, align_corners, interp, bound=0.0, n_valid=None, found_inf=None):
        mlr, ws, ctl, _ = GridBackend._backward_call(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, found_inf)
        _check(lib().s3d_grid_encode_backward(*_bwd_tables(grad, inputs, embeddings, offsets, grad_embeddings, mlr, B, D, Cc, L, S, H),
                                              _p(dy_dx), _p(grad_inputs), *_bwd_options(gridtype, align_corners, interp, grad, ws, bound, n_valid),
                                              C.c_int(GridBackend._backward_path), *_bwd_flags(found_inf, ctl), _stream()),
               "grid_encode_backward")

    class _GridAdam(C.Structure):
        _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("param_half", C.c_void_p),
                    ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                    ("step", C.c_void_p), ("grad_scale", C.c_void_p), ("lr_scale", C.c_void_p)]

    @staticmethod
    def _grid_adam(adam):
        ga = GridBackend._GridAdam()
        ga.param, ga.exp_avg, ga.exp_avg_sq = adam["param"].data_ptr(), adam["exp_avg"].data_ptr(), adam["exp_avg_sq"].data_ptr()
        ga.param_half = adam["param_half"].data_ptr() if adam.get("param_half") is not None else None
        ga.lr, (ga.beta1, ga.beta2), ga.eps = float(adam["lr"]), adam["betas"], float(adam["eps"])
        ga.step = adam["step"].data_ptr()
        ga.grad_scale = adam["grad_scale"].data_ptr() if adam.get("grad_scale") is not None else None
        ga.lr_scale = adam["lr_scale"].data_ptr() if adam.get("lr_scale") is not None else None
        return ga

    @staticmethod
    def grid_encode_backward_adam(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, S, H, gridtype, align_corners,
                                  interp, adam, bound=0.0, n_valid=None, found_inf=None):
        """backward of a table with its Adam update inside the accumulate kernel (include/seal3d_hip.h:
        s3d_grid_encode_backward_adam).  `adam`: dict(param, exp_avg, exp_avg_sq, param_half, lr, betas, eps, step, grad_scale,
        lr_scale).  Returns True when the update was applied there, False when the plain backward ran (the gradient is in
        `grad_embeddings`)."""
        mlr, ws, ctl, ga = GridBackend._backward_call(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, found_inf, adam)
        applied = C.c_int(0)
        _check(lib().s3d_grid_encode_backward_adam(*_bwd_tables(grad, inputs, embeddings, offsets, grad_embeddings, mlr, B, D, Cc, L, S, H),
                                                   *_bwd_options(gridtype, align_corners, interp, grad, ws, bound, n_valid),
                                                   *_bwd_flags(found_inf, ctl), C.byref(ga), C.byref(applied), _stream()),
               "grid_encode_backward_adam")
        return bool(applied.value)

    class _StepTail(C.Structure):
        """seal3d_hip.h: s3d_step_tail"""
        _net = lambda x: [("workspace_" + x, C.c_void_p), ("B_" + x, C.c_uint32), ("input_dim_" + x, C.c_uint32),
                          ("hidden_dim_" + x, C.c_uint32), ("num_layers_" + x, C.c_uint32), ("grad_weights_" + x, C.c_void_p),
                          ("accumulate_" + x, C.c_int), ("found_inf_" + x, C.c_void_p)]
        _fields_ = _net("a") + _net("b") + [
            ("loss_workspace", C.c_void_p), ("loss_N", C.c_uint32), ("loss_with_depth", C.c_int), ("loss_depth_weight", C.c_float),
            ("loss", C.c_void_p), ("tensors", C.c_void_p), ("n_tensors", C.c_int32), ("scale", C.c_void_p),
            ("growth_tracker", C.c_void_p), ("growth_factor", C.c_float), ("backoff_factor", C.c_float),
            ("growth_interval", C.c_int32), ("adam_step", C.c_void_p), ("ring_loss", C.c_void_p), ("counter", C.c_void_p),
            ("loss_ring", C.c_void_p), ("counter_ring", C.c_void_p), ("cursor", C.c_void_p), ("ring", C.c_int32),
            ("loss_slots", C.c_int32)]

        def fill(self, names, c_args):
            """file a part: the C arguments its stand-alone entry point would pass, under the fields' names (None: not a field)"""
            for name, v in zip(names, c_args):
                if name is not None:
                    setattr(self, name, v.value)

    TAIL_WGRAD_REDUCE, TAIL_LOSS, TAIL_ADAM, TAIL_EPILOGUE = 1, 2, 4, 8

    @staticmethod
    def grid_encode_backward_adam_tail(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, S, H, gridtype, align_corners,
                                       interp, adam, tail, bound=0.0, n_valid=None, found_inf=None):
        """grid_encode_backward_adam with a step tail (include/seal3d_hip.h: s3d_grid_encode_backward_adam_tail).  `tail`: dict of
        optional parts — reduce=(a, b) as for FFMLPBackend.wgrad_reduce_pair, loss=(workspace, N, with_depth, depth_weight, loss)
        as for RaymarchingBackend.loss_terms_reduce, adam=items as for OptimBackend.adam_step_multi, epilogue=(scale,
        growth_tracker, growth_factor, backoff_factor, growth_interval, adam_step[, loss, counter, loss_ring, counter_ring,
        cursor]) as for OptimBackend.scaler_update / step_epilogue.  Returns (applied, TAIL_* bits of the parts that ran inside
        the backward's launches); a call that falls back has issued reduce and loss as ordinary launches in front."""
        mlr, ws, ctl, ga = GridBackend._backward_call(grad, inputs, embeddings, offsets, grad_embeddings, B, D, Cc, L, found_inf, adam)
        st, who = GridBackend._StepTail(), "step tail"
        if tail.get("reduce") is not None:
            for x, job in zip("ab", tail["reduce"]):
                st.fill([name for name, _ in GridBackend._StepTail._net(x)], _reduce_job_args(job, who))
        if tail.get("loss") is not None:
            st.fill(("loss_workspace", "loss_N", "loss_with_depth", "loss_depth_weight", "loss"), _loss_terms_args(*tail["loss"], who))
        arr = OptimBackend._adam_tensors(tail.get("adam") or [])
        st.tensors, st.n_tensors = C.cast(arr, C.c_void_p), len(arr)
        if tail.get("epilogue") is not None:
            ep = tail["epilogue"]  # (no found_inf in the struct: the riders take the call's own)
            st.fill(("scale", "growth_tracker", None, "growth_factor", "backoff_factor", "growth_interval", "adam_step"),
                    _scaler_update_args(*ep[:2], None, *ep[2:6], who))
            if len(ep) > 6:
                st.fill(("ring_loss", "counter", "loss_ring", "counter_ring", "cursor", "ring", "loss_slots"), _ring_push_args(*ep[6:11], who))
        applied, parts = C.c_int(0), C.c_uint32(0)
        _check(lib().s3d_grid_encode_backward_adam_tail(*_bwd_tables(grad, inputs, embeddings, offsets, grad_embeddings, mlr, B, D, Cc, L, S, H),
                                                        *_bwd_options(gridtype, align_corners, interp, grad, ws, bound, n_valid),
                                                        *_bwd_flags(found_inf, ctl), C.byref(ga), C.byref(st), C.byref(applied),
                                                        C.byref(parts), _stream()), "grid_encode_backward_adam_tail")
        return bool(applied.value), int(parts.value)

    _backward_path = 0  # `path` argument of s3d_grid_encode_backward (binding-side state for tests / experiments)

    @staticmethod
    def set_backward_path(path):
        """0 = auto, 1 = direct global atomics, 2 = binned: partition + LDS accumulate (tests / experiments)"""
        GridBackend._backward_path = int(path)

    @staticmethod
    def grad_total_variation(inputs, embeddings, grad, offsets, weight, B, D, Cc, L, S, H, gridtype, align_corners):
        _need(embeddings, torch.float32, "embeddings")
        _need(inputs, torch.float32, "inputs")
        _check(lib().s3d_grad_total_variation(_p(inputs), _p(embeddings), _p(grad), _p(offsets), _f(weight), _u(B),
                                              _u(D), _u(Cc), _u(L), _f(S), _u(H), _u(gridtype),
                                              C.c_int(int(align_corners)), _stream()), "grad_total_variation")


class SHBackend:
    """shencoder/src/shencoder.h:9-10"""

    @staticmethod
    def sh_encode_forward(inputs, outputs, B, D, Cc, dy_dx):
        _need(inputs, torch.float32, "inputs")
        _check(lib().s3d_sh_encode_forward(_p(inputs), _p(outputs), _u(B), _u(D), _u(Cc), _p(dy_dx), _stream()),
               "sh_encode_forward")

    @staticmethod
    def sh_encode_backward(grad, inputs, B, D, Cc, dy_dx, grad_inputs):
        _need(grad, torch.float32, "grad")
        _check(lib().s3d_sh_encode_backward(_p(grad), _p(inputs), _u(B), _u(D), _u(Cc), _p(dy_dx), _p(grad_inputs),
                                            _stream()), "sh_encode_backward")


class FreqBackend:
    """freqencoder/src/freqencoder.h:7,10"""

    @staticmethod
    def freq_encode_forward(inputs, B, D, deg, Cc, outputs):
        _need(inputs, torch.float32, "inputs")
        _check(lib().s3d_freq_encode_forward(_p(inputs), _u(B), _u(D), _u(deg), _u(Cc), _p(outputs), _stream()),
               "freq_encode_forward")

    @staticmethod
    def freq_encode_pack_forward(a, d, deg1, deg2, out, n_valid=None):
        """out fp16 [B, ld] = [freq(a) | freq(d) | 0]: a fp16 [B, D1], d fp32 [B, D2] (seal3d_hip.h)"""
        _need(a, torch.float16, "a"); _need(d, torch.float32, "d"); _need(out, torch.float16, "out")
        B = a.shape[0]
        if not (a.is_contiguous() and d.is_contiguous() and out.is_contiguous()) or d.shape[0] != B or out.shape[0] != B:
            raise RuntimeError("freq_encode_pack_forward: contiguous a [B, D1], d [B, D2], out [B, ld]")
        _check(lib().s3d_freq_encode_pack_forward(_p(a), _p(d), _u(B), _u(a.shape[1]), _u(deg1), _u(d.shape[1]), _u(deg2), _u(out.shape[1]),
                                                  _p(out), _nv(n_valid), _stream()), "freq_encode_pack_forward")

    @staticmethod
    def freq_encode_pack_backward(grad, a, deg1, grad_a, n_valid=None):
        """grad_a fp16 [B, ldg] (columns behind D1 zero) from the packed row's gradient fp16 [B, ld]"""
        _need(grad, torch.float16, "grad"); _need(a, torch.float16, "a"); _need(grad_a, torch.float16, "grad_a")
        B = a.shape[0]
        if not (grad.is_contiguous() and a.is_contiguous() and grad_a.is_contiguous()) or grad.shape[0] != B or grad_a.shape[0] != B:
            raise RuntimeError("freq_encode_pack_backward: contiguous grad [B, ld], a [B, D1], grad_a [B, ldg]")
        _check(lib().s3d_freq_encode_pack_backward(_p(grad), _p(a), _u(B), _u(a.shape[1]), _u(deg1), _u(grad.shape[1]), _u(grad_a.shape[1]),
                                                   _p(grad_a), _nv(n_valid), _stream()), "freq_encode_pack_backward")

    @staticmethod
    def freq_encode_backward(grad, outputs, B, D, deg, Cc, grad_inputs):
        _need(grad, torch.float32, "grad")
        _check(lib().s3d_freq_encode_backward(_p(grad), _p(outputs), _u(B), _u(D), _u(deg), _u(Cc), _p(grad_inputs),
                                              _stream()), "freq_encode_backward")


class FFMLPBackend:
    """ffmlp/src/ffmlp.h:8-14"""

    @staticmethod
    def allocate_splitk(n):
        _check(lib().s3d_ffmlp_allocate_splitk(C.c_size_t(int(n))), "allocate_splitk")

    @staticmethod
    def free_splitk():
        _check(lib().s3d_ffmlp_free_splitk(), "free_splitk")

    @staticmethod
    def ffmlp_forward(inputs, weights, B, input_dim, output_dim, hidden_dim, num_layers, activation,
                      output_activation, forward_buffer, outputs, input_layout=0, n_valid=None, rgb_head=None, mid=None):
        """`mid` = (dirs f32 [B,3], sigma f32 [B], color_in f16 [B,32], h0 f16 [B]): the density head (seal3d_hip.h)"""
        _need(inputs, torch.float16, "inputs")
        _need(weights, torch.float16, "weights")
        if rgb_head is not None:
            _need(rgb_head, torch.float32, "rgb_head")
        _check(lib().s3d_ffmlp_forward(_p(inputs), _p(weights), _u(B), _u(input_dim), _u(output_dim), _u(hidden_dim),
                                       _u(num_layers), _u(activation), _u(output_activation), _p(forward_buffer),
                                       _p(outputs), C.c_int(int(input_layout)), _nv(n_valid), _p(rgb_head), *_mid_fwd_args(mid, B),
                                       _stream()), "ffmlp_forward")

    @staticmethod
    def ffmlp_inference(inputs, weights, B, input_dim, output_dim, hidden_dim, num_layers, activation,
                        output_activation, inference_buffer, outputs, input_layout=0, n_valid=None, rgb_head=None, mid=None):
        _need(inputs, torch.float16, "inputs")
        _need(weights, torch.float16, "weights")
        if rgb_head is not None:
            _need(rgb_head, torch.float32, "rgb_head")
        _check(lib().s3d_ffmlp_inference(_p(inputs), _p(weights), _u(B), _u(input_dim), _u(output_dim),
                                         _u(hidden_dim), _u(num_layers), _u(activation), _u(output_activation),
                                         _p(inference_buffer), _p(outputs), C.c_int(int(input_layout)), _nv(n_valid),
                                         _p(rgb_head), *_mid_fwd_args(mid, B), _stream()), "ffmlp_inference")

    @staticmethod
    def ngp_pair_inference(inputs, weights_sigma, weights_color, B, hidden_dim, num_layers_sigma, num_layers_color, dirs,
                           sigma, rgb, input_layout=0, n_valid=None, color_in=None, h0=None, enc_color=None):
        """density network + head + colour network + sigmoid in one launch (seal3d_hip.h: s3d_ffmlp_ngp_pair_inference)"""
        for t, n in ((inputs, "inputs"), (weights_sigma, "weights_sigma"), (weights_color, "weights_color")):
            _need(t, torch.float16, n)
        for t, n in ((dirs, "dirs"), (sigma, "sigma"), (rgb, "rgb")):
            _need(t, torch.float32, n)
        _check(lib().s3d_ffmlp_ngp_pair_inference(_p(inputs), _p(weights_sigma), _p(weights_color), _u(B), _u(hidden_dim),
                                                  _u(num_layers_sigma), _u(num_layers_color), C.c_int(int(input_layout)),
                                                  _nv(n_valid), _p(dirs), _p(sigma), _p(rgb), _p(color_in), _p(h0), _p(enc_color),
                                                  _stream()),
               "ffmlp_ngp_pair_inference")

    @staticmethod
    def fused_backward_supported(input_dim, output_dim, hidden_dim, num_layers, activation):
        """True when ffmlp_backward can run without forward_buffer / backward_buffer (re-computing fused kernel)"""
        return bool(lib().s3d_ffmlp_fused_backward_supported(_u(input_dim), _u(output_dim), _u(hidden_dim),
                                                             _u(num_layers), _u(activation)))

    @staticmethod
    def ffmlp_backward(grad, inputs, weights, forward_buffer, B, input_dim, output_dim, hidden_dim, num_layers,
                       activation, output_activation, calc_grad_inputs, backward_buffer, grad_inputs, grad_weights,
                       input_layout=0, accumulate=False, n_valid=None, found_inf=None, grad_rgb=None, rgb_head=None, mid=None,
                       workspace=None, defer_reduce=False):
        """`mid` = (grad_sigma f32 [B] or None, grad_color_in f16 [B,32], h0 f16 [B]): the density head's gradients instead of
        `grad` (seal3d_hip.h); `defer_reduce` + `workspace` (a caller-owned uint8 tensor of ffmlp_backward_workspace_size bytes):
        the weight gradient stays as partial sums in it for wgrad_reduce_pair"""
        if grad_rgb is not None:
            _need(grad_rgb, torch.float32, "grad_rgb"); _need(rgb_head, torch.float32, "rgb_head")
        elif mid is None:
            _need(grad, torch.float16, "grad")
        if found_inf is not None:
            _need(found_inf, torch.float32, "found_inf")
        nbytes = lib().s3d_ffmlp_backward_workspace_size(_u(input_dim), _u(output_dim), _u(hidden_dim),
                                                        _u(num_layers))
        ws = workspace if workspace is not None else _ws.get(nbytes, inputs.device)
        if ws.numel() * ws.element_size() < nbytes:
            raise RuntimeError("ffmlp_backward: workspace too small")
        _check(lib().s3d_ffmlp_backward(_p(grad), _p(inputs), _p(weights), _p(forward_buffer), _u(B), _u(input_dim),
                                        _u(output_dim), _u(hidden_dim), _u(num_layers), _u(activation),
                                        _u(output_activation), C.c_int(int(bool(calc_grad_inputs))),
                                        _p(backward_buffer), _p(grad_inputs if calc_grad_inputs else None),
                                        _p(grad_weights), _p(ws), C.c_size_t(ws.numel()), C.c_int(int(input_layout)),
                                        C.c_int(2 if defer_reduce else int(bool(accumulate))), _nv(n_valid), _p(found_inf), _p(grad_rgb), _p(rgb_head),
                                        *_mid_bwd_args(mid, B), _stream()), "ffmlp_backward")

    @staticmethod
    def backward_workspace_bytes(input_dim, output_dim, hidden_dim, num_layers):
        return int(lib().s3d_ffmlp_backward_workspace_size(_u(input_dim), _u(output_dim), _u(hidden_dim), _u(num_layers)))

    @staticmethod
    def wgrad_reduce_pair(a, b):
        """finish two deferred backward calls: a, b = (workspace, B, input_dim, hidden_dim, num_layers, grad_weights, accumulate, found_inf)"""
        _check(lib().s3d_ffmlp_wgrad_reduce_pair(*_reduce_job_args(a, "wgrad_reduce_pair"), *_reduce_job_args(b, "wgrad_reduce_pair"),
                                                 _stream()), "ffmlp_wgrad_reduce_pair")


def _mid_fwd_args(mid, B):
    """the four density-head arguments of s3d_ffmlp_forward / _inference from (dirs, sigma, color_in, h0) or None"""
    if mid is None:
        return (C.c_void_p(0),) * 4
    dirs, sigma, cin, h0 = mid
    _need(dirs, torch.float32, "mid dirs"); _need(sigma, torch.float32, "mid sigma")
    _need(cin, torch.float16, "mid color_in"); _need(h0, torch.float16, "mid h0")
    if dirs.numel() != 3 * B or sigma.numel() != B or cin.numel() != 32 * B or h0.numel() != B:
        raise RuntimeError("ffmlp density head: dirs [B,3], sigma [B], color_in [B,32], h0 [B]")
    return _p(dirs), _p(sigma), _p(cin), _p(h0)


def _mid_bwd_args(mid, B):
    """the three density-head arguments of s3d_ffmlp_backward from (grad_sigma or None, grad_color_in, h0) or None"""
    if mid is None:
        return (C.c_void_p(0),) * 3
    if mid[0] is not None:
        _need(mid[0], torch.float32, "mid grad_sigma")
    _need(mid[1], torch.float16, "mid grad_color_in"); _need(mid[2], torch.float16, "mid h0")
    if mid[1].numel() != 32 * B or mid[2].numel() != B or (mid[0] is not None and mid[0].numel() != B):
        raise RuntimeError("ffmlp density head: grad_sigma [B], grad_color_in [B,32], h0 [B]")
    return _p(mid[0]), _p(mid[1]), _p(mid[2])


class _AdamTensor(C.Structure):
    """seal3d_hip.h: s3d_adam_tensor"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("param_half", C.c_void_p), ("n", C.c_size_t), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("grad_dtype", C.c_int), ("consume", C.c_int), ("pack_cols", C.c_uint32),
                ("pack_stride", C.c_uint32), ("l1", C.c_float)]


class OptimBackend:
    """csrc/optim.hip — Adam + GradScaler bookkeeping straight from the (fp16) gradients"""

    @staticmethod
    def grads_nonfinite(grad, found_inf):
        _need(found_inf, torch.float32, "found_inf")
        _check(lib().s3d_grads_nonfinite(_p(grad), C.c_size_t(grad.numel()), C.c_int(_dt(grad)), _p(found_inf), _stream()),
               "grads_nonfinite")

    @staticmethod
    def adam_step(param, grad, exp_avg, exp_avg_sq, param_half, lr, beta1, beta2, eps, step, grad_scale, found_inf, lr_scale=None):
        _need(param, torch.float32, "param")
        _need(exp_avg, torch.float32, "exp_avg")
        _need(exp_avg_sq, torch.float32, "exp_avg_sq")
        if grad.numel() != param.numel() or not grad.is_contiguous() or not param.is_contiguous():
            raise RuntimeError("adam_step: param and grad must be contiguous and of equal size")
        if param_half is not None:
            _need(param_half, torch.float16, "param_half")
        _check(lib().s3d_adam_step(_p(param), _p(grad), C.c_int(_dt(grad)), _p(exp_avg), _p(exp_avg_sq), _p(param_half),
                                   C.c_size_t(param.numel()), _f(lr), _f(beta1), _f(beta2), _f(eps), _p(step),
                                   _p(grad_scale), _p(found_inf), _p(lr_scale), _stream()), "adam_step")

    @staticmethod
    def adam_step_multi(items, step, grad_scale, found_inf, consume_grads=False, lr_scale=None):
        """`items`: (param, grad, exp_avg, exp_avg_sq, param_half or None, lr, beta1, beta2, eps[, consume[, l1]]) per tensor —
        adam_step for all of them in one launch; `consume_grads` (all tensors) / the optional tenth element (that tensor): the
        gradient is cleared behind the read; eleventh element: coefficient of an L1 penalty whose gradient the update adds
        (seal3d_hip.h)"""
        arr = OptimBackend._adam_tensors(items)
        _check(lib().s3d_adam_step_multi(arr, C.c_int32(len(items)), _p(step), _p(grad_scale), _p(found_inf), _p(lr_scale),
                                         C.c_int(int(bool(consume_grads))), _stream()), "adam_step_multi")

    @staticmethod
    def _adam_tensors(items):
        """the s3d_adam_tensor array of adam_step_multi's `items`"""
        arr = (_AdamTensor * len(items))()
        for a, item in zip(arr, items):
            param, grad, exp_avg, exp_avg_sq, param_half, lr, beta1, beta2, eps = item[:9]
            a.consume = int(bool(item[9])) if len(item) > 9 else 0
            a.l1 = float(item[10]) if len(item) > 10 else 0.0
            _need(param, torch.float32, "param"); _need(exp_avg, torch.float32, "exp_avg"); _need(exp_avg_sq, torch.float32, "exp_avg_sq")
            packed = grad.dim() == 2 and not grad.is_contiguous()
            if packed:
                # [rows, cols] views into a packed weight buffer (row stride > cols): gradient and fp16 copy share the layout
                if (tuple(grad.shape) != tuple(param.shape) or grad.stride(1) != 1 or not grad.is_cuda or not param.is_contiguous()
                        or (param_half is not None and (param_half.stride() != grad.stride() or param_half.dtype != torch.float16
                                                        or not param_half.is_cuda))):
                    raise RuntimeError("adam_step_multi: a packed gradient is a [rows, cols] row-strided view; the fp16 copy shares its strides")
                a.pack_cols, a.pack_stride = int(grad.shape[1]), int(grad.stride(0))
                a.param, a.grad, a.exp_avg, a.exp_avg_sq = _p(param), C.c_void_p(grad.data_ptr()), _p(exp_avg), _p(exp_avg_sq)
                a.param_half = C.c_void_p(param_half.data_ptr() if param_half is not None else 0)
            else:
                if grad.numel() != param.numel() or not grad.is_contiguous() or not param.is_contiguous():
                    raise RuntimeError("adam_step_multi: param and grad must be contiguous and of equal size")
                if param_half is not None:
                    _need(param_half, torch.float16, "param_half")
                a.param, a.grad, a.exp_avg, a.exp_avg_sq = _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq)
                a.param_half = _p(param_half)
            a.n = param.numel()
            a.lr, a.beta1, a.beta2, a.eps = float(lr), float(beta1), float(beta2), float(eps)
            a.grad_dtype = _dt(grad)
        return arr

    @staticmethod
    def scaler_update(scale, growth_tracker, found_inf, growth_factor, backoff_factor, growth_interval, adam_step=None):
        _check(lib().s3d_scaler_update(*_scaler_update_args(scale, growth_tracker, found_inf, growth_factor, backoff_factor,
                                                            growth_interval, adam_step, "scaler_update"), _stream()), "scaler_update")

    @staticmethod
    def adam_advance(step, found_inf):
        _check(lib().s3d_adam_advance(_p(step), _p(found_inf), _stream()), "adam_advance")

    @staticmethod
    def step_epilogue(scale, growth_tracker, found_inf, growth_factor, backoff_factor, growth_interval, adam_step, loss, counter,
                      loss_ring, counter_ring, cursor):
        """scaler_update + step_ring_push in one launch (seal3d_hip.h)"""
        _check(lib().s3d_step_epilogue(*_scaler_update_args(scale, growth_tracker, found_inf, growth_factor, backoff_factor,
                                                            growth_interval, adam_step, "step_epilogue"),
                                       *_ring_push_args(loss, counter, loss_ring, counter_ring, cursor, "step_epilogue"), _stream()),
               "step_epilogue")

    @staticmethod
    def step_ring_push(loss, counter, loss_ring, counter_ring, cursor):
        """file `loss` [] / `counter` [2] in slot *cursor of the rings, clear the counter, advance the cursor (seal3d_hip.h)"""
        _check(lib().s3d_step_ring_push(*_ring_push_args(loss, counter, loss_ring, counter_ring, cursor, "step_ring_push"), _stream()),
               "step_ring_push")


class _EmaTensor(C.Structure):
    """seal3d_hip.h: s3d_ema_tensor"""
    _fields_ = [("param", C.c_void_p), ("shadow", C.c_void_p), ("n", C.c_size_t)]


class EmaBackend:
    """csrc/ema.hip — the parameters' exponential moving average (torch_ema's update) and the by-value swap"""

    @staticmethod
    def _tensors(pairs, who):
        """the s3d_ema_tensor array of `pairs` = [(param, shadow), ...]: fp32, contiguous, on the GPU, of equal size"""
        arr = (_EmaTensor * max(len(pairs), 1))()
        for a, (param, shadow) in zip(arr, pairs):
            _need(param, torch.float32, f"{who}: param"); _need(shadow, torch.float32, f"{who}: shadow")
            if param.numel() != shadow.numel():
                raise RuntimeError(f"{who}: param and shadow must be of equal size, got {param.numel()} and {shadow.numel()}")
            if param.device != shadow.device:
                raise RuntimeError(f"{who}: param and shadow must live on one device")
            a.param, a.shadow, a.n = _p(param), _p(shadow), param.numel()
        return arr

    @staticmethod
    def update_multi(pairs, decay, num_updates, use_num_updates=True):
        """shadow -= (1 - d) * (shadow - param) for every (param, shadow) of `pairs`, torch_ema's three roundings, one launch;
        `num_updates`: the device int64 [1] count (advanced by one; None only with use_num_updates=False) — seal3d_hip.h"""
        if num_updates is not None:
            _need(num_updates, torch.int64, "ema_update_multi: num_updates")
            if num_updates.numel() != 1:
                raise RuntimeError("ema_update_multi: num_updates is one int64")
        elif use_num_updates:
            raise RuntimeError("ema_update_multi: the warm-up schedule needs the device update count")
        arr = EmaBackend._tensors(pairs, "ema_update_multi")
        _check(lib().s3d_ema_update_multi(arr, C.c_int32(len(pairs)), C.c_double(float(decay)), C.c_int(int(bool(use_num_updates))),
                                          _p(num_updates), _stream()), "ema_update_multi")

    @staticmethod
    def exchange_multi(pairs):
        """param <-> shadow, elementwise and in place, for every (param, shadow) of `pairs` in one launch"""
        arr = EmaBackend._tensors(pairs, "ema_exchange_multi")
        _check(lib().s3d_ema_exchange_multi(arr, C.c_int32(len(pairs)), _stream()), "ema_exchange_multi")


class NgpHeadBackend:
    """csrc/ngp_head.hip — the elementwise glue between the two MLPs of nerf/network_ff.py"""

    @staticmethod
    def mid_forward(h, dirs, sigma, color_in, n_valid=None):
        _need(h, torch.float16, "h"); _need(dirs, torch.float32, "dirs")
        _need(sigma, torch.float32, "sigma"); _need(color_in, torch.float16, "color_in")
        _check(lib().s3d_ngp_mid_forward(_p(h), _p(dirs), _u(h.shape[0]), _p(sigma), _p(color_in), _nv(n_valid), _stream()),
               "ngp_mid_forward")

    @staticmethod
    def mid_backward(grad_color_in, grad_sigma, h, grad_h, n_valid=None):
        _need(grad_color_in, torch.float16, "grad_color_in"); _need(grad_h, torch.float16, "grad_h")
        if grad_sigma is not None:
            _need(grad_sigma, torch.float32, "grad_sigma")
        _check(lib().s3d_ngp_mid_backward(_p(grad_color_in), _p(grad_sigma), _p(h), _u(h.shape[0]), _p(grad_h), _nv(n_valid),
                                          _stream()), "ngp_mid_backward")

    @staticmethod
    def mid2_forward(h, dirs, enc_color, sigma, color_in, n_valid=None):
        """two-encoder network: color_in [B,64] = [SH | geo | enc_color | 0]; enc_color level-major [16,B,2] fp16"""
        _need(h, torch.float16, "h"); _need(dirs, torch.float32, "dirs"); _need(enc_color, torch.float16, "enc_color")
        _need(sigma, torch.float32, "sigma"); _need(color_in, torch.float16, "color_in")
        B = h.shape[0]
        if tuple(enc_color.shape) != (16, B, 2) or tuple(color_in.shape) != (B, 64):
            raise RuntimeError("mid2_forward: enc_color must be [16,B,2], color_in [B,64]")
        _check(lib().s3d_ngp_mid2_forward(_p(h), _p(dirs), _p(enc_color), _u(B), _p(sigma), _p(color_in), _nv(n_valid), _stream()),
               "ngp_mid2_forward")

    @staticmethod
    def mid2_backward(grad_color_in, grad_sigma, h, grad_h, grad_enc_color, n_valid=None):
        _need(grad_color_in, torch.float16, "grad_color_in"); _need(grad_h, torch.float16, "grad_h")
        if grad_sigma is not None:
            _need(grad_sigma, torch.float32, "grad_sigma")
        if grad_enc_color is not None:
            _need(grad_enc_color, torch.float16, "grad_enc_color")
        # h: the density network's [B, 16] output, or its first column [B] alone (the one-launch pair keeps only that)
        _need(h, torch.float16, "h")
        _check(lib().s3d_ngp_mid2_backward(_p(grad_color_in), _p(grad_sigma), _p(h), _u(16 if h.dim() == 2 else 1), _u(h.shape[0]),
                                           _p(grad_h), _p(grad_enc_color), _nv(n_valid), _stream()), "ngp_mid2_backward")

    @staticmethod
    def rgb_forward(out, rgb, n_valid=None):
        _need(out, torch.float16, "out"); _need(rgb, torch.float32, "rgb")
        _check(lib().s3d_ngp_rgb_forward(_p(out), _u(out.shape[0]), _p(rgb), _nv(n_valid), _stream()), "ngp_rgb_forward")

    @staticmethod
    def rgb_backward(grad_rgb, rgb, grad_out, n_valid=None):
        _need(grad_rgb, torch.float32, "grad_rgb"); _need(rgb, torch.float32, "rgb"); _need(grad_out, torch.float16, "grad_out")
        _check(lib().s3d_ngp_rgb_backward(_p(grad_rgb), _p(rgb), _u(rgb.shape[0]), _p(grad_out), _nv(n_valid), _stream()),
               "ngp_rgb_backward")

    @staticmethod
    def bg_mse_forward(image, weights_sum, gt, bg_rgb, loss, grad_loss=None, grad_image=None, grad_weights_sum=None,
                       depth=None, gt_depth=None, depth_weight=1.0):
        """`depth`, `gt_depth` (both or neither): + depth_weight * L1(nan_to_num(depth), gt_depth) in the loss VALUE (seal3d_hip.h)"""
        for t, n in ((image, "image"), (weights_sum, "weights_sum"), (gt, "gt"), (loss, "loss")):
            _need(t, torch.float32, n)
        if grad_loss is not None:
            for t, n in ((grad_loss, "grad_loss"), (grad_image, "grad_image"), (grad_weights_sum, "grad_weights_sum")):
                _need(t, torch.float32, n)
        if depth is not None:
            _need(depth, torch.float32, "depth"); _need(gt_depth, torch.float32, "gt_depth")
            if depth.numel() != image.shape[0] or gt_depth.numel() != image.shape[0]:
                raise RuntimeError("bg_mse_forward: depth and gt_depth hold one value per ray")
        bg = (C.c_float * 3)(*[float(v) for v in bg_rgb])
        _check(lib().s3d_bg_mse_forward(_p(image), _p(weights_sum), _p(gt), bg, _u(image.shape[0]), _p(loss), _p(grad_loss),
                                        _p(grad_image), _p(grad_weights_sum), _p(depth), _p(gt_depth), _f(depth_weight), _stream()),
               "bg_mse_forward")

    @staticmethod
    def bg_targets(image, weights_sum, depth, bg_rgb, out_rgb, out_depth=None):
        """out_rgb = nan_to_num(image + (1 - weights_sum) * bg), out_depth = nan_to_num(depth): a teacher render's targets"""
        for t, n in ((image, "image"), (weights_sum, "weights_sum"), (out_rgb, "out_rgb")):
            _need(t, torch.float32, n)
        N = image.shape[0]
        if out_rgb.numel() != 3 * N or weights_sum.numel() != N:
            raise RuntimeError("bg_targets: image / out_rgb [N,3], weights_sum [N]")
        if out_depth is not None:
            _need(depth, torch.float32, "depth"); _need(out_depth, torch.float32, "out_depth")
            if depth.numel() != N or out_depth.numel() != N:
                raise RuntimeError("bg_targets: depth / out_depth [N]")
        bg = (C.c_float * 3)(*[float(v) for v in bg_rgb])
        _check(lib().s3d_bg_targets(_p(image), _p(weights_sum), _p(depth if out_depth is not None else None), bg, _u(N),
                                    _p(out_rgb), _p(out_depth), _stream()), "bg_targets")

    @staticmethod
    def bg_targets_rays(image, weights_sum, depth, bg, out_rgb, out_depth=None):
        """bg_targets with a per-ray background bg [N,3] (device)"""
        for t, n in ((image, "image"), (weights_sum, "weights_sum"), (bg, "bg"), (out_rgb, "out_rgb")):
            _need(t, torch.float32, n)
        N = image.shape[0]
        if out_rgb.numel() != 3 * N or weights_sum.numel() != N or bg.numel() != 3 * N:
            raise RuntimeError("bg_targets_rays: image / bg / out_rgb [N,3], weights_sum [N]")
        if out_depth is not None:
            _need(depth, torch.float32, "depth"); _need(out_depth, torch.float32, "out_depth")
            if depth.numel() != N or out_depth.numel() != N:
                raise RuntimeError("bg_targets_rays: depth / out_depth [N]")
        _check(lib().s3d_bg_targets_rays(_p(image), _p(weights_sum), _p(depth if out_depth is not None else None), _p(bg), _u(N),
                                         _p(out_rgb), _p(out_depth), _stream()), "bg_targets_rays")

    @staticmethod
    def _background_args(sph, dirs, table, offsets, w0, w1, rgb, what):
        """shape / dtype checks shared by background_forward and background_backward; returns N"""
        for t, n in ((sph, "sph"), (dirs, "dirs"), (w0, "w0"), (w1, "w1"), (rgb, "rgb")):
            _need(t, torch.float32, n)
        _need(offsets, torch.int32, "offsets")
        N = sph.shape[0]
        if (sph.shape != (N, 2) or dirs.shape != (N, 3) or rgb.shape != (N, 3) or offsets.numel() != 5 or table.dim() != 2
                or table.shape[1] != 2 or w0.shape != (64, 24) or w1.shape != (3, 64)):
            raise RuntimeError(f"{what}: sph [N,2], dirs / rgb [N,3], offsets [5], table [rows,2], w0 [64,24], w1 [3,64]")
        return N

    @staticmethod
    def background_forward(sph, dirs, table, offsets, S, H, w0, w1, rgb, features=None):
        """the background model (seal3d_hip.h: s3d_background_forward): sph [N,2], dirs [N,3] fp32, table [rows,2] fp32/fp16,
        offsets [5] int32, w0 [64,24] / w1 [3,64] fp32 (read as fp16) -> rgb [N,3] fp32 (+ the grid features [4,N,2] of the table's dtype)"""
        N = NgpHeadBackend._background_args(sph, dirs, table, offsets, w0, w1, rgb, "background_forward")
        if features is not None and (features.dtype != table.dtype or features.shape != (4, N, 2)):
            raise RuntimeError("background_forward: features [4,N,2] of the table's dtype")
        _check(lib().s3d_background_forward(_p(sph), _p(dirs), _p(table), _p(offsets), _u(N), _f(S), _u(H), C.c_int(_dt(table)),
                                            _p(w0), _p(w1), _p(rgb), _p(features), _stream()), "background_forward")

    @staticmethod
    def background_backward(grad_rgb, rgb, sph, dirs, table, offsets, S, H, w0, w1, grad_table, grad_w0, grad_w1, found_inf=None):
        """backward of background_forward: ADDS the table gradient into grad_table (the table's shape and dtype; None: no table
        gradient), overwrites grad_w0 [64,24] / grad_w1 [3,64] (fp32); found_inf (optional fp32 [1]) raised for a non-finite gradient"""
        N = NgpHeadBackend._background_args(sph, dirs, table, offsets, w0, w1, rgb, "background_backward")
        _need(grad_rgb, torch.float32, "grad_rgb"); _need(grad_w0, torch.float32, "grad_w0"); _need(grad_w1, torch.float32, "grad_w1")
        if (grad_rgb.shape != (N, 3) or grad_w0.shape != (64, 24) or grad_w1.shape != (3, 64)
                or (grad_table is not None and (grad_table.shape != table.shape or grad_table.dtype != table.dtype))):
            raise RuntimeError("background_backward: grad_rgb [N,3], grad_table like table, grad_w0 [64,24], grad_w1 [3,64]")
        ws, nb = _background_workspace(lib().s3d_background_backward_workspace_size, N, sph.device, found_inf)
        _check(lib().s3d_background_backward(_p(grad_rgb), _p(rgb), _p(sph), _p(dirs), _p(table), _p(offsets), _u(table.shape[0]), _u(N),
                                             _f(S), _u(H), C.c_int(_dt(table)), _p(w0), _p(w1), _p(grad_table), _p(grad_w0),
                                             _p(grad_w1), _p(found_inf), _p(ws), nb, _stream()), "background_backward")

    _l1_ws = {}

    @staticmethod
    def l1_pair_loss(sigma, color, gt_sigma, gt_color, n_total, loss, grad_loss=None, grad_sigma=None, grad_color=None):
        """Seal-3D's pretraining loss L1(sigma) + L1(colour) (+ its gradients for a known upstream gradient), seal3d_hip.h"""
        for t, n in ((sigma, "sigma"), (color, "color"), (gt_sigma, "gt_sigma"), (gt_color, "gt_color"), (loss, "loss")):
            _need(t, torch.float32, n)
        n, n_rows = gt_sigma.numel(), sigma.numel()
        if color.numel() != 3 * n_rows or n_rows < n or gt_color.numel() != 3 * n:
            raise RuntimeError("l1_pair_loss: sigma [n_rows] / color [n_rows,3], gt_sigma [n] / gt_color [n,3], n_rows >= n")
        if grad_loss is not None:
            for t, nm in ((grad_loss, "grad_loss"), (grad_sigma, "grad_sigma"), (grad_color, "grad_color")):
                _need(t, torch.float32, nm)
        # one workspace (partial sums + the last-block ticket) per (device, stream): two launches in flight on different
        # streams — a pretraining graph on a side stream next to an eager call, two trainers — must not share a ticket
        key = (sigma.device.index, torch.cuda.current_stream(sigma.device).cuda_stream)
        ws = NgpHeadBackend._l1_ws.get(key)
        if ws is None:  # (zeroed once: the kernel leaves its ticket word zero)
            n_ws = lib().s3d_l1_pair_workspace_size() // 4
            if torch.cuda.is_current_stream_capturing():
                # (torch captures every graph on its own stream: a buffer first asked for during a capture is allocated from
                #  that graph's pool and zeroed by a fill the graph replays — it is not cached beyond the capture)
                ws = torch.zeros(n_ws, dtype=torch.float32, device=sigma.device)
            else:
                ws = NgpHeadBackend._l1_ws[key] = torch.zeros(n_ws, dtype=torch.float32, device=sigma.device)
        _check(lib().s3d_l1_pair_loss(_p(sigma), _p(color), _p(gt_sigma), _p(gt_color), _u(n), _u(n_rows), _u(n_total), _p(loss), _p(grad_loss),
                                      _p(grad_sigma), _p(grad_color), _p(ws), _stream()), "l1_pair_loss")

    @staticmethod
    def bg_mse_backward(image, weights_sum, gt, bg_rgb, grad_loss, grad_image, grad_weights_sum):
        _need(grad_loss, torch.float32, "grad_loss")
        bg = (C.c_float * 3)(*[float(v) for v in bg_rgb])
        _check(lib().s3d_bg_mse_backward(_p(image), _p(weights_sum), _p(gt), bg, _u(image.shape[0]), _p(grad_loss),
                                         _p(grad_image), _p(grad_weights_sum), _stream()), "bg_mse_backward")


class RaySampleBackend:
    """csrc/raysample.hip — training rays drawn on the device (nerf/utils.py:92-114 with or without an error map), the
    error map's EMA update (nerf/utils.py:506-528) and the frames of generated orbit poses (SealNeRF/provider.py:145-178)"""

    @staticmethod
    def sample_train_rays(error_map, index, N, H, W, poses, intrinsics, rays_o, rays_d, inds, inds_coarse=None, images=None,
                          depths=None, gt=None, gt_depth=None, seed=0, ctl=None, u_keys=None, u_fine=None, out_index=None,
                          rgba=False, random_bg=True, u_bg=None, out_bg=None):
        """seal3d_hip.h: s3d_sample_train_rays.  index [B] int64; outputs [B, N, ...] preallocated by the caller.  `rgba`:
        images are [n_images, H, W, 4] and s3d_sample_train_rays_rgba blends them into gt (onto `random_bg`: a per-pixel
        random background, handed out in out_bg [B, N, 3]; False: onto 1); u_bg [B, N, 3]: explicit uniforms (test entry)"""
        B = index.numel()
        _need(index, torch.int64, "index"); _need(poses, torch.float32, "poses"); _need(inds, torch.int64, "inds")
        for t, n in ((rays_o, "rays_o"), (rays_d, "rays_d"), (gt, "gt"), (gt_depth, "gt_depth"), (error_map, "error_map"),
                     (depths, "depths"), (u_keys, "u_keys"), (u_fine, "u_fine"), (u_bg, "u_bg"), (out_bg, "out_bg")):
            if t is not None:
                _need(t, torch.float32, n)
        for t, n in ((inds_coarse, "inds_coarse"), (out_index, "out_index")):
            if t is not None:
                _need(t, torch.int64, n)
        if out_index is not None and out_index.numel() != B:
            raise RuntimeError("sample_train_rays: out_index must hold B values")
        if ctl is not None:
            _need(ctl, torch.int32, "ctl")
        for t, n, w in ((rays_o, "rays_o", 3), (rays_d, "rays_d", 3), (inds, "inds", 1), (inds_coarse, "inds_coarse", 1),
                        (gt, "gt", 3), (gt_depth, "gt_depth", 1), (u_fine, "u_fine", 2), (u_bg, "u_bg", 3), (out_bg, "out_bg", 3)):
            if t is not None and t.numel() != B * N * w:
                raise RuntimeError(f"sample_train_rays: {n} must hold {B} x {N} x {w} values")
        n_img = poses.shape[0]
        if error_map is not None and error_map.numel() != n_img * 128 * 128:
            raise RuntimeError("sample_train_rays: error_map must be [n_images, 128 * 128]")
        if u_keys is not None and u_keys.numel() != B * 128 * 128:
            raise RuntimeError("sample_train_rays: u_keys must be [B, 128 * 128]")
        dt, ch = F32, 4 if rgba else 3
        if not rgba and (u_bg is not None or out_bg is not None):
            raise RuntimeError("sample_train_rays: u_bg / out_bg belong to RGBA frames (rgba=True)")
        if images is not None:
            if images.dtype not in (torch.float32, torch.float16) or images.shape[-1] != ch or images.numel() != n_img * H * W * ch:
                raise RuntimeError(f"sample_train_rays: images must be [n_images, H, W, {ch}] fp32 / fp16")
            dt = F16 if images.dtype == torch.float16 else F32
        if depths is not None and depths.numel() != n_img * H * W:
            raise RuntimeError("sample_train_rays: depths must hold one value per pixel")
        intr = (C.c_float * 4)(*[float(v) for v in intrinsics])
        if rgba:
            _check(lib().s3d_sample_train_rays_rgba(_p(error_map), _p(index), _u(B), _u(N), _u(n_img), _u(H), _u(W), _p(poses), intr,
                                                    _p(images), C.c_int(dt), _p(depths), _u(int(seed) & 0xFFFFFFFF), _p(ctl),
                                                    _p(u_keys), _p(u_fine), C.c_int(1 if random_bg else 0), _p(u_bg), _p(rays_o),
                                                    _p(rays_d), _p(gt), _p(out_bg), _p(gt_depth), _p(inds), _p(inds_coarse),
                                                    _p(out_index), _stream()), "s3d_sample_train_rays_rgba")
            return
        _check(lib().s3d_sample_train_rays(_p(error_map), _p(index), _u(B), _u(N), _u(n_img), _u(H), _u(W), _p(poses), intr,
                                           _p(images), C.c_int(dt), _p(depths), _u(int(seed) & 0xFFFFFFFF), _p(ctl), _p(u_keys),
                                           _p(u_fine), _p(rays_o), _p(rays_d), _p(gt), _p(gt_depth), _p(inds), _p(inds_coarse),
                                           _p(out_index), _stream()), "s3d_sample_train_rays")

    @staticmethod
    def rgba_targets(images, gt, bg=None, random_bg=True, seed=0, ctl=None, u_bg=None):
        """seal3d_hip.h: s3d_rgba_targets.  images [..., 4] fp32 / fp16 -> gt [..., 3] fp32 blended onto bg [..., 3] fp32 (random_bg:
        the per-pixel random background, drawn at step ctl[0] or taken from u_bg; False: 1, bg may be None)"""
        if images.dtype not in (torch.float32, torch.float16) or images.dim() < 1 or images.shape[-1] != 4:
            raise RuntimeError("rgba_targets: images must be [..., 4] fp32 / fp16")
        R = images.numel() // 4
        for t, n in ((gt, "gt"), (bg, "bg"), (u_bg, "u_bg")):
            if t is not None:
                _need(t, torch.float32, n)
                if t.numel() != R * 3:
                    raise RuntimeError(f"rgba_targets: {n} must hold {R} x 3 values")
        if ctl is not None:
            _need(ctl, torch.int32, "ctl")
        if random_bg and bg is None:
            raise RuntimeError("rgba_targets: a random background is handed out in bg")
        _check(lib().s3d_rgba_targets(_p(images), C.c_int(F16 if images.dtype == torch.float16 else F32), _u(R),
                                      C.c_int(1 if random_bg else 0), _u(int(seed) & 0xFFFFFFFF), _p(ctl), _p(u_bg), _p(gt), _p(bg),
                                      _stream()), "s3d_rgba_targets")

    @staticmethod
    def orbit_rays(B, rH, rW, intrinsics, rays_o, rays_d, poses_out=None, look_at=None, radius=1.0, theta_range=(math.pi / 3, 2 * math.pi / 3),
                   phi_range=(0.0, 2 * math.pi), seed=0, ctl=None, u_pose=None):
        """seal3d_hip.h: s3d_orbit_rays.  B orbit poses around `look_at` (3 host numbers; None: the origin) at distance `radius`
        and the rays of each pose's rH x rW frame: rays_o, rays_d [B, rH*rW, 3], poses_out [B, 4, 4] (optional), all fp32 and
        preallocated.  `intrinsics`: fx, fy, cx, cy of the rH x rW frame.  The draw is keyed by (`seed`, ctl[0]); u_pose [B, 2]:
        explicit uniforms of theta and phi (test entry, ctl is left alone)"""
        B, rH, rW = int(B), int(rH), int(rW)
        for t, n, w in ((rays_o, "rays_o", rH * rW * 3), (rays_d, "rays_d", rH * rW * 3), (poses_out, "poses_out", 16), (u_pose, "u_pose", 2)):
            if t is not None:
                _need(t, torch.float32, n)
                if t.numel() != B * w:
                    raise RuntimeError(f"orbit_rays: {n} must hold {B} x {w} values")
        if ctl is not None:
            _need(ctl, torch.int32, "ctl")
            if ctl.numel() < 2:
                raise RuntimeError("orbit_rays: ctl holds {step, 0}")
        intr = (C.c_float * 4)(*[float(v) for v in intrinsics])
        look = None if look_at is None else (C.c_float * 3)(*[float(v) for v in look_at])
        _check(lib().s3d_orbit_rays(_u(B), _u(rH), _u(rW), intr, look, C.c_float(float(radius)), C.c_double(float(theta_range[0])),
                                    C.c_double(float(theta_range[1])), C.c_double(float(phi_range[0])), C.c_double(float(phi_range[1])),
                                    _u(int(seed) & 0xFFFFFFFF), _p(ctl), _p(u_pose), _p(poses_out), _p(rays_o), _p(rays_d), _stream()),
               "s3d_orbit_rays")

    @staticmethod
    def frame_rays(pose, intrinsics, rH, rW, rays_o, rays_d):
        """seal3d_hip.h: s3d_frame_rays.  The rays of the one camera `pose` (16 host numbers, a row-major 4 x 4 cam2world
        matrix) for its whole rH x rW frame: rays_o, rays_d [rH*rW, 3] fp32, preallocated.  `intrinsics`: fx, fy, cx, cy of
        the rH x rW frame (host numbers).  Pose and intrinsics travel in the launch's arguments: no staging copy."""
        rH, rW = int(rH), int(rW)
        for t, n in ((rays_o, "rays_o"), (rays_d, "rays_d")):
            _need(t, torch.float32, n)
            if t.numel() != rH * rW * 3:
                raise RuntimeError(f"frame_rays: {n} must hold {rH * rW} x 3 values")
        vals = [float(v) for row in pose for v in (row if hasattr(row, "__len__") else (row,))]
        if len(vals) != 16:
            raise RuntimeError("frame_rays: pose holds the 16 numbers of a 4 x 4 matrix")
        mat = (C.c_float * 16)(*vals)
        intr = (C.c_float * 4)(*[float(v) for v in intrinsics])
        _check(lib().s3d_frame_rays(mat, intr, _u(rH), _u(rW), _p(rays_o), _p(rays_d), _stream()), "s3d_frame_rays")

    @staticmethod
    def error_map_update(error_map, index, inds_coarse, image, gt, weights_sum=None, bg=None, depth=None, gt_depth=None,
                         depth_weight=1.0):
        """seal3d_hip.h: s3d_error_map_update.  bg: None, 3 floats, or a per-ray fp32 tensor [B*N, 3]"""
        B, N = inds_coarse.shape
        _need(error_map, torch.float32, "error_map"); _need(index, torch.int64, "index"); _need(inds_coarse, torch.int64, "inds_coarse")
        for t, n in ((image, "image"), (gt, "gt"), (weights_sum, "weights_sum"), (depth, "depth"), (gt_depth, "gt_depth")):
            if t is not None:
                _need(t, torch.float32, n)
        if index.numel() != B or image.numel() != B * N * 3 or gt.numel() != B * N * 3:
            raise RuntimeError("error_map_update: index [B], inds_coarse [B, N], image / gt [B*N, 3]")
        if weights_sum is not None and weights_sum.numel() != B * N:
            raise RuntimeError("error_map_update: weights_sum holds one value per ray")
        if (depth is None) != (gt_depth is None) or (depth is not None and (depth.numel() != B * N or gt_depth.numel() != B * N)):
            raise RuntimeError("error_map_update: depth and gt_depth (one value per ray) go together")
        bg_rgb, bg_rays = None, None
        if torch.is_tensor(bg):
            _need(bg, torch.float32, "bg")
            if bg.numel() != B * N * 3:
                raise RuntimeError("error_map_update: a per-ray background is [B*N, 3]")
            bg_rays = bg
        elif bg is not None:
            bg_rgb = (C.c_float * 3)(*[float(v) for v in bg])
        if error_map.dim() != 2 or error_map.shape[1] != 128 * 128:
            raise RuntimeError("error_map_update: error_map must be [n_images, 128 * 128]")
        _check(lib().s3d_error_map_update(_p(error_map), _u(error_map.shape[0]), _p(index), _p(inds_coarse), _u(B), _u(N), _p(image), _p(weights_sum),
                                          _p(gt), bg_rgb, _p(bg_rays), _p(depth), _p(gt_depth), C.c_float(float(depth_weight)),
                                          _stream()), "s3d_error_map_update")


class SealBackend:
    """csrc/seal.hip — Seal-3D's proxy mappers (SealNeRF/seal_utils.py:132-570, 630-685: bbox, brush, anchor) on the device"""

    @staticmethod
    def bbox_map(points, dirs, host, out_points, out_dirs, mask, n_valid=None):
        """`host`: dict of float32 numpy arrays (triangles, bounds, inv_transform, inv_rotation, inv_scale, center and
        optionally empty_bound, map_source) — the edit's constants live on the host."""
        import numpy as np
        _need(points, torch.float32, "points")
        if mask.dtype != torch.uint8:
            raise RuntimeError("mask must be uint8")

        def hp(name):
            a = host.get(name)
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=np.float32)
            return a, a.ctypes.data_as(C.POINTER(C.c_float))
        keep = [hp(k) for k in ("triangles", "bounds", "inv_transform", "inv_rotation", "inv_scale", "center", "empty_bound",
                                "map_source")]
        ptr = [k[1] for k in keep]
        _check(lib().s3d_seal_bbox_map(_p(points), _p(dirs), _u(points.shape[0]), ptr[0], _u(keep[0][0].shape[0]), ptr[1],
                                       _u(keep[1][0].shape[0]), ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], ptr[7], _p(out_points),
                                       _p(out_dirs), _p(mask), _nv(n_valid), _stream()), "seal_bbox_map")


    @staticmethod
    def brush_map(points, dev, out_points, mask, n_valid=None):
        """brush tool (include/seal3d_hip.h: s3d_seal_brush_map); `dev`: the mapper's device constants (triangles, bounds,
        border as fp32 GPU tensors with their counts, normal_expand / center as 3 host floats, attenuation_distance, linear)"""
        import numpy as np
        _need(points, torch.float32, "points")
        if mask.dtype != torch.uint8:
            raise RuntimeError("mask must be uint8")
        ne = np.ascontiguousarray(dev["normal_expand"], dtype=np.float32)
        ce = np.ascontiguousarray(dev["center"], dtype=np.float32)
        fp = C.POINTER(C.c_float)
        border = dev["border"] if dev["n_border"] else None
        _check(lib().s3d_seal_brush_map(_p(points), _u(points.shape[0]), _p(dev["triangles"]), _u(dev["n_tris"]), _p(dev["bounds"]),
                                        _u(dev["n_bounds"]), _p(border), _u(dev["n_border"]), ne.ctypes.data_as(fp),
                                        ce.ctypes.data_as(fp), C.c_float(dev["attenuation_distance"]), C.c_int(1 if dev["linear"] else 0),
                                        _p(out_points), _p(mask), _nv(n_valid), _stream()), "seal_brush_map")

    @staticmethod
    def anchor_map(points, dev, out_points, mask, flag, n_valid=None):
        """anchor tool (include/seal3d_hip.h: s3d_seal_anchor_map); `dev`: triangles (fp32 GPU tensor) + n_tris, bounds [2,3]
        and params [14] as host float32 arrays; `flag`: a 4-byte GPU scratch tensor"""
        import numpy as np
        _need(points, torch.float32, "points")
        if mask.dtype != torch.uint8:
            raise RuntimeError("mask must be uint8")
        bo = np.ascontiguousarray(dev["bounds"], dtype=np.float32)
        pa = np.ascontiguousarray(dev["params"], dtype=np.float32)
        if bo.size != 6 or pa.size != 14:
            raise RuntimeError("anchor_map: bounds [2,3] and params [14]")
        fp = C.POINTER(C.c_float)
        _check(lib().s3d_seal_anchor_map(_p(points), _u(points.shape[0]), _p(dev["triangles"]), _u(dev["n_tris"]), bo.ctypes.data_as(fp),
                                         pa.ctypes.data_as(fp), _p(out_points), _p(mask), _p(flag), _nv(n_valid), _stream()),
               "seal_anchor_map")

    @staticmethod
    def map_color(rgbs, mask, hsv, rgb_target, light_offset, out, stats=None, n_valid=None):
        """colour edit of the moved samples (include/seal3d_hip.h: s3d_seal_map_color); `hsv` / `rgb_target`: 3 floats or None"""
        if rgbs.dtype not in (torch.float32, torch.float16) or out.dtype != rgbs.dtype or not rgbs.is_contiguous() or not out.is_contiguous():
            raise RuntimeError("map_color: contiguous f32 / f16 colours")
        if mask.dtype != torch.uint8:
            raise RuntimeError("mask must be uint8")
        h = (C.c_float * 3)(*[float(v) for v in hsv]) if hsv is not None else None
        t = (C.c_float * 3)(*[float(v) for v in rgb_target]) if rgb_target is not None else None
        if t is not None and stats is None:
            stats = torch.empty(2, dtype=torch.int64, device=rgbs.device)
        _check(lib().s3d_seal_map_color(_p(rgbs), _p(mask), _u(rgbs.shape[0]), C.c_int(_dt(rgbs)), h, t, C.c_float(float(light_offset)),
                                        _p(out), _p(stats), _nv(n_valid), _stream()), "seal_map_color")

    @staticmethod
    def map_color_image(rgbs, points, mask, hsv, texture, quad, light_offset, out, stats=None, texel_out=None, n_valid=None):
        """texture painting of the moved samples (include/seal3d_hip.h: s3d_seal_map_color_image); `texture`: fp32 GPU tensor
        [H, W, 4] of (h, s, v, alpha) texels, `quad`: 14 host floats (o, ow, oh, normal, |ow|^2, |oh|^2), `hsv`: 3 floats or
        None, `texel_out`: optional int32 GPU tensor [M, 2] for the (idx_h, idx_w) of the masked rows"""
        import numpy as np
        if rgbs.dtype not in (torch.float32, torch.float16) or out.dtype != rgbs.dtype or not rgbs.is_contiguous() or not out.is_contiguous():
            raise RuntimeError("map_color_image: contiguous f32 / f16 colours")
        if rgbs.dim() != 2 or rgbs.shape[1] != 3 or out.shape != rgbs.shape:
            raise RuntimeError("map_color_image: colours [M, 3]")
        _need(points, torch.float32, "points")
        if tuple(points.shape) != tuple(rgbs.shape) or mask.numel() != rgbs.shape[0]:
            raise RuntimeError("map_color_image: one point [3] and one mask byte per colour row")
        if mask.dtype != torch.uint8:
            raise RuntimeError("mask must be uint8")
        _need(texture, torch.float32, "texture")
        if texture.dim() != 3 or texture.shape[2] != 4:
            raise RuntimeError("map_color_image: texture [H, W, 4] of (h, s, v, alpha)")
        if texel_out is not None and (texel_out.dtype != torch.int32 or tuple(texel_out.shape) != (rgbs.shape[0], 2)):
            raise RuntimeError("map_color_image: texel_out must be int32 [M, 2]")
        q = np.ascontiguousarray(quad, dtype=np.float32)
        if q.size != 14:
            raise RuntimeError("map_color_image: quad [14]")
        h = (C.c_float * 3)(*[float(v) for v in hsv]) if hsv is not None else None
        if stats is None:
            stats = torch.empty(2, dtype=torch.int64, device=rgbs.device)
        _check(lib().s3d_seal_map_color_image(_p(rgbs), _p(points), _p(mask), _u(rgbs.shape[0]), C.c_int(_dt(rgbs)), h, _p(texture),
                                              _u(texture.shape[0]), _u(texture.shape[1]), q.ctypes.data_as(C.POINTER(C.c_float)),
                                              C.c_float(float(light_offset)), _p(out), _p(stats), _p(texel_out), _nv(n_valid),
                                              _stream()), "seal_map_color_image")


def _zeros_like_many(tensors, words=0):
    """zero tensors shaped like `tensors` (fp32, contiguous) + `words` zero int32 words, carved out of ONE filled buffer: one fill
    launch instead of one per tensor (seven to eight ~5 us launches per factor backward otherwise); segments start on 16 bytes"""
    sizes = [(t.numel() + 3) // 4 * 4 for t in tensors]
    flat = torch.zeros(sum(sizes) + (words + 3) // 4 * 4, dtype=torch.float32, device=tensors[0].device)
    out, off = [], 0
    for t, n in zip(tensors, sizes):
        out.append(flat[off:off + t.numel()].view(t.shape))
        off += n
    return out, (flat[off:off + words].view(torch.int32) if words else None)


def _native_bins(x, rank, res, n_bounds, n_valid):
    """(perm [6,N] i32, start [6,n_bounds] i32, n_bounds): the points of x sorted by plane tile (rows 0-2, `rank` decides the tile)
    and by 64-row line chunk (rows 3-5) in native launches — the sort both TensoRF backends' factor backward reads"""
    N, dev = x.shape[0], x.device
    perm = torch.empty(6, N, dtype=torch.int32, device=dev)
    start = torch.empty(6, n_bounds, dtype=torch.int32, device=dev)
    nbytes = int(lib().s3d_vm_backward_bins_workspace_size(_u(N), _u(n_bounds)))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _check(lib().s3d_vm_backward_bins(_p(x), _u(N), rank, res, _p(perm), _p(start), _u(n_bounds), _p(work), C.c_size_t(nbytes),
                                      _nv(n_valid), _stream()), "vm_backward_bins")
    return perm, start, n_bounds


def _rows_of_32(grad_out, N):
    """grad_out fp16 [N, Cb <= 32] as the colour backward kernels read it — a point's gradients as four 16-byte words: rows padded
    to 32 columns.  A [:, :Cb] view of a zero-padded [N, 32] buffer (FreqBackend.freq_encode_pack_backward's caller marks what it
    wrote, tensoRF/network.py: _MlpInput) is taken as it is: the buffer behind the view."""
    base = grad_out._base
    if (base is not None and getattr(base, "_s3d_zero_padded", False) and base.shape == (N, 32) and base.is_contiguous()
            and grad_out.data_ptr() == base.data_ptr() and grad_out.stride() == (32, 1)):
        return base
    return torch.nn.functional.pad(grad_out, (0, 32 - grad_out.shape[1])).contiguous()


class VmBackend:
    """csrc/tensorf.hip — TensoRF vector-matrix features (tensoRF/network.py:112-153 of the reference)"""

    @staticmethod
    def _factors(planes, lines, resolution, what="vm features"):
        """a factor set as the C calls take it: (planes pointers, lines pointers, rank, res, sum of the ranks).  The factors are
        fp32 contiguous GPU tensors (`what` names the caller in the message); `lines` is None where only the geometry is read."""
        for t in list(planes) + list(lines or ()):
            _need(t, torch.float32, "factor")
            if not t.is_cuda or not t.is_contiguous():
                raise RuntimeError(f"{what}: factors must be contiguous GPU tensors")
        ptr3, u3 = C.c_void_p * 3, C.c_uint32 * 3
        ranks = [int(t.shape[1]) for t in planes]
        return (ptr3(*[t.data_ptr() for t in planes]), None if lines is None else ptr3(*[t.data_ptr() for t in lines]),
                u3(*ranks), u3(*[int(r) for r in resolution]), sum(ranks))

    @staticmethod
    def features_forward(x, planes, lines, resolution, reduce, out, n_valid=None, shadows=None):
        """x [N,3] fp32; planes[i] [1,R_i,H,W] / lines[i] [1,R_i,D,1] fp32 (the reference's parameter shapes);
        out [N] (reduce) or [sum R_i, N]"""
        _need(x, torch.float32, "x"); _need(out, torch.float32, "out")
        pl, ln, rank, res, _ = VmBackend._factors(planes, lines, resolution)
        if not x.is_contiguous() or x.shape[-1] != 3:
            raise RuntimeError("vm features: x must be contiguous [N,3]")
        _check(lib().s3d_vm_features_forward(_p(x), _u(x.shape[0]), pl, ln, rank, res, C.c_int(int(bool(reduce))), _p(out),
                                             *_shadow2(shadows), _nv(n_valid), _stream()), "vm_features_forward")

    @staticmethod
    def _background_args(sph, dirs, plane, w0, w1, rgb, what):
        """shape / dtype checks shared by background_forward and background_backward; returns (N, R, H, W)"""
        for t, n in ((sph, "sph"), (dirs, "dirs"), (plane, "plane"), (w0, "w0"), (w1, "w1"), (rgb, "rgb")):
            _need(t, torch.float32, n)
        N = sph.shape[0]
        if (sph.shape != (N, 2) or dirs.shape != (N, 3) or rgb.shape != (N, 3) or plane.dim() != 4 or plane.shape[0] != 1
                or plane.shape[1] != 8 or min(plane.shape[2:]) < 2 or w0.shape != (64, 23) or w1.shape != (3, 64)):
            raise RuntimeError(f"{what}: sph [N,2], dirs / rgb [N,3], plane [1,8,H,W] with H, W >= 2, w0 [64,23], w1 [3,64]")
        return N, 8, int(plane.shape[2]), int(plane.shape[3])

    @staticmethod
    def background_forward(sph, dirs, plane, w0, w1, rgb, features=None):
        """the TensoRF background model (seal3d_hip.h: s3d_vm_background_forward): sph [N,2], dirs [N,3], plane `bg_mat` [1,8,H,W],
        w0 [64,23] / w1 [3,64] fp32 (read as fp16) -> rgb [N,3] fp32 (+ the plane samples [N,8] fp32)"""
        N, R, H, W = VmBackend._background_args(sph, dirs, plane, w0, w1, rgb, "vm background_forward")
        if features is not None and (features.dtype != torch.float32 or features.shape != (N, R)):
            raise RuntimeError("vm background_forward: features [N,8] fp32")
        _check(lib().s3d_vm_background_forward(_p(sph), _p(dirs), _p(plane), _u(R), _u(H), _u(W), _p(w0), _p(w1), _u(N), _p(rgb),
                                               _p(features), _stream()), "vm_background_forward")

    @staticmethod
    def background_backward(grad_rgb, rgb, sph, dirs, plane, w0, w1, grad_plane, grad_w0, grad_w1, found_inf=None):
        """backward of background_forward: ADDS the plane gradient into grad_plane (fp32, the plane's shape; None: no plane
        gradient), overwrites grad_w0 [64,23] / grad_w1 [3,64] (fp32); found_inf (optional fp32 [1]) raised for a non-finite gradient"""
        N, R, H, W = VmBackend._background_args(sph, dirs, plane, w0, w1, rgb, "vm background_backward")
        _need(grad_rgb, torch.float32, "grad_rgb"); _need(grad_w0, torch.float32, "grad_w0"); _need(grad_w1, torch.float32, "grad_w1")
        if (grad_rgb.shape != (N, 3) or grad_w0.shape != (64, 23) or grad_w1.shape != (3, 64)
                or (grad_plane is not None and (grad_plane.shape != plane.shape or grad_plane.dtype != torch.float32))):
            raise RuntimeError("vm background_backward: grad_rgb [N,3], grad_plane like plane, grad_w0 [64,23], grad_w1 [3,64]")
        ws, nb = _background_workspace(lib().s3d_vm_background_backward_workspace_size, N, sph.device, found_inf)
        _check(lib().s3d_vm_background_backward(_p(grad_rgb), _p(rgb), _p(sph), _p(dirs), _p(plane), _u(R), _u(H), _u(W), _p(w0), _p(w1),
                                                _u(N), _p(grad_plane), _p(grad_w0), _p(grad_w1), _p(found_inf), _p(ws), nb,
                                                _stream()), "vm_background_backward")

    @staticmethod
    def aabb_normalize(x, aabb, out):
        """out = 2 (x - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1 per row of x [N, 3] (seal3d_hip.h)"""
        _need(x, torch.float32, "x"); _need(aabb, torch.float32, "aabb"); _need(out, torch.float32, "out")
        if not (x.is_contiguous() and out.is_contiguous() and aabb.is_contiguous()) or x.shape[-1] != 3 or aabb.numel() != 6 or out.shape != x.shape:
            raise RuntimeError("aabb_normalize: contiguous x / out [N, 3], aabb [6]")
        _check(lib().s3d_aabb_normalize(_p(x), _p(aabb), _u(x.shape[0]), _p(out), _stream()), "aabb_normalize")

    @staticmethod
    def weighted_abs_sum(tensors, weights, out):
        """out (fp32 scalar tensor) = sum_i weights[i] * sum |tensors[i]| (seal3d_hip.h)"""
        _need(out, torch.float32, "out")
        n = len(tensors)
        for t in tensors:
            _need(t, torch.float32, "tensor")
            if not t.is_contiguous() or not t.is_cuda:
                raise RuntimeError("weighted_abs_sum: contiguous GPU tensors")
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
        numel = (C.c_uint64 * n)(*[t.numel() for t in tensors])
        ws = (C.c_float * n)(*[float(w) for w in weights])
        work = torch.empty(int(lib().s3d_weighted_abs_sum_workspace_size()) // 4, dtype=torch.float32, device=out.device)
        _check(lib().s3d_weighted_abs_sum(ptrs, numel, ws, C.c_int32(n), _p(out), _p(work), _stream()), "weighted_abs_sum")

    @staticmethod
    def _chain_args(mats, padded_rows, ld):
        n = len(mats)
        for m in mats:
            _need(m, torch.float32, "matrix")
            if m.dim() != 2 or not m.is_contiguous() or not m.is_cuda:
                raise RuntimeError("linear chain pack: contiguous fp32 GPU matrices")
        u = C.c_uint32 * n
        return ((C.c_void_p * n)(*[m.data_ptr() for m in mats]), u(*[m.shape[0] for m in mats]), u(*[m.shape[1] for m in mats]),
                u(*[int(r) for r in padded_rows]), u(*[int(v) for v in ld]), C.c_int32(n))

    @staticmethod
    def pack_linear_chain(mats, padded_rows, ld, flat):
        """flat fp16 = the matrices in the ffmlp layout, zero padded (seal3d_hip.h)"""
        _need(flat, torch.float16, "flat")
        if flat.numel() != sum(int(r) * int(v) for r, v in zip(padded_rows, ld)) or not flat.is_contiguous():
            raise RuntimeError("pack_linear_chain: flat holds sum(padded_rows * ld) elements")
        a = VmBackend._chain_args(mats, padded_rows, ld)
        _check(lib().s3d_pack_linear_chain(a[0], a[1], a[2], a[3], a[4], a[5], _p(flat), _stream()), "pack_linear_chain")

    @staticmethod
    def unpack_linear_chain(flat, mats, padded_rows, ld):
        """the matrices (fp32, the parameters' shapes) out of a flat fp16 vector in the ffmlp layout"""
        _need(flat, torch.float16, "flat")
        if flat.numel() != sum(int(r) * int(v) for r, v in zip(padded_rows, ld)) or not flat.is_contiguous():
            raise RuntimeError("unpack_linear_chain: flat holds sum(padded_rows * ld) elements")
        a = VmBackend._chain_args(mats, padded_rows, ld)
        _check(lib().s3d_unpack_linear_chain(_p(flat), a[0], a[1], a[2], a[3], a[4], a[5], _stream()), "unpack_linear_chain")

    # False (test reference): keys + torch.sort + searchsorted, the twin of s3d_vm_backward_bins
    native_bins = True

    @staticmethod
    def backward_bins(x, planes, resolution, n_valid=None):
        """(perm [6,N] i32, start [6,n_bounds] i32, n_bounds): the points sorted by plane tile / line chunk, as the backward
        kernels want them.  Depends on x and the resolution only — the density and the colour factors of one network share it."""
        N, dev = x.shape[0], x.device
        _, _, rank, res, _ = VmBackend._factors(planes, None, resolution)
        n_bounds = int(lib().s3d_vm_backward_max_bins(res)) + 2
        if VmBackend.native_bins:
            return _native_bins(x, rank, res, n_bounds, n_valid)
        if n_valid is not None:
            raise RuntimeError("vm backward bins: the torch.sort twin (A/B) has no padded-batch form")
        keys = torch.empty(6, N, dtype=torch.int32, device=dev)
        _check(lib().s3d_vm_backward_keys(_p(x), _u(N), rank, res, _p(keys), _stream()), "vm_backward_keys")
        # (A/B path: the same list through torch.sort — one sort over all six rows, row number above the key bits)
        bits = max(int(n_bounds).bit_length(), 1)
        if bits > 27:
            raise RuntimeError("vm features backward: resolution too large for 32-bit sort keys")
        rows6 = torch.arange(6, dtype=torch.int32, device=dev).unsqueeze(1)
        skeys, order = torch.sort(((rows6 << bits) | keys.clamp_(max=(1 << bits) - 1)).view(-1), stable=True)
        bounds = (rows6 << bits) | torch.arange(n_bounds, dtype=torch.int32, device=dev).unsqueeze(0)
        start = (torch.searchsorted(skeys, bounds.view(-1)).view(6, n_bounds) - rows6 * N).to(torch.int32).contiguous()
        perm = (order.view(6, N) - rows6.long() * N).to(torch.int32).contiguous()
        return perm, start, n_bounds

    @staticmethod
    def transpose_factors(planes, lines, resolution):
        """rank-fastest shadows of a factor set (s3d_vm_transpose_factors): ([H, W, R_i] x 3, [Dn, R_i] x 3) fp32, from the CURRENT
        values of the parameters — the caller takes them afresh whenever the parameters may have changed"""
        pl, ln, rank, res, _ = VmBackend._factors(planes, lines, resolution, "vm transpose")
        ptr3 = C.c_void_p * 3
        pt = [torch.empty(t.shape[2], t.shape[3], t.shape[1], dtype=torch.float32, device=t.device) for t in planes]
        lt = [torch.empty(t.shape[2], t.shape[1], dtype=torch.float32, device=t.device) for t in lines]
        _check(lib().s3d_vm_transpose_factors(pl, ln, rank, res, ptr3(*[t.data_ptr() for t in pt]), ptr3(*[t.data_ptr() for t in lt]),
                                              _stream()), "vm_transpose_factors")
        return pt, lt

    @staticmethod
    def _backward_buffers(x, planes, lines, resolution, rank, res, rows, bins, n_valid, extra=()):
        """what a factor backward allocates: (perm, start, n_bounds, gm, gs, bound_words, line_scratch, stage).  `bins`: a
        backward_bins() result or None (taken here); gs: zeroed gradients shaped like planes + lines + extra, in one buffer with
        the 4 bound words; stage: staging rows of the flushes (s3d_vm_backward_stage_bytes; uint8, no initialisation).
        The callers keep every one of them in a named local until the call has returned: temporaries created inside the
        argument list would be freed one by one and handed the SAME block."""
        N, dev = x.shape[0], x.device
        perm, start, n_bounds = bins if bins is not None else VmBackend.backward_bins(x, planes, resolution, n_valid)
        gm = torch.empty(N, rows, dtype=torch.float32, device=dev)  # (written by the plane pass for every point the line pass reads)
        gs, bound_words = _zeros_like_many(list(planes) + list(lines) + list(extra), 4)
        line_scratch = torch.empty(sum(t.numel() for t in lines), dtype=torch.float32, device=dev)
        stage = torch.empty(int(lib().s3d_vm_backward_stage_bytes(_u(N), rank, res)), dtype=torch.uint8, device=dev)
        return perm, start, n_bounds, gm, gs, bound_words, line_scratch, stage

    @staticmethod
    def features_backward(x, planes, lines, resolution, reduce, grad, bins=None, found_inf=None, n_valid=None, shadows=None):
        """gradients of features_forward w.r.t. planes / lines (lists shaped like the factors).  grad: [N] (reduce) or
        [N, sum R_i] point-major.  `bins`: a backward_bins() result for the same x / resolution."""
        _need(x, torch.float32, "x"); _need(grad, torch.float32, "grad")
        N, ptr3 = x.shape[0], C.c_void_p * 3
        pl, ln, rank, res, rows = VmBackend._factors(planes, lines, resolution)
        if not grad.is_contiguous() or grad.numel() != (N if reduce else N * rows):
            raise RuntimeError("vm features backward: grad must be contiguous [N] / [N, sum rank]")
        perm, start, n_bounds, gm, gs, bound_words, line_scratch, stage = VmBackend._backward_buffers(
            x, planes, lines, resolution, rank, res, rows, bins, n_valid)
        g_planes, g_lines = gs[:3], gs[3:]
        _check(lib().s3d_vm_features_backward(_p(x), _u(N), pl, ln, rank, res, C.c_int(int(bool(reduce))),
                                              _p(grad), _p(perm), _p(start), _u(n_bounds), _p(gm),
                                              ptr3(*[t.data_ptr() for t in g_planes]), ptr3(*[t.data_ptr() for t in g_lines]),
                                              _p(bound_words), _p(line_scratch), _p(stage), C.c_size_t(stage.numel()), _p(found_inf),
                                              *_shadow1(shadows), _nv(n_valid), _stream()), "vm_features_backward")
        return g_planes, g_lines

    @staticmethod
    def color_forward(x, planes, lines, resolution, basis, out, n_valid=None, shadows=None):
        """colour products with basis_mat applied in the kernel: basis fp16 [Cb, sum R_i] (the Linear's weight), out fp16 [N, Cb]"""
        _need(x, torch.float32, "x"); _need(basis, torch.float16, "basis"); _need(out, torch.float16, "out")
        pl, ln, rank, res, rows = VmBackend._factors(planes, lines, resolution)
        if not x.is_contiguous() or x.shape[-1] != 3 or not basis.is_contiguous() or basis.shape[1] != rows:
            raise RuntimeError("vm color: x must be contiguous [N,3], basis contiguous [Cb, sum rank]")
        if not out.is_contiguous() or out.numel() != x.shape[0] * basis.shape[0]:
            raise RuntimeError("vm color: out must be contiguous [N, Cb]")
        _check(lib().s3d_vm_color_forward(_p(x), _u(x.shape[0]), pl, ln, rank, res, _p(basis), _u(basis.shape[0]), _p(out),
                                          *_shadow2(shadows), _nv(n_valid), _stream()), "vm_color_forward")

    @staticmethod
    def color_backward(x, planes, lines, resolution, basis, grad_out, bins=None, found_inf=None, n_valid=None, shadows=None):
        """gradients of color_forward w.r.t. planes / lines / basis from grad_out fp16 [N, Cb]: (g_planes, g_lines, g_basis fp32)"""
        _need(x, torch.float32, "x"); _need(basis, torch.float16, "basis"); _need(grad_out, torch.float16, "grad_out")
        N, ptr3 = x.shape[0], C.c_void_p * 3
        pl, ln, rank, res, rows = VmBackend._factors(planes, lines, resolution)
        if grad_out.shape != (N, basis.shape[0]) or not basis.is_contiguous() or basis.shape[1] != rows or basis.shape[0] > 32:
            raise RuntimeError("vm color backward: grad_out must be [N, Cb <= 32], basis contiguous [Cb, sum rank]")
        grad_out = _rows_of_32(grad_out, N)
        perm, start, n_bounds, gm, gs, bound_words, line_scratch, stage = VmBackend._backward_buffers(
            x, planes, lines, resolution, rank, res, rows, bins, n_valid, extra=[basis])
        g_planes, g_lines, g_basis = gs[:3], gs[3:6], gs[6]
        _check(lib().s3d_vm_color_backward(_p(x), _u(N), pl, ln, rank, res, _p(basis), _u(basis.shape[0]), _p(grad_out),
                                           _p(perm), _p(start), _u(n_bounds), _p(gm), ptr3(*[t.data_ptr() for t in g_planes]),
                                           ptr3(*[t.data_ptr() for t in g_lines]), _p(g_basis),
                                           _p(bound_words), _p(line_scratch), _p(stage), C.c_size_t(stage.numel()), _p(found_inf),
                                           *_shadow1(shadows), _nv(n_valid), _stream()), "vm_color_backward")
        return g_planes, g_lines, g_basis


class CpBackend:
    """csrc/tensorf_cp.hip — TensoRF CP features (tensoRF/network_cp.py:78-111 of the reference): three line factors
    [1,R,D_i,1] per factor set, equal ranks"""

    @staticmethod
    def _lines(lines, resolution, what):
        """(lines pointers, rank, res, R) of a line set as the C calls take it"""
        for t in lines:
            _need(t, torch.float32, "line factor")
            if not t.is_cuda or not t.is_contiguous() or t.dim() != 4 or t.shape[0] != 1 or t.shape[3] != 1:
                raise RuntimeError(f"{what}: lines must be contiguous [1,R,D,1] GPU tensors")
        ptr3, u3 = C.c_void_p * 3, C.c_uint32 * 3
        ranks = [int(t.shape[1]) for t in lines]
        if len(lines) != 3 or len(set(ranks)) != 1:
            raise RuntimeError(f"{what}: three lines of equal rank, got ranks {ranks}")
        for t, a in zip(lines, (2, 1, 0)):
            if int(t.shape[2]) != int(resolution[a]):
                raise RuntimeError(f"{what}: line of {t.shape[2]} rows along axis {a} of resolution {list(resolution)}")
        return ptr3(*[t.data_ptr() for t in lines]), u3(*ranks), u3(*[int(r) for r in resolution]), ranks[0]

    @staticmethod
    def _shadows(shadows):
        return None if shadows is None else (C.c_void_p * 3)(*[t.data_ptr() for t in shadows])

    @staticmethod
    def _x(x, what):
        _need(x, torch.float32, "x")
        if not x.is_contiguous() or x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError(f"{what}: x must be contiguous [N,3]")
        return x.shape[0]

    @staticmethod
    def transpose_lines(lines, resolution):
        """rank-fastest shadows [D_i, R] x 3 (fp32) from the CURRENT values of the lines (s3d_cp_transpose_lines)"""
        ln, rank, res, _ = CpBackend._lines(lines, resolution, "cp transpose_lines")
        lt = [torch.empty(t.shape[2], t.shape[1], dtype=torch.float32, device=t.device) for t in lines]
        _check(lib().s3d_cp_transpose_lines(ln, rank, res, (C.c_void_p * 3)(*[t.data_ptr() for t in lt]), _stream()), "cp_transpose_lines")
        return lt

    @staticmethod
    def features_forward(x, lines, resolution, reduce, out, n_valid=None, shadows=None):
        """x [N,3] fp32; lines[i] [1,R,D_i,1] fp32; out [N] (reduce) or [R, N]"""
        N = CpBackend._x(x, "cp features_forward")
        _need(out, torch.float32, "out")
        ln, rank, res, R = CpBackend._lines(lines, resolution, "cp features_forward")
        if not out.is_contiguous() or out.numel() != (N if reduce else N * R):
            raise RuntimeError("cp features_forward: out must be contiguous [N] / [R, N]")
        _check(lib().s3d_cp_features_forward(_p(x), _u(N), ln, rank, res, C.c_int(int(bool(reduce))), _p(out),
                                             CpBackend._shadows(shadows), _nv(n_valid), _stream()), "cp_features_forward")

    @staticmethod
    def color_forward(x, lines, resolution, basis, out, n_valid=None, shadows=None):
        """the products with basis_mat applied in the kernel: basis fp16 [Cb <= 32, R] (the Linear's weight), out fp16 [N, Cb]"""
        N = CpBackend._x(x, "cp color_forward")
        _need(basis, torch.float16, "basis"); _need(out, torch.float16, "out")
        ln, rank, res, R = CpBackend._lines(lines, resolution, "cp color_forward")
        if not basis.is_contiguous() or basis.dim() != 2 or basis.shape[1] != R or not out.is_contiguous() or out.numel() != N * basis.shape[0]:
            raise RuntimeError("cp color_forward: basis contiguous [Cb, R], out contiguous [N, Cb]")
        _check(lib().s3d_cp_color_forward(_p(x), _u(N), ln, rank, res, _p(basis), _u(basis.shape[0]), _p(out),
                                          CpBackend._shadows(shadows), _nv(n_valid), _stream()), "cp_color_forward")

    @staticmethod
    def backward_bins(x, resolution, n_valid=None):
        """(perm, start, n_bounds): the points sorted by 64-row line chunk — the sort of the VM backward (s3d_vm_backward_bins),
        whose rows 3-5 the CP backward reads.  Depends on x, the resolution and n_valid only: the density and the colour lines of
        one network share it."""
        CpBackend._x(x, "cp backward_bins")
        u3 = C.c_uint32 * 3
        rank, res = u3(1, 1, 1), u3(*[int(r) for r in resolution])
        return _native_bins(x, rank, res, int(lib().s3d_vm_backward_max_bins(res)) + 2, n_valid)

    @staticmethod
    def features_backward(x, lines, resolution, reduce, grad, bins=None, found_inf=None, n_valid=None, shadows=None):
        """gradients of features_forward w.r.t. the lines (a list shaped like them).  grad: [N] (reduce) or [N, R] point-major."""
        N = CpBackend._x(x, "cp features_backward")
        _need(grad, torch.float32, "grad")
        ln, rank, res, R = CpBackend._lines(lines, resolution, "cp features_backward")
        if not grad.is_contiguous() or grad.numel() != (N if reduce else N * R):
            raise RuntimeError("cp features_backward: grad must be contiguous [N] / [N, R]")
        if found_inf is not None:
            _need(found_inf, torch.float32, "found_inf")
        perm, start, n_bounds = bins if bins is not None else CpBackend.backward_bins(x, resolution, n_valid)
        gs, _ = _zeros_like_many(list(lines))
        _check(lib().s3d_cp_features_backward(_p(x), _u(N), ln, rank, res, C.c_int(int(bool(reduce))), _p(grad), _p(perm), _p(start),
                                              _u(n_bounds), (C.c_void_p * 3)(*[t.data_ptr() for t in gs]), _p(found_inf),
                                              CpBackend._shadows(shadows), _nv(n_valid), _stream()), "cp_features_backward")
        return gs

    @staticmethod
    def color_backward(x, lines, resolution, basis, grad_out, bins=None, found_inf=None, n_valid=None, shadows=None):
        """gradients of color_forward w.r.t. the lines and basis from grad_out fp16 [N, Cb]: (g_lines, g_basis fp32)"""
        N = CpBackend._x(x, "cp color_backward")
        _need(basis, torch.float16, "basis"); _need(grad_out, torch.float16, "grad_out")
        ln, rank, res, R = CpBackend._lines(lines, resolution, "cp color_backward")
        if grad_out.shape != (N, basis.shape[0]) or not basis.is_contiguous() or basis.shape[1] != R or basis.shape[0] > 32:
            raise RuntimeError("cp color_backward: grad_out must be [N, Cb <= 32], basis contiguous [Cb, R]")
        if found_inf is not None:
            _need(found_inf, torch.float32, "found_inf")
        grad_out = _rows_of_32(grad_out, N)
        perm, start, n_bounds = bins if bins is not None else CpBackend.backward_bins(x, resolution, n_valid)
        gs, _ = _zeros_like_many(list(lines) + [basis])
        g_lines, g_basis = gs[:3], gs[3]
        _check(lib().s3d_cp_color_backward(_p(x), _u(N), ln, rank, res, _p(basis), _u(basis.shape[0]), _p(grad_out), _p(perm), _p(start),
                                           _u(n_bounds), (C.c_void_p * 3)(*[t.data_ptr() for t in g_lines]), _p(g_basis), _p(found_inf),
                                           CpBackend._shadows(shadows), _nv(n_valid), _stream()), "cp_color_backward")
        return g_lines, g_basis


class _CcGroup(C.Structure):
    _fields_ = [("line", C.c_void_p * 3), ("plane", C.c_void_p * 3), ("s_vec", C.c_void_p), ("s_mat", C.c_void_p),
                ("rank_vec", C.c_uint32), ("rank_mat", C.c_uint32)]


class _CcGroupGrad(C.Structure):
    _fields_ = [("line", C.c_void_p * 3), ("plane", C.c_void_p * 3), ("s_vec", C.c_void_p), ("s_mat", C.c_void_p)]


class CcBackend:
    """csrc/tensorf_cc.hip — CCNeRF features (tensoRF/network_cc.py:128-250, :287-291 of the reference).  A group is the tuple
    (lines, planes, s_vec, s_mat): three lines [1,R,D_i,1] + s_vec [rows, R] and / or three planes [1,R,H_i,W_i] + s_mat [rows, R];
    an absent component is (None, None).  rows = 1 (degree 0: the density head) or 3 * degree^2 (colour, with directions)."""
    MAX_GROUPS, TABLE, MAX_DEGREE = 8, 7168, 4

    @staticmethod
    def refusal(groups, degree):
        """None, or why the kernels do not cover these groups (the network then takes the grid_sample route)"""
        if degree > CcBackend.MAX_DEGREE:
            return f"degree {degree} above {CcBackend.MAX_DEGREE}"
        if not 1 <= len(groups) <= CcBackend.MAX_GROUPS:
            return f"{len(groups)} groups (1 .. {CcBackend.MAX_GROUPS})"
        rows = 3 * degree * degree if degree else 1
        if all(s_vec is None and s_mat is None for _, _, s_vec, s_mat in groups):
            return "no component in any group"
        for lines, planes, s_vec, s_mat in groups:
            rank = (0 if s_vec is None else s_vec.shape[1]) + (0 if s_mat is None else s_mat.shape[1])
            if rank * rows > CcBackend.TABLE:
                return f"a group of rank {rank} with {rows} rows above the {CcBackend.TABLE}-float table"
            for t in list(lines or ()) + list(planes or ()) + [s for s in (s_vec, s_mat) if s is not None]:
                if not t.is_cuda or t.dtype != torch.float32:
                    return "factors must be fp32 GPU tensors"
        return None

    @staticmethod
    def _groups(groups, resolution, degree, what):
        why = CcBackend.refusal(groups, degree)
        if why is not None:
            raise RuntimeError(f"{what}: {why}")
        rows = 3 * degree * degree if degree else 1
        res = [int(r) for r in resolution]
        arr = (_CcGroup * len(groups))()
        for rec, (lines, planes, s_vec, s_mat) in zip(arr, groups):
            if (lines is None) != (s_vec is None) or (planes is None) != (s_mat is None):
                raise RuntimeError(f"{what}: a component is its three factors and its S")
            if s_vec is not None:
                rec.rank_vec = R = int(s_vec.shape[1])
                for i, t in enumerate(lines):
                    if tuple(t.shape) != (1, R, res[2 - i], 1) or not t.is_contiguous():
                        raise RuntimeError(f"{what}: line {i} must be contiguous [1,{R},{res[2 - i]},1], got {tuple(t.shape)}")
                    rec.line[i] = t.data_ptr()
                if tuple(s_vec.shape) != (rows, R) or not s_vec.is_contiguous():
                    raise RuntimeError(f"{what}: s_vec must be contiguous [{rows},{R}]")
                rec.s_vec = s_vec.data_ptr()
            if s_mat is not None:
                rec.rank_mat = R = int(s_mat.shape[1])
                for i, (m0, m1) in enumerate(((0, 1), (0, 2), (1, 2))):
                    t = planes[i]
                    if tuple(t.shape) != (1, R, res[m1], res[m0]) or not t.is_contiguous():
                        raise RuntimeError(f"{what}: plane {i} must be contiguous [1,{R},{res[m1]},{res[m0]}], got {tuple(t.shape)}")
                    rec.plane[i] = t.data_ptr()
                if tuple(s_mat.shape) != (rows, R) or not s_mat.is_contiguous():
                    raise RuntimeError(f"{what}: s_mat must be contiguous [{rows},{R}]")
                rec.s_mat = s_mat.data_ptr()
        return arr, (C.c_uint32 * 3)(*res)

    @staticmethod
    def _points(x, dirs, degree, what):
        _need(x, torch.float32, "x")
        if not x.is_contiguous() or x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError(f"{what}: x must be contiguous [N,3]")
        if (dirs is None) != (degree == 0):
            raise RuntimeError(f"{what}: directions go with a degree of 1 .. {CcBackend.MAX_DEGREE}, none with degree 0")
        if dirs is not None:
            _need(dirs, torch.float32, "dirs")
            if not dirs.is_contiguous() or dirs.shape != x.shape:
                raise RuntimeError(f"{what}: dirs must be contiguous [N,3]")
        return x.shape[0]

    @staticmethod
    def forward(x, dirs, groups, resolution, degree, residual, half, out, n_valid=None):
        """out fp32 [K_out, N] (degree 0, dirs None) or [K_out, N, 3]; K_out = len(groups) if residual else 1"""
        N = CcBackend._points(x, dirs, degree, "cc forward")
        arr, res = CcBackend._groups(groups, resolution, degree, "cc forward")
        _need(out, torch.float32, "out")
        if not out.is_contiguous() or out.numel() != (len(groups) if residual else 1) * N * (3 if degree else 1):
            raise RuntimeError("cc forward: out must be contiguous [K_out, N] / [K_out, N, 3]")
        if degree == 0:
            _check(lib().s3d_cc_features_forward(_p(x), _u(N), arr, _u(len(groups)), res, C.c_int(int(bool(residual))),
                                                 C.c_int(int(bool(half))), _p(out), _nv(n_valid), _stream()), "cc_features_forward")
        else:
            _check(lib().s3d_cc_color_forward(_p(x), _p(dirs), _u(N), arr, _u(len(groups)), res, _u(degree), C.c_int(int(bool(residual))),
                                              C.c_int(int(bool(half))), _p(out), _nv(n_valid), _stream()), "cc_color_forward")

    @staticmethod
    def backward(x, dirs, groups, resolution, degree, residual, half, grad, found_inf=None, n_valid=None):
        """parameter gradients of forward from grad fp32 [K_out, N] / [K_out, N, 3]: a list shaped like `groups`"""
        N = CcBackend._points(x, dirs, degree, "cc backward")
        arr, res = CcBackend._groups(groups, resolution, degree, "cc backward")
        _need(grad, torch.float32, "grad")
        if not grad.is_contiguous() or grad.numel() != (len(groups) if residual else 1) * N * (3 if degree else 1):
            raise RuntimeError("cc backward: grad must be contiguous [K_out, N] / [K_out, N, 3]")
        if found_inf is not None:
            _need(found_inf, torch.float32, "found_inf")
        flat = [t for lines, planes, s_vec, s_mat in groups
                for t in list(lines or ()) + list(planes or ()) + [s for s in (s_vec, s_mat) if s is not None]]
        zeros, _ = _zeros_like_many(flat)
        garr, out, it = (_CcGroupGrad * len(groups))(), [], iter(zeros)
        for rec, (lines, planes, s_vec, s_mat) in zip(garr, groups):
            gl = [next(it) for _ in lines] if lines is not None else None
            gp = [next(it) for _ in planes] if planes is not None else None
            gsv = next(it) if s_vec is not None else None
            gsm = next(it) if s_mat is not None else None
            for i in range(3):
                rec.line[i] = gl[i].data_ptr() if gl is not None else None
                rec.plane[i] = gp[i].data_ptr() if gp is not None else None
            rec.s_vec = gsv.data_ptr() if gsv is not None else None
            rec.s_mat = gsm.data_ptr() if gsm is not None else None
            out.append((gl, gp, gsv, gsm))
        if degree == 0:
            _check(lib().s3d_cc_features_backward(_p(x), _u(N), arr, _u(len(groups)), res, C.c_int(int(bool(residual))),
                                                  C.c_int(int(bool(half))), _p(grad), garr, _p(found_inf), _nv(n_valid), _stream()),
                   "cc_features_backward")
        else:
            _check(lib().s3d_cc_color_backward(_p(x), _p(dirs), _u(N), arr, _u(len(groups)), res, _u(degree),
                                               C.c_int(int(bool(residual))), C.c_int(int(bool(half))), _p(grad), garr, _p(found_inf),
                                               _nv(n_valid), _stream()), "cc_color_backward")
        return out


class MeshBackend:
    """Mesh export (csrc/mesh.hip): marching cubes on the device."""

    @staticmethod
    def marching_cubes(u, iso, bounds):
        """u [nx, ny, nz] fp32 on the GPU, bounds = 6 numbers or a tensor (min xyz, max xyz) -> (vertices [V, 3] float32 in
        world coordinates, triangles [T, 3] int32), both on u's device, in the fixed order of include/seal3d_hip.h.  The two
        totals are read on the host between the counting and the emitting pass (an export is not part of a step), so the
        call cannot run while the stream is being captured."""
        if not isinstance(u, torch.Tensor) or not u.is_cuda:
            raise RuntimeError("seal3d HIP backend needs GPU tensors (no CPU fallback in the product path)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("marching_cubes reads its totals on the host: it cannot be captured into a graph")
        _need(u, torch.float32, "u")
        if u.dim() != 3:
            raise RuntimeError(f"marching_cubes: u must be [nx, ny, nz], got {tuple(u.shape)}")
        u = u.contiguous()
        nx, ny, nz = u.shape
        if min(nx, ny, nz) < 2 or nx * ny * nz >= 2 ** 31:
            raise RuntimeError(f"marching_cubes: every axis needs at least 2 points and the volume fewer than 2^31, got {nx} x {ny} x {nz}")
        bounds = torch.as_tensor(bounds, dtype=torch.float32).reshape(6).to(u.device).contiguous()
        ws = _ws.get(lib().s3d_mc_workspace_bytes(_u(nx), _u(ny), _u(nz)), u.device)
        totals = torch.empty(2, dtype=torch.int64, device=u.device)  # (room for two uint32, 8-byte aligned)
        _check(lib().s3d_mc_count(_p(u), _u(nx), _u(ny), _u(nz), _f(iso), _p(ws), _p(totals), _stream()), "mc_count")
        V, T = (int(v) for v in totals.view(torch.int32)[:2].cpu().numpy().view("uint32"))
        if V == 0xFFFFFFFF or T == 0xFFFFFFFF:
            raise RuntimeError("marching_cubes: the mesh has 2^32 - 1 vertices or triangles, or more")
        vertices = torch.empty(V, 3, dtype=torch.float32, device=u.device)
        triangles = torch.empty(T, 3, dtype=torch.int32, device=u.device)
        _check(lib().s3d_mc_emit(_p(u), _u(nx), _u(ny), _u(nz), _f(iso), _p(ws), _p(bounds), _p(vertices), _u(V), _p(triangles), _u(T), _stream()),
               "mc_emit")
        return vertices, triangles


class PreviewBackend:
    """The tail of an interactive preview frame (csrc/preview.hip; include/seal3d_hip.h "interactive preview")."""

    @staticmethod
    def resolve(image, depth, H, W, to_srgb=False, rays_o=None, rays_d=None, return_pos=False, buffer=None, mode="image", masks=None,
                color=(1.0, 0.0, 0.0), alpha=1.0, spp=0):
        """seal3d_hip.h: s3d_preview_resolve.  image [rH, rW, 3], depth [rH, rW] fp32 (the renderer's output) -> frame_image
        [H, W, 3] (`image` itself where the two are equal: full resolution, no conversion), frame_depth [H, W] (and pos
        [H, W, 3] with `return_pos`, which needs the frame's rays and rH == H, rW == W).
        `buffer` [H, W, 3] fp32, the display buffer, is updated in place: `mode` image / depth, `masks` [K, H, W] uint8 painted
        with `color` at `alpha`, accumulated onto the `spp` frames it already holds."""
        H, W = int(H), int(W)
        _need(image, torch.float32, "image"); _need(depth, torch.float32, "depth")
        if image.dim() != 3 or image.shape[2] != 3 or tuple(depth.shape) != tuple(image.shape[:2]):
            raise RuntimeError("preview resolve: image [rH, rW, 3] and depth [rH, rW]")
        if mode not in ("image", "depth"):
            raise RuntimeError(f"preview resolve: mode is 'image' or 'depth', got {mode!r}")
        rH, rW = image.shape[:2]
        dev = image.device
        # (rendered at full resolution and not converted: the frame image IS the renderer's, handed back without a copy)
        same = (rH, rW) == (H, W) and not to_srgb
        frame_image = None if same else torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        frame_depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        pos = None
        if return_pos:
            if rays_o is None or rays_d is None or (rH, rW) != (H, W):
                raise RuntimeError("preview resolve: pos needs rays_o / rays_d of a frame rendered at full resolution")
            for t, n in ((rays_o, "rays_o"), (rays_d, "rays_d")):
                _need(t, torch.float32, n)
                if t.numel() != H * W * 3:
                    raise RuntimeError(f"preview resolve: {n} must hold {H * W} x 3 values")
            pos = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        K, col, ws = 0, None, None
        if buffer is not None:
            _need(buffer, torch.float32, "buffer")
            if tuple(buffer.shape) != (H, W, 3):
                raise RuntimeError(f"preview resolve: buffer must be [{H}, {W}, 3]")
            if masks is not None and masks.numel():
                _need(masks, torch.uint8, "masks")
                if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
                    raise RuntimeError(f"preview resolve: masks must be [K, {H}, {W}]")
                K = masks.shape[0]
                col = (C.c_float * 3)(*[float(v) for v in color])
            if mode == "depth":
                ws = torch.empty(1, dtype=torch.int32, device=dev)
        _check(lib().s3d_preview_resolve(_p(image), _p(depth), _u(rH), _u(rW), _u(H), _u(W), C.c_int(int(bool(to_srgb))),
                                         _p(rays_o if return_pos else None), _p(rays_d if return_pos else None), _p(frame_image),
                                         _p(frame_depth), _p(pos), _p(buffer), C.c_int(int(mode == "depth")), _p(masks if K else None),
                                         _u(K), col, C.c_double(float(alpha)), _u(spp), _p(ws), _stream()), "s3d_preview_resolve")
        return (image if same else frame_image), frame_depth, pos

    @staticmethod
    def mask_positions(masks, pos):
        """seal3d_hip.h: s3d_mask_positions_count / _emit.  masks [K, H, W] uint8, pos [H, W, 3] fp32 -> (rows [sum n_k, 3] fp32
        on the device, offsets: K + 1 host ints): rows[offsets[k]:offsets[k + 1]] = pos[masks[k] > 0] in numpy's order.  The
        offsets are read on the host between the two passes (the output's size depends on them): not capturable."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mask_positions reads its counts on the host: it cannot be captured into a graph")
        _need(masks, torch.uint8, "masks"); _need(pos, torch.float32, "pos")
        if masks.dim() != 3 or masks.shape[0] == 0 or pos.dim() != 3 or tuple(pos.shape) != (masks.shape[1], masks.shape[2], 3):
            raise RuntimeError("mask_positions: masks [K >= 1, H, W] and pos [H, W, 3]")
        K, H, W = masks.shape
        nbytes = lib().s3d_mask_positions_workspace_bytes(_u(K), _u(H), _u(W))
        if nbytes == 0:
            raise RuntimeError(f"mask_positions: {K} masks of {H} x {W} are empty or too large")
        ws = _ws.get(nbytes, masks.device)
        offsets = torch.empty(K + 1, dtype=torch.int64, device=masks.device)
        _check(lib().s3d_mask_positions_count(_p(masks), _u(K), _u(H), _u(W), _p(ws), _p(offsets), _stream()), "mask_positions_count")
        offs = [int(v) for v in offsets.cpu()]
        rows = torch.empty(offs[-1], 3, dtype=torch.float32, device=masks.device)
        _check(lib().s3d_mask_positions_emit(_p(masks), _u(K), _u(H), _u(W), _p(ws), _p(pos), _p(rows), _u(offs[-1]), _stream()),
               "mask_positions_emit")
        return rows, offs


class DnerfBackend:
    """D-NeRF glue (csrc/dnerf.hip): the two fp16 input rows din [B, 80] / sin [B, 112] of the deformation and the density
    network, the warp + grid lookup, and the two backward steps around the grid backward (include/seal3d_hip.h)."""

    DIN, SIN, GRID_COLS = 80, 112, 32

    @staticmethod
    def _rows(din, sin, B):
        for name, t, cols in (("din", din, DnerfBackend.DIN), ("sin", sin, DnerfBackend.SIN)):
            if t is None:
                continue
            _need(t, torch.float16, name)
            if tuple(t.shape) != (B, cols) or not t.is_contiguous():
                raise RuntimeError(f"{name} must be a contiguous fp16 [{B}, {cols}] tensor, got {tuple(t.shape)}")

    @staticmethod
    def encode_forward(x, t, din, sin, n_valid=None):
        """din and sin[:, 32:] from x fp32 [B, 3] and t fp32 (one element: one time for all rows; B elements: one per row)"""
        _need(x, torch.float32, "x"); _need(t, torch.float32, "t")
        B = x.shape[0]
        if x.dim() != 2 or x.shape[1] != 3 or t.numel() not in (1, B):
            raise RuntimeError("encode_forward: x [B, 3], t with 1 or B elements")
        DnerfBackend._rows(din, sin, B)
        # (t of one element is read with stride 0 whatever B is: a [1, 1] time serves a batch of one row as well)
        _check(lib().s3d_dnerf_encode_forward(_p(x), _p(t), _u(0 if t.numel() == 1 else 1), _u(B), _p(din), _p(sin), _nv(n_valid),
                                              _stream()), "dnerf_encode_forward")

    @staticmethod
    def warp_grid_forward(x, dout, embeddings, offsets, S, H, gridtype, align_corners, interp, bound, sin, xw, deform=None,
                          dy_dx=None, reg_sum=None, n_valid=None):
        _need(x, torch.float32, "x"); _need(dout, torch.float16, "dout"); _need(offsets, torch.int32, "offsets")
        _need(xw, torch.float32, "xw")
        B, L = x.shape[0], offsets.shape[0] - 1
        if tuple(dout.shape) != (B, 16) or tuple(xw.shape) != (B, 3) or embeddings.dim() != 2 or embeddings.shape[1] != 2:
            raise RuntimeError("warp_grid_forward: dout [B, 16], xw [B, 3], a table of two features per row")
        DnerfBackend._rows(None, sin, B)
        if deform is not None:
            _need(deform, torch.float32, "deform")
            if tuple(deform.shape) != (B, 3):
                raise RuntimeError("warp_grid_forward: deform must be [B, 3]")
        if dy_dx is not None and (dy_dx.dtype != embeddings.dtype or dy_dx.numel() != B * L * 6):
            raise RuntimeError("warp_grid_forward: dy_dx must hold [B, L, 3, 2] values of the table's dtype")
        ws, nb = None, 0
        if reg_sum is not None:
            _need(reg_sum, torch.float32, "reg_sum")
            nb = int(lib().s3d_dnerf_warp_grid_workspace_size(_u(B)))
            ws = _ws.get(nb, x.device)
        _check(lib().s3d_dnerf_warp_grid_forward(_p(x), _p(dout), _p(embeddings), _p(offsets), _u(B), _u(L), _f(S), _u(H), _u(gridtype),
                                                 C.c_int(int(align_corners)), _u(interp), C.c_int(_dt(embeddings)), _f(bound), _p(sin),
                                                 _p(xw), _p(deform), _p(dy_dx), _p(reg_sum), _p(ws), C.c_size_t(nb), _nv(n_valid),
                                                 _stream()), "dnerf_warp_grid_forward")

    @staticmethod
    def split_grad(grad_sin, grad_levels, n_valid=None):
        """grad_levels [L, B, 2] (fp16 or fp32) = the grid columns of grad_sin fp16 [B, 112], level-major"""
        B = grad_sin.shape[0]
        DnerfBackend._rows(None, grad_sin, B)
        if grad_levels.dim() != 3 or grad_levels.shape[1] != B or grad_levels.shape[2] != 2 or grad_levels.shape[0] > 16:
            raise RuntimeError("split_grad: grad_levels must be [L <= 16, B, 2]")
        _check(lib().s3d_dnerf_split_grad(_p(grad_sin), _u(B), _u(grad_levels.shape[0]), C.c_int(_dt(grad_levels)), _p(grad_levels),
                                          _nv(n_valid), _stream()), "dnerf_split_grad")

    @staticmethod
    def warp_backward(grad_xw, grad_scale, deform, coef, grad_dout, n_valid=None):
        _need(grad_dout, torch.float16, "grad_dout")
        B = grad_dout.shape[0]
        if tuple(grad_dout.shape) != (B, 16) or tuple(grad_xw.shape) != (B, 3):
            raise RuntimeError("warp_backward: grad_xw [B, 3], grad_dout [B, 16]")
        if coef is not None:
            _need(coef, torch.float32, "coef"); _need(deform, torch.float32, "deform")
            if tuple(deform.shape) != (B, 3):
                raise RuntimeError("warp_backward: deform must be [B, 3]")
        _check(lib().s3d_dnerf_warp_backward(_p(grad_xw), C.c_int(_dt(grad_xw)), _f(grad_scale), _p(deform if coef is not None else None),
                                             _p(coef), _u(B), _p(grad_dout), _nv(n_valid), _stream()), "dnerf_warp_backward")


class DnerfBasisBackend:
    """The density head of the D-NeRF temporal-basis backbone (csrc/dnerf_basis.hip; include/seal3d_hip.h): sigma =
    exp(half(h[:, :32] . sigma_basis)) and the colour net's input row [half(SH_4(d)) | h[:, 32:]], one kernel per direction."""

    ROW, CIN, BASIS = 64, 48, 32

    @staticmethod
    def _check_rows(h, sigma_basis, who):
        _need(h, torch.float16, "h"); _need(sigma_basis, torch.float16, "sigma_basis")
        if h.dim() != 2 or h.shape[1] != DnerfBasisBackend.ROW or sigma_basis.numel() != DnerfBasisBackend.BASIS:
            raise RuntimeError(f"{who}: h [B, 64] fp16, sigma_basis [32] fp16")
        return h.shape[0]

    @staticmethod
    def mid_forward(h, dirs, sigma_basis, sigma, color_in=None, n_valid=None):
        B = DnerfBasisBackend._check_rows(h, sigma_basis, "basis_mid_forward")
        _need(sigma, torch.float32, "sigma")
        if sigma.numel() != B:
            raise RuntimeError("basis_mid_forward: sigma must be [B]")
        if color_in is not None:
            _need(color_in, torch.float16, "color_in"); _need(dirs, torch.float32, "dirs")
            if tuple(color_in.shape) != (B, DnerfBasisBackend.CIN) or tuple(dirs.shape) != (B, 3):
                raise RuntimeError("basis_mid_forward: dirs [B, 3], color_in [B, 48]")
        _check(lib().s3d_dnerf_basis_mid_forward(_p(h), _p(dirs if color_in is not None else None), _p(sigma_basis), _u(B), _p(sigma),
                                                 _p(color_in), _nv(n_valid), _stream()), "dnerf_basis_mid_forward")

    @staticmethod
    def mid_backward(grad_color_in, grad_sigma, h, sigma_basis, grad_h, grad_sigma_basis=None, n_valid=None):
        B = DnerfBasisBackend._check_rows(h, sigma_basis, "basis_mid_backward")
        _need(grad_color_in, torch.float16, "grad_color_in"); _need(grad_h, torch.float16, "grad_h")
        if tuple(grad_color_in.shape) != (B, DnerfBasisBackend.CIN) or tuple(grad_h.shape) != (B, DnerfBasisBackend.ROW):
            raise RuntimeError("basis_mid_backward: grad_color_in [B, 48], grad_h [B, 64]")
        if grad_sigma is not None:
            _need(grad_sigma, torch.float32, "grad_sigma")
            if grad_sigma.numel() != B:
                raise RuntimeError("basis_mid_backward: grad_sigma must be [B]")
        ws, nb = None, 0
        if grad_sigma_basis is not None:
            _need(grad_sigma_basis, torch.float32, "grad_sigma_basis")
            if grad_sigma_basis.numel() != DnerfBasisBackend.BASIS:
                raise RuntimeError("basis_mid_backward: grad_sigma_basis must be [32]")
            nb = int(lib().s3d_dnerf_basis_mid_workspace_size(_u(B)))
            ws = _ws.get(nb, h.device)
        _check(lib().s3d_dnerf_basis_mid_backward(_p(grad_color_in), _p(grad_sigma), _p(h), _p(sigma_basis), _u(B), _p(grad_h),
                                                  _p(grad_sigma_basis), _p(ws), C.c_size_t(nb), _nv(n_valid), _stream()),
               "dnerf_basis_mid_backward")


class DnerfHyperBackend:
    """The 4-D grid lookup of the D-NeRF hyper backbone (csrc/dnerf_hyper.hip; include/seal3d_hip.h): features, the 4-D input row
    and the ambient column of the Jacobian from one launch; the transposition of the feature gradient and grad_ambient from one."""

    MAX_LEVELS = 16

    @staticmethod
    def _table(embeddings, offsets, who):
        _need(offsets, torch.int32, "offsets")
        L = offsets.shape[0] - 1
        if embeddings.dim() != 2 or embeddings.shape[1] != 2 or embeddings.dtype not in (torch.float16, torch.float32) \
                or not 1 <= L <= DnerfHyperBackend.MAX_LEVELS:
            raise RuntimeError(f"{who}: a table of two fp16 / fp32 features per row, 1 <= L <= 16")
        return L

    @staticmethod
    def grid_forward(x, ambient, embeddings, offsets, S, H, gridtype, align_corners, interp, bound, feat, x4=None, dy_da=None,
                     n_valid=None):
        """feat fp16 [B, 2L] (+ x4 fp32 [B, 4] = [x | ambient], dy_da [B, L, 2] in the table's dtype) from x fp32 [B, 3] and the one
        fp32 device word `ambient`"""
        _need(x, torch.float32, "x"); _need(ambient, torch.float32, "ambient"); _need(feat, torch.float16, "feat")
        L = DnerfHyperBackend._table(embeddings, offsets, "hyper grid_forward")
        B = x.shape[0]
        if x.dim() != 2 or x.shape[1] != 3 or ambient.numel() != 1 or tuple(feat.shape) != (B, 2 * L):
            raise RuntimeError(f"hyper grid_forward: x [B, 3], ambient of one element, feat [B, {2 * L}]")
        if x4 is not None:
            _need(x4, torch.float32, "x4")
            if tuple(x4.shape) != (B, 4):
                raise RuntimeError("hyper grid_forward: x4 must be [B, 4]")
        if dy_da is not None and (dy_da.dtype != embeddings.dtype or tuple(dy_da.shape) != (B, L, 2)):
            raise RuntimeError("hyper grid_forward: dy_da must be [B, L, 2] in the table's dtype")
        _check(lib().s3d_dnerf_hyper_grid_forward(_p(x), _p(ambient), _p(embeddings), _p(offsets), _u(B), _u(L), _f(S), _u(H),
                                                  _u(gridtype), C.c_int(int(align_corners)), _u(interp), C.c_int(_dt(embeddings)),
                                                  _f(bound), _p(feat), _p(x4), _p(dy_da), _nv(n_valid), _stream()),
               "dnerf_hyper_grid_forward")

    @staticmethod
    def backward_workspace_size(B):
        return int(lib().s3d_dnerf_hyper_backward_workspace_size(_u(B)))

    @staticmethod
    def grid_backward(grad_feat, dy_da, grad_scale, grad_levels, grad_ambient=None, n_valid=None):
        """grad_levels [L, B, 2] (fp16 or fp32) = grad_feat fp16 [B, 2L] transposed; grad_ambient fp32 [1] = grad_scale * the
        fixed-order sum of grad_feat . dy_da over the live rows (written when dy_da and grad_ambient are both given)"""
        _need(grad_feat, torch.float16, "grad_feat")
        if grad_levels.dim() != 3 or grad_levels.shape[2] != 2 or not 1 <= grad_levels.shape[0] <= DnerfHyperBackend.MAX_LEVELS \
                or grad_levels.dtype not in (torch.float16, torch.float32):
            raise RuntimeError("hyper grid_backward: grad_levels must be [L <= 16, B, 2], fp16 or fp32")
        L, B = grad_levels.shape[0], grad_levels.shape[1]
        if tuple(grad_feat.shape) != (B, 2 * L):
            raise RuntimeError(f"hyper grid_backward: grad_feat must be [B, {2 * L}]")
        if dy_da is not None and (dy_da.dtype != grad_levels.dtype or tuple(dy_da.shape) != (B, L, 2)):
            raise RuntimeError("hyper grid_backward: dy_da must be [B, L, 2] in grad_levels' dtype")
        ws, nb = None, 0
        if grad_ambient is not None:
            _need(grad_ambient, torch.float32, "grad_ambient")
            if grad_ambient.numel() != 1:
                raise RuntimeError("hyper grid_backward: grad_ambient must hold one element")
            if dy_da is not None:
                nb = DnerfHyperBackend.backward_workspace_size(B)
                ws = _ws.get(nb, grad_feat.device)
        _check(lib().s3d_dnerf_hyper_grid_backward(_p(grad_feat), _p(dy_da), _u(B), _u(L), C.c_int(_dt(grad_levels)), _f(grad_scale),
                                                   _p(grad_levels), _p(grad_ambient), _p(ws), C.c_size_t(nb), _nv(n_valid), _stream()),
               "dnerf_hyper_grid_backward")


class HierBackend:
    """The sampling path without the occupancy grid (csrc/hiersample.hip; include/seal3d_hip.h): stratified samples, inverse-CDF
    upsampling with the depth merge, weights, compositing and its backward.  S = num_steps, U = upsample_steps, K = S + U; rows
    of sigma, rgbs, weights, mask and the gradients are in the concatenated [coarse | fine] order, `order` maps depth-sorted
    slots to those columns (None: the identity, only with U = 0).  Every tensor fp32 unless noted; outputs are the caller's."""

    @staticmethod
    def max_samples():
        """the largest K = S + U the kernels take; above it every method raises and the renderer keeps its torch route"""
        return int(lib().s3d_hier_max_samples())

    @staticmethod
    def supports(S, U):
        return S >= 3 and U >= 0 and S + U <= HierBackend.max_samples()

    @staticmethod
    def _shape(who, S, U):
        if S < 3 or U < 0:
            raise RuntimeError(f"{who}: num_steps >= 3 and upsample_steps >= 0, got {S} and {U}")
        if S + U > HierBackend.max_samples():
            raise RuntimeError(f"{who}: num_steps + upsample_steps = {S + U} exceeds the cap of {HierBackend.max_samples()} samples per ray")

    @staticmethod
    def _rows(who, N, **tensors):
        """name=(tensor, dtype, trailing shape): [N, *shape], contiguous (None is skipped)"""
        for name, (t, dtype, shape) in tensors.items():
            if t is None:
                continue
            _need(t, dtype, name)
            if tuple(t.shape) != (N,) + tuple(shape) or not t.is_contiguous():
                raise RuntimeError(f"{who}: {name} must be a contiguous [{N}, {', '.join(map(str, shape))}] tensor, got {tuple(t.shape)}")

    @staticmethod
    def coarse_samples(rays_o, rays_d, aabb, min_near, num_steps, nears, fars, z, xyz, noise=None):
        f, S, N = torch.float32, int(num_steps), rays_o.shape[0]
        HierBackend._shape("coarse_samples", S, 0)
        HierBackend._rows("coarse_samples", N, rays_o=(rays_o, f, (3,)), rays_d=(rays_d, f, (3,)), nears=(nears, f, ()), fars=(fars, f, ()),
                          z=(z, f, (S,)), xyz=(xyz, f, (S, 3)), noise=(noise, f, (S,)))
        HierBackend._rows("coarse_samples", 6, aabb=(aabb, f, ()))
        _check(lib().s3d_hier_coarse_samples(_p(rays_o), _p(rays_d), _p(aabb), _u(N), _f(min_near), _u(S), _p(noise), _p(nears),
                                             _p(fars), _p(z), _p(xyz), _stream()), "hier_coarse_samples")

    @staticmethod
    def upsample(z, sigma, nears, fars, density_scale, u, rays_o, rays_d, aabb, upsample_steps, new_z, new_xyz, z_sorted, order):
        """u: [N, U] uniforms, or None for the deterministic torch.linspace(0.5 / U, 1 - 0.5 / U, U)"""
        f, N, S, U = torch.float32, z.shape[0], z.shape[1], int(upsample_steps)
        HierBackend._shape("upsample", S, U)
        if U < 1:
            raise RuntimeError("upsample: upsample_steps must be at least 1 (none: skip the call)")
        HierBackend._rows("upsample", N, z=(z, f, (S,)), sigma=(sigma, f, (S,)), nears=(nears, f, ()), fars=(fars, f, ()), u=(u, f, (U,)),
                          rays_o=(rays_o, f, (3,)), rays_d=(rays_d, f, (3,)), new_z=(new_z, f, (U,)), new_xyz=(new_xyz, f, (U, 3)),
                          z_sorted=(z_sorted, f, (S + U,)), order=(order, torch.int32, (S + U,)))
        HierBackend._rows("upsample", 6, aabb=(aabb, f, ()))
        _check(lib().s3d_hier_upsample(_p(z), _p(sigma), _p(nears), _p(fars), _f(density_scale), _p(u), _p(rays_o), _p(rays_d), _p(aabb),
                                       _u(N), _u(S), _u(U), _p(new_z), _p(new_xyz), _p(z_sorted), _p(order), _stream()), "hier_upsample")

    @staticmethod
    def _merged(who, num_steps, z_sorted, order):
        N, K, S = z_sorted.shape[0], z_sorted.shape[1], int(num_steps)
        HierBackend._shape(who, S, K - S)
        if order is None and K != S:
            raise RuntimeError(f"{who}: order may be omitted (the identity) only without upsampling")
        return N, K, S

    @staticmethod
    def weights(z_sorted, order, sigma_cat, nears, fars, density_scale, num_steps, weights, mask):
        """mask: a torch.bool (or uint8) tensor [N, K]"""
        f = torch.float32
        N, K, S = HierBackend._merged("weights", num_steps, z_sorted, order)
        HierBackend._rows("weights", N, z_sorted=(z_sorted, f, (K,)), order=(order, torch.int32, (K,)), sigma_cat=(sigma_cat, f, (K,)),
                          nears=(nears, f, ()), fars=(fars, f, ()), weights=(weights, f, (K,)))
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (N, K):
            raise RuntimeError(f"weights: mask must be a bool or uint8 [{N}, {K}] tensor")
        _check(lib().s3d_hier_weights(_p(z_sorted), _p(order), _p(sigma_cat), _p(nears), _p(fars), _f(density_scale), _u(N), _u(S),
                                      _u(K - S), _p(weights), _p(mask), _stream()), "hier_weights")

    @staticmethod
    def composite_forward(weights, rgbs, z_sorted, order, nears, fars, num_steps, weights_sum, depth, image):
        f = torch.float32
        N, K, S = HierBackend._merged("composite_forward", num_steps, z_sorted, order)
        HierBackend._rows("composite_forward", N, weights=(weights, f, (K,)), rgbs=(rgbs, f, (K, 3)), z_sorted=(z_sorted, f, (K,)),
                          order=(order, torch.int32, (K,)), nears=(nears, f, ()), fars=(fars, f, ()), weights_sum=(weights_sum, f, ()),
                          depth=(depth, f, ()), image=(image, f, (3,)))
        _check(lib().s3d_hier_composite_forward(_p(weights), _p(rgbs), _p(z_sorted), _p(order), _p(nears), _p(fars), _u(N), _u(S),
                                                _u(K - S), _p(weights_sum), _p(depth), _p(image), _stream()), "hier_composite_forward")

    @staticmethod
    def composite_backward(grad_image, grad_weights_sum, grad_depth, sigma_cat, rgbs, z_sorted, order, nears, fars, density_scale,
                           num_steps, grad_sigma_cat, grad_rgbs):
        """grad_image [N, 3], grad_weights_sum [N], grad_depth [N]: each may be None for zero"""
        f = torch.float32
        N, K, S = HierBackend._merged("composite_backward", num_steps, z_sorted, order)
        HierBackend._rows("composite_backward", N, grad_image=(grad_image, f, (3,)), grad_weights_sum=(grad_weights_sum, f, ()),
                          grad_depth=(grad_depth, f, ()), sigma_cat=(sigma_cat, f, (K,)), rgbs=(rgbs, f, (K, 3)),
                          z_sorted=(z_sorted, f, (K,)), order=(order, torch.int32, (K,)), nears=(nears, f, ()), fars=(fars, f, ()),
                          grad_sigma_cat=(grad_sigma_cat, f, (K,)), grad_rgbs=(grad_rgbs, f, (K, 3)))
        _check(lib().s3d_hier_composite_backward(_p(grad_image), _p(grad_weights_sum), _p(grad_depth), _p(sigma_cat), _p(rgbs),
                                                 _p(z_sorted), _p(order), _p(nears), _p(fars), _f(density_scale), _u(N), _u(S), _u(K - S),
                                                 _p(grad_sigma_cat), _p(grad_rgbs), _stream()), "hier_composite_backward")


class SdfBackend:
    """The SDF backbone's data path (csrc/sdf.hip; include/seal3d_hip.h "SDF"): signed distance and winding number of points against a
    triangle mesh, one dataset item's points, and the MAPE criterion with its gradient.  Every tensor fp32 unless noted; outputs
    are allocated here and returned."""

    @staticmethod
    def tile():
        """triangles per LDS tile of mesh_sdf (tests place F at its edges)"""
        return int(lib().s3d_mesh_sdf_tile())

    @staticmethod
    def _triangles(who, triangles):
        _need(triangles, torch.float32, "triangles")
        if triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3):
            raise RuntimeError(f"{who}: triangles must be [F, 3, 3], got {tuple(triangles.shape)}")
        return triangles.shape[0]

    @staticmethod
    def _query(who, points, want_winding, want_face, launch):
        """what mesh_sdf and mesh_sdf_bvh share: the points check, the outputs and their order; launch(N, sdf, winding, face)"""
        _need(points, torch.float32, "points")
        if points.dim() != 2 or points.shape[1] != 3:
            raise RuntimeError(f"{who}: points must be [N, 3], got {tuple(points.shape)}")
        N, dev = points.shape[0], points.device
        sdf = torch.empty(N, dtype=torch.float32, device=dev)
        winding = torch.empty(N, dtype=torch.float32, device=dev) if want_winding else None
        face = torch.empty(N, dtype=torch.int32, device=dev) if want_face else None
        launch(N, sdf, winding, face)
        out = (sdf,) + ((winding,) if want_winding else ()) + ((face,) if want_face else ())
        return out[0] if len(out) == 1 else out

    @staticmethod
    def mesh_sdf(points, triangles, want_winding=False, want_face=False):
        """points [N, 3], triangles [F, 3, 3] -> sdf [N] (negative inside), then winding [N] and nearest_face [N] int32 as asked"""
        F = SdfBackend._triangles("mesh_sdf", triangles)
        return SdfBackend._query("mesh_sdf", points, want_winding, want_face, lambda N, sdf, winding, face: _check(
            lib().s3d_mesh_sdf(_p(points), _u(N), _p(triangles), _u(F), _p(sdf), _p(winding), _p(face), _stream()), "mesh_sdf"))

    @staticmethod
    def bvh_leaf():
        """faces per leaf of the mesh BVH (sdf/bvh.py builds to it)"""
        return int(lib().s3d_mesh_bvh_leaf())

    @staticmethod
    def bvh_stage(triangles):
        """triangles [F, 3, 3] in the tree's sorted order -> staged [F, 20], the records a pair test of mesh_sdf_bvh reads"""
        F = SdfBackend._triangles("bvh_stage", triangles)
        staged = torch.empty(F, 20, dtype=torch.float32, device=triangles.device)
        _check(lib().s3d_mesh_bvh_stage(_p(triangles), _u(F), _p(staged), _stream()), "mesh_bvh_stage")
        return staged

    @staticmethod
    def mesh_sdf_bvh(points, bvh, beta=3.0, want_winding=False, want_face=False):
        """points [N, 3], bvh a sdf.bvh.MeshBVH -> what mesh_sdf returns: the same distance and nearest face bit for bit, the winding
        number through the tree's far-field terms (`beta`: a node farther than beta radii is taken as a dipole)"""
        def launch(N, sdf, winding, face):
            nodes, staged, perm = bvh.device_arrays(points.device)
            _check(lib().s3d_mesh_sdf_bvh(_p(points), _u(N), _p(nodes), _p(staged), _p(perm), _u(bvh.F), _u(bvh.L), _f(beta), _p(sdf),
                                          _p(winding), _p(face), _stream()), "mesh_sdf_bvh")
        return SdfBackend._query("mesh_sdf_bvh", points, want_winding, want_face, launch)

    @staticmethod
    def sample_points(triangles, cdf, N, key, step, noise_std=0.01, want_face=False):
        """one dataset item's points [N, 3] (surface | perturbed surface | uniform), a pure function of (key, step)"""
        F = SdfBackend._triangles("sample_points", triangles)
        _need(cdf, torch.float32, "cdf")
        N = int(N)
        if cdf.numel() != F or N < 0 or N % 8:
            raise RuntimeError(f"sample_points: cdf holds one value per triangle, num_samples must be divisible by 8, got {N}")
        points = torch.empty(N, 3, dtype=torch.float32, device=triangles.device)
        face = torch.empty(N, dtype=torch.int32, device=triangles.device) if want_face else None
        _check(lib().s3d_sdf_sample_points(_p(triangles), _p(cdf), _u(F), _u(N), _u(int(key) & 0xFFFFFFFF), _u(int(step) & 0xFFFFFFFF),
                                           _f(noise_std), _p(points), _p(face), _stream()), "sdf_sample_points")
        return (points, face) if want_face else points

    @staticmethod
    def mape_forward_backward(pred, target, clip=None, grad_scale=1.0):
        """pred fp16 [B, 16] (the MLP's padded rows, column 0 the distance) or fp32 [B, 1]; target [B] or [B, 1] -> (loss fp32
        scalar, grad laid out as pred)"""
        _need(target, torch.float32, "target")
        B = pred.shape[0]
        if pred.dim() != 2 or pred.shape[1] != (16 if pred.dtype == torch.float16 else 1) or target.numel() != B:
            raise RuntimeError("mape_forward_backward: pred is fp16 [B, 16] or fp32 [B, 1], target holds B values")
        dt = _dt(pred)
        nb = int(lib().s3d_sdf_mape_workspace_size(_u(B)))
        ws = _ws.get(nb, pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        _check(lib().s3d_sdf_mape_forward_backward(_p(pred), C.c_int(dt), _p(target), _u(B), _f(clip if clip else 0.0), _f(grad_scale),
                                                   _p(loss), _p(grad), _p(ws), C.c_size_t(ws.numel()), _stream()),
               "sdf_mape_forward_backward")
        return loss, grad
