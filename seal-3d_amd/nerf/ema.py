"""Exponential moving average of a model's parameters with torch_ema 0.3's interface and state layout (the reference's trainers
keep one: `ExponentialMovingAverage(model.parameters(), decay=ema_decay)`, nerf/utils.py:356-357, updated after every optimizer
step :733 / :882, swapped in for evaluation :774-785 / :919-1011 and for the `best` checkpoint :1060-1071, carried as `ema` in
full checkpoints :1034-1035).

    shadow -= (1 - d) * (shadow - param),   d = min(decay, (1 + n) / (10 + n)),   n = updates so far, this one included

as three fp32 roundings per element (tmp = s - p; tmp.mul_(c); s.sub_(tmp) with c = float32(1 - d)).  On the GPU every fp32
parameter is updated by one launch of s3d_ema_update_multi (csrc/ema.hip: 12 B per parameter instead of 32, one launch instead
of three per tensor, bit-identical); the update count lives in device memory, so the launch can be captured in a HIP graph and a
replay uses the count of its own time.  On the CPU, and for a parameter that is not fp32, the three torch ops run.

`average_parameters()` on the GPU swaps parameters and shadows BY VALUE (s3d_ema_exchange_multi) on entry and again on exit:
no third copy of the model, the restore is exact, and no tensor moves — a captured training step, which holds the parameters'
addresses, replays unchanged afterwards."""
import contextlib

import torch


def weights_changed(optimizer=None):
    """The fp32 parameters were written from outside the optimizer (checkpoint load, an EMA's swap / copy_to / restore): the fp16
    copies the kernels read — eval cache of the tables, packed MLP weights, the optimizer's hand-over copies — follow them."""
    from gridencoder.grid import bump_weights_epoch
    bump_weights_epoch()
    resync = getattr(optimizer, "resync_half", None)
    if resync is not None:
        resync()


def decay_at(decay, num_updates):
    """the decay of update number `num_updates` (counted from 1) under torch_ema's warm-up; None: the constant decay"""
    if num_updates is None:
        return decay
    return min(decay, (1 + num_updates) / (10 + num_updates))


class NativeEMA:
    """torch_ema.ExponentialMovingAverage(parameters, decay, use_num_updates): shadows of ALL given parameters in the given order
    (frozen ones included — freezing a module later does not change the list).  `on_weights_changed`: called after the
    parameters' values were replaced (copy_to, restore, both ends of average_parameters)."""

    def __init__(self, parameters, decay, use_num_updates=True, on_weights_changed=None):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = float(decay)
        self.use_num_updates = bool(use_num_updates)
        self.on_weights_changed = on_weights_changed
        self.collected_params = None
        self.reseed(parameters)

    def reseed(self, parameters=None):
        """start over from the current values of `parameters` (default: the ones on hand): fresh shadows, update count 0"""
        if parameters is not None:
            self._params = list(parameters)
        self.shadow_params = [p.clone().detach() for p in self._params]
        self.collected_params = None
        dev = self._params[0].device if self._params else torch.device("cpu")
        # the number of updates so far: device memory next to the parameters, read back by state_dict() alone
        self._count = torch.zeros(1, dtype=torch.int64, device=dev) if self.use_num_updates else None

    def _parameters(self, parameters):
        if parameters is None:
            return self._params
        parameters = list(parameters)
        if len(parameters) != len(self.shadow_params):
            raise ValueError(f"Number of parameters passed as argument is different from number of shadow parameters maintained "
                             f"by this ExponentialMovingAverage ({len(parameters)} != {len(self.shadow_params)})")
        return parameters

    @staticmethod
    def _native(p, s):
        return (p.is_cuda and s.is_cuda and p.dtype == torch.float32 and s.dtype == torch.float32 and p.is_contiguous()
                and s.is_contiguous() and p.device == s.device)

    def _pairs(self, parameters):
        native, other = [], []
        for p, s in zip(parameters, self.shadow_params):
            (native if self._native(p, s) else other).append((p.detach(), s))
        return native, other

    @torch.no_grad()
    def update(self, parameters=None):
        """one update from the parameters' current values.  Takes no overflow flag: on a step the loss scaler skipped the
        parameters are unchanged, the count advances and the shadows move toward them, as in the reference."""
        native, other = self._pairs(self._parameters(parameters))
        count = self._count
        if other:
            if count is None:
                c = 1.0 - self.decay
            elif count.is_cuda:  # (no host read: the coefficient is formed on the device, from the count before the launch advances it)
                n = (count + 1).to(torch.float64)
                c = (1.0 - torch.clamp((1.0 + n) / (10.0 + n), max=self.decay)).to(torch.float32).reshape(())
            else:
                c = 1.0 - decay_at(self.decay, int(count) + 1)
            for p, s in other:
                tmp = s - p.to(s.dtype)
                tmp.mul_(c)
                s.sub_(tmp)
        if native:
            import s3d_hip
            s3d_hip.EmaBackend.update_multi(native, self.decay, count, use_num_updates=self.use_num_updates)  # (advances the count)
        elif count is not None:
            count += 1

    @torch.no_grad()
    def copy_to(self, parameters=None):
        for s, p in zip(self.shadow_params, self._parameters(parameters)):
            p.data.copy_(s.data)
        self._changed()

    @torch.no_grad()
    def store(self, parameters=None):
        self.collected_params = [p.clone() for p in self._parameters(parameters)]

    @torch.no_grad()
    def restore(self, parameters=None):
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        for c, p in zip(self.collected_params, self._parameters(parameters)):
            p.data.copy_(c.data)
        self._changed()

    def _changed(self):
        if self.on_weights_changed is not None:
            self.on_weights_changed()

    @torch.no_grad()
    def _exchange(self, parameters):
        native, other = self._pairs(parameters)
        if native:
            import s3d_hip
            s3d_hip.EmaBackend.exchange_multi(native)
        for p, s in other:
            tmp = p.clone()
            p.copy_(s.to(p.dtype))
            s.copy_(tmp.to(s.dtype))
        self._changed()

    @contextlib.contextmanager
    def average_parameters(self, parameters=None):
        """the parameters hold the averaged values inside the block and their own values, bit for bit, after it.  GPU: swapped
        with the shadows by value (no extra memory; do not update() inside the block); CPU: store / copy_to / restore."""
        parameters = self._parameters(parameters)
        swap = any(p.is_cuda for p in parameters)
        if swap:
            self._exchange(parameters)
        else:
            self.store(parameters)
            self.copy_to(parameters)
        try:
            yield
        finally:
            if swap:
                self._exchange(parameters)
            else:
                self.restore(parameters)
                self.collected_params = None

    def state_dict(self):
        """torch_ema's layout; the one place that reads the update count back from the device"""
        return {"decay": self.decay, "num_updates": None if self._count is None else int(self._count.item()),
                "shadow_params": self.shadow_params, "collected_params": self.collected_params}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        decay, num_updates = state_dict["decay"], state_dict["num_updates"]
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        if not (num_updates is None or isinstance(num_updates, int)):
            raise TypeError("Invalid num_updates")
        shadow, collected = state_dict["shadow_params"], state_dict["collected_params"]
        for name, lst in (("shadow_params", shadow), ("collected_params", collected)):
            if lst is None and name == "collected_params":
                continue
            if not isinstance(lst, list):
                raise TypeError(f"{name} must be a list")
            if not all(isinstance(t, torch.Tensor) for t in lst):
                raise TypeError(f"{name} must all be Tensors")
            if len(lst) != len(self._params):
                raise ValueError(f"{name} and the parameters have different length ({len(lst)} != {len(self._params)})")
            for t, p in zip(lst, self._params):
                if t.shape != p.shape:
                    raise ValueError(f"{name}: shape {tuple(t.shape)} does not fit the parameter's {tuple(p.shape)}")
        self.decay = float(decay)
        self.use_num_updates = num_updates is not None
        # (written in place where a tensor of the right kind exists: a captured update holds the shadows' and the count's addresses)
        for k, (t, p) in enumerate(zip(shadow, self._params)):
            s = self.shadow_params[k]
            if s.device == p.device and s.dtype == p.dtype and s.shape == p.shape:
                s.copy_(t)
            else:
                self.shadow_params[k] = t.to(device=p.device, dtype=p.dtype).clone()
        self.collected_params = None if collected is None else \
            [t.to(device=p.device, dtype=p.dtype).clone() for t, p in zip(collected, self._params)]
        if num_updates is None:
            self._count = None
        elif self._count is None:
            dev = self._params[0].device if self._params else torch.device("cpu")
            self._count = torch.full((1,), num_updates, dtype=torch.int64, device=dev)
        else:
            self._count.fill_(num_updates)
