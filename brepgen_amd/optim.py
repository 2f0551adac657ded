"""The update half of a trainer iteration on the MI355X: what every one of the reference's six trainers runs after its loss,

    self.scaler.scale(total_loss).backward()
    nn.utils.clip_grad_norm_(self.network_params, max_norm=50.0)
    self.scaler.step(self.optimizer)                   # torch.optim.AdamW
    self.scaler.update()

as three launches with no host synchronisation (csrc/optim.hip):

    AdamW            torch.optim.AdamW's surface and state_dict layout         -> bg_mt_grad_stats, bg_mt_adamw_step, bg_optim_finish
    GradScaler       torch.amp.GradScaler's: scale / step / update / get_scale -> the same launches, with the scale on the device
    clip_grad_norm_  nn.utils.clip_grad_norm_ (2-norm)                         -> bg_mt_grad_stats, bg_mt_scale_grads

The four lines above run unchanged with these three names swapped in.  `scaler.step(optimizer, max_norm=50.0)` is the fused form of
lines two and three: the same bits in p, exp_avg and exp_avg_sq, one pass less over the gradients.

Differences from torch, all deliberate:
  * a step is skipped when a gradient is non-finite AFTER clipping and unscaling (torch looks before unscaling, so a scale below 1 can
    push an inf into its parameters); the host never learns whether a step was skipped -- `get_scale()` and `state_dict()` are the calls
    that synchronise;
  * the fused `step` leaves `.grad` as backward() wrote it (torch leaves it clipped and unscaled); the next zero_grad discards it;
  * one step counter per optimiser, advanced by every step that is not skipped: a parameter whose `.grad` is None in some steps is left
    out of them as in torch, but its bias correction follows the optimiser's counter;
  * `unscale_`, `amsgrad`, `maximize`, 16-bit parameters and more than one device are not provided.
Parameters and gradients are fp32, contiguous and on the device; anything else raises (ValueError, or BrepgenHipError for CPU tensors:
there is no CPU fallback).  tests/optim_restate.py states the arithmetic in numpy.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, stream
from ._train import require_device

CHUNK, MAX_BLOCKS = 4096, 2048                     # BG_OPTIM_CHUNK, BG_OPTIM_MAX_BLOCKS of include/brepgen_hip.h

_ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("lr", "<f8"), ("decay", "<f4"),
                 ("has_decay", "<i4")])
_CHUNK = np.dtype([("first", "<i8"), ("tensor", "<i4"), ("_pad", "<i4")])
assert _ROW.itemsize == C.sizeof(_lib.MtRow) and _CHUNK.itemsize == C.sizeof(_lib.MtChunk)

# the group keys of torch.optim.AdamW's state_dict that this optimiser does not act on, with the values a torch optimiser needs to
# continue from ours as AdamW (decoupled decay, single-tensor or foreach as it likes)
_TORCH_GROUP_DEFAULTS = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                         "fused": None, "decoupled_weight_decay": True}


def _check_param(p, what="parameter"):
    if not torch.is_tensor(p):
        raise TypeError(f"optimizer can only optimize Tensors, but one of the params is {type(p).__name__}")
    if p.dtype != torch.float32:
        raise ValueError(f"{what}: expected torch.float32, got {p.dtype} (16-bit parameters and moments are not provided)")
    if not p.is_contiguous():
        raise ValueError(f"{what} of shape {tuple(p.shape)} is not contiguous")


def _chunks_of(numels):
    """The chunk list of tensors of `numels` elements: (tensor, first element) per CHUNK elements, the last chunk of a tensor short."""
    numels = np.asarray(numels, dtype=np.int64)
    counts = -(-numels // CHUNK)
    total = int(counts.sum())
    chunks = np.zeros(total, _CHUNK)
    chunks["tensor"] = np.repeat(np.arange(len(numels), dtype=np.int32), counts)
    chunks["first"] = (np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)) * CHUNK
    return chunks


class _Lists:
    """The device-resident table and chunk list of one caller, re-uploaded only when their bytes changed: asynchronously, from one
    of two pinned staging buffers; a buffer is written again only after the copy that last read it has finished."""

    def __init__(self):
        self.key, self.dev, self.n_chunks, self.chunk_off = None, None, 0, 0
        self.stage, self.events, self.turn = [None, None], [None, None], 0
        self.partials = None

    def sync(self, rows, device):
        key = rows.tobytes()
        if self.partials is None or self.partials.device != device:
            self.partials = torch.empty(MAX_BLOCKS * 16, dtype=torch.uint8, device=device)
            self.key, self.dev = None, None
        if key == self.key:
            return
        chunks = _chunks_of(rows["numel"])
        total = len(chunks)
        self.chunk_off = -(-len(key) // 16) * 16
        blob = key + b"\0" * (self.chunk_off - len(key)) + chunks.tobytes()
        n = max(len(blob), 16)
        k = self.turn
        self.turn ^= 1
        if self.stage[k] is None or self.stage[k].numel() < n:
            self.stage[k], self.events[k] = torch.empty(max(n, 4096), dtype=torch.uint8).pin_memory(), None
        if self.events[k] is not None:
            self.events[k].synchronize()           # the upload before last; long finished unless the table changes at every step
        self.stage[k][:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        if self.dev is None or self.dev.numel() < n:
            self.dev = torch.empty(max(n, 4096), dtype=torch.uint8, device=device)
        self.dev[:n].copy_(self.stage[k][:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k], self.key, self.n_chunks = ev, key, total

    @property
    def table(self):
        return self.dev.data_ptr()

    @property
    def chunks(self):
        return self.dev.data_ptr() + self.chunk_off


def _struct_tensor(st, device):
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(device)


def _beta_pow(beta, step):
    x = 1.0
    for _ in range(int(step)):                    # the device keeps beta ** step as `step` fp64 multiplications: rebuilt the same way
        x *= beta
    return x


class AdamW:
    """torch.optim.AdamW on the device (see the module docstring).  `owners`: objects whose `invalidate()` is called after every
    enqueued step -- the brepgen_amd modules that cache packed copies of the parameters this optimiser rewrites."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, owners=()):
        if torch.is_tensor(params):
            raise TypeError("params argument given to the optimizer should be an iterable of Tensors or dicts")
        params = list(params)
        if not params:
            raise ValueError("optimizer got an empty parameter list")
        if not isinstance(params[0], dict):
            params = [{"params": params}]
        self.defaults = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, **_TORCH_GROUP_DEFAULTS}
        self.param_groups, seen = [], set()
        for g in params:
            g = dict(g)
            ps = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])
            for p in ps:
                _check_param(p)
                if id(p) in seen:
                    raise ValueError("some parameters appear in more than one parameter group")
                seen.add(id(p))
            g["params"] = ps
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            g["betas"] = tuple(g["betas"])
            self.param_groups.append(g)
        self._check_groups()
        self.owners = tuple(owners)
        self.state = {}                            # param -> {"exp_avg", "exp_avg_sq"} (fp32, contiguous, the param's device)
        self._step, self._state_dev = 0, None      # the counter as last known on the host / the device block (made at the first step)
        self._lists, self._pending, self._slots = _Lists(), None, {}

    def _check_groups(self):
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise ValueError("betas and eps must be equal across parameter groups (lr and weight_decay may differ)")
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("amsgrad and maximize are not provided")
            b1, b2 = g["betas"]
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g["eps"] >= 0.0 and g["lr"] >= 0.0 and g["weight_decay"] >= 0.0):
                raise ValueError(f"invalid hyper-parameters: lr={g['lr']} betas={g['betas']} eps={g['eps']} weight_decay={g['weight_decay']}")

    def _moments(self, p):
        """(address of exp_avg, address of exp_avg_sq, numel) of a parameter that is about to be stepped; the moments are created (zeros)
        or validated once and remembered until `state[p]` or its tensors are replaced."""
        st = self.state.get(p)
        c = self._slots.get(id(p))
        if c is not None and st is c[0] and st.get("exp_avg") is c[1] and st.get("exp_avg_sq") is c[2]:
            return c[3]
        require_device(p, "AdamW.step")
        if st is None:
            st = self.state[p] = {}
        for k in ("exp_avg", "exp_avg_sq"):
            if k not in st:
                st[k] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            _check_param(st[k], k)
            if st[k].device != p.device or st[k].numel() != p.numel():
                raise ValueError(f"{k} does not match its parameter")
        out = (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
        self._slots[id(p)] = (st, st["exp_avg"], st["exp_avg_sq"], out)
        return out

    # ---- the launches ---------------------------------------------------------------------------------------------------------------
    def _enqueue(self, scaler, max_norm):
        if self._pending is not None:
            raise RuntimeError("the previous step has not been finished: call scaler.update() after scaler.step(optimizer)")
        self._check_groups()
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError(f"max_norm must be >= 0, got {max_norm}")
        cols, device = [], None
        for g in self.param_groups:
            lr, wd = float(g["lr"]), float(g["weight_decay"])
            decay, has_decay = float(np.float32(1.0 - lr * wd)), int(wd != 0)
            for p in g["params"]:
                grad = p.grad
                if grad is None:
                    continue
                pm, pv, numel = self._moments(p)
                if grad.dtype is not torch.float32 or not grad.is_contiguous() or grad.device != p.device or grad.shape != p.shape:
                    _check_param(grad, "gradient")
                    raise ValueError(f"gradient {tuple(grad.shape)} on {grad.device} for a parameter {tuple(p.shape)} on {p.device}")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise ValueError("parameters on more than one device")
                cols.append((p.data_ptr(), grad.data_ptr(), pm, pv, numel, lr, decay, has_decay))
        rows = np.array(cols, dtype=_ROW) if cols else np.zeros(0, _ROW)
        if device is None:                         # no gradient anywhere: nothing to enqueue, nothing to finish
            return
        lib = _lib.load()
        with torch.cuda.device(device):
            self._lists.sync(rows, device)
            if self._state_dev is None or self._state_dev.device != device:
                b1, b2 = self.param_groups[0]["betas"]
                self._state_dev = _struct_tensor(_lib.OptimState(_beta_pow(b1, self._step), _beta_pow(b2, self._step), self._step, 0.0, 0, 0),
                                                 device)
            L, n = self._lists, self._lists.n_chunks
            b1, b2 = self.param_groups[0]["betas"]
            sc = None if scaler is None else scaler._device_state(device).data_ptr()
            mn = -1.0 if max_norm is None else float(max_norm)
            check(lib.bg_mt_grad_stats(L.table, L.chunks, n, L.partials.data_ptr(), stream()), "bg_mt_grad_stats")
            check(lib.bg_mt_adamw_step(L.table, L.chunks, n, L.partials.data_ptr(), self._state_dev.data_ptr(), sc, mn, float(b1), float(b2),
                                       float(self.param_groups[0]["eps"]), stream()), "bg_mt_adamw_step")
        self._pending = (device, n, mn)
        for o in self.owners:                      # skipped or not: the host does not know
            if hasattr(o, "invalidate"):
                o.invalidate()

    def _finish(self, scaler):
        device, n, mn = self._pending
        self._pending = None
        b1, b2 = self.param_groups[0]["betas"]
        with torch.cuda.device(device):
            sc = None if scaler is None else scaler._device_state(device).data_ptr()
            gf, bf, gi = (2.0, 0.5, 1) if scaler is None else (scaler._growth_factor, scaler._backoff_factor, scaler._growth_interval)
            check(_lib.load().bg_optim_finish(self._lists.partials.data_ptr(), n, self._state_dev.data_ptr(), sc, mn, float(b1), float(b2),
                                              float(gf), float(bf), int(gi), stream()), "bg_optim_finish")

    @torch.no_grad()
    def step(self, closure=None):
        """One update without a scaler and without clipping (a non-finite gradient still skips it).  Does not synchronise."""
        if closure is not None:
            raise ValueError("closures are not provided")
        self._enqueue(None, None)
        if self._pending is not None:
            self._finish(None)

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.requires_grad_(False)
                    p.grad.zero_()

    # ---- what the device knows (each of these synchronises) -----------------------------------------------------------------------------
    def _read_state(self):
        if self._pending is not None:
            raise RuntimeError("a step is enqueued but not finished: call scaler.update() first")
        if self._state_dev is None:
            return _lib.OptimState(0.0, 0.0, self._step, 0.0, 0, 0)
        st = _lib.OptimState.from_buffer_copy(self._state_dev.cpu().numpy().tobytes())
        self._step = st.step
        return st

    def last_step_info(self):
        """{"step", "total_norm", "found_inf"} of the last finished step, read back from the device."""
        st = self._read_state()
        return {"step": st.step, "total_norm": st.total_norm, "found_inf": bool(st.found_inf)}

    def state_dict(self):
        """torch.optim.AdamW's layout: state[index] = {"step", "exp_avg", "exp_avg_sq"} for every parameter that has been stepped,
        param_groups with torch's keys and parameter indices.  A torch.optim.AdamW loads it and continues."""
        step = self._read_state().step
        index, groups = {}, []
        for g in self.param_groups:
            out = {k: v for k, v in g.items() if k != "params"}
            out["params"] = []
            for p in g["params"]:
                index[id(p)] = len(index)
                out["params"].append(index[id(p)])
            groups.append(out)
        state = {index[id(p)]: {"step": torch.tensor(float(step)), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
                 for p, st in self.state.items() if "exp_avg" in st and "exp_avg_sq" in st}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        """From ours or from a torch.optim.AdamW over the same parameters.  The moments are copied to the parameters' devices as fp32;
        the per-parameter steps must agree (one counter here)."""
        if self._pending is not None:
            raise RuntimeError("a step is enqueued but not finished: call scaler.update() first")
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")
        steps, new_state = set(), {}
        ordered = [p for g in self.param_groups for p in g["params"]]
        ids = [i for g in groups for i in g["params"]]
        for i, p in zip(ids, ordered):
            st = state_dict["state"].get(i)
            if st is None:
                continue
            steps.add(int(float(st["step"])))
            new_state[p] = {}
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f"{k} of parameter {i} has shape {tuple(st[k].shape)}, the parameter {tuple(p.shape)}")
                new_state[p][k] = st[k].detach().to(device=p.device, dtype=torch.float32).contiguous().clone()
        if len(steps) > 1:
            raise ValueError(f"per-parameter steps differ ({sorted(steps)}); this optimiser keeps one counter")
        for mine, theirs in zip(self.param_groups, groups):
            for k, v in theirs.items():
                if k != "params":
                    mine[k] = tuple(v) if k == "betas" else v
        self._check_groups()
        self.state, self._step, self._state_dev = new_state, (steps.pop() if steps else 0), None


class GradScaler:
    """torch.amp.GradScaler with the scale and the growth tracker on the device.  `step(optimizer, max_norm)` takes a brepgen_amd AdamW;
    `unscale_` is not provided (the reference never calls it: it clips the scaled gradients and unscales afterwards)."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        if not enabled:
            raise ValueError("a disabled scaler is not provided: call optimizer.step() instead")
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) >= 1 and init_scale > 0.0):
            raise ValueError("need growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1, init_scale > 0")
        self._scale, self._growth_tracker = float(np.float32(init_scale)), 0          # as last known on the host
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._dev, self._stepped = None, None

    def _device_state(self, device):
        if self._dev is None or self._dev.device != device:
            self._dev = _struct_tensor(_lib.ScalerState(self._scale, self._growth_tracker), device)
        return self._dev

    def scale(self, loss):
        """loss * scale as a device multiplication (the scale is read on the device)."""
        _lib.load()
        require_device(loss, "GradScaler.scale")
        return loss * self._device_state(loss.device)[:4].view(torch.float32)[0]

    @torch.no_grad()
    def step(self, optimizer, max_norm=None):
        """Clip to max_norm (None: no clipping), unscale, inf check and AdamW: launches 1 and 2.  Does not synchronise and returns None."""
        if not isinstance(optimizer, AdamW):
            raise TypeError("GradScaler.step takes a brepgen_amd.optim.AdamW")
        if self._stepped is not None:
            raise RuntimeError("step() has already been called since the last update()")
        optimizer._enqueue(self, max_norm)
        if optimizer._pending is not None:
            self._stepped = optimizer

    @torch.no_grad()
    def update(self):
        """Launch 3: the scale backs off after a skipped step and grows after growth_interval good ones."""
        if self._stepped is None:
            raise RuntimeError("no step was recorded prior to update()")
        opt, self._stepped = self._stepped, None
        opt._finish(self)

    def _read(self):
        if self._dev is not None:
            st = _lib.ScalerState.from_buffer_copy(self._dev.cpu().numpy().tobytes())
            self._scale, self._growth_tracker = st.scale, st.growth_tracker
        return self._scale, self._growth_tracker

    def get_scale(self):
        """The current scale; the one call of a training loop that synchronises."""
        return self._read()[0]

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def is_enabled(self):
        return True

    def state_dict(self):
        scale, tracker = self._read()
        return {"scale": scale, "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict):
        if self._stepped is not None:
            raise RuntimeError("a step is enqueued but not finished: call update() first")
        self._scale, self._growth_tracker = float(np.float32(state_dict["scale"])), int(state_dict["_growth_tracker"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._dev = None


_clip_lists = {}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """nn.utils.clip_grad_norm_ for the 2-norm: every .grad times min(1, max_norm / (total_norm + 1e-6)) in place (times 1.0 where
    nothing is clipped, as torch does).  Returns total_norm as a 0-d device tensor (with no gradient anywhere: a zero on the first
    parameter's device); does not synchronise."""
    if float(norm_type) != 2.0:
        raise ValueError("only the 2-norm is provided")
    if not float(max_norm) >= 0.0:
        raise ValueError(f"max_norm must be >= 0, got {max_norm}")
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:                                  # nothing to clip: 0 on the parameters' device (no parameters at all: on the host)
        return torch.zeros((), dtype=torch.float32, device=params[0].device if params else "cpu")
    lib = _lib.load()
    rows = np.zeros(len(grads), _ROW)
    for i, g in enumerate(grads):
        _check_param(g, "gradient")
        require_device(g, "clip_grad_norm_")
        if g.device != grads[0].device:
            raise ValueError("gradients on more than one device")
        rows[i]["g"], rows[i]["numel"] = g.data_ptr(), g.numel()
    device = grads[0].device
    L = _clip_lists.setdefault(device, _Lists())
    with torch.cuda.device(device):
        L.sync(rows, device)
        norm = torch.empty((), dtype=torch.float32, device=device)
        check(lib.bg_mt_grad_stats(L.table, L.chunks, L.n_chunks, L.partials.data_ptr(), stream()), "bg_mt_grad_stats")
        check(lib.bg_mt_scale_grads(L.table, L.chunks, L.n_chunks, L.partials.data_ptr(), float(max_norm), norm.data_ptr(), stream()),
              "bg_mt_scale_grads")
    return norm
