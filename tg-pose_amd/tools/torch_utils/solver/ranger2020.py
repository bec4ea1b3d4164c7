"""Drop-in for ``tools/torch_utils/solver/ranger2020.py`` (:43-246): the Ranger optimizer (RAdam + Lookahead + gradient
centralisation) with its step as ONE HIP launch over every parameter that has a gradient (tgp_ranger_step, csrc/ranger.hip).

Same constructor, defaults, checks, param-group keys (``step_counter``, ``N_sma_threshhold``, ...) and per-parameter state keys
(``step`` int, ``exp_avg``, ``exp_avg_sq``, ``slow_buffer``) as the reference, so ``optimizer_state_dict`` of a reference checkpoint
loads and continues.  The host does what the reference computes in Python doubles -- the step counters, N_sma and step_size (with
the reference's ten-slot ``radam_buffer``), the adaptive and the lookahead decisions -- per tensor, since a parameter whose ``.grad``
is None is skipped and gets no state, so counters can differ.  The device does every elementwise op in fp32 in the reference's order.

The state lives in one flat device buffer (3 rows: exp_avg, exp_avg_sq, slow_buffer; every tensor 16-byte aligned); ``self.state``
holds views of it.  It is flattened again after ``load_state_dict`` and when a parameter receives its first gradient.  The launch's
descriptor table is rebuilt only when a parameter's or gradient's data_ptr, or the set of None gradients, changes; each step rewrites
its per-tensor scalars and copies it to the device from pinned memory without waiting (``step()`` never synchronises).

fp32 dense contiguous CUDA tensors only, and ``gc_loc=True`` (the trainer's setting): anything else raises.
"""
import ctypes
import math

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from .... import _lib, ops


# a numpy view of the descriptor table, field for field at the offsets of the ctypes struct (its per-step columns are written at once)
_NP = {ctypes.c_void_p: "<u8", ctypes.c_int64: "<i8", ctypes.c_int: "<i4", ctypes.c_float: "<f4"}
_TABLE_DTYPE = np.dtype({"names": [n for n, _ in _lib.RangerTensor._fields_],
                         "formats": [_NP[t] for _, t in _lib.RangerTensor._fields_],
                         "offsets": [getattr(_lib.RangerTensor, n).offset for n, _ in _lib.RangerTensor._fields_],
                         "itemsize": ctypes.sizeof(_lib.RangerTensor)})


def centralized_gradient(x, use_gc=True, gc_conv_only=False):
    """ranger2020.py:31-40 as a torch op (gradient centralisation in place); Ranger.step does this inside its launch"""
    if use_gc and x.dim() > (3 if gc_conv_only else 1):
        x.add_(-x.mean(dim=tuple(range(1, x.dim())), keepdim=True))
    return x


class Ranger(Optimizer):
    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0,
                 use_gc=True, gc_conv_only=False, gc_loc=True):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        if not gc_loc:
            raise NotImplementedError("Ranger: gc_loc=False (centralising the update instead of the gradient) is not implemented "
                                      "in the fused step; the trainer uses gc_loc=True")
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.radam_buffer = [[None, None, None] for _ in range(10)]
        self.gc_loc = gc_loc
        self.use_gc = use_gc
        self.gc_conv_only = gc_conv_only
        self._reset_cache()

    def _reset_cache(self):
        self._key = None            # (param ptr, grad ptr, ...) of the table below
        self._flat = None           # (3, total) fp32: exp_avg, exp_avg_sq, slow_buffer of every parameter with state
        self._flat_params = ()      # the parameters whose state is in _flat, in order
        self._all = None            # [(p, group index, has a descriptor)] of the parameters with gradients, in order
        self._gidx = None           # group index of every descriptor
        self._table = None          # ctypes array of _lib.RangerTensor (host)
        self._tab = None            # structured numpy view of it
        self._table_dev = None      # its device copy
        self._units = 0

    def __setstate__(self, state):
        super().__setstate__(state)
        self._reset_cache()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = int(st["step"].item())
        self._reset_cache()         # the loaded tensors are flattened again at the next step

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_key"):
            self._key = None

    # ------------------------------------------------------------------------------------------------------------- state
    def _flatten(self):
        """every parameter that has state gets its three tensors as views of one new flat buffer (existing values copied in)"""
        params = [p for group in self.param_groups for p in group["params"] if len(self.state.get(p, {})) > 0]
        same = len(params) == len(self._flat_params) and all(a is b for a, b in zip(params, self._flat_params))
        if same and all(self._is_view(p) for p in params):
            return
        dev = params[0].device
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        flat = torch.zeros(3, max(total, 4), device=dev, dtype=torch.float32)
        for p, o in zip(params, offs):
            st = self.state[p]
            for row, name in enumerate(("exp_avg", "exp_avg_sq", "slow_buffer")):
                view = flat[row, o:o + p.numel()].view_as(p)
                src = st.get(name)
                if src is not None:
                    if tuple(src.shape) != tuple(p.shape):
                        raise ValueError("Ranger: state %r of shape %s for a parameter of shape %s" % (name, tuple(src.shape), tuple(p.shape)))
                    view.copy_(src, non_blocking=True)
                st[name] = view
        self._flat, self._flat_params = flat, tuple(params)

    def _is_view(self, p):
        st = self.state[p]
        f = self._flat
        return f is not None and all(st[n].untyped_storage().data_ptr() == f.untyped_storage().data_ptr()
                                     for n in ("exp_avg", "exp_avg_sq", "slow_buffer"))

    def _check(self, p):
        g = p.grad
        if g.is_sparse:
            raise RuntimeError("Ranger optimizer does not support sparse gradients")
        if p.dtype != torch.float32 or g.dtype != torch.float32:
            raise TypeError("Ranger: fp32 parameters and gradients only (got %s / %s)" % (p.dtype, g.dtype))
        if not p.is_cuda or g.device != p.device:
            raise ValueError("Ranger: parameters and gradients must be on one GPU (the step is a HIP kernel)")
        if not (p.is_contiguous() and g.is_contiguous()):
            raise ValueError("Ranger: contiguous parameters and gradients only")

    def _rebuild(self, entries):
        dev = entries[0][0].device
        for p, gi in entries:
            self._check(p)
            if p.device != dev:
                raise ValueError("Ranger: all parameters with gradients must be on one device")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
                st["slow_buffer"] = p.detach().clone()
        self._flatten()
        live = [(p, gi) for p, gi in entries if p.numel() > 0]       # empty tensors get state and a step count, no descriptor
        self._all = [(p, gi, p.numel() > 0) for p, gi in entries]
        self._gidx = np.array([gi for _, gi in live], dtype=np.int64)
        self._table = table = (_lib.RangerTensor * len(live))()
        for d, (p, gi) in zip(table, live):
            st = self.state[p]
            d.p, d.g = p.data_ptr(), p.grad.data_ptr()
            d.m, d.v, d.slow = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["slow_buffer"].data_ptr()
            d.numel = p.numel()
            if self.use_gc and p.dim() > (3 if self.gc_conv_only else 1):
                d.row_len, d.flags = p.numel() // p.shape[0], _lib.RANGER_GC
        self._units = ops.ranger_plan(table)
        self._tab = np.frombuffer(table, dtype=_TABLE_DTYPE) if live else None
        self._gc = self._tab["flags"].copy() if live else None
        self._table_dev = torch.empty(ctypes.sizeof(table), dtype=torch.uint8, device=dev) if live else None

    # -------------------------------------------------------------------------------------------------------------- step
    def _radam(self, step, beta1, beta2):
        """ranger2020.py:194-216: (N_sma, step_size) through the reference's ten-slot buffer, in Python doubles"""
        buffered = self.radam_buffer[int(step % 10)]
        if step == buffered[0]:
            return buffered[1], buffered[2]
        buffered[0] = step
        beta2_t = beta2 ** step
        N_sma_max = 2 / (1 - beta2) - 1
        N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
        buffered[1] = N_sma
        if N_sma > self.N_sma_threshhold:
            step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (
                1 - beta1 ** step)
        else:
            step_size = 1.0 / (1 - beta1 ** step)
        buffered[2] = step_size
        return N_sma, step_size

    @torch.no_grad()
    def step(self, closure=None):
        """one Ranger step over every parameter whose .grad is not None (the reference ignores closure, and so does this)"""
        entries, key = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Ranger optimizer does not support sparse gradients")
                entries.append((p, gi))
                key.append(p.data_ptr())
                key.append(g.data_ptr())
        if not entries:
            return None
        key = tuple(key)
        if key != self._key:
            self._rebuild(entries)
            self._key = key
        groups, thr = self.param_groups, self.N_sma_threshhold
        lr, flags = [], []
        for p, gi, live in self._all:
            group = groups[gi]
            st = self.state[p]
            st["step"] += 1
            step = st["step"]
            beta1, beta2 = group["betas"]
            N_sma, step_size = self._radam(step, beta1, beta2)
            if live:
                lr.append(-step_size * group["lr"])
                flags.append((_lib.RANGER_ADAPTIVE if N_sma > thr else 0) | (_lib.RANGER_LOOKAHEAD if step % group["k"] == 0 else 0))
        if not lr:
            return None
        # the reference's scalars, each rounded once to fp32 as torch rounds a Python float operand of an fp32 op
        tab = self._tab
        tab["neg_step_lr"] = lr
        tab["flags"] = self._gc | np.array(flags, dtype=np.int32)
        per_group = np.array([(g["betas"][0], 1 - g["betas"][0], g["betas"][1], 1 - g["betas"][1], g["eps"], g["weight_decay"])
                              for g in groups], dtype=np.float64)[self._gidx]
        for j, name in enumerate(("beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "eps", "weight_decay")):
            tab[name] = per_group[:, j]
        tab["alpha"] = self.alpha
        host = torch.from_numpy(np.frombuffer(self._table, dtype=np.uint8)).pin_memory()
        self._table_dev.copy_(host, non_blocking=True)
        ops.ranger_step(self._table_dev, len(tab), self._units)
        return None

