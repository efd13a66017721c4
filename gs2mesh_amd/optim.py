"""The training update as native code: ``adam_step`` / ``densify_stats`` (thin wrappers of ``gs2m_adam_step`` /
``gs2m_densify_stats``, gs2mesh_amd/csrc/optim_kernels.h) and ``FusedAdam``, a ``torch.optim.Optimizer`` whose ``step`` is
one kernel launch over all its tensors (chunks of 8) with no host wait.  include/gs2mesh_amd.h states the arithmetic and
how far it is from ``torch.optim.Adam``.  Importing this module needs neither a GPU nor the built library."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream_of


def _count(x):
    return int(np.prod(x.shape, dtype=np.int64))


def _check_f32(x, name, what="adam_step"):
    f32 = torch.float32 if isinstance(x, torch.Tensor) else np.float32
    if x.dtype != f32:
        raise TypeError(f"{what}: {name} must be float32, got {x.dtype}")


def adam_step(segments, row_visible=None, lib=None, stream=None):
    """``gs2m_adam_step`` on contiguous f32 device tensors (numpy arrays on the emulator back-end of the tests), in place.

    ``segments``: 1 to 8 dicts ``{"param", "grad", "exp_avg", "exp_avg_sq", "step", "lr", "betas", "eps"}``; ``step`` is the
    number of the step being taken (1 for the first), an int.  ``row_visible``: None, or an int32 buffer of one entry per
    leading row of every tensor: only rows whose entry is > 0 are updated, the others are neither read nor written.
    Asynchronous on the stream; nothing is read on the host."""
    lib = lib or _lib.get()
    n = len(segments)
    table = (_lib.AdamSegment * max(n, 1))()
    rows = 0
    if row_visible is not None:
        i32 = torch.int32 if isinstance(row_visible, torch.Tensor) else np.int32
        if row_visible.dtype != i32:
            raise TypeError(f"adam_step: row_visible must be int32, got {row_visible.dtype}")
        rows = _count(row_visible)
    first = None
    for s, seg in zip(table, segments):
        p, g, m, v = seg["param"], seg["grad"], seg["exp_avg"], seg["exp_avg_sq"]
        first = p if first is None else first
        for x, name in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            _check_f32(x, name)
            if tuple(x.shape) != tuple(p.shape):
                raise ValueError(f"adam_step: {name} has shape {tuple(x.shape)}, param {tuple(p.shape)}")
        s.param, s.grad = _ptr(p, None, "param"), _ptr(g, None, "grad")
        s.exp_avg, s.exp_avg_sq = _ptr(m, None, "exp_avg"), _ptr(v, None, "exp_avg_sq")
        s.count = _count(p)
        s.step = int(seg["step"])
        if row_visible is not None and (p.ndim == 0 or int(p.shape[0]) != rows):
            raise ValueError(f"adam_step: row_visible has {rows} rows, a tensor of shape {tuple(p.shape)} does not")
        s.row_width = s.count // rows if row_visible is not None and rows > 0 else 1
        s.lr, s.eps = float(seg["lr"]), float(seg["eps"])
        s.beta1, s.beta2 = float(seg["betas"][0]), float(seg["betas"][1])
    _lib.check(lib.gs2m_adam_step(n, table, _ptr(row_visible, None, "row_visible") if rows else None, rows,
                                  _stream_of(first, stream)), lib)


def densify_stats(radii, viewspace_grad, max_radii2D, grad_accum, denom, lib=None, stream=None):
    """``gs2m_densify_stats``, in place: where ``radii`` [P] int32 is > 0, ``max_radii2D`` [P] takes the larger radius,
    ``grad_accum`` [P] (or [P,1]) gains the norm of columns 0 and 1 of ``viewspace_grad`` [P,3], and ``denom`` gains 1."""
    lib = lib or _lib.get()
    P = _count(radii)
    i32 = torch.int32 if isinstance(radii, torch.Tensor) else np.int32
    if radii.dtype != i32:
        raise TypeError(f"densify_stats: radii must be int32, got {radii.dtype}")
    if tuple(viewspace_grad.shape) != (P, 3):
        raise ValueError(f"densify_stats: viewspace_grad must be [{P}, 3], got {tuple(viewspace_grad.shape)}")
    for x, name in ((viewspace_grad, "viewspace_grad"), (max_radii2D, "max_radii2D"), (grad_accum, "grad_accum"), (denom, "denom")):
        _check_f32(x, name, "densify_stats")
        if name != "viewspace_grad" and _count(x) != P:
            raise ValueError(f"densify_stats: {name} must hold {P} elements, got {tuple(x.shape)}")
    _lib.check(lib.gs2m_densify_stats(P, _ptr(radii, None, "radii"), _ptr(viewspace_grad, None, "viewspace_grad"),
                                      _ptr(max_radii2D, None, "max_radii2D"), _ptr(grad_accum, None, "grad_accum"),
                                      _ptr(denom, None, "denom"), _stream_of(radii, stream)), lib)


class FusedAdam(torch.optim.Optimizer):
    """Adam (no amsgrad, no weight decay) whose ``step`` is ``gs2m_adam_step``: one launch for all parameters, chunks of 8.

    Constructor arguments and param-group keys are those ``GaussianModel.training_setup`` uses (``params``, ``lr``,
    ``name``, ``betas``, ``eps``); the per-parameter state has ``torch.optim.Adam``'s keys (``step``, ``exp_avg``,
    ``exp_avg_sq``), so a ``state_dict`` of either optimiser loads into the other and code that edits the state of one
    edits the state of this one.  ``step`` is kept as torch keeps it, a float32 scalar tensor on the host; an int loaded
    from elsewhere is accepted.  The groups also carry ``weight_decay = 0`` and ``amsgrad = False``, the two keys
    ``torch.optim.Adam`` needs to find in a loaded ``state_dict``; any other value of them is refused by ``step``.
    Parameters must be contiguous float32 tensors on the HIP device."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, lib=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        self._lib = lib
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0.0, amsgrad=False))

    @torch.no_grad()
    def step(self, closure=None, *, visible=None):
        """One step of every parameter that has a gradient (a ``.grad`` of None is skipped, as torch does).  ``visible``:
        None, or the int32 row mask of the sparse variant (the rasteriser's ``radii``): only rows whose entry is > 0 are
        updated.  It is valid only when every parameter has ``len(visible)`` leading entries.  Reads no device data."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        segments = []
        for group in self.param_groups:
            if group.get("weight_decay", 0.0) != 0.0 or group.get("amsgrad", False) or group.get("maximize", False):
                raise RuntimeError("FusedAdam implements plain Adam: weight_decay, amsgrad and maximize must be off")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam does not take sparse gradients; pass the row mask to step(visible=...)")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                t = state["step"]
                if isinstance(t, torch.Tensor):
                    if t.is_cuda:
                        raise RuntimeError("FusedAdam: state['step'] lives on the device (a capturable or fused torch "
                                           "optimiser wrote it); move it to the host before loading")
                    t += 1
                    t = int(t)
                else:
                    t = state["step"] = int(t) + 1
                for k in ("exp_avg", "exp_avg_sq"):
                    if not state[k].is_contiguous():
                        state[k] = state[k].contiguous()
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                segments.append(dict(param=p.data, grad=grad, exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"],
                                     step=t, lr=group["lr"], betas=group["betas"], eps=group["eps"]))
        for k in range(0, len(segments), _lib.ADAM_MAX_SEGMENTS):
            adam_step(segments[k:k + _lib.ADAM_MAX_SEGMENTS], row_visible=visible, lib=self._lib)
        return loss
