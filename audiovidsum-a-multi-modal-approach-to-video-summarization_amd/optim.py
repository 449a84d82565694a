"""FusedAdamW: the optimiser step of the scorer's training loop on libavsum_optim.so (include/avsum_optim.h).

One step is at most 1 + 2 * ceil(n / 32) launches on the current stream for n parameters with a gradient: the optional
norm pass (one fp64 partial per 4096-element chunk of every gradient), one single-workgroup kernel that turns the
partials into the clip coefficient and the skip decision and advances the step count ON THE DEVICE, and the apply
pass, which reads p, g, m, v and writes p, m, v once (28 bytes per element).  The pointer table of a launch travels in
its kernel arguments, so the new addresses ``.grad`` gets after every ``zero_grad()`` cost no upload.

What differs from torch.optim.AdamW, by design:
  * ``max_grad_norm`` clips by the global norm INSIDE the update: the update uses g * clip, ``.grad`` itself is left
    unscaled (torch.nn.utils.clip_grad_norm_ rescales it in place).
  * ``skip_nonfinite`` drops a step whose squared gradient norm is inf or NaN: nothing is stored, the step count does
    not advance.  The version counters that key the runners' weight caches live on the host, so in this mode - and in
    this mode only - step() reads the 4-byte decision back through pinned memory and waits for it: one host wait per
    step, what torch's GradScaler.step pays for the same decision.  Without ``skip_nonfinite`` step() never waits for
    the device, clipping included.
  * one step count for all parameters, kept on the device; ``state_dict()`` reports it as every parameter's ``step``.

``adamw_reference`` restates the arithmetic on torch-CPU in float64 or float32; the tests compare against it.
"""
import ctypes
import math
from ctypes import c_void_p

import torch

from . import _optim_abi

MAX_TENSORS = _optim_abi.MAX_TENSORS
CHUNK = _optim_abi.CHUNK
TABLE_COLS = _optim_abi.TABLE_COLS
_STATE_DOUBLES = _optim_abi.SHARED["AVSO_STATE_DOUBLES"]
_COEF_OFFSET = _optim_abi.SHARED["AVSO_COEF_OFFSET"]
_PARTIALS_OFFSET = _optim_abi.SHARED["AVSO_PARTIALS_OFFSET"]
_COEF_SKIP = _optim_abi.SHARED["AVSO_COEF_SKIP"]
_S_APPLIED, _S_SKIPPED, _S_NORM2, _S_CLIP = (_optim_abi.SHARED["AVSO_STATE_" + n]
                                             for n in ("APPLIED", "SKIPPED", "NORM2", "CLIP"))
_ARENA_ALIGN = 4      # elements: every parameter's slice of an arena starts on a 16-byte boundary


def chunks_of(numel):
    return -(-int(numel) // CHUNK)


def launch_plan(numels):
    """Host only.  The launches that cover tensors of ``numels`` elements (all > 0), in order: a list of
    {"rows": (lo, hi), "first_chunk": c, "starts": [...]} with hi - lo <= AVSO_MAX_TENSORS, ``starts`` the exclusive
    scan of the rows' chunk counts (hi - lo + 1 entries - what the entry point puts beside the table in the kernel
    argument) and ``first_chunk`` the launch's first index into the step's partials; and the total chunk count."""
    plan, total = [], 0
    for lo in range(0, len(numels), MAX_TENSORS):
        hi = min(lo + MAX_TENSORS, len(numels))
        starts = [0]
        for n in numels[lo:hi]:
            if n <= 0:
                raise ValueError(f"launch_plan: a tensor of {n} elements (empty tensors are dropped before planning)")
            starts.append(starts[-1] + chunks_of(n))
        plan.append({"rows": (lo, hi), "first_chunk": total, "starts": starts})
        total += starts[-1]
    return plan, total


def pack_table(rows, out=None):
    """Host only.  ``rows`` = (param, grad, exp_avg, exp_avg_sq, numel) address tuples of ONE launch -> the int64
    [len(rows), AVSO_TABLE_COLS] host table the entry points take, as a ctypes array (``out`` is reused when given)."""
    if not 1 <= len(rows) <= MAX_TENSORS:
        raise ValueError(f"pack_table: {len(rows)} rows, must be 1..{MAX_TENSORS}")
    table = out if out is not None else (ctypes.c_int64 * (MAX_TENSORS * TABLE_COLS))()
    flat = [value for row in rows for value in row]
    if len(flat) != TABLE_COLS * len(rows):
        raise ValueError(f"pack_table: every row has {TABLE_COLS} entries")
    table[:len(flat)] = flat
    return table


def _check_hyper(lr, betas, eps, weight_decay, max_grad_norm):
    if not 0.0 <= lr:
        raise ValueError(f"FusedAdamW: lr = {lr!r}")
    if not 0.0 <= eps:
        raise ValueError(f"FusedAdamW: eps = {eps!r}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"FusedAdamW: weight_decay = {weight_decay!r}")
    if len(betas) != 2 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"FusedAdamW: betas = {betas!r}, each must lie in [0, 1)")
    if max_grad_norm is not None and not (0.0 < max_grad_norm < math.inf):
        raise ValueError(f"FusedAdamW: max_grad_norm = {max_grad_norm!r}, must be None or a positive number")


def make_workspace(numels, device):
    """The zeroed workspace (float64 tensor: state | coefficients | partials) for steps over tensors of ``numels``
    elements - the most that one step will ever pass."""
    _, total = launch_plan([n for n in numels if n > 0])
    nbytes = _optim_abi.lib().avso_workspace_bytes(total)
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=device)


def read_stats(workspace):
    """One download: {"applied", "skipped"} step counts, and of the last step "norm" (the gradients' global norm, None
    when no norm pass ran), "norm2" (its square, as the device summed it) and "clip"."""
    s = workspace[:_STATE_DOUBLES].cpu().tolist()
    have = s[_S_NORM2] >= 0.0 or s[_S_NORM2] != s[_S_NORM2]
    return {"applied": int(s[_S_APPLIED]), "skipped": int(s[_S_SKIPPED]), "norm2": s[_S_NORM2] if have else None,
            "norm": math.sqrt(s[_S_NORM2]) if have else None, "clip": s[_S_CLIP]}


def multi_tensor_adamw(params, grads, exp_avgs, exp_avg_sqs, workspace, lr, betas, eps, weight_decay,
                       max_grad_norm=None, skip_nonfinite=False, table=None):
    """One AdamW step over four aligned lists of dense fp32 tensors on ONE device, in place, on the current stream:
    at most 1 + 2 * ceil(n / AVSO_MAX_TENSORS) launches, no host synchronisation, no allocation on the device, no torch
    kernel.  Tensors without elements are dropped; longer lists are sliced into launches of AVSO_MAX_TENSORS.
    ``workspace``: make_workspace() of these tensors (or more); it carries the step count from call to call."""
    _check_hyper(lr, betas, eps, weight_decay, max_grad_norm)
    if not len(params) == len(grads) == len(exp_avgs) == len(exp_avg_sqs):
        raise ValueError("multi_tensor_adamw: the four lists differ in length")
    device = workspace.device
    if device.type != "cuda" or workspace.dtype != torch.float64 or not workspace.is_contiguous():
        raise ValueError("multi_tensor_adamw: the workspace is a contiguous float64 tensor on the GPU")
    rows = []
    for i, group in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        for name, x in zip(("parameter", "gradient", "exp_avg", "exp_avg_sq"), group):
            if x.dtype != torch.float32 or x.is_sparse or not x.is_contiguous():
                raise ValueError(f"multi_tensor_adamw: the {name} of tensor {i} ({x.dtype}, {x.layout}) "
                                 "is not a dense contiguous fp32 tensor")
            if x.device != device or x.shape != group[0].shape:
                raise ValueError(f"multi_tensor_adamw: the {name} of tensor {i} is {tuple(x.shape)} on {x.device}, "
                                 f"expected {tuple(group[0].shape)} on {device}")
        if group[0].numel():
            rows.append(tuple(x.data_ptr() for x in group) + (group[0].numel(),))
    if rows:
        _launch_step(rows, workspace, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, table)


def _launch_step(rows, workspace, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, table):
    """The launches of one step over validated table rows (at least one, none empty)."""
    plan, total = launch_plan([r[4] for r in rows])
    device = workspace.device
    capacity = workspace.numel() - _PARTIALS_OFFSET // 8
    beta1, beta2 = betas
    with_norm = max_grad_norm is not None or bool(skip_nonfinite)
    lib = _optim_abi.lib()
    base = workspace.data_ptr()
    d_state, d_coef, d_partials = c_void_p(base), c_void_p(base + _COEF_OFFSET), c_void_p(base + _PARTIALS_OFFSET)
    with torch.cuda.device(device):
        stream = c_void_p(torch.cuda.current_stream().cuda_stream)
        if with_norm:
            for launch in plan:
                lo, hi = launch["rows"]
                _optim_abi.check(lib.avso_grad_sumsq_f32(pack_table(rows[lo:hi], table), hi - lo, d_partials,
                                                         launch["first_chunk"], capacity, stream),
                                 "avso_grad_sumsq_f32")
        _optim_abi.check(lib.avso_adamw_prepare(d_partials, total if with_norm else 0, float(lr), float(beta1),
                                                float(beta2), float(weight_decay),
                                                float(max_grad_norm) if max_grad_norm is not None else 0.0,
                                                int(bool(skip_nonfinite)), d_state, d_coef, stream),
                         "avso_adamw_prepare")
        for launch in plan:
            lo, hi = launch["rows"]
            _optim_abi.check(lib.avso_adamw_apply_f32(pack_table(rows[lo:hi], table), hi - lo, d_coef, float(beta1),
                                                      float(beta2), float(eps), stream), "avso_adamw_apply_f32")


class FusedAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay) over fp32 CUDA parameters of one device, one parameter group.

    ``exp_avg`` and ``exp_avg_sq`` live in one arena each, allocated and zeroed here.  ``step()`` takes no closure,
    leaves out parameters whose ``.grad`` is None, allocates nothing after the first call, runs no torch kernel, reads
    ``lr`` (and the other hyper-parameters) from the group on every call, and bumps the version counter of every
    parameter it updated (models/av_model.py and cnn.py key their kernel-layout weight caches on it).
    ``state_dict()`` / ``load_state_dict()`` speak torch.optim.AdamW's format, so a checkpoint moves between the two.

    In data-parallel training call dist.allreduce_gradients before step(): every rank then holds the same gradients,
    computes the same norm and takes the same skip decision, so the replicas stay identical."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 skip_nonfinite=False, amsgrad=False, maximize=False):
        _check_hyper(lr, betas, eps, weight_decay, max_grad_norm)
        # torch.optim.AdamW's keys (so that either optimiser loads the other's state_dict) and the two of this class
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=True, max_grad_norm=max_grad_norm, skip_nonfinite=bool(skip_nonfinite))
        super().__init__(params, defaults)
        self._check_group()
        plist = self.param_groups[0]["params"]
        device = plist[0].device
        for i, p in enumerate(plist):
            if p.dtype != torch.float32:
                raise ValueError(f"FusedAdamW: parameter {i} is {p.dtype}, fp32 only")
            if p.is_sparse or not p.is_contiguous():
                raise ValueError(f"FusedAdamW: parameter {i} is not a dense contiguous tensor")
            if p.device != device:
                raise ValueError(f"FusedAdamW: parameter {i} is on {p.device}, parameter 0 on {device}; one device only")
        if device.type != "cuda":
            raise ValueError(f"FusedAdamW: the parameters are on {device}; the step runs on the GPU only")
        self._device = device
        offsets, total = [], 0
        for p in plist:
            offsets.append(total)
            total += -(-p.numel() // _ARENA_ALIGN) * _ARENA_ALIGN
        self._exp_avg = torch.zeros(max(total, 1), dtype=torch.float32, device=device)
        self._exp_avg_sq = torch.zeros(max(total, 1), dtype=torch.float32, device=device)
        for p, off in zip(plist, offsets):
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": self._exp_avg[off:off + p.numel()].view_as(p),
                             "exp_avg_sq": self._exp_avg_sq[off:off + p.numel()].view_as(p)}
        self._fixed = [(self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(), p.numel())
                       for p in plist]
        self._ws = make_workspace([p.numel() for p in plist], device)
        self._coef = self._ws[_COEF_OFFSET // 8:_PARTIALS_OFFSET // 8].view(torch.float32)
        self._skip_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._skip_event = torch.cuda.Event()
        self._table = (ctypes.c_int64 * (MAX_TENSORS * TABLE_COLS))()

    def _check_group(self):
        if len(self.param_groups) != 1:
            raise ValueError(f"FusedAdamW: {len(self.param_groups)} parameter groups; one group only")
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FusedAdamW: amsgrad and maximize are not supported")
        if g.get("decoupled_weight_decay", True) is not True:
            raise ValueError("FusedAdamW: weight decay is decoupled (AdamW); Adam's coupled decay is not supported")
        g.setdefault("max_grad_norm", self.defaults["max_grad_norm"])
        g.setdefault("skip_nonfinite", self.defaults["skip_nonfinite"])
        _check_hyper(g["lr"], g["betas"], g["eps"], g["weight_decay"], g["max_grad_norm"])

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        """One AdamW step; returns None.  Without ``skip_nonfinite`` no host synchronisation."""
        if closure is not None:
            raise ValueError("FusedAdamW.step takes no closure")
        self._check_group()
        group = self.param_groups[0]
        # the parameters and their moments were validated at construction: per step only what can change is checked
        params, rows = [], []
        f32, dev = torch.float32, self._device
        for i, p in enumerate(group["params"]):
            g = p.grad
            if g is None:
                continue
            m_ptr, v_ptr, numel = self._fixed[i]
            if (g.dtype is not f32 or g.device != dev or g.shape != p.shape or g.is_sparse or not g.is_contiguous()
                    or p.dtype is not f32 or p.device != dev or p.numel() != numel or not p.is_contiguous()):
                raise ValueError(f"FusedAdamW.step: parameter {i} ({p.dtype}, {tuple(p.shape)}, {p.device}) and its "
                                 f"gradient ({g.dtype}, {tuple(g.shape)}, {g.device}, {g.layout}) must be dense "
                                 f"contiguous fp32 tensors of {numel} elements on {dev}")
            if numel:
                params.append(p)
                rows.append((p.data_ptr(), g.data_ptr(), m_ptr, v_ptr, numel))
        if not rows:
            return None
        skip_nonfinite = bool(group["skip_nonfinite"])
        _launch_step(rows, self._ws, group["lr"], group["betas"], group["eps"], group["weight_decay"],
                     group["max_grad_norm"], skip_nonfinite, self._table)
        if skip_nonfinite:
            # the one host wait of this mode: were the parameters written?  (a 4-byte copy into pinned memory)
            with torch.cuda.device(self._device):
                self._skip_host.copy_(self._coef[_COEF_SKIP:_COEF_SKIP + 1], non_blocking=True)
                self._skip_event.record()
                self._skip_event.synchronize()
            if float(self._skip_host[0]) != 0.0:
                return None
        torch.autograd.graph.increment_version(params)
        return None

    # ------------------------------------------------------------------ state
    def stats(self):
        """One download: see read_stats."""
        return read_stats(self._ws)

    def state_dict(self):
        """torch.optim.AdamW's format: per parameter ``step`` (= steps applied, the same for all), ``exp_avg``,
        ``exp_avg_sq``.  One download."""
        applied = float(self.stats()["applied"])
        for state in self.state.values():
            state["step"] = torch.tensor(applied)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Takes a state_dict of this class or of torch.optim.AdamW.  The moments are copied into the arenas; the
        parameters' ``step`` counts must agree (this optimiser keeps one) and become the device's count.  A parameter
        without an entry starts from zero moments."""
        arenas = {p: (s["exp_avg"], s["exp_avg_sq"]) for p, s in self.state.items()}
        super().load_state_dict(state_dict)
        self._check_group()
        steps = set()
        for p, (m, v) in arenas.items():
            loaded = self.state.get(p, {})
            if "exp_avg" in loaded:
                m.copy_(loaded["exp_avg"])
                v.copy_(loaded["exp_avg_sq"])
                steps.add(float(loaded["step"]))
            else:
                m.zero_()
                v.zero_()
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": m, "exp_avg_sq": v}
        if len(steps) > 1:
            raise ValueError(f"FusedAdamW.load_state_dict: the parameters' step counts differ ({sorted(steps)}); "
                             "this optimiser keeps one count for all")
        self._ws[_S_APPLIED] = steps.pop() if steps else 0.0


def adamw_reference(params, grads_per_step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                    max_grad_norm=None, skip_nonfinite=False, dtype=torch.float64, exp_avg=None, exp_avg_sq=None,
                    applied=0):
    """The arithmetic of libavsum_optim.so restated on torch-CPU, elementwise in ``dtype`` (float64: the yardstick;
    float32: the same operations in the kernels' precision, scalars rounded once from their float64 values).

    ``grads_per_step``: one list per step, aligned with ``params``; None = no gradient, the parameter is left out.
    The squared norm is summed in float64 whatever ``dtype``.  Returns one dict per step: "params", "exp_avg",
    "exp_avg_sq" (lists of ``dtype`` tensors, copies), "applied", "skipped", "norm2" (None without a norm pass),
    "clip", "skip"."""
    beta1, beta2 = betas
    p = [x.detach().cpu().to(dtype).clone() for x in params]
    m = [torch.zeros_like(x) if exp_avg is None else exp_avg[i].detach().cpu().to(dtype).clone()
         for i, x in enumerate(p)]
    v = [torch.zeros_like(x) if exp_avg_sq is None else exp_avg_sq[i].detach().cpu().to(dtype).clone()
         for i, x in enumerate(p)]

    def scalar(x):
        return torch.tensor(x, dtype=torch.float64).to(dtype)

    history, skipped = [], 0
    for grads in grads_per_step:
        present = [i for i, g in enumerate(grads) if g is not None and g.numel() > 0]
        norm2, clip, skip = None, 1.0, False
        if (max_grad_norm is not None or skip_nonfinite) and present:
            norm2 = math.fsum(float(grads[i].detach().cpu().double().pow(2).sum()) for i in present)
            skip = bool(skip_nonfinite) and not math.isfinite(norm2)
            if max_grad_norm is not None:
                c = max_grad_norm / (math.sqrt(norm2) + 1e-6)
                clip = c if c < 1.0 else 1.0
        if present and skip:
            skipped += 1
        elif present:
            t = applied + 1
            applied = t
            decay, step_size = scalar(1.0 - lr * weight_decay), scalar(lr / (1.0 - beta1 ** t))
            bc2s, clip_t = scalar(math.sqrt(1.0 - beta2 ** t)), scalar(clip)
            omb1, b2, omb2, eps_t = scalar(1.0 - beta1), scalar(beta2), scalar(1.0 - beta2), scalar(eps)
            clip = float(clip_t)
            for i in present:
                g = grads[i].detach().cpu().to(dtype) * clip_t
                p[i] = p[i] * decay
                m[i] = m[i] + (g - m[i]) * omb1
                v[i] = v[i] * b2 + g * g * omb2
                p[i] = p[i] - step_size * m[i] / (v[i].sqrt() / bc2s + eps_t)
        history.append({"params": [x.clone() for x in p], "exp_avg": [x.clone() for x in m],
                        "exp_avg_sq": [x.clone() for x in v], "applied": applied, "skipped": skipped,
                        "norm2": norm2, "clip": clip, "skip": skip})
    return history
