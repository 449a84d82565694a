"""Seeded inputs and yardsticks of the fused AdamW tests (test_optim_host.py on the CPU, test_gpu_optim.py on the GPU).

The unit table: element counts COUNTS cycled to 70 tensors (three launches of at most 32 rows), tensor k a view at
element offset k % 4 behind a 16-byte boundary of one buffer per kind (parameter, gradient, exp_avg, exp_avg_sq), so
both the 16-byte and the scalar path and every tail run; SENTINEL elements fill the buffers between the views.

The bound is tests/scorer_f64_inputs.py::compare: err <= 4 * e32 + 8 * eps32 * scale, both errors against
avsum_amd.optim.adamw_reference in float64, e32 the error of torch.optim.AdamW(foreach=False) on the CPU in fp32 on
the same inputs (for a clip case its gradients pre-multiplied by the fp32 clip coefficient), scale = max(1, max|p_ref|)
for parameters and max|ref| for exp_avg and exp_avg_sq.
"""
import math

import numpy as np
import torch

from scorer_f64_inputs import EPS32, compare

COUNTS = (0, 1, 3, 4, 5, 64, 4095, 4096, 4097, 8193)
NUM_TENSORS = 70
SENTINEL = -77.25
LR = 1e-2
STEPS = 3
EPS = 1e-8
# (name, weight_decay, betas, max_grad_norm): the gradients' norm is in the hundreds, so 1.0 clips every step
CASES = (("wd", 0.01, (0.9, 0.999), None), ("nowd", 0.0, (0.8, 0.95), None), ("clip", 0.01, (0.9, 0.999), 1.0))
KINDS = ("params", "exp_avg", "exp_avg_sq")


def wide_grads(shape, gen):
    """randn * 10^U(-6, 1): seven decades of gradient magnitude, so the eps term of the denominator matters for some
    elements and not for others."""
    return torch.randn(shape, generator=gen) * torch.pow(10.0, torch.rand(shape, generator=gen) * 7.0 - 6.0)


class UnitTable:
    """``layout``: (first element, count) of every tensor in each of the buffers; ``params`` / ``grads[s]``: the fp32
    CPU buffers (SENTINEL between the views); moments start from zero inside the views."""

    def __init__(self, seed=2024, counts=COUNTS, num_tensors=NUM_TENSORS, steps=STEPS):
        gen = torch.Generator().manual_seed(seed)
        self.layout, cursor = [], 0
        for k in range(num_tensors):
            n = counts[k % len(counts)]
            cursor = -(-cursor // 4) * 4 + 4 + k % 4        # at least one sentinel in front; offset k % 4 behind 16 bytes
            self.layout.append((cursor, n))
            cursor += n
        self.size = cursor + 5
        self.params = self.fill(lambda n: torch.randn(n, generator=gen))
        self.grads = [self.fill(lambda n: wide_grads((n,), gen)) for _ in range(steps)]
        self.zeros = self.fill(lambda n: torch.zeros(n))

    def fill(self, make):
        buf = torch.full((self.size,), SENTINEL, dtype=torch.float32)
        for lo, n in self.layout:
            buf[lo:lo + n] = make(n)
        return buf

    def views(self, buf):
        return [buf[lo:lo + n] for lo, n in self.layout]

    def sentinels_intact(self, buf):
        mask = torch.ones(self.size, dtype=torch.bool)
        for lo, n in self.layout:
            mask[lo:lo + n] = False
        return bool((buf.cpu()[mask] == SENTINEL).all())


def clip_coefficient(grads, max_grad_norm):
    """The fp64 formula of the clip coefficient over a list of gradients (exact squares, math.fsum), and the exact
    squared norm."""
    norm2 = math.fsum(x for g in grads for x in (g.double() * g.double()).tolist())
    c = max_grad_norm / (math.sqrt(norm2) + 1e-6)
    return (c if c < 1.0 else 1.0), norm2


def torch_adamw_fp32(params, grads_per_step, lr, betas, eps, weight_decay, max_grad_norm=None, state=None):
    """torch.optim.AdamW(foreach=False) on the CPU in fp32: the e32 yardstick.  One dict of lists per step.  For a clip
    case the gradients are pre-multiplied by the fp32 clip coefficient.  ``state``: a state_dict to start from."""
    ps = [torch.nn.Parameter(p.detach().cpu().float().clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    if state is not None:
        opt.load_state_dict(state)
    history = []
    for grads in grads_per_step:
        present = [g for g in grads if g is not None and g.numel()]
        clip = torch.tensor(clip_coefficient(present, max_grad_norm)[0] if max_grad_norm is not None else 1.0,
                            dtype=torch.float64).float()
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.detach().cpu().float() * clip
        opt.step()
        history.append({"params": [p.detach().clone() for p in ps],
                        "exp_avg": [opt.state[p]["exp_avg"].clone() if p in opt.state else torch.zeros_like(p)
                                    for p in ps],
                        "exp_avg_sq": [opt.state[p]["exp_avg_sq"].clone() if p in opt.state else torch.zeros_like(p)
                                       for p in ps]})
    return history


def variant_fp32(params, grads_per_step, lr, betas, eps, weight_decay, mistake=None):
    """AdamW in fp32 on the CPU, written in ANOTHER order than adamw_reference (moments first, bias corrections as
    divisions of the moments, the decay last) - correct for mistake=None - or with one planted mistake:
    "coupled" (decay added to the gradient), "step_off_by_one" (t starts at 2), "no_bias_correction",
    "eps_in_sqrt" (sqrt(v_hat + eps))."""
    beta1, beta2 = betas
    p = [x.detach().cpu().float().clone() for x in params]
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    history = []
    for s, grads in enumerate(grads_per_step):
        t = s + (2 if mistake == "step_off_by_one" else 1)
        bc1 = 1.0 if mistake == "no_bias_correction" else 1.0 - beta1 ** t
        bc2 = 1.0 if mistake == "no_bias_correction" else 1.0 - beta2 ** t
        for i, g in enumerate(grads):
            g = g.float()
            if mistake == "coupled":
                g = g + weight_decay * p[i]
            m[i] = beta1 * m[i] + (1.0 - beta1) * g
            v[i] = beta2 * v[i] + (1.0 - beta2) * (g * g)
            m_hat, v_hat = m[i] / bc1, v[i] / bc2
            denom = (v_hat + eps).sqrt() if mistake == "eps_in_sqrt" else v_hat.sqrt() + eps
            update = lr * (m_hat / denom)
            if mistake != "coupled":
                update = update + (lr * weight_decay) * p[i]
            p[i] = p[i] - update
        history.append({"params": [x.clone() for x in p], "exp_avg": [x.clone() for x in m],
                        "exp_avg_sq": [x.clone() for x in v]})
    return history


def check_step(got, ref64, cpu32, kinds=KINDS):
    """Every tensor of every kind of one step against the bound of scorer_f64_inputs.compare,
    err <= 4 * e32 + 8 * eps32 * scale, with e32 and scale taken over the whole kind (all tensors of the table: a
    tensor of one element has no error statistics of its own).  ``got``, ``ref64``, ``cpu32``: dicts of lists.
    Returns (worst err / bound, [(kind, tensor index, err, e32, bound) of every miss]); a non-finite value is a miss."""
    worst, misses = 0.0, []
    for kind in kinds:
        used = [i for i, r in enumerate(ref64[kind]) if r.numel()]
        top = max((ref64[kind][i].abs().max().item() for i in used), default=0.0)
        scale = max(1.0, top) if kind == "params" else top
        e32 = max((compare(cpu32[kind][i], ref64[kind][i], cpu32[kind][i])[1] for i in used), default=0.0)
        bound = 4.0 * e32 + 8.0 * EPS32 * scale
        for i in used:
            g = got[kind][i].detach().cpu()
            err = (g.double() - ref64[kind][i].double()).abs().max().item()
            if not (bool(torch.isfinite(g).all()) and err <= bound):
                misses.append((kind, i, err, e32, bound))
                err = err if err == err else math.inf
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
    return worst, misses


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))
