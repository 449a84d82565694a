"""Inputs, float64 reference, fp32 restatements, the bound and the planted mistakes of the per-kernel tests of the two
fused attention kernels of csrc/attention.hip (test_mhsa_f64_host.py on the host, test_gpu_mhsa_f64.py on the device).
torch-CPU only: both tests build the same seeded cases from here.

The operation:  ctx[b, q, h*D:(h+1)*D] = softmax_k(Q[b,q,h] . K[b,k,h] / sqrt(D)) . V[b,k,h],  rows b*T + q.

Layout of a case (``buffers``).  Q, K and V each live in a buffer of their own, [b*T, ld] with ld > heads*D, the heads
starting at column ``col0`` (4 floats for the fp32 kernel, 8 slots for the f16x2 one: what the C ABI's alignment rules
allow); every other column holds SENTINEL.  ctx is [b*T + 2, ldo], ldo > heads*D, pre-filled with SENTINEL: a guard row in
front, a guard row behind, the heads from column ``ocol0`` = 4.  ``strided=False`` is the layout of ops.mhsa_flash:
ld = ldo = E, no offsets (the guard rows stay).

Value regimes (``REGIMES``): ``flat`` (q, k = 0.6 N(0,1): scaled scores of standard deviation 0.36, what the module-level
tests draw), ``peaked`` (q = 8 N, k = N: scores reach +-40, one or two keys hold a row), ``ramp_up`` / ``ramp_down``
(k = 0.3 N + c_j u, q = 0.3 N + u with u a unit vector and c_j = 40 sqrt(D) j / (T - 1) rising or falling with the key
index: every key tile raises the running maximum, or none after the first does; the range of a row's scores is about
40 (1 + 0.3 N) whatever T is), ``huge`` (q = 80 N: scores reach +-250, exp without a shift overflows fp32), ``offset_v``
(v = 100 + N), ``tiny_v`` (v = 2^-10 N: the lo halves of V are fp16 denormals; f16x2 only), ``equal_keys`` (every key row
of a (batch, head) identical) and ``twins`` (query rows i, i+16, i+32, i+64, i+128 identical for i < 16, batch entry 2 a
copy of batch entry 0).

References and bounds.  fp32 kernel: float64 on the fp32 inputs; yardstick e32 = softmax(q @ k^T / sqrt(D)) @ v in fp32
on the CPU.  f16x2 kernel: the operands are packed on the CPU (``emu_pack`` of test_gpu_f16x2.py, bit for bit the device's
pack kernel); the reference is float64 on the UNPACKED operands, so that operand rounding is not charged to the kernel;
the yardstick e_h2 is the kernel's arithmetic restated in fp32 with one global row maximum: scores
(kh.qh + kl.qh + kh.ql) * (1/sqrt(D)), p = exp(s - max) split into fp16 hi | lo as avs_f16x2_split8 does,
o = (vh.ph + vl.ph + vh.pl) / sum(p).  Either way the bound is scorer_f64_inputs.compare: 4 * e + 8 * eps32 * scale with
scale = max(1, max|ref|).  ``tiny_v`` takes scale = max|ref| instead: everything the kernel does after loading V is linear
in V and far from the fp32 denormals, so its error shrinks with V; a floor of 8 eps32 * 1 would be a thousand times the
outputs' own rounding there.

``restate(..., online=True)`` is the same arithmetic in the kernels' online form (tiles of 32 keys, running maximum,
``corr = exp(m_run - m_new)`` applied to the accumulator and the running sum); the planted mistakes (MISTAKES) are made in
that form.  NOTICED_BY names, per mistake, the case at which the host test shows it to lie outside the bound."""
import functools
import math
from types import SimpleNamespace

import torch

from scorer_f64_inputs import EPS32, SENTINEL, compare  # noqa: F401  (one definition of the bound, shared)
from test_gpu_f16x2 import emu_pack, emu_unpack  # noqa: F401  (the AVS_F16X2 format restated on the CPU, shared)

KINDS = ("f32", "f16x2")
HEAD_DIMS = (64, 128, 256)
T_LIST = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
T_LONG = 1031                                   # 33 key tiles, the last one partial
SMALL, LARGE = (1, 2), (4, 4)                   # (b, heads): the fp32 kernel's 2-wave and 4-wave instance at every T_LIST
REGIMES = ("flat", "peaked", "ramp_up", "ramp_down", "huge", "offset_v", "tiny_v", "equal_keys", "twins")
RAMP_RANGE = 40.0
KEY_TILE = 32
MISTAKES = ("no_running_max", "drop_corr", "tail_unmasked", "swap_key_slots", "wrong_head_v", "batch_offset_ignored",
            "scale_missing", "p_hi_only", "drop_cross_term")
F16X2_ONLY = ("p_hi_only", "drop_cross_term")
# mistake -> (regime, T, (b, heads)): where it is looked for.  no_running_max only shows where exp overflows; drop_corr
# where the maximum rises from tile to tile; tail_unmasked where the softmax is flat and the phantom keys are many;
# swap_key_slots where neighbouring keys weigh alike (flat), not on a ramp; the precision mistakes where a few keys
# hold the row (the probabilities are then not all near 1/T, and their lo halves matter)
NOTICED_BY = {
    "no_running_max": ("huge", 33, SMALL),
    "drop_corr": ("ramp_up", 65, SMALL),
    "tail_unmasked": ("flat", 15, SMALL),
    "swap_key_slots": ("flat", 65, SMALL),
    "wrong_head_v": ("flat", 33, SMALL),
    "batch_offset_ignored": ("flat", 33, LARGE),
    "scale_missing": ("peaked", 65, SMALL),
    "p_hi_only": ("peaked", 65, SMALL),
    "drop_cross_term": ("peaked", 65, SMALL),
}


def mistakes_of(kind):
    return tuple(m for m in MISTAKES if kind == "f16x2" or m not in F16X2_ONLY)


def f32_waves(b, heads, t):
    """Waves per workgroup of the flash_mhsa_kernel instance that avs_mhsa_flash_f32 launches: the rule of its host code."""
    return 2 if -(-t // 128) * heads * b < 16 else 4


# --------------------------------------------------------------------------- the case list
def specs(kind, d):
    """[(kind, d, t, b, heads, regime, strided)] of the short cases of one (kernel, head dim) family."""
    out = []
    add = lambda t, bh, regime, strided=True: out.append((kind, d, t, bh[0], bh[1], regime, strided))
    for t in T_LIST:
        add(t, SMALL, "flat")
        add(t, LARGE, "flat")
    for t in (17, 33, 65, 129, 257):
        add(t, SMALL, "peaked")
        add(t, LARGE, "peaked")
    for regime in ("ramp_up", "ramp_down"):
        for t in (33, 65, 129, 257):        # ramp_up: the row maximum lies in the partial last tile
            add(t, SMALL, regime)
        for t in (65, 257):
            add(t, LARGE, regime)
    for t in (33, 65):
        add(t, SMALL, "huge")
        add(t, LARGE, "huge")
    for regime in ("offset_v",) + (("tiny_v",) if kind == "f16x2" else ()):
        add(33, SMALL, regime)
        add(129, LARGE, regime)
    add(31, SMALL, "equal_keys")
    add(65, LARGE, "equal_keys")
    add(33, LARGE, "twins")
    add(257, LARGE, "twins")
    add(129, LARGE, "flat", False)          # the contiguous layout of ops.mhsa_flash
    return out


def long_specs(kind, d):
    """One long row per regime whose behaviour changes with the number of key tiles: b = 1, heads = 2, T = 1031."""
    return [(kind, d, T_LONG, 1, 2, regime, True) for regime in ("flat", "peaked", "ramp_up", "ramp_down")]


def label(spec):
    kind, d, t, b, heads, regime, strided = spec
    return f"{kind} D={d} T={t} b={b} heads={heads} {regime}" + ("" if strided else " contiguous")


def _draw(regime, d, t, b, heads, g):
    shape = (b, t, heads, d)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v = 0.6 * rn(*shape), 0.6 * rn(*shape), rn(*shape)
    if regime == "peaked":
        q, k = 8.0 * rn(*shape), rn(*shape)
    elif regime in ("ramp_up", "ramp_down"):
        u = rn(b, 1, heads, d)
        u = u / u.norm(dim=-1, keepdim=True)
        ramp = torch.linspace(0.0, 1.0, t) if t > 1 else torch.zeros(1)
        if regime == "ramp_down":
            ramp = ramp.flip(0)
        c = (RAMP_RANGE * math.sqrt(d)) * ramp
        k = 0.3 * rn(*shape) + c[None, :, None, None] * u
        q = 0.3 * rn(*shape) + u
    elif regime == "huge":
        q, k = 80.0 * rn(*shape), rn(*shape)
    elif regime == "offset_v":
        v = 100.0 + v
    elif regime == "tiny_v":
        v = v * 2.0 ** -10
    elif regime == "equal_keys":
        k = k[:, :1].expand(shape).contiguous()
    return q.contiguous(), k.contiguous(), v.contiguous()


def make_case(spec):
    """The seeded case of a spec: q, k, v fp32 [b, T, heads, D] and the layout numbers."""
    kind, d, t, b, heads, regime, strided = spec
    assert kind in KINDS and regime in REGIMES and d in HEAD_DIMS
    seed = 9000 + 100003 * REGIMES.index(regime) + 7919 * d + 31 * t + 7 * b + heads
    q, k, v = _draw("flat" if regime == "twins" else regime, d, t, b, heads, torch.Generator().manual_seed(seed))
    twin_rows, twin_batches = [], []
    if regime == "twins":
        for i in range(min(16, t)):
            for off in (16, 32, 64, 128):
                if i + off < t:
                    q[:, i + off] = q[:, i]
                    twin_rows.append((i, i + off))
        if b >= 3:
            q[2], k[2], v[2] = q[0], k[0], v[0]
            twin_batches.append((0, 2))
    e = heads * d
    col0 = (4 if kind == "f32" else 8) if strided else 0
    ld = e + 3 * col0
    ocol0 = 4 if strided else 0
    ldo = e + 2 * ocol0
    return SimpleNamespace(spec=spec, kind=kind, d=d, t=t, b=b, heads=heads, regime=regime, strided=strided, e=e, q=q, k=k,
                           v=v, ld=ld, col0=col0, ldo=ldo, ocol0=ocol0, rows=b * t, nw=f32_waves(b, heads, t),
                           twin_rows=twin_rows, twin_batches=twin_batches, label=label(spec))


# --------------------------------------------------------------------------- operands and buffers
def _bhtd(x):
    return x.permute(0, 2, 1, 3).contiguous()          # [b, T, heads, D] -> [b, heads, T, D]


def packed(case):
    """(qp, kp, vp): the AVS_F16X2 images of q, k, v as [b*T, E] float32-typed tensors (runs of 8 slots: hi | lo)."""
    return tuple(emu_pack(x.reshape(case.rows, case.e)) for x in (case.q, case.k, case.v))


def _halves(p, case):
    """(hi, lo) of a packed [b*T, E] image as fp32 [b, heads, T, D]."""
    runs = p.contiguous().view(torch.float16).reshape(-1, 2, 8).float()
    shape = (case.b, case.t, case.heads, case.d)
    return _bhtd(runs[:, 0].reshape(shape)), _bhtd(runs[:, 1].reshape(shape))


def buffers(case):
    """(qbuf, kbuf, vbuf, ctx) as the kernel under test is handed them (see the module docstring), on the CPU."""
    src = packed(case) if case.kind == "f16x2" else tuple(x.reshape(case.rows, case.e) for x in (case.q, case.k, case.v))
    bufs = []
    for x in src:
        buf = torch.full((case.rows, case.ld), SENTINEL)
        buf.view(torch.int32)[:, case.col0:case.col0 + case.e] = x.contiguous().view(torch.int32)    # bits, not values
        bufs.append(buf)
    return (*bufs, torch.full((case.rows + 2, case.ldo), SENTINEL))


def reference(case):
    """float64 [b*T, E]: the operation on the values the kernel is handed (fp32 inputs, or the unpacked f16x2 operands)."""
    if case.kind == "f16x2":
        q, k, v = (sum(h.double() for h in _halves(p, case)) for p in packed(case))
    else:
        q, k, v = (_bhtd(x).double() for x in (case.q, case.k, case.v))
    return attention_core(q, k, v).permute(0, 2, 1, 3).reshape(case.rows, case.e)


def attention_core(q, k, v):
    """softmax(q @ k^T / sqrt(D)) @ v on [b, heads, T, D] tensors, in their dtype."""
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    return torch.softmax(s, dim=-1) @ v


# --------------------------------------------------------------------------- the fp32 restatements
def _split(p):
    """fp32 -> (hi, lo) as fp32 values of fp16 numbers: avs_f16x2_split8."""
    pc = p.clamp(-65504.0, 65504.0)
    hi = pc.half().float()
    return hi, (pc - hi).half().float()


def restate(case, online=False, mistake=None):
    """The kernel's arithmetic in fp32 on the CPU, [b*T, E].  online=False: one global row maximum (the yardstick of the
    bound); online=True: tiles of 32 keys with a running maximum, the accumulator and the running sum rescaled by
    corr = exp(m_run - m_new) - the form in which ``mistake`` (one of MISTAKES) is planted."""
    assert mistake is None or (mistake in mistakes_of(case.kind) and online)
    h2 = case.kind == "f16x2"
    if h2:
        (qh, ql), (kh, kl), (vh, vl) = (_halves(p, case) for p in packed(case))
        ops = [qh, ql, kh, kl, vh, vl]
    else:
        ops = [_bhtd(x) for x in (case.q, case.k, case.v)]
    nq = 2 if h2 else 1                                  # tensors per operand
    if mistake == "batch_offset_ignored":
        ops = [x[:1].expand_as(x) for x in ops]
    if mistake == "wrong_head_v":
        ops[2 * nq:] = [x[:, :1].expand_as(x) for x in ops[2 * nq:]]
    sqrt_d = torch.tensor(math.sqrt(case.d), dtype=torch.float32)
    inv_sqrt_d = 1.0 / sqrt_d

    def scores(kt):                                      # kt: the key operand(s), [b, heads, keys, D]
        if h2:
            s = ops[0] @ kt[0].transpose(-1, -2)
            if mistake != "drop_cross_term":
                s = s + ops[0] @ kt[1].transpose(-1, -2)
            s = s + ops[1] @ kt[0].transpose(-1, -2)
            return s if mistake == "scale_missing" else s * inv_sqrt_d
        s = ops[0] @ kt[0].transpose(-1, -2)
        return s if mistake == "scale_missing" else s / sqrt_d

    def weighted(p, vt):                                 # p [b, heads, T, keys], vt: the value operand(s)
        if not h2:
            return p @ vt[0]
        ph, pl = _split(p)
        o = ph @ vt[0]
        if mistake != "drop_cross_term":
            o = o + ph @ vt[1]
        return o if mistake == "p_hi_only" else o + pl @ vt[0]

    kops, vops = ops[nq:2 * nq], ops[2 * nq:]
    if not online:
        s = scores(kops)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = weighted(p, vops) / p.sum(-1, keepdim=True)
        return o.permute(0, 2, 1, 3).reshape(case.rows, case.e)

    t, pad = case.t, -case.t % KEY_TILE
    zpad = lambda x: torch.cat([x, x.new_zeros(*x.shape[:2], pad, x.shape[3])], 2) if pad else x
    kops, vops = [zpad(x) for x in kops], [zpad(x) for x in vops]
    m_run = torch.full((case.b, case.heads, t, 1), -math.inf)
    l_run = torch.zeros(case.b, case.heads, t, 1)
    acc = torch.zeros(case.b, case.heads, t, case.d)
    for k0 in range(0, t, KEY_TILE):
        kt, vt = [x[:, :, k0:k0 + KEY_TILE] for x in kops], [x[:, :, k0:k0 + KEY_TILE] for x in vops]
        if mistake == "swap_key_slots":
            perm = list(range(KEY_TILE))
            perm[1], perm[4] = 4, 1
            vt = [x[:, :, perm] for x in vt]
        s = scores(kt)
        if mistake != "tail_unmasked":
            s = s.masked_fill(torch.arange(k0, k0 + KEY_TILE) >= t, -math.inf)
        m_new = torch.zeros_like(m_run) if mistake == "no_running_max" else torch.maximum(m_run, s.max(-1, keepdim=True).values)
        corr = torch.exp(m_run - m_new) if mistake != "no_running_max" else torch.ones_like(m_run)
        p = torch.exp(s - m_new)
        l_run = l_run * corr + p.sum(-1, keepdim=True)
        acc = (acc if mistake == "drop_corr" else acc * corr) + weighted(p, vt)
        m_run = m_new
    return (acc / l_run).permute(0, 2, 1, 3).reshape(case.rows, case.e)


def scale_of(case, ref):
    """The ``scale`` of scorer_f64_inputs.compare for a case: max(1, max|ref|), but max|ref| alone for tiny_v (see the
    module docstring)."""
    return ref.abs().max().item() if case.regime == "tiny_v" else max(1.0, ref.abs().max().item())


def check(case, got, ref, yard):
    """(ok, err, e, bound) of ``got`` [b*T, E] for a case with its reference and yardstick."""
    return compare(got, ref, yard, scale_of(case, ref))


@functools.lru_cache(maxsize=None)
def bundle(spec):
    """(case, float64 reference, fp32 yardstick), computed once per process and shared by the tests; none of them is
    modified by a test."""
    case = make_case(spec)
    return case, reference(case), restate(case)
