"""Inputs, float64 references, fp32 / bf16 restatements, planted mistakes and the bound of the per-kernel tests of the bf16
convolution + BatchNorm kernels of the throughput path: conv1x1_bn_kernel (avs_conv1x1_bn_bf16, avs_conv1x1_bn_in_bf16,
avs_conv1x1_affine_bf16) and bn_gram_affine_kernel (avs_bn_gram_affine_bf16) of csrc/convbn.hip, the bf16 instances of
avs_conv2d_nhwc_bnstats / avs_conv2d_nhwc_bnlocal of csrc/igemm.hip and the fused stem avs_stem_conv_bn_pool_bf16 of
csrc/stem.hip.  test_convbn_f64_host.py uses it on the host, test_gpu_convbn_f64.py on the device.  torch-CPU only: both
build the same seeded cases from here.

Operands are drawn in fp32 and rounded to bf16 on the CPU; the float64 reference works on exactly those rounded values
(exact products, biased variance, scale = gamma / sqrt(var + eps), shift = beta - mean * scale,
relu(acc * scale + shift + residual')), so operand rounding is not charged to a kernel.

The restatement (cpu32) follows the kernels' order of operations in fp32 and bf16:
  * a transformed input is a = bf16(relu(x * in_scale + in_shift)), the product and the sum rounded separately (the
    library is built without contraction; only an explicit fmaf is fused);
  * the statistics come from the fp32 accumulators BEFORE any rounding, as E[y^2] - mean^2 clamped at 0;
  * the output is t = bf16(fma(acc, scale, shift));
  * with a residual a SECOND rounding follows: bf16(t + r), or bf16(t + (r * rs + rh)) with a residual affine, three
    fp32 roundings;
  * ReLU comes last (on the rounded value: the same number as before the rounding).
The sums of the two-pass kernel and of avs_conv2d_nhwc_bnstats are added in the lanes' order (sums_two_pass,
sums_row_tiles: 32 same-signed values in a row lose more than a pairwise sum does where mean >> spread); the matrix cores'
order inside a dot product, and the sums of the tile-local form and of the Gram kernel, are not restated.

The bound is scorer_f64_inputs.compare unchanged, 4 * e32 + 8 * EPS32 * scale, applied per (group, output channel):
``compare_groups`` takes err, e32 and scale over that group's rows of that one channel, so a channel whose gamma is small
is held to its own magnitude; nothing is left out.  The moments check (``moments`` / ``compare_moments``) holds, for the
forms that return no (scale, shift), two numbers per (group, channel) of a case without residual and ReLU: the mean over
the group's rows of got - ref (a wrong mean) and of (got - ref) * z, z the standardised reference (a wrong scale: the
plain mean of the error cannot see one, it is beta - beta), each divided by the channel's magnitude in that group.  The
bf16 output rounding averages out over a group, so these see statistics mistakes of 1/R size.  Each pair is held to its
OWN restatement moment, 4 * e32 + 8 * EPS32 * scale, with a floor in the scale term (``moments_floor``: half a bf16 step
of the pair's magnitude over sqrt(R)): a pair's own mean rounding error passes close to 0 by chance (it is a sum of R
signed roundings), and one output that rounds the other way on the device - a 1e-7 difference before the rounding is
enough - would then fail a correct kernel.  The floor is below the planted statistics mistakes at every group size of the
cases (unbiased: 1 / (2 R) of the spread; a row left out or too many: 1 / R of it).

Returned (scale, shift) [groups, n] - the Gram kernel, bnstats, the stem - are compared directly, ``compare`` on the whole
tensor as test_gpu_visual_f64.py does for avs_bn_batch_stats (the stem per group: its 64 channels are alike): where mean
>> spread the fp32 error of E[y^2] - mean^2 is one rounding of a number 1600 times the variance, in the kernel and in the
restatement alike but not the same one (the matrix cores' order inside a dot product moves it), so e32 has to be the
largest of many such samples, not one channel's.  The ordinary channels of a mean40 case are held more loosely for it; the
normal regime of the same shape holds them tightly, and the host file shows that the comparison rejects the unbiased
variance and a missing row in every case, mean40 and const included (AFFINE_MISTAKES).

The stem's restatement: the image through the table bf16((v / denom - mean) / std), statistics from per-tile sums (16 x 16
convolution outputs) added in frame and tile order, the raw map rounded to bf16 and pooled 3x3/2 - the maximum where
gamma >= 0, the minimum elsewhere, the padding never winning - then bf16(act(sel * scale + shift)).

``conv_restatement(case, mistake)`` / ``local_restatement`` / ``stem_restatement`` plant one deliberate error (CONV_MISTAKES,
STEM_MISTAKES); the NOTICED_BY tables name, per mistake, the case at which the host test shows it to lie outside the bound."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from scorer_f64_inputs import EPS32, SENTINEL, compare  # noqa: F401  (one definition of the bound, shared)

BN_EPS = 1e-5
MAX_K = 512                     # AVS_CONVBN_MAX_K (the input affine's LDS table)
REGIMES = ("normal", "mean40", "const")
FORMS = ("two_pass", "affine", "affine_ra")
GAMMA_SMALL = 2.0 ** -10        # channel 4: a small gamma, held to its own magnitude
CONST_CH, MEAN40_CH = 3, (5, 6)
MEAN40_CH_2D = tuple(range(5, 21))   # conv2d cases: 16 channels, so that the largest fp32 error of E[y^2] - mean^2 over a
#                                      case's (group, channel) pairs is a stable yardstick (two channels' is a lottery)
ONE_COL, CONST_COL, DEAD_COL = 0, 1, 2      # input columns: the constant 1 (mean40), the constant of "const", rectified to 0

CONV_MISTAKES = ("unbiased", "drop_last_row", "first_row_of_next_group", "no_eps", "stats_of_rounded_output",
                 "relu_before_residual", "res_affine_of_next_group", "gamma_next_channel", "in_affine_of_group_0",
                 "k_tail_dropped")


def bf(x):
    """The fp32 values bf16 stores for x (round to nearest even)."""
    return x.float().bfloat16().float()


def eps32(eps=BN_EPS):
    return torch.tensor(eps, dtype=torch.float32)


def _fma(a, b, c):
    """fmaf: the product of two fp32 is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _seed(*key):
    s = 17
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
        s = (s * 131 + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def randomize_bn(n, g):
    """gamma with both signs, an exact 0 (channel 1) and a small value (channel 4); a non-trivial beta, exactly
    representable in bf16 in the channel the "const" regime makes constant."""
    gamma = torch.randn(n, generator=g)
    gamma = torch.where(gamma.abs() < 0.25, gamma.sign() * 0.25 + gamma, gamma)
    gamma[0], gamma[1], gamma[2], gamma[4] = gamma[0].abs() + 0.5, 0.0, -gamma[2].abs() - 0.5, GAMMA_SMALL
    beta = torch.randn(n, generator=g)
    beta[CONST_CH] = 0.75
    return gamma, beta


# --------------------------------------------------------------------------- the bound, per (group, channel)
def _per_group(t, groups, rpg):
    """[groups * rpg, n] -> [groups, rpg, n]"""
    return t.reshape(groups, rpg, t.shape[-1])


def compare_groups(got, ref, cpu32, groups, rpg):
    """(ok, worst) of ``compare`` applied to every (group, channel) on its own: err, e32 and scale = max(1, max|ref|) over
    that group's rows of that channel.  worst = (err, e32, bound, group, channel) of the pair whose err / bound is
    largest, its figures taken from ``compare`` itself."""
    g3, r3, c3 = (_per_group(t.double(), groups, rpg) for t in (got, ref, cpu32))
    err = (g3 - r3).abs().amax(1)
    e32 = (c3 - r3).abs().amax(1)
    bound = 4.0 * e32 + 8.0 * EPS32 * r3.abs().amax(1).clamp_min(1.0)
    finite = torch.isfinite(g3).all(1)
    ok = bool(((err <= bound) & finite).all())
    ratio = torch.where(finite, err / bound, torch.full_like(err, float("inf")))
    gi, ci = divmod(int(ratio.argmax()), ratio.shape[1])
    ok1, e1, e321, b1 = compare(g3[gi, :, ci], r3[gi, :, ci], c3[gi, :, ci])
    assert ok1 or not ok
    return ok, (e1, e321, b1, gi, ci)


def moments(y, ref, groups, rpg):
    """[2, groups, n] float64: per (group, channel) the mean over the group's rows of (y - ref) and of (y - ref) * z, z the
    standardised reference (0 where the reference is constant), both divided by max|ref| of the pair."""
    y3, r3 = _per_group(y.double(), groups, rpg), _per_group(ref.double(), groups, rpg)
    d = y3 - r3
    mu = r3.mean(1, keepdim=True)
    sd = ((r3 - mu) ** 2).mean(1, keepdim=True).sqrt()
    z = torch.where(sd > 0, (r3 - mu) / sd.clamp_min(1e-300), torch.zeros_like(r3))
    mag = r3.abs().amax(1).clamp_min(1e-30)
    return torch.stack([d.mean(1) / mag, (d * z).mean(1) / mag])


def moments_floor(rpg):
    """Half a bf16 step of a pair's magnitude over sqrt(R), as a multiple of that magnitude: 2^-8 / sqrt(R).  A bf16 step
    of the pair's largest output is at most 2^-7 of it; the mean of R independent roundings has a standard deviation of
    step / sqrt(12 R), so this is 1.7 of them - and sqrt(R) / 2 outputs that round the other way on the device than in
    the restatement (each moves the mean by step / R), which a difference of 1e-7 before the rounding is enough for:
    about 1e-4 of the outputs do, 4e-3 where mean >> spread, so 1.5 of 257 rows at the most against the 8 allowed."""
    return 2.0 ** -8 / float(rpg) ** 0.5


def compare_moments(got, ref, cpu32, groups, rpg):
    """(ok, err, e32, bound, (moment, group, channel)): ``compare`` of each moment of each (group, channel) of got against
    the SAME pair's moment of the restatement (the reference's are 0): bound = 4 * e32 + 8 * EPS32 * scale with scale = 1 +
    moments_floor(R) / (8 * EPS32), i.e. 4 * e32 + 8 * EPS32 + the floor.  A pair whose output is constant (gamma == 0: the
    same rounding of beta in every row, which does not average out) has a large e32 of its own and loosens nobody else.
    The figures returned are those of the pair closest to (or furthest beyond) its bound, taken from ``compare``."""
    mg, mc = moments(got, ref, groups, rpg), moments(cpu32, ref, groups, rpg)
    scale = 1.0 + moments_floor(rpg) / (8.0 * EPS32)
    bound = 4.0 * mc.abs() + 8.0 * EPS32 * scale
    finite = torch.isfinite(mg)
    ratio = torch.where(finite, mg.abs() / bound, torch.full_like(mg, float("inf")))
    ok = bool(((mg.abs() <= bound) & finite).all())
    flat = int(ratio.argmax())
    mi, rest = divmod(flat, mg.shape[1] * mg.shape[2])
    gi, ci = divmod(rest, mg.shape[2])
    ok1, err, e32, b1 = compare(mg[mi, gi, ci], torch.zeros((), dtype=torch.float64), mc[mi, gi, ci], scale)
    assert ok1 or not ok
    return ok, err, e32, b1, (mi, gi, ci)


# --------------------------------------------------------------------------- conv1x1_bn_kernel
# (rows_per_group, k, n, groups)
CONV_SHAPES = ((1, 8, 8, 3),            # variance exactly 0: the output is beta
               (33, 40, 72, 9),         # one short tile, the K tail, a partly filled 128-wide slab, a 9-workgroup grid
               (130, 72, 200, 3),       # a second tile of 2 rows, two slabs with 72 live columns in the second
               (161, 128, 256, 5),      # a second tile of 33 rows: live in 33..64
               (257, 64, 64, 2),        # the narrow 64-column instance, a last tile of 1 row
               (196, 512, 136, 2))      # k at AVS_CONVBN_MAX_K for the input affine
CONST_GROUP = 1
PAD_X, PAD_Y, PAD_R, OFF_Y = 8, 16, 8, 8        # lin_stride = k + 8, ldc = n + 16, ldr = n + 8, y from column 8


def conv_options(si, form, ri):
    """(xf, res, relu, padded) of shape number si in ``form`` and regime number ri: seeded combinations, not the full
    product.  xf alternates with si + ri, so that every (shape, form) runs with and without an input affine; the two-pass
    form without residual and ReLU in the regimes "normal" and "mean40" (the moments check needs them bare)."""
    fi = FORMS.index(form)
    xf = (si + ri) % 2 == 0
    if form == "two_pass" and ri < 2:
        res, relu = False, False
    else:
        res = form == "affine_ra" or (si + fi + ri) % 2 == 0
        relu = (si + 2 * fi + ri) % 3 != 0
    padded = (si + fi + ri) % 2 == 1
    return xf, res, relu, padded


def conv_case_keys():
    return [(si, form, regime) for si in range(len(CONV_SHAPES)) for form in FORMS for regime in REGIMES]


def kernel_instance(n, xf, form):
    """(BN, XF, PRE, RA) of the conv1x1_bn_kernel instance the launcher picks: n <= 64 -> 64-column slabs; XF with an input
    affine; PRE with a given output affine; RA with a residual affine."""
    return 64 if n <= 64 else 128, bool(xf), form != "two_pass", form == "affine_ra"


def live_branches(rpg, form):
    """The branches of ``live`` (rows of a wave's 64 that exist: <= 0, 1..32, 33..64) the one-pass form takes at this
    group size, over its tiles of 128 rows and both row-waves."""
    out = set()
    if form == "two_pass":
        return out
    for tm in range(-(-rpg // 128)):
        for wr in (0, 1):
            live = rpg - tm * 128 - wr * 64
            out.add("le0" if live <= 0 else "1_32" if live <= 32 else "33_64")
    return out


def remapped_workgroups(nwg):
    """conv1x1_bn_kernel's map block id -> workgroup (blocks that share an XCD take consecutive workgroups)."""
    q, rr = nwg >> 3, nwg & 7
    return [(x * (q + 1) if x < rr else rr * (q + 1) + (x - rr) * q) + (o >> 3) for o in range(nwg) for x in [o & 7]]


@functools.lru_cache(maxsize=None)
def conv_case(si, form, regime):
    rpg, k, n, groups = CONV_SHAPES[si]
    ri = REGIMES.index(regime)
    xf, has_res, relu, padded = conv_options(si, form, ri)
    rows = groups * rpg
    g = _seed("conv1x1", si, form, regime)
    x = bf(torch.randn(rows, k, generator=g))
    w = bf(torch.randn(n, k, generator=g) / k ** 0.5)
    isc = ish = None
    if xf:      # scales of both signs; column DEAD_COL is rectified to 0 in every row; ONE_COL / CONST_COL come out constant
        isc = (torch.rand(groups, k, generator=g) + 0.5) * torch.where(torch.rand(groups, k, generator=g) < 0.5, -1.0, 1.0)
        ish = torch.randn(groups, k, generator=g) * 0.5
        isc[:, DEAD_COL], ish[:, DEAD_COL] = 0.5, -100.0
        isc[:, ONE_COL], ish[:, ONE_COL] = 0.0, 1.0
    else:
        x[:, ONE_COL] = 1.0
    if regime != "mean40":
        w[:, ONE_COL] = 0.0
    cg = min(CONST_GROUP, groups - 1)
    if regime == "const":       # channel CONST_CH reads column CONST_COL alone, which is constant in group cg
        w[CONST_CH] = 0.0
        w[CONST_CH, CONST_COL] = 0.75
        x[cg * rpg:(cg + 1) * rpg, CONST_COL] = 1.5
        if xf:
            isc[cg, CONST_COL], ish[cg, CONST_COL] = 0.5, 0.25
    a = conv_input(x, isc, ish, groups, rpg)
    if regime == "mean40":      # |mean| / std about 40 in channels MEAN40_CH, through the constant column
        sd = (a.double() @ w.double().t()).std(0)
        for ch in MEAN40_CH:
            w[ch, ONE_COL] = bf(40.0 * sd[ch].float() * (1.0 if ch % 2 else -1.0))
    gamma, beta = randomize_bn(n, g)
    res = bf(torch.randn(rows, n, generator=g)) if has_res else None
    rsc = rsh = None
    if form == "affine_ra":
        rsc = (torch.rand(groups, n, generator=g) + 0.5) * torch.where(torch.rand(groups, n, generator=g) < 0.5, -1.0, 1.0)
        rsh = torch.randn(groups, n, generator=g)
    case = SimpleNamespace(si=si, form=form, regime=regime, rpg=rpg, k=k, n=n, groups=groups, rows=rows, xf=xf, relu=relu,
                           padded=padded, x=x, w=w, isc=isc, ish=ish, a=a, gamma=gamma, beta=beta, res=res, rsc=rsc, rsh=rsh,
                           const_group=cg, pre=None,
                           lin_stride=k + (PAD_X if padded else 0), ldc=n + (PAD_Y if padded else 0),
                           ldr=n + (PAD_R if padded else 0), off_y=OFF_Y if padded else 0,
                           label=f"rpg={rpg} k={k} n={n} G={groups} {form} {regime} xf={int(xf)} res={int(has_res)} "
                                 f"relu={int(relu)} padded={int(padded)}")
    if form != "two_pass":      # the given affine: the float64 BatchNorm's, as the fp32 numbers a caller would hand over
        sc, sh = conv_stats_reference(case)
        case.pre = (sc.float(), sh.float())
    return case


def conv_input(x, isc, ish, groups, rpg, mistake=None):
    """a = x, or bf16(relu(x * in_scale[g] + in_shift[g])) with an input affine (two fp32 roundings)."""
    if isc is None:
        return x
    gi = torch.arange(groups).repeat_interleave(rpg)
    if mistake == "in_affine_of_group_0":
        gi = torch.zeros_like(gi)
    return bf((x * isc[gi] + ish[gi]).clamp_min(0.0))


def conv_stats_reference(case):
    """float64 (scale, shift) [groups, n] of the BatchNorm of the exact products."""
    y = _per_group(case.a.double() @ case.w.double().t(), case.groups, case.rpg)
    mu = y.mean(1)
    var = ((y - mu[:, None]) ** 2).mean(1)
    scale = case.gamma.double() / torch.sqrt(var + eps32().double())
    return scale, case.beta.double() - mu * scale


def conv_reference(case):
    """float64 y [rows, n]: relu(acc * scale + shift + residual'), the affine the BatchNorm's (two-pass) or the given one."""
    acc = case.a.double() @ case.w.double().t()
    sc, sh = conv_stats_reference(case) if case.pre is None else (case.pre[0].double(), case.pre[1].double())
    gi = torch.arange(case.groups).repeat_interleave(case.rpg)
    y = acc * sc[gi] + sh[gi]
    if case.res is not None:
        r = case.res.double()
        if case.rsc is not None:
            r = r * case.rsc.double()[gi] + case.rsh.double()[gi]
        y = y + r
    return y.clamp_min(0.0) if case.relu else y


# rows of a wave's 64 that one lane of each half (lh) holds, in the order it adds them: 32 * mt + (e & 3) + 8 * (e >> 2) + 4 * lh
_LANE_ROWS = torch.tensor([[32 * mt + (e & 3) + 8 * (e >> 2) + 4 * lh for mt in (0, 1) for e in range(16)] for lh in (0, 1)])


def _lane_chain(blk, s1, s2):
    """One wave block blk [..., 64, n] added to the running sums s1, s2 [..., 2, n] of the two lanes that share a column, as
    the kernels do: s1 += v, s2 = fma(v, v, s2), 32 values each in accumulator order."""
    for step in range(32):
        v = blk[..., _LANE_ROWS[:, step], :]
        s1, s2 = s1 + v, _fma(v, v, s2)
    return s1, s2


def sums_two_pass(blk):
    """(s1, s2) [n] of one group's accumulators blk [R, n] in conv1x1_bn_kernel's order: tiles of 128 rows, two row-waves
    of 64; a lane's sums run on over the tiles; then the lane halves, then the row-waves are added.  Rows past the group
    are zeros."""
    r, n = blk.shape
    tiles = -(-r // 128)
    pad = torch.cat([blk, blk.new_zeros(tiles * 128 - r, n)]).view(tiles, 2, 64, n)
    s1, s2 = blk.new_zeros(2, 2, n), blk.new_zeros(2, 2, n)
    for tm in range(tiles):
        s1, s2 = _lane_chain(pad[tm], s1, s2)
    s1, s2 = s1[:, 0] + s1[:, 1], s2[:, 0] + s2[:, 1]
    return s1[0] + s1[1], s2[0] + s2[1]


def sums_row_tiles(acc, r0, r1):
    """(s1, s2) [n] of rows [r0, r1) of acc in avs_conv2d_nhwc_bnstats' order: per wave block of 64 rows (aligned to the
    row tiles) a lane adds its rows of the group, the lane halves are added, and the blocks are added in row order (how
    the blocks are associated into tiles of 128 or 256 rows is not restated).  Rows outside the group add exact zeros."""
    n = acc.shape[1]
    t1, t2 = acc.new_zeros(n), acc.new_zeros(n)
    for b in range(r0 // 64, (r1 - 1) // 64 + 1):
        lo, hi = max(r0, b * 64), min(r1, (b + 1) * 64)
        blk = acc.new_zeros(64, n)
        blk[lo - b * 64:hi - b * 64] = acc[lo:hi]
        s1, s2 = _lane_chain(blk, acc.new_zeros(2, n), acc.new_zeros(2, n))
        t1, t2 = t1 + (s1[0] + s1[1]), t2 + (s2[0] + s2[1])
    return t1, t2


def fold_stats(acc, groups, rpg, gamma, beta, eps=BN_EPS, mistake=None, lanes=False):
    """The kernels' statistics in fp32 from accumulators acc [groups * rpg, n]: sums and sums of squares (lanes: in
    conv1x1_bn_kernel's order, sums_two_pass), mean = s1 / R, var = max(s2 / R - mean^2, 0), scale = gamma / sqrt(var +
    eps), shift = beta - mean * scale."""
    n = acc.shape[1]
    if mistake == "stats_of_rounded_output":
        acc = bf(acc)
    if mistake == "gamma_next_channel":
        gamma, beta = gamma.roll(-1), beta.roll(-1)
    scale, shift = torch.zeros(groups, n), torch.zeros(groups, n)
    one = torch.ones((), dtype=torch.float32)
    for g in range(groups):
        r0, r1 = g * rpg, (g + 1) * rpg
        if mistake == "drop_last_row" and rpg > 1:
            r1 -= 1
        if mistake == "first_row_of_next_group":
            blk = torch.cat([acc[r0:r1], acc[(r1 % acc.shape[0]):(r1 % acc.shape[0]) + 1]])
        else:
            blk = acc[r0:r1]
        cnt = blk.shape[0]
        inv_n = one / float(cnt)
        s1, s2 = sums_two_pass(blk) if lanes else (blk.sum(0), (blk * blk).sum(0))
        mean = s1 * inv_n
        var = (s2 * inv_n - mean * mean).clamp_min(0.0)
        if mistake == "unbiased":
            var = var * (one * float(cnt) / float(max(cnt - 1, 1)))
        scale[g] = gamma / torch.sqrt(var + (0.0 if mistake == "no_eps" else eps32(eps)))
        shift[g] = beta - mean * scale[g]
    return scale, shift


def finish(acc, scale, shift, groups, rpg, res=None, rsc=None, rsh=None, relu=False, mistake=None):
    """The epilogue: t = bf16(fma(acc, scale[g], shift[g])); with a residual bf16(t + r) or bf16(t + (r * rs[g] + rh[g]));
    then ReLU."""
    gi = torch.arange(groups).repeat_interleave(rpg)
    t = bf(_fma(acc, scale[gi], shift[gi]))
    if mistake == "relu_before_residual" and relu:
        t = t.clamp_min(0.0)
    if res is not None:
        r = res
        if rsc is not None:
            gr = (gi + 1) % groups if mistake == "res_affine_of_next_group" else gi
            r = res * rsc[gr] + rsh[gr]
        t = bf(t + r)
    return t.clamp_min(0.0) if relu else t


def conv_restatement(case, mistake=None):
    """conv1x1_bn_kernel in fp32 / bf16 on the CPU: (y [rows, n], (scale, shift) the kernel used)."""
    assert mistake is None or mistake in CONV_MISTAKES
    a = conv_input(case.x, case.isc, case.ish, case.groups, case.rpg, mistake)
    w = case.w
    if mistake == "k_tail_dropped":
        kk = case.k // 32 * 32
        a, w = a[:, :kk], w[:, :kk]
    acc = a @ w.t() if a.shape[1] else torch.zeros(case.rows, case.n)
    if case.pre is None:
        sc, sh = fold_stats(acc, case.groups, case.rpg, case.gamma, case.beta, mistake=mistake, lanes=True)
    else:
        sc, sh = case.pre
    return finish(acc, sc, sh, case.groups, case.rpg, case.res, case.rsc, case.rsh, case.relu, mistake), (sc, sh)


@functools.lru_cache(maxsize=None)
def conv_bundle(si, form, regime):
    """(case, float64 reference, restatement), computed once per process; no test modifies them."""
    case = conv_case(si, form, regime)
    return case, conv_reference(case), conv_restatement(case)[0]


def has_moments(case):
    return case.form == "two_pass" and case.res is None and not case.relu


# --------------------------------------------------------------------------- bn_gram_affine_kernel
GRAM_K, GRAM_N, GRAM_RPG, GRAM_GROUPS = (64, 128), (32, 96, 160), (1, 63, 64, 65, 130), (1, 3)
GRAM_REGIMES = ("normal", "mean40")
GRAM_STORES = ("off", "separate", "inplace")


def gram_case_keys():
    """(k, n, rpg, groups, regime, xf, store): every k, n, rows_per_group, group count, regime, the input affine off and
    on and the three d_a_out modes, in seeded combinations (each value of each axis with each k)."""
    keys = []
    for ki, k in enumerate(GRAM_K):
        for i, rpg in enumerate(GRAM_RPG):
            for j, regime in enumerate(GRAM_REGIMES):
                n = GRAM_N[(i + j + ki) % 3]
                groups = GRAM_GROUPS[(i + j) % 2]
                xf = (i + j + ki) % 2 == 0
                store = GRAM_STORES[(i + ki) % 3] if xf else "off"
                keys.append((k, n, rpg, groups, regime, xf, store))
        keys.append((k, 160, 65, 3, "normal", True, "separate"))
        keys.append((k, 32, 130, 1, "mean40", True, "inplace"))
        keys.append((k, 96, 64, 3, "normal", False, "off"))
    return keys


@functools.lru_cache(maxsize=None)
def gram_case(k, n, rpg, groups, regime, xf, store):
    rows = groups * rpg
    g = _seed("gram", k, n, rpg, groups, regime, xf, store)
    x = torch.randn(rows, k, generator=g)
    isc = ish = None
    if xf:
        isc = (torch.rand(groups, k, generator=g) + 0.5) * torch.where(torch.rand(groups, k, generator=g) < 0.5, -1.0, 1.0)
        ish = torch.randn(groups, k, generator=g) * 0.5
        isc[:, DEAD_COL], ish[:, DEAD_COL] = 0.5, -100.0
        if regime == "mean40":      # input channels 8..15: mean^2 / variance about 1600 after the transform
            isc[:, 8:16], ish[:, 8:16] = isc[:, 8:16].abs(), 40.0 * isc[:, 8:16].abs()
    elif regime == "mean40":
        x[:, 8:16] += 40.0
    x = bf(x)
    w = bf(torch.randn(n, k, generator=g) / k ** 0.5)
    gamma, beta = randomize_bn(n, g)
    a = conv_input(x, isc, ish, groups, rpg)
    return SimpleNamespace(k=k, n=n, rpg=rpg, groups=groups, rows=rows, regime=regime, xf=xf, store=store, x=x, w=w, isc=isc,
                           ish=ish, a=a, gamma=gamma, beta=beta, lin_stride=k + 8, lda=k + 8,
                           label=f"k={k} n={n} rpg={rpg} G={groups} {regime} xf={int(xf)} a_out={store}")


def gram_restatement(case, mistake=None):
    """bn_gram_affine_kernel in fp32 / bf16: channel sums and a^T a in fp32, C = a^T a / R - m m^T split into bf16 hi + lo,
    T = W . C_hi + W . C_lo, var_y[n] = sum_l T[n, l] W[n, l] clamped at 0, mean_y = W . m, then the folded affine."""
    assert mistake is None or mistake in AFFINE_MISTAKES
    scale, shift = torch.zeros(case.groups, case.n), torch.zeros(case.groups, case.n)
    rows = case.rpg - 1 if mistake == "drop_last_row" else case.rpg
    inv_r = torch.ones((), dtype=torch.float32) / float(rows)
    for g in range(case.groups):
        a = case.a[g * case.rpg:g * case.rpg + rows]
        m = a.sum(0) * inv_r
        c = (a.t() @ a) * inv_r - m[:, None] * m[None, :]
        hi = bf(c)
        lo = bf(c - hi)
        t = case.w @ hi + case.w @ lo
        var = (t * case.w).sum(1).clamp_min(0.0)
        if mistake == "unbiased":
            var = var * (float(rows) / float(rows - 1))
        scale[g] = case.gamma / torch.sqrt(var + eps32())
        shift[g] = case.beta - (case.w @ m) * scale[g]
    return scale, shift


@functools.lru_cache(maxsize=None)
def gram_bundle(*key):
    case = gram_case(*key)
    return case, conv_stats_reference(case), gram_restatement(case)


# --------------------------------------------------------------------------- conv2d + statistics / tile-local BatchNorm
# (frames, hw, cin, cout, kernel, stride, frames per group): bnlocal groups of 49, 64, 100 and 196 rows (tiles of 5, 4, 2
# and 1 groups, a last tile with fewer); bnstats groups of 64 rows and more that straddle the row tiles, the last shorter
LOCAL_SHAPES = ((9, 7, 72, 64, 1, 1, 1),       # 49 rows: tiles of 5 and of 4 groups
                (6, 8, 64, 128, 3, 1, 1),      # 64 rows: a full tile of 4 groups, then 2
                (3, 10, 72, 64, 1, 1, 1),      # 100 rows: 2 groups, then 1
                (2, 14, 32, 128, 3, 1, 1),     # 196 rows: one group per tile
                (5, 14, 64, 64, 3, 2, 1),      # 3x3 / stride 2 to 7x7
                (4, 14, 72, 64, 1, 2, 1))      # 1x1 / stride 2 to 7x7: one tile, 4 of its 5 groups
STATS_SHAPES = ((5, 10, 64, 64, 1, 1, 2), (3, 14, 32, 128, 3, 1, 1), (7, 8, 72, 136, 1, 1, 3), (5, 14, 64, 64, 3, 2, 2),
                (5, 8, 64, 64, 1, 1, 1))       # groups of 200, 196, 192, 98 and 64 rows; last groups of 100, 196, 64, 49, 64


def conv2d_geometry(shape):
    frames, hw, cin, cout, k, s, fpg = shape
    pad = k // 2
    ho = (hw + 2 * pad - k) // s + 1
    return SimpleNamespace(frames=frames, hw=hw, cin=cin, cout=cout, k=k, s=s, pad=pad, ho=ho, rpg=fpg * ho * ho,
                           rows=frames * ho * ho, geom=(frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout),
                           xs=(hw * hw * cin, hw * cin, cin))


def stats_groups(rows, rpg):
    """Row offsets of the groups of avs_conv2d_nhwc_bnstats: groups of rpg rows, the last one shorter."""
    return list(range(0, rows, rpg)) + [rows]


@functools.lru_cache(maxsize=None)
def conv2d_case(kind, shape, regime, with_res=False, relu=False):
    """x [frames, hw, hw, cin], w [cout, k, k, cin] (bf16 values); accumulators in float64 and fp32."""
    ge = conv2d_geometry(shape)
    g = _seed("conv2d", kind, shape, regime, with_res, relu)
    x = bf(torch.randn(ge.frames, ge.hw, ge.hw, ge.cin, generator=g))
    w4 = bf(torch.randn(ge.cout, ge.cin, ge.k, ge.k, generator=g) / (ge.cin * ge.k * ge.k) ** 0.5)
    x[..., ONE_COL] = 1.0
    centre = ge.k // 2
    if regime != "mean40":
        w4[:, ONE_COL] = 0.0
    if regime == "const":       # channel CONST_CH reads the centre tap of column CONST_COL alone, constant in frame 1
        w4[CONST_CH] = 0.0
        w4[CONST_CH, CONST_COL, centre, centre] = 0.75
        x[1, :, :, CONST_COL] = 1.5
    conv = lambda xx, ww: F.conv2d(xx.permute(0, 3, 1, 2), ww, stride=ge.s, padding=ge.pad).permute(0, 2, 3, 1).reshape(-1, ge.cout)
    if regime == "mean40":
        sd = conv(x.double(), w4.double()).std(0)
        for ch in MEAN40_CH_2D:    # through the centre tap of the constant column: the borders see it too
            w4[ch, ONE_COL] = 0.0
            w4[ch, ONE_COL, centre, centre] = bf(40.0 * sd[ch].float() * (1.0 if ch % 2 else -1.0))
    gamma, beta = randomize_bn(ge.cout, g)
    res = bf(torch.randn(ge.rows, ge.cout, generator=g)) if with_res else None
    acc64, acc32 = conv(x.double(), w4.double()), conv(x, w4)
    wt = w4.permute(0, 2, 3, 1).reshape(ge.cout, -1).contiguous()
    return SimpleNamespace(kind=kind, shape=shape, regime=regime, ge=ge, x=x, wt=wt, gamma=gamma, beta=beta, res=res, relu=relu,
                           acc64=acc64, acc32=acc32, label=f"{kind} {shape} {regime} res={int(with_res)} relu={int(relu)}")


AFFINE_MISTAKES = ("unbiased", "drop_last_row")


def ragged_stats(acc, offsets, gamma, beta, dtype, mistake=None):
    """(scale, shift) [G, n] in ``dtype`` over row groups given by offsets (float64: the reference, centred; float32: the
    kernels' E[y^2] - mean^2 clamped at 0 on sums in avs_conv2d_nhwc_bnstats' order, sums_row_tiles)."""
    n = acc.shape[1]
    scale, shift = torch.zeros(len(offsets) - 1, n, dtype=dtype), torch.zeros(len(offsets) - 1, n, dtype=dtype)
    assert mistake is None or (mistake in AFFINE_MISTAKES and dtype == torch.float32)
    for g, (r0, r1) in enumerate(zip(offsets[:-1], offsets[1:])):
        if mistake == "drop_last_row":
            r1 -= 1
        blk = acc[r0:r1].to(dtype)
        if dtype == torch.float64:
            mu = blk.mean(0)
            var = ((blk - mu) ** 2).mean(0)
        else:
            inv_n = torch.ones((), dtype=dtype) / float(r1 - r0)
            s1, s2 = sums_row_tiles(acc, r0, r1)
            mu = s1 * inv_n
            var = (s2 * inv_n - mu * mu).clamp_min(0.0)
            if mistake == "unbiased":
                var = var * (float(r1 - r0) / float(r1 - r0 - 1))
        scale[g] = gamma.to(dtype) / torch.sqrt(var + eps32().to(dtype))
        shift[g] = beta.to(dtype) - mu * scale[g]
    return scale, shift


def local_reference(case):
    ge = case.ge
    groups = ge.rows // ge.rpg
    sc, sh = ragged_stats(case.acc64, stats_groups(ge.rows, ge.rpg), case.gamma, case.beta, torch.float64)
    gi = torch.arange(groups).repeat_interleave(ge.rpg)
    y = case.acc64 * sc[gi] + sh[gi]
    if case.res is not None:
        y = y + case.res.double()
    return y.clamp_min(0.0) if case.relu else y


def local_restatement(case, mistake=None):
    ge = case.ge
    groups = ge.rows // ge.rpg
    sc, sh = fold_stats(case.acc32, groups, ge.rpg, case.gamma, case.beta, mistake=mistake)
    return finish(case.acc32, sc, sh, groups, ge.rpg, case.res, None, None, case.relu, mistake)


# --------------------------------------------------------------------------- the fused stem
STEM_CASES = ((2, 1), (3, 3), (4, 2))       # (frames, frames per group)
STEM_MISTAKES = ("min_max_pool_swapped", "pad_pool_with_zero")
STEM_MEAN, STEM_STD, STEM_DENOM = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 255.0
CONST_FRAME, CONST_COLOUR = 1, (200, 30, 117)


def normalize_lut(denom=STEM_DENOM, mean=STEM_MEAN, std=STEM_STD):
    """[3, 256] fp32: bf16((v / denom - mean_c) / std_c) for every byte value, each operation rounded to fp32
    (frames_normalize_kernel's expression; the stem reads the same table)."""
    v = torch.arange(256, dtype=torch.float32)
    f = v / torch.tensor(denom, dtype=torch.float32)
    return torch.stack([bf((f - torch.tensor(m, dtype=torch.float32)) / torch.tensor(sd, dtype=torch.float32))
                        for m, sd in zip(mean, std)])


def all_bytes_frame():
    """uint8 [1, 16, 16, 3]: every byte value once per channel, in a different order in each."""
    v = torch.arange(256)
    return torch.stack([v, v.flip(0), (v * 7 + 3) % 256], 1).to(torch.uint8).view(1, 16, 16, 3)


def pool3x3s2(raw, use_min, pad_zero=False):
    """3x3 / stride 2 / pad 1 pooling of raw [n, c, h, w]: the maximum, or the minimum in the channels of ``use_min``; the
    padding never wins (pad_zero: the planted mistake, a padding of 0)."""
    sign = torch.where(use_min, -1.0, 1.0).to(raw.dtype).view(1, -1, 1, 1)
    if pad_zero:
        return F.max_pool2d(F.pad(raw * sign, (1, 1, 1, 1)), 3, 2, 0) * sign
    return F.max_pool2d(raw * sign, 3, 2, 1) * sign


@functools.lru_cache(maxsize=None)
def stem_case(n, fpg):
    """frames uint8 [n, 224, 224, 3] (frame CONST_FRAME a single colour: its output is constant away from the borders), the
    stem weight [64, 3, 7, 7] in bf16 values, gamma with both signs and a zero."""
    g = _seed("stem", n, fpg)
    frames = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, generator=g)
    frames[CONST_FRAME] = torch.tensor(CONST_COLOUR, dtype=torch.uint8)
    w4 = bf(torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5)
    gamma, beta = randomize_bn(64, g)
    return SimpleNamespace(n=n, fpg=fpg, groups=n // fpg, frames=frames, w4=w4, gamma=gamma, beta=beta,
                           label=f"n={n} frames_per_group={fpg}")


def stem_image(case):
    """The normalised image [n, 3, 224, 224] in bf16 values, through the table."""
    lut = normalize_lut()
    return torch.stack([lut[c][case.frames[..., c].long()] for c in range(3)], 1)


@functools.lru_cache(maxsize=None)
def stem_bundle(n, fpg):
    """(case, acc64, acc32 [n, 64, 112, 112], float64 (scale, shift), fp32 (scale, shift)); computed once."""
    case = stem_case(n, fpg)
    x = stem_image(case)
    acc64 = F.conv2d(x.double(), case.w4.double(), None, 2, 3)
    acc32 = F.conv2d(x, case.w4, None, 2, 3)
    rows = lambda a: a.permute(0, 2, 3, 1).reshape(-1, 64)
    off = list(range(0, n * 112 * 112 + 1, fpg * 112 * 112))
    return (case, acc64, acc32, ragged_stats(rows(acc64), off, case.gamma, case.beta, torch.float64),
            stem_fold(acc32, fpg, case.gamma, case.beta))


def stem_fold(acc32, fpg, gamma, beta, eps=BN_EPS, mistake=None):
    """stem_fused_kernel's partial sums and stem_fold_kernel in fp32: the sums and sums of squares of every tile of 16 x 16
    convolution outputs, added per group in frame and tile order; var = max(s2 / R - mean^2, 0)."""
    n = acc32.shape[0]
    tiles = acc32.view(n, 64, 7, 16, 7, 16).permute(0, 2, 4, 1, 3, 5).reshape(n * 49, 64, 256)
    p1, p2 = tiles.sum(2), (tiles * tiles).sum(2)
    groups = n // fpg
    scale, shift = torch.zeros(groups, 64), torch.zeros(groups, 64)
    inv_n = torch.ones((), dtype=torch.float32) / float(fpg * 112 * 112)
    for g in range(groups):
        s1, s2 = torch.zeros(64), torch.zeros(64)
        for t in range(g * fpg * 49, (g + 1) * fpg * 49):
            s1, s2 = s1 + p1[t], s2 + p2[t]
        if mistake == "drop_last_row":      # the last convolution output of the group's last frame
            last = acc32[(g + 1) * fpg - 1, :, -1, -1]
            s1, s2, inv_n = s1 - last, s2 - last * last, torch.ones((), dtype=torch.float32) / float(fpg * 112 * 112 - 1)
        mean = s1 * inv_n
        var = (s2 * inv_n - mean * mean).clamp_min(0.0)
        if mistake == "unbiased":
            var = var * (float(fpg * 112 * 112) / float(fpg * 112 * 112 - 1))
        scale[g] = gamma / torch.sqrt(var + eps32(eps))
        shift[g] = beta - mean * scale[g]
    return scale, shift


def stem_reference(n, fpg, apply, relu):
    """float64 [n * 56 * 56, 64]: apply = 0 the pooled raw map (the maximum where gamma >= 0, the minimum elsewhere);
    apply = 1 pool(act(acc * scale + shift)), which the monotone map makes act(sel * scale + shift)."""
    case, acc64, _, (sc, sh), _ = stem_bundle(n, fpg)
    if not apply:
        return pool3x3s2(acc64, case.gamma < 0).permute(0, 2, 3, 1).reshape(-1, 64)
    gi = torch.arange(case.groups).repeat_interleave(fpg)
    y = acc64 * sc[gi][:, :, None, None] + sh[gi][:, :, None, None]
    y = y.clamp_min(0.0) if relu else y
    return F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, 64)


def stem_restatement(n, fpg, apply, relu, mistake=None):
    """The fused stem in fp32 / bf16: the raw map rounded to bf16, pooled (max, or min where gamma < 0; the padding never
    wins); apply = 1: bf16(act(sel * scale + shift)), product and sum rounded separately."""
    assert mistake is None or mistake in STEM_MISTAKES
    case, _, acc32, _, (sc, sh) = stem_bundle(n, fpg)
    use_min = case.gamma < 0
    if mistake == "min_max_pool_swapped":
        use_min = ~use_min
    sel = pool3x3s2(bf(acc32), use_min, mistake == "pad_pool_with_zero").permute(0, 2, 3, 1).reshape(-1, 64)
    if not apply:
        return sel
    gi = torch.arange(case.groups).repeat_interleave(fpg * 56 * 56)
    y = sel * sc[gi] + sh[gi]
    return bf(y.clamp_min(0.0) if relu else y)


# --------------------------------------------------------------------------- which case notices which mistake
# conv1x1: (shape number, form, regime) and the check ("elements" / "moments"); "unbiased" also at the 49-row groups of the
# tile-local form (NOTICED_BY_LOCAL)
NOTICED_BY = {
    "unbiased": ((1, "two_pass", "normal"), "moments"),
    "drop_last_row": ((1, "two_pass", "normal"), "moments"),
    "first_row_of_next_group": ((1, "two_pass", "normal"), "moments"),
    "no_eps": ((1, "two_pass", "const"), "elements"),
    "stats_of_rounded_output": ((5, "two_pass", "mean40"), "moments"),
    "relu_before_residual": ((3, "affine_ra", "normal"), "elements"),
    "res_affine_of_next_group": ((3, "affine_ra", "normal"), "elements"),
    "gamma_next_channel": ((2, "two_pass", "normal"), "elements"),
    "in_affine_of_group_0": ((2, "two_pass", "normal"), "elements"),
    "k_tail_dropped": ((1, "two_pass", "normal"), "elements"),
}
NOTICED_BY_LOCAL = {"unbiased": (LOCAL_SHAPES[4], "normal")}      # 49-row groups, by the moments check alone
NOTICED_BY_STEM = {"min_max_pool_swapped": ((3, 3), 0, 0), "pad_pool_with_zero": ((3, 3), 0, 0)}  # ((n, fpg), apply, relu)
