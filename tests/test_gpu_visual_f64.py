"""The BatchNorm and pooling kernels of the visual front end (csrc/visual.hip), each on its own against float64:
avs_bn_batch_stats, avs_bn_apply, avs_pool2d_nhwc, avs_bn_maxpool_nhwc, avs_global_avgpool_nhwc and avs_segment_mean_f32,
in fp32, bf16 (the 8-channel instances and the narrow 4-channel one, forced by c % 8 != 0, by a stride % 8 != 0 and by an
8-byte aligned view) and f16x2 (operands packed on the CPU).  Cases, references, restatements and the bound come from
visual_f64_inputs; test_visual_f64_host.py shows on the host that the bound passes the fp32 restatement and fails every
planted mistake, and that the cases reach every kernel instance.

Every destination - scale / shift included - is pre-filled with NaN inside its window and with a sentinel in its pad
columns: the window must be finite afterwards, the pad columns and the rows outside every group bit for bit what they
were.  Every call runs twice, into fresh destinations, and must give the same bits.  All calls stay inside the documented
alignment (16 bytes fp32, 8 bytes narrow bf16, 32 bytes f16x2); misaligned calls are exercised as refusals on the host.

Left out on purpose: the second trip of the grid-stride loops of pool2d, bn_maxpool and global_avgpool (their caps of
65536 and 16384 blocks need hundreds of MB; bn_apply's second trip is run), and the P8 format, which no kernel here reads.

avs_bn_maxpool_nhwc is also held to the two-kernel sequence avs_bn_apply + avs_pool2d_nhwc(max) at these shapes: bit for
bit in fp32 and bf16; in f16x2 to the same stored values, because a value has more than one hi | lo image and splitting a
stored value again need not reproduce its halves: a stored value that lies halfway between two fp16 numbers, hi below and
lo = +half a step, splits again into hi above (ties to even) and lo = -half a step.  In the 3x3/2 ReLU case 4 of 3240
slots do so, on the device and in the CPU restatement of the format alike.

RATIO lines (printed per check; run with -s).  Measured on an MI355X, the largest err / e32 per kernel family and format
over all cases of this file (err and e32 both against float64), with the case where err came closest to its bound:

  family          format(s)                      checks  max err/e32  closest to the bound
  bn_batch_stats  f32                            18      1.00         c=4 mean40 shift: err 3.7e-3, bound 5.2e-2
  bn_batch_stats  bf16                           18      1.00         c=64 mean40 shift: err 3.4e-3, bound 4.1e-2
  bn_batch_stats  f16x2                          14      1.00         c=64 mean40 shift: err 4.1e-3, bound 4.8e-2
  bn_apply        f32 (incl. 32769 x 256)        10      1.00         c=64 inplace_res: err 2.7e-6, bound 3.0e-5
  bn_apply        bf16 wide / narrow c, stride,  8 each  1.00         narrow-c c=68 inplace_res: err 3.1e-2, bound 1.2e-1
                  view
  bn_apply        f16x2                          8       1.00         c=64 res_relu: err 2.5e-6, bound 2.9e-5
  pool2d avg      f32                            80      1.00         c=12 plain 5x5/1 p2 7x7: err 1.9e-7, bound 1.7e-6
  pool2d avg      bf16 wide, narrow stride, view 40 each 1.00         wide bias_relu 3x3/1 p1 17x13: err 3.9e-3, bound 1.6e-2
  pool2d avg      bf16 narrow c (c = 12 and 4)   80      1.00         c=12 bias_relu 3x3/2 p1 1x1: err 2.6e-3, bound 1.0e-2
  pool2d avg      f16x2                          40      1.00         plain 5x5/1 p2 17x13: err 1.7e-7, bound 1.6e-6
  bn_maxpool      f32                            5       1.00         3x3/2 p1 relu: err 8.7e-7, bound 1.7e-5
  bn_maxpool      bf16 wide / the three narrow   5 each  1.00         narrow-stride 3x3/2 p1: err 5.8e-2, bound 2.3e-1
  bn_maxpool      f16x2                          5       1.00         3x3/2 p1 relu groups=0: err 1.5e-6, bound 1.6e-5
  global_avgpool  f32                            10      1.00         n=600 hw=64 c=8: err 6.6e-7, bound 4.0e-6
  global_avgpool  bf16, bf16 8-byte view         10 each 1.00         n=600 hw=64 c=8: err 7.5e-8, bound 1.7e-6
  global_avgpool  f16x2                          6       1.00         n=600 hw=64 c=8: err 4.9e-7, bound 3.3e-6

No family exceeds err / e32 = 1.00: the restatements follow the kernels' order of operations, so the kernels' largest
error is the restatement's (in bf16 half an ulp of the stored result: err = e32 = a quarter of the bound).  Max pooling
and segment_mean are held to equality, not to the bound."""
import pytest
import torch

import visual_f64_inputs as vfi

pytestmark = pytest.mark.gpu

S = vfi.SENTINEL
NAN = float("nan")
IDS = [vfi.iname(*i) for i in vfi.INSTANCES]


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _code(ops, fmt):
    return ops.dtype_code(torch.bfloat16) if fmt == "bf16" else ops.dtype_code(torch.float32, "f16x2" if fmt == "f16x2" else False)


def _encode(fmt, t):
    """fp32 values [rows, ld] -> the format's storage (CPU)."""
    return t.bfloat16() if fmt == "bf16" else vfi.emu_pack(t) if fmt == "f16x2" else t.clone()


def _decode(fmt, t):
    t = t.cpu()
    return t.float() if fmt == "bf16" else vfi.emu_unpack(t.contiguous()) if fmt == "f16x2" else t.clone()


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _place(fmt, values, ld, off, dev):
    """values [rows, c] in columns [off, off + c) of a matrix ``ld`` wide whose other columns hold the sentinel:
    (the matrix on the device, the window)."""
    rows, c = values.shape
    assert ld >= off + c
    wide = torch.full((rows, ld), S)
    wide[:, off:off + c] = values
    buf = _encode(fmt, wide).to(dev)
    return buf, buf[:, off:off + c]


def _nan_dest(fmt, rows, c, ld, off, dev):
    return _place(fmt, torch.full((rows, c), NAN), ld, off, dev)


def _read(fmt, buf, before, off, c, live=None):
    """The window of a destination as fp32 on the CPU, after asserting that everything outside it - pad columns, and
    rows where ``live`` is False - is bit for bit what it was, and that the window is finite where live."""
    a, b = _bits(buf).clone(), _bits(before).clone()
    got = _decode(fmt, buf[:, off:off + c])
    if live is None:
        live = torch.ones(a.shape[0], dtype=torch.bool)
    a[live, off:off + c] = 0
    b[live, off:off + c] = 0
    assert torch.equal(a, b), "a pad column or a row outside every group was written"
    assert torch.isfinite(got[live]).all(), "a destination element was left unwritten or is not finite"
    return got


def _check(family, fmt, label, name, got, ref, cpu32, scale=None):
    ok, err, e32, bound = vfi.compare(got, ref, cpu32, scale)
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO family={family!r} fmt={fmt!r} case={label!r} tensor={name} err={err:.3e} e32={e32:.3e} bound={bound:.3e} "
          f"err/e32={ratio:.2f}")
    assert ok, f"{family} {label} {name}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e})"


# --------------------------------------------------------------------------- statistics
def _stats_into(fmt, xw, rows, ldx, gr, gamma, beta, scale, shift):
    """avs_bn_batch_stats through the C ABI into destinations of the caller (ops.bn_batch_stats allocates its own)."""
    ops, abi = _api()
    abi.check(abi.lib().avs_bn_batch_stats(_code(ops, fmt), ops._p(xw), rows, xw.shape[1], ldx, ops._p(gr), gr.numel() - 1,
                                           ops._p(gamma), ops._p(beta), vfi.BN_EPS, ops._p(scale), ops._p(shift),
                                           ops._stream()), "avs_bn_batch_stats")


@pytest.mark.parametrize("fmt", vfi.STATS_FORMATS)
def test_bn_batch_stats(dev, fmt):
    """c from one channel-thread (256 row-threads) to two blocks in y with one live channel-thread in the second; groups
    of 1, 0, 3, 1, tr - 1, tr + 1 and 777 rows; N(0, 1), mean 40 >> spread 1 and a constant group; gamma of both signs and
    an exact 0; x a column window (ldx = c + 8).  An empty group gives scale = shift = 0."""
    ops, abi = _api()
    for c, regime in vfi.stats_cases(fmt):
        case, ref, cpu32 = vfi.stats_bundle(fmt, c, regime)
        xbuf, xw = _place(fmt, case.x, case.ldx, 0, dev)
        gr = torch.tensor(case.group_rows, dtype=torch.int64, device=dev)
        gamma, beta = case.gamma.to(dev), case.beta.to(dev)
        n_groups = len(case.group_rows) - 1
        runs = []
        for _ in range(2):
            scale = torch.full((n_groups, c), NAN, device=dev)
            shift = torch.full((n_groups, c), NAN, device=dev)
            _stats_into(fmt, xw, case.rows, case.ldx, gr, gamma, beta, scale, shift)
            runs.append((scale.cpu(), shift.cpu()))
        (scale, shift), again = runs
        assert torch.equal(_bits(scale), _bits(again[0])) and torch.equal(_bits(shift), _bits(again[1]))
        assert torch.isfinite(scale).all() and torch.isfinite(shift).all(), case.label
        assert (scale[1] == 0).all() and (shift[1] == 0).all(), "empty group: scale = shift = 0"
        via_ops = ops.bn_batch_stats(xw, gr, gamma, beta, vfi.BN_EPS, code=_code(ops, fmt))
        assert torch.equal(_bits(via_ops[0]), _bits(scale)) and torch.equal(_bits(via_ops[1]), _bits(shift))
        _check("bn_batch_stats", fmt, case.label, "scale", scale, ref[0], cpu32[0])
        _check("bn_batch_stats", fmt, case.label, "shift", shift, ref[1], cpu32[1])
        nonempty = [g for g in range(n_groups) if g != 1]
        assert (scale[:, 1] == 0).all() and (shift[nonempty, 1] == case.beta[1]).all(), "gamma == 0: scale = 0, shift = beta"
        for g in (0, 3) + ((vfi.CONST_GROUP,) if regime == "const" else ()):      # variance exactly 0
            want = case.gamma.double() / torch.sqrt(vfi.eps32().double())
            assert ((scale[g].double() - want).abs() <= 4 * vfi.EPS32 * want.abs()).all(), (case.label, g)
        assert torch.equal(_bits(xbuf), _bits(_place(fmt, case.x, case.ldx, 0, "cpu")[0]))


# --------------------------------------------------------------------------- apply
def _run_apply(ops, dev, case):
    fmt, c = case.fmt, case.c
    gr = torch.tensor(case.group_rows, dtype=torch.int64, device=dev) if case.group_rows is not None else None
    sc, sf = case.scale.to(dev), case.shift.to(dev)
    res = None
    if case.res is not None:
        rbuf = _encode(fmt, case.res_wide).to(dev)
        res = rbuf[:, case.ores[1]:case.ores[1] + c]
    live = case.gidx >= 0
    outs = []
    for _ in range(2):
        xbuf, xw = _place(fmt, case.x, case.ox[0], case.ox[1], dev)
        if case.inplace:
            ybuf, yw, before, (ld, off) = xbuf, xw, xbuf.clone(), case.ox
        else:
            ld, off = case.oy
            ybuf, yw = _nan_dest(fmt, case.rows, c, ld, off, dev)
            before = ybuf.clone()
        ret = ops.bn_apply(xw, sc, sf, gr, case.max_group_rows, res, ops.ACT_RELU if case.relu else ops.ACT_NONE, out=yw,
                           code=_code(ops, fmt))
        assert ret.data_ptr() == yw.data_ptr()
        got = _read(fmt, ybuf, before, off, c, live)
        if not case.inplace:
            assert torch.equal(_bits(xbuf), _bits(_place(fmt, case.x, case.ox[0], case.ox[1], "cpu")[0]))
        outs.append((got, _bits(ybuf)))
    assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
    if res is not None:
        assert torch.equal(_bits(rbuf), _bits(_encode(fmt, case.res_wide)))
    got = outs[0][0]
    got[~live] = 0.0
    return got


@pytest.mark.parametrize("fmt,narrow", vfi.INSTANCES, ids=IDS)
def test_bn_apply(dev, fmt, narrow):
    """The group tables of the statistics (an empty group between unequal ones, rows after the last group); ldx, ldy and
    ldr pairwise different; in place with a residual (the product's call); max_group_rows = 1 with larger groups present;
    groups == 0; ReLU on and off."""
    ops, _ = _api()
    for base_c in vfi.APPLY_BASE_C:
        for variant in vfi.APPLY_VARIANTS:
            case, ref, mag, cpu32 = vfi.apply_bundle(fmt, narrow, base_c, variant)
            got = _run_apply(ops, dev, case)
            _check("bn_apply", vfi.iname(fmt, narrow), case.label, "y", got, ref, cpu32, mag)


def test_bn_apply_second_trip_of_the_capped_grid(dev):
    """32769 x 256 fp32 = 2 097 216 vectors: the 8192 blocks of 256 threads cover all but the last 64, which only the
    second trip of the grid-stride loop reaches."""
    ops, _ = _api()
    rows, c = vfi.APPLY_BIG
    case, ref, mag, cpu32 = vfi.apply_bundle("f32", None, c, "res_relu", True)
    assert case.rows == rows and case.c == c and case.max_group_rows == rows
    got = _run_apply(ops, dev, case)
    _check("bn_apply", "f32", case.label, "y", got, ref, cpu32, mag)
    _check("bn_apply", "f32", case.label + " last row", "y", got[-1:], ref[-1:], cpu32[-1:], mag)


# --------------------------------------------------------------------------- pooling
def _place4(fmt, x, ps, off, dev):
    n, h, w, c = x.shape
    buf, _ = _place(fmt, x.reshape(-1, c), ps, off, dev)
    return buf, buf.view(n, h, w, ps)[..., off:off + c]


def _nan_dest4(fmt, n, h, w, c, ps, off, dev):
    return _place4(fmt, torch.full((n, h, w, c), NAN), ps, off, dev)


def _pool_cases(fmt, narrow, mode):
    return [vfi.pool_case(fmt, narrow, b, mode, fl, ksp, hw) for b in vfi.pool_bases(fmt, narrow) for fl in vfi.POOL_FLAVOURS[mode]
            for ksp in vfi.POOL_KSP for hw in vfi.POOL_MAPS]


@pytest.mark.parametrize("mode", ("max", "avg"))
@pytest.mark.parametrize("fmt,narrow", vfi.INSTANCES, ids=IDS)
def test_pool2d(dev, fmt, narrow, mode):
    """Windows 3x3/2 p1, 3x3/2 p0, 3x3/1 p1, 2x2/2 and 5x5/1 p2 on maps of 1x1, 2x5, 7x7 and 17x13 (smaller than the
    window, non-square, window, padding and edge meeting on both sides), input and output channel slices; c = 12 and 4 where 4 channels make a vector, 24 elsewhere.  Max pooling
    - also of an all-negative map, where a padding of 0 would win - equals the float64 maximum; the average, with
    count_include_pad, plain and as relu(avg + bias), lies within the bound."""
    ops, _ = _api()
    for case in _pool_cases(fmt, narrow, mode):
        c = case.c
        xbuf, xv = _place4(fmt, case.x, case.ox[0], case.ox[1], dev)
        bias = case.bias.to(dev) if case.bias is not None else None
        outs = []
        for _ in range(2):
            ybuf, yv = _nan_dest4(fmt, case.n, case.ho, case.wo, c, case.oy[0], case.oy[1], dev)
            before = ybuf.clone()
            ops.pool2d(xv, mode, case.k, case.s, case.p, yv, bias=bias, act=ops.ACT_RELU if case.relu else ops.ACT_NONE,
                       code=_code(ops, fmt))
            outs.append((_read(fmt, ybuf, before, case.oy[1], c), _bits(ybuf)))
        assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
        got = outs[0][0].view(case.n, case.ho, case.wo, c)
        ref = vfi.pool_eval(case, torch.float64)
        if mode == "max":
            assert torch.equal(got.double(), ref), case.label
            if case.flavour == "negative":
                assert (got <= -0.5).all()
        else:
            _check("pool2d avg", vfi.iname(fmt, narrow), case.label, "y", got, ref, vfi.pool_restatement(case))
        assert torch.equal(_bits(xbuf), _bits(_place4(fmt, case.x, case.ox[0], case.ox[1], "cpu")[0]))


# --------------------------------------------------------------------------- BatchNorm apply + max pooling
@pytest.mark.parametrize("fmt,narrow", vfi.INSTANCES, ids=IDS)
def test_bn_maxpool(dev, fmt, narrow):
    """9 images of 6x10 in groups of 1, 1, 0, 3, 1 and 3 images (the binary search over 7 offsets, an empty group among
    them) and with groups == 0; scales of both signs; ReLU on and off; 3x3/2 p1 and 2x2/2.  Against float64, and bit for
    bit avs_bn_apply followed by avs_pool2d_nhwc(max)."""
    ops, _ = _api()
    base_c = vfi.pool_bases(fmt, narrow)[0]
    cases = [vfi.bnmaxpool_case(fmt, narrow, base_c, ksp, relu) for ksp in vfi.BMP_KSP for relu in (False, True)] + \
        [vfi.bnmaxpool_case(fmt, narrow, base_c, vfi.BMP_KSP[0], True, grouped=False)]
    for case in cases:
        c, code = case.c, _code(ops, fmt)
        xbuf, xv = _place4(fmt, case.x, case.ox[0], case.ox[1], dev)
        gr = torch.tensor(case.group_rows, dtype=torch.int64, device=dev) if case.group_rows is not None else None
        sc, sf = case.scale.to(dev), case.shift.to(dev)
        outs = []
        for _ in range(2):
            ybuf, yv = _nan_dest4(fmt, case.n, case.ho, case.wo, c, case.oy[0], case.oy[1], dev)
            before = ybuf.clone()
            ops.bn_maxpool(xv, sc, sf, gr, case.relu, case.k, case.s, case.p, yv, code=code)
            outs.append((_read(fmt, ybuf, before, case.oy[1], c), _bits(ybuf)))
        assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
        got = outs[0][0].view(case.n, case.ho, case.wo, c)
        ref, mag = vfi.bnmaxpool_eval(case, torch.float64)
        _check("bn_maxpool", vfi.iname(fmt, narrow), case.label, "y", got, ref, vfi.bnmaxpool_restatement(case), mag)
        # the two-kernel sequence: the full-resolution map through avs_bn_apply, then max pooling
        rows = case.n * case.h * case.w
        x2d = xbuf[:, case.ox[1]:case.ox[1] + c]
        full_buf, full = _nan_dest(fmt, rows, c, case.oy[0], case.oy[1], dev)
        ops.bn_apply(x2d, sc, sf, gr, 3 * case.h * case.w, None, ops.ACT_RELU if case.relu else ops.ACT_NONE, out=full,
                     code=code)
        zbuf, zv = _nan_dest4(fmt, case.n, case.ho, case.wo, c, case.oy[0], case.oy[1], dev)
        ops.pool2d(full_buf.view(case.n, case.h, case.w, case.oy[0])[..., case.oy[1]:case.oy[1] + c], "max", case.k, case.s,
                   case.p, zv, code=code)
        if fmt == "f16x2":      # a value has more than one hi | lo image: re-splitting the stored full-resolution value need
            # not reproduce the halves that splitting the fp32 maximum gives - the stored VALUES are the same
            assert torch.equal(_read(fmt, zbuf, before, case.oy[1], c), outs[0][0]), case.label
        else:
            assert torch.equal(_bits(zbuf), outs[0][1]), case.label
        assert torch.equal(_bits(xbuf), _bits(_place4(fmt, case.x, case.ox[0], case.ox[1], "cpu")[0]))


# --------------------------------------------------------------------------- global average pooling
@pytest.mark.parametrize("fmt,view", [("f32", False), ("bf16", False), ("bf16", True), ("f16x2", False)],
                         ids=["f32", "bf16", "bf16-view", "f16x2"])
def test_global_avgpool(dev, fmt, view):
    """A single pixel, 49 and 64; c = 4 (one vector per image), 8 and 2048; 1, 3 and 600 images (600 x c/4 threads: more
    than one block); the fp32 output a slice of a wider matrix; bf16 also from an 8-byte aligned view."""
    ops, _ = _api()
    for n, hw, c in vfi.gap_shapes(fmt):
        case = vfi.gap_case(fmt, n, hw, c, view)
        flat = torch.full((n * hw * c + 16,), S)
        lead = 4 if view else 0
        flat[lead:lead + n * hw * c] = case.x.reshape(-1)
        enc = _encode(fmt, flat.view(1, -1)).view(-1).to(dev)
        x = enc[lead:lead + n * hw * c].view(n, hw, 1, c)
        assert x.is_contiguous() and x.data_ptr() % (8 if view else 32 if fmt == "f16x2" else 16) == 0
        outs = []
        for _ in range(2):
            ybuf, yw = _nan_dest("f32", n, c, case.ldy, case.off_y, dev)
            before = ybuf.clone()
            ops.global_avgpool(x, out=yw, code=_code(ops, fmt))
            outs.append((_read("f32", ybuf, before, case.off_y, c), _bits(ybuf)))
        assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
        _check("global_avgpool", fmt + ("-view" if view else ""), case.label, "y", outs[0][0], vfi.gap_reference(case),
               vfi.gap_restatement(case))
        if hw == 1:
            assert torch.equal(outs[0][0], case.x[:, 0])
        assert torch.equal(_bits(enc), _bits(_encode(fmt, flat.view(1, -1)).view(-1)))


# --------------------------------------------------------------------------- segment mean
@pytest.mark.parametrize("d,seg", vfi.SEGMENT_CASES, ids=[f"d{d}-{len(s) - 1}seg" for d, s in vfi.SEGMENT_CASES])
def test_segment_mean(dev, d, seg):
    """ldx > d and ldo > d; empty segments (zeros), single rows and 39 rows; 3000 one-row segments; rows before the first
    and after the last offset belong to no segment.  Bit for bit the sequential fp32 sum in row order, one division."""
    ops, _ = _api()
    case = vfi.segment_case(d, seg)
    xbuf = case.wide.to(dev)
    segd = torch.tensor(seg, dtype=torch.int64, device=dev)
    want = vfi.segment_mean_sequential(case.x, seg)
    outs = []
    for _ in range(2):
        ybuf, yw = _nan_dest("f32", len(seg) - 1, d, case.ldo, 0, dev)
        before = ybuf.clone()
        ops.segment_mean(xbuf[:, :d], segd, out=yw)
        outs.append((_read("f32", ybuf, before, 0, d), _bits(ybuf)))
    assert torch.equal(outs[0][1], outs[1][1]), "two runs differ"
    assert torch.equal(_bits(outs[0][0]), _bits(want)), case.label
    empty = torch.tensor([b == a for a, b in zip(seg[:-1], seg[1:])])
    assert (outs[0][0][empty] == 0).all()
    assert torch.equal(xbuf.cpu(), case.wide)
