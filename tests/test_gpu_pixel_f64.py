"""The kernels that touch raw uint8 pixels, each on its own: avs_resize_bilinear_u8, avs_frames_normalize_u8,
avs_hsv_frame_diff_u8, avs_pull_copy_u8 (csrc/visual.hip), avs_resize_bilinear_gather2_u8 (csrc/stage1_batch.hip) and
avs_hsv_frame_diff_batch_u8 (csrc/shots_batch.hip).  Cases, float64 references, restatements and bounds come from
pixel_f64_inputs; test_pixel_f64_host.py shows on the host that the oracles lie within the derived bounds of the float64
definitions, that every planted mistake is noticed, and that the cases reach every path.

Every comparison is equality with a CPU restatement of the kernel's integer or fp32 arithmetic, or the derived bound:
  * resize: EVERY output byte within ``resize_bound`` (0.8818 + 1.5e-5 (sh + sw + 1) grey levels) of the float64 bilinear
    definition, and equal to the 32-bit restatement (= oracle.cnn.cv_resize_linear_u8); the gather form equal to it too;
  * HSV sums: equal to the restatement's (= oracle.shots.bgr2hsv_u8, which the host test holds to V exact, |S - def| <=
    0.5311, circular |H - def| <= 0.6556 on all 2^24 colours);
  * normalise: bits of the fp32 restatement (rounded to bf16, or packed by emu_pack), which lies within
    scorer_f64_inputs.compare of the float64 expression;
  * pull copy: the bytes of the pinned source.

Margins measured on the host: the oracle's largest distance to the float64 resize 0.8026 levels (bound 0.8818+), to the
float64 S 0.5215 (0.5311), to H 0.6400 (0.6556); the smallest excess of a ‡ mistake over the resize bound 0.40 levels.

Every destination is followed (the gather form's: preceded too) by sentinel bytes that must stay, every call runs twice
into fresh destinations and must give the same bits.

Measured on an MI355X (RATIO lines, run with -s): every comparison holds; the dense resize's distance to the float64
definition is the oracle's at every case (largest 0.8026 levels at 37 x 53 -> 36 x 300 noise, 0.7934 at 240 x 320 ->
224 x 224 noise; 0.5 at the exact 2 x ratio, 0 at the exact 3 x ratio, at 1 x 1 sources and at the identity).  52 tests,
2.1 s in all; the slowest is the 257-frame colour cube (0.65 s, most of it the restatement on the host)."""
import functools

import numpy as np
import pytest
import torch

import pixel_f64_inputs as pfi

pytestmark = pytest.mark.gpu

S8 = pfi.SENTINEL_U8
PAD = 64
F32 = np.float32
SHAPE, ALIGN = -2, -3      # AVS_E_SHAPE, AVS_E_ALIGN


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _id(pair):
    (sh, sw), (dh, dw) = pair
    return f"{sh}x{sw}-{dh}x{dw}"


@functools.lru_cache(maxsize=None)
def _resize_refs(src, content, dst, frames=pfi.RESIZE_FRAMES):
    """(restatement uint8, float64 reference) of one case, computed once and shared."""
    f = pfi.resize_case(src, content, frames)
    return pfi.resize_restatement(f, *dst), pfi.resize_reference(f, *dst)


def _resize_dense(dev, frames_t, dh, dw):
    """avs_resize_bilinear_u8 into a sentinel-followed buffer: uint8 [n, dh, dw, 3] on the host."""
    ops, abi = _api()
    n, sh, sw, _ = frames_t.shape
    count = n * dh * dw * 3
    buf = torch.full((count + PAD,), S8, dtype=torch.uint8, device=dev)
    abi.check(abi.lib().avs_resize_bilinear_u8(ops._p(frames_t), n, sh, sw, ops._p(buf), dh, dw, ops._stream()), "resize")
    host = buf.cpu()
    assert (host[count:] == S8).all()
    return host[:count].view(n, dh, dw, 3).numpy()


# --------------------------------------------------------------------------- resize
@pytest.mark.parametrize("pair", pfi.RESIZE_PAIRS, ids=_id)
def test_resize_every_byte_within_the_bound_of_float64(dev, pair):
    src, dst = pair
    for content in pfi.CONTENTS:
        want, ref = _resize_refs(src, content, dst)
        d = torch.from_numpy(np.array(pfi.resize_case(src, content))).to(dev)
        got = _resize_dense(dev, d, *dst)
        dist = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"RATIO resize {_id(pair)} {content}: distance {dist:.4f} bound {pfi.resize_bound(*src):.4f}")
        assert dist <= pfi.resize_bound(*src), (pair, content, dist)
        assert np.array_equal(got, want), (pair, content)
        assert np.array_equal(_resize_dense(dev, d, *dst), got)


def test_resize_second_grid_stride_trip(dev):
    """65 537 frames of 3 x 5 -> 8 x 8: 64 pixels past the 16384 x 256 threads of one trip."""
    big = pfi.RESIZE_BIG
    want, ref = _resize_refs(big.src, "noise", big.dst, big.base)
    which = torch.arange(big.frames) % big.base
    d = torch.from_numpy(np.array(pfi.resize_case(big.src, "noise", big.base))).to(dev).index_select(0, which.to(dev))
    got = _resize_dense(dev, d, *big.dst)
    assert np.array_equal(got, want[which.numpy()])
    worst = 0.0
    for a in range(0, big.frames, 8192):
        k = which.numpy()[a:a + 8192]
        worst = max(worst, float(np.abs(got[a:a + 8192].astype(np.float64) - ref[k]).max()))
    assert worst <= pfi.resize_bound(*big.src)
    assert np.array_equal(_resize_dense(dev, d, *big.dst), got)


@pytest.mark.parametrize("pair", pfi.RESIZE_PAIRS, ids=_id)
def test_resize_gather_gives_the_dense_bytes(dev, pair):
    """One and two destinations, bases at byte offsets 0, 1 and 15 of sentinel-filled buffers, through an index with a
    repeat, a descending run and one row outside the source: the bytes of the restatement (which the dense form is held
    to above), the skipped row and every sentinel as they were."""
    ops, _ = _api()
    src, dst = pair
    idx = torch.tensor(pfi.GATHER_INDEX, dtype=torch.int64, device=dev)
    count, bad = len(pfi.GATHER_INDEX), pfi.GATHER_SKIPPED
    rows = [i for i in range(count) if i != bad]
    for content in ("noise", "checker"):
        d = torch.from_numpy(np.array(pfi.resize_case(src, content))).to(dev)
        for sizes in ([dst], [dst, pfi.GATHER_SECOND], [pfi.GATHER_SECOND, dst]):
            for off in pfi.GATHER_OFFSETS:
                for rep in range(2 if off == 1 else 1):
                    bufs, outs = [], []
                    for k, (dh, dw) in enumerate(sizes):
                        o = (off + 7 * k) % 16                      # (the second destination at another alignment)
                        nb = count * dh * dw * 3
                        bufs.append((torch.full((o + nb + PAD,), S8, dtype=torch.uint8, device=dev), o, nb))
                        outs.append(bufs[-1][0][o:o + nb].view(count, dh, dw, 3))
                    ops.resize_gather(d, idx, count, sizes, outs)
                    for (buf, o, nb), size in zip(bufs, sizes):
                        host = buf.cpu()
                        assert (host[:o] == S8).all() and (host[o + nb:] == S8).all(), (pair, content, size, off)
                        got = host[o:o + nb].view(count, *size, 3).numpy()
                        want = _resize_refs(src, content, size)[0]
                        assert (got[bad] == S8).all(), (pair, content, size, off)
                        assert np.array_equal(got[rows], want[[pfi.GATHER_INDEX[i] for i in rows]]), (pair, content, size, off)
        dense = _resize_dense(dev, d, *dst)                                 # and the dense form on the device, directly
        assert np.array_equal(ops.resize_gather(d, idx, 4, [dst])[0].cpu().numpy(), dense[list(pfi.GATHER_INDEX[:4])])


# --------------------------------------------------------------------------- HSV
def _hsv(dev, frames_t, step, offsets_t=None):
    """The per-video (or, with offsets, the batch) entry point into sentinel-followed sums: int64 [n, 3] on the host."""
    ops, abi = _api()
    n, h, w, _ = frames_t.shape
    sums = torch.full((n * 3 + 8,), -7, dtype=torch.int32, device=dev)
    if offsets_t is None:
        abi.check(abi.lib().avs_hsv_frame_diff_u8(ops._p(frames_t), n, h, w, step, ops._p(sums), ops._stream()), "hsv")
    else:
        abi.check(abi.lib().avs_hsv_frame_diff_batch_u8(ops._p(frames_t), n, h, w, step, ops._p(offsets_t),
                                                        offsets_t.numel() - 1, ops._p(sums), ops._stream()), "hsv batch")
    host = sums.cpu()
    assert (host[n * 3:] == -7).all()
    return (host[:n * 3].to(torch.int64) & 0xFFFFFFFF).view(n, 3).numpy()


def test_hsv_all_colours_through_the_device_conversion(dev):
    """257 frames of 256 x 256, frame 1 + b = the colours (b, y, x): every colour is converted twice (as the current and as
    the previous frame), 32 workgroups a frame, 8 trips."""
    ops, _ = _api()
    cube = pfi.hsv_cube()
    want = pfi.hsv_sums(cube)
    d = torch.from_numpy(cube).to(dev)
    got = _hsv(dev, d, 1)
    assert np.array_equal(got, want)
    assert np.array_equal(_hsv(dev, d, 1), got)
    assert np.array_equal(ops.hsv_frame_diff(d[:9]).cpu().numpy(), want[:9])


@pytest.mark.parametrize("size", pfi.HSV_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hsv_sums_per_video_and_batch(dev, size):
    ops, _ = _api()
    frames = pfi.hsv_case(size)
    d = torch.from_numpy(np.array(frames)).to(dev)
    tables = ops.ShotTables(pfi.HSV_VIDEOS, 15, dev)
    for step in pfi.HSV_STEPS:
        want = pfi.hsv_sums(frames, step)
        for n in (3, 1, 2, pfi.HSV_FRAMES):
            got = _hsv(dev, d[:n], step)
            assert np.array_equal(got, want[:n]), (size, step, n)
            assert np.array_equal(_hsv(dev, d[:n], step), got)
        cut = pfi.hsv_sums(frames, step, pfi.HSV_VIDEOS)
        got = _hsv(dev, d, step, tables.offsets_t)
        assert np.array_equal(got, cut), (size, step)
        assert np.array_equal(_hsv(dev, d, step, tables.offsets_t), got)
        assert np.array_equal(ops.hsv_frame_diff_batch(d, tables, step).cpu().numpy(), cut)
        for a, b in zip(pfi.HSV_VIDEOS[:-1], pfi.HSV_VIDEOS[1:]):
            one = _hsv(dev, d[a:b], step)
            assert not one[0].any() and np.array_equal(one, got[a:b]), (size, step, a)       # zeros at each first frame


def test_hsv_refuses_more_than_65536_frames_and_writes_nothing(dev):
    ops, abi = _api()
    n = pfi.HSV_MAX_FRAMES + 1
    d = torch.zeros((n, 1, 1, 3), dtype=torch.uint8, device=dev)
    sums = torch.full((n * 3,), -7, dtype=torch.int32, device=dev)
    assert abi.lib().avs_hsv_frame_diff_u8(ops._p(d), n, 1, 1, 1, ops._p(sums), ops._stream()) == SHAPE
    torch.cuda.synchronize()
    assert (sums == -7).all()
    got = _hsv(dev, d[:n - 1], 1)                          # 65 536 frames: the most one call takes
    assert got.shape == (n - 1, 3) and not got.any()
    tables = ops.ShotTables([0, 5, n], 15, dev)            # the batch form has no such limit
    assert not _hsv(dev, d, 1, tables.offsets_t).any()


# --------------------------------------------------------------------------- normalise
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16x2": torch.float32}
_FILL = 93.0            # exact in bf16 and fp32; no normalised value of these cases equals it


def _normalize(dev, fmt, frames_t, denom, affine, oh, ow, pt, pl):
    """ops.frames_normalize into a buffer followed by a sentinel image: the output [n, oh, ow, 4] on the host."""
    ops, abi = _api()
    n = frames_t.shape[0]
    count, tail = n * oh * ow * 4, oh * ow * 4
    buf = torch.full((count + tail,), _FILL, dtype=_TORCH[fmt], device=dev)
    mean, std = pfi.NORM_STATS[float(denom)]
    ops.frames_normalize(frames_t, _TORCH[fmt], denom, mean, std, oh, ow, pt, pl, affine, buf[:count].view(n, oh, ow, 4),
                         code=abi.AVS_F16X2 if fmt == "f16x2" else None)
    host = buf.cpu()
    assert (host[count:] == _FILL).all()
    return host[:count].view(n, oh, ow, 4)


def _norm_expected(fmt, r32):
    """The bits the kernel must write for the fp32 restatement r32 [n, oh, ow, 4]."""
    if fmt == "f32":
        return torch.from_numpy(r32).view(torch.int32)
    if fmt == "bf16":
        return torch.from_numpy(r32).bfloat16().view(torch.int16)
    return pfi.h2_words(r32)


def _norm_bits(fmt, got):
    if fmt == "f32":
        return got.view(torch.int32)
    if fmt == "bf16":
        return got.view(torch.int16)
    return got.contiguous().view(torch.int16).reshape(-1, 2, 8)


@pytest.mark.parametrize("denom", [255.0, 1.0])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine6"])
@pytest.mark.parametrize("fmt", pfi.NORM_FORMATS)
def test_normalize_every_byte_value_and_geometry(dev, fmt, affine, denom):
    frames = pfi.norm_case()
    d = torch.from_numpy(np.array(frames)).to(dev)
    aff = pfi.NORM_AFFINE if affine else None
    for pt, pl in pfi.NORM_PADS:
        oh, ow = pfi.norm_geometry(pt, pl)
        r32 = pfi.normalize_eval(frames, denom, aff, oh, ow, pt, pl)
        got = _normalize(dev, fmt, d, denom, aff, oh, ow, pt, pl)
        bits = _norm_bits(fmt, got)
        assert torch.equal(bits, _norm_expected(fmt, r32)), (fmt, affine, denom, pt, pl)
        assert torch.equal(_norm_bits(fmt, _normalize(dev, fmt, d, denom, aff, oh, ow, pt, pl)), bits)
        inside = np.zeros((frames.shape[0], oh, ow, 4), dtype=bool)
        inside[:, pt:pt + frames.shape[1], pl:pl + frames.shape[2], :3] = True
        if fmt == "f16x2":       # the padding and the fourth channel: zero in both halves
            zero = torch.from_numpy(~inside).reshape(-1, 8)
            assert (bits[:, 0][zero] == 0).all() and (bits[:, 1][zero] == 0).all()
        else:
            assert (bits[torch.from_numpy(~inside)] == 0).all()
        if fmt == "f32":         # and the float64 definition, by the shared bound
            r64 = pfi.normalize_eval(frames, denom, aff, oh, ow, pt, pl, dtype=np.float64)
            ok, err, e32, bound = pfi.compare(got, r64, r64.astype(F32))
            assert ok, (affine, denom, pt, pl, err, bound)


@pytest.mark.parametrize("fmt", pfi.NORM_FORMATS)
def test_normalize_second_grid_stride_trip(dev, fmt):
    """2 x 2 frames into 4 x 4 images (pad 1 / 1), one frame more than one trip of the capped grid covers."""
    n, nb = pfi.NORM_BIG[fmt], pfi.NORM_BIG_BASE
    base = pfi.norm_case((2, 2), nb)
    which = torch.arange(n) % nb
    d = torch.from_numpy(np.array(base)).to(dev).index_select(0, which.to(dev))
    r32 = pfi.normalize_eval(base, 255.0, pfi.NORM_AFFINE, 4, 4, 1, 1)
    got = _normalize(dev, fmt, d, 255.0, pfi.NORM_AFFINE, 4, 4, 1, 1)
    want = _norm_expected(fmt, r32)
    per = want.numel() // nb
    assert torch.equal(_norm_bits(fmt, got).reshape(n, per), want.reshape(nb, per).index_select(0, which))


# --------------------------------------------------------------------------- pull copy
def _pull(dev, src, workgroups):
    ops, _ = _api()
    nbytes = len(src)
    host = torch.from_numpy(src).pin_memory()
    buf = torch.full((PAD + nbytes + PAD,), S8, dtype=torch.uint8, device=dev)
    ops.pull_copy(host, buf[PAD:PAD + nbytes], workgroups)
    torch.cuda.current_stream().synchronize()
    out = buf.cpu().numpy()
    assert (out[:PAD] == S8).all() and (out[PAD + nbytes:] == S8).all(), (workgroups, nbytes)
    return out[PAD:PAD + nbytes]


@pytest.mark.parametrize("workgroups", pfi.PULL_WORKGROUPS)
def test_pull_copy_every_unit_count_and_tail(dev, workgroups):
    for n16 in pfi.pull_units(workgroups):
        for tail in pfi.PULL_TAILS:
            if n16 == 0 and tail == 0:
                continue
            src = pfi.pull_source(n16 * 16 + tail)
            assert np.array_equal(_pull(dev, src, workgroups), src), (workgroups, n16, tail)


def test_pull_copy_1024_workgroups_and_no_bytes(dev):
    ops, abi = _api()
    wg = pfi.PULL_BIG_WORKGROUPS
    src = pfi.pull_source((4 * pfi.THREADS * wg + 1) * 16)
    assert np.array_equal(_pull(dev, src, wg), src)
    host = torch.from_numpy(pfi.pull_source(64)).pin_memory()
    buf = torch.full((64,), S8, dtype=torch.uint8, device=dev)
    assert abi.lib().avs_pull_copy_u8(host.data_ptr(), ops._p(buf), 0, 4, ops._stream()) == 0
    torch.cuda.current_stream().synchronize()
    assert (buf == S8).all()


def test_pull_copy_refusals(dev):
    ops, abi = _api()
    host = torch.from_numpy(pfi.pull_source(80)).pin_memory()
    buf = torch.full((128,), S8, dtype=torch.uint8, device=dev)
    for wg in (0, pfi.PULL_MAX_WORKGROUPS + 1):
        with pytest.raises(abi.AvsError, match=f"status {SHAPE}"):
            ops.pull_copy(host[:64], buf[:64], wg)
    with pytest.raises(ValueError, match="pinned"):
        ops.pull_copy(torch.from_numpy(pfi.pull_source(64)), buf[:64], 4)          # a pageable source
    with pytest.raises(ValueError, match="same byte size"):
        ops.pull_copy(host[:64], buf[:48], 4)
    # (refused by the library's alignment check, or already by the wrapper where torch does not report a slice as pinned)
    with pytest.raises((abi.AvsError, ValueError), match=f"status {ALIGN}|pinned"):
        ops.pull_copy(host[1:65], buf[:64], 4)                                      # a source sliced to a misaligned offset
    with pytest.raises(abi.AvsError, match=f"status {ALIGN}"):
        ops.pull_copy(host[:64], buf[8:72], 4)
    torch.cuda.synchronize()
    assert (buf == S8).all()
