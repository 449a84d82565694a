"""Counter-based Dropout without a GPU: the host definition of avsum_amd.dropout (Philox4x32-10 against the Random123
known-answer vectors, the threshold, batch invariance of the masks), the binding derived from include/avsum_dropout.h,
the CounterDropout state, and the launch arithmetic the large GPU case of test_gpu_dropout.py relies on."""
import ctypes
import os
import re

import numpy as np
import pytest

from dropout_inputs import LARGE_COLS, OFFSETS, large_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's kat_vectors for philox4x32 with ten rounds: (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _misses(**planted):
    """How many of the known-answer vectors a generator with the planted mistake fails."""
    from avsum_amd.dropout import philox4x32_10
    return sum(philox4x32_10(np.array(c), np.array(k), **planted).tolist() != list(want) for c, k, want in KNOWN_ANSWERS)


def test_known_answer_vectors():
    from avsum_amd.dropout import philox4x32_10
    for counter, key, want in KNOWN_ANSWERS:
        got = philox4x32_10(np.array(counter), np.array(key))
        assert got.dtype == np.uint32 and got.tolist() == list(want)
    # vectorised: the three at once, counters and keys broadcast row by row
    got = philox4x32_10(np.array([c for c, _, _ in KNOWN_ANSWERS]), np.array([k for _, k, _ in KNOWN_ANSWERS]))
    assert got.tolist() == [list(w) for _, _, w in KNOWN_ANSWERS]


@pytest.mark.parametrize("planted", [
    dict(rounds=9),
    dict(m0=0xCD9E8D57, m1=0xD2511F53),      # the multipliers swapped
    dict(swap_hi_lo=True),
    dict(w0=0, w1=0),                        # the key never advances
], ids=["nine-rounds", "swapped-multipliers", "hi-lo-exchanged", "key-not-advanced"])
def test_planted_mistakes_are_caught(planted):
    assert _misses() == 0
    assert _misses(**planted) >= 1


def test_threshold_and_scale():
    from avsum_amd.dropout import scale, threshold
    assert threshold(0.3) == 0x4CCCCCCC and threshold(0) == 0 and threshold(0.5) == 1 << 31
    assert threshold(np.nextafter(1.0, 0.0)) < 1 << 32
    assert scale(0) == 1.0 and np.float32(scale(0.3)) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            threshold(bad)


def test_kept_count_is_pinned():
    """Seed 2024, sample 0, branch 0, 4096 rows x 512 columns, p = 0.3: 1 467 418 of 2 097 152 kept (0.69972, 0.89
    standard deviations from 0.7)."""
    from avsum_amd.dropout import keep_mask_host, scale
    mask = keep_mask_host(2024, 0.3, 0, 0, [0, 4096], 512)
    assert mask.dtype == np.float32 and mask.shape == (4096, 512)
    assert int((mask != 0).sum()) == 1467418
    assert set(np.unique(mask).tolist()) == {0.0, scale(0.3)}
    assert (keep_mask_host(2024, 0.0, 0, 0, [0, 7], 8) == 1.0).all()


def test_masks_do_not_depend_on_batching():
    from avsum_amd.dropout import keep_mask_host
    samples = [5, 6, 7, 8]
    for branch in (0, 1):
        whole = keep_mask_host(11, 0.3, samples, branch, OFFSETS, 32)
        alone = [keep_mask_host(11, 0.3, [s], branch, [0, hi - lo], 32)
                 for s, lo, hi in zip(samples, OFFSETS[:-1], OFFSETS[1:])]
        assert np.array_equal(whole, np.concatenate(alone))
        assert np.array_equal(whole, keep_mask_host(11, 0.3, 5, branch, OFFSETS, 32))     # consecutive ids by base
    # a narrower mask is the left part of a wider one: the column enters through (c >> 2, c & 3) only
    assert np.array_equal(keep_mask_host(11, 0.3, samples, 0, OFFSETS, 64)[:, :32],
                          keep_mask_host(11, 0.3, samples, 0, OFFSETS, 32))


def test_every_input_changes_the_mask():
    from avsum_amd.dropout import keep_mask_host
    base = keep_mask_host(11, 0.3, [5], 0, [0, 16], 32)
    assert not np.array_equal(base, keep_mask_host(12, 0.3, [5], 0, [0, 16], 32))               # seed, low word
    assert not np.array_equal(base, keep_mask_host(11 + (1 << 32), 0.3, [5], 0, [0, 16], 32))   # seed, high word
    assert not np.array_equal(base, keep_mask_host(11, 0.3, [5], 1, [0, 16], 32))               # branch
    assert not np.array_equal(base, keep_mask_host(11, 0.3, [6], 0, [0, 16], 32))               # sample
    three, far = (keep_mask_host(11, 0.3, [s], 0, [0, 16], 32) for s in (3, 2 ** 32 + 3))
    assert not np.array_equal(three, far)                                                       # sample, high word
    assert not np.array_equal(base[0], base[1])                                                 # row
    for bad in ([-1], [1 << 63], [1.0], [True]):
        with pytest.raises(ValueError):
            keep_mask_host(11, 0.3, bad, 0, [0, 16], 32)
    with pytest.raises(ValueError):
        keep_mask_host(11, 0.3, [1, 2], 0, [0, 16], 32)                                          # one id per video
    with pytest.raises(ValueError):
        keep_mask_host(11, 0.3, [1], 0, [0, 16], 30)                                             # cols % 4


def test_binding_is_derived_from_the_header():
    from avsum_amd import _dropout_abi as abi
    text = open(os.path.join(ROOT, "include", "avsum_dropout.h")).read()
    declared = set(re.findall(r"\b(avsd_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    assert declared == set(abi.declared_symbols()) == set(abi._SIGNATURES)
    assert {"avsd_keep_mask_f32", "avsd_dropout_fwd_f32", "avsd_relu_dropout_bwd_f32"} <= declared
    assert abi.ABI_VERSION == int(re.search(r"#define\s+AVSD_ABI_VERSION\s+(\d+)", text).group(1))
    assert abi.VEC == 4 and abi.SHARED["AVSD_OK"] == 0
    lib = abi.lib()                                    # loads without a GPU; every prototype is bound with its types
    assert lib.avsd_abi_version() == abi.ABI_VERSION
    for name, (res, args) in abi._SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    res, args = abi._SIGNATURES["avsd_keep_mask_f32"]
    assert res is ctypes.c_int and args[6] is ctypes.c_uint64 and args[7] is ctypes.c_uint and args[8] is ctypes.c_float


def test_module_imports_numpy_and_torch_only():
    import avsum_amd.dropout as d
    src = open(d.__file__).read()
    top = re.findall(r"^(?:import|from)\s+(\S+)", src, flags=re.M)
    assert sorted(top) == ["numpy", "torch"]


def test_counter_dropout_state():
    from avsum_amd.dropout import CounterDropout
    c = CounterDropout(77)
    assert c.state() == (77, 0.3, 0)
    assert c.take(1) == 0 and c.take(8) == 1 and c.take() == 9 and c.next_sample == 10
    saved = c.state()
    assert c.take(3) == 10
    d = CounterDropout(1, 0.5)
    d.load_state(saved)
    assert d.state() == saved == (77, 0.3, 10) and d.take(3) == 10
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            c.take(bad)
    for bad in (-1, 1 << 64, 1.0, None):
        with pytest.raises(ValueError):
            CounterDropout(bad)
    with pytest.raises(ValueError):
        CounterDropout(1, 1.0)
    with pytest.raises(ValueError):
        d.load_state((1, 0.3, -5))
    with pytest.raises(OverflowError):
        CounterDropout(1, 0.3, (1 << 63) - 2).take(3)


def test_large_gpu_case_reaches_the_second_grid_stride_trip():
    from avsum_amd import _dropout_abi as abi
    off = large_offsets()
    lengths = np.diff(off)
    assert len(lengths) == 300 and lengths.min() == 1 and lengths.max() == 39
    items = int(off[-1]) * LARGE_COLS // abi.VEC
    resident = abi.BLOCK * abi.MAX_GROUPS
    assert resident < items <= 2 * resident          # some threads take a second item, none a third


def test_refusals_before_any_launch():
    """Every refusal of the host side comes back as a status with a message, before any HIP call (no GPU here)."""
    from avsum_amd import _dropout_abi as abi
    lib, C = abi.lib(), abi.SHARED
    fake = 4096    # a non-null, 16-byte aligned "pointer" that is never dereferenced on the paths below
    tail = (2024, 0x4CCCCCCC, 1.0, 0, 0, None, None)   # seed, thr, scale, branch, sample_base, d_samples, stream

    def mask(out=fake, ldo=32, off=fake, nseq=2, rows=8, cols=32, tail=tail):
        return lib.avsd_keep_mask_f32(out, ldo, off, nseq, rows, cols, *tail)

    def message():
        return lib.avsd_last_error().decode()

    assert mask(cols=30) == C["AVSD_E_SHAPE"] and "multiple of 4" in message()
    assert mask(ldo=28) == C["AVSD_E_SHAPE"] and "row stride" in message()            # below cols
    assert mask(ldo=34) == C["AVSD_E_SHAPE"] and "row stride" in message()            # no multiple of 4
    assert mask(out=fake + 4) == C["AVSD_E_ALIGN"] and "16-byte" in message()
    assert mask(off=fake + 4) == C["AVSD_E_ALIGN"]
    assert mask(nseq=abi.MAX_SEQ + 1) == C["AVSD_E_ARG"] and "nseq" in message()
    assert mask(nseq=0) == C["AVSD_E_ARG"]
    assert mask(out=None) == C["AVSD_E_ARG"] and "null" in message()
    assert mask(off=None) == C["AVSD_E_ARG"] and "null" in message()
    assert mask(rows=-1) == C["AVSD_E_SHAPE"] and "negative" in message()
    assert mask(cols=-4) == C["AVSD_E_SHAPE"] and "negative" in message()
    assert mask(rows=abi.MAX_ROWS + 1) == C["AVSD_E_SHAPE"]
    assert mask(tail=(1, 2, 1.0, 2, 0, None, None)) == C["AVSD_E_ARG"] and "branch" in message()
    assert mask(tail=(1, 2, 1.0, 0, -1, None, None)) == C["AVSD_E_ARG"] and "sample" in message()
    assert mask(tail=(1, 2, 1.0, 0, (1 << 63) - 1, None, None)) == C["AVSD_E_ARG"]      # the second video's id: 2^63
    assert mask(tail=(1, 2, 1.0, 0, 0, fake + 4, None)) == C["AVSD_E_ALIGN"]
    # the two other entry points check every operand of theirs
    fwd, bwd = lib.avsd_dropout_fwd_f32, lib.avsd_relu_dropout_bwd_f32
    assert fwd(None, 32, fake, 32, fake, 2, 8, 32, *tail) == C["AVSD_E_ARG"]
    assert fwd(fake, 28, fake, 32, fake, 2, 8, 32, *tail) == C["AVSD_E_SHAPE"]
    assert fwd(fake, 32, fake + 8, 32, fake, 2, 8, 32, *tail) == C["AVSD_E_ALIGN"]
    assert bwd(fake, 32, None, 32, fake, 32, fake, 2, 8, 32, *tail) == C["AVSD_E_ARG"]
    assert bwd(fake, 32, fake, 30, fake, 32, fake, 2, 8, 32, *tail) == C["AVSD_E_SHAPE"]
    assert bwd(fake, 32, fake, 32, fake + 4, 32, fake, 2, 8, 32, *tail) == C["AVSD_E_ALIGN"]
    # nothing to do is no error, and launches nothing
    assert mask(rows=0) == C["AVSD_OK"] and mask(cols=0, ldo=0) == C["AVSD_OK"]
