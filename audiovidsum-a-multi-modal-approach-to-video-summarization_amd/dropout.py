"""Counter-based Dropout for a ragged batch of videos: the launch wrappers of libavsum_dropout.so
(include/avsum_dropout.h - its comment is the definition), the same definition restated on the host in numpy, and the
little host state a training run keeps.

Every element of a mask is a pure function of (seed, sample id of its video, branch, row inside the video, column):

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (column >> 2, row, sample & 0xffffffff, (((sample >> 32) << 1) | branch) & 0xffffffff)
    word    = word (column & 3) of Philox4x32-10(counter, key)
    m       = scale(p) if word >= threshold(p) else 0

so a video has the same mask alone and in any batch, the backward computes it again instead of keeping it, a run is
replayed from three integers, and a test can name a mask before any kernel has run.  Branch 0 is the visual branch of
AVBiLSTMModel, branch 1 the audio branch.

    keep_mask(...)   the multipliers as a tensor [R, cols]                (avsd_keep_mask_f32)
    apply(x, ...)    x * m, bit for bit ops.mul(x, keep_mask(...))        (avsd_dropout_fwd_f32)
    relu_bwd(...)    bit for bit ops.relu_dropout_bwd(dy, relu_out, keep_mask(...))   (avsd_relu_dropout_bwd_f32)

``samples`` of the wrappers: an int - video v of the batch has the id samples + v, nothing is uploaded - or an int64
device tensor [V] (sample_table() validates host ids and uploads them once; a host list of V ids is taken too, and
uploaded by every call that gets it).  ``offsets``: an ops.SeqTable, or the
int64 device tensor [V + 1] of one (SeqTable.offsets_t), which the caller has validated.  Host tensors are refused:
there is no CPU fallback.  numpy and torch are all this module imports; the library is loaded at the first launch.
"""
import numpy as np
import torch

__all__ = ["PHILOX_M0", "PHILOX_M1", "PHILOX_W0", "PHILOX_W1", "philox4x32_10", "threshold", "scale", "keep_mask_host",
           "sample_table", "Draw", "keep_mask", "apply", "relu_bwd", "CounterDropout"]

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57     # Salmon et al., SC'11
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF
_U32 = np.uint64(_MASK32)
_SHIFT32 = np.uint64(32)


# --------------------------------------------------------------------------- the definition, on the host
def philox4x32_10(counter, key, rounds=10, m0=PHILOX_M0, m1=PHILOX_M1, w0=PHILOX_W0, w1=PHILOX_W1, swap_hi_lo=False):
    """Philox4x32-10, vectorised: ``counter`` [..., 4] and ``key`` [..., 2] hold 32-bit words (any integer dtype; they
    broadcast against each other); returns uint32 [..., 4].  The keyword arguments exist for the tests, which plant a
    mistake (nine rounds, swapped multipliers, hi and lo exchanged, a key that does not advance: w0 = w1 = 0) and
    expect a known-answer vector to catch it."""
    counter = np.asarray(counter).astype(np.uint64) & _U32
    key = np.asarray(key).astype(np.uint64) & _U32
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape) for i in range(2))
    m0, m1, w0, w1 = (np.uint64(x) for x in (m0, m1, w0, w1))
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> _SHIFT32, p0 & _U32, p1 >> _SHIFT32, p1 & _U32
        if swap_hi_lo:
            hi0, lo0, hi1, lo1 = lo0, hi0, lo1, hi1
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + w0) & _U32, (k1 + w1) & _U32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _probability(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"the Dropout probability must lie in [0, 1), got {p}")
    return p


def threshold(p):
    """thr = floor(p * 2^32) in float64: an element is kept iff its 32-bit word is >= thr."""
    return int(np.floor(np.float64(_probability(p)) * np.float64(2.0 ** 32)))


def scale(p):
    """The multiplier of a kept element, 1.0f / (1.0f - (float)p), as a Python float that holds the fp32 value."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(_probability(p))))


def _seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"the Dropout seed must be an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def _branch(branch):
    if isinstance(branch, bool) or branch not in (0, 1):
        raise ValueError(f"branch must be 0 (visual) or 1 (audio), got {branch!r}")
    return int(branch)


def _sample_ids(samples, nseq, what):
    """Host ids of ``nseq`` videos as int64 [nseq]: an int is the first of nseq consecutive ids; a sequence holds one
    id per video.  Every id is an integer in [0, 2^63)."""
    if isinstance(samples, (int, np.integer)) and not isinstance(samples, bool):
        ids = [int(samples) + v for v in range(nseq)]
    else:
        ids = list(np.asarray(samples).reshape(-1).tolist()) if isinstance(samples, np.ndarray) else list(samples)
        if len(ids) != nseq:
            raise ValueError(f"{what}: {len(ids)} sample ids for {nseq} videos")
    for s in ids:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < 1 << 63:
            raise ValueError(f"{what}: a sample id must be an integer in [0, 2^63), got {s!r}")
    return np.array([int(s) for s in ids], dtype=np.int64)


def _host_offsets(offsets, what):
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if off.size < 2 or off[0] != 0 or (np.diff(off) <= 0).any():
        raise ValueError(f"{what}: offsets must hold V + 1 >= 2 entries, start at 0 and increase strictly")
    return off


def keep_mask_host(seed, p, samples, branch, offsets, cols):
    """The multipliers of one branch for the ragged batch ``offsets`` (host int64 [V + 1]) as numpy fp32 [R, cols]:
    the definition, evaluated on the host.  ``samples``: an int (video v has the id samples + v) or V ids."""
    what = "keep_mask_host"
    seed, branch, thr, mult = _seed(seed), _branch(branch), threshold(p), np.float32(scale(p))
    off = _host_offsets(offsets, what)
    ids = _sample_ids(samples, off.size - 1, what).astype(np.uint64)
    cols = int(cols)
    if cols < 0 or cols % 4:
        raise ValueError(f"{what}: cols must be a non-negative multiple of 4, got {cols}")
    rows = int(off[-1])
    video = np.repeat(np.arange(off.size - 1), np.diff(off))
    local = (np.arange(rows, dtype=np.int64) - off[video]).astype(np.uint64)
    counter = np.empty((rows, cols // 4, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(cols // 4, dtype=np.uint64)[None, :]
    counter[..., 1] = local[:, None]
    counter[..., 2] = (ids[video] & _U32)[:, None]
    counter[..., 3] = ((((ids[video] >> _SHIFT32) << np.uint64(1)) | np.uint64(branch)) & _U32)[:, None]
    words = philox4x32_10(counter, np.array([seed & _MASK32, seed >> 32], dtype=np.uint64)).reshape(rows, cols)
    return np.where(words >= np.uint32(thr), mult, np.float32(0.0)).astype(np.float32)


# --------------------------------------------------------------------------- launches
class Draw:
    """What names the masks of one forward / backward pair without holding them: ``seed``, ``p`` and ``samples`` (an
    int: the first of V consecutive ids; or the int64 device tensor [V] of sample_table()).  ScorerTrainFunction is
    handed one in place of the two mask tensors."""

    __slots__ = ("seed", "p", "samples")

    def __init__(self, seed, p, samples):
        self.seed, self.p, self.samples = _seed(seed), _probability(p), samples

    def __repr__(self):
        return f"Draw(seed={self.seed}, p={self.p}, samples={self.samples!r})"


def sample_table(samples, nseq, device):
    """Host sample ids of ``nseq`` videos, validated (integers in [0, 2^63), one per video) and uploaded once: the int64
    device tensor [nseq] the wrappers take as ``samples``."""
    return torch.from_numpy(_sample_ids(samples, int(nseq), "sample_table")).to(device)


def _abi():
    from . import _dropout_abi
    return _dropout_abi


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _operand(x, name, what, rows=None, cols=None, device=None):
    """An fp32 device operand [rows, cols] with unit column stride (a column slice of a wider buffer is fine: the row
    stride travels with it).  Returns its row stride in elements."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what}: {name} must be a device tensor (there is no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"{what}: {name} must be float32 [rows, cols] with unit column stride, got {x.dtype} "
                         f"{list(x.shape)} strides {list(x.stride())}")
    if (rows is not None and x.shape[0] != rows) or (cols is not None and x.shape[1] != cols) or \
            (device is not None and x.device != device):
        raise ValueError(f"{what}: {name} must be [{rows}, {cols}] on {device}, got {list(x.shape)} on {x.device}")
    return x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def _batch_args(what, seed, p, samples, branch, offsets, rows, device):
    """The arguments every entry point shares, from d_offsets on."""
    from .ragged import SeqTable
    if isinstance(offsets, SeqTable):
        if offsets.device.type != "cuda" or offsets.device != device:
            raise ValueError(f"{what}: the offsets table is on {offsets.device}, the rows on {device}")
        if offsets.rows != rows:
            raise ValueError(f"{what}: the offsets end at {offsets.rows}, the operands have {rows} rows")
        offsets = offsets.offsets_t
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.dtype != torch.int64 or \
            offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 2 or offsets.device != device:
        raise ValueError(f"{what}: offsets must be an ops.SeqTable or a contiguous int64 device tensor [V + 1], V >= 1, "
                         f"on {device}")
    nseq = offsets.numel() - 1
    if isinstance(samples, (list, tuple, np.ndarray)):
        samples = sample_table(samples, nseq, device)       # host ids: validated, uploaded for this call
    if isinstance(samples, torch.Tensor):
        if not samples.is_cuda or samples.dtype != torch.int64 or samples.dim() != 1 or samples.numel() != nseq or \
                not samples.is_contiguous() or samples.device != device:
            raise ValueError(f"{what}: a samples tensor must be contiguous int64 [{nseq}] on {device} (sample_table() "
                             f"makes one)")
        base, table = 0, _ptr(samples)
    else:
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or \
                not 0 <= int(samples) <= (1 << 63) - nseq:
            raise ValueError(f"{what}: samples must be the int64 device tensor of sample_table() or the first of "
                             f"{nseq} consecutive ids in [0, 2^63), got {samples!r}")
        base, table = int(samples), None
    import ctypes
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return (_ptr(offsets), nseq, rows), (_seed(seed), threshold(p), scale(p), _branch(branch), base, table, stream)


def keep_mask(seed, p, samples, branch, offsets, cols=None, out=None):
    """The multipliers of one branch as an fp32 device tensor [R, cols].  ``out``: the buffer to write into (then cols
    is its width; a column slice of a wider buffer is fine, what lies outside it is left alone); otherwise ``offsets``
    must be an ops.SeqTable, which says how many rows to allocate."""
    what = "keep_mask"
    if out is None:
        from .ragged import SeqTable
        if not isinstance(offsets, SeqTable) or cols is None:
            raise ValueError(f"{what}: without out=, offsets must be an ops.SeqTable and cols given")
        out = torch.empty((offsets.rows, int(cols)), dtype=torch.float32, device=offsets.device)
    ldo = _operand(out, "out", what, cols=None if cols is None else int(cols))
    rows, cols = out.shape
    (off, nseq, rows), tail = _batch_args(what, seed, p, samples, branch, offsets, rows, out.device)
    abi = _abi()
    abi.check(abi.lib().avsd_keep_mask_f32(_ptr(out), ldo, off, nseq, rows, cols, *tail), "avsd_keep_mask_f32")
    return out


def apply(x, seed, p, samples, branch, offsets, out=None):
    """x * m for the fp32 device tensor x [R, cols]: Dropout's forward with inverted scaling.  ``out=x`` works in
    place."""
    what = "dropout.apply"
    ldx = _operand(x, "x", what)
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    ldo = _operand(out, "out", what, rows, cols, x.device)
    (off, nseq, rows), tail = _batch_args(what, seed, p, samples, branch, offsets, rows, x.device)
    abi = _abi()
    abi.check(abi.lib().avsd_dropout_fwd_f32(_ptr(x), ldx, _ptr(out), ldo, off, nseq, rows, cols, *tail),
              "avsd_dropout_fwd_f32")
    return out


def relu_bwd(dy, relu_out, seed, p, samples, branch, offsets, out=None):
    """relu_out > 0 ? dy * m : 0 for fp32 device tensors [R, cols]: the gradient gate of Linear -> ReLU -> Dropout with
    the mask computed again."""
    what = "dropout.relu_bwd"
    lddy = _operand(dy, "dy", what)
    rows, cols = dy.shape
    ldr = _operand(relu_out, "relu_out", what, rows, cols, dy.device)
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=dy.device)
    ldo = _operand(out, "out", what, rows, cols, dy.device)
    (off, nseq, rows), tail = _batch_args(what, seed, p, samples, branch, offsets, rows, dy.device)
    abi = _abi()
    abi.check(abi.lib().avsd_relu_dropout_bwd_f32(_ptr(dy), lddy, _ptr(relu_out), ldr, _ptr(out), ldo, off, nseq, rows,
                                                  cols, *tail), "avsd_relu_dropout_bwd_f32")
    return out


# --------------------------------------------------------------------------- the state of a run
class CounterDropout:
    """What a training run holds instead of a generator: ``seed``, ``p`` and the host integer ``next_sample``, the id
    the next video gets.  take(n) hands out n consecutive ids.  state() / load_state() are the three fields as a tuple,
    to be stored beside a checkpoint: it is no part of a model's state_dict()."""

    def __init__(self, seed, p=0.3, next_sample=0):
        self.seed, self.p = _seed(seed), _probability(p)
        self.next_sample = 0
        self._set_next(next_sample)

    def _set_next(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 1 << 63:
            raise ValueError(f"next_sample must be an integer in [0, 2^63], got {value!r}")
        self.next_sample = int(value)

    def take(self, n=1):
        """The first of ``n`` consecutive sample ids; the next call starts after them."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"take(n): n must be a positive integer, got {n!r}")
        first = self.next_sample
        if first + int(n) > 1 << 63:
            raise OverflowError("the sample ids are used up: 2^63 videos have been drawn")
        self.next_sample = first + int(n)
        return first

    def state(self):
        return (self.seed, self.p, self.next_sample)

    def load_state(self, state):
        seed, p, next_sample = state
        self.seed, self.p = _seed(seed), _probability(p)
        self._set_next(next_sample)

    def __repr__(self):
        return f"CounterDropout(seed={self.seed}, p={self.p}, next_sample={self.next_sample})"
