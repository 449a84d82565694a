"""Host plans of the ragged-batch layers: row offsets validated on the host and uploaded once (RaggedOffsets and the
nine tables built on it - EvalTables, SeqTable, AttnTable, ShotTables, StageOneTables, SummaryTables, KtsTables,
RankTables, RenderTables) and the
pair tables of the batched fusion (FusionTables).
Pure host code on numpy and torch: nothing here touches the kernel library, so the plans can be built and checked with
``device="cpu"`` where there is no GPU.  ops.py re-exports every name and holds the launch wrappers that take them."""
import numpy as np
import torch

from ._attn_abi import load_header as _load_attn_header   # (the header's reader only: the library is not loaded here)
from ._header import load as _load_header
from ._loss_abi import load_header as _load_loss_header   # (again the reader only)
from ._render_abi import load_header as _load_render_header   # (again the reader only)
from .features.kts import KTS_MAX_SAMPLES, kts_penalties   # (pure numpy: the limit and the penalty of the definitions)

# The sizes the tables below share with the kernels that read them are the header's (include/avsum_hip.h, where each is
# described), never a second copy.
_H = _load_header().constants
FUSION_MAX_N = _H["AVS_FUSION_MAX_N"]        # 6400: rows of the visual side of one pair (the per-pair limit of dtw_path)
FUSION_SMALL_L = _H["AVS_FUSION_SMALL_L"]    # 64, 512: size classes by l = min(n, m) - one wave per pair (four pairs per
FUSION_MID_L = _H["AVS_FUSION_MID_L"]        # workgroup), one 256-thread workgroup per pair, above that 1024 threads
_FUSION_TILE = _H["AVS_FUSION_TILE"]         # 32: the cost kernel's output tile
_FUSION_PAIR_COLS = _H["AVS_FUSION_PAIR_COLS"]   # 8: int64 per row of the pair table

EVAL_MAX_T = _H["AVS_EVAL_MAX_T"]            # 32768: rows of one video
EVAL_TILE = _H["AVS_EVAL_TILE"]              # 256: rows of a video per workgroup of the pair-count kernel
EVAL_CHUNK = _H["AVS_EVAL_CHUNK"]            # 1024: columns it stages through LDS per step
EVAL_COLS = _H["AVS_EVAL_COLS"]              # 10: int64 per video of the fold (ops.EVAL_COLUMNS names them)

SHOT_INTERVAL = _H["AVS_SHOT_INTERVAL"]      # 3 (features/extractors.py FRAME_INTERVAL): the sampled frames are its multiples,
SHOT_MAX_FRAMES = _H["AVS_SHOT_MAX_FRAMES"]  # 100 (MAX_FRAMES): at most that many per shot,
SHOT_MICRO_BATCH = _H["AVS_SHOT_MICRO_BATCH"]    # 4 (MICRO_BATCH): in BatchNorm groups of 4 with a shorter tail group

SUMMARY_MAX_CAPACITY = _H["AVS_SUMMARY_MAX_CAPACITY"]   # 8191: knapsack cells 0 .. capacity, both fp64 rows LDS-resident
SUMMARY_MAX_ROWS = 1024       # score rows of one knapsack batch (grid y).  The take-bit workspace holds rows * shot_cap *
                              # words uint64 entries with words <= 128: below 2^31 for every shot_cap below 2^14 = 16 384
                              # at the full 1024 rows and 8191 cells; past that the wrapper refuses by take_words itself

# KTS_MAX_SAMPLES (2048, from features/kts.py): samples of one video - the two fp64 rows of the dynamic programme live in LDS
KTS_TILE = _H["AVS_KTS_TILE"]                # 64: rows and columns of a Gram tile
KTS_MAX_VIDEOS = _H["AVS_KTS_MAX_VIDEOS"]    # 65535: videos of one batch (a grid dimension)
_KTS_VIDEO_COLS = _H["AVS_KTS_VIDEO_COLS"]   # 10: int64 per row of the video table

# include/avsum_attn.h: the tile sizes of the ragged-batch attention kernels
_HA = _load_attn_header().constants
ATTN_FWD_TILE = _HA["AVSA_FWD_TILE"]         # 128: queries of a forward workgroup
ATTN_BWD_TILE = _HA["AVSA_BWD_TILE"]         # 32: keys of a dK/dV workgroup = queries of a dQ workgroup
_ATTN_TILE_COLS = _HA["AVSA_TILE_COLS"]      # 2: int32 per row of a tile table
_ATTN_MAX_ROWS = _HA["AVSA_MAX_ROWS"]        # 2^31 - 1: the last offset at most

# include/avsum_loss.h: the tile of the pairwise ranking loss and its limits
_HL = _load_loss_header().constants
RANK_TILE = _HL["AVSL_TILE"]                 # 256: rows of a video per workgroup of the pair kernel
RANK_MAX_T = _HL["AVSL_MAX_T"]               # 32768: rows of one video (pair counts: < 2^30 per row, < 2^31 per video)
_RANK_TILE_COLS = _HL["AVSL_TILE_COLS"]      # 2: int32 per row of the tile table

# include/avsum_render.h: the tile of the summary index and its limits
_HR = _load_render_header().constants
RENDER_TILE = _HR["AVSR_TILE"]               # 1024: frames of a video per workgroup of the summary index
RENDER_MAX_FRAMES = _HR["AVSR_MAX_FRAMES"]   # 2^24: frames of one batch
_RENDER_TILE_COLS = _HR["AVSR_TILE_COLS"]    # 2: int32 per row of the tile table


def exclusive_offsets(lengths):
    """int64 [len + 1]: the exclusive prefix sums of ``lengths`` and, last, their total."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    out = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=out[1:])
    return out


def segment_tiles(per):
    """Segment p owns per[p] tiles: (segment, k) int64 [sum(per)] each, k counting 0 .. per[segment] - 1."""
    per = np.asarray(per, dtype=np.int64).reshape(-1)
    segment = np.repeat(np.arange(per.size, dtype=np.int64), per)
    k = np.arange(segment.size, dtype=np.int64) - np.repeat(exclusive_offsets(per)[:-1], per)
    return segment, k


def _upload(device, *arrays):
    """The numpy ``arrays`` as tensors on ``device``: None = the current HIP device, "cpu" = they stay on the host."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    return [torch.from_numpy(a).to(device) for a in arrays]


def _bound(n):
    return f"2^{n.bit_length() - 1}" if n & (n - 1) == 0 else str(n)


class RaggedOffsets:
    """Row offsets [V + 1] of a ragged batch of V segments (segment v is rows offsets[v] .. offsets[v + 1] of the
    concatenated rows), validated on the host and uploaded ONCE.

    Host side (numpy int64): ``offsets``, ``lengths``; ``count`` (V), ``total`` (= offsets[-1]) and ``max_len`` (0 for
    an empty batch).  Device side: ``offsets_t`` int64 [V + 1] on ``device`` (None: the current HIP device; "cpu": it
    stays on the host).  ``what`` starts every message.  The rules, each refused with a ValueError: ``zero_start`` (the
    first offset is 0, else only non-negative), ``allow_empty`` (a lone [0] for V = 0), ``min_length`` / ``max_length``
    of a segment, ``max_total`` for the last offset (``total_inclusive``: it may be reached) and ``rows`` (what the last
    offset must equal; None: wherever the offsets end).  Decreasing offsets and a device tensor are always refused:
    the offsets are a host array."""

    def __init__(self, offsets_host, what, *, device=None, zero_start=True, allow_empty=False, min_length=1,
                 max_length=None, max_total=1 << 31, total_inclusive=False, rows=None):
        if isinstance(offsets_host, torch.Tensor):
            if offsets_host.is_cuda:
                raise ValueError(f"{what}: the offsets are a HOST array (they are validated before the upload)")
            offsets_host = offsets_host.numpy()
        off = np.array(offsets_host, dtype=np.int64).reshape(-1)
        if off.size < (1 if allow_empty else 2):
            raise ValueError(f"{what}: offsets must hold V + 1 entries" + (" (a single 0 for an empty batch)"
                             if allow_empty else " for V >= 1 videos (the batch is empty)"))
        if off[0] < 0:
            raise ValueError(f"{what}: negative row offset")
        if zero_start and off[0] != 0:
            raise ValueError(f"{what}: offsets must start at 0, got {int(off[0])}")
        t = np.diff(off)
        shortest, longest = (int(t.min()), int(t.max())) if t.size else (min_length, 0)
        if shortest < 0:
            raise ValueError(f"{what}: the offsets decrease")
        total = int(off[-1])
        if rows is not None and total != rows:
            raise ValueError(f"{what}: the offsets end at {total}, the batch has {int(rows)} rows")
        if total > max_total or (total == max_total and not total_inclusive):
            raise ValueError(f"{what}: {total} rows, the kernels take {'at most' if total_inclusive else 'fewer than'} "
                             f"{_bound(max_total)}")
        if shortest < min_length:
            raise ValueError(f"{what}: a video has {shortest} rows, it needs at least {min_length} (the offsets "
                             "must increase)")
        if max_length is not None and longest > max_length:
            raise ValueError(f"{what}: a video has {longest} rows, above the limit {max_length}")
        self.offsets, self.lengths, self.count, self.total, self.max_len = off, t, int(t.size), total, longest
        self.offsets_t, = _upload(device, off)
        self.device = self.offsets_t.device


class EvalTables(RaggedOffsets):
    """The host plan of one batch layout for eval_counts, built once from the host row offsets [V + 1] of the videos
    in the concatenated score vectors (video v is rows offsets[v] .. offsets[v + 1]).

    Host side (numpy): ``offsets``, ``lengths``, ``nvideos``, ``rows`` (= offsets[-1], the rows the vectors must have),
    ``max_t``, ``tiles`` int32 [ntiles, 2] = (video, row tile of 256 rows), ``ntiles``.  Device side: ``offsets_t``
    int64 [V + 1], ``tiles_t``.  ``device="cpu"`` keeps everything on the host (the builder can be checked without a
    GPU).  Refused, each with a ValueError: a video shorter than 2 rows (no pair to rank) or longer than 32768 (the
    int64-exact limit), decreasing or negative offsets, 2^31 rows or more.  The first video may start after row 0 and
    the batch may be empty ([0])."""

    def __init__(self, offsets_host, device=None):
        super().__init__(offsets_host, "eval_counts", device=device, zero_start=False, allow_empty=True, min_length=2,
                         max_length=EVAL_MAX_T)
        self.nvideos, self.rows, self.max_t = self.count, self.total, self.max_len
        self.tiles = np.stack(segment_tiles(-(-self.lengths // EVAL_TILE)), 1).astype(np.int32).reshape(-1, 2)
        self.ntiles = self.tiles.shape[0]
        self.tiles_t, = _upload(self.device, self.tiles)


class SeqTable(RaggedOffsets):
    """Row offsets of a ragged batch of V videos for the batched training step: ``offsets`` / ``lengths`` (numpy
    int64), ``nseq``, ``rows``, ``max_t`` and the device copy ``offsets_t`` int64 [V + 1] that the recurrences,
    seq_shift_rows and seq_mse read.  ``rows``: the row count the offsets must end at (None: wherever they end).
    Refused with a ValueError: fewer than one video, offsets that do not start at 0, an empty video (offsets must
    increase strictly), a last offset other than ``rows``, 2^31 rows or more.  ``device="cpu"`` keeps the table on the
    host (the builder is checked without a GPU)."""

    def __init__(self, offsets_host, rows=None, device=None):
        super().__init__(offsets_host, "SeqTable", device=device, rows=rows)
        self.nseq, self.rows, self.max_t = self.count, self.total, self.max_len


class AttnTable(RaggedOffsets):
    """The host plan of one batch layout for the ragged-batch attention (attn.mhsa_rows_fwd / mhsa_rows_bwd,
    MultiHeadSelfAttention.forward_rows), built once from the host row offsets [V + 1] of the sequences in the
    concatenated projections (sequence v is rows offsets[v] .. offsets[v + 1]).

    Host side (numpy): ``offsets``, ``lengths`` (int64), ``nseq``, ``first_row`` (= offsets[0]: the first sequence may
    start after row 0), ``rows`` (= offsets[-1]: the buffers need at least that many rows), ``max_t``; ``fwd_tiles``
    int32 [n_fwd, 2] = (sequence, tile of 128 queries) for the forward and ``bwd_tiles`` int32 [n_bwd, 2] = (sequence,
    tile of 32) for the two gradient kernels, whose query tiles and key tiles are the same table - every sequence's
    tiles 0 .. ceil(T_v / tile) - 1, sequence after sequence.  Device side: ``offsets_t`` int64 [V + 1], ``fwd_tiles_t``,
    ``bwd_tiles_t``, uploaded once.  ``device="cpu"`` keeps everything on the host (the builder can be checked without
    a GPU or the library).  Refused, each with a ValueError: an empty batch, an empty sequence (the offsets must
    increase strictly), negative or decreasing offsets, 2^31 rows or more.  uniform(b, t) is the table of a dense
    [b, t] batch."""

    def __init__(self, offsets_host, device=None):
        super().__init__(offsets_host, "AttnTable", device=device, zero_start=False, max_total=_ATTN_MAX_ROWS,
                         total_inclusive=True)
        self.nseq, self.first_row, self.rows, self.max_t = self.count, int(self.offsets[0]), self.total, self.max_len
        self.fwd_tiles, self.bwd_tiles = (
            np.stack(segment_tiles(-(-self.lengths // tile)), 1).astype(np.int32).reshape(-1, _ATTN_TILE_COLS)
            for tile in (ATTN_FWD_TILE, ATTN_BWD_TILE))
        self.n_fwd, self.n_bwd = self.fwd_tiles.shape[0], self.bwd_tiles.shape[0]
        self.fwd_tiles_t, self.bwd_tiles_t = _upload(self.device, self.fwd_tiles, self.bwd_tiles)

    @classmethod
    def uniform(cls, b, t, device=None):
        """The table of ``b`` sequences of ``t`` rows each, from row 0."""
        return cls(np.arange(int(b) + 1, dtype=np.int64) * int(t), device=device)


class ShotTables(RaggedOffsets):
    """The host plan of one batch layout for the batched shot detector, built once from the host frame offsets [V + 1]
    of the videos in the concatenated frames (video v is frames offsets[v] .. offsets[v + 1]) and ``min_scene_len``.

    Host side (numpy): ``offsets``, ``lengths``, ``nvideos``, ``frames`` (= offsets[-1]), ``min_scene_len``, ``cut_off``
    int64 [V + 1] (video v's slot of the cut buffer: (n_v - 1) // min_scene_len entries, the most the greedy rule can
    place) and the capacities, all from the offsets alone: ``cut_cap``, ``shot_cap`` = sum of (slot + 1), ``sample_cap``
    = sum of ceil(n_v / 3) (the shots of a video tile it, so they hold at most its multiples of 3) and ``group_cap`` =
    sum of (ceil(n_v / 3) // 4 + slot + 1) (sum of ceil(c / 4) <= (F + 3 S) / 4 <= F // 4 + S in integers);
    ``packed_sizes``: the entries of the five parts of ops.shot_tables' one int64 buffer - counts, per-video offsets,
    shots, sample offsets, group offsets - at those capacities.  Device side: ``offsets_t``, ``cut_off_t``.
    ``device="cpu"`` keeps everything on the host (the builder can be checked without a GPU).  Refused, each with a
    ValueError: an empty batch, offsets that do not start at 0 or do not increase strictly (an empty video), more than
    2^24 frames (the frame is on grid x in workgroups of 256, and a launch holds fewer than 2^32 threads per grid
    dimension), min_scene_len < 1."""

    def __init__(self, offsets_host, min_scene_len=15, device=None):
        super().__init__(offsets_host, "ShotTables", device=device, max_total=1 << 24, total_inclusive=True)
        if int(min_scene_len) < 1:
            raise ValueError(f"ShotTables: min_scene_len must be >= 1, got {min_scene_len}")
        self.nvideos, self.frames, self.min_scene_len = self.count, self.total, int(min_scene_len)
        slots = (self.lengths - 1) // self.min_scene_len
        thirds = -(-self.lengths // SHOT_INTERVAL)
        self.cut_off = exclusive_offsets(slots)
        self.cut_cap = int(slots.sum())
        self.shot_cap = int((slots + 1).sum())
        self.sample_cap = int(thirds.sum())
        self.group_cap = int((thirds // SHOT_MICRO_BATCH + slots + 1).sum())
        self.packed_sizes = (4, 3 * (self.nvideos + 1), 2 * self.shot_cap, self.shot_cap + 1, self.group_cap + 1)
        self.cut_off_t, = _upload(self.device, self.cut_off)


class StageOneTables(RaggedOffsets):
    """The host plan of the batched stage-1 extraction (VisualFeatureExtractor.embed_shots), built once from the host
    frame offsets [V + 1] of the videos in the concatenated frames and one ``[(start, end)]`` shot list per video - any
    list AVProcessor.process_decoded takes: shots may overlap, ``end`` past the video is clipped to its length,
    ``start >= end`` is an empty shot, a video may have none.  from_result builds it from a detect_shots_batch result.

    Host side (numpy int64): ``offsets``, ``lengths``, ``nvideos``, ``frames``; ``shot_offsets`` [V + 1], ``shots``
    [S, 2] (video-relative, as given), ``shot_video`` [S], ``nshots``; ``sample_offsets`` [S + 1], ``sample_index`` [F]
    (rows of the concatenated frames, shot by shot: base[v] + sample_shot_indices(start, min(end, n_v))), ``nsamples``;
    ``group_offsets`` [G + 1]: per shot ceil(c / 4) BatchNorm groups of 4 with a shorter tail, never across two shots
    (for shots that tile the videos: the tables of features.shots.shot_tables_host).  The uniform sets: for each group
    size r of 4, 3, 2, 1 that occurs the sample positions of all frames in groups of r frames, in shot order, one set
    after another, are ``pass_order`` [F] (pass row -> sample position); ``row_of_sample`` [F] is its inverse,
    ``pass_frame_index`` = sample_index[pass_order] the source frame of every pass row, and ``passes`` the list of
    (group size, row_lo, row_hi) covering 0 .. F in order: each holds whole groups of ONE size and at most
    ``chunk_frames`` frames.  ``samples``: sample_offsets as the RaggedOffsets ops.segment_mean_perm checks.
    Device side: ``offsets_t``, ``pass_frame_index_t``, ``row_of_sample_t``, ``sample_offsets_t`` and ``pass_counts_t``
    [len(passes)] (hi - lo: the device row count ops.gather_rows reads), each uploaded once.  ``device="cpu"`` keeps
    everything on the host (the builder can be checked without a GPU).  Refused, each with a ValueError: what ShotTables
    refuses about the offsets (more than 2^24 frames among it), a list count other than V, a negative start,
    chunk_frames < 4."""

    def __init__(self, offsets_host, shots_per_video, chunk_frames=4096, device=None):
        super().__init__(offsets_host, "StageOneTables", device=device, max_total=1 << 24, total_inclusive=True)
        if int(chunk_frames) < SHOT_MICRO_BATCH:
            raise ValueError(f"StageOneTables: chunk_frames must be >= {SHOT_MICRO_BATCH}, got {chunk_frames}")
        shots_per_video = list(shots_per_video)
        if len(shots_per_video) != self.count:
            raise ValueError(f"StageOneTables: {len(shots_per_video)} shot lists for {self.count} videos")
        self.nvideos, self.frames, self.chunk_frames = self.count, self.total, int(chunk_frames)
        per_video = [np.asarray(list(s), dtype=np.int64).reshape(-1, 2) for s in shots_per_video]
        self.shot_offsets = exclusive_offsets([s.shape[0] for s in per_video])
        self.shots = np.concatenate(per_video).reshape(-1, 2)
        self.nshots = self.shots.shape[0]
        self.shot_video = np.repeat(np.arange(self.nvideos, dtype=np.int64), np.diff(self.shot_offsets))
        start, end = self.shots[:, 0], np.minimum(self.shots[:, 1], self.lengths[self.shot_video])
        if (start < 0).any():
            raise ValueError("StageOneTables: a shot starts at a negative frame")
        first = -(-start // SHOT_INTERVAL)                                     # ceil(start / 3)
        count = np.clip(-(-end // SHOT_INTERVAL) - first, 0, SHOT_MAX_FRAMES)   # (start >= end: no multiple of 3 between)
        self.samples = RaggedOffsets(exclusive_offsets(count), "StageOneTables: sample_offsets", device=self.device,
                                     allow_empty=True, min_length=0)
        self.sample_offsets, self.nsamples = self.samples.offsets, self.samples.total
        shot_of, k = segment_tiles(count)
        self.sample_index = self.offsets[self.shot_video[shot_of]] + SHOT_INTERVAL * (first[shot_of] + k)
        # group g of a shot holds its samples 4 g .. min(4 g + 4, c): the size of the group a sample lies in
        groups = -(-count // SHOT_MICRO_BATCH)
        gshot, g = segment_tiles(groups)
        self.group_offsets = np.concatenate([self.sample_offsets[:-1][gshot] + SHOT_MICRO_BATCH * g,
                                             [self.nsamples]]).astype(np.int64)
        size_of = np.minimum(SHOT_MICRO_BATCH, count[shot_of] - k // SHOT_MICRO_BATCH * SHOT_MICRO_BATCH)
        order, self.passes = [], []
        for r in range(SHOT_MICRO_BATCH, 0, -1):
            members = np.flatnonzero(size_of == r)
            row0, step = sum(o.size for o in order), self.chunk_frames // r * r
            self.passes += [(r, row0 + lo, row0 + min(lo + step, members.size)) for lo in range(0, members.size, step)]
            order.append(members)
        self.pass_order = np.concatenate(order).astype(np.int64)
        self.row_of_sample = np.empty(self.nsamples, dtype=np.int64)
        self.row_of_sample[self.pass_order] = np.arange(self.nsamples, dtype=np.int64)
        self.pass_frame_index = self.sample_index[self.pass_order]
        self.pass_counts = np.array([hi - lo for _, lo, hi in self.passes], dtype=np.int64)
        self.sample_offsets_t = self.samples.offsets_t
        self.pass_frame_index_t, self.row_of_sample_t, self.pass_counts_t = _upload(
            self.device, self.pass_frame_index, self.row_of_sample, self.pass_counts)

    @classmethod
    def from_result(cls, result, chunk_frames=4096):
        """The plan of a features.shots.ShotBatchResult (detect_shots_batch): its videos and the shots of its
        host_tables() - the result's one download - on the result's device."""
        t, plan = result.host_tables(), result.plan
        shots, off = t["shots"], t["shot_offsets"]
        return cls(plan.offsets, [shots[off[v]:off[v + 1]] for v in range(plan.nvideos)], chunk_frames, plan.device)


class SummaryTables(RaggedOffsets):
    """The host plan of one batch layout for the keyshot summaries (shot_value_sums, knapsack_batch,
    mask_overlap_counts), built once from the host frame offsets [V + 1] of the videos in the concatenated scores, the
    summary ``ratio`` and ``shot_cap``, the rows of the shot table the kernels will be given (an int, or a ShotTables
    whose shot_cap is taken).

    Host side (numpy): ``offsets``, ``lengths``, ``nvideos``, ``frames`` (= offsets[-1]), ``ratio``, ``capacity`` int64 [V]
    = int(floor(float64(n_v) * float64(ratio))), the frames a summary of video v may hold - computed HERE and never on
    the device - ``max_capacity``, ``shot_cap``, ``words`` = ceil((max_capacity + 1) / 64), the uint64 words of one
    shot's take bits, and take_words(k).  Device side: ``offsets_t``, ``capacity_t``.  ``device="cpu"`` keeps everything
    on the host (the builder can be checked without a GPU).  Refused, each with a ValueError: what ShotTables refuses
    about the offsets, a ratio that is not finite or lies outside (0, 1], a capacity above 8191 (the LDS-resident
    limit), shot_cap < 1."""

    def __init__(self, offsets_host, ratio=0.15, shot_cap=1, device=None):
        super().__init__(offsets_host, "SummaryTables", device=device, max_total=1 << 24, total_inclusive=True)
        ratio = float(ratio)
        if not (np.isfinite(ratio) and 0.0 < ratio <= 1.0):
            raise ValueError(f"SummaryTables: ratio must lie in (0, 1], got {ratio}")
        if isinstance(shot_cap, ShotTables):
            shot_cap = shot_cap.shot_cap
        if int(shot_cap) < 1:
            raise ValueError(f"SummaryTables: shot_cap must be >= 1, got {shot_cap}")
        self.nvideos, self.frames, self.ratio, self.shot_cap = self.count, self.total, ratio, int(shot_cap)
        self.capacity = np.floor(self.lengths.astype(np.float64) * np.float64(ratio)).astype(np.int64)
        over = np.flatnonzero(self.capacity > SUMMARY_MAX_CAPACITY)
        if over.size:
            v = int(over[0])
            raise ValueError(f"SummaryTables: video {v} has {int(self.lengths[v])} frames, a summary of "
                             f"{int(self.capacity[v])} frames at ratio {ratio}, above the LDS-resident limit "
                             f"{SUMMARY_MAX_CAPACITY}")
        self.max_capacity = int(self.capacity.max())
        self.words = (self.max_capacity + 1 + 63) // 64
        self.capacity_t, = _upload(self.device, self.capacity)

    def take_words(self, k):
        """uint64 entries of the take-bit workspace [k][shot_cap][words] of a knapsack batch of ``k`` score rows."""
        return int(k) * self.shot_cap * self.words


class KtsTables(RaggedOffsets):
    """The host plan of one batch layout for kernel temporal segmentation (kts_gram, kts_segment), built once from the
    host frame offsets [V + 1] of the videos in the concatenated feature rows, the subsampling ``stride``, ``ncp`` (the
    most change points tried: None = n - 1, an int, or one entry per video, None among them), ``vmax`` (the weight of
    cpd_auto's penalty) and ``lmin`` (the shortest segment, in samples).

    Host side (numpy): ``offsets``, ``lengths``, ``nvideos``, ``frames``; ``n`` int64 [V] = ceil(N_v / stride), the
    samples of a video (sample i is its row i * stride), ``max_n``; ``m_max`` int64 [V] = max(0, min(ncp, n // lmin -
    1)); ``k_offsets`` [V + 1], the exclusive sums of n^2: video v's [n, n] row-major block of the packed fp64 Gram
    buffer (``k_entries`` in all); ``k1_offsets`` over n + 1, ``jt_offsets`` over (n + 1)^2 and ``p_offsets`` over
    (m_max + 1)(n + 1): the blocks of K1, Jt[l][t] and p_k[l] in the workspace; ``cost_offsets`` over m_max + 1 and
    ``cost_cap`` = ``shot_cap`` = their total: the slots of the costs, the change points and the shots;
    ``penalties`` float64 [cost_cap] (kts_penalties per video); ``tiles`` int32 [ntiles, 3] = (video, ti, tj) with
    ti <= tj, the 64 x 64 tiles of the upper triangles; ``workspace_bytes`` (= avs_kts_workspace_bytes of the entries).
    Device side: ``offsets_t``, ``videos_t`` int64 [V, 10] (the per-video row of all of the above, the layout
    include/avsum_hip.h gives), ``tiles_t``, ``penalties_t``.  ``device="cpu"`` keeps everything on the host (the builder
    can be checked without a GPU).  Refused, each with a ValueError: what SeqTable refuses about the offsets, more than
    65535 videos, stride < 1, lmin < 1, a video of more than 2048 samples, ncp < 0 (or a list of another length than
    V), a vmax that is not finite or is <= 0, a packed size of 2^31 entries or more."""

    def __init__(self, video_offsets, stride=15, ncp=None, vmax=1.0, lmin=1, device=None):
        super().__init__(video_offsets, "KtsTables", device=device)
        if int(stride) < 1 or int(lmin) < 1:
            raise ValueError(f"KtsTables: stride and lmin must be >= 1, got stride = {stride}, lmin = {lmin}")
        vmax = float(vmax)
        if not (np.isfinite(vmax) and vmax > 0.0):
            raise ValueError(f"KtsTables: vmax must be finite and > 0, got {vmax}")
        if self.count > KTS_MAX_VIDEOS:
            raise ValueError(f"KtsTables: {self.count} videos, a batch takes at most {KTS_MAX_VIDEOS}")
        self.nvideos, self.frames = self.count, self.total
        self.stride, self.lmin, self.vmax = int(stride), int(lmin), vmax
        self.n = -(-self.lengths // self.stride)
        self.max_n = int(self.n.max())
        if self.max_n > KTS_MAX_SAMPLES:
            v = int(np.argmax(self.n))
            raise ValueError(f"KtsTables: video {v} has {int(self.n[v])} samples at stride {self.stride}, above the "
                             f"LDS-resident limit {KTS_MAX_SAMPLES}")
        if ncp is None or np.isscalar(ncp):
            ncp = [ncp] * self.nvideos
        ncp = list(ncp)
        if len(ncp) != self.nvideos:
            raise ValueError(f"KtsTables: {len(ncp)} ncp entries for {self.nvideos} videos")
        self.ncp = np.array([int(nv) - 1 if c is None else int(c) for c, nv in zip(ncp, self.n)], dtype=np.int64)
        if (self.ncp < 0).any():
            raise ValueError(f"KtsTables: ncp must be >= 0, got {int(self.ncp.min())}")
        self.m_max = np.maximum(0, np.minimum(self.ncp, self.n // self.lmin - 1))
        self.k_offsets = exclusive_offsets(self.n * self.n)
        self.k1_offsets = exclusive_offsets(self.n + 1)
        self.jt_offsets = exclusive_offsets((self.n + 1) * (self.n + 1))
        self.p_offsets = exclusive_offsets((self.m_max + 1) * (self.n + 1))
        self.cost_offsets = exclusive_offsets(self.m_max + 1)
        self.k_entries, self.k1_entries = int(self.k_offsets[-1]), int(self.k1_offsets[-1])
        self.jt_entries, self.p_entries = int(self.jt_offsets[-1]), int(self.p_offsets[-1])
        self.cost_cap = self.shot_cap = int(self.cost_offsets[-1])
        nt = -(-self.n // KTS_TILE)
        upper = [np.triu_indices(int(t)) for t in nt]                  # (ti, tj), ti <= tj, row by row
        self.tiles = np.concatenate([np.stack([np.full(ti.size, v), ti, tj], 1) for v, (ti, tj) in enumerate(upper)])
        self.tiles = self.tiles.astype(np.int32).reshape(-1, 3)
        self.ntiles = self.tiles.shape[0]
        for name, entries in (("Gram", self.k_entries), ("Jt", self.jt_entries), ("p", self.p_entries),
                              ("tile", self.ntiles)):
            if entries >= 1 << 31:
                raise ValueError(f"KtsTables: the packed {name} buffer needs {entries} entries, the kernels take fewer "
                                 "than 2^31")
        self.penalties = np.concatenate([kts_penalties(nv, mm, vmax) for nv, mm in zip(self.n, self.m_max)])
        self.workspace_bytes = sum((int(b) + 255) & ~255 for b in (8 * self.k1_entries, 8 * self.k_entries,
                                                                   8 * self.jt_entries, 2 * self.p_entries))
        self.videos = np.zeros((self.nvideos, _KTS_VIDEO_COLS), dtype=np.int64)
        for col, x in enumerate((self.offsets[:-1], self.lengths, self.n, self.m_max, self.k_offsets[:-1],
                                 self.k1_offsets[:-1], self.jt_offsets[:-1], self.p_offsets[:-1], self.cost_offsets[:-1])):
            self.videos[:, col] = x
        self.videos_t, self.tiles_t, self.penalties_t = _upload(self.device, self.videos, self.tiles, self.penalties)

    def shots_of(self, v, change_points):
        """The [(start, end)] list, in video-relative FRAME rows, that ``change_points`` (ascending sample indices)
        cut video ``v`` into: b_0 = 0, b_j = cp[j - 1] * stride, the last end N_v."""
        b = [0] + [int(c) * self.stride for c in change_points] + [int(self.lengths[v])]
        return list(zip(b[:-1], b[1:]))


class RankTables(RaggedOffsets):
    """The host plan of one batch layout for the pairwise ranking loss (loss.rank_loss), built once from the host row
    offsets [V + 1] of the videos in the concatenated scores (video v is rows offsets[v] .. offsets[v + 1]).

    Host side (numpy): ``offsets``, ``lengths`` (int64), ``nseq``, ``rows`` (= offsets[-1]), ``max_t``, ``tiles`` int32
    [ntiles, 2] = (video, row tile of 256 rows) - every video's tiles 0 .. ceil(T_v / 256) - 1, video after video -
    ``ntiles``.  Device side: ``offsets_t`` int64 [V + 1], ``tiles_t``, uploaded once.  ``device="cpu"`` keeps everything
    on the host (the builder can be checked without a GPU or the library).  Refused, each with a ValueError: an empty
    batch, offsets that do not start at 0 or do not increase strictly, a video longer than 32768 rows (its pair counts
    stay below 2^30 per row and below 2^31 summed over a video), 2^31 rows or more.  A video of one row is allowed: it
    has no pair, its loss and gradient are 0."""

    def __init__(self, offsets_host, rows=None, device=None):
        super().__init__(offsets_host, "RankTables", device=device, max_length=RANK_MAX_T, rows=rows)
        self.nseq, self.rows, self.max_t = self.count, self.total, self.max_len
        self.tiles = np.stack(segment_tiles(-(-self.lengths // RANK_TILE)), 1).astype(np.int32).reshape(
            -1, _RANK_TILE_COLS)
        self.ntiles = self.tiles.shape[0]
        self.tiles_t, = _upload(self.device, self.tiles)


class RenderTables(RaggedOffsets):
    """The host plan of one batch layout for rendering a summary (render.summary_index, summary_frames, summary_audio),
    built once from the host frame offsets [V + 1] of the videos in the concatenated frames and the capacities of the
    buffers the summary is written to - host numbers, so that no launch waits for a count.

    ``capacity``: int64 [V], the most frames a summary of video v may hold (a SummaryTables' ``capacity``; None: the
    whole video, for a bare mask).  ``frame_cap``: entries of the frame list (default: sum(capacity), N for a bare
    mask).  ``run_cap``: rows of the run table (default ceil(N / 2) + V: a video of n frames has at most ceil(n / 2)
    runs; from_keyshots passes the shot capacity, since a run is one or more whole shots).  Both at least 1.
    Audio (all three of ``wave_offsets``, ``fps`` given, ``sr``): ``wave_offsets`` the host sample offsets [V + 1] of the
    tracks in the concatenated waveform (start at 0, do not decrease), ``fps`` one number or one per video, converted
    to float64 HERE and uploaded with the plan, ``sr`` the sample rate.  ``sample_cap`` (None: computed) bounds the
    summary's samples.  DERIVED, not measured: a run (s, e) of video v holds floor(e / fps * sr) - floor(s / fps * sr)
    < (e - s) * sr / fps + 1 samples in exact arithmetic, the runs of v hold at most capacity[v] frames together and
    there are at most R_v = min(capacity[v], ceil(n_v / 2)) of them, and no run leaves the track, so video v holds at
    most min(len_v, ceil(capacity[v] * sr / fps_v) + R_v + 1) samples; the last + 1 absorbs the float64 rounding of the
    two bounds of every run, which sums to less than one sample while R_v * n_v * sr / fps_v < 2^50.  sample_cap is the
    sum over the videos, and S, the whole waveform, for a bare mask.  Every store is guarded by its capacity on the
    device whatever the bound.

    Host side (numpy): ``offsets``, ``lengths``, ``nvideos``, ``frames``, ``bare`` (no capacity was given),
    ``capacity``, ``frame_cap``, ``run_cap``,
    ``tiles`` int32 [ntiles, 2] = (video, tile of 1024 frames) - every video's tiles, video after video -, ``ntiles``;
    with audio ``wave_offsets``, ``fps`` float64 [V], ``sr``, ``samples`` (= wave_offsets[-1]), ``sample_cap``.
    Device side: ``offsets_t``, ``tiles_t``; with audio ``wave_offsets_t``, ``fps_t``.  ``device="cpu"`` keeps everything
    on the host (the builder can be checked without a GPU or the library).  Refused, each with a ValueError: what
    ShotTables refuses about the offsets (more than 2^24 frames among it), a capacity of another length than V or
    negative, frame_cap or run_cap below 1, wave offsets of another length, not starting at 0 or decreasing, an fps or
    sr that is not finite and positive, wave_offsets without fps or the reverse."""

    def __init__(self, offsets_host, frame_cap=None, run_cap=None, capacity=None, wave_offsets=None, fps=None, sr=16000,
                 sample_cap=None, device=None):
        super().__init__(offsets_host, "RenderTables", device=device, max_total=RENDER_MAX_FRAMES, total_inclusive=True)
        self.nvideos, self.frames = self.count, self.total
        bare = capacity is None
        capacity = self.lengths.copy() if bare else np.array(capacity, dtype=np.int64).reshape(-1)
        if capacity.size != self.nvideos or (capacity < 0).any():
            raise ValueError(f"RenderTables: capacity must hold one non-negative entry per video ({self.nvideos})")
        self.bare, self.capacity = bare, np.minimum(capacity, self.lengths)
        self.frame_cap = max(int(self.capacity.sum()), 1) if frame_cap is None else int(frame_cap)
        self.run_cap = -(-self.frames // 2) + self.nvideos if run_cap is None else int(run_cap)
        if self.frame_cap < 1 or self.run_cap < 1:
            raise ValueError(f"RenderTables: frame_cap and run_cap must be >= 1, got {self.frame_cap} and {self.run_cap}")
        self.tiles = np.stack(segment_tiles(-(-self.lengths // RENDER_TILE)), 1).astype(np.int32).reshape(
            -1, _RENDER_TILE_COLS)
        self.ntiles = self.tiles.shape[0]
        self.tiles_t, = _upload(self.device, self.tiles)
        self.has_audio = wave_offsets is not None
        if self.has_audio != (fps is not None):
            raise ValueError("RenderTables: wave_offsets and fps come together")
        if not self.has_audio:
            self.wave_offsets = self.fps = self.sr = self.samples = self.sample_cap = None
            return
        tracks = RaggedOffsets(wave_offsets, "RenderTables: wave_offsets", device=self.device, min_length=0,
                               max_total=1 << 62)
        if tracks.count != self.nvideos:
            raise ValueError(f"RenderTables: {tracks.count} tracks for {self.nvideos} videos")
        fps = np.array(fps, dtype=np.float64).reshape(-1)
        fps = np.repeat(fps, self.nvideos) if fps.size == 1 else fps
        self.sr = float(sr)
        if fps.size != self.nvideos or not (np.isfinite(fps).all() and (fps > 0).all()):
            raise ValueError(f"RenderTables: fps must be one finite positive number, or one per video ({self.nvideos})")
        if not (np.isfinite(self.sr) and self.sr > 0):
            raise ValueError(f"RenderTables: sr must be finite and positive, got {sr}")
        self.wave_offsets, self.wave_offsets_t, self.fps, self.samples = tracks.offsets, tracks.offsets_t, fps, tracks.total
        self.fps_t, = _upload(self.device, fps)
        runs = np.minimum(self.capacity, -(-self.lengths // 2))
        per_video = np.minimum(tracks.lengths, np.ceil(self.capacity * self.sr / fps).astype(np.int64) + runs + 1)
        if sample_cap is None:
            sample_cap = self.samples if bare else int(per_video.sum())
        self.sample_cap = max(int(sample_cap), 1)

    @classmethod
    def from_keyshots(cls, plan, **kw):
        """The plan for rendering row(s) of the KeyshotResult computed with ``plan`` (a SummaryTables, or the result
        itself): frame_cap = plan.capacity.sum(), run_cap = plan.shot_cap, on the plan's device; ``kw``: the audio
        arguments."""
        plan = getattr(plan, "plan", plan)
        if not isinstance(plan, SummaryTables):
            raise ValueError("RenderTables.from_keyshots: plan must be a SummaryTables or a KeyshotResult")
        return cls(plan.offsets, max(int(plan.capacity.sum()), 1), plan.shot_cap, plan.capacity,
                   device=kw.pop("device", plan.device), **kw)


class FusionTables:
    """The host plan of one batch layout for fusion_batch, built once from the host list of pairs
    ``(v_row0, n, a_row0, m)``: pair p is rows v_row0 .. v_row0 + n of the visual matrix against rows a_row0 ..
    a_row0 + m of the audio matrix.  Nothing is padded; the pairs may leave gaps and come in any order.

    Host side (numpy): ``n``, ``m``, ``cell_off`` (first element of the pair's [n, m] block in the cost buffer and the
    code workspace), ``path_off`` / ``path_cap`` (its path slot: n + m - 1 rows), ``row_off`` (first of its n row
    counts), ``cls`` (size class 0/1/2), ``order`` (pairs sorted by class, longest sweep first inside a class),
    ``class_count``, ``class_max_l``, ``tiles`` (pair, row tile, column tile), ``cells``, ``path_rows``, ``rows``,
    ``workspace_bytes``.  Device side: ``pairs`` int64 [P, 8], ``order_t``, ``tiles_t``, ``row_pair`` int32 [rows].
    ``device="cpu"`` keeps everything on the host (the table builder can be checked without a GPU)."""

    def __init__(self, pairs, device=None):
        arr = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 4)
        v0, n, a0, m = (arr[:, k].copy() for k in range(4))
        if (n <= 0).any() or (m <= 0).any():
            raise ValueError("fusion_batch: a pair is empty (n == 0 or m == 0)")
        if (v0 < 0).any() or (a0 < 0).any():
            raise ValueError("fusion_batch: negative row offset")
        if (n > FUSION_MAX_N).any():
            raise ValueError(f"fusion_batch: a pair has n = {int(n.max())} rows, above the LDS-resident limit {FUSION_MAX_N}")
        if (m >= 1 << 30).any():
            raise ValueError("fusion_batch: a pair has m >= 2^30 rows")
        npairs = arr.shape[0]
        self.npairs, self.v_row0, self.n, self.a_row0, self.m = npairs, v0, n, a0, m
        self.v_rows_needed = int((v0 + n).max()) if npairs else 0
        self.a_rows_needed = int((a0 + m).max()) if npairs else 0
        cell, path, row = exclusive_offsets(n * m), exclusive_offsets(n + m - 1), exclusive_offsets(n)
        self.cell_off, self.path_off, self.row_off = cell[:-1], path[:-1], row[:-1]
        self.path_cap = n + m - 1
        self.cells, self.path_rows, self.rows = int(cell[-1]), int(path[-1]), int(row[-1])
        small = np.minimum(n, m)
        self.cls = (small > FUSION_SMALL_L).astype(np.int64) + (small > FUSION_MID_L)
        # by class, then the most anti-diagonals first (neighbours in a class-0 workgroup sweep about as long); stable
        self.order = np.lexsort((np.arange(npairs), -(n + m), self.cls)).astype(np.int32)
        self.class_count = [int((self.cls == c).sum()) for c in range(3)]
        self.class_max_l = [int(small[self.cls == c].max()) if self.class_count[c] else 0 for c in range(3)]
        self.max_n = int(n.max()) if npairs else 0
        ti, tj = -(-n // _FUSION_TILE), -(-m // _FUSION_TILE)
        tp, k = segment_tiles(ti * tj)
        self.ntiles = tp.size
        self.tiles = np.stack([tp, k // tj[tp], k % tj[tp]], 1).astype(np.int32).reshape(-1, 3)
        self.row_pair_host = np.repeat(np.arange(npairs, dtype=np.int32), n)
        self.workspace_bytes = (self.cells + 255) & ~255     # avs_dtw_batch_workspace_bytes: one code byte per cell
        table = np.zeros((npairs, _FUSION_PAIR_COLS), dtype=np.int64)
        for col, x in enumerate((v0, n, a0, m, self.cell_off, self.path_off, self.row_off)):
            table[:, col] = x
        self.pairs, self.order_t, self.tiles_t, self.row_pair = _upload(device, table, self.order, self.tiles,
                                                                        self.row_pair_host)
        self.device = self.pairs.device
        self._out = {}
        self.out_offsets(None)

    def out_rows(self, target_length=None):
        """Rows each pair contributes to the fused output: min(n, target_length)."""
        return self.n if target_length is None else np.minimum(self.n, max(int(target_length), 0))

    def out_offsets(self, target_length=None):
        """(device int64 [P + 1] row offsets of the fused output, host total) for a target length; uploaded once per
        length and kept, so that a repeated fusion_batch call moves nothing between host and device."""
        key = None if target_length is None else max(int(target_length), 0)
        if key not in self._out:
            off = exclusive_offsets(self.out_rows(key))
            self._out[key] = (_upload(self.device, off)[0], int(off[-1]))
        return self._out[key]
