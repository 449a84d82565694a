"""Shot segmentation on the MI355X: the front end that features/extractors.py:388-393 delegates
to ``scenedetect.detect(video_path, ContentDetector())``.

PySceneDetect is a third-party dependency absent here and unpinned; restated from its published algorithm
[3P-memory, v0.6.x defaults: threshold 27.0, min_scene_len 15, weights hue/sat/lum = 1/1/1, edges 0,
auto-downscale to ~256 px wide by striding]: a frame's content score is the mean of the three mean absolute
differences of OpenCV's 8-bit HSV against the previous frame; a cut is placed where the score reaches the
threshold and at least min_scene_len frames passed since the last cut; scenes are the intervals between cuts
(empty when there is no cut).  The per-frame sums come from the GPU scan; the thresholding is a host loop over
N numbers.

detect_shots_batch does the same for a ragged batch of videos without that download: the sums, the threshold decision,
the greedy rule and the tables stage 1 is driven by (shots, sampled frames, BatchNorm micro-batches) are kernels of
csrc/shots_batch.hip, and sample_frames gathers the sampled frames into one dense tensor.
"""
import numpy as np
import torch

from .. import ops
from ..ingest import Nv12Frames, nv12_hsv_frame_diff_batch
from ..yuv import YuvFrames, yuv_hsv_frame_diff_batch
from ..ragged import exclusive_offsets

DEFAULT_MIN_WIDTH = 256  # scenedetect.scene_manager.DEFAULT_MIN_WIDTH


def downscale_factor(frame_width, effective_width=DEFAULT_MIN_WIDTH):
    if frame_width < effective_width:
        return 1
    return int(frame_width / float(effective_width))


def content_scores(frames_u8, step=None):
    """frames uint8 [n,h,w,3] (device) -> float64 [n] content scores (score[0] = 0)."""
    n, h, w, _ = frames_u8.shape
    step = downscale_factor(w) if step is None else step
    sums = ops.hsv_frame_diff(frames_u8, step).cpu().numpy().astype(np.float64)
    pixels = float(len(range(0, h, step)) * len(range(0, w, step)))
    return (sums / pixels).sum(axis=1) / 3.0


def cuts_from_scores(scores, threshold=27.0, min_scene_len=15):
    cuts, last = [], 0
    for f in range(1, len(scores)):
        if scores[f] >= threshold and f - last >= min_scene_len:
            cuts.append(f)
            last = f
    return cuts


def detect_shots(frames_u8, threshold=27.0, min_scene_len=15):
    """[(start_frame, end_frame)] like scenedetect.detect(...): empty when no cut was found."""
    if not torch.is_tensor(frames_u8):
        frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8))
    if not frames_u8.is_cuda:
        frames_u8 = frames_u8.cuda()
    n = frames_u8.shape[0]
    cuts = cuts_from_scores(content_scores(frames_u8.contiguous()), threshold, min_scene_len)
    if not cuts:
        return []
    bounds = [0] + cuts + [n]
    return [(bounds[i], bounds[i + 1]) for i in range(len(bounds) - 1)]


# --------------------------------------------------------------------------- a ragged batch of videos
def shot_tables_host(cuts_per_video, lengths):
    """The tables of the batched detector from per-video cut lists, in numpy: the closed forms the kernels use, for tests
    and for callers that bring their own shots.  ``cuts_per_video[v]``: ascending video-relative cut frames in
    1 .. lengths[v] - 1 ([] = no cut = no shot, as detect_shots).  A shot (s, e) holds c = min(100, ceil(e/3) -
    ceil(s/3)) sampled frames, frame k being 3 (ceil(s/3) + k) - what sample_shot_indices(s, e) lists - in ceil(c/4)
    BatchNorm groups of 4 with a shorter tail group.  Returns a dict of int64 arrays: shot_offsets [V + 1], shots [S, 2]
    (video-relative), sample_offsets [S + 1], sample_index [F] (rows of the concatenated frames), group_offsets [G + 1]
    (rows of the sampled tensor), counts [4] = (S, F, G, most sampled frames of a shot)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if len(cuts_per_video) != lengths.size:
        raise ValueError("shot_tables_host: one cut list per video")
    base = exclusive_offsets(lengths)
    starts, ends, video, per_video = [], [], [], []
    for v, (cuts, n) in enumerate(zip(cuts_per_video, lengths)):
        cuts = np.asarray(cuts, dtype=np.int64).reshape(-1)
        if cuts.size and (cuts[0] < 1 or cuts[-1] >= n or (np.diff(cuts) <= 0).any()):
            raise ValueError(f"shot_tables_host: video {v}: the cuts must ascend strictly inside 1 .. {int(n) - 1}")
        bounds = np.concatenate([[0], cuts, [n]]) if cuts.size else np.zeros(1, dtype=np.int64)
        starts.append(bounds[:-1])
        ends.append(bounds[1:])
        video.append(np.full(bounds.size - 1, v, dtype=np.int64))
        per_video.append(bounds.size - 1)
    start, end, video = (np.concatenate(x).astype(np.int64) for x in (starts, ends, video))
    first = -(-start // ops.SHOT_INTERVAL)                                  # ceil(s / 3)
    count = np.minimum(ops.SHOT_MAX_FRAMES, -(-end // ops.SHOT_INTERVAL) - first)
    groups = -(-count // ops.SHOT_MICRO_BATCH)
    sample_offsets, group_first = exclusive_offsets(count), exclusive_offsets(groups)
    nsample, ngroup = int(sample_offsets[-1]), int(group_first[-1])
    k = np.arange(nsample, dtype=np.int64) - np.repeat(sample_offsets[:-1], count)
    sample_index = np.repeat(base[video] + ops.SHOT_INTERVAL * first, count) + ops.SHOT_INTERVAL * k
    g = np.arange(ngroup, dtype=np.int64) - np.repeat(group_first[:-1], groups)
    group_offsets = np.concatenate([np.repeat(sample_offsets[:-1], groups) + ops.SHOT_MICRO_BATCH * g, [nsample]])
    return {"shot_offsets": exclusive_offsets(per_video), "shots": np.stack([start, end], 1).reshape(-1, 2),
            "sample_offsets": sample_offsets, "sample_index": sample_index.astype(np.int64),
            "group_offsets": group_offsets.astype(np.int64),
            "counts": np.array([start.size, nsample, ngroup, int(count.max()) if count.size else 0], dtype=np.int64)}


class ShotBatchResult:
    """What detect_shots_batch leaves on the device: ``plan`` (the ops.ShotTables), ``sums`` int32 [N,3] (uint32 bit
    patterns), ``cuts`` / ``totals`` (ops.shot_cuts_batch) and the tables of ops.shot_tables at their capacities -
    ``counts``, ``shot_offsets``, ``shots``, ``sample_offsets``, ``sample_index``, ``group_offsets``.  Nothing has been
    read back; host() is the one download."""

    def __init__(self, plan, sums, cuts, totals, tables):
        self.plan, self.sums, self.cuts, self.totals = plan, sums, cuts, totals
        self.counts, self.shot_offsets, self.shots = tables["counts"], tables["shot_offsets"], tables["shots"]
        self.sample_offsets, self.sample_index = tables["sample_offsets"], tables["sample_index"]
        self.group_offsets, self._packed = tables["group_offsets"], tables["packed"]
        self._host = None

    def host_tables(self):
        """The tables but sample_index as numpy arrays cut to their counts (dict as shot_tables_host): ONE download, kept."""
        if self._host is None:
            nv, plan = self.plan.nvideos, self.plan
            flat = self._packed.cpu().numpy()
            counts, video_off, shots, sample_offsets, group_offsets = np.split(flat, np.cumsum(plan.packed_sizes)[:-1])
            s, f, g, _ = (int(x) for x in counts)
            if s > plan.shot_cap or f > plan.sample_cap or g > plan.group_cap:
                raise RuntimeError(f"detect_shots_batch: counts {counts.tolist()} exceed the capacities "
                                   f"{(plan.shot_cap, plan.sample_cap, plan.group_cap)}")
            self._host = {"counts": counts, "shot_offsets": video_off[:nv + 1], "shots": shots.reshape(-1, 2)[:s],
                          "sample_offsets": sample_offsets[:s + 1], "group_offsets": group_offsets[:g + 1]}
        return self._host

    def host(self):
        """Per video the list detect_shots returns - [(start_frame, end_frame)], [] when the video has no cut."""
        t = self.host_tables()
        off, shots = t["shot_offsets"], t["shots"]
        return [[(int(a), int(b)) for a, b in shots[off[v]:off[v + 1]]] for v in range(self.plan.nvideos)]

    def audio_bounds(self, fps, sr):
        """Per video the [(int(start / fps * sr), int(end / fps * sr))] list of its shots - process_decoded's arithmetic,
        what AudioFeatureExtractor.forward_shots_batch takes.  ``fps``: one number or one per video."""
        fps = [fps] * self.plan.nvideos if np.isscalar(fps) else list(fps)
        if len(fps) != self.plan.nvideos:
            raise ValueError("audio_bounds: one fps per video")
        return [[(int(start / f * sr), int(end / f * sr)) for start, end in shots] for f, shots in zip(fps, self.host())]


def detect_shots_batch(frames_u8, video_offsets, threshold=27.0, min_scene_len=15, step=None, matrix="bt601"):
    """detect_shots for a ragged batch: frames uint8 [N,h,w,3] on the device, the videos concatenated, and the host frame
    offsets [V + 1] (or a prepared ops.ShotTables) -> ShotBatchResult.  Four kernels' worth of launches - the frame
    differences of all videos, one workgroup per video for the cuts, a scan, one workgroup per video for the tables -
    and no host round trip: the cut lists, the shot table, the sampled-frame table and the BatchNorm micro-batch table
    stay on the device until ShotBatchResult.host().  ``frames_u8`` may be an ingest.Nv12Frames or a yuv.YuvFrames (I420,
    P010, ...): the frame differences then read the decoder's surfaces (converted by ``matrix`` on the way in, no BGR
    copy) and give the integers of the converted frames; everything after them is the same launches."""
    nv12, yuv = isinstance(frames_u8, Nv12Frames), isinstance(frames_u8, YuvFrames)
    data = frames_u8.data if nv12 or yuv else frames_u8
    if not torch.is_tensor(data) or not data.is_cuda:
        raise ValueError("detect_shots_batch: frames must be a device tensor (there is no CPU fallback)")
    plan = video_offsets if isinstance(video_offsets, ops.ShotTables) else \
        ops.ShotTables(video_offsets, min_scene_len, data.device)
    if plan.min_scene_len != int(min_scene_len):
        raise ValueError(f"detect_shots_batch: the tables were built for min_scene_len {plan.min_scene_len}")
    if not (nv12 or yuv):
        frames_u8 = frames_u8.contiguous()
    h, w = frames_u8.shape[1:3]
    step = downscale_factor(w) if step is None else int(step)
    pixels = float(len(range(0, h, step)) * len(range(0, w, step)))
    if nv12:
        sums = nv12_hsv_frame_diff_batch(frames_u8, plan, step, raw=True, matrix=matrix)
    elif yuv:
        sums = yuv_hsv_frame_diff_batch(frames_u8, plan, step, raw=True, matrix=matrix)
    else:
        sums = ops.hsv_frame_diff_batch(frames_u8, plan, step, raw=True)
    cuts, totals = ops.shot_cuts_batch(plan, sums, pixels, threshold)
    return ShotBatchResult(plan, sums, cuts, totals, ops.shot_tables(plan, cuts, totals))


def sample_frames(frames_u8, result):
    """(sampled frames uint8 [F,h,w,3] on the device, group offsets int64 [G + 1] on the host) of a ShotBatchResult:
    frames_u8[result.sample_index], gathered with the row count read on the device, and the BatchNorm micro-batch table -
    ready for VisualFeatureExtractor.embed(frames, group_frames).  The gather is launched before the result's one
    download; the download only cuts the dense tensor to F rows."""
    if not isinstance(result, ShotBatchResult):
        raise ValueError("sample_frames: result must come from detect_shots_batch")
    if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda:
        raise ValueError("sample_frames: frames must be a device tensor (there is no CPU fallback)")
    if frames_u8.shape[0] != result.plan.frames:
        raise ValueError(f"sample_frames: {frames_u8.shape[0]} frames, the result was computed for {result.plan.frames}")
    dense = ops.gather_rows(frames_u8.contiguous(), result.sample_index, result.counts[1:2])
    t = result.host_tables()
    return dense[:int(t["counts"][1])], torch.from_numpy(t["group_offsets"].copy())
