"""Counterpart of the reference's scripts/train_av_model.py:11-96 on the MI355X.

``train_on_dataset`` is the reference's loop step for step (DataLoader(batch_size=8, shuffle=True,
collate_fn=lambda x: x[0]) — i.e. one of every eight videos per step, SURVEY Q12 —, one shot boundary
(0, num_shots), fps 30, AdamW lr 1e-4, MSE against the single broadcast target, Dropout active).  The model's
forward/backward run through libavsum_hip.so; the loss, the optimiser and the data loader are the caller's
torch, exactly as in the reference.  ``train()`` reads the TVSum HDF5 annotations like the reference and needs
h5py + the dataset on disk; ``train_synthetic`` is the BASELINE config-5 harness (synthetic labels ~U[1,5]).
With torch.distributed initialised (one process per GPU) the gradients are all-reduced before each step.

``train_on_dataset(..., videos_per_step=k)`` with k in 2..8 trains on k of the eight videos the loader draws, as ONE ragged
batch per optimiser step (``collate_videos`` -> ``train_step_batch``: AVBiLSTMModel.train_rows, ops.seq_mse, the mean
of the per-video losses).  The default k = 1 is the reference's loop, untouched.

``train_on_dataset(..., optimizer="fused")`` replaces torch.optim.AdamW by optim.FusedAdamW (libavsum_optim.so: the whole
step in at most three launches, optionally with global-norm clipping and the skip of a non-finite step, both decided on
the device).  The default "torch" is the reference's optimiser, untouched.

``train_on_dataset(..., dropout_seed=s)`` seeds the model's Dropout (AVBiLSTMModel.seed_dropout: counter-based masks,
dropout.py) and gives the video at position i of the b-th drawn batch of 8 the sample id 8 * b + i, so its masks depend
on (s, b, i) only - not on videos_per_step, not on the number of ranks.  The default None draws with torch, untouched.

``train_on_dataset(..., targets="shots", loss="mse+rank")`` (videos_per_step >= 2) trains every row towards the target of
ITS shot (loss.shot_targets: the reference's align_shots_to_annotations over the item's shot table) and adds the pairwise
ranking loss of loss.rank_loss (libavsum_loss.so) per video.  The defaults "video" / "mse" are the step above, untouched.
"""
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from .. import dist as avd, ops
from ..models.av_model import AVBiLSTMModel
from ..ragged import exclusive_offsets
from ..utils.alignments import align_shots_to_annotations


def train_step(model, optimizer, features, frame_scores, device="cuda", sample=None):
    """Lines 72-96 of the reference for one (features, frame_scores) item.  Returns the loss value.  ``sample``: the
    sample id of this video's Dropout masks, for a model after seed_dropout(seed) (None: the model's next id)."""
    num_shots = features["visual"].shape[0]
    shot_scores = align_shots_to_annotations(shot_boundaries=[(0, num_shots)], annotations=frame_scores.numpy(),
                                             fps=30)
    visual = features["visual"].unsqueeze(0).to(device)
    audio = features["audio"].unsqueeze(0).to(device)
    preds = model(visual, audio) if sample is None else model(visual, audio, sample=sample)
    loss = F.mse_loss(preds, shot_scores.to(device).float())
    optimizer.zero_grad()
    loss.backward()
    avd.allreduce_gradients(model)
    optimizer.step()
    return float(loss.item())


def collate_videos(items, targets="video"):
    """Host only (torch on the CPU): V dataset items ({"visual": [S_v, Dv], "audio": [S_v, Da]}, frame scores) as one
    ragged batch -> (visual_rows fp32 [R, Dv], audio_rows fp32 [R, Da], offsets int64 [V + 1], targets fp32 [V]).
    targets[v] is the target train_step builds for that video: the single shot score of the boundary (0, S_v) at fps 30.
    Refused with a ValueError: no item, a video without shots, visual / audio of different lengths, feature widths that
    differ between the videos.

    ``targets="shots"``: every item's features also hold "shots", int64 [S_v, 2] video-relative frame bounds, one per
    row (a missing or mis-sized table is a ValueError).  The fourth entry is then what loss.shot_targets takes instead
    of [V] scalars: the tuple (annotations fp32 [sum of A_v], the frame-score vectors concatenated; ann_offsets int64
    [V + 1]; shots int64 [R, 2]) - the shot offsets are ``offsets``, a row per shot."""
    if targets not in ("video", "shots"):
        raise ValueError(f"collate_videos: targets must be 'video' or 'shots', got {targets!r}")
    if len(items) == 0:
        raise ValueError("collate_videos: no video")
    vis, aud, lengths, per_video, shots = [], [], [], [], []
    for i, (features, frame_scores) in enumerate(items):
        v, a = features["visual"], features["audio"]
        if v.dim() != 2 or a.dim() != 2 or v.shape[0] != a.shape[0]:
            raise ValueError(f"collate_videos: video {i} has visual {tuple(v.shape)} and audio {tuple(a.shape)}")
        if v.shape[0] == 0:
            raise ValueError(f"collate_videos: video {i} is empty")
        if vis and (v.shape[1] != vis[0].shape[1] or a.shape[1] != aud[0].shape[1]):
            raise ValueError(f"collate_videos: video {i} has feature widths {v.shape[1]} / {a.shape[1]}, video 0 "
                             f"{vis[0].shape[1]} / {aud[0].shape[1]}")
        if targets == "shots":
            table = features.get("shots")
            if table is None:
                raise ValueError(f"collate_videos: targets='shots' needs features['shots'], video {i} has none")
            table = torch.as_tensor(table)
            if table.dtype != torch.int64 or tuple(table.shape) != (v.shape[0], 2):
                raise ValueError(f"collate_videos: video {i} has {v.shape[0]} rows and a shot table {table.dtype} "
                                 f"{tuple(table.shape)}: it must be int64 [{v.shape[0]}, 2]")
            shots.append(table)
            per_video.append(frame_scores.reshape(-1).float())
        else:
            shot_scores = align_shots_to_annotations(shot_boundaries=[(0, v.shape[0])],
                                                     annotations=frame_scores.numpy(), fps=30)
            per_video.append(shot_scores.float().reshape(1))
        vis.append(v.float())
        aud.append(a.float())
        lengths.append(v.shape[0])
    offsets = torch.from_numpy(exclusive_offsets(lengths))
    if targets == "shots":
        ann_offsets = torch.from_numpy(exclusive_offsets([p.shape[0] for p in per_video]))
        return torch.cat(vis), torch.cat(aud), offsets, (torch.cat(per_video), ann_offsets, torch.cat(shots))
    return torch.cat(vis), torch.cat(aud), offsets, torch.cat(per_video)


LOSSES = ("mse", "rank", "mse+rank")


def _check_objective(targets, loss, what):
    if targets not in ("video", "shots"):
        raise ValueError(f"{what}: targets must be 'video' or 'shots', got {targets!r}")
    if loss not in LOSSES:
        raise ValueError(f"{what}: loss must be one of {LOSSES}, got {loss!r}")
    if loss != "mse" and targets == "video":
        raise ValueError(f"{what}: loss={loss!r} needs targets='shots' (with one target per video every pair is tied)")


def train_step_batch(model, optimizer, items, device="cuda", samples=None, targets="video", loss="mse", rank_weight=1.0,
                     rank_kind="logistic", rank_scale=1.0, rank_margin=0.1, fps=30):
    """One optimiser step on V videos at once: one upload of the collated rows, one forward / backward over the ragged
    batch, the loss = the mean of the per-video MSEs - its gradient is the average of the per-video gradients, i.e.
    what V ranks that take one video each hold after dist.allreduce_gradients (the same step up to summation order).
    Returns the per-video losses (a list of floats) from ONE download, after the step.  ``samples``: host sample ids
    [V] of the videos' Dropout masks, for a model after seed_dropout(seed) (None: the model's next V ids); with them the
    step IS the one V data-parallel ranks take with one video and its id each, Dropout included.

    ``targets="shots"``: every row is trained towards the target of its own shot, loss.shot_targets over the items'
    shot tables at ``fps`` (a scalar or one per video), computed on the device.  ``loss``: "mse" (ops.seq_mse), "rank"
    (loss.rank_loss of kind ``rank_kind`` with ``rank_scale`` / ``rank_margin``) or "mse+rank" (seq_mse + rank_weight *
    rank_loss per video); "rank" and "mse+rank" with targets="video" are refused, every pair would be tied.  The
    per-video losses and the flags of shot_targets come back in the step's ONE download; a set flag (a shot whose
    annotation slice is empty: its target is NaN) raises a ValueError after it, naming the video."""
    _check_objective(targets, loss, "train_step_batch")
    if targets == "video":
        visual, audio, offsets, video_targets = collate_videos(items)
    else:
        visual, audio, offsets, (annotations, ann_offsets, shots) = collate_videos(items, targets="shots")
    table = ops.SeqTable(offsets, visual.shape[0], device)
    if samples is None:
        preds = model.train_rows(visual.to(device), audio.to(device), table)
    else:
        preds = model.train_rows(visual.to(device), audio.to(device), table, samples=samples)
    flags = None
    if targets == "video":
        row_targets = video_targets.to(device)
    else:
        from .. import loss as avloss
        row_targets, flags = avloss.shot_targets(annotations.to(device), ann_offsets, shots, offsets, fps)
    if loss == "mse":
        losses = ops.seq_mse(preds, row_targets, table)
    else:
        ranks = avloss.rank_loss(preds, row_targets, ops.RankTables(offsets, visual.shape[0], device), rank_kind,
                                 rank_scale, rank_margin)
        losses = ranks if loss == "rank" else ops.seq_mse(preds, row_targets, table) + float(rank_weight) * ranks
    step_loss = losses.mean()
    optimizer.zero_grad()
    step_loss.backward()
    avd.allreduce_gradients(model)
    optimizer.step()
    if flags is None:
        return losses.detach().cpu().tolist()
    both = torch.cat([losses.detach(), flags.float()]).cpu()      # the one download: V losses, then V flags
    nv = len(items)
    bad = torch.nonzero(both[nv:]).reshape(-1).tolist()
    if bad:
        raise ValueError(f"train_step_batch: video {bad[0]} of the batch has a shot whose annotation slice is empty "
                         f"(its target is NaN): the shot table does not fit the annotations at fps {fps}")
    return both[:nv].tolist()


def select_positions(n, rank, world, videos_per_step):
    """The positions in a drawn batch of ``n`` videos that this rank trains on: (rank + j * world) % n for
    j < videos_per_step, duplicates dropped (a short last batch yields fewer)."""
    picked = []
    for j in range(videos_per_step):
        i = (rank + j * world) % n
        if i not in picked:
            picked.append(i)
    return picked


def select_items(items, rank, world, videos_per_step):
    """The videos of one drawn batch that this rank trains on: those at select_positions(len(items), ...)."""
    return [items[i] for i in select_positions(len(items), rank, world, videos_per_step)]


def train_on_dataset(dataset, epochs=100, lr=1e-4, model=None, on_step=None, device="cuda", videos_per_step=1,
                     optimizer="torch", max_grad_norm=None, skip_nonfinite=False, dropout_seed=None, targets="video",
                     loss="mse", rank_weight=1.0, rank_kind="logistic", rank_scale=1.0, rank_margin=0.1):
    """One process: the reference's loop exactly (its DataLoader, its global-RNG shuffle, item 0 of every batch of 8).
    With torch.distributed initialised (one process per GPU) it is data-parallel over that loop: rank 0's weights are
    broadcast first (C1), every rank draws the SAME shuffled batches of 8 (the shuffle seed comes from rank 0) and
    takes item `rank` of each (rank 0 the item the reference would take), gradients are averaged (C3) before every
    AdamW step - so the replicas and their optimiser states stay identical.

    videos_per_step = k in 2..8: every optimiser step trains on k videos of the drawn batch of 8 as one ragged batch
    (train_step_batch) - positions (rank + j * world) % len(batch), j < k, duplicates dropped; k = 8 in one process
    uses every video the loader draws.  on_step then receives the mean of the step's per-video losses.  Dropout draws
    its masks for the whole batch at once, so torch's RNG is consumed differently from k one-video steps.

    optimizer = "torch" (the default): torch.optim.AdamW, as the reference; max_grad_norm and skip_nonfinite must be
    left unset.  optimizer = "fused": optim.FusedAdamW(lr=lr, max_grad_norm=..., skip_nonfinite=...), the same update
    in fused HIP kernels; the model's ``fused_optimizer`` attribute then holds it (stats(), state_dict()).  In a
    data-parallel run allreduce_gradients runs BEFORE step() (train_step, train_step_batch), so every rank sees the same
    gradients, computes the same norm and takes the same skip decision: the replicas stay identical.

    dropout_seed = an integer in [0, 2^64): model.seed_dropout(dropout_seed), and every step hands the sample ids of its
    videos to train_step(sample=...) / train_step_batch(samples=...): 8 * (index of the drawn batch, counted through
    the epochs) + the video's position in that batch of 8.  A video's Dropout masks are then a function of (seed, batch
    index, position) alone: the same under any videos_per_step and any number of ranks, and a run is replayed from the
    seed.  torch's RNG is not consumed by Dropout.  None (the default): torch's generator draws the masks, as before.

    targets, loss, rank_weight, rank_kind, rank_scale, rank_margin: handed to train_step_batch, which describes them
    (the frame rate stays its default, the reference's 30).  videos_per_step == 1 stays the reference's loop: anything but targets="video" and loss="mse" is refused
    there.  The defaults hand train_step_batch nothing new."""
    import torch.distributed as tdist
    _check_objective(targets, loss, "train_on_dataset")
    objective = {} if (targets, loss) == ("video", "mse") else dict(
        targets=targets, loss=loss, rank_weight=rank_weight, rank_kind=rank_kind, rank_scale=rank_scale,
        rank_margin=rank_margin)
    if objective and videos_per_step == 1:
        raise ValueError("train_on_dataset: targets='shots' and the ranking losses need videos_per_step >= 2 "
                         "(videos_per_step = 1 is the reference's loop)")
    if optimizer not in ("torch", "fused"):
        raise ValueError(f"optimizer must be 'torch' or 'fused', got {optimizer!r}")
    if optimizer == "torch" and (max_grad_norm is not None or skip_nonfinite):
        raise ValueError("max_grad_norm and skip_nonfinite need optimizer='fused'")
    if not isinstance(videos_per_step, int) or not 1 <= videos_per_step <= 8:
        raise ValueError(f"videos_per_step must be 1..8 (the loader draws batches of 8), got {videos_per_step!r}")
    model = (model or AVBiLSTMModel()).to(device)
    if dropout_seed is not None:
        model.seed_dropout(dropout_seed)
    rank, world, gen = 0, 1, None
    if tdist.is_initialized() and tdist.get_world_size() > 1:
        rank, world = tdist.get_rank(), tdist.get_world_size()
        avd.broadcast_module(model, 0)
        seed = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64).to(device)
        tdist.broadcast(seed, 0)
        gen = torch.Generator().manual_seed(int(seed.item()))
    # a drawn batch -> (the positions of this rank's videos in it, the videos)
    if videos_per_step == 1:
        collate = lambda items: (rank % len(items), items[rank % len(items)])  # noqa: E731
    else:
        def collate(items):
            positions = select_positions(len(items), rank, world, videos_per_step)
            return positions, [items[i] for i in positions]
    loader = DataLoader(dataset, batch_size=8, shuffle=True, generator=gen, collate_fn=collate)
    if optimizer == "fused":
        from ..optim import FusedAdamW
        optimizer = FusedAdamW(model.parameters(), lr=lr, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        model.fused_optimizer = optimizer
    else:
        optimizer = torch.optim.AdamW(model.parameters(), lr=lr)
    drawn = 0                                                # batches of 8 drawn so far, through the epochs
    for _ in range(epochs):
        model.train()
        if videos_per_step == 1:
            for position, (features, frame_scores) in loader:
                ids = {} if dropout_seed is None else {"sample": 8 * drawn + position}
                loss = train_step(model, optimizer, features, frame_scores, device, **ids)
                drawn += 1
                if on_step is not None:
                    on_step(loss)
        else:
            for positions, items in loader:
                ids = {} if dropout_seed is None else {"samples": [8 * drawn + i for i in positions]}
                losses = train_step_batch(model, optimizer, items, device, **ids, **objective)
                drawn += 1
                if on_step is not None:
                    on_step(sum(losses) / len(losses))
        # the recurrences run split over four CUs (ops.lstm*): no bounded wait may have run out during the epoch
        dev = next(model.parameters()).device
        if dev.type == "cuda":
            bad = ops.lstm_split_errors(dev)
            if bad:
                raise RuntimeError(f"split LSTM recurrence: {bad} workgroup(s) gave up waiting for a partner's step vector")
    return model


class SyntheticShotDataset(torch.utils.data.Dataset):
    """TVSumDataset-shaped items: ({"visual": [S,4096], "audio": [S,296]}, frame scores [n_frames] ~ U[1,5]).
    ``with_shots=True`` adds "shots" to every item's features: int64 [S, 2], a ragged partition of the video's 30 * S
    frames into S shots of at least one frame - drawn after everything else, so the other values of the items are what
    they are without it."""

    def __init__(self, num_videos=8, shots=(20, 60), seed=5005, visual_dim=4096, audio_dim=296, with_shots=False):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for _ in range(num_videos):
            s = int(torch.randint(shots[0], shots[1] + 1, (1,), generator=g))
            feats = {"visual": torch.randn(s, visual_dim, generator=g), "audio": torch.zeros(s, audio_dim)}
            self.items.append((feats, torch.rand(s * 30, generator=g) * 4 + 1))
        if with_shots:
            for feats, scores in self.items:
                s, frames = feats["visual"].shape[0], scores.shape[0]
                cuts = torch.sort(torch.randperm(frames - 1, generator=g)[:s - 1] + 1).values      # s - 1 distinct cuts
                bounds = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([frames])])
                feats["shots"] = torch.stack([bounds[:-1], bounds[1:]], 1)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def train_synthetic(steps=20, seed=7, **dataset_kw):
    """BASELINE config 5 on synthetic labels: returns the list of per-step losses."""
    torch.manual_seed(seed)
    losses = []
    ds = SyntheticShotDataset(**dataset_kw)
    epochs = max(1, -(-steps * 8 // len(ds)) // 1)
    train_on_dataset(ds, epochs=epochs, on_step=losses.append)
    return losses[:steps]


def train():
    """The reference's entry point: TVSum .mat (HDF5) -> DataFrame -> TVSumDataset -> the loop above."""
    try:
        import h5py
    except ImportError as e:
        raise RuntimeError("train() reads ydata-tvsum50.mat with h5py, which is not installed here; "
                           "use train_on_dataset(dataset) or train_synthetic()") from e
    import pandas as pd
    from ..data.dataset import TVSumDataset
    with h5py.File("Evaluation/TVSum/ydata-tvsum50-matlab/matlab/ydata-tvsum50.mat", "r") as f:
        titles_ref = f["tvsum50/title"][:]
        videos_ref = f["tvsum50/video"][:]
        titles = ["".join(chr(c) for c in f[ref][:].flatten()) for ref in titles_ref.squeeze()]
        videos = ["".join(chr(c) for c in f[ref][:].flatten()) for ref in videos_ref.squeeze()]
        user_anno = f["tvsum50/user_anno"][:]
        rows = []
        for vid_idx in range(50):
            user_annotations = f[user_anno[vid_idx, 0]][:]
            for user_idx in range(20):
                rows.append({"Video Title": titles[vid_idx], "Video File Name": videos[vid_idx],
                             "User ID": user_idx + 1, "Annotations": user_annotations[user_idx].flatten()})
    return train_on_dataset(TVSumDataset(pd.DataFrame(rows), "data/processed"))
