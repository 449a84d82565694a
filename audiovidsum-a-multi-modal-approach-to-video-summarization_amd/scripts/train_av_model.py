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


def collate_videos(items):
    """Host only (torch on the CPU): V dataset items ({"visual": [S_v, Dv], "audio": [S_v, Da]}, frame scores) as one
    ragged batch -> (visual_rows fp32 [R, Dv], audio_rows fp32 [R, Da], offsets int64 [V + 1], targets fp32 [V]).
    targets[v] is the target train_step builds for that video: the single shot score of the boundary (0, S_v) at fps 30.
    Refused with a ValueError: no item, a video without shots, visual / audio of different lengths, feature widths that
    differ between the videos."""
    if len(items) == 0:
        raise ValueError("collate_videos: no video")
    vis, aud, lengths, targets = [], [], [], []
    for i, (features, frame_scores) in enumerate(items):
        v, a = features["visual"], features["audio"]
        if v.dim() != 2 or a.dim() != 2 or v.shape[0] != a.shape[0]:
            raise ValueError(f"collate_videos: video {i} has visual {tuple(v.shape)} and audio {tuple(a.shape)}")
        if v.shape[0] == 0:
            raise ValueError(f"collate_videos: video {i} is empty")
        if vis and (v.shape[1] != vis[0].shape[1] or a.shape[1] != aud[0].shape[1]):
            raise ValueError(f"collate_videos: video {i} has feature widths {v.shape[1]} / {a.shape[1]}, video 0 "
                             f"{vis[0].shape[1]} / {aud[0].shape[1]}")
        shot_scores = align_shots_to_annotations(shot_boundaries=[(0, v.shape[0])], annotations=frame_scores.numpy(),
                                                 fps=30)
        vis.append(v.float())
        aud.append(a.float())
        lengths.append(v.shape[0])
        targets.append(shot_scores.float().reshape(1))
    return torch.cat(vis), torch.cat(aud), torch.from_numpy(exclusive_offsets(lengths)), torch.cat(targets)


def train_step_batch(model, optimizer, items, device="cuda", samples=None):
    """One optimiser step on V videos at once: one upload of the collated rows, one forward / backward over the ragged
    batch, the loss = the mean of the per-video MSEs - its gradient is the average of the per-video gradients, i.e.
    what V ranks that take one video each hold after dist.allreduce_gradients (the same step up to summation order).
    Returns the per-video losses (a list of floats) from ONE download, after the step.  ``samples``: host sample ids
    [V] of the videos' Dropout masks, for a model after seed_dropout(seed) (None: the model's next V ids); with them the
    step IS the one V data-parallel ranks take with one video and its id each, Dropout included."""
    visual, audio, offsets, targets = collate_videos(items)
    table = ops.SeqTable(offsets, visual.shape[0], device)
    if samples is None:
        preds = model.train_rows(visual.to(device), audio.to(device), table)
    else:
        preds = model.train_rows(visual.to(device), audio.to(device), table, samples=samples)
    losses = ops.seq_mse(preds, targets.to(device), table)
    loss = losses.mean()
    optimizer.zero_grad()
    loss.backward()
    avd.allreduce_gradients(model)
    optimizer.step()
    return losses.detach().cpu().tolist()


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
                     optimizer="torch", max_grad_norm=None, skip_nonfinite=False, dropout_seed=None):
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
    seed.  torch's RNG is not consumed by Dropout.  None (the default): torch's generator draws the masks, as before."""
    import torch.distributed as tdist
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
                losses = train_step_batch(model, optimizer, items, device, **ids)
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
    """TVSumDataset-shaped items: ({"visual": [S,4096], "audio": [S,296]}, frame scores [n_frames] ~ U[1,5])."""

    def __init__(self, num_videos=8, shots=(20, 60), seed=5005, visual_dim=4096, audio_dim=296):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for _ in range(num_videos):
            s = int(torch.randint(shots[0], shots[1] + 1, (1,), generator=g))
            feats = {"visual": torch.randn(s, visual_dim, generator=g), "audio": torch.zeros(s, audio_dim)}
            self.items.append((feats, torch.rand(s * 30, generator=g) * 4 + 1))

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
