"""Host side of the batched training step (no GPU): collate_videos, the offsets table, and which videos of a drawn batch
train_on_dataset(videos_per_step=k) hands to train_step_batch."""
import pytest
import torch
from torch.utils.data import DataLoader


def _items(lengths, seed=3, dv=12, da=5):
    g = torch.Generator().manual_seed(seed)
    return [({"visual": torch.randn(s, dv, generator=g), "audio": torch.randn(s, da, generator=g)},
             torch.rand(s * 30, generator=g) * 4 + 1) for s in lengths]


def test_collate_videos_rows_offsets_targets():
    from avsum_amd.scripts import train_av_model as tr
    from avsum_amd.utils.alignments import align_shots_to_annotations
    lengths = [5, 1, 9, 2]
    items = _items(lengths)
    visual, audio, offsets, targets = tr.collate_videos(items)
    assert offsets.dtype == torch.int64 and offsets.tolist() == [0, 5, 6, 15, 17]
    assert visual.dtype == audio.dtype == targets.dtype == torch.float32
    assert visual.shape == (17, 12) and audio.shape == (17, 5) and targets.shape == (4,)
    assert not visual.is_cuda and not audio.is_cuda and not targets.is_cuda
    for v, (feats, frame_scores) in enumerate(items):
        a, b = offsets[v], offsets[v + 1]
        assert torch.equal(visual[a:b], feats["visual"]) and torch.equal(audio[a:b], feats["audio"])
        want = align_shots_to_annotations([(0, lengths[v])], frame_scores.numpy(), 30).float()
        assert want.shape == (1,) and torch.equal(targets[v:v + 1], want)


def test_collate_videos_refuses_bad_batches():
    from avsum_amd.scripts import train_av_model as tr
    good = _items([4, 3])
    empty = ({"visual": torch.zeros(0, 12), "audio": torch.zeros(0, 5)}, torch.ones(30))
    with pytest.raises(ValueError, match="empty"):
        tr.collate_videos([good[0], empty])
    with pytest.raises(ValueError, match="widths"):
        tr.collate_videos([good[0], _items([3], dv=13)[0]])
    with pytest.raises(ValueError, match="widths"):
        tr.collate_videos([good[0], _items([3], da=6)[0]])
    with pytest.raises(ValueError):
        tr.collate_videos([({"visual": torch.zeros(3, 12), "audio": torch.zeros(4, 5)}, torch.ones(90))])
    with pytest.raises(ValueError):
        tr.collate_videos([])


def test_seq_table_validates_on_the_host():
    from avsum_amd import ops
    t = ops.SeqTable([0, 1, 24, 26, 33], 33, "cpu")
    assert (t.nseq, t.rows, t.max_t) == (4, 33, 23) and t.lengths.tolist() == [1, 23, 2, 7]
    assert t.offsets_t.dtype == torch.int64 and t.offsets_t.tolist() == [0, 1, 24, 26, 33]
    assert ops.SeqTable(torch.tensor([0, 3]), None, "cpu").rows == 3
    for bad, rows in (([0, 4, 4, 9], 9),      # an empty video
                      ([1, 4, 9], 9),         # does not start at 0
                      ([0, 5, 3, 9], 9),      # decreases
                      ([0, 4, 8], 9),         # does not end at R
                      ([0], 0), ([], 0)):     # no video
        with pytest.raises(ValueError):
            ops.SeqTable(bad, rows, "cpu")


def test_select_items_rule():
    from avsum_amd.scripts.train_av_model import select_items
    batch = list("abcdefgh")
    assert select_items(batch, 0, 1, 8) == batch                      # every video the loader drew
    assert select_items(batch, 0, 1, 3) == list("abc")
    assert select_items(batch, 1, 2, 3) == list("bdf")                # (rank + j * world) % 8
    assert select_items(batch, 0, 2, 8) == list("aceg")               # positions wrap: duplicates dropped
    assert select_items(batch, 1, 2, 8) == list("bdfh")
    short = list("xyz")
    assert select_items(short, 0, 1, 8) == short                      # a short last batch yields fewer
    assert select_items(short, 1, 2, 2) == list("yx")                 # 1, then (1 + 2) % 3 = 0
    assert select_items(short, 1, 2, 4) == list("yxz")                # 1, 0, 2, then 1 again: dropped


class _TinyScorer(torch.nn.Module):
    """CPU stand-in with AVBiLSTMModel's call signature (the HIP model has no CPU path)."""

    def __init__(self):
        super().__init__()
        self.v = torch.nn.Linear(12, 6)
        self.a = torch.nn.Linear(5, 6)
        self.head = torch.nn.Linear(6, 1)

    def forward(self, visual, audio):
        return torch.sigmoid(self.head(torch.relu(self.v(visual) + self.a(audio)))).squeeze()


def _key(item):
    return float(item[0]["visual"].sum())


def _run_spied(monkeypatch, ds, k, epochs, seed, on_step=None):
    from avsum_amd.scripts import train_av_model as tr
    batches, single = [], []

    def spy_batch(model, optimizer, items, device="cuda"):
        batches.append([_key(it) for it in items])
        return [float(len(items))] * len(items)

    real_step = tr.train_step

    def spy_step(model, optimizer, features, frame_scores, device="cuda"):
        single.append(float(features["visual"].sum()))
        return real_step(model, optimizer, features, frame_scores, device)

    monkeypatch.setattr(tr, "train_step_batch", spy_batch)
    monkeypatch.setattr(tr, "train_step", spy_step)
    torch.manual_seed(seed)
    tr.train_on_dataset(ds, epochs=epochs, lr=1e-2, model=_TinyScorer(), device="cpu", videos_per_step=k, on_step=on_step)
    return batches, single


def _drawn_batches(ds, epochs, generator=None):
    """The batches train_on_dataset's loader draws, in order (same RNG state, same loader arguments)."""
    loader = DataLoader(ds, batch_size=8, shuffle=True, generator=generator, collate_fn=lambda items: items)
    return [[_key(it) for it in items] for _ in range(epochs) for items in loader]


@pytest.mark.parametrize("k", [2, 3, 8])
def test_videos_per_step_selection_world1(monkeypatch, k):
    from avsum_amd.scripts import train_av_model as tr
    ds = tr.SyntheticShotDataset(num_videos=11, shots=(4, 9), seed=5, visual_dim=12, audio_dim=5)   # 8 + a short 3
    seen = []
    batches, single = _run_spied(monkeypatch, ds, k, 2, 21, on_step=seen.append)
    torch.manual_seed(21)
    _TinyScorer()           # (the run above built its model after seeding: the loader starts from the same RNG state)
    drawn = _drawn_batches(ds, 2)
    assert single == [] and len(batches) == len(drawn) == 4
    for got, batch in zip(batches, drawn):
        assert got == batch[:min(k, len(batch))]                       # positions 0 .. k - 1 at world 1
        assert len(set(got)) == len(got)                               # no video twice in a step
    assert [len(b) for b in batches] == [min(k, 8), min(k, 3)] * 2     # the short last batch yields fewer
    assert seen == [float(len(b)) for b in batches]                    # on_step: the mean of the per-video losses
    if k == 8:
        every = sorted(_key(ds[i]) for i in range(len(ds)))
        assert sorted(batches[0] + batches[1]) == every                # k = 8 trains on every video the loader draws


@pytest.mark.parametrize("rank", [0, 1])
def test_videos_per_step_selection_faked_world2(monkeypatch, rank):
    import torch.distributed as tdist
    from avsum_amd import dist as avd
    from avsum_amd.scripts import train_av_model as tr
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **kw: 2)
    monkeypatch.setattr(tdist, "get_rank", lambda *a, **kw: rank)
    monkeypatch.setattr(tdist, "broadcast", lambda *a, **kw: None)
    monkeypatch.setattr(avd, "broadcast_module", lambda *a, **kw: None)
    ds = tr.SyntheticShotDataset(num_videos=11, shots=(4, 9), seed=5, visual_dim=12, audio_dim=5)
    batches, single = _run_spied(monkeypatch, ds, 3, 1, 33)
    torch.manual_seed(33)
    _TinyScorer()
    seed = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64)      # the shuffle seed the loop draws (and broadcasts)
    drawn = _drawn_batches(ds, 1, torch.Generator().manual_seed(int(seed.item())))
    assert single == [] and len(batches) == len(drawn) == 2
    full, short = drawn
    assert batches[0] == [full[(rank + 2 * j) % 8] for j in range(3)]
    want_short = []
    for j in range(3):
        x = short[(rank + 2 * j) % 3]
        if x not in want_short:
            want_short.append(x)
    assert batches[1] == want_short and len(set(batches[1])) == len(batches[1])
    assert batches[0][0] == full[rank]                                 # position `rank` first: the video the k = 1 loop takes


def test_videos_per_step_default_is_the_reference_loop(monkeypatch):
    from avsum_amd.scripts import train_av_model as tr
    ds = tr.SyntheticShotDataset(num_videos=11, shots=(4, 9), seed=5, visual_dim=12, audio_dim=5)
    batches, single = _run_spied(monkeypatch, ds, 1, 2, 21)
    torch.manual_seed(21)
    _TinyScorer()
    drawn = _drawn_batches(ds, 2)
    assert batches == []                                               # never the batched step
    assert single == [b[0] for b in drawn]                             # item 0 of every batch of 8, as before


@pytest.mark.parametrize("k", [0, 9, -1, 2.0, None])
def test_videos_per_step_out_of_range(k):
    from avsum_amd.scripts import train_av_model as tr
    ds = tr.SyntheticShotDataset(num_videos=3, shots=(4, 5), seed=5, visual_dim=12, audio_dim=5)
    with pytest.raises(ValueError, match="videos_per_step"):
        tr.train_on_dataset(ds, epochs=1, model=_TinyScorer(), device="cpu", videos_per_step=k)


def test_alias_packages_expose_the_new_names():
    import avsum_amd.scripts.train_av_model as real
    import scripts.train_av_model as alias
    import src.scripts.train_av_model as alias2
    for name in ("collate_videos", "train_step_batch", "train_on_dataset", "train_step"):
        assert getattr(alias, name) is getattr(real, name) and getattr(alias2, name) is getattr(real, name)


def test_new_entry_points_validate_before_launch():
    """Bad arguments come back as a status code before any HIP call (no GPU here)."""
    from avsum_amd import _abi
    lib = _abi.lib()
    fake = 4096   # a non-null "pointer" that is never dereferenced on the paths below
    ARG, SHAPE = -1, -2
    assert lib.avs_seq_shift_rows_f32(fake, 8, 0, 4, -1, fake, 1, 1, fake, 4, None) == SHAPE
    assert lib.avs_seq_shift_rows_f32(fake, 8, 6, 4, 10, fake, 1, 1, fake, 4, None) == SHAPE     # window past the row
    assert lib.avs_seq_shift_rows_f32(fake, 8, 0, 4, 10, fake, 1, 1, fake, 3, None) == SHAPE     # out narrower than cols
    assert lib.avs_seq_shift_rows_f32(fake, 8, 0, 4, 10, fake, 1, 0, fake, 4, None) == ARG and b"direction" in lib.avs_last_error()
    assert lib.avs_seq_shift_rows_f32(None, 8, 0, 4, 10, fake, 1, 1, fake, 4, None) == ARG and b"null" in lib.avs_last_error()
    assert lib.avs_seq_shift_rows_f32(None, 8, 0, 4, 0, None, 0, 1, None, 4, None) == 0          # nothing to do
    assert lib.avs_seq_mse_f32(fake, fake, 0, -1, fake, 1, fake, None) == SHAPE
    assert lib.avs_seq_mse_f32(fake, fake, 2, 10, fake, 1, fake, None) == ARG and b"target_stride" in lib.avs_last_error()
    assert lib.avs_seq_mse_f32(fake, None, 0, 10, fake, 1, fake, None) == ARG
    assert lib.avs_seq_mse_f32(None, None, 0, 0, None, 0, None, None) == 0
    assert lib.avs_seq_mse_bwd_f32(fake, fake, fake, 0, 10, fake, -1, 5, fake, None) == SHAPE
    assert lib.avs_seq_mse_bwd_f32(fake, fake, fake, 3, 10, fake, 1, 5, fake, None) == ARG
    assert lib.avs_seq_mse_bwd_f32(None, fake, fake, 0, 10, fake, 1, 5, fake, None) == ARG
    assert lib.avs_seq_mse_bwd_f32(None, None, None, 0, 0, None, 0, 0, None, None) == 0
