"""Per-shot targets and the pairwise ranking loss on the MI355X (libavsum_loss.so through avsum_amd/loss.py): the kernels
against the host definitions - bit for bit where the arithmetic is integer or a single float64 expression (the targets,
the pair counts, the hinge gradient), within the bounds DERIVED in rank_loss_inputs elsewhere - batch invariance,
repeatability, the backward, and the training step that uses them.  Cases, references and bounds: rank_loss_inputs."""
import copy

import numpy as np
import pytest
import torch

import rank_loss_inputs as rli
from avsum_amd import loss as avloss

pytestmark = pytest.mark.gpu

SMALL = dict(visual_dim=64, audio_dim=24, hidden_dim=32)
SEED = 2024


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _fwd(dev, s, y, off, kind):
    return avloss.rank_loss_fwd(torch.tensor(s).to(dev), torch.tensor(y).to(dev), off, kind, rli.SCALE, rli.MARGIN)


# --------------------------------------------------------------------------- shot targets
@pytest.mark.parametrize("tables", ["host", "device"])
def test_shot_targets_equal_the_host_definition(dev, tables):
    ann, aoff, shots, soff, fps = rli.shot_batch()
    want, want_flags = avloss.shot_targets_host(ann, aoff, shots, soff, fps)
    assert want_flags.tolist() == [1, 0, 1] and np.isnan(want).sum() == 2
    nshots, extra = shots.shape[0], 5 if tables == "device" else 0
    buf = torch.full((nshots + extra + 16,), rli.SENTINEL, device=dev)
    fbuf = torch.full((3 + 8,), 9, dtype=torch.uint8, device=dev)
    out, fout = buf[8:8 + nshots + extra], fbuf[4:7]
    if tables == "device":           # tables at a capacity above S, as a detector leaves them: the rows past S are never read
        cap = np.concatenate([shots, np.full((extra, 2), 123456789, dtype=np.int64)])
        shot_arg, off_arg = torch.from_numpy(cap).to(dev), torch.from_numpy(soff).to(dev)
    else:
        shot_arg, off_arg = shots, soff
    got, flags = avloss.shot_targets(torch.from_numpy(ann).to(dev), aoff, shot_arg, off_arg, fps, out=out, flags_out=fout)
    assert got is out and flags is fout
    got_host = got.cpu().numpy()
    assert np.array_equal(np.isnan(got_host[:nshots]), np.isnan(want))
    keep = ~np.isnan(want)
    assert np.array_equal(got_host[:nshots][keep].view(np.int32), want[keep].view(np.int32))        # bit for bit
    assert flags.cpu().tolist() == want_flags.tolist()
    whole, fwhole = buf.cpu(), fbuf.cpu()
    assert (whole[:8] == rli.SENTINEL).all() and (whole[8 + nshots:] == rli.SENTINEL).all()
    assert (fwhole[:4] == 9).all() and (fwhole[7:] == 9).all()
    # allocated by the wrapper, a scalar frame rate, one video: the same values as on the host
    one, f1 = avloss.shot_targets(torch.from_numpy(ann[:aoff[1]]).to(dev), [0, aoff[1]], shots[:soff[1]], [0, soff[1]],
                                  29.97)
    w1, wf1 = avloss.shot_targets_host(ann[:aoff[1]], [0, aoff[1]], shots[:soff[1]], [0, soff[1]], 29.97)
    assert np.array_equal(one.cpu().numpy(), w1, equal_nan=True) and f1.cpu().tolist() == wf1.tolist()


# --------------------------------------------------------------------------- the ranking loss
def _check_against_host(name, kind, losses, g, pairs):
    s, y, off = rli.batch(name)
    want_l, want_g, want_p = rli.host_reference(name, kind)
    assert pairs.cpu().tolist() == want_p.tolist()
    got_l, got_g = losses.cpu().numpy().astype(np.float64), g.cpu().numpy()
    for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
        t, p = int(b - a), int(want_p[v])
        assert abs(got_l[v] - want_l[v]) <= rli.loss_bound(want_l[v], t), (name, kind, v, got_l[v], want_l[v])
        if kind == "hinge":
            assert np.array_equal(got_g[a:b].view(np.int32), want_g[a:b].astype(np.float32).view(np.int32)), (name, v)
        else:
            bound = np.array([rli.grad_bound(x, t, p, rli.SCALE) for x in want_g[a:b]])
            err = np.abs(got_g[a:b].astype(np.float64) - want_g[a:b])
            assert (err <= bound).all(), (name, kind, v, float(err.max()), float(bound.min()))
        if p == 0:
            assert got_l[v] == 0 and (got_g[a:b] == 0).all()


@pytest.mark.parametrize("kind", rli.KINDS)
@pytest.mark.parametrize("name", ["main", "tied"])
def test_rank_loss_matches_the_host_definition(dev, name, kind):
    s, y, off = rli.batch(name)
    losses, g, pairs = _fwd(dev, s, y, off, kind)
    assert losses.dtype == torch.float32 and g.dtype == torch.float32 and pairs.dtype == torch.int64
    _check_against_host(name, kind, losses, g, pairs)
    # two runs: identical bits
    again = _fwd(dev, s, y, off, kind)
    assert torch.equal(_bits(again[0]), _bits(losses)) and torch.equal(_bits(again[1]), _bits(g))
    assert torch.equal(again[2], pairs)


@pytest.mark.parametrize("kind", rli.KINDS)
def test_rank_loss_large_video(dev, kind):
    s, y, off = rli.batch("large")
    _check_against_host("large", kind, *_fwd(dev, s, y, off, kind))


@pytest.mark.parametrize("kind", rli.KINDS)
def test_a_video_gives_the_same_bits_alone_and_anywhere_in_a_batch(dev, kind):
    from avsum_amd import ops
    s, y, off = rli.batch("main")
    table = ops.RankTables(off, device=dev)                       # a prepared table is taken as it is
    losses, g, pairs = _fwd(dev, s, y, table, kind)
    order = [3, 0, 4, 2, 1]                                        # every video at another position
    s2 = np.concatenate([s[off[v]:off[v + 1]] for v in order])
    y2 = np.concatenate([y[off[v]:off[v + 1]] for v in order])
    off2 = np.concatenate([[0], np.cumsum([rli.LENGTHS[v] for v in order])])
    losses2, g2, pairs2 = _fwd(dev, s2, y2, off2, kind)
    for pos, v in enumerate(order):
        a, b = off[v], off[v + 1]
        l1, g1, p1 = _fwd(dev, s[a:b], y[a:b], [0, b - a], kind)
        assert torch.equal(_bits(l1), _bits(losses[v:v + 1])) and torch.equal(_bits(g1), _bits(g[a:b]))
        assert torch.equal(_bits(losses2[pos:pos + 1]), _bits(l1)) and int(p1) == int(pairs[v]) == int(pairs2[pos])
        assert torch.equal(_bits(g2[off2[pos]:off2[pos + 1]]), _bits(g1))


@pytest.mark.parametrize("kind", rli.KINDS)
def test_backward_scales_the_saved_gradient(dev, kind):
    s, y, off = rli.batch("main")
    scores = torch.tensor(s).to(dev).requires_grad_(True)
    targets = torch.tensor(y).to(dev)
    losses = avloss.rank_loss(scores, targets, off, kind, rli.SCALE, rli.MARGIN)
    fwd_l, g, _ = avloss.rank_loss_fwd(scores.detach(), targets, off, kind, rli.SCALE, rli.MARGIN)
    assert torch.equal(_bits(losses), _bits(fwd_l)) and losses.requires_grad
    dl = torch.tensor([3.0, -0.5, 0.25, 1.75, -2.0], device=dev)
    losses.backward(dl)
    want = torch.repeat_interleave(dl, torch.tensor(rli.LENGTHS, device=dev)) * g          # one fp32 product per row
    assert torch.equal(_bits(scores.grad), _bits(want)) and (scores.grad != 0).any()


def test_wrapper_refusals(dev):
    from avsum_amd import ops
    s, y = torch.rand(9, device=dev), torch.rand(9, device=dev)
    for bad in (dict(offsets=[0, 4, 8]), dict(offsets=ops.RankTables([0, 4, 9], device="cpu")), dict(kind="softmax"),
                dict(scale=-1.0), dict(margin=float("inf")), dict(targets=y[:8]), dict(targets=y.double()),
                dict(targets=y.cpu()), dict(scores=torch.rand(18, device=dev)[::2])):
        kw = dict(scores=s, targets=y, offsets=[0, 4, 9])
        kw.update(bad)
        with pytest.raises(ValueError):
            avloss.rank_loss(**kw)
    ann = torch.rand(6, device=dev)
    for bad in (dict(ann_offsets=[0, 5]), dict(fps=0), dict(fps=[30, 30]), dict(shots=[(-1, 4)]),
                dict(shot_offsets=[0, 2]), dict(annotations=ann.cpu()), dict(bin_seconds=0),
                dict(shots=torch.zeros(1, 2, dtype=torch.int32, device=dev))):
        kw = dict(annotations=ann, ann_offsets=[0, 6], shots=[(0, 40)], shot_offsets=[0, 1], fps=30)
        kw.update(bad)
        with pytest.raises(ValueError):
            avloss.shot_targets(**kw)


# --------------------------------------------------------------------------- the training step
def _dataset(with_shots=True, n=3):
    from avsum_amd.scripts import train_av_model as tr
    return tr.SyntheticShotDataset(num_videos=n, shots=(4, 9), seed=5, visual_dim=SMALL["visual_dim"],
                                   audio_dim=SMALL["audio_dim"], with_shots=with_shots)


def _model(dev):
    from avsum_amd.models.av_model import AVBiLSTMModel
    torch.manual_seed(3)
    return AVBiLSTMModel(**SMALL).to(dev).train()


@pytest.mark.parametrize("kind", rli.KINDS)
def test_train_step_batch_with_shot_targets_and_rank_loss(dev, kind):
    from avsum_amd.scripts import train_av_model as tr
    ds = _dataset()
    items = [ds[i] for i in range(len(ds))]
    model = _model(dev).seed_dropout(SEED)
    twin = copy.deepcopy(model)
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    weight = 0.7
    got = tr.train_step_batch(model, opt, items, dev, samples=[0, 1, 2], targets="shots", loss="mse+rank",
                              rank_weight=weight, rank_kind=kind, rank_scale=rli.SCALE, rank_margin=rli.MARGIN)
    assert any(not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))       # the step moved them
    # the same forward again on the untouched copy: the same Dropout masks (seed, ids), hence the same scores
    visual, audio, offsets, (ann, ann_off, shots) = tr.collate_videos(items, targets="shots")
    off = offsets.numpy()
    scores = twin.train_rows(visual.to(dev), audio.to(dev), off, samples=[0, 1, 2]).detach().cpu().numpy()
    y, flags = avloss.shot_targets_host(ann.numpy(), ann_off.numpy(), shots.numpy(), off, 30)
    assert not flags.any() and len(np.unique(y)) > len(items)
    rank, _, pairs = avloss.rank_loss_host(scores, y, off, kind, rli.SCALE, rli.MARGIN)
    assert (pairs > 0).all()
    for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
        mse = float(np.mean((scores[a:b].astype(np.float64) - y[a:b].astype(np.float64)) ** 2))
        want = mse + weight * rank[v]
        # seq_mse's one cast, the fp32 product and the fp32 sum: three roundings of values <= want; the rank loss's own
        bound = 3 * rli.W * want + weight * rli.loss_bound(rank[v], int(b - a))
        assert abs(got[v] - want) <= bound, (v, got[v], want, bound)
    # "rank" alone and "mse" on shot targets run too, and give the two parts
    for name in ("rank", "mse"):
        other = copy.deepcopy(twin)
        part = tr.train_step_batch(other, torch.optim.AdamW(other.parameters(), lr=1e-3), items, dev,
                                   samples=[0, 1, 2], targets="shots", loss=name, rank_kind=kind, rank_scale=rli.SCALE,
                                   rank_margin=rli.MARGIN)
        assert len(part) == 3 and all(np.isfinite(part))


def test_train_step_batch_defaults_are_the_parents_step(dev):
    from avsum_amd import dist as avd, ops
    from avsum_amd.scripts import train_av_model as tr
    ds = _dataset(with_shots=False)
    items = [ds[i] for i in range(len(ds))]
    new, old = _model(dev).seed_dropout(SEED), _model(dev).seed_dropout(SEED)
    opt_new = torch.optim.AdamW(new.parameters(), lr=1e-3)
    opt_old = torch.optim.AdamW(old.parameters(), lr=1e-3)
    got = tr.train_step_batch(new, opt_new, items, dev, samples=[4, 5, 6])
    # the step as it was before the objective became selectable, spelled out
    visual, audio, offsets, targets = tr.collate_videos(items)
    table = ops.SeqTable(offsets, visual.shape[0], dev)
    preds = old.train_rows(visual.to(dev), audio.to(dev), table, samples=[4, 5, 6])
    losses = ops.seq_mse(preds, targets.to(dev), table)
    opt_old.zero_grad()
    losses.mean().backward()
    avd.allreduce_gradients(old)
    opt_old.step()
    assert got == losses.detach().cpu().tolist()
    for (k, p), q in zip(new.named_parameters(), old.parameters()):
        assert torch.equal(p.detach(), q.detach()), k


def test_training_refusals_and_pass_through(dev):
    from avsum_amd.scripts import train_av_model as tr
    ds = _dataset(n=5)
    items = [ds[i] for i in range(3)]
    model = _model(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    for kw in (dict(loss="rank"), dict(loss="mse+rank"), dict(loss="huber", targets="shots"), dict(targets="rows")):
        with pytest.raises(ValueError):
            tr.train_step_batch(model, opt, items, dev, **kw)
    with pytest.raises(ValueError, match="needs features"):
        plain = _dataset(with_shots=False)
        tr.train_step_batch(model, opt, [plain[i] for i in range(3)], dev, targets="shots")
    with pytest.raises(ValueError, match="rank_loss: kind"):
        tr.train_step_batch(model, opt, items, dev, targets="shots", loss="rank", rank_kind="softmax")
    for kw in (dict(targets="shots"), dict(targets="shots", loss="rank")):
        with pytest.raises(ValueError, match="videos_per_step"):
            tr.train_on_dataset(ds, epochs=1, device=dev, videos_per_step=1, **kw)
    with pytest.raises(ValueError, match="needs targets='shots'"):
        tr.train_on_dataset(ds, epochs=1, device=dev, videos_per_step=4, loss="mse+rank")
    # the options travel through train_on_dataset: one epoch of five videos, one batched step
    seen = []
    tr.train_on_dataset(ds, epochs=1, lr=1e-3, model=_model(dev), on_step=seen.append, device=dev, videos_per_step=5,
                        dropout_seed=SEED, targets="shots", loss="mse+rank", rank_kind="hinge", rank_weight=0.5)
    assert len(seen) == 1 and np.isfinite(seen[0]) and seen[0] > 0
    # a shot that starts past the annotations: its target is NaN, the flag comes back with the losses and raises
    spoiled = [(dict(f), s) for f, s in items]
    table = spoiled[1][0]["shots"].clone()
    table[-1] = torch.tensor([10 ** 7, 10 ** 7 + 5])
    spoiled[1][0]["shots"] = table
    with pytest.raises(ValueError, match="video 1 of the batch"):
        tr.train_step_batch(model, opt, spoiled, dev, targets="shots", loss="mse")
