"""A ragged batch of videos per optimiser step on the GPU: ops.seq_shift_rows, ops.seq_mse, AVBiLSTMModel.train_rows
against per-video B = 1 calls and the oracle, train_step_batch over several steps, train_on_dataset(videos_per_step=8)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OFFSETS = [0, 1, 24, 26, 33]       # a one-row video first, adjacent boundaries, a two-row video
SMALL = dict(visual_dim=64, audio_dim=24, hidden_dim=32)


# --------------------------------------------------------------------------- seq_shift_rows
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("col0,cols,width", [(8, 16, 40),     # float4 path: a window inside a wider matrix
                                             (3, 10, 37),     # scalar path: nothing a multiple of 4
                                             (0, 40, 40)])    # the whole row
def test_seq_shift_rows(dev, direction, col0, cols, width):
    from avsum_amd import ops
    g = torch.Generator().manual_seed(cols)
    src = torch.randn(OFFSETS[-1], width, generator=g)
    want = torch.zeros(OFFSETS[-1], cols)
    for a, b in zip(OFFSETS[:-1], OFFSETS[1:]):     # per video, with torch slicing
        seg = src[a:b, col0:col0 + cols]
        if b - a > 1:
            if direction == 1:
                want[a + 1:b] = seg[:-1]
            else:
                want[a:b - 1] = seg[1:]
    table = ops.SeqTable(OFFSETS, OFFSETS[-1], dev)
    got = ops.seq_shift_rows(src.to(dev), col0, cols, table.offsets_t, direction)
    assert got.shape == (OFFSETS[-1], cols) and torch.equal(got.cpu(), want)


def test_seq_shift_rows_many_blocks_and_single_video(dev):
    """More rows than one grid pass of float4s covers per block, 300 videos: every boundary row is zero, every other an
    exact copy; and V = 1 is the plain shift the one-video backward used to build with slicing."""
    from avsum_amd import ops
    g = torch.Generator().manual_seed(9)
    lengths = torch.randint(1, 40, (300,), generator=g).tolist()
    off = np.concatenate([[0], np.cumsum(lengths)])
    rows = int(off[-1])
    src = torch.randn(rows, 256, generator=g).to(dev)
    table = ops.SeqTable(off, rows, dev)
    first, last = torch.from_numpy(off[:-1]), torch.from_numpy(off[1:] - 1)
    for direction, edge in ((1, first), (-1, last)):
        got = ops.seq_shift_rows(src, 0, 256, table.offsets_t, direction).cpu()
        want = torch.roll(src.cpu(), direction, 0)
        want[edge] = 0
        assert torch.equal(got, want)
    one = ops.SeqTable([0, rows], rows, dev)
    got = ops.seq_shift_rows(src, 128, 128, one.offsets_t, 1).cpu()
    want = torch.zeros(rows, 128)
    want[1:] = src.cpu()[:-1, 128:]
    assert torch.equal(got, want)


# --------------------------------------------------------------------------- seq_mse
MSE_OFFSETS = OFFSETS + [OFFSETS[-1] + 1800]


@functools.lru_cache(None)
def _mse_inputs():
    g = torch.Generator().manual_seed(17)
    rows, nv = MSE_OFFSETS[-1], len(MSE_OFFSETS) - 1
    scores = torch.rand(rows, generator=g) * 0.98 + 0.01                  # in (0, 1)
    per_video = torch.rand(nv, generator=g) * 4 + 1                       # in [1, 5]
    per_row = torch.rand(rows, generator=g) * 4 + 1
    weights = torch.rand(nv, generator=g) + 0.5                           # upstream gradient of the losses
    return scores, per_video, per_row, weights


def _mse_ref(scores, targets_rows):
    """float64 on the same fp32 inputs: per-video loss, and d loss_v / d score_r."""
    p, y = scores.numpy().astype(np.float64), targets_rows.numpy().astype(np.float64)
    loss = np.array([np.mean((p[a:b] - y[a:b]) ** 2) for a, b in zip(MSE_OFFSETS[:-1], MSE_OFFSETS[1:])])
    grad = np.concatenate([2.0 / (b - a) * (p[a:b] - y[a:b]) for a, b in zip(MSE_OFFSETS[:-1], MSE_OFFSETS[1:])])
    return loss, grad


@pytest.mark.parametrize("form", ["per_video", "per_row"])
def test_seq_mse_forward(dev, form):
    from avsum_amd import ops
    scores, per_video, per_row, _ = _mse_inputs()
    lengths = torch.tensor(np.diff(MSE_OFFSETS))
    targets = per_video if form == "per_video" else per_row
    rows_t = torch.repeat_interleave(per_video, lengths) if form == "per_video" else per_row
    want, _ = _mse_ref(scores, rows_t)
    sd, td = scores.to(dev), targets.to(dev)
    got = ops.seq_mse(sd, td, MSE_OFFSETS)
    assert got.shape == (len(MSE_OFFSETS) - 1,) and got.dtype == torch.float32
    g = got.cpu().numpy()
    for v in range(len(want)):
        ulp = float(np.spacing(np.float32(want[v])))
        err = abs(float(g[v]) - want[v])
        print(f"seq_mse {form} video {v} T={int(lengths[v])}: got {g[v]!r} f64 {want[v]!r} err {err:.3e} ulp {ulp:.3e}")
        assert err <= ulp, (v, g[v], want[v])
    # a video's loss does not depend on where it sits, or on what else is in the batch
    for v, (a, b) in enumerate(zip(MSE_OFFSETS[:-1], MSE_OFFSETS[1:])):
        alone = ops.seq_mse(sd[a:b].contiguous(), td[v:v + 1] if form == "per_video" else td[a:b].contiguous(), [0, b - a])
        assert torch.equal(alone, got[v:v + 1]), v
    rev = ops.seq_mse(torch.cat([sd[33:], sd[:33]]), torch.cat([td[4:], td[:4]]) if form == "per_video"
                      else torch.cat([td[33:], td[:33]]), [0, 1800] + [1800 + o for o in OFFSETS[1:]])
    assert torch.equal(rev, torch.cat([got[4:], got[:4]]))


@pytest.mark.parametrize("form", ["per_video", "per_row"])
def test_seq_mse_backward(dev, form):
    from avsum_amd import ops
    scores, per_video, per_row, weights = _mse_inputs()
    lengths = torch.tensor(np.diff(MSE_OFFSETS))
    targets = per_video if form == "per_video" else per_row
    rows_t = torch.repeat_interleave(per_video, lengths) if form == "per_video" else per_row
    _, grad = _mse_ref(scores, rows_t)
    want = grad * torch.repeat_interleave(weights, lengths).numpy().astype(np.float64)
    sd = scores.to(dev).requires_grad_(True)
    losses = ops.seq_mse(sd, targets.to(dev), ops.SeqTable(MSE_OFFSETS, scores.shape[0], dev))
    (losses * weights.to(dev)).sum().backward()
    got = sd.grad.cpu().numpy().astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print(f"seq_mse backward {form}: max relative error {rel.max():.3e}")
    assert rel.max() <= 5e-7      # four fp32 roundings of 2^-24 each, doubled
    # .mean(): the average of the per-video gradients
    sd.grad = None
    ops.seq_mse(sd, targets.to(dev), MSE_OFFSETS).mean().backward()
    rel = np.abs(sd.grad.cpu().numpy().astype(np.float64) - grad / len(lengths)) / np.abs(grad / len(lengths))
    assert rel.max() <= 5e-7


def test_seq_mse_refuses_bad_arguments(dev):
    from avsum_amd import ops
    s = torch.rand(10, device=dev)
    with pytest.raises(ValueError):
        ops.seq_mse(s, torch.rand(3, device=dev), [0, 4, 10])          # neither per video nor per row
    with pytest.raises(ValueError):
        ops.seq_mse(s, torch.rand(2, device=dev), [0, 4, 9])           # does not end at R
    with pytest.raises(ValueError):
        ops.seq_mse(s, torch.rand(3, device=dev), [0, 4, 4, 10])       # an empty video
    with pytest.raises(ValueError):
        ops.seq_mse(s.cpu(), torch.rand(2), [0, 4, 10])                # no CPU fallback


# --------------------------------------------------------------------------- train_rows
CASES = {"small": (SMALL, [1, 23, 2, 7], 5),
         "full": ({}, [61, 1, 17], 9),                                  # hidden 256, 12 recurrences: the four-CU form
         "many": ({}, [2 + (i * 7) % 4 for i in range(53)], 11)}       # 212 recurrences: the one-CU resident form


def _seeded_scorer(seed, **kw):
    from avsum_amd.models.av_model import AVBiLSTMModel
    torch.manual_seed(seed)
    m = AVBiLSTMModel(**kw).eval()
    with torch.no_grad():       # as tests/test_gpu_models.py: scores away from 0.5, gradients of a useful size
        m.scorer[0].weight.mul_(6.0)
        m.scorer[2].weight.mul_(6.0)
    return m


@functools.lru_cache(None)
def _case(name):
    """Host-side inputs of one case, built once: model, rows, offsets, masks, per-video targets."""
    dims, lengths, seed = CASES[name]
    m = _seeded_scorer(seed, **dims)
    hidden = m.visual_fc[0].out_features
    rows = sum(lengths)
    g = torch.Generator().manual_seed(seed + 1)
    # (the tests move the model to the device in place: the oracle works on this host copy of its parameters)
    return dict(model=m, params={k: p.detach().clone() for k, p in m.named_parameters()}, lengths=lengths, offsets=[0] + np.cumsum(lengths).tolist(),
                v=torch.randn(rows, m.visual_fc[0].in_features, generator=g),
                a=torch.randn(rows, m.audio_fc[0].in_features, generator=g),
                keep_v=(torch.rand(rows, hidden, generator=g) >= 0.3).float() / 0.7,
                keep_a=(torch.rand(rows, hidden, generator=g) >= 0.3).float() / 0.7,
                targets=torch.rand(len(lengths), generator=g))


@functools.lru_cache(None)
def _oracle_grads(name):
    """torch autograd over the oracle restatement, called per video: the mean of the per-video mse_loss."""
    from oracle import scorer as osc
    c = _case(name)
    sd = {k: p.clone().requires_grad_(True) for k, p in c["params"].items()}
    v, a = c["v"].clone().requires_grad_(True), c["a"].clone().requires_grad_(True)
    losses, outs = [], []
    for i, (lo, hi) in enumerate(zip(c["offsets"][:-1], c["offsets"][1:])):
        out = osc.av_bilstm_forward_train(sd, v[lo:hi][None], a[lo:hi][None], c["keep_v"][lo:hi], c["keep_a"][lo:hi])
        out = out.reshape(-1)
        outs.append(out.detach())
        losses.append(torch.nn.functional.mse_loss(out, c["targets"][i].expand_as(out)))
    names = list(sd)
    grads = torch.autograd.grad(torch.stack(losses).mean(), [sd[k] for k in names] + [v, a], allow_unused=True)
    return dict(zip(names + ["dvis", "daud"], grads)), torch.cat(outs), torch.stack(losses).detach()


def _close(got, ref, what):
    """tests/test_gpu_models.py:145-146: |got - ref| <= 1e-4 * max|ref| + 1e-9."""
    ref = torch.zeros_like(got) if ref is None else ref
    scale = max(ref.abs().max().item(), 1e-8)
    err = (got - ref).abs().max().item()
    assert err <= 1e-4 * scale + 1e-9, (what, err, scale)


@pytest.mark.parametrize("name", ["small", "full", "many"])
def test_train_rows_forward_equals_per_video_calls(dev, name):
    c = _case(name)
    md = c["model"].to(dev).train()
    kv, ka = c["keep_v"].to(dev), c["keep_a"].to(dev)
    v, a = c["v"].to(dev), c["a"].to(dev)
    md._dropout_keep = (kv, ka)
    try:
        together = md.train_rows(v, a, c["offsets"])
        assert together.shape == (v.shape[0],) and together.dtype == torch.float32 and together.requires_grad
        assert torch.isfinite(together).all()
        for lo, hi in zip(c["offsets"][:-1], c["offsets"][1:]):
            md._dropout_keep = (kv[lo:hi], ka[lo:hi])
            one = md(v[lo:hi][None], a[lo:hi][None])
            assert torch.equal(one.reshape(-1), together[lo:hi]), (lo, hi)
    finally:
        del md._dropout_keep
        md.eval()


def test_train_rows_eval_mode_and_refusals(dev):
    """Eval mode with gradients: keep masks of ones, what forward() does for each video alone; bad offsets are refused
    on the host; forward() still refuses B > 1 in training."""
    c = _case("small")
    md = c["model"].to(dev).eval()
    v, a = c["v"].to(dev), c["a"].to(dev)
    got = md.train_rows(v, a, c["offsets"])
    assert got.requires_grad
    for lo, hi in zip(c["offsets"][:-1], c["offsets"][1:]):
        one = md(v[lo:hi][None], a[lo:hi][None])
        assert one.requires_grad and torch.equal(one.reshape(-1), got[lo:hi])
    for bad in ([0, 1, 1, 33], [1, 24, 33], [0, 24, 32], [0, 24, 34], [0]):
        with pytest.raises(ValueError):
            md.train_rows(v, a, bad)
    with pytest.raises(ValueError):
        md.train_rows(v, a[:-1], c["offsets"])
    with pytest.raises(RuntimeError):
        md.train_rows(v.cpu(), a.cpu(), c["offsets"])
    with pytest.raises(NotImplementedError):
        md.train()(v[:32].view(2, 16, -1), a[:32].view(2, 16, -1))
    md.eval()


@pytest.mark.parametrize("name", ["small", "full"])
def test_train_rows_gradients(dev, name):
    from avsum_amd import ops
    c = _case(name)
    ref, out_ref, loss_ref = _oracle_grads(name)
    md = c["model"].to(dev).train()
    params = dict(md.named_parameters())
    kv, ka = c["keep_v"].to(dev), c["keep_a"].to(dev)
    v, a = c["v"].to(dev).requires_grad_(True), c["a"].to(dev).requires_grad_(True)
    try:
        md._dropout_keep = (kv, ka)
        md.zero_grad()
        out = md.train_rows(v, a, c["offsets"])
        assert (out.detach().cpu() - out_ref).abs().max().item() < 1e-5
        losses = ops.seq_mse(out, c["targets"].to(dev), c["offsets"])
        assert (losses.detach().cpu() - loss_ref).abs().max().item() < 1e-6
        losses.mean().backward()
        got = {k: p.grad.detach().cpu().clone() for k, p in params.items()}
        assert len(got) == 28
        for k, g in got.items():
            _close(g, ref[k], k)
        if name == "small":
            _close(v.grad.cpu(), ref["dvis"], "dvis")
            _close(a.grad.cpu(), ref["daud"], "daud")
        # the same bar against the average of the V per-video B = 1 HIP backward passes
        acc = {k: torch.zeros_like(g) for k, g in got.items()}
        for i, (lo, hi) in enumerate(zip(c["offsets"][:-1], c["offsets"][1:])):
            md._dropout_keep = (kv[lo:hi], ka[lo:hi])
            md.zero_grad()
            one = md(v[lo:hi].detach()[None], a[lo:hi].detach()[None]).reshape(-1)
            torch.nn.functional.mse_loss(one, c["targets"][i].to(dev).expand_as(one)).backward()
            for k, p in params.items():
                acc[k] += p.grad.detach().cpu() / len(c["lengths"])
        for k, g in got.items():
            _close(g, acc[k], k + " (per-video HIP passes)")
    finally:
        del md._dropout_keep
        md.zero_grad()
        md.eval()


# --------------------------------------------------------------------------- the script layer
def test_train_step_batch_matches_oracle_loop(dev):
    """Six steps of three videos each (AdamW lr 1e-4, the mean of the per-video MSEs): the per-video loss trajectory of
    train_step_batch against a CPU loop over the oracle restatement."""
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import collate_videos, train_step_batch
    from oracle import scorer as osc
    torch.manual_seed(77)
    m = AVBiLSTMModel(visual_dim=128, audio_dim=40, hidden_dim=64)
    ref_params = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters()}
    opt_ref = torch.optim.AdamW(list(ref_params.values()), lr=1e-4)
    md = m.to(dev).train()
    opt = torch.optim.AdamW(md.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(3)
    got, want = [], []
    for step in range(6):
        lengths = [20 + 3 * step, 40 - 2 * step, 27 + step]
        items = [({"visual": torch.randn(t, 128, generator=g), "audio": torch.randn(t, 40, generator=g)},
                  torch.rand(t * 30, generator=g) * 4 + 1) for t in lengths]
        rows = sum(lengths)
        kv = (torch.rand(rows, 64, generator=g) >= 0.3).float() / 0.7
        ka = (torch.rand(rows, 64, generator=g) >= 0.3).float() / 0.7
        _, _, offsets, targets = collate_videos(items)
        per_video = []
        for i, (feats, _) in enumerate(items):
            lo, hi = int(offsets[i]), int(offsets[i + 1])
            out = osc.av_bilstm_forward_train(ref_params, feats["visual"][None], feats["audio"][None], kv[lo:hi], ka[lo:hi])
            per_video.append(torch.nn.functional.mse_loss(out, targets[i].expand_as(out)))
        opt_ref.zero_grad()
        torch.stack(per_video).mean().backward()
        opt_ref.step()
        want += [x.item() for x in per_video]
        md._dropout_keep = (kv.to(dev), ka.to(dev))
        losses = train_step_batch(md, opt, items, dev)
        assert isinstance(losses, list) and len(losses) == 3 and all(isinstance(x, float) for x in losses)
        got += losses
    rel = max(abs(x - y) / abs(y) for x, y in zip(got, want))
    print("train_step_batch: max relative loss difference over 6 steps x 3 videos:", rel)
    assert rel < 1e-4, (got, want)
    assert ops.lstm_split_errors(dev) == 0


def test_train_on_dataset_videos_per_step_8(dev):
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import SyntheticShotDataset, train_on_dataset
    torch.manual_seed(4)
    ds = SyntheticShotDataset(num_videos=8, shots=(5, 12), visual_dim=64, audio_dim=24)
    seen = []
    model = train_on_dataset(ds, epochs=2, model=AVBiLSTMModel(**SMALL), on_step=seen.append, device=dev,
                             videos_per_step=8)
    assert len(seen) == 2 and all(np.isfinite(x) and x > 0 for x in seen)
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert ops.lstm_split_errors(dev) == 0
