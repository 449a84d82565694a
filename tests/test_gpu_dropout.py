"""Counter-based Dropout on the MI355X (libavsum_dropout.so): the three kernels against the host definition and against
the mask-tensor kernels they replace, bit for bit; every refusal; AVBiLSTMModel with seed_dropout; the training script
with dropout_seed.  Nothing here needs a tolerance: the mask is integer arithmetic and a comparison, and applying it is
the same fp32 product either way.  Layouts come from dropout_inputs (see its docstring)."""
import copy

import numpy as np
import pytest
import torch

import dropout_inputs as di
from avsum_amd import dropout

pytestmark = pytest.mark.gpu

SMALL = dict(visual_dim=64, audio_dim=24, hidden_dim=32)
SEED, P = 2024, 0.3


def _table(dev, offsets=di.OFFSETS):
    from avsum_amd import ops
    return ops.SeqTable(offsets, int(offsets[-1]), dev)


def _host(samples, branch, offsets=di.OFFSETS, cols=di.SMALL_COLS, seed=SEED, p=P):
    return torch.from_numpy(dropout.keep_mask_host(seed, p, samples, branch, offsets, cols))


# --------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("branch", [0, 1])
@pytest.mark.parametrize("by", ["base", "table"])
def test_keep_mask_equals_the_host_definition(dev, branch, by):
    table = _table(dev)
    host_ids = 5 if by == "base" else di.SAMPLE_TABLE
    samples = 5 if by == "base" else dropout.sample_table(di.SAMPLE_TABLE, 4, dev)
    buf = torch.full((di.BUFFER_ROWS, di.BUFFER_COLS), di.SENTINEL, device=dev)
    view = buf[:33, 4:4 + di.SMALL_COLS]
    got = dropout.keep_mask(SEED, P, samples, branch, table.offsets_t, out=view)
    assert got is view
    want = _host(host_ids, branch)
    assert torch.equal(view.cpu(), want)
    assert set(want.unique().tolist()) == {0.0, dropout.scale(P)}
    whole = buf.cpu()
    assert (whole[:, :4] == di.SENTINEL).all() and (whole[:, 36:] == di.SENTINEL).all()      # the sentinel columns
    assert (whole[33:] == di.SENTINEL).all()                                                  # the rows after 33
    # allocated by the wrapper from the table: the same mask
    assert torch.equal(dropout.keep_mask(SEED, P, samples, branch, table, di.SMALL_COLS).cpu(), want)
    if by == "table":
        assert torch.equal(want[0], want[26])          # videos 0 and 3 share the id 7: the same row 0
        assert not torch.equal(want[0], want[1])
        assert not torch.equal(want, _host(di.SAMPLE_TABLE, 1 - branch))


def test_keep_mask_large_case_and_p_zero(dev):
    off = di.large_offsets()
    table = _table(dev, off)
    ids = [(3 * v) % 50 + (v % 3 << 32) for v in range(di.LARGE_VIDEOS)]
    got = dropout.keep_mask(SEED, P, dropout.sample_table(ids, di.LARGE_VIDEOS, dev), 1, table, di.LARGE_COLS)
    assert torch.equal(got.cpu(), _host(ids, 1, off, di.LARGE_COLS))
    got = dropout.keep_mask(SEED, P, 2 ** 40, 0, table, di.LARGE_COLS)
    assert torch.equal(got.cpu(), _host(2 ** 40, 0, off, di.LARGE_COLS))
    ones = dropout.keep_mask(SEED, 0.0, 0, 0, _table(dev), di.SMALL_COLS)
    assert torch.equal(ones.cpu(), torch.ones(33, di.SMALL_COLS))


def _planted(rows, cols, dev, seed):
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    specials = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0]
    for i in range(60):                     # kept and dropped positions both get every special value
        flat[(i * 17) % flat.numel()] = specials[i % len(specials)]
    return x.to(dev)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("branch", [0, 1])
def test_apply_equals_mul_by_the_mask(dev, branch):
    from avsum_amd import ops
    table = _table(dev)
    samples = dropout.sample_table(di.SAMPLE_TABLE, 4, dev)
    x = _planted(33, di.SMALL_COLS, dev, 1)
    mask = dropout.keep_mask(SEED, P, samples, branch, table, di.SMALL_COLS)
    want = ops.mul(x, mask)
    assert torch.isnan(want).any() and torch.isinf(want).any()
    got = dropout.apply(x, SEED, P, samples, branch, table)
    assert _same_bits(got, want)
    assert _same_bits(dropout.apply(x, SEED, P, samples, branch, table.offsets_t), want)
    inplace = x.clone()
    assert dropout.apply(inplace, SEED, P, samples, branch, table, out=inplace) is inplace
    assert _same_bits(inplace, want)
    # a column slice of a wider buffer, in and out
    wide = torch.full((33, di.BUFFER_COLS), di.SENTINEL, device=dev)
    wide[:, 4:36] = x
    out = torch.full((33, 48), di.SENTINEL, device=dev)
    dropout.apply(wide[:, 4:36], SEED, P, samples, branch, table, out=out[:, 8:40])
    assert _same_bits(out[:, 8:40].contiguous(), want)
    assert (out[:, :8] == di.SENTINEL).all() and (out[:, 40:] == di.SENTINEL).all()


@pytest.mark.parametrize("branch", [0, 1])
def test_relu_bwd_equals_relu_dropout_bwd_with_the_mask(dev, branch):
    from avsum_amd import ops
    table = _table(dev)
    dy = _planted(33, di.SMALL_COLS, dev, 2)
    relu_out = torch.relu(_planted(33, di.SMALL_COLS, dev, 3))           # zeros, -0.0 -> 0, NaN and Inf stay
    mask = dropout.keep_mask(SEED, P, 9, branch, table, di.SMALL_COLS)
    want = ops.relu_dropout_bwd(dy, relu_out, mask)
    got = dropout.relu_bwd(dy, relu_out, SEED, P, 9, branch, table)
    assert _same_bits(got, want)
    assert (got == 0).any() and (got != 0).any()


def test_every_refusal_raises(dev):
    from avsum_amd import _dropout_abi as abi
    table = _table(dev)
    good = torch.zeros(33, 32, device=dev)
    with pytest.raises(abi.AvsdError, match="multiple of 4"):                       # cols % 4
        dropout.keep_mask(SEED, P, 0, 0, table, out=torch.zeros(33, 30, device=dev))
    with pytest.raises(abi.AvsdError, match="row stride"):                          # a stride that is no multiple of 4
        dropout.keep_mask(SEED, P, 0, 0, table, out=torch.zeros(33, 42, device=dev)[:, :32])
    with pytest.raises(abi.AvsdError, match="16-byte"):                             # a misaligned pointer
        dropout.keep_mask(SEED, P, 0, 0, table, out=torch.zeros(33, 40, device=dev)[:, 1:33])
    with pytest.raises(abi.AvsdError, match="16-byte"):
        dropout.apply(torch.zeros(33, 40, device=dev)[:, 2:34], SEED, P, 0, 0, table)
    with pytest.raises(abi.AvsdError, match="row stride"):
        dropout.relu_bwd(good, torch.zeros(33, 34, device=dev)[:, :32], SEED, P, 0, 0, table)
    # what the wrappers cannot express goes to the entry point itself
    lib, off, ptr = abi.lib(), table.offsets_t.data_ptr(), good.data_ptr()
    tail = (SEED, dropout.threshold(P), dropout.scale(P), 0, 0, None, None)
    for args, word in (((ptr, 28, off, 4, 33, 32), "row stride"),                   # a stride below cols
                       ((ptr, 32, off, abi.MAX_SEQ + 1, 33, 32), "nseq"),           # nseq above the header's limit
                       ((None, 32, off, 4, 33, 32), "null"),                        # null pointers
                       ((ptr, 32, None, 4, 33, 32), "null"),
                       ((ptr, 32, off, 4, -1, 32), "negative"),                     # negative sizes
                       ((ptr, 32, off, 4, 33, -4), "negative")):
        with pytest.raises(abi.AvsdError, match=word):
            abi.check(lib.avsd_keep_mask_f32(*args, *tail), "avsd_keep_mask_f32")
    with pytest.raises(abi.AvsdError, match="null"):
        abi.check(lib.avsd_dropout_fwd_f32(None, 32, ptr, 32, off, 4, 33, 32, *tail), "avsd_dropout_fwd_f32")
    with pytest.raises(abi.AvsdError, match="null"):
        abi.check(lib.avsd_relu_dropout_bwd_f32(ptr, 32, None, 32, ptr, 32, off, 4, 33, 32, *tail),
                  "avsd_relu_dropout_bwd_f32")
    # and what the wrappers refuse themselves, before the library is asked
    for bad in (dict(samples=-1), dict(samples=1 << 63), dict(samples=torch.zeros(3, dtype=torch.int64, device=dev)),
                dict(branch=2), dict(seed=-1), dict(p=1.0), dict(offsets=table.offsets_t.cpu()),
                dict(offsets=_table(dev, [0, 32]))):
        kw = dict(seed=SEED, p=P, samples=0, branch=0, offsets=table)
        kw.update(bad)
        with pytest.raises(ValueError):
            dropout.apply(good, **kw)
    with pytest.raises(ValueError):
        dropout.apply(good.cpu(), SEED, P, 0, 0, table)
    with pytest.raises(ValueError):
        dropout.sample_table([1, 2, 3.5, 4], 4, dev)
    torch.cuda.synchronize()
    assert (good == 0).all()                            # no refused call wrote anything


# --------------------------------------------------------------------------- the model
def _model_case(dev):
    from avsum_amd.models.av_model import AVBiLSTMModel
    torch.manual_seed(3)
    model = AVBiLSTMModel(**SMALL).to(dev).train()
    g = torch.Generator().manual_seed(4)
    v = torch.randn(33, SMALL["visual_dim"], generator=g).to(dev)
    a = torch.randn(33, SMALL["audio_dim"], generator=g).to(dev)
    w = torch.randn(33, generator=g).to(dev)
    return model, v, a, w


def _scores_and_grads(model, v, a, w, **kw):
    model.zero_grad()
    out = model.train_rows(v, a, di.OFFSETS, **kw)
    (out * w).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad()
    return out.detach().clone(), grads


@pytest.mark.parametrize("ids", [None, di.SAMPLE_TABLE], ids=["consecutive", "given"])
def test_train_rows_seeded_equals_injected_keep_masks(dev, ids):
    model, v, a, w = _model_case(dev)
    assert len(model.state_dict()) == 28
    table = _table(dev)
    hidden = SMALL["hidden_dim"]
    samples = 0 if ids is None else dropout.sample_table(ids, 4, dev)
    keep = tuple(dropout.keep_mask(SEED, P, samples, b, table, hidden) for b in (0, 1))
    assert not torch.equal(keep[0], keep[1])
    model._dropout_keep = keep
    try:
        want, want_grads = _scores_and_grads(model, v, a, w)
    finally:
        del model._dropout_keep
    model.seed_dropout(SEED)
    kw = {} if ids is None else {"samples": ids}
    got, got_grads = _scores_and_grads(model, v, a, w, **kw)
    assert model.counter_dropout.next_sample == (4 if ids is None else 0)
    assert torch.equal(got, want)
    assert len(got_grads) == 28
    for k in want_grads:
        assert torch.equal(got_grads[k], want_grads[k]), k
    # an injected pair still wins over the seed, and the state dict holds no trace of it
    model._dropout_keep = tuple(torch.ones_like(k) for k in keep)
    try:
        ones, _ = _scores_and_grads(model, v, a, w)
    finally:
        del model._dropout_keep
    assert not torch.equal(ones, want) and len(model.state_dict()) == 28
    with pytest.raises(ValueError):
        model.train_rows(v, a, di.OFFSETS, samples=[1, 2, 3])
    with pytest.raises(ValueError):
        model.train_rows(v, a, di.OFFSETS, samples=[1, 2, -3, 4])
    model.seed_dropout(None)
    with pytest.raises(ValueError):
        model.train_rows(v, a, di.OFFSETS, samples=[1, 2, 3, 4])


def test_per_video_forwards_equal_the_batched_pass(dev):
    model, v, a, _ = _model_case(dev)
    model.seed_dropout(SEED)
    alone = [model(v[lo:hi][None], a[lo:hi][None]).detach().reshape(-1)
             for lo, hi in zip(di.OFFSETS[:-1], di.OFFSETS[1:])]
    assert model.counter_dropout.state() == (SEED, P, 4)
    model.seed_dropout(SEED)
    together = model.train_rows(v, a, di.OFFSETS).detach()
    assert torch.equal(torch.cat(alone), together)
    # the same seed again: the same scores; another seed, or other ids: others
    model.seed_dropout(SEED)
    assert torch.equal(model.train_rows(v, a, di.OFFSETS).detach(), together)
    assert not torch.equal(model.train_rows(v, a, di.OFFSETS).detach(), together)            # ids 4 .. 7 now
    model.seed_dropout(SEED + 1)
    assert not torch.equal(model.train_rows(v, a, di.OFFSETS).detach(), together)
    # a saved state replays: ids 4 .. 7 of SEED again
    model.seed_dropout(SEED)
    model.counter_dropout.load_state((SEED, P, 4))
    replay = model.train_rows(v, a, di.OFFSETS).detach()
    assert torch.equal(replay, model.train_rows(v, a, di.OFFSETS, samples=[4, 5, 6, 7]).detach())
    # forward(sample=...) names the id itself
    lo, hi = di.OFFSETS[1], di.OFFSETS[2]
    assert torch.equal(model(v[lo:hi][None], a[lo:hi][None], sample=1).detach().reshape(-1), together[lo:hi])


def test_eval_mode_ignores_the_seed(dev):
    model, v, a, _ = _model_case(dev)
    model.eval()
    with torch.no_grad():
        plain = model(v[None, :24], a[None, :24])
    plain_rows = model.train_rows(v, a, di.OFFSETS).detach()
    model.seed_dropout(SEED)
    with torch.no_grad():
        assert torch.equal(model(v[None, :24], a[None, :24]), plain)
    assert torch.equal(model.train_rows(v, a, di.OFFSETS).detach(), plain_rows)
    assert model.counter_dropout.next_sample == 0


def test_unseeded_model_draws_with_torch_as_before(dev):
    from avsum_amd.models._scorer_train import dropout_keep
    model, v, a, _ = _model_case(dev)
    assert model.counter_dropout is None
    model.seed_dropout(SEED).seed_dropout(None)
    assert model.counter_dropout is None
    hidden = SMALL["hidden_dim"]
    torch.manual_seed(77)
    got = model(v[None, :24], a[None, :24]).detach()
    after = torch.cuda.get_rng_state(dev)
    torch.manual_seed(77)
    keep = (dropout_keep((24, hidden), dev), dropout_keep((24, hidden), dev))
    assert torch.equal(torch.cuda.get_rng_state(dev), after)            # the RNG was consumed exactly so
    model._dropout_keep = keep
    try:
        want = model(v[None, :24], a[None, :24]).detach()
    finally:
        del model._dropout_keep
    assert torch.equal(got, want)
    # seeded, the model leaves torch's generator alone
    model.seed_dropout(SEED)
    model(v[None, :24], a[None, :24])
    assert torch.equal(torch.cuda.get_rng_state(dev), after)


# --------------------------------------------------------------------------- the script
def _run_script(monkeypatch, base, ds, videos_per_step, dev):
    """One epoch of train_on_dataset(dropout_seed=SEED); returns (per-step losses, {video key: sample id}, the
    (lengths, ids) of every batched step)."""
    from avsum_amd.scripts import train_av_model as tr
    ids, batches, losses = {}, [], []
    real_step, real_batch = tr.train_step, tr.train_step_batch

    def key(features):
        return float(features["visual"].sum())

    def spy_step(model, optimizer, features, frame_scores, device="cuda", sample=None):
        ids[key(features)] = sample
        return real_step(model, optimizer, features, frame_scores, device, sample=sample)

    def spy_batch(model, optimizer, items, device="cuda", samples=None):
        for (features, _), s in zip(items, samples):
            ids[key(features)] = s
        batches.append(([f["visual"].shape[0] for f, _ in items], list(samples)))
        return real_batch(model, optimizer, items, device, samples=samples)

    with monkeypatch.context() as patch:
        patch.setattr(tr, "train_step", spy_step)
        patch.setattr(tr, "train_step_batch", spy_batch)
        torch.manual_seed(21)
        tr.train_on_dataset(ds, epochs=1, lr=1e-3, model=copy.deepcopy(base), on_step=losses.append, device=dev,
                            videos_per_step=videos_per_step, dropout_seed=SEED)
    return losses, ids, batches


def test_script_sample_ids_do_not_depend_on_videos_per_step(dev, monkeypatch):
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts import train_av_model as tr
    ds = tr.SyntheticShotDataset(num_videos=11, shots=(4, 9), seed=5, visual_dim=SMALL["visual_dim"],
                                 audio_dim=SMALL["audio_dim"])                          # a batch of 8 and a short one of 3
    torch.manual_seed(3)
    base = AVBiLSTMModel(**SMALL)
    losses8, ids8, batches8 = _run_script(monkeypatch, base, ds, 8, dev)
    losses1, ids1, batches1 = _run_script(monkeypatch, base, ds, 1, dev)
    assert batches1 == [] and len(losses1) == 2 and len(losses8) == 2
    assert sorted(ids8.values()) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]                  # 8 * batch + position
    assert [b[1] for b in batches8] == [list(range(8)), [8, 9, 10]]
    assert sorted(ids1.values()) == [0, 8]                                              # position 0 of each batch
    for video, sample in ids1.items():
        assert ids8[video] == sample                                                    # the same video, the same id
    # ... and so the same masks: the rows of video 0 in the batch's masks are the masks of that id alone
    hidden = SMALL["hidden_dim"]
    for lengths, samples in batches8:
        off = np.concatenate([[0], np.cumsum(lengths)])
        for branch in (0, 1):
            batch = dropout.keep_mask(SEED, P, dropout.sample_table(samples, len(samples), dev), branch,
                                      _table(dev, off), hidden)
            alone = dropout.keep_mask(SEED, P, samples[0], branch, _table(dev, [0, lengths[0]]), hidden)
            assert torch.equal(batch[:lengths[0]], alone)
    # two identical runs: identical per-step losses
    again8, again_ids8, _ = _run_script(monkeypatch, base, ds, 8, dev)
    assert again8 == losses8 and again_ids8 == ids8
    again1, _, _ = _run_script(monkeypatch, base, ds, 1, dev)
    assert again1 == losses1
    assert all(np.isfinite(losses8)) and all(np.isfinite(losses1))
