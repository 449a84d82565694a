"""What the launch wrappers of the ragged-batch layers refuse, one wrong thing at a time, on tensors of at most 16
elements: a host tensor, a wrong dtype, a non-contiguous tensor, a wrong length or shape, a tables object of the wrong
class or built with device="cpu".  The expected types are read off the wrappers as they were before they shared
ops._device_arg / ops._tables_arg: ValueError everywhere, except where a check is not the wrapper's own - seq_shift_rows
checks src's dtype through ops._f32 (TypeError), and seq_mse hands whatever is not an ops.SeqTable to numpy as host
offsets, which refuses an object that is no array with a TypeError.  The one refusal that changed its type: device
offsets handed to ops.EvalTables, now the ValueError of the other two plans.  Nothing is launched: the library is out of
reach while the refusals run.  One positive case covers the two places where the shared offsets base could go wrong without a
refusal: one SeqTable serving seq_mse and train_rows, and an EvalTables that starts after row 0."""
import numpy as np
import pytest
import torch

import eval_batch_inputs as ebi

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def _cases(dev):
    """[(label, call, expected exception type)]"""
    from avsum_amd import ops
    z = lambda *shape, dtype=F32: torch.zeros(shape, dtype=dtype, device=dev)
    fusion, fusion_cpu = ops.FusionTables([(0, 2, 0, 2)], dev), ops.FusionTables([(0, 2, 0, 2)], "cpu")
    evalt, evalt_cpu = ops.EvalTables([0, 4], dev), ops.EvalTables([0, 4], "cpu")
    seq, seq_cpu, seq3 = ops.SeqTable([0, 1, 4], 4, dev), ops.SeqTable([0, 1, 4], 4, "cpu"), ops.SeqTable([0, 1, 3], 3, dev)
    shot, shot_cpu = ops.ShotTables([0, 31], 15, dev), ops.ShotTables([0, 31], 15, "cpu")      # two cut slots
    one, one_cpu = ops.ShotTables([0, 1], 15, dev), ops.ShotTables([0, 1], 15, "cpu")          # one frame
    assert shot.cut_cap == 2 and one.frames == 1
    off_t = torch.tensor([0, 1, 4], dtype=I64, device=dev)
    V, T = ValueError, TypeError
    out = []

    def add(wrapper, label, exc, *args, **kw):
        out.append((f"{wrapper.__name__}: {label}", lambda: wrapper(*args, **kw), exc))

    v = z(2, 4)
    for label, exc, args in (
            ("v on the host", V, (fusion, v.cpu(), v)), ("a on the host", V, (fusion, v, v.cpu())),
            ("v float64", V, (fusion, v.double(), v)), ("a int32", V, (fusion, v, z(2, 4, dtype=I32))),
            ("v not contiguous", V, (fusion, z(4, 2).t(), v)), ("a not contiguous", V, (fusion, v, z(4, 2).t())),
            ("v a vector", V, (fusion, z(8), v)), ("other column counts", V, (fusion, v, z(2, 3))),
            ("too few rows", V, (fusion, z(1, 4), v)), ("tables of another class", V, (evalt, v, v)),
            ("tables on the host", V, (fusion_cpu, v, v)), ("host pairs for tables", V, ([(0, 2, 0, 2)], v, v))):
        add(ops.fusion_batch, label, exc, *args)

    x = z(4)
    for label, exc, args in (
            ("x on the host", V, (x.cpu(), [0, 4])), ("x int32", V, (z(4, dtype=I32), [0, 4])),
            ("x not contiguous", V, (z(8)[::2], [0, 4])), ("x a matrix", V, (z(2, 2), [0, 4])),
            ("offsets past the end", V, (x, [0, 5])), ("offsets decrease", V, (x, [0, 3, 2])),
            ("offsets tensor on the host", V, (x, torch.tensor([0, 4]))),
            ("offsets tensor int32", V, (x, torch.tensor([0, 4], dtype=I32, device=dev))),
            ("offsets tensor not contiguous", V, (x, torch.tensor([0, 9, 4, 9], device=dev)[::2])),
            ("offsets tensor a matrix", V, (x, torch.tensor([[0, 4]], device=dev))),
            ("offsets tensor empty", V, (x, z(0, dtype=I64)))):
        add(ops.segment_mean_mask, label, exc, *args)

    for label, exc, args in (
            ("pred on the host", V, (evalt, x.cpu(), x)), ("target on the host", V, (evalt, x, x.cpu())),
            ("pred float64", V, (evalt, x.double(), x)), ("target int32", V, (evalt, x, z(4, dtype=I32))),
            ("pred not contiguous", V, (evalt, z(8)[::2], x)), ("target not contiguous", V, (evalt, x, z(8)[::2])),
            ("pred a matrix", V, (evalt, z(4, 1), x)), ("pred too short", V, (evalt, z(3), z(3))),
            ("target of another length", V, (evalt, x, z(5))), ("tables of another class", V, (seq, x, x)),
            ("tables on the host", V, (evalt_cpu, x, x))):
        add(ops.eval_counts, label, exc, *args)

    src = z(4, 4)
    for label, exc, args in (
            ("src on the host", V, (src.cpu(), 0, 4, off_t, 1)), ("src float64", T, (src.double(), 0, 4, off_t, 1)),
            ("src with a column stride", V, (z(4, 4).t(), 0, 4, off_t, 1)), ("src a vector", V, (z(16), 0, 4, off_t, 1)),
            ("columns outside src", V, (src, 2, 3, off_t, 1)), ("direction 2", V, (src, 0, 4, off_t, 2)),
            ("offsets_t on the host", V, (src, 0, 4, off_t.cpu(), 1)), ("offsets_t int32", V, (src, 0, 4, off_t.int(), 1)),
            ("offsets_t not contiguous", V, (src, 0, 4, torch.tensor([0, 9, 4, 9], device=dev)[::2], 1)),
            ("offsets_t a matrix", V, (src, 0, 4, off_t.view(1, 3), 1)), ("offsets_t of one entry", V, (src, 0, 4, off_t[:1], 1)),
            ("out of another shape", V, (src, 0, 4, off_t, 1, z(4, 3)))):
        add(ops.seq_shift_rows, label, exc, *args)

    y = z(2)
    for label, exc, args in (
            ("scores on the host", V, (x.cpu(), y, seq)), ("targets on the host", V, (x, y.cpu(), seq)),
            ("scores float64", V, (x.double(), y, seq)), ("targets float64", V, (x, y.double(), seq)),
            ("scores not contiguous", V, (z(8)[::2], y, seq)), ("targets not contiguous", V, (x, z(4)[::2], seq)),
            ("scores a matrix", V, (z(4, 1), y, seq)), ("three targets", V, (x, z(3), seq)),
            ("table of other rows", V, (x, y, seq3)), ("host offsets of other rows", V, (x, y, [0, 1, 3])),
            ("table on the host", V, (x, y, seq_cpu)), ("tables of another class", T, (x, y, evalt))):
        add(ops.seq_mse, label, exc, *args)

    frame = z(1, 2, 2, 3, dtype=U8)
    for label, exc, args in (
            ("frames on the host", V, (frame.cpu(), one)), ("frames float32", V, (z(1, 2, 2, 3), one)),
            ("frames not contiguous", V, (z(1, 2, 3, 2, dtype=U8).transpose(2, 3), one)),
            ("four channels", V, (z(1, 2, 2, 4, dtype=U8), one)), ("a single image", V, (z(2, 2, 3, dtype=U8), one)),
            ("another frame count", V, (frame, shot)), ("step 0", V, (frame, one, 0)),
            ("tables of another class", V, (frame, seq)), ("tables on the host", V, (frame, one_cpu))):
        add(ops.hsv_frame_diff_batch, label, exc, *args)

    sums = z(1, 3, dtype=I32)
    for label, exc, args in (
            ("sums on the host", V, (one, sums.cpu(), 4.0)), ("sums int64", V, (one, sums.long(), 4.0)),
            ("sums not contiguous", V, (one, z(3, 2, dtype=I32)[:, :1].t(), 4.0)),
            ("sums of two frames", V, (one, z(2, 3, dtype=I32), 4.0)), ("sums flat", V, (one, z(3, dtype=I32), 4.0)),
            ("no pixels", V, (one, sums, 0.0)), ("tables of another class", V, (evalt, sums, 4.0)),
            ("tables on the host", V, (one_cpu, sums, 4.0))):
        add(ops.shot_cuts_batch, label, exc, *args)

    cuts, totals = z(2, dtype=I64), z(1, 4, dtype=I64)
    for label, exc, args in (
            ("cuts on the host", V, (shot, cuts.cpu(), totals)), ("totals on the host", V, (shot, cuts, totals.cpu())),
            ("cuts int32", V, (shot, cuts.int(), totals)), ("totals float32", V, (shot, cuts, totals.float())),
            ("cuts not contiguous", V, (shot, z(4, dtype=I64)[::2], totals)),
            ("totals not contiguous", V, (shot, cuts, z(4, 2, dtype=I64)[:, :1].t())),
            ("three cuts", V, (shot, z(3, dtype=I64), totals)), ("totals of three columns", V, (shot, cuts, z(1, 3, dtype=I64))),
            ("tables of another class", V, (seq, cuts, totals)), ("tables on the host", V, (shot_cpu, cuts, totals))):
        add(ops.shot_tables, label, exc, *args)

    rows, index, count = z(4, 2), z(2, dtype=I64), torch.ones(1, dtype=I64, device=dev)
    for label, exc, args in (
            ("src on the host", V, (rows.cpu(), index, count)), ("index on the host", V, (rows, index.cpu(), count)),
            ("count on the host", V, (rows, index, count.cpu())), ("out on the host", V, (rows, index, count, z(2, 2).cpu())),
            ("index int32", V, (rows, index.int(), count)), ("count int32", V, (rows, index, count.int())),
            ("src not contiguous", V, (z(2, 4).t(), index, count)), ("index not contiguous", V, (rows, z(4, dtype=I64)[::2], count)),
            ("index a matrix", V, (rows, z(2, 1, dtype=I64), count)), ("count of two entries", V, (rows, index, z(2, dtype=I64))),
            ("src a scalar", V, (z(), index, count)), ("empty rows", V, (z(4, 0), index, count)),
            ("out of another shape", V, (rows, index, count, z(3, 2))), ("out float64", V, (rows, index, count, z(2, 2, dtype=F64))),
            ("out not contiguous", V, (rows, index, count, z(2, 2).t()))):
        add(ops.gather_rows, label, exc, *args)

    # the offsets of a plan are a host array: a device tensor is refused by all three in the same words
    for cls, args in ((ops.EvalTables, (dev,)), (ops.SeqTable, (4, dev)), (ops.ShotTables, (15, dev))):
        add(cls, "device offsets", V, off_t, *args)
    return out


def test_wrappers_refuse_one_wrong_argument_at_a_time(dev, monkeypatch):
    from avsum_amd import ops
    cases = _cases(dev)
    assert len({label for label, _, _ in cases}) == len(cases)
    wrappers = {label.split(":")[0] for label, _, _ in cases}
    assert {"fusion_batch", "segment_mean_mask", "eval_counts", "seq_shift_rows", "seq_mse", "hsv_frame_diff_batch",
            "shot_cuts_batch", "shot_tables", "gather_rows"} <= wrappers

    def no_launch():
        raise AssertionError("a refusal test reached the library")
    monkeypatch.setattr(ops, "lib", no_launch)
    wrong = []
    for label, call, exc in cases:
        try:
            call()
        except (ValueError, TypeError) as e:
            if type(e) is not exc:
                wrong.append((label, type(e).__name__, str(e)))
        else:
            wrong.append((label, "accepted", ""))
    assert not wrong, wrong
    for cls in (ops.EvalTables, ops.SeqTable, ops.ShotTables):
        with pytest.raises(ValueError, match="HOST array"):
            cls(torch.tensor([0, 4], device=dev), device=dev)


def test_one_seq_table_and_a_late_start(dev):
    """Two videos of 1 and 3 rows: one SeqTable, built once, serves train_rows and seq_mse and gives what host offsets
    give; an EvalTables that starts at row 3 gives the counts of the same videos laid out from row 0."""
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    offsets = [0, 1, 4]
    table = ops.SeqTable(offsets, 4, dev)
    assert (table.nseq, table.rows, table.max_t) == (2, 4, 3) and table.offsets_t.tolist() == offsets
    torch.manual_seed(3)
    md = AVBiLSTMModel(visual_dim=64, audio_dim=24, hidden_dim=32).to(dev).eval()
    g = torch.Generator().manual_seed(4)
    v, a = torch.randn(4, 64, generator=g).to(dev), torch.randn(4, 24, generator=g).to(dev)
    scores = md.train_rows(v, a, table)
    assert scores.shape == (4,) and scores.requires_grad and torch.equal(scores, md.train_rows(v, a, offsets))
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        assert torch.equal(md(v[lo:hi][None], a[lo:hi][None]).reshape(-1), scores[lo:hi]), (lo, hi)
    targets = torch.tensor([0.25, 0.75], device=dev)
    losses = ops.seq_mse(scores, targets, table)
    assert torch.equal(losses, ops.seq_mse(scores, targets, offsets))
    p, y = scores.detach().cpu().numpy().astype(np.float64), np.repeat(targets.cpu().numpy().astype(np.float64), [1, 3])
    want = np.array([np.mean((p[lo:hi] - y[lo:hi]) ** 2) for lo, hi in zip(offsets[:-1], offsets[1:])])
    got = losses.detach().cpu().numpy()
    # the kernel sums in fp64 and rounds once (tests/test_gpu_train_batch.py holds every video to one ulp)
    assert (np.abs(got - want) <= np.spacing(want.astype(np.float32))).all(), (got, want)
    leaf = scores.detach().requires_grad_(True)
    ops.seq_mse(leaf, targets, table).sum().backward()
    dwant = np.concatenate([2.0 / (hi - lo) * (p[lo:hi] - y[lo:hi]) for lo, hi in zip(offsets[:-1], offsets[1:])])
    # four fp32 roundings of 2^-24 each, doubled (the bound of tests/test_gpu_train_batch.py)
    assert (np.abs(leaf.grad.cpu().numpy() - dwant) <= 5e-7 * np.abs(dwant)).all(), (leaf.grad, dwant)

    pairs = [ebi.video(31, 2, 5), ebi.video(32, 4, 5)]
    pred, target, off0 = ebi.layout(pairs)
    pred3, target3, off3 = ebi.layout(pairs, first=3)
    assert list(off0) == [0, 2, 6] and list(off3) == [3, 5, 9]
    late = ops.EvalTables(off3, dev)
    assert (late.nvideos, late.rows, late.max_t, late.ntiles) == (2, 9, 4, 2) and late.offsets_t.tolist() == [3, 5, 9]
    counts = ops.eval_counts(late, torch.from_numpy(pred3).to(dev), torch.from_numpy(target3).to(dev)).cpu()
    from0 = ops.eval_counts(ops.EvalTables(off0, dev), torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)).cpu()
    assert torch.equal(counts, from0)
    assert counts.numpy().tolist() == ebi.brute_counts_batch(pairs).tolist()
