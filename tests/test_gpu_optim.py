"""The fused AdamW step on the MI355X (libavsum_optim.so through avsum_amd/optim.py) against adamw_reference in float64
within the project's bound (tests/optim_inputs.py), bit-reproducibility across table position and alignment, the norm
pass and the clip coefficient, the overflow skip, no host synchronisation, the scorer's training loop against
torch.optim.AdamW, checkpoint exchange with torch.optim.AdamW, and train_on_dataset(optimizer="fused")."""
import copy
import math

import numpy as np
import pytest
import torch

import optim_inputs as oi

pytestmark = pytest.mark.gpu

_RUNS = {}
_TABLE = []


def _table():
    if not _TABLE:
        _TABLE.append(oi.UnitTable())
    return _TABLE[0]


def _device_run(dev, weight_decay, betas, max_grad_norm):
    """The unit table through multi_tensor_adamw, STEPS steps: per step the downloaded buffers and stats.  Run once
    per setting and shared."""
    from avsum_amd import optim
    key = (weight_decay, betas, max_grad_norm)
    if key in _RUNS:
        return _RUNS[key]
    table = _table()
    p, m, v = table.params.to(dev), table.zeros.to(dev), table.zeros.to(dev)
    ws = optim.make_workspace([n for _, n in table.layout], dev)
    steps = []
    for s in range(oi.STEPS):
        g = table.grads[s].to(dev)
        optim.multi_tensor_adamw(table.views(p), table.views(g), table.views(m), table.views(v), ws, lr=oi.LR,
                                 betas=betas, eps=oi.EPS, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        steps.append({"params": p.cpu(), "exp_avg": m.cpu(), "exp_avg_sq": v.cpu(), "grads": g.cpu(),
                      "stats": optim.read_stats(ws)})
    _RUNS[key] = steps
    return steps


# --------------------------------------------------------------------------- 1. the unit table against float64
@pytest.mark.parametrize("case", oi.CASES, ids=[c[0] for c in oi.CASES])
def test_unit_table_against_float64(dev, case):
    from avsum_amd import optim
    _, weight_decay, betas, max_grad_norm = case
    table = _table()
    params, grads = table.views(table.params), [table.views(g) for g in table.grads]
    kw = dict(lr=oi.LR, betas=betas, eps=oi.EPS, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    ref64 = optim.adamw_reference(params, grads, dtype=torch.float64, **kw)
    cpu32 = oi.torch_adamw_fp32(params, grads, **kw)
    steps = _device_run(dev, weight_decay, betas, max_grad_norm)
    for s, got in enumerate(steps):
        views = {kind: table.views(got[kind]) for kind in oi.KINDS}
        worst, misses = oi.check_step(views, ref64[s], cpu32[s])
        print(f"fused AdamW, case {case[0]}, step {s + 1}: worst err / bound = {worst:.3f}")
        assert not misses, misses[:5]
        for kind in oi.KINDS:
            assert table.sentinels_intact(got[kind]), (kind, s)
        assert torch.equal(got["grads"], table.grads[s])          # the gradient is read, never rescaled
        assert got["stats"]["applied"] == s + 1 and got["stats"]["skipped"] == 0
        assert (got["stats"]["norm"] is None) == (max_grad_norm is None)


# --------------------------------------------------------------------------- 2. position, alignment, repetition
def _place(tensors, offsets, dev, fill=oi.SENTINEL):
    """One device buffer holding ``tensors`` back to back, tensor i at element offset offsets[i] behind a 16-byte
    boundary; returns (buffer, views)."""
    starts, cursor = [], 0
    for t, off in zip(tensors, offsets):
        cursor = -(-cursor // 4) * 4 + 4 + off
        starts.append(cursor)
        cursor += t.numel()
    buf = torch.full((cursor + 4,), fill, dtype=torch.float32)
    for t, lo in zip(tensors, starts):
        buf[lo:lo + t.numel()] = t
    buf = buf.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf[lo:lo + t.numel()] for t, lo in zip(tensors, starts)]


def _run_order(dev, params, grads_per_step, order, offsets, max_grad_norm=1.0):
    """multi_tensor_adamw over the tensors in ``order`` (indices into params) at the given alignments; returns the final
    p, m, v per ORIGINAL index, and the stats."""
    from avsum_amd import optim
    _, p = _place([params[i] for i in order], offsets, dev)
    _, m = _place([torch.zeros_like(params[i]) for i in order], offsets, dev)
    _, v = _place([torch.zeros_like(params[i]) for i in order], offsets, dev)
    ws = optim.make_workspace([params[i].numel() for i in order], dev)
    for grads in grads_per_step:
        _, g = _place([grads[i] for i in order], offsets, dev)
        optim.multi_tensor_adamw(p, g, m, v, ws, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                                 max_grad_norm=max_grad_norm)
    out = {}
    for j, i in enumerate(order):
        out[i] = (p[j].cpu(), m[j].cpu(), v[j].cpu())
    return out, optim.read_stats(ws)


def test_same_bytes_wherever_a_tensor_sits(dev):
    gen = torch.Generator().manual_seed(11)
    sizes = [3 * 4096 + 1, 5, 4097, 64, 4096]                     # tensor 0: three full chunks and a tail of one
    params = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[oi.wide_grads((n,), gen) for n in sizes] for _ in range(2)]
    first, s_first = _run_order(dev, params, grads, [0, 1, 2, 3, 4], [0, 1, 0, 2, 0])     # first row, 16-byte aligned
    last, s_last = _run_order(dev, params, grads, [1, 2, 3, 4, 0], [1, 0, 2, 0, 3])       # last row, offset 3
    again, s_again = _run_order(dev, params, grads, [0, 1, 2, 3, 4], [0, 1, 0, 2, 0])
    assert s_first["clip"] < 1.0 and s_first["clip"] == s_last["clip"]
    for a, b in zip(first[0], last[0]):
        assert torch.equal(a, b)
    for i in range(len(sizes)):
        for a, b in zip(first[i], again[i]):
            assert torch.equal(a, b)
    assert s_first == s_again
    # the norm partials depend on a chunk's length only: one tensor, aligned and not, the same bits of norm2
    _, s0 = _run_order(dev, params, grads[:1], [0], [0])
    _, s3 = _run_order(dev, params, grads[:1], [0], [3])
    assert s0["norm2"] == s3["norm2"] and s0["norm2"] > 0


# --------------------------------------------------------------------------- 3. the norm and the clip coefficient
def test_norm_and_clip_coefficient(dev):
    table = _table()
    _, weight_decay, betas, max_grad_norm = oi.CASES[2]
    steps = _device_run(dev, weight_decay, betas, max_grad_norm)
    n = sum(count for _, count in table.layout)
    for s, got in enumerate(steps):
        want_clip, norm2 = oi.clip_coefficient([g for g in table.views(table.grads[s]) if g.numel()], max_grad_norm)
        rel = abs(got["stats"]["norm"] ** 2 - norm2) / norm2
        print(f"step {s + 1}: norm^2 relative error {rel:.3e} (allowed {n * 2.0 ** -52:.3e}), clip "
              f"{got['stats']['clip']!r} against {want_clip!r}")
        assert rel <= n * 2.0 ** -52
        assert want_clip < 0.1
        assert abs(got["stats"]["clip"] - float(np.float32(want_clip))) <= 2 * oi.ulp32(want_clip)
    # a max_grad_norm above the norm: the unclipped run, bit for bit
    plain = _device_run(dev, weight_decay, betas, None)
    loose = _device_run(dev, weight_decay, betas, 1e6)
    for a, b in zip(plain, loose):
        assert b["stats"]["clip"] == 1.0 and b["stats"]["norm"] > 100.0
        for kind in oi.KINDS:
            assert torch.equal(a[kind], b[kind]), kind


# --------------------------------------------------------------------------- 4. the overflow skip
def _small_problem(dev, seed, steps):
    gen = torch.Generator().manual_seed(seed)
    shapes = [(5,), (4097,), (64, 3), (4096,)]
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[oi.wide_grads(s, gen) for s in shapes] for _ in range(steps)]
    params = [torch.nn.Parameter(x.clone().to(dev)) for x in init]
    return init, grads, params


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone().to(p.device)


def _state_lists(opt, params):
    return {"params": [p.detach().cpu() for p in params], "exp_avg": [opt.state[p]["exp_avg"].cpu() for p in params],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"].cpu() for p in params]}


@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_step_is_skipped(dev, poison):
    from avsum_amd import optim
    init, grads, params = _small_problem(dev, 21, 3)
    grads[1][1][1234] = poison                                    # one element of one tensor
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt = optim.FusedAdamW(params, skip_nonfinite=True, **kw)
    _set_grads(params, grads[0])
    opt.step()
    before, versions = _state_lists(opt, params), [p._version for p in params]
    assert opt.stats()["applied"] == 1 and all(v == 1 for v in versions)
    _set_grads(params, grads[1])
    opt.step()
    after = _state_lists(opt, params)
    for kind in oi.KINDS:
        for a, b in zip(before[kind], after[kind]):
            assert torch.equal(a, b), kind                        # every byte of every p, m, v
    assert [p._version for p in params] == versions
    stats = opt.stats()
    assert stats["skipped"] == 1 and stats["applied"] == 1 and not math.isfinite(stats["norm2"])
    _set_grads(params, grads[2])
    opt.step()
    assert [p._version for p in params] == [v + 1 for v in versions]
    stats = opt.stats()
    assert stats["skipped"] == 1 and stats["applied"] == 2
    # the next finite step is the reference's step t = applied + 1 = 2
    ref64 = optim.adamw_reference(init, grads, skip_nonfinite=True, **kw)
    assert [h["applied"] for h in ref64] == [1, 1, 2]
    cpu32 = oi.torch_adamw_fp32(init, [grads[0], grads[2]], **kw)
    worst, misses = oi.check_step(_state_lists(opt, params), ref64[-1], cpu32[-1])
    print(f"step after a skipped one ({poison}): worst err / bound = {worst:.3f}")
    assert not misses, misses[:5]


# --------------------------------------------------------------------------- 5. no host synchronisation
@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["plain", "clip"])
def test_step_does_not_synchronise_or_allocate(dev, max_grad_norm):
    from avsum_amd import optim
    _, grads, params = _small_problem(dev, 31, 1)
    opt = optim.FusedAdamW(params, lr=1e-3, max_grad_norm=max_grad_norm)
    _set_grads(params, grads[0])
    opt.step()
    torch.cuda.synchronize(dev)
    allocated = torch.cuda.memory_allocated(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated(dev) == allocated
    assert opt.stats()["applied"] == 3


def test_step_refuses_what_it_cannot_run(dev):
    from avsum_amd import optim
    _, grads, params = _small_problem(dev, 33, 1)
    opt = optim.FusedAdamW(params, lr=1e-3)
    assert opt.step() is None and opt.stats()["applied"] == 0     # no gradient anywhere: nothing runs, nothing counts
    _set_grads(params, [grads[0][0], None, grads[0][2], None])
    before = [p.detach().clone() for p in params]
    opt.step()                                                    # parameters without a gradient are left out
    assert [torch.equal(a, b) for a, b in zip(before, params)] == [False, True, False, True]
    assert [p._version for p in params] == [1, 0, 1, 0]
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    params[2].grad = torch.zeros(3, 64, device=dev).t()           # the right shape, strided
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    assert opt.stats()["applied"] == 1
    opt.param_groups[0]["lr"] = -1.0                              # hyper-parameters are read, and checked, every call
    with pytest.raises(ValueError, match="lr"):
        opt.step()


# --------------------------------------------------------------------------- 6. the scorer's training loop
def test_scorer_training_matches_torch_adamw(dev):
    from avsum_amd import ops, optim
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.scripts.train_av_model import train_step
    dims = dict(visual_dim=128, audio_dim=40, hidden_dim=64)
    torch.manual_seed(77)
    a = AVBiLSTMModel(**dims)
    b = AVBiLSTMModel(**dims)
    b.load_state_dict(a.state_dict())
    a, b = a.to(dev).train(), b.to(dev).train()
    opt_a = torch.optim.AdamW(a.parameters(), lr=1e-4)
    opt_b = optim.FusedAdamW(b.parameters(), lr=1e-4)
    assert len(list(b.parameters())) == 28
    gen = torch.Generator().manual_seed(3)
    t = 24
    got, want = [], []
    for step in range(6):
        if step != 1:                                             # step 2 sees the input of step 1 again
            feats = {"visual": torch.randn(t, 128, generator=gen), "audio": torch.randn(t, 40, generator=gen)}
            scores = torch.rand(t * 30, generator=gen) * 4 + 1
            keep = tuple(((torch.rand(t, 64, generator=gen) >= 0.3).float() / 0.7).to(dev) for _ in range(2))
        a._dropout_keep = b._dropout_keep = keep
        want.append(train_step(a, opt_a, feats, scores, dev))
        got.append(train_step(b, opt_b, feats, scores, dev))
    rel = max(abs(x - y) / abs(y) for x, y in zip(got, want))
    print("FusedAdamW against torch.optim.AdamW: max relative loss difference over 6 steps:", rel, got)
    assert rel < 1e-4, (got, want)
    # the same input twice: another loss, so the kernel-layout weight caches were rebuilt after the step
    assert got[1] != got[0] and want[1] != want[0]
    assert opt_b.stats()["applied"] == 6
    assert ops.lstm_split_errors(dev) == 0


# --------------------------------------------------------------------------- 7. checkpoint exchange
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_checkpoint_exchange_with_torch_adamw(dev, direction):
    from avsum_amd import optim
    init, grads, params = _small_problem(dev, 41, 3)
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    make = {"fused": lambda ps: optim.FusedAdamW(ps, **kw), "torch": lambda ps: torch.optim.AdamW(ps, **kw)}
    src, dst = direction.split("_to_")
    opt = make[src](params)
    for s in range(2):
        _set_grads(params, grads[s])
        opt.step()
    sd = copy.deepcopy(opt.state_dict())      # as a checkpoint on disk: torch's load_state_dict shares tensors it is given
    assert all(float(state["step"]) == 2.0 for state in sd["state"].values()) and len(sd["state"]) == len(params)
    others = [torch.nn.Parameter(p.detach().clone()) for p in params]
    other = make[dst](others)
    other.load_state_dict(sd)
    _set_grads(params, grads[2])
    _set_grads(others, grads[2])
    opt.step()
    other.step()
    ref64 = optim.adamw_reference(init, grads, **kw)
    cpu32 = oi.torch_adamw_fp32(init, grads, **kw)
    fused_opt, fused_params = (opt, params) if src == "fused" else (other, others)
    torch_opt, torch_params = (other, others) if src == "fused" else (opt, params)
    fused = _state_lists(fused_opt, fused_params)
    plain = {"params": [p.detach().cpu() for p in torch_params],
             "exp_avg": [torch_opt.state[p]["exp_avg"].cpu() for p in torch_params],
             "exp_avg_sq": [torch_opt.state[p]["exp_avg_sq"].cpu() for p in torch_params]}
    for name, lists in (("fused", fused), ("torch", plain)):
        worst, misses = oi.check_step(lists, ref64[-1], cpu32[-1])
        print(f"{direction}: third step of the {name} optimiser, worst err / bound = {worst:.3f}")
        assert not misses, (name, misses[:5])
    assert fused_opt.stats()["applied"] == 3
    assert float(torch_opt.state[torch_params[0]]["step"]) == 3.0


# --------------------------------------------------------------------------- 8. the script layer
def test_train_on_dataset_with_the_fused_optimizer(dev):
    from avsum_amd import ops
    from avsum_amd.models.av_model import AVBiLSTMModel
    from avsum_amd.optim import FusedAdamW
    from avsum_amd.scripts.train_av_model import SyntheticShotDataset, train_on_dataset
    torch.manual_seed(4)
    ds = SyntheticShotDataset(num_videos=8, shots=(5, 9), visual_dim=128, audio_dim=40)
    small = AVBiLSTMModel(visual_dim=128, audio_dim=40, hidden_dim=64)
    seen = []
    model = train_on_dataset(ds, epochs=1, model=small, on_step=seen.append, device=dev, optimizer="fused",
                             max_grad_norm=1.0, skip_nonfinite=True)
    assert len(seen) >= 1 and all(np.isfinite(x) for x in seen)
    assert isinstance(model.fused_optimizer, FusedAdamW)
    stats = model.fused_optimizer.stats()
    assert stats["applied"] == len(seen) and stats["skipped"] == 0 and 0.0 < stats["clip"] <= 1.0
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert ops.lstm_split_errors(dev) == 0
    with pytest.raises(ValueError, match="optimizer"):
        train_on_dataset(ds, epochs=1, model=small, device=dev, optimizer="adam")
    with pytest.raises(ValueError, match="fused"):
        train_on_dataset(ds, epochs=1, model=small, device=dev, max_grad_norm=1.0)
