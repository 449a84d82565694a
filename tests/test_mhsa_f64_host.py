"""Host checks of what test_gpu_mhsa_f64.py holds the two fused attention kernels to (no GPU):

  * the float64 reference of mhsa_f64_inputs is the module's operation: oracle.scorer.mhsa_forward with projections
    that hand it the case's q, k and v;
  * the case list reaches every (head dim, wave count) instance of the fp32 kernel, by the rule of its host code, and
    lays the buffers out as the device test states;
  * the kernels' arithmetic restated in fp32 in its ONLINE form (tiles of 32 keys, running maximum, rescaled
    accumulator) lies within the bound at every case - the bound is not tighter than a correct kernel of that form;
  * every planted mistake lies outside the bound, for every (kernel, head dim) family, at the case that
    mhsa_f64_inputs.NOTICED_BY names for it - the bound is not slack enough to pass a wrong kernel."""
import math

import pytest
import torch

import mhsa_f64_inputs as mfi
from oracle import scorer as osc

FAMILIES = [(kind, d) for kind in mfi.KINDS for d in mfi.HEAD_DIMS]


def _spec(kind, d, where):
    regime, t, (b, heads) = where
    return (kind, d, t, b, heads, regime, True)


@pytest.mark.parametrize("spec", [("f32", 64, 33, 1, 2, "peaked", True), ("f16x2", 64, 17, 4, 4, "flat", True),
                                  ("f32", 128, 65, 1, 2, "ramp_up", True)])
def test_reference_is_the_modules_operation(spec):
    """oracle.scorer.mhsa_forward on a model of 4E features whose projections are selections: head h of its query is
    (2 q_h, 0, 0, 0), of its key (k_h, 0, 0, 0), of its value (v_h, 0, 0, 0), the output projection the identity.  Its
    head dim is 4 D, so its scores are 2 q.k / sqrt(4 D) = q.k / sqrt(D) to the bit (powers of two), and the first D
    columns of every head of its output are the operation the kernels compute."""
    case = mfi.make_case(spec)
    ref = mfi.reference(case)
    if case.kind == "f16x2":
        q, k, v = (mfi.emu_unpack(p).double() for p in mfi.packed(case))
    else:
        q, k, v = (x.reshape(case.rows, case.e).double() for x in (case.q, case.k, case.v))
    e, d, e4 = case.e, case.d, 4 * case.e
    x = torch.cat([q, k, v, torch.zeros_like(q)], 1).reshape(case.b, case.t, e4)
    cols = torch.arange(e)
    rows = (cols // d) * 4 * d + cols % d                 # where head h's D columns sit among the model's 4 D
    sd = {}
    for blk, (name, w) in enumerate((("query", 2.0), ("key", 1.0), ("value", 1.0))):
        m = torch.zeros(e4, e4, dtype=torch.float64)
        m[rows, blk * e + cols] = w
        sd[name + ".weight"], sd[name + ".bias"] = m, torch.zeros(e4, dtype=torch.float64)
    sd["out.weight"], sd["out.bias"] = torch.eye(e4, dtype=torch.float64), torch.zeros(e4, dtype=torch.float64)
    out = osc.mhsa_forward(sd, x, case.heads).reshape(case.rows, e4)
    assert out.dtype == torch.float64
    # float64 rounding of two summation orders of D (+ T) terms: 2^10 roundings cover it
    assert (out[:, rows] - ref).abs().max().item() <= 2.0 ** 10 * 2.0 ** -53 * max(1.0, ref.abs().max().item())
    keep = torch.ones(e4, dtype=torch.bool)
    keep[rows] = False
    assert (out[:, keep] == 0).all()


def test_case_list_reaches_every_instance_and_regime():
    for kind in mfi.KINDS:
        for d in mfi.HEAD_DIMS:
            short, long_ = mfi.specs(kind, d), mfi.long_specs(kind, d)
            assert len(set(short + long_)) == len(short + long_)
            waves = {(s[1], mfi.f32_waves(s[3], s[4], s[2])) for s in short + long_}
            assert waves == {(d, 2), (d, 4)}
            for bh, nw in ((mfi.SMALL, 2), (mfi.LARGE, 4)):          # each T on both instances
                assert {s[2] for s in short if (s[3], s[4]) == bh and s[5] == "flat" and s[6]} == set(mfi.T_LIST)
                assert all(mfi.f32_waves(*bh, t) == nw for t in mfi.T_LIST)
            assert all(mfi.f32_waves(s[3], s[4], s[2]) == 4 and s[2] == mfi.T_LONG for s in long_)
            regimes = {s[5] for s in short}
            assert regimes == set(mfi.REGIMES) - (set() if kind == "f16x2" else {"tiny_v"})
            assert any(not s[6] for s in short)
            # every strided regime of the issue's list runs on both fp32 instances
            for regime in ("flat", "peaked", "ramp_up", "ramp_down", "huge"):
                assert {mfi.f32_waves(s[3], s[4], s[2]) for s in short + long_ if s[5] == regime} == {2, 4}
            # ramp_up with the row maximum in a partial last tile
            assert any(s[5] == "ramp_up" and s[2] % mfi.KEY_TILE for s in short)
            for m in mfi.mistakes_of(kind):
                assert _spec(kind, d, mfi.NOTICED_BY[m]) in short, m
    # the rule itself, at its threshold: cdiv(t, 128) * heads * b against 16
    assert mfi.f32_waves(1, 2, 1024) == 4 and mfi.f32_waves(1, 2, 896) == 2 and mfi.f32_waves(4, 4, 1) == 4
    assert mfi.f32_waves(1, 15, 128) == 2 and mfi.f32_waves(1, 15, 129) == 4


@pytest.mark.parametrize("kind", mfi.KINDS)
def test_case_layout_is_the_one_the_device_test_states(kind):
    case = mfi.make_case((kind, 64, 33, 4, 4, "twins", True))
    c0 = 4 if kind == "f32" else 8
    assert (case.col0, case.ld, case.ocol0, case.ldo, case.rows, case.e) == (c0, 256 + 3 * c0, 4, 264, 132, 256)
    assert case.ld % (4 if kind == "f32" else 8) == 0 and case.ldo % 4 == 0
    qb, kb, vb, ctx = mfi.buffers(case)
    assert ctx.shape == (case.rows + 2, case.ldo) and (ctx == mfi.SENTINEL).all()
    for buf, x in ((qb, case.q), (kb, case.k), (vb, case.v)):
        assert buf.shape == (case.rows, case.ld)
        assert (buf[:, :c0] == mfi.SENTINEL).all() and (buf[:, c0 + case.e:] == mfi.SENTINEL).all()
        inner = buf[:, c0:c0 + case.e].contiguous()
        if kind == "f32":
            assert torch.equal(inner, x.reshape(case.rows, case.e))
        else:       # 22 significant bits of the value, hi | lo runs
            assert torch.equal(inner.view(torch.int32), mfi.emu_pack(x.reshape(case.rows, case.e)).view(torch.int32))
            assert (mfi.emu_unpack(inner) - x.reshape(case.rows, case.e)).abs().max().item() <= 2.0 ** -21 * x.abs().max().item()
    assert torch.equal(case.q[:, 3], case.q[:, 19]) and torch.equal(case.q[:, 0], case.q[:, 32])
    assert (3, 19) in case.twin_rows and (0, 32) in case.twin_rows and len(case.twin_rows) == 16 + 1
    assert torch.equal(case.k[0], case.k[2]) and not torch.equal(case.k[0], case.k[1]) and case.twin_batches == [(0, 2)]
    again = mfi.make_case(case.spec)
    assert torch.equal(case.q, again.q) and torch.equal(case.k, again.k) and torch.equal(case.v, again.v)
    flat = mfi.make_case((kind, 64, 129, 4, 4, "flat", False))
    assert (flat.col0, flat.ld, flat.ocol0, flat.ldo) == (0, 256, 0, 256)


def test_regimes_are_what_they_claim():
    """The scaled scores of each regime, in float64: flat stays flat, peaked and the ramps span about 40, huge overflows
    an unshifted exp, and the ramps put the row maximum in the last (first) key tile."""
    def scores(regime, t, d=64):
        case = mfi.make_case(("f32", d, t, 1, 2, regime, True))
        q, k = (x.permute(0, 2, 1, 3).double() for x in (case.q, case.k))
        return q @ k.transpose(-1, -2) / math.sqrt(d)
    s = scores("flat", 129)
    assert 0.25 < s.std().item() < 0.45 and torch.softmax(s, -1).max().item() < 8 / 129
    s = scores("peaked", 129)
    assert 25 < s.abs().max().item() < 60 and torch.softmax(s, -1).max(-1).values.median().item() > 0.5
    for t in (65, 257, mfi.T_LONG):
        for d in (64, 256):
            up, down = scores("ramp_up", t, d), scores("ramp_down", t, d)
            spread = (up.max(-1).values - up.min(-1).values)
            assert 25 < spread.median().item() < 60 and spread.max().item() < 160, (t, d)
            # the row maximum lies in the last (first) tile for most rows - at T = 65 and 257 the last tile holds ONE key -
            # and the tile maxima rise from tile to tile for the typical row
            last = -(-t // mfi.KEY_TILE) - 1
            assert (up.argmax(-1) // mfi.KEY_TILE == last).float().mean().item() > 0.8
            assert (down.argmax(-1) // mfi.KEY_TILE == 0).float().mean().item() > 0.8
            tiles = torch.stack([up[..., k0:k0 + mfi.KEY_TILE].max(-1).values for k0 in range(0, t, mfi.KEY_TILE)], -1)
            assert (tiles[..., 1:] > tiles[..., :-1]).float().mean().item() > 0.9
    s = scores("huge", 65)
    assert s.abs().max().item() > 150 and not torch.isfinite(torch.exp(s.float())).all()
    ek = mfi.make_case(("f32", 64, 31, 1, 2, "equal_keys", True))
    assert torch.equal(ek.k[:, 7], ek.k[:, 0])
    tv = mfi.make_case(("f16x2", 64, 33, 1, 2, "tiny_v", True))
    lo = mfi.packed(tv)[2].view(torch.float16).reshape(-1, 2, 8)[:, 1].float().abs()
    assert (lo[lo > 0] < 2.0 ** -14).all()          # every lo half of V is an fp16 denormal


@pytest.mark.parametrize("kind,d", FAMILIES)
def test_online_restatement_lies_within_the_bound_at_every_case(kind, d):
    """A correct kernel of the online form - another summation order, the rescaling by corr - fits the bound made from the
    global-maximum yardstick, at every case of the device test; the yardstick itself is finite and useful (its bound
    stays below 1e-3 of the output scale except in the ``huge`` regime, whose bound only has to be finite)."""
    worst = 0.0
    for spec in mfi.specs(kind, d) + mfi.long_specs(kind, d):
        case, ref, yard = mfi.bundle(spec)
        assert torch.isfinite(ref).all() and torch.isfinite(yard).all(), case.label
        ok, err, e, bound = mfi.check(case, mfi.restate(case, online=True), ref, yard)
        assert ok, f"{case.label}: online form err {err:.3e} > bound {bound:.3e} (yardstick {e:.3e})"
        assert mfi.check(case, yard, ref, yard)[0]
        scale = max(1.0, ref.abs().max().item())
        if case.regime != "huge":
            assert bound <= 1e-3 * scale, (case.label, bound)
        worst = max(worst, err / bound)
    print(f"\n{kind} D={d}: online form at most {worst:.2f} of the bound")
    if kind == "f32" and d == 64:       # a non-finite result is never within the bound
        bad = yard.clone()
        bad[0, 0] = float("nan")
        assert not mfi.check(case, bad, ref, yard)[0]


@pytest.mark.parametrize("kind,d", FAMILIES)
def test_each_planted_mistake_is_noticed(kind, d):
    """Which case notices which mistake: mhsa_f64_inputs.NOTICED_BY, the same table for every family."""
    table = []
    for mistake in mfi.mistakes_of(kind):
        case, ref, yard = mfi.bundle(_spec(kind, d, mfi.NOTICED_BY[mistake]))
        assert mfi.check(case, mfi.restate(case, online=True), ref, yard)[0], case.label
        ok, err, e, bound = mfi.check(case, mfi.restate(case, online=True, mistake=mistake), ref, yard)
        table.append(f"{mistake:22s} {case.label:44s} err {err:.2e}  bound {bound:.2e}  yardstick {e:.2e}")
        assert not ok, table[-1]
    print("\n" + "\n".join(table))
    assert set(mfi.mistakes_of(kind)) == set(mfi.MISTAKES) - (set() if kind == "f16x2" else set(mfi.F16X2_ONLY))
