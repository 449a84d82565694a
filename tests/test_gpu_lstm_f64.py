"""The nine LSTM recurrence kernels, each against float64 (oracle.scorer.lstm_recurrence + autograd), fed the projected
input directly so that no GEMM stands between the kernel and the check.  The bound is scorer_f64_inputs.compare:
4 * e32 + 8 * eps32 * scale, e32 = the error of the same recurrence in fp32 on the CPU (tests/test_lstm_f64_host.py shows
that this bound rejects four planted formula mistakes at every hidden size used here and accepts fp32 itself).

Layout of every case: rows start at row 2 of the buffers, h goes to columns [4, 4 + ndir*H) of an output ndir*H + 9 wide
that is pre-filled with a sentinel - every other element must come back untouched.  Generic kernels: ndir 3, mask 0b010,
lengths [0, 1, 2, 9], hidden 1, 3, 20, 33, 90, 255, 257, 300, 600, 1024 (LSTM_AUTO and LSTM_STREAM); hidden 256: ndir 4,
mask 0b1010, lengths [700, 1, 0, 333, 2], every form, and one inference chain of 2000 steps.

Measured on an MI355X: the largest err / e32 per kernel family over all cases of this file, err and e32 both against the
float64 reference (the bound allows 4 plus the floor; nothing here needed more, and no case needed a note of its own):

    family              out    gates   cell   dxproj   dxproj, backward fed the reference's gates and cell
    generic forward     2.11   2.84    1.97                      (largest at H = 1024: one 1024-term fmaf chain per gate)
    generic backward                          1.46     1.59
    resident forward    1.01   1.21    1.11
    resident backward                         1.46     0.90
    split forward       1.01   1.21    1.11
    split backward                            1.46     0.90

The 2000-step inference chain: 0.80 on every form (err 1.7e-7, e32 2.1e-7).  Closest to the bound: the gates of the
generic forward at H = 1024, err 5.4e-7 against a bound of 1.7e-6."""
import pytest
import torch

import scorer_f64_inputs as sfi

pytestmark = pytest.mark.gpu

S = sfi.SENTINEL


def _api():
    from avsum_amd import _abi, ops
    return ops, _abi


def _report(family, label, name, err, e32, bound):
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO family={family!r} case={label!r} tensor={name} err={err:.3e} e32={e32:.3e} bound={bound:.3e} "
          f"err/e32={ratio:.2f}")


def _check(family, label, name, got, ref, cpu32, scale=None):
    ok, err, e32, bound = sfi.compare(got, ref, cpu32, scale)
    _report(family, label, name, err, e32, bound)
    assert ok, f"{family} {label} {name}: err {err:.3e} > bound {bound:.3e} (e32 {e32:.3e}, err/e32 {err / max(e32, 1e-300):.1f})"


class _Device:
    """A case's tensors on the device."""

    def __init__(self, case, dev):
        self.case = case
        self.xproj = case.xproj.to(dev)
        self.whh = case.whh.to(dev)
        self.whh_t = self.whh.transpose(1, 2).contiguous()
        self.dout = case.dout.to(dev)
        self.seq = torch.from_numpy(case.seq_rows).to(dev)
        self.dev = dev

    def blank(self):
        return torch.full((self.case.rows, self.case.ldo), S, dtype=torch.float32, device=self.dev)

    def args(self):
        c = self.case
        return c.hidden, c.ndir, c.reverse_mask, self.seq

    def infer(self, variant):
        ops, _ = _api()
        out = self.blank()
        ops.lstm(self.xproj, self.whh_t, *self.args(), out, self.case.out_col0, variant=variant)
        return out.cpu()

    def train(self, variant):
        ops, _ = _api()
        out = self.blank()
        gates, cell = ops.lstm_train_fwd(self.xproj, self.whh_t, *self.args(), out, self.case.out_col0, variant=variant)
        return out.cpu(), gates, cell

    def bwd(self, gates, cell, variant):
        ops, _ = _api()
        c = self.case
        return ops.lstm_bwd(self.dout, c.out_col0, gates, cell, self.whh, c.hidden, c.ndir, c.reverse_mask, self.seq,
                            variant=variant).cpu()


def _expected_out(case, values):
    """The whole output buffer: the sentinel, except h in the rows of the sequences and the columns of the directions."""
    want = torch.full((case.rows, case.ldo), S, dtype=values.dtype)
    cols = slice(case.out_col0, case.out_col0 + case.ndir * case.hidden)
    want[case.in_seq, cols] = values[case.in_seq]
    return want


def _check_out(family, label, case, out, ref, cpu32):
    cols = slice(case.out_col0, case.out_col0 + case.ndir * case.hidden)
    untouched = _expected_out(case, torch.zeros(case.rows, case.ndir * case.hidden)) == S
    assert torch.equal(out[untouched], torch.full_like(out[untouched], S)), f"{family} {label}: wrote outside its columns / rows"
    _check(family, label, "out", out[case.in_seq, cols], ref.out[case.in_seq], cpu32.out[case.in_seq])


def _run_training_forms(dev, bundle, forms, label):
    """forms: [(family forward, family backward, variant)].  Forward out / gates / cell and backward dxproj of every form
    against float64; the backward also on the reference's own saved tensors rounded to fp32."""
    case, ref, cpu32, iso32 = bundle
    d = _Device(case, dev)
    rows = case.in_seq
    gscale = ref.dxproj.abs().max().item()
    ref_gates, ref_cell = ref.gates.float().to(dev), ref.cell.float().to(dev)
    results = {}
    for fam_f, fam_b, variant in forms:
        out, gates, cell = d.train(variant)
        _check_out(fam_f, label, case, out, ref, cpu32)
        _check(fam_f, label, "gates", gates.cpu()[rows], ref.gates[rows], cpu32.gates[rows])
        _check(fam_f, label, "cell", cell.cpu()[rows], ref.cell[rows], cpu32.cell[rows])
        assert torch.equal(d.infer(variant), out), f"{fam_f} {label}: inference and training forward differ"
        dx = d.bwd(gates, cell, variant)
        assert torch.isfinite(dx[rows]).all()
        _check(fam_b, label, "dxproj", dx[rows], ref.dxproj[rows], cpu32.dxproj[rows], gscale)
        dx_iso = d.bwd(ref_gates, ref_cell, variant)
        _check(fam_b, label, "dxproj_iso", dx_iso[rows], ref.dxproj[rows], iso32.dxproj[rows], gscale)
        results[variant] = (out, gates.cpu(), cell.cpu(), dx)
    return results


# --------------------------------------------------------------------------- generic kernels
@pytest.mark.parametrize("hidden", sfi.GENERIC_HIDDEN)
def test_generic_kernels_against_float64(dev, hidden):
    """lstm_kernel, lstm_train_fwd_kernel and lstm_bwd_kernel at the edges of their run-time slicing (KQ = min(1024/H, H),
    kpq = ceil(H/KQ), JQ / jpq): KQ clamped to H (1, 3), trailing empty slices (33, 90), either side of the specialised
    size (255, 257), an idle fourth slice (300), one slice and 424 idle threads (600), the declared limit (1024)."""
    ops, abi = _api()
    bundle = sfi.lstm_bundle(hidden)
    _run_training_forms(dev, bundle, [("generic forward", "generic backward", abi.LSTM_AUTO),
                                      ("generic forward", "generic backward", abi.LSTM_STREAM)], f"H={hidden}")


@pytest.mark.parametrize("hidden", [0, 1025])
def test_hidden_outside_the_declared_range_is_refused(dev, hidden):
    ops, abi = _api()
    ndir, rows = 3, 15
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    xproj, whh_t, whh = z(rows, ndir * 4 * hidden), z(ndir, hidden, 4 * hidden), z(ndir, 4 * hidden, hidden)
    seq = torch.tensor([2, 2, 3, 5, 14], dtype=torch.int64, device=dev)
    out = torch.full((rows, ndir * hidden + 9), S, dtype=torch.float32, device=dev)
    with pytest.raises(abi.AvsError, match="avs_lstm_f32"):
        ops.lstm(xproj, whh_t, hidden, ndir, 0b010, seq, out, 4)
    with pytest.raises(abi.AvsError, match="avs_lstm_train_fwd_f32"):
        ops.lstm_train_fwd(xproj, whh_t, hidden, ndir, 0b010, seq, out, 4)
    with pytest.raises(abi.AvsError, match="avs_lstm_bwd_f32"):
        ops.lstm_bwd(out, 4, xproj, z(rows, ndir * hidden), whh, hidden, ndir, 0b010, seq)
    torch.cuda.synchronize(dev)
    assert (out == S).all()     # nothing ran


@pytest.mark.parametrize("hidden", [255, 257])
def test_forms_built_for_256_refuse_its_neighbours(dev, hidden):
    ops, abi = _api()
    d = _Device(sfi.lstm_bundle(hidden)[0], dev)
    for variant in (abi.LSTM_RESIDENT_20_8, abi.LSTM_RESIDENT_16_8, abi.LSTM_SPLIT4):
        with pytest.raises(abi.AvsError, match="256"):
            d.infer(variant)
    with pytest.raises(abi.AvsError, match="256"):
        d.train(abi.LSTM_SPLIT4)


# --------------------------------------------------------------------------- hidden = 256
def _forms_256(abi):
    # LSTM_AUTO takes the four-CU split at these few recurrences (ops.LSTM_SPLIT_MAX_RECURRENCES)
    return [("split forward", "split backward", abi.LSTM_AUTO), ("generic forward", "generic backward", abi.LSTM_STREAM),
            ("resident forward", "resident backward", abi.LSTM_RESIDENT_20_8),
            ("split forward", "split backward", abi.LSTM_SPLIT4)]


def test_hidden_256_every_form_against_float64(dev):
    """20 recurrences of up to 700 steps on LSTM_AUTO, LSTM_STREAM, LSTM_RESIDENT_20_8 and LSTM_SPLIT4 (training forward,
    inference, backward) and LSTM_RESIDENT_16_8 (inference): each against float64, not against each other."""
    ops, abi = _api()
    bundle = sfi.lstm_bundle(256, 4, 0b1010, sfi.H256_LENS)
    case, ref, cpu32, _ = bundle
    assert ops._lstm_takes_split(abi.LSTM_AUTO, 256, case.ndir, len(case.lens))
    _run_training_forms(dev, bundle, _forms_256(abi), "H=256 lens=700,1,0,333,2")
    out = _Device(case, dev).infer(abi.LSTM_RESIDENT_16_8)
    _check_out("resident forward", "H=256 16+8 inference", case, out, ref, cpu32)
    assert ops.lstm_split_errors(dev) == 0


def test_hidden_256_inference_chain_of_2000_steps(dev):
    ops, abi = _api()
    case, ref, cpu32, _ = sfi.lstm_bundle(256, 2, 0b10, (2000,), backward=False)
    d = _Device(case, dev)
    for family, variant in (("split forward", abi.LSTM_AUTO), ("generic forward", abi.LSTM_STREAM),
                            ("resident forward", abi.LSTM_RESIDENT_20_8), ("resident forward", abi.LSTM_RESIDENT_16_8),
                            ("split forward", abi.LSTM_SPLIT4)):
        _check_out(family, f"H=256 T=2000 variant={variant}", case, d.infer(variant), ref, cpu32)
    assert ops.lstm_split_errors(dev) == 0


# --------------------------------------------------------------------------- saturated gates, twin sequences
@pytest.mark.parametrize("hidden", [20, 256])
def test_saturated_gates(dev, hidden):
    """A third of the pre-activations times 30: sigmoid rounds to 0 or 1 and tanh to +-1 in fp32.  Everything stays finite
    and within the bound, and where the float64 gradient is exactly 0 (a gate at exactly 1, tanh at exactly +-1, the
    forget gate's gradient at the first step) the kernel's is exactly 0 too."""
    ops, abi = _api()
    bundle = sfi.lstm_bundle(hidden, saturate=True)
    case, ref, _, _ = bundle
    rows = case.in_seq
    assert (ref.gates[rows] == 1).any() and (ref.gates[rows] == -1).any()      # saturated in float64 as well
    zero = ref.dxproj[rows] == 0
    assert zero.sum() > 0.02 * zero.numel()
    forms = _forms_256(abi)[1:] if hidden == 256 else [("generic forward", "generic backward", abi.LSTM_AUTO)]
    for variant, (out, gates, cell, dx) in _run_training_forms(dev, bundle, forms, f"H={hidden} saturated").items():
        for t in (out[rows, 4:4 + case.ndir * hidden], gates[rows], cell[rows], dx[rows]):
            assert torch.isfinite(t).all()
        assert (dx[rows][zero] == 0).all(), variant
    assert ops.lstm_split_errors(dev) == 0


@pytest.mark.parametrize("hidden", [20, 256])
def test_twin_sequences_give_identical_bits(dev, hidden):
    """Sequences 2 and 4 of one launch have the same content at different rows: the same bits, forward and backward."""
    ops, abi = _api()
    case = sfi.lstm_case(hidden, lens=(5, 0, 9, 1, 9), twins=(2, 4))
    d = _Device(case, dev)
    a, b = (slice(int(case.seq_rows[i]), int(case.seq_rows[i + 1])) for i in (2, 4))
    variants = (abi.LSTM_AUTO, abi.LSTM_STREAM) + ((abi.LSTM_RESIDENT_20_8, abi.LSTM_SPLIT4) if hidden == 256 else ())
    for variant in variants:
        out, gates, cell = d.train(variant)
        dx = d.bwd(gates, cell, variant)
        for t in (out, d.infer(variant), gates.cpu(), cell.cpu(), dx):
            assert torch.equal(t[a], t[b]), variant
    assert ops.lstm_split_errors(dev) == 0
