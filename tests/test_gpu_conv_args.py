"""What the convolution + BatchNorm wrappers refuse in their per-group affine operands, one wrong thing at a time, on
tensors of at most 16 x 64 elements: every (scale, shift) goes through ops._group_affine - a contiguous fp32 device tensor
[groups, cols] - and every refusal is a ValueError that starts with the wrapper's name.  Nothing is launched: the library
is out of reach while the refusals run.

Before the wrappers shared that check, each carried its own copy, and the copies had drifted apart.  The parent let
through, to be read by the kernel as fp32 [groups, cols] whatever it was:
  * a bf16 (any non-fp32) in_affine of conv1x1_bn, bn_gram_affine, bn_gram_affine_h2 and conv1x1_affine;
  * every res_affine of conv2d_affine: without a residual, of the wrong shape, fp64;
  * an x_affine of conv2d_raw of the wrong shape ([groups, cin + 1]).
The other cases (a transposed in_affine, one with a group too few, a scale of the wrong width, conv1x1_affine's
res_affine) were refused before, by the copies.

One positive case per body that two wrappers now share: bn_gram_affine and bn_gram_affine_h2 at the smallest shape the
kernels take.  The numerical checks of these wrappers are the convbn_f64, f16x2, bncluster_packed, local224_mfma16,
lstm_f64 and train_batch suites."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ROWS, RPG, GROUPS, K, N = 16, 8, 2, 8, 4       # 16 rows in 2 groups of 8; K = cin = 8, N = cout = 4


def _cases(dev):
    """[(label, call)]: each call has exactly one wrong argument."""
    from avsum_amd import ops
    z = lambda *shape, dtype=F32: torch.zeros(shape, dtype=dtype, device=dev)
    pair = lambda *shape, dtype=F32: (z(*shape, dtype=dtype), z(*shape, dtype=dtype))
    x, w, out, res = z(ROWS, K, dtype=BF16), z(N, K, dtype=BF16), z(ROWS, N, dtype=BF16), z(ROWS, N, dtype=BF16)
    xh, wh = z(ROWS, K), z(N, K)
    gamma, beta = z(N), z(N)
    good_in, good_out = pair(GROUPS, K), pair(GROUPS, N)
    code = ops.dtype_code(F32, "f16x2")
    out_cases = []

    def add(name, label, call):
        out_cases.append((f"{name}: {label}", call))

    bad_in = (("in_affine bf16", pair(GROUPS, K, dtype=BF16)),
              ("in_affine transposed", (z(K, GROUPS).t(), z(K, GROUPS).t())),
              ("in_affine one group too few", pair(GROUPS - 1, K)),
              ("in_affine shift of another width", (good_in[0], z(GROUPS, K + 1))),
              ("in_affine on the host", (good_in[0].cpu(), good_in[1].cpu())))
    for label, aff in bad_in:
        add("conv1x1_bn", label, lambda aff=aff: ops.conv1x1_bn(x, w, RPG, gamma, beta, 1e-5, out, in_affine=aff))
        add("bn_gram_affine", label, lambda aff=aff: ops.bn_gram_affine(x, w, RPG, gamma, beta, 1e-5, aff))
        add("bn_gram_affine_h2", label, lambda aff=aff: ops.bn_gram_affine_h2(xh, wh, RPG, gamma, beta, 1e-5, aff))
        add("conv1x1_affine", label, lambda aff=aff: ops.conv1x1_affine(x, w, RPG, *good_out, out, in_affine=aff))

    def conv1x1_affine(scale=good_out[0], shift=good_out[1], **kw):
        return ops.conv1x1_affine(x, w, RPG, scale, shift, out, **kw)

    def conv2d_affine(scale=good_out[0], shift=good_out[1], **kw):
        return ops.conv2d_affine(code, 1, 4, 4, K, 1, 1, 4, 4, N, z(1, 4, 4, K), 16 * K, 4 * K, K, wh, K, z(1, 4, 4, N), N,
                                 RPG, scale, shift, **kw)

    for name, wrapper, residual in (("conv1x1_affine", conv1x1_affine, res), ("conv2d_affine", conv2d_affine, z(ROWS, N))):
        add(name, "scale of the wrong width", lambda f=wrapper: f(scale=z(GROUPS, N + 1)))
        add(name, "shift bf16", lambda f=wrapper: f(shift=z(GROUPS, N, dtype=BF16)))
        add(name, "res_affine without a residual", lambda f=wrapper: f(res_affine=good_out))
        add(name, "res_affine of the wrong shape", lambda f=wrapper, r=residual: f(residual=r, res_affine=pair(GROUPS + 1, N)))
        add(name, "res_affine float64", lambda f=wrapper, r=residual: f(residual=r, res_affine=pair(GROUPS, N, dtype=F64)))
        add(name, "res_affine transposed",
            lambda f=wrapper, r=residual: f(residual=r, res_affine=(z(N, GROUPS).t(), z(N, GROUPS).t())))

    def conv2d_raw(x_affine):
        return ops.conv2d_raw(code, 1, 4, 4, K, 3, 3, 1, 1, 1, 1, 4, 4, N, z(1, 4, 4, K), 16 * K, 4 * K, K, z(N, 9 * K), 9 * K,
                              z(1, 4, 4, N), N, bnstats=(RPG, gamma, beta, 1e-5), x_affine=x_affine)

    add("conv2d_raw", "x_affine of [groups, cin + 1]", lambda: conv2d_raw((*pair(GROUPS, K + 1), True)))
    add("conv2d_raw", "x_affine float64", lambda: conv2d_raw((*pair(GROUPS, K, dtype=F64), True)))
    add("conv2d_raw", "x_affine transposed", lambda: conv2d_raw((z(K, GROUPS).t(), z(K, GROUPS).t(), True)))
    return out_cases


def test_wrappers_refuse_a_wrong_group_affine(dev, monkeypatch):
    from avsum_amd import ops
    cases = _cases(dev)
    assert len({label for label, _ in cases}) == len(cases)
    assert {label.split(":")[0] for label, _ in cases} == {"conv1x1_bn", "bn_gram_affine", "bn_gram_affine_h2",
                                                           "conv1x1_affine", "conv2d_affine", "conv2d_raw"}

    def no_launch():
        raise AssertionError("a refusal test reached the library")
    monkeypatch.setattr(ops, "lib", no_launch)
    wrong = []
    for label, call in cases:
        name, operand = label.split(":")[0], label.split(": ")[1].split(" ")[0]
        try:
            call()
        except (ValueError, TypeError) as e:
            if type(e) is not ValueError or not str(e).startswith(name + ":") or operand not in str(e):
                wrong.append((label, type(e).__name__, str(e)))
        else:
            wrong.append((label, "accepted", ""))
    assert not wrong, wrong


@pytest.mark.parametrize("h2", [False, True], ids=["bf16", "f16x2"])
def test_gram_affine_smallest_shape(dev, h2):
    """K = 64, N = 32, one group of 128 rows, with an input affine: both names of the shared body return finite [1, 32]
    pairs, bit-identical across two calls."""
    from avsum_amd import ops
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(128, 64, generator=g).to(dev), (torch.randn(32, 64, generator=g) * 0.125).to(dev)
    gamma, beta = (torch.rand(32, generator=g) + 0.5).to(dev), torch.randn(32, generator=g).to(dev)
    in_affine = ((torch.rand(1, 64, generator=g) + 0.5).to(dev), torch.randn(1, 64, generator=g).to(dev))
    if h2:
        x, w, fn = ops.f16x2_pack(x), ops.f16x2_pack(w), ops.bn_gram_affine_h2
    else:
        x, w, fn = x.bfloat16(), w.bfloat16(), ops.bn_gram_affine
    first = fn(x, w, 128, gamma, beta, 1e-5, in_affine)
    second = fn(x, w, 128, gamma, beta, 1e-5, in_affine)
    for a, b in zip(first, second):
        assert a.shape == (1, 32) and a.dtype == F32 and torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
