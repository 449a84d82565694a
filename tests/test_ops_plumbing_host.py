"""The plumbing that ops.py keeps once for all its wrappers, driven directly on CPU tensors: the exchange buffer of the
clustered BatchNorm and the split LSTM (tag ranges, growth, and the error word that survives both), the per-(kind, device,
stream) scratch buffer, the unwrap of the library's host-only queries, and the group-affine check reached with a host
tensor.  No GPU: the classes only allocate, zero and read back, which torch does on the host as well."""
import pytest
import torch

MIB = 1 << 20
CPU = torch.device("cpu")


def _set_error_word(buf, value):
    buf[:4].view(torch.int32)[0] = value


def test_exchange_tag_sequences_are_the_wrappers():
    """The clustered BatchNorm reserves one tag per launch and passes base + 1 (the library refuses tag 0): 1, 2, 3.
    The split LSTM reserves rows + 1 and passes base: 0, 8, 16 for 7 rows."""
    from avsum_amd import ops
    ex = ops._Exchange()
    assert [ex.reserve(CPU, 64, 1)[1] + 1 for _ in range(3)] == [1, 2, 3]
    ex = ops._Exchange()
    assert [ex.reserve(CPU, 64, 7 + 1)[1] for _ in range(3)] == [0, 8, 16]


def test_exchange_growth():
    from avsum_amd import ops
    ex = ops._Exchange()
    buf, base = ex.reserve(CPU, 100, 1)
    assert buf.dtype == torch.uint8 and buf.numel() == MIB and not buf.any() and base == 0
    buf[8:16] = 7                                            # (granules of an earlier launch)
    same, base = ex.reserve(CPU, MIB, 1)
    assert same is buf and base == 1 and same[8] == 7        # within the current size: the same buffer, left as it is
    big, base = ex.reserve(CPU, MIB + 1, 1)
    assert big is not buf and big.numel() == MIB + 1 and not big.any() and base == 0
    assert ex.reserve(CPU, 100, 1)[0] is big                 # never shrinks


def test_exchange_error_word_survives_growth_and_the_tag_wrap():
    """A bounded wait that ran out before the buffer grew (layers of one forward ask for different sizes) or before the
    32-bit tags wrapped is still reported: 3 + 0, then 3 + 2 = 5."""
    from avsum_amd import ops
    ex = ops._Exchange()
    assert ex.errors() == 0
    buf, _ = ex.reserve(CPU, 100, 1)
    _set_error_word(buf, 3)
    assert ex.errors() == 3
    big, base = ex.reserve(CPU, 2 * MIB, 1)
    assert big is not buf and base == 0
    assert ex.errors() == 3                                  # (the parent reported 0 here)
    # the wrap: the next range would reach the limit -> the buffer is cleared, tags start over, the count is kept
    ex.tags = ops._Exchange.TAG_LIMIT - 8 - 2
    kept, base = ex.reserve(CPU, 100, 8)
    assert kept is big and base == ex.tags - 8 and ex.errors() == 3       # base + tags + 1 == limit - 1: no wrap yet
    big[100] = 9
    kept, base = ex.reserve(CPU, 100, 8)
    assert kept is big and base == 0 and ex.tags == 8 and not big.any() and ex.errors() == 3
    _set_error_word(big, 2)
    assert ex.errors() == 5
    ex.reserve(CPU, 3 * MIB, 1)
    assert ex.errors() == 5
    assert ex.errors() == 5                                  # reading does not reset


def test_exchange_users_are_separate_per_kind_and_key(monkeypatch):
    from avsum_amd import ops
    stream = [1]
    monkeypatch.setattr(ops, "_ws_key", lambda device: (device, stream[0]))
    monkeypatch.setattr(ops, "_exchanges", {})
    cl = ops._exchange("cluster", CPU)
    assert ops._exchange("cluster", CPU) is cl and ops._exchange("lstm", CPU) is not cl
    _set_error_word(cl.reserve(CPU, 64, 1)[0], 4)
    assert ops.cluster_exchange_errors(CPU) == 4 and ops.lstm_split_errors(CPU) == 0
    stream[0] = 2
    assert ops._exchange("cluster", CPU) is not cl and ops.cluster_exchange_errors(CPU) == 0


def test_scratch_growth_floors_kinds_and_keys(monkeypatch):
    from avsum_amd import ops
    stream = [1]
    monkeypatch.setattr(ops, "_ws_key", lambda device: (device, stream[0]))
    monkeypatch.setattr(ops, "_scratch", {})
    # the floors of the four users: 1 MiB (convolution statistics), 256 B (stems), 64 KiB (audio means), none (VGGish)
    for kind, floor in (("stats", MIB), ("stem", 256), ("segmean", 1 << 16), ("vggish", 0)):
        ws = ops._scratch_buf(kind, CPU, 10, floor)
        assert ws.dtype == torch.uint8 and ws.numel() == max(10, floor), kind
        assert ops._scratch_buf(kind, CPU, 10, floor) is ws and ops._scratch_buf(kind, CPU, 5, floor) is ws, kind
        assert ops._scratch_buf(kind, CPU, ws.numel(), floor) is ws, kind
        big = ops._scratch_buf(kind, CPU, ws.numel() + 1, floor)
        assert big is not ws and big.numel() == ws.numel() + 1, kind
        assert ops._scratch_buf(kind, CPU, 10, floor) is big, kind             # never shrinks
    kinds = [ops._scratch_buf(k, CPU, 1) for k in ("stats", "stem", "segmean", "vggish")]
    assert len({t.data_ptr() for t in kinds}) == 4
    stream[0] = 2                                                              # another stream: another buffer
    other = ops._scratch_buf("stem", CPU, 1, 256)
    assert other is not kinds[1] and other.numel() == 256
    stream[0] = 1
    assert ops._scratch_buf("stem", CPU, 1, 256) is kinds[1]


def test_query_unwrap():
    from avsum_amd import _abi, ops
    assert _abi.E_UNSUPPORTED < 0
    assert ops._query(_abi.E_UNSUPPORTED, "avs_query") is None
    assert ops._query(0, "avs_query") == 0 and ops._query(4096, "avs_query") == 4096
    with pytest.raises(_abi.AvsError, match="avs_query"):
        ops._query(_abi.E_UNSUPPORTED, "avs_query", may_decline=False)
    other = -1 if _abi.E_UNSUPPORTED != -1 else -2
    with pytest.raises(_abi.AvsError, match="avs_query"):
        ops._query(other, "avs_query")


def _affine_on_host_cases():
    """[(wrapper, the affine operand it checks first, call)]: every wrapper that goes through ops._group_affine, with all
    its affines given and on the host, all arguments well-formed: 16 rows in 2 groups of 8, K = cin = 8, N = cout = 4.
    (Operand by operand, with the others on the device: tests/test_gpu_conv_args.py.)"""
    from avsum_amd import ops
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16)
    f = lambda *s: torch.zeros(s)
    x, w, out, res = bf(16, 8), bf(4, 8), bf(16, 4), bf(16, 4)
    xh, wh = f(16, 8), f(4, 8)
    gamma, beta = f(4), f(4)
    ina, outa = (f(2, 8), f(2, 8)), (f(2, 4), f(2, 4))
    code = ops.dtype_code(torch.float32, "f16x2")
    return [
        ("conv1x1_bn", "in_affine", lambda: ops.conv1x1_bn(x, w, 8, gamma, beta, 1e-5, out, in_affine=ina)),
        ("bn_gram_affine", "in_affine", lambda: ops.bn_gram_affine(x, w, 8, gamma, beta, 1e-5, ina)),
        ("bn_gram_affine_h2", "in_affine", lambda: ops.bn_gram_affine_h2(xh, wh, 8, gamma, beta, 1e-5, ina)),
        ("conv1x1_affine", "scale", lambda: ops.conv1x1_affine(x, w, 8, *outa, out, residual=res, in_affine=ina,
                                                               res_affine=outa)),
        ("conv2d_affine", "scale", lambda: ops.conv2d_affine(
            code, 1, 4, 4, 8, 1, 1, 4, 4, 4, f(1, 4, 4, 8), 128, 32, 8, wh, 8, f(1, 4, 4, 4), 4, 8, *outa,
            residual=f(16, 4), res_affine=outa)),
        ("conv2d_raw", "x_affine", lambda: ops.conv2d_raw(
            code, 1, 4, 4, 8, 3, 3, 1, 1, 1, 1, 4, 4, 4, f(1, 4, 4, 8), 128, 32, 8, f(4, 72), 72, f(1, 4, 4, 4), 4,
            bnstats=(8, gamma, beta, 1e-5), x_affine=(ina[0], ina[1], True))),
    ]


def test_group_affine_on_the_host_is_refused_by_name(monkeypatch):
    """A host tensor as an affine: a ValueError in the wording tests/test_abi_and_host.py pins for ops._dev, which starts
    with the wrapper's name and names the operand.  ops._dev is taken out of the way so that the affine check is what
    refuses (on a machine without a GPU every other operand is a host tensor too), and the library is out of reach."""
    from avsum_amd import ops
    cases = _affine_on_host_cases()
    assert {w for w, _, _ in cases} == {"conv1x1_bn", "bn_gram_affine", "bn_gram_affine_h2", "conv1x1_affine",
                                        "conv2d_affine", "conv2d_raw"}
    for _, _, call in cases:                 # as the wrappers stand, the first check refuses the host operands
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()

    def no_launch():
        raise AssertionError("a refusal test reached the library")
    monkeypatch.setattr(ops, "lib", no_launch)
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    for wrapper, operand, call in cases:
        with pytest.raises(ValueError, match="no CPU fallback") as err:
            call()
        text = str(err.value)
        assert text.startswith(wrapper + ":") and operand in text.split(" must ")[0], (wrapper, operand, text)
