"""GPU parity of the host-side mirrors (reference API surface) against the oracle on seeded inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _seeded_scorer(seed, spread=True, **kw):
    from avsum_amd.models.av_model import AVBiLSTMModel
    torch.manual_seed(seed)
    m = AVBiLSTMModel(**kw).eval()
    if spread:
        # default init gives scores within ~0.01 of each other; widen the last layers so that
        # the selection rule is exercised away from the decision boundary
        with torch.no_grad():
            m.scorer[0].weight.mul_(6.0)
            m.scorer[2].weight.mul_(6.0)
    return m


def _guarded_equal_selection(got, ref, tol):
    from oracle import selection
    mean = np.mean(ref)
    safe = np.abs(ref - mean) > 2 * tol
    sel_ref = ref > mean
    sel_got = got > np.mean(got)
    assert np.array_equal(sel_ref[safe], sel_got[safe])
    return int((~safe).sum()), selection.select_frames(ref)


@pytest.mark.parametrize("b,t", [(1, 300), (1, 1), (2, 17), (3, 5), (1, 1800), (1, 5000)])
def test_av_bilstm_full_dims(dev, b, t):
    from oracle import scorer as osc
    m = _seeded_scorer(7)
    g = torch.Generator().manual_seed(100 + t)
    visual = torch.randn(b, t, 4096, generator=g)
    audio = torch.zeros(b, t, 296)  # the literal audio features are all-zero
    ref = osc.av_bilstm_forward(m.state_dict(), visual, audio)
    md = m.to(dev)
    with torch.no_grad():
        got = md(visual.to(dev), audio.to(dev)).cpu()
    assert got.shape == ref.shape  # .squeeze() rules (av_model.py:46)
    tol = 1e-4  # north_star: importance scores within 1e-4 fp32
    assert (got - ref).abs().max().item() < tol
    if b == 1 and t > 1:
        dropped, _ = _guarded_equal_selection(got.numpy(), ref.numpy(), 2e-6)
        assert dropped <= t // 10


@pytest.mark.parametrize("t_len", [1800, 5000])
def test_av_bilstm_long_golden(dev, t_len):
    """configs[1] / configs[3] sequence lengths against the scores the REFERENCE CLASS produced (models/av_model.py:6-46;
    tests/golden/scorer_long.npz, written by tests/golden/make_golden.py from the imported class): 1800- and 5000-step
    fp32 recurrences on the register / LDS-resident kernel.  North_star's bar: scores within 1e-4."""
    import os
    from avsum_amd.models.av_model import AVBiLSTMModel
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scorer_long.npz"))
    torch.manual_seed(int(z["seed"]))
    m = AVBiLSTMModel().eval().to(dev)
    v = torch.randn(1, t_len, 4096, generator=torch.Generator().manual_seed(int(z[f"t{t_len}_input_seed"])))
    with torch.no_grad():
        got = m(v.to(dev), torch.zeros(1, t_len, 296, device=dev)).cpu().numpy()
    ref = z[f"t{t_len}_out"]
    assert got.shape == ref.shape == (t_len,)
    err = np.abs(got - ref).max()
    assert err < 1e-4, err
    # default init: the scores lie within ~1e-2 of each other, so the selection is decided by 1e-6-level differences;
    # outside a 2e-6 guard band the selected indices must be the reference's
    dropped, _ = _guarded_equal_selection(got, ref, 2e-6)
    assert dropped <= t_len // 10


def test_score_rows_config3_share_equals_per_video_calls(dev):
    """One rank's configs[3] share in ONE call - 50 sequences x 5000 steps as concatenated rows - is bit for bit what 50
    per-video forward() calls return (the reference scores one video per call, scripts/evaluate.py:15-19): no coupling
    between sequences, no dependence on where a sequence sits in the launch."""
    m = _seeded_scorer(7).to(dev)
    n_seq, t_len = 50, 5000
    g = torch.Generator(device=dev).manual_seed(31)
    vis = torch.randn(n_seq * t_len, 4096, generator=g, device=dev)
    aud = torch.zeros(n_seq * t_len, 296, device=dev)
    seq = torch.arange(0, (n_seq + 1) * t_len, t_len, dtype=torch.int64, device=dev)
    with torch.no_grad():
        together = m.score_rows(vis, aud, seq, attn_batch=1)
        for i in (0, 1, 17, 49):
            one = m(vis[i * t_len:(i + 1) * t_len].unsqueeze(0), aud[:t_len].unsqueeze(0))
            assert torch.equal(one, together[i * t_len:(i + 1) * t_len]), i
    assert torch.isfinite(together).all()


def test_av_bilstm_small_dims_random_audio(dev):
    from oracle import scorer as osc
    m = _seeded_scorer(3, visual_dim=64, audio_dim=24, hidden_dim=32)
    g = torch.Generator().manual_seed(5)
    v, a = torch.randn(2, 40, 64, generator=g), torch.randn(2, 40, 24, generator=g)
    ref = osc.av_bilstm_forward(m.state_dict(), v, a)
    with torch.no_grad():
        got = m.to(dev)(v.to(dev), a.to(dev)).cpu()
    assert (got - ref).abs().max().item() < 1e-5


def test_av_bilstm_unsupported_calls_fail_loudly(dev):
    m = _seeded_scorer(1, visual_dim=64, audio_dim=24, hidden_dim=32).to(dev).train()
    with pytest.raises(NotImplementedError):  # the training path is one sequence per call, like the reference's loop
        m(torch.zeros(2, 4, 64, device=dev), torch.zeros(2, 4, 24, device=dev))
    with pytest.raises(RuntimeError):
        m.eval()(torch.zeros(1, 4, 64), torch.zeros(1, 4, 24))  # host tensors: no CPU fallback
    with pytest.raises(NotImplementedError):  # eval mode, B > 1, autograd on: no silent graph-less result
        m.eval()(torch.zeros(2, 4, 64, device=dev), torch.zeros(2, 4, 24, device=dev))
    with torch.no_grad():
        assert m.eval()(torch.zeros(2, 4, 64, device=dev), torch.zeros(2, 4, 24, device=dev)).shape == (2, 4)


def _train_case(dev, dims, t, seed):
    """Gradients of the train-mode forward (Dropout masks injected on both sides) vs torch autograd over the
    oracle restatement."""
    from avsum_amd.models._scorer_train import dropout_keep
    from oracle import scorer as osc
    m = _seeded_scorer(seed, **dims)
    hidden = m.visual_fc[0].out_features
    g = torch.Generator().manual_seed(seed + 1)
    v = torch.randn(1, t, m.visual_fc[0].in_features, generator=g)
    a = torch.randn(1, t, m.audio_fc[0].in_features, generator=g)
    keep_v = (torch.rand(t, hidden, generator=g) >= 0.3).float() / 0.7
    keep_a = (torch.rand(t, hidden, generator=g) >= 0.3).float() / 0.7
    target = torch.rand(1, generator=g)
    sd = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters()}
    ref = osc.av_bilstm_forward_train(sd, v, a, keep_v, keep_a)
    loss_ref = torch.nn.functional.mse_loss(ref, target.squeeze().expand_as(ref))
    names = list(sd.keys())
    grads_ref = torch.autograd.grad(loss_ref, [sd[k] for k in names], allow_unused=True)
    md = m.to(dev).train()
    md._dropout_keep = (keep_v.to(dev), keep_a.to(dev))
    out = md(v.to(dev), a.to(dev))
    assert out.shape == ref.shape and (out.detach().cpu() - ref.detach()).abs().max().item() < 1e-5
    loss = torch.nn.functional.mse_loss(out, target.to(dev).squeeze().expand_as(out))
    assert abs(loss.item() - loss_ref.item()) < 1e-6
    loss.backward()
    for k, gr in zip(names, grads_ref):
        got = dict(md.named_parameters())[k].grad
        assert got is not None, k
        gr = torch.zeros_like(got.cpu()) if gr is None else gr
        scale = max(gr.abs().max().item(), 1e-8)
        assert (got.cpu() - gr).abs().max().item() <= 1e-4 * scale + 1e-9, (k, (got.cpu() - gr).abs().max().item(), scale)
    return md


def test_av_bilstm_backward_small(dev):
    _train_case(dev, dict(visual_dim=64, audio_dim=24, hidden_dim=32), 23, 5)
    _train_case(dev, dict(visual_dim=64, audio_dim=24, hidden_dim=32), 1, 6)


def test_av_bilstm_backward_full_dims(dev):
    _train_case(dev, {}, 61, 9)


def test_training_loop_matches_oracle(dev):
    """The reference's loop (scripts/train_av_model.py:70-96: AdamW lr 1e-4, one video per step, one broadcast
    target, MSE) for 6 steps: same loss trajectory on the HIP path and on the CPU restatement."""
    from avsum_amd.models.av_model import AVBiLSTMModel
    from oracle import scorer as osc
    dims = dict(visual_dim=128, audio_dim=40, hidden_dim=64)
    torch.manual_seed(77)
    m = AVBiLSTMModel(**dims)
    ref_params = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters()}
    opt_ref = torch.optim.AdamW(list(ref_params.values()), lr=1e-4)
    md = m.to(dev).train()
    opt = torch.optim.AdamW(md.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(3)
    losses, losses_ref = [], []
    for step in range(6):
        t = 20 + 3 * step
        v, a = torch.randn(1, t, 128, generator=g), torch.randn(1, t, 40, generator=g)
        kv = (torch.rand(t, 64, generator=g) >= 0.3).float() / 0.7
        ka = (torch.rand(t, 64, generator=g) >= 0.3).float() / 0.7
        target = torch.rand(1, generator=g) * 4 + 1
        out_ref = osc.av_bilstm_forward_train(ref_params, v, a, kv, ka)
        lr_ = torch.nn.functional.mse_loss(out_ref, target.expand_as(out_ref))
        opt_ref.zero_grad()
        lr_.backward()
        opt_ref.step()
        md._dropout_keep = (kv.to(dev), ka.to(dev))
        out = md(v.to(dev), a.to(dev))
        loss = torch.nn.functional.mse_loss(out, target.to(dev).expand_as(out))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        losses_ref.append(lr_.item())
    rel = max(abs(x - y) / abs(y) for x, y in zip(losses, losses_ref))
    assert rel < 1e-4, (losses, losses_ref)  # SURVEY cfg5: loss trajectory <= 1e-4 relative


@pytest.mark.parametrize("e,h,b,t", [(1024, 4, 1, 300), (512, 8, 2, 77), (64, 4, 3, 1), (1024, 4, 1, 1801),
                                     (512, 4, 2, 33), (256, 4, 1, 129), (1024, 4, 2, 1), (1024, 4, 1, 5000),
                                     (512, 4, 1, 700)])   # head dim 128, 22 key tiles, the fp32 kernel's 4-wave instance
def test_mhsa(dev, e, h, b, t):
    from avsum_amd.models.attention import MultiHeadSelfAttention
    from oracle import scorer as osc
    torch.manual_seed(11)
    m = MultiHeadSelfAttention(e, h).eval()
    x = torch.randn(b, t, e, generator=torch.Generator().manual_seed(t))
    ref = osc.mhsa_forward(m.state_dict(), x, h)
    md = m.to(dev)
    with torch.no_grad():
        md.use_flash = True   # fused kernel, split precision on the fp16 matrix cores (head dims 64/128/256;
        got = md(x.to(dev)).cpu()   # silently the GEMM path otherwise): the default ("auto")
        md.use_flash = "f32"  # the fused kernel on the fp32 MFMA
        got3 = md(x.to(dev)).cpu()
        md.use_flash = False  # the materialised-score path must agree too
        got2 = md(x.to(dev)).cpu()
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-4
    assert (got2 - ref).abs().max().item() < 1e-4
    assert (got3 - ref).abs().max().item() < 1e-4


def test_mhsa_long_golden(dev):
    """MultiHeadSelfAttention(1024, 4) at T = 5000 against 64 output rows + the absolute sum of the REFERENCE CLASS's output
    (models/attention.py:15-25; tests/golden/mhsa_long.npz): the fused f16x2 core ("auto"), the fused fp32 core and the
    materialising path."""
    import os
    from avsum_amd.models.attention import MultiHeadSelfAttention
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mhsa_long.npz"))
    torch.manual_seed(int(z["seed"]))
    m = MultiHeadSelfAttention(1024, 4).eval().to(dev)
    x = torch.randn(1, int(z["t"]), 1024, generator=torch.Generator().manual_seed(int(z["input_seed"]))).to(dev)
    rows = torch.from_numpy(z["rows"]).to(dev)
    ref_rows = torch.from_numpy(z["out_rows"])
    with torch.no_grad():
        for mode in ("auto", True, "f32", False):
            m.use_flash = mode
            got = m(x)
            assert (got[0, rows].cpu() - ref_rows).abs().max().item() < 1e-4, mode
            assert abs(float(got.double().abs().sum()) / float(z["out_abs_sum"]) - 1) < 1e-5, mode


@pytest.mark.parametrize("e,h,b,t,flash", [(512, 8, 2, 77, True), (1024, 4, 1, 300, True), (64, 4, 3, 5, True),
                                           (256, 4, 1, 129, "f32"), (96, 4, 2, 31, False), (512, 4, 1, 1, True)])
def test_mhsa_backward(dev, e, h, b, t, flash):
    """Autograd through MultiHeadSelfAttention (reference: an ordinary autograd module, models/attention.py:5-25):
    the gradients of the input and of all 8 parameters against torch autograd through the oracle's forward (pinned to
    the reference class in tests/test_oracle_pins.py), <= 1e-4 relative to each tensor's largest entry."""
    from avsum_amd.models.attention import MultiHeadSelfAttention
    from oracle import scorer as osc
    torch.manual_seed(13)
    m = MultiHeadSelfAttention(e, h)
    x = torch.randn(b, t, e, generator=torch.Generator().manual_seed(t + e))
    gout = torch.randn(b, t, e, generator=torch.Generator().manual_seed(3))
    sd = {k_: v_.detach().clone().requires_grad_(True) for k_, v_ in m.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ref = osc.mhsa_forward(sd, xr, h)
    ref.backward(gout)
    md = m.to(dev)
    md.use_flash = flash
    xd = x.to(dev).requires_grad_(True)
    got = md(xd)
    assert got.requires_grad and (got.detach().cpu() - ref.detach()).abs().max().item() < 1e-4
    got.backward(gout.to(dev))

    def close(a, r, name):
        err = (a.cpu() - r).abs().max().item()
        # (key.bias: its gradient is analytically zero - the softmax is invariant to a shift of all keys' scores - and
        #  both sides hold rounding noise of ~1e-7 there: hence the absolute floor of 1e-6)
        assert err <= 1e-4 * max(r.abs().max().item(), 1e-2), (name, err, r.abs().max().item())

    close(xd.grad, xr.grad, "x")
    for name, prm in md.named_parameters():
        close(prm.grad, sd[name].grad, name)
    # parameters frozen: the input gradient alone; input without grad: the parameter gradients alone
    for prm in md.parameters():
        prm.grad = None
        prm.requires_grad_(False)
    xd2 = x.to(dev).requires_grad_(True)
    md(xd2).backward(gout.to(dev))
    close(xd2.grad, xr.grad, "x (frozen parameters)")
    with torch.no_grad():
        assert not md(x.to(dev)).requires_grad


def _frames(n, seed, h=224, w=224):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def test_resnet50_trunk_batchstat_fp32(dev):
    """5 frames = micro-batches of 4 + 1 (extractors.py:48-56): train-mode BN statistics per micro-batch."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    from oracle import cnn as ocnn
    torch.manual_seed(21)
    trunk = resnet50_trunk()
    frames = _frames(5, 1)
    sd = trunk.state_dict()
    with torch.no_grad():
        x = torch.cat([ocnn.preprocess_frame(f) for f in frames])
        ref = torch.cat([ocnn.resnet50_trunk_forward(sd, x[:4]), ocnn.resnet50_trunk_forward(sd, x[4:])])
    runner = ResNet50Runner(trunk.to(dev), torch.float32, "batch")
    got = runner.forward(torch.from_numpy(frames).to(dev), [0, 4, 5]).cpu()
    assert got.shape == (5, 2048)
    err = (got - ref).abs().max().item()
    assert err < 1e-4 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("gsize", [1, 2])
def test_resnet50_trunk_equal_groups(dev, gsize):
    """Equal-sized BatchNorm groups: per-frame groups (the per-frame scoring mode) and 2-frame groups,
    fp32 parity mode against the oracle."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    from oracle import cnn as ocnn
    torch.manual_seed(24)
    trunk = resnet50_trunk()
    frames = _frames(4, 5)
    sd = trunk.state_dict()
    with torch.no_grad():
        x = torch.cat([ocnn.preprocess_frame(f) for f in frames])
        ref = torch.cat([ocnn.resnet50_trunk_forward(sd, x[i:i + gsize]) for i in range(0, 4, gsize)])
    got = ResNet50Runner(trunk.to(dev), torch.float32, "batch").forward(
        torch.from_numpy(frames).to(dev), list(range(0, 5, gsize))).cpu()
    err = (got - ref).abs().max().item()
    # 53 batch-normalised layers whose statistics come from as few as 49 samples: the fp32 features themselves
    # are conditioned to a few 1e-4 (relative to the largest feature); the 1e-4 bar of north_star is on the
    # importance SCORES and is checked end to end in test_pipeline_end_to_end_fp32
    assert err < 5e-4 * max(1.0, ref.abs().max().item()), err


def test_conv_bnstats_epilogue_matches_separate_pass(dev):
    """Statistics from the convolution's epilogue (per-tile partial sums folded in tile order) against the separate
    statistics pass over the stored output; groups that straddle tiles, a ragged last tile, a shorter last group.
    The fused form is deterministic: a second run gives bit-identical scale / shift."""
    from avsum_amd import ops
    g = torch.Generator().manual_seed(6)
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 2e-3)):
        # (frames, hw, cin, cout, kernel, frames per group)
        for n, hw, cin, cout, k, gf in ((6, 7, 64, 128, 3, 2), (6, 14, 32, 64, 1, 2), (6, 6, 64, 192, 1, 2),
                                        (5, 28, 64, 64, 3, 1), (7, 14, 64, 256, 1, 3), (9, 10, 32, 64, 1, 1)):
            rpg = gf * hw * hw
            x = (torch.randn(n, hw, hw, cin, generator=g) + 0.5).to(dtype).to(dev)
            wt = (torch.randn(cout, k * k * cin, generator=g) / (k * k * cin) ** 0.5).to(dtype).to(dev)
            gamma = (torch.rand(cout, generator=g) + 0.5).to(dev)
            beta = torch.randn(cout, generator=g).to(dev)
            y1 = torch.empty((n, hw, hw, cout), dtype=dtype, device=dev)
            sc1, sh1 = ops.conv2d(x, wt, k, k, 1, k // 2, y1, bnstats=(rpg, gamma, beta, 1e-5))
            y2 = torch.empty_like(y1)
            ops.conv2d(x, wt, k, k, 1, k // 2, y2)
            bounds = list(range(0, n, gf)) + [n]           # the last group may be shorter
            rows = torch.tensor(bounds, dtype=torch.int64, device=dev) * hw * hw
            sc2, sh2 = ops.bn_batch_stats(y2.view(-1, cout), rows, gamma, beta, 1e-5)
            assert torch.equal(y1, y2)
            assert sc1.shape == sc2.shape
            assert (sc1 - sc2).abs().max().item() < tol * sc2.abs().max().item()
            assert (sh1 - sh2).abs().max().item() < tol * max(1.0, sh2.abs().max().item())
            sc3, sh3 = ops.conv2d(x, wt, k, k, 1, k // 2, y1, bnstats=(rpg, gamma, beta, 1e-5))
            assert torch.equal(sc1, sc3) and torch.equal(sh1, sh3)
    # groups of fewer than 64 rows are declined (None): the caller runs the separate statistics pass
    x = torch.zeros((4, 5, 5, 64), dtype=torch.bfloat16, device=dev)
    wt = torch.zeros((64, 64), dtype=torch.bfloat16, device=dev)
    assert ops.conv2d(x, wt, 1, 1, 1, 0, torch.empty_like(x), bnstats=(25, gamma[:64], beta[:64], 1e-5)) is None


@pytest.mark.parametrize("rpg,k,n,with_res,relu", [(196, 256, 1024, True, True), (3136, 64, 256, True, True),
                                                     (784, 512, 128, False, True), (300, 64, 64, False, False),
                                                     (128, 128, 200, True, False)])
def test_conv1x1_bn_one_kernel(dev, rpg, k, n, with_res, relu):
    """The one-kernel 1x1 conv + batch-stat BN (+residual, +ReLU) against the same arithmetic in fp32 on the
    bf16-rounded operands; bf16 output => compare to ~2 bf16 ulps of the output scale."""
    from avsum_amd import ops
    g = torch.Generator().manual_seed(rpg + k)
    groups = 3
    rows = groups * rpg
    x = (torch.randn(rows, k, generator=g) + 0.3).bfloat16()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
    gamma, beta = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    res = torch.randn(rows, n, generator=g).bfloat16() if with_res else None
    raw = x.float() @ w.float().t()
    ref = torch.empty(rows, n)
    for gi in range(groups):
        blk = raw[gi * rpg:(gi + 1) * rpg]
        mean, var = blk.mean(0), blk.var(0, unbiased=False)
        ref[gi * rpg:(gi + 1) * rpg] = (blk - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    if with_res:
        ref = ref + res.float()
    if relu:
        ref = torch.relu(ref)
    out = torch.empty(rows, n, dtype=torch.bfloat16, device=dev)
    ops.conv1x1_bn(x.to(dev), w.to(dev), rpg, gamma.to(dev), beta.to(dev), 1e-5, out,
                   res.to(dev) if with_res else None, relu)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 0.03 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("rpg,k,n,with_res", [(3136, 64, 256, True), (784, 128, 512, True), (300, 64, 64, False),
                                               (196, 256, 1024, True), (128, 512, 200, False)])
def test_conv1x1_bn_input_affine_is_bn_apply_first(dev, rpg, k, n, with_res):
    """avs_conv1x1_bn_in_bf16 (the previous layer's BatchNorm + ReLU applied while staging the input) must be
    BIT-IDENTICAL to avs_bn_apply on the raw input followed by avs_conv1x1_bn_bf16."""
    from avsum_amd import ops
    g = torch.Generator().manual_seed(rpg * 3 + k)
    groups = 4
    rows = groups * rpg
    raw = (torch.randn(rows, k, generator=g) * 2 + 0.3).bfloat16().to(dev)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16().to(dev)
    isc = torch.randn(groups, k, generator=g).to(dev)            # both signs
    ish = torch.randn(groups, k, generator=g).to(dev)
    gamma, beta = (torch.rand(n, generator=g) + 0.5).to(dev), torch.randn(n, generator=g).to(dev)
    res = torch.randn(rows, n, generator=g).bfloat16().to(dev) if with_res else None
    grows = torch.arange(0, rows + 1, rpg, dtype=torch.int64, device=dev)
    xin = ops.bn_apply(raw, isc, ish, grows, rpg, None, ops.ACT_RELU)
    want = ops.conv1x1_bn(xin, w, rpg, gamma, beta, 1e-5, torch.empty(rows, n, dtype=torch.bfloat16, device=dev), res, True)
    got = ops.conv1x1_bn(raw, w, rpg, gamma, beta, 1e-5, torch.empty(rows, n, dtype=torch.bfloat16, device=dev), res, True,
                         in_affine=(isc, ish))
    assert torch.equal(got, want)


@pytest.mark.parametrize("rpg,k,n,with_res,xf", [(3136, 64, 256, True, True), (784, 128, 512, True, True),
                                                  (3136, 64, 256, False, False), (300, 64, 64, False, True),
                                                  (100, 128, 224, True, False), (64, 128, 32, False, True)])
def test_conv1x1_gram_statistics_and_streaming_pass(dev, rpg, k, n, with_res, xf):
    """avs_bn_gram_affine_bf16 (BatchNorm statistics of a 1x1 convolution from the Gram matrix of its input) against
    float64 statistics of the actual products, and the one-pass convolution with that affine against (i) the same
    arithmetic in fp32 and (ii) the two-pass kernel.  Groups whose row count is not a multiple of the 64-row tile,
    input affine (previous BatchNorm + ReLU) on and off; deterministic."""
    from avsum_amd import ops
    g = torch.Generator().manual_seed(rpg + k + n)
    groups = 3
    rows = groups * rpg
    raw = (torch.randn(rows, k, generator=g) * 1.5 + 0.3).bfloat16()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
    gamma, beta = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    res = torch.randn(rows, n, generator=g).bfloat16() if with_res else None
    in_aff = None
    a = raw.float()
    if xf:
        isc, ish = torch.randn(groups, k, generator=g), torch.randn(groups, k, generator=g)
        in_aff = (isc.to(dev), ish.to(dev))
        a = torch.relu(raw.float().view(groups, rpg, k) * isc[:, None, :] + ish[:, None, :]).bfloat16().float().view(rows, k)
    y = a.double() @ w.double().t()
    yg = y.view(groups, rpg, n)
    mean, var = yg.mean(1), yg.var(1, unbiased=False)
    sc_ref = gamma.double() / torch.sqrt(var + 1e-5)
    sh_ref = beta.double() - mean * sc_ref
    xd, wd, gd, bd = raw.to(dev), w.to(dev), gamma.to(dev), beta.to(dev)
    sc, sh = ops.bn_gram_affine(xd, wd, rpg, gd, bd, 1e-5, in_aff)
    assert sc.shape == (groups, n)
    assert ((sc.cpu().double() - sc_ref).abs() / sc_ref.abs()).max().item() < 2e-4
    assert (sh.cpu().double() - sh_ref).abs().max().item() < 2e-4 * max(1.0, sh_ref.abs().max().item())
    sc2, sh2 = ops.bn_gram_affine(xd, wd, rpg, gd, bd, 1e-5, in_aff)
    assert torch.equal(sc, sc2) and torch.equal(sh, sh2)
    ref = (yg * sc_ref[:, None, :] + sh_ref[:, None, :]).view(rows, n).float()
    if with_res:
        ref = ref + res.float()
    ref = torch.relu(ref)
    out = torch.empty(rows, n, dtype=torch.bfloat16, device=dev)
    rd = res.to(dev) if with_res else None
    ops.conv1x1_gram_bn(xd, wd, rpg, gd, bd, 1e-5, out, rd, True, in_aff)
    got = out.float().cpu()
    scale = max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() < 0.03 * scale and (got - ref).abs().mean().item() < 0.004 * scale
    if xf:
        # finish_input: the statistics kernel overwrites the raw input with a = bf16(relu(x * isc + ish)) and the pass
        # reads it finished - the same arithmetic, bit-identical output
        xc = xd.clone()
        out_f = ops.conv1x1_gram_bn(xc, wd, rpg, gd, bd, 1e-5, torch.empty_like(out), rd, True, in_aff, finish_input=True)
        assert torch.equal(out_f, out)
        assert torch.equal(xc.float().cpu(), a.bfloat16().float())
    if with_res:
        # residual affine: the residual as a RAW convolution output whose BatchNorm is folded into the add, against
        # the same kernel on the residual finished first by avs_bn_apply (one bf16 rounding more)
        rsc, rsh = (torch.rand(groups, n, generator=g) + 0.5).to(dev), torch.randn(groups, n, generator=g).to(dev)
        grows = torch.arange(0, rows + 1, rpg, dtype=torch.int64, device=dev)
        rfin = ops.bn_apply(rd, rsc, rsh, grows, rpg, None, ops.ACT_NONE)
        want = ops.conv1x1_gram_bn(xd, wd, rpg, gd, bd, 1e-5, torch.empty_like(out), rfin, True, in_aff).float()
        gota = ops.conv1x1_gram_bn(xd, wd, rpg, gd, bd, 1e-5, torch.empty_like(out), rd, True, in_aff,
                                   res_affine=(rsc, rsh)).float()
        da = (gota - want).abs()
        sa = max(1.0, want.abs().max().item())
        assert da.max().item() < 0.02 * sa and (da > 0).float().mean().item() < 0.2
        ref_a = torch.relu((yg * sc_ref[:, None, :] + sh_ref[:, None, :]).view(rows, n).float()
                           + (res.float().view(groups, rpg, n) * rsc.cpu()[:, None, :] + rsh.cpu()[:, None, :]).view(rows, n))
        assert (gota.cpu() - ref_a).abs().max().item() < 0.03 * sa
        assert (gota.cpu() - ref_a).abs().mean().item() <= (want.cpu() - ref_a).abs().mean().item() * 1.05 + 1e-6
    two = torch.empty_like(out)
    ops.conv1x1_bn(xd, wd, rpg, gd, bd, 1e-5, two, rd, True, in_aff)
    # same products, affines equal to fp32 rounding: outputs differ by at most one bf16 step here and there
    diff = (got - two.float().cpu()).abs()
    assert diff.max().item() < 0.02 * scale and (diff > 0).float().mean().item() < 0.05


@pytest.mark.parametrize("n,fpg", [(6, 1), (8, 4), (3, 3)])
def test_fused_stem_against_the_unfused_sequence_and_torch(dev, n, fpg):
    """avs_stem_conv_bn_pool_bf16 (uint8 frames -> normalise -> conv1 7x7/2 -> per-tile partial sums + the pooled raw
    map, max or min by the sign of gamma -> bn1 + ReLU) against (i) torch fp32 on the bf16-rounded operands
    and (ii) the unfused HIP sequence (normalise, convolution + statistics, BatchNorm + ReLU + maxpool).  gamma has both
    signs so that the min-pooled map is exercised; image borders exercise the -inf padding of the pooling."""
    from avsum_amd import ops
    from avsum_amd.cnn import RESNET_MEAN, RESNET_STD, _stem_weight
    g = torch.Generator().manual_seed(40 + n)
    frames = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, generator=g)
    w4 = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5
    gamma = torch.randn(64, generator=g)                      # both signs
    beta = torch.randn(64, generator=g) * 0.5
    wk = _stem_weight(w4, 8, torch.bfloat16).to(dev)
    fd, gd, bd = frames.to(dev), gamma.to(dev), beta.to(dev)
    y, sc, sh = ops.stem_conv_bn_pool(fd, wk, 1.0, RESNET_MEAN, RESNET_STD, fpg, gd, bd, 1e-5)
    y2, sc2, sh2 = ops.stem_conv_bn_pool(fd, wk, 1.0, RESNET_MEAN, RESNET_STD, fpg, gd, bd, 1e-5)
    assert torch.equal(y, y2) and torch.equal(sc, sc2) and torch.equal(sh, sh2)     # deterministic
    assert y.shape == (n, 56, 56, 64) and sc.shape == (n // fpg, 64)
    # (i) torch fp32 on the bf16-rounded normalised input and weights
    mean = torch.tensor(RESNET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(RESNET_STD).view(1, 3, 1, 1)
    x = ((frames.permute(0, 3, 1, 2).float() - mean) / std).bfloat16().float()
    raw = F.conv2d(x, w4.bfloat16().float(), None, 2, 3)                             # [n,64,112,112]
    rg = raw.view(n // fpg, fpg, 64, 112, 112)
    m = rg.mean((1, 3, 4), keepdim=True)
    v = rg.var((1, 3, 4), unbiased=False, keepdim=True)
    scale_ref = (gamma.view(1, 1, 64, 1, 1) / torch.sqrt(v + 1e-5))
    shift_ref = beta.view(1, 1, 64, 1, 1) - m * scale_ref
    assert (sc.cpu() - scale_ref.view(-1, 64)).abs().max().item() < 2e-3 * scale_ref.abs().max().item()
    act = torch.relu(rg.bfloat16().float() * scale_ref + shift_ref).view(n, 64, 112, 112)
    ref = F.max_pool2d(act, 3, 2, 1).permute(0, 2, 3, 1)
    got = y.float().cpu()
    tol = max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() < 0.03 * tol and (got - ref).abs().mean().item() < 0.004 * tol
    # (ii) the unfused HIP sequence: identical convolution values up to the summation order => a bf16 step here and there
    x0 = ops.frames_normalize(fd, torch.bfloat16, 1.0, RESNET_MEAN, RESNET_STD, 230, 232, 3, 3)
    rawd = torch.empty((n, 112, 112, 64), dtype=torch.bfloat16, device=dev)
    geom, xs = (n, 230, 112, 32, 7, 1, 2, 1, 0, 0, 112, 112, 64), (230 * 232 * 4, 232 * 4, 8)
    scu, shu = ops.conv2d_raw(ops.dtype_code(torch.bfloat16), *geom, x0, *xs, wk, wk.stride(0), rawd, 64,
                              bnstats=(fpg * 112 * 112, gd, bd, 1e-5))
    rows = torch.arange(0, n + 1, fpg, dtype=torch.int64, device=dev) * 112 * 112
    yu = ops.bn_maxpool(rawd, scu, shu, rows, True, 3, 2, 1, torch.empty_like(y))
    assert (sc - scu).abs().max().item() < 1e-4 * scu.abs().max().item()
    diff = (y.float() - yu.float()).abs()
    assert diff.max().item() < 0.03 * tol and (diff > 0).float().mean().item() < 0.02
    # (iii) apply = 0: the pooled RAW map (max where gamma >= 0, min elsewhere) + bn1's affine; the BatchNorm apply
    # pass on it gives the finished map bit for bit
    yr, sc3, sh3 = ops.stem_conv_bn_pool(fd, wk, 1.0, RESNET_MEAN, RESNET_STD, fpg, gd, bd, 1e-5, apply=False)
    assert torch.equal(sc3, sc) and torch.equal(sh3, sh)
    rows56 = torch.arange(0, n + 1, fpg, dtype=torch.int64, device=dev) * 56 * 56
    fin = torch.empty_like(yr).view(-1, 64)
    ops.bn_apply(yr.view(-1, 64), sc3, sh3, rows56, fpg * 56 * 56, None, ops.ACT_RELU, fin)
    assert torch.equal(fin.view_as(y), y)
    pooled = F.max_pool2d(raw.bfloat16().float() * torch.sign(gamma + (gamma == 0)).view(1, 64, 1, 1), 3, 2, 1) \
        * torch.sign(gamma + (gamma == 0)).view(1, 64, 1, 1)
    dr = (yr.float().cpu() - pooled.permute(0, 2, 3, 1)).abs()
    assert dr.max().item() < 0.03 * max(1.0, pooled.abs().max().item()) and (dr > 0).float().mean().item() < 0.02


def test_resnet50_bf16_deferred_bn_apply_close(dev):
    """Whole trunk with bn2 applied inside conv3's kernel vs applied by its own pass: the same arithmetic, every
    kernel on the path deterministic => bit-identical features."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(29)
    trunk = resnet50_trunk().to(dev)
    frames = torch.from_numpy(_frames(8, 6)).to(dev)
    a = ResNet50Runner(trunk, torch.bfloat16)
    b = ResNet50Runner(trunk, torch.bfloat16)
    a.defer_res_apply = False     # (folds the downsample's BatchNorm into conv3's add: one bf16 rounding less, not identical)
    b.defer_bn_apply = False
    fa, fb = a.forward(frames).cpu(), b.forward(frames).cpu()
    assert torch.equal(fa, fb)


@pytest.mark.parametrize("gsize", [1, 4])
def test_resnet50_bf16_raw_stem_path(dev, gsize):
    """Whole trunk with bn1 + ReLU of the stem applied inside the first block's conv1 / downsample (one shared Gram
    matrix) against the stem finished by its own pass: the downsample branch is the same arithmetic (bit-identical
    operands), conv1 changes form (Gram statistics + one pass instead of convolution + statistics + apply), so the
    features agree to bf16 noise - and the path is deterministic.  The same for layer 2's downsample branch kept raw
    with its BatchNorm folded into conv3's residual add (defer_res_apply)."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(31)
    trunk = resnet50_trunk().to(dev)
    with torch.no_grad():
        trunk[1].weight.mul_(torch.where(torch.arange(64, device=dev) % 5 == 0, -1.0, 1.0))   # both signs of gamma
    frames = torch.from_numpy(_frames(8, 9)).to(dev)
    groups = list(range(0, 9, gsize))
    a = ResNet50Runner(trunk, torch.bfloat16)
    b = ResNet50Runner(trunk, torch.bfloat16)
    b.stem_raw = b.defer_res_apply = False
    fa, fa2, fb = a.forward(frames, groups).cpu(), a.forward(frames, groups).cpu(), b.forward(frames, groups).cpu()
    assert torch.equal(fa, fa2)
    f32 = ResNet50Runner(trunk, torch.float32).forward(frames, groups).cpu()
    ea, eb = ((fa - f32).norm() / f32.norm()).item(), ((fb - f32).norm() / f32.norm()).item()
    cos = torch.nn.functional.cosine_similarity(fa, fb, dim=1).min().item()
    assert cos > 0.98 and ea < 0.2 and ea < 1.25 * eb + 0.01, (cos, ea, eb)


@pytest.mark.parametrize("gsize", [1, 3, 4])
def test_resnet50_bf16_is_deterministic(dev, gsize):
    """No float atomics anywhere on the throughput path: two runs of the same frames give bit-identical features
    (per-frame groups, the reference's 4-frame micro-batches, and an odd group size that no fused form takes)."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(31)
    trunk = resnet50_trunk().to(dev)
    frames = torch.from_numpy(_frames(24, 8)).to(dev)
    runner = ResNet50Runner(trunk, torch.bfloat16)
    groups = list(range(0, 25, gsize))
    a = runner.forward(frames, groups).clone()
    b = runner.forward(frames, groups)
    assert torch.equal(a, b)
    assert torch.isfinite(a).all()


def _bn_reference(raw, rpg, gamma, beta, res, relu):
    rows, n = raw.shape
    ref = torch.empty(rows, n)
    for gi in range(rows // rpg):
        blk = raw[gi * rpg:(gi + 1) * rpg]
        mean, var = blk.mean(0), blk.var(0, unbiased=False)
        ref[gi * rpg:(gi + 1) * rpg] = (blk - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    if res is not None:
        ref = ref + res.float()
    return torch.relu(ref) if relu else ref


# (frames, hw in, cin, cout, kernel, stride, frames per BatchNorm group, residual, relu)
# groups that fit a 256-row tile whole -> the tile-local one-launch form
_LOCAL_CASES = [
    (11, 14, 256, 1024, 1, 1, 1, True, True),   # 196 rows: one group per tile
    (11, 14, 256, 256, 3, 1, 1, False, True),   # 3x3 taps, 196-row groups
    (7, 14, 1024, 256, 1, 1, 1, False, False),  # long reduction
    (13, 8, 128, 128, 3, 1, 1, True, True),     # 64-row groups: four per tile, the tile exactly full
    (6, 10, 128, 64, 1, 1, 1, False, True),     # 100-row groups: two per tile; 64-wide tile
    (9, 7, 2048, 512, 1, 1, 1, False, True),    # 49-row groups: five per tile, last tile 4 groups
    (9, 7, 512, 2048, 1, 1, 1, True, True),     # layer4 conv3: 49-row groups, residual
    (8, 7, 512, 512, 3, 2, 4, False, True),     # stride 2 to 4x4 maps, 4-frame groups of 64 rows
    (8, 28, 256, 512, 1, 2, 1, False, False),   # strided downsample to 14x14, no ReLU
]
# larger groups -> the split path (statistics in the convolution's epilogue + avs_bn_apply)
_SPLIT_CASES = [
    (12, 56, 64, 256, 1, 1, 1, True, True),     # layer1 conv3: two column tiles, tiles straddle groups (3136 % 128 != 0)
    (12, 56, 64, 64, 3, 1, 1, False, True),     # layer1 conv2: 64-wide tile, spatial taps
    (8, 28, 128, 128, 3, 2, 4, False, True),    # long reduction (128-byte rows), stride 2, 4-frame groups
    (5, 14, 1024, 256, 1, 1, 5, False, True),   # ONE group for the whole call (980 rows)
    (64, 56, 64, 256, 1, 1, 4, True, True),     # the reference's 4-frame micro-batches, 200k rows
]


def _conv_bn_operands(cfg):
    frames, hw, cin, cout, k, s, gf, with_res, relu = cfg
    g = torch.Generator().manual_seed(sum(cfg[:6]))
    pad = k // 2
    ho = (hw + 2 * pad - k) // s + 1
    rpg = gf * ho * ho
    x = (torch.randn(frames, hw, hw, cin, generator=g) + 0.3).bfloat16()
    w4 = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).bfloat16()
    wt = w4.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    res = torch.randn(frames * ho * ho, cout, generator=g).bfloat16() if with_res else None
    raw = F.conv2d(x.float().permute(0, 3, 1, 2), w4.float(), stride=s, padding=pad).permute(0, 2, 3, 1).reshape(-1, cout)
    ref = _bn_reference(raw, rpg, gamma, beta, res, relu)
    return x, wt, gamma, beta, res, ref, pad, ho, rpg


def _split_path(dev, cfg, xd, wd, gamma, beta, res, pad, ho, rpg):
    from avsum_amd import ops
    frames, hw, cin, cout, k, s, gf, with_res, relu = cfg
    y2 = torch.empty((frames, ho, ho, cout), dtype=torch.bfloat16, device=dev)
    rows = torch.arange(0, frames * ho * ho + 1, rpg, dtype=torch.int64, device=dev)
    affine = ops.conv2d(xd, wd, k, k, s, pad, y2, bnstats=(rpg, gamma.to(dev), beta.to(dev), 1e-5))
    if affine is None:   # groups of fewer than 64 rows: the separate statistics pass (what the runner does)
        ops.conv2d(xd, wd, k, k, s, pad, y2)
        affine = ops.bn_batch_stats(y2.view(-1, cout), rows, gamma.to(dev), beta.to(dev), 1e-5)
    sc, sh = affine
    ops.bn_apply(y2.view(-1, cout), sc, sh, rows, rpg, res.to(dev) if with_res else None,
                 ops.ACT_RELU if relu else ops.ACT_NONE, y2.view(-1, cout))
    return y2.float().cpu().view(-1, cout)


@pytest.mark.parametrize("cfg", _LOCAL_CASES)
def test_conv_bnlocal_one_launch(dev, cfg):
    """Convolution + whole batch-statistics BatchNorm (+residual, +ReLU) in one launch, tiles that hold whole groups,
    against the same arithmetic in fp32 on the bf16-rounded operands and against the split HIP path; deterministic."""
    from avsum_amd import ops
    frames, hw, cin, cout, k, s, gf, with_res, relu = cfg
    x, wt, gamma, beta, res, ref, pad, ho, rpg = _conv_bn_operands(cfg)
    geom = (frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    code = ops.dtype_code(torch.bfloat16)
    tile_rows = ops.conv_bnlocal_tile_rows(code, *geom, *xs, wt.shape[1], cout, rpg)
    assert tile_rows == 256 // rpg * rpg
    xd, wd = x.to(dev), wt.to(dev)
    outs = []
    for _ in range(2):
        y = torch.empty((frames, ho, ho, cout), dtype=torch.bfloat16, device=dev)
        ops.conv2d_raw(code, *geom, xd, *xs, wd, wd.stride(0), y, cout, act=ops.ACT_RELU if relu else ops.ACT_NONE,
                       bnlocal=(rpg, gamma.to(dev), beta.to(dev), 1e-5, res.to(dev) if with_res else None))
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].float().cpu().view(-1, cout)
    scale = max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() < 0.03 * scale
    assert (got - ref).abs().mean().item() < 0.004 * scale
    split = _split_path(dev, cfg, xd, wd, gamma, beta, res, pad, ho, rpg)
    assert (got - split).abs().max().item() < 0.03 * scale


@pytest.mark.parametrize("cfg", _SPLIT_CASES)
def test_conv_bn_split_path(dev, cfg):
    """Groups too large for a tile: statistics from the convolution's epilogue + avs_bn_apply against the same
    arithmetic in fp32 on the bf16-rounded operands; the one-launch form declines these shapes."""
    from avsum_amd import ops
    frames, hw, cin, cout, k, s, gf, with_res, relu = cfg
    x, wt, gamma, beta, res, ref, pad, ho, rpg = _conv_bn_operands(cfg)
    geom = (frames, hw, hw, cin, k, k, s, s, pad, pad, ho, ho, cout)
    xs = (hw * hw * cin, hw * cin, cin)
    assert ops.conv_bnlocal_tile_rows(ops.dtype_code(torch.bfloat16), *geom, *xs, wt.shape[1], cout, rpg) is None
    xd, wd = x.to(dev), wt.to(dev)
    got = _split_path(dev, cfg, xd, wd, gamma, beta, res, pad, ho, rpg)
    again = _split_path(dev, cfg, xd, wd, gamma, beta, res, pad, ho, rpg)
    assert torch.equal(got, again)
    scale = max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() < 0.03 * scale
    assert (got - ref).abs().mean().item() < 0.004 * scale


def test_conv_bnlocal_declines(dev):
    """Shapes the one-launch form cannot take are declined up front (None -> the caller uses the split path)."""
    from avsum_amd import _abi, ops
    code = ops.dtype_code(torch.bfloat16)
    geom = lambda n, hw, cin, cout: ((n, hw, hw, cin, 1, 1, 1, 1, 0, 0, hw, hw, cout), (hw * hw * cin, hw * cin, cin))
    g, xs = geom(8, 4, 128, 64)
    assert ops.conv_bnlocal_tile_rows(code, *g, *xs, 128, 64, 16) is None          # 16-row groups
    g, xs = geom(4, 8, 128, 96)
    assert ops.conv_bnlocal_tile_rows(code, *g, *xs, 128, 96, 64) is None          # cout not a tile multiple
    g, xs = geom(4, 12, 128, 64)
    assert ops.conv_bnlocal_tile_rows(code, *g, *xs, 128, 64, 144) is None         # 144 rows fill 56 % of a tile
    g, xs = geom(4, 28, 128, 64)
    assert ops.conv_bnlocal_tile_rows(code, *g, *xs, 128, 64, 784) is None         # a group larger than a tile
    g, xs = geom(4, 14, 128, 64)
    assert ops.conv_bnlocal_tile_rows(ops.dtype_code(torch.float32), *g, *xs, 128, 64, 196) is None
    assert ops.conv_bnlocal_tile_rows(code, *g, *xs, 128, 64, 196) == 196


@pytest.mark.parametrize("gsize", [1, 4])
def test_resnet50_bf16_planned_local_form_close_to_split_form(dev, gsize, monkeypatch):
    """Whole trunk: one-launch convolution + BatchNorm on the layers that take it against the two-pass / split forms
    (both bf16) and fp32."""
    from avsum_amd import ops
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(23)
    trunk = resnet50_trunk().to(dev)
    frames = torch.from_numpy(_frames(16, 4)).to(dev)
    groups = list(range(0, 17, gsize))
    local = ResNet50Runner(trunk, torch.bfloat16)
    launched = []
    raw = ops.conv2d_raw

    def spy(*a, **k):
        if k.get("bnlocal") is not None:
            launched.append(k.get("cluster", 1))
        return raw(*a, **k)

    monkeypatch.setattr(ops, "conv2d_raw", spy)
    got = local.forward(frames, groups).cpu()
    monkeypatch.undo()
    # the form really ran (14x14 + 7x7 layers / 7x7 layers), as the plan says
    assert len(launched) == (28 if gsize == 1 else 9)
    assert sum(s.form in ("local", "cluster") for s in local.plan(16, groups)) == len(launched)
    split = ResNet50Runner(trunk, torch.bfloat16)
    split.bn_local = False
    ref_bf = split.forward(frames, groups).cpu()
    ref32 = ResNet50Runner(trunk, torch.float32).forward(frames, groups).cpu()
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a, b, dim=1).min().item()
    assert cos(got, ref32) > 0.98 and cos(got, ref_bf) > 0.98
    # the one-launch form normalises the fp32 accumulators (no bf16 rounding of the raw convolution in between):
    # it must not be further from fp32 than the split form is
    e_local = ((got - ref32).norm() / ref32.norm()).item()
    e_split = ((ref_bf - ref32).norm() / ref32.norm()).item()
    assert e_local < 0.2 and e_local < 1.25 * e_split, (e_local, e_split)


@pytest.mark.parametrize("groups", [[0, 4, 8], [0, 4, 7, 8]])
def test_resnet50_bf16_close_to_fp32(dev, groups):
    """bf16 throughput mode (equal groups: statistics fused into the convolution epilogue; ragged groups:
    separate statistics pass) against the fp32 parity mode."""
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(22)
    trunk = resnet50_trunk().to(dev)
    frames = torch.from_numpy(_frames(8, 2)).to(dev)
    f32 = ResNet50Runner(trunk, torch.float32).forward(frames, groups).cpu()
    bf = ResNet50Runner(trunk, torch.bfloat16).forward(frames, groups).cpu()
    # bf16 activations through 53 batch-normalised layers of a RANDOM-weight network: the feature vectors
    # stay strongly aligned but not close element-wise (measured ~0.11 relative L2)
    rel = ((bf - f32).norm() / f32.norm()).item()
    cos = torch.nn.functional.cosine_similarity(bf, f32, dim=1).min().item()
    assert rel < 0.2 and cos > 0.98, (rel, cos)


def test_inception_v3_fp32(dev):
    from avsum_amd.cnn import Inception3, InceptionV3Runner
    from oracle import cnn as ocnn
    torch.manual_seed(23)
    net = Inception3()
    # non-trivial running stats so that the BN folding is exercised
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    frames = _frames(2, 3)
    sd = net.state_dict()
    with torch.no_grad():
        ref = ocnn.inception_v3_forward(sd, torch.cat([ocnn.preprocess_inception(f) for f in frames]))
    from avsum_amd import ops
    big = ops.resize_bilinear(torch.from_numpy(frames).to(dev), 299, 299)
    runner = InceptionV3Runner(net.to(dev), torch.float32)
    got = runner.forward(big).cpu()
    err = (got - ref).abs().max().item()
    assert err < 1e-4 * max(1.0, ref.abs().max().item()), err
    # branch_pool in the reference's order (average, then 1x1 convolution) instead of convolution first: the same
    # linear map, equal to fp32 reassociation
    runner.pool_after_conv = False
    lit = runner.forward(big).cpu()
    assert (lit - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())
    assert (lit - got).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    # the same trunk in the f16x2 mode (fp16 hi | lo storage, three fp16 MFMAs per product, bias + ReLU in the epilogue,
    # pooling and the channel-concat slices on f16x2 tensors): fp32-class agreement, deterministic
    rh = InceptionV3Runner(net, torch.float32, f32_split="f16x2")
    goth = rh.forward(big).cpu()
    assert torch.equal(goth, rh.forward(big).cpu())
    assert (goth - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())


def test_visual_extractor_api(dev):
    from avsum_amd.features.extractors import VisualFeatureExtractor
    from oracle import cnn as ocnn
    torch.manual_seed(31)
    ext = VisualFeatureExtractor()
    frames = list(_frames(6, 4))
    ref = ocnn.visual_forward(ext.resnet.state_dict(), ext.inception.state_dict(), frames)
    ext = ext.to(dev)
    got = ext(frames)
    assert got.dtype == np.float32 and got.shape == (4096,)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    assert np.array_equal(ext([]), np.zeros(4096, np.float32))  # extractors.py:44-45
    # the same call in the f16x2 arithmetic (selected by name), both trunks: fp32-class agreement
    exth = VisualFeatureExtractor(arith="f16x2")
    exth.load_state_dict(ext.state_dict())
    goth = exth.to(dev)(frames)
    assert goth.dtype == np.float32 and np.abs(goth - ref).max() < 5e-4 * max(1.0, np.abs(ref).max())
    with pytest.raises(ValueError):
        VisualFeatureExtractor(arith="fp8")
    p = ext._preprocess_frame(frames[0])
    assert p.shape == (1, 3, 224, 224) and torch.equal(p, ocnn.preprocess_frame(frames[0]))
    pi = ext._preprocess_inception(frames[0])
    assert pi.shape == (1, 3, 299, 299) and torch.equal(pi, ocnn.preprocess_inception(frames[0]))


def test_pipeline_end_to_end_fp32(dev):
    """frames -> ResNet-50 (per-frame batch-stat BN) | Inception-v3 -> AVBiLSTM scorer -> selection, fp32 parity
    mode, against the oracle end to end: scores within 1e-4, selected indices identical (guard-banded)."""
    from avsum_amd.features.extractors import VisualFeatureExtractor
    from avsum_amd.pipeline import FrameScoringPipeline
    from oracle import cnn as ocnn, scorer as osc
    torch.manual_seed(51)
    ext = VisualFeatureExtractor(torch.float32, "batch")
    model = _seeded_scorer(52)
    frames = _frames(7, 9)
    offsets = [0, 4, 7]  # two videos
    rsd, isd, ssd = ext.resnet.state_dict(), ext.inception.state_dict(), model.state_dict()
    with torch.no_grad():
        feats = []
        for f in frames:
            r = ocnn.resnet50_trunk_forward(rsd, ocnn.preprocess_frame(f))
            i = ocnn.inception_v3_forward(isd, ocnn.preprocess_inception(f))
            feats.append(torch.cat([r, i], 1))
        feats = torch.cat(feats)
        ref = torch.cat([osc.av_bilstm_forward(ssd, feats[a:b].unsqueeze(0), torch.zeros(1, b - a, 296)).reshape(-1)
                         for a, b in zip(offsets[:-1], offsets[1:])])
    pipe = FrameScoringPipeline(ext.to(dev), model.to(dev), use_inception=True, chunk_frames=4, frames_per_group=1)
    scores = pipe.score(torch.from_numpy(frames).to(dev), offsets)
    got = scores.cpu()
    assert (got - ref).abs().max().item() < 1e-4
    sel = pipe.select(scores, offsets)
    for (a, b), idx in zip(zip(offsets[:-1], offsets[1:]), sel):
        dropped, sel_ref = _guarded_equal_selection(got[a:b].numpy(), ref[a:b].numpy(), 2e-6)
        if dropped == 0:
            assert np.array_equal(idx, sel_ref)


def test_audio_extractor_api(dev):
    from avsum_amd.features.extractors import AudioFeatureExtractor
    from oracle import audio as oa
    torch.manual_seed(41)
    ext = AudioFeatureExtractor()
    t = np.arange(32000) / 16000.0
    wave = (0.4 * np.sin(2 * np.pi * 300 * t) + 0.01 * np.random.default_rng(0).standard_normal(32000)).astype(np.float32)
    lit = ext(wave)
    assert lit.dtype == np.float64 and lit.shape == (296,) and not lit.any()  # literal zeros
    assert ext(wave[:0]).dtype == np.float32
    mel = ext._extract_mel(torch.from_numpy(wave))
    assert mel.shape == (161, 128) and mel.dtype == np.float32
    truth = oa.extract_mel_f64(wave)
    ref32 = oa.extract_mel(torch.from_numpy(wave))
    assert np.abs(mel - truth).max() < 1e-4  # vs the float64 value of the reference's formula
    assert np.abs(mel - ref32).max() <= np.abs(ref32 - truth).max() + 1e-4  # vs the fp32 CPU reference
    mf = ext._extract_mfcc(torch.from_numpy(wave))
    ref = oa.extract_mfcc(torch.from_numpy(wave), ext.mfcc_proj.weight.detach().cpu(), ext.mfcc_proj.bias.detach().cpu())
    assert mf.shape == (161, 128) and np.abs(mf - ref).max() < 1e-4 * np.abs(ref).max()


def test_fusion_api(dev):
    from avsum_amd.features import fusion
    from oracle import fusion as ofu
    g = torch.Generator().manual_seed(2)
    v, a = torch.randn(60, 512, generator=g), torch.randn(80, 512, generator=g)
    c = fusion.compute_dtw(v, a)
    assert c.dtype == np.float64 and np.abs(c - ofu.compute_dtw(v, a)).max() < 1e-12 * c.max()
    path = fusion.compute_optimal_path(c)
    assert np.array_equal(path, ofu.compute_optimal_path(ofu.compute_dtw(v, a)))
    out = fusion.interpolate_features(v, path, 50)
    assert torch.equal(out, ofu.interpolate_features(v, path, 50))
    with pytest.raises(ValueError):
        fusion.compute_dtw(v, torch.randn(5, 7))


def test_train_synthetic_and_evaluate_scripts(dev, tmp_path):
    """BASELINE config 5 harness (reference loop on synthetic labels) runs on the HIP path and learns; then the
    reference's evaluate() loop over a dataset of the on-disk feature format."""
    from avsum_amd.data.dataset import BaseDataset, save_features
    from avsum_amd.scripts.evaluate import evaluate
    from avsum_amd.scripts.train_av_model import SyntheticShotDataset, train_on_dataset
    torch.manual_seed(1)
    ds = SyntheticShotDataset(num_videos=8, shots=(6, 12), seed=11)
    before = None
    losses = []
    model = train_on_dataset(ds, epochs=6, lr=1e-3, on_step=losses.append)
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]  # targets ~U[1,5] vs sigmoid outputs: the loss falls as the bias saturates
    rng = np.random.default_rng(0)
    for i in range(3):
        s = 9 + i
        save_features(str(tmp_path), f"vid{i}", rng.standard_normal((s, 4096)).astype(np.float32),
                      np.zeros((s, 296), np.float32))
        np.save(tmp_path / f"vid{i}" / "scores.npy", rng.random(s).astype(np.float32))
    # a fresh model for the evaluation loop: the over-trained one above saturates to a constant score, for which
    # the reference's unguarded precision / correlation are NaN (scripts/evaluate.py:29-36)
    out = evaluate(_seeded_scorer(4).to(dev), BaseDataset(str(tmp_path)))
    assert set(out) == {"f1", "spearman", "kendall"} and all(np.isfinite(list(out.values())))
    assert 0.0 <= out["f1"] <= 1.0
    with pytest.raises(ValueError):
        save_features(str(tmp_path), "bad", np.zeros((3, 100), np.float32), np.zeros((3, 296), np.float32))


def test_vggish_vs_oracle(dev):
    """VGGish on the HIP path (fp64-MFMA front end, fp32-MFMA network) against the CPU restatement: log-mel examples
    <= 1e-4 abs, embeddings <= 1e-4 of their scale, quantised output identical up to rare +-1 round-off flips."""
    from avsum_amd.vggish import VGGish, VGGishFrontEnd
    from oracle import vggish as ov
    torch.manual_seed(5)
    net = VGGish()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    rng = np.random.default_rng(3)
    t = np.arange(16000 * 3 + 777) / 16000.0
    wave = (0.4 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) + 0.05 * rng.standard_normal(t.size))
    wave = wave.astype(np.float32)
    ref_ex = ov.waveform_to_examples(wave)
    ex = VGGishFrontEnd.get(dev).examples(torch.from_numpy(wave).to(dev))
    assert ex.shape == (3, 96, 64) and (ex.cpu() - ref_ex[:, 0]).abs().max().item() < 1e-4
    with torch.no_grad():
        ref_emb = ov.network(sd, ref_ex)
        ref_out = ov.postprocess(sd, ref_emb)
    net = net.to(dev)
    emb = net.embed_examples(ex.contiguous()).cpu()
    assert (emb - ref_emb).abs().max().item() < 1e-4 * max(1.0, ref_emb.abs().max().item())
    out = net(wave, 16000).cpu()
    assert out.shape == (3, 128) and out.min() >= 0 and out.max() <= 255
    diff = (out - ref_out).abs()
    assert diff.max().item() <= 1 and (diff > 0).float().mean().item() < 0.01
    assert net(wave[:16000], 16000).shape == (128,)          # one example: squeezed like the hub model
    assert net(wave[:8000], 16000).shape == (0, 128)         # shorter than one example
    with pytest.raises(AttributeError):
        net(torch.from_numpy(wave))                          # the hub model only takes numpy / a path


def test_resample_and_audio_intent_mode(dev):
    from avsum_amd import ops
    from avsum_amd.audio import resample_to
    from avsum_amd.features.extractors import AVProcessor, AudioFeatureExtractor
    from oracle import audio as oa
    rng = np.random.default_rng(8)
    for sr, ch in ((48000, 1), (44100, 2), (22050, 1), (8000, 1), (16000, 2)):
        x = rng.standard_normal((sr // 2 + 13, ch)).astype(np.float32)
        ref = oa.resample_sinc(x, sr, 16000).numpy()
        got = resample_to(torch.from_numpy(x if ch > 1 else x[:, 0].copy()).to(dev), sr, 16000).cpu().numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() < 2e-5, (sr, ch)
    proc = AVProcessor(strict_reference=False)
    pcm = (rng.standard_normal((48000, 2)) * 8000).astype(np.int16)
    mono = proc.prepare_audio(pcm, 48000)
    assert mono.shape == (16000,) and mono.dtype == np.float32
    assert np.abs(mono - oa.resample_sinc(pcm.astype(np.float32) / 32768.0, 48000, 16000).numpy()).max() < 2e-5
    # "intent" mode of the audio extractor: [mean MFCC(40) | mean log2-mel(128) | mean VGGish(128)] = 296
    torch.manual_seed(1)
    ext = AudioFeatureExtractor(strict_reference=False)
    t = np.arange(40000) / 16000.0
    wave = (0.5 * np.sin(2 * np.pi * 660 * t)).astype(np.float32)
    feat = ext(wave)
    assert feat.shape == (296,) and np.isfinite(feat).all()
    from oracle import vggish as ov
    sd = {k: v.cpu() for k, v in ext.vggish.state_dict().items()}
    want = ov.vggish_forward(sd, wave).mean(0).numpy()
    assert np.abs(feat[168:] - want).max() <= 1.0
    assert np.abs(feat[40:168] - oa.extract_mel_f64(wave).mean(0)).max() < 1e-3
    assert np.array_equal(AudioFeatureExtractor()(wave), np.zeros(296))      # the literal reference behaviour stays
