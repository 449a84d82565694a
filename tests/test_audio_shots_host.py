"""Per-shot audio tables on the host (audio.MelPlan.shot_tables on device="cpu") and the argument checks of the per-shot
C entries, which return before any launch: no GPU needed."""
import numpy as np
import torch

ARG, SHAPE, WORKSPACE = -1, -2, -5   # AVS_E_ARG, AVS_E_SHAPE, AVS_E_WORKSPACE


def _tables(waves, bounds):
    from avsum_amd.audio import MelPlan
    return MelPlan.shot_tables(waves, bounds, "cpu")


def test_shot_tables_frames_blocks_examples_and_slices():
    from avsum_amd.vggish import VGGishFrontEnd
    waves = [np.zeros(50003, np.float32), torch.zeros(36001, dtype=torch.float64), np.zeros(20000, np.float32)]
    bounds = [[(0, 17000), (5, 6), (700, 700), (45001, 60000), (39001, 41500), (100, 450), (900, 100), (-1000, -10)],
              [(3, 19000), (35000, 36001)],
              [(0, 20000), (15599, 31199)]]
    tb = _tables(waves, bounds)
    lens = [len(range(*slice(a, b).indices(w.shape[0]))) for w, bb in zip(waves, bounds) for a, b in bb]
    assert lens == [17000, 1, 0, 5002, 2499, 350, 0, 990, 18997, 1001, 20000, 4401]
    shots = tb.shots.numpy()
    assert shots.shape == (12, 3) and shots[:, 2].tolist() == lens
    assert shots[:, 0].tolist() == [0] * 8 + [1] * 2 + [2] * 2
    assert shots[3, 1] == 45001 and shots[7, 1] == 50003 - 1000 and shots[6, 2] == 0   # clipped, negative, reversed
    # frames: 1 + max(L, 960) // 200 per non-empty shot, none for an empty one
    want_frames = [1 + max(n, 960) // 200 if n else 0 for n in lens]
    assert tb.seg_frames.numpy().tolist() == want_frames
    # blocks: each shot in runs of at most 32 frames, in order, covering exactly its frames
    blocks, seg_block = tb.blocks.numpy(), tb.seg_block.numpy()
    assert blocks.shape[1] == 3 and (blocks[:, 1] >= 1).all() and (blocks[:, 1] <= 32).all()
    for s, nf in enumerate(want_frames):
        rows = blocks[seg_block[s]:seg_block[s + 1]]
        assert (rows[:, 2] == s).all()
        assert rows[:, 0].tolist() == list(range(0, nf, 32)) and rows[:, 1].sum() == nf
    # VGGish examples: num_examples(Lp), none below 15 600 samples; starts inside the buffer at the shot's offset
    want_ex = [VGGishFrontEnd.num_examples(max(n, 960)) if n else 0 for n in lens]
    assert want_ex == [1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0]
    assert np.diff(tb.ex_seg.numpy()).tolist() == want_ex
    offs = tb.track_off.numpy()
    assert (offs % 4 == 0).all() and tb.track_len.numpy().tolist() == [50003, 36001, 20000]
    assert tb.waves.numel() % 4 == 0 and tb.waves.dtype == torch.float32
    assert tb.ex_start.numpy().tolist() == [offs[0] + 0, offs[1] + 3, offs[2] + 0]


def test_shot_tables_copy_the_tracks():
    rng = np.random.default_rng(0)
    waves = [rng.standard_normal(n).astype(np.float32) * 2 for n in (1001, 7, 4096)]
    tb = _tables(waves, [[(0, 5)], [], [(1, 2)]])
    for w, o in zip(waves, tb.track_off.tolist()):
        assert np.array_equal(tb.waves[o:o + w.size].numpy(), w)   # stored unclamped: the clamp happens at load
    assert tb.seg_block.numel() == 3 and tb.ex_seg.tolist() == [0, 0, 0]


def test_shot_tables_empty_batch():
    tb = _tables([np.zeros(100, np.float32)], [[]])
    assert tb.shots.shape == (0, 3) and tb.blocks.shape == (0, 3) and tb.seg_block.tolist() == [0]


def test_shot_entries_validate_before_launch():
    from avsum_amd import _abi
    lib = _abi.lib()
    P = [None] * 64
    ws_need = lib.avs_stft_mel_shots_workspace_bytes(10, 128, 1, 1)
    assert ws_need == 10 * 128 * 4 * (2 + 32)
    assert lib.avs_stft_mel_shots_workspace_bytes(3, 128, 1, 0) == 3 * 128 * 4
    assert lib.avs_stft_mel_shots_workspace_bytes(-1, 128, 1, 1) < 0
    # negative counts / a waveform buffer that is not a whole number of 16-byte quads
    assert lib.avs_stft_mel_shots_f32(None, 8, None, None, -1, None, 1, *P[:6], 128, None, 0, None, None, None, 80.0,
                                      None, 128, None, 128, None, 0, None) == SHAPE
    assert lib.avs_stft_mel_shots_f32(None, 6, None, None, 1, None, 1, *P[:6], 128, None, 0, None, None, None, 80.0,
                                      None, 128, None, 128, None, 0, None) == SHAPE
    assert lib.avs_stft_mel_shots_f32(None, 8, None, None, 1, None, -2, *P[:6], 128, None, 0, None, None, None, 80.0,
                                      None, 128, None, 128, None, 0, None) == SHAPE
    # null pointers
    assert lib.avs_stft_mel_shots_f32(None, 8, None, None, 1, None, 1, *P[:6], 128, None, 1, None, None, None, 80.0,
                                      None, 128, None, 128, None, 0, None) == ARG
    assert b"null" in lib.avs_last_error()
    # a workspace that is too short (all pointers plausible, nothing dereferenced on the host)
    fake = 1 << 20   # a 16-byte aligned non-null address; never read, the call returns before any HIP call
    assert lib.avs_stft_mel_shots_f32(fake, 8, fake, fake, 1, fake, 1, fake, fake, fake, fake, fake, fake, 128, fake, 1,
                                      fake, fake, fake, 80.0, fake, 128, fake, 128, fake, ws_need // 10 - 1, None) == WORKSPACE
    assert b"workspace" in lib.avs_last_error()
    # the VGGish examples entry
    assert lib.avs_vggish_examples_workspace_bytes(3) == 3 * 96 * 514 * 4
    assert lib.avs_vggish_examples_workspace_bytes(-1) < 0
    assert lib.avs_vggish_examples_f32(None, 20000, None, -1, None, 576, None, None, None, 64, None, None, 0, None) == SHAPE
    assert lib.avs_vggish_examples_f32(None, 20000, None, 2, None, 576, None, None, None, 64, None, None, 0, None) == ARG
    assert lib.avs_vggish_examples_f32(fake, 100, fake, 2, fake, 576, fake, fake, fake, 64, fake, fake, 1 << 30,
                                       None) == SHAPE    # a buffer shorter than one example
    assert lib.avs_vggish_examples_f32(fake, 20000, fake, 2, fake, 576, fake, fake, fake, 64, fake, fake, 100, None) == WORKSPACE
    assert b"workspace" in lib.avs_last_error()
    # nothing to do: no launch, success
    assert lib.avs_vggish_examples_f32(None, 0, None, 0, None, 576, None, None, None, 64, None, None, 0, None) == 0
