"""Per-shot targets and the pairwise ranking loss without a GPU: the host definitions of avsum_amd.loss against a dense
float64 torch formulation, brute-force pair counts and the reference's align_shots_to_annotations; the planted mistakes,
each noticed by the cases of rank_loss_inputs; ops.RankTables and its refusals; the binding derived from
include/avsum_loss.h and the refusals of the entry points before any launch; collate_videos(targets="shots")."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rank_loss_inputs as rli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- rank_loss_host
@pytest.mark.parametrize("kind", rli.KINDS)
@pytest.mark.parametrize("name", ["main", "tied"])
def test_host_gradient_equals_autograd_through_the_dense_formulation(name, kind):
    s, y, off = rli.batch(name)
    losses, g, pairs = rli.host_reference(name, kind)
    dense, leaf = rli.dense_torch_loss(s, y, off, kind, rli.SCALE, rli.MARGIN)
    dense.sum().backward()
    # two float64 evaluations of one formula: they differ by summation order alone (T^2 terms at most, each < 2)
    t = int(np.diff(off).max())
    assert np.abs(dense.detach().numpy() - losses).max() <= 2 * t * t * rli.U
    assert np.abs(leaf.grad.numpy() - g).max() <= 2 * rli.SCALE * t * rli.U * 4
    assert pairs.tolist() == [rli.brute_force_pairs(y[a:b]) for a, b in zip(off[:-1], off[1:])]
    if name == "main":
        assert pairs[0] == 0 and pairs[1] == 1 and losses[0] == 0 and (g[:1] == 0).all()
        t5 = rli.LENGTHS[rli.QUANTISED]
        assert 0 < pairs[rli.QUANTISED] < t5 * (t5 - 1) // 2 * 0.85          # 5 levels: a fifth of the pairs are ties
        assert (losses[2:] > 0).all() and (kind == "hinge" or losses[1] > 0)   # (the one pair may clear the margin)
    else:
        assert pairs[1] == 0 and losses[1] == 0 and (g[off[1]:off[2]] == 0).all() and pairs[0] > 0 and pairs[2] > 0
    # the gradient of a video sums to zero (every pair pushes two rows by opposite amounts)
    for a, b in zip(off[:-1], off[1:]):
        assert abs(g[a:b].sum()) <= (b - a) * 4 * rli.U * max(1.0, np.abs(g[a:b]).sum())


@pytest.mark.parametrize("kind", rli.KINDS)
@pytest.mark.parametrize("planted", rli.RANK_PLANTED)
def test_planted_rank_mistakes_are_noticed(planted, kind):
    from avsum_amd.loss import rank_loss_host
    s, y, off = rli.batch("main")
    losses, g, pairs = rli.host_reference("main", kind)
    bad_l, bad_g, bad_p = rank_loss_host(s, y, off, kind, rli.SCALE, rli.MARGIN, planted=planted)
    t = int(np.diff(off).max())
    tol_l = max(rli.loss_bound(v, t) for v in losses)
    tol_g = rli.grad_bound(np.abs(g).max(), t, 1, rli.SCALE)
    noticed = {"losses": np.abs(bad_l - losses).max() > tol_l, "g": np.abs(bad_g - g).max() > tol_g,
               "pairs": bad_p.tolist() != pairs.tolist()}
    want = {"ge": ("pairs", "losses"), "t_squared": ("losses", "g"), "sign": ("g",)}[planted]
    for key in want:
        assert noticed[key], (planted, kind, key)


def test_planted_tile_mistake_is_noticed():
    from avsum_amd import ops
    table = ops.RankTables(rli.OFFSETS, device="cpu")
    good = rli.rows_covered(table.tiles.tolist(), rli.LENGTHS)
    assert all((c == 1).all() for c in good)
    bad = rli.rows_covered(rli.floor_tiles(rli.LENGTHS), rli.LENGTHS)
    assert bad[2][256] == 0 and bad[2][:256].all() and bad[3][1024] == 0        # row 256 of the 257-row video is dropped


# --------------------------------------------------------------------------- shot_targets_host
def _ulp_apart(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    return np.where(both_nan, 0.0, np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)))


@pytest.mark.parametrize("fps", rli.FPS_VALUES)
def test_shot_targets_host_equals_the_reference_alignment(fps):
    from avsum_amd.loss import shot_targets_host
    from avsum_amd.utils.alignments import align_shots_to_annotations
    ann, shots = rli.annotations(), rli.shot_case(fps)
    got, flags = shot_targets_host(ann, [0, ann.size], shots, [0, len(shots)], fps)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = align_shots_to_annotations(shots, ann.astype(np.float64), fps).numpy()
    assert got.dtype == np.float32 and flags.dtype == np.uint8 and flags.tolist() == [1]
    assert np.isnan(got[-1]) and np.isnan(want[-1]) and np.isfinite(got[:-1]).all()      # the shot that starts past the end
    assert (_ulp_apart(got, want.astype(np.float32)) <= 1).all()
    # the shot whose end bin runs past the annotations is the mean of the bins that exist
    start = int((shots[-2][0] / fps) // 2)
    assert start < ann.size and abs(got[-2] - ann[start:].astype(np.float64).mean()) <= np.spacing(got[-2])
    # the planted mistake: end_idx without the + 1
    bad, _ = shot_targets_host(ann, [0, ann.size], shots, [0, len(shots)], fps, planted="end_without_plus_one")
    assert (_ulp_apart(bad, want.astype(np.float32)) > 1).any() or np.isnan(bad[:-1]).any()


def test_shot_targets_host_batch_and_refusals():
    from avsum_amd.loss import shot_targets_host
    ann, aoff, shots, soff, fps = rli.shot_batch()
    got, flags = shot_targets_host(ann, aoff, shots, soff, fps)
    assert flags.tolist() == [1, 0, 1]
    for v in range(3):                                             # a video alone gives what it gives in the batch
        alone, f = shot_targets_host(ann[aoff[v]:aoff[v + 1]], [0, aoff[v + 1] - aoff[v]], shots[soff[v]:soff[v + 1]],
                                     [0, soff[v + 1] - soff[v]], fps[v])
        assert np.array_equal(alone, got[soff[v]:soff[v + 1]], equal_nan=True) and f[0] == flags[v]
    for bad in (dict(fps=0.0), dict(fps=[30.0, 30.0]), dict(fps=float("nan")), dict(bin_seconds=0.0),
                dict(shots=-shots), dict(shot_offsets=soff[:-1]), dict(ann_offsets=[0, 5, 3, ann.size])):
        kw = dict(annotations=ann, ann_offsets=aoff, shots=shots, shot_offsets=soff, fps=fps)
        kw.update(bad)
        with pytest.raises(ValueError):
            shot_targets_host(**kw)


# --------------------------------------------------------------------------- RankTables
def test_rank_tables_and_refusals(monkeypatch):
    from avsum_amd import _loss_abi, ops, ragged
    monkeypatch.setattr(_loss_abi, "LIB_PATH", "/nonexistent/libavsum_loss.so")      # device="cpu" needs no library
    monkeypatch.setattr(_loss_abi, "_lib", None)
    t = ops.RankTables(rli.OFFSETS, device="cpu")
    assert ops.RankTables is ragged.RankTables and isinstance(t, ragged.RaggedOffsets)
    assert (t.nseq, t.rows, t.max_t, t.ntiles) == (5, 1585, 1025, 1 + 1 + 2 + 5 + 2)
    assert t.tiles.dtype == np.int32 and t.tiles.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [3, 0], [3, 1], [3, 2],
                                                              [3, 3], [3, 4], [4, 0], [4, 1]]
    assert t.tiles_t.device.type == "cpu" and t.offsets_t.tolist() == rli.OFFSETS.tolist()
    assert ops.RankTables([0, 1], device="cpu").ntiles == 1                              # a one-row video is allowed
    assert ops.RankTables([0, 32768], device="cpu").ntiles == 128                        # the longest video
    assert ragged.RANK_TILE == _loss_abi.TILE == 256 and ragged.RANK_MAX_T == _loss_abi.MAX_T == 32768
    for bad in ([0, 32769], [0], [], [1, 4], [0, 4, 4], [0, 5, 3], [-1, 3]):
        with pytest.raises(ValueError):
            ops.RankTables(bad, device="cpu")
    with pytest.raises(ValueError, match="2\\^31"):
        ops.RankTables(np.arange(0, 2 ** 31 + 32768, 32768), device="cpu")               # 2^31 rows
    with pytest.raises(ValueError):
        ops.RankTables([0, 4, 9], rows=10, device="cpu")
    with pytest.raises(_loss_abi.AvslError, match="has not been built"):
        _loss_abi.lib()


# --------------------------------------------------------------------------- the binding
def test_binding_is_derived_from_the_header():
    from avsum_amd import _loss_abi as abi
    text = open(os.path.join(ROOT, "include", "avsum_loss.h")).read()
    declared = set(re.findall(r"\b(avsl_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    assert declared == set(abi.declared_symbols()) == set(abi._SIGNATURES)
    assert declared == {"avsl_abi_version", "avsl_last_error", "avsl_shot_targets_f32", "avsl_rank_workspace_bytes",
                        "avsl_rank_loss_f32", "avsl_rank_loss_bwd_f32"}
    assert abi.ABI_VERSION == int(re.search(r"#define\s+AVSL_ABI_VERSION\s+(\d+)", text).group(1))
    assert abi.KINDS == {"logistic": 0, "hinge": 1} and abi.SHARED["AVSL_OK"] == 0 and abi.CHUNK == 1024
    lib = abi.lib()                                    # loads without a GPU; every prototype is bound with its types
    assert lib.avsl_abi_version() == abi.ABI_VERSION
    for name, (res, args) in abi._SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    res, args = abi._SIGNATURES["avsl_rank_loss_f32"]
    assert res is ctypes.c_int and args[9] is ctypes.c_double and args[10] is ctypes.c_double
    assert args[12] is ctypes.c_size_t and abi._SIGNATURES["avsl_rank_workspace_bytes"][0] is ctypes.c_size_t
    assert lib.avsl_rank_workspace_bytes(0) == 0 and lib.avsl_rank_workspace_bytes(1) == 768
    assert lib.avsl_rank_workspace_bytes(1585) >= 20 * 1585
    # the source includes its own header only, and the Makefile builds it into its own library
    src = open(os.path.join(os.path.dirname(os.path.dirname(abi.LIB_PATH)), "csrc", "loss.hip")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["../../include/avsum_loss.h"]
    assert not re.search(r"atomicAdd|atomicCAS|__hip_atomic|hipMalloc|hipFree|hipDeviceSynchronize|hipMemcpy", src)


def test_module_imports_math_numpy_and_torch_only():
    import avsum_amd.loss as m
    top = re.findall(r"^(?:import|from)\s+(\S+)", open(m.__file__).read(), flags=re.M)
    assert sorted(top) == ["math", "numpy", "torch"]


def test_refusals_before_any_launch():
    """Every refusal of the entry points comes back as a status with a message, before any HIP call (no GPU here)."""
    from avsum_amd import _loss_abi as abi
    lib, C = abi.lib(), abi.SHARED
    fake = 4096    # a non-null, aligned "pointer" that is never dereferenced on the paths below

    def rank(scores=fake, targets=fake, rows=8, off=fake, nseq=2, tiles=fake, ntiles=2, max_t=5, kind=0, scale=1.0,
             margin=0.1, ws=fake, ws_bytes=1 << 20, losses=fake, g=fake, pairs=fake):
        return lib.avsl_rank_loss_f32(scores, targets, rows, off, nseq, tiles, ntiles, max_t, kind, scale, margin, ws,
                                      ws_bytes, losses, g, pairs, None)

    def message():
        return lib.avsl_last_error().decode()

    assert rank(rows=0) == C["AVSL_E_SHAPE"] and "rows" in message()
    assert rank(rows=abi.MAX_ROWS + 1) == C["AVSL_E_SHAPE"]
    assert rank(nseq=0) == C["AVSL_E_SHAPE"] and rank(nseq=9) == C["AVSL_E_SHAPE"] and "nseq" in message()
    assert rank(ntiles=1) == C["AVSL_E_SHAPE"] and "ntiles" in message()
    assert rank(max_t=0) == C["AVSL_E_SHAPE"] and rank(max_t=abi.MAX_T + 1) == C["AVSL_E_SHAPE"] and "max_t" in message()
    assert rank(kind=2) == C["AVSL_E_ARG"] and "kind" in message()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert rank(scale=bad) == C["AVSL_E_ARG"] and "scale" in message()
    assert rank(margin=float("nan")) == C["AVSL_E_ARG"] and "margin" in message()
    for name in ("scores", "targets", "off", "tiles", "ws", "losses", "g", "pairs"):
        assert rank(**{name: None}) == C["AVSL_E_ARG"] and "null" in message(), name
    assert rank(ws_bytes=lib.avsl_rank_workspace_bytes(8) - 1) == C["AVSL_E_SHAPE"] and "workspace" in message()
    assert rank(ws=fake + 4) == C["AVSL_E_ALIGN"] and rank(off=fake + 4) == C["AVSL_E_ALIGN"]
    assert rank(scores=fake + 2) == C["AVSL_E_ALIGN"] and rank(pairs=fake + 4) == C["AVSL_E_ALIGN"]
    bwd = lib.avsl_rank_loss_bwd_f32
    assert bwd(None, fake, 8, fake, 2, fake, None) == C["AVSL_E_ARG"]
    assert bwd(fake, fake, 0, fake, 2, fake, None) == C["AVSL_E_SHAPE"]
    assert bwd(fake, fake, 8, fake, 9, fake, None) == C["AVSL_E_SHAPE"]
    assert bwd(fake, fake, 8, fake + 4, 2, fake, None) == C["AVSL_E_ALIGN"]

    def shot(ann=fake, nann=10, aoff=fake, shots=fake, nshots=4, soff=fake, fps=fake, nv=2, bin_s=2.0, out=fake,
             flags=fake):
        return lib.avsl_shot_targets_f32(ann, nann, aoff, shots, nshots, soff, fps, nv, bin_s, out, flags, None)

    assert shot(nv=0) == C["AVSL_E_ARG"] and "nvideos" in message()
    assert shot(nann=-1) == C["AVSL_E_SHAPE"] and shot(nshots=abi.MAX_ROWS + 1) == C["AVSL_E_SHAPE"]
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert shot(bin_s=bad) == C["AVSL_E_ARG"] and "bin_seconds" in message()
    for name in ("ann", "aoff", "shots", "soff", "fps", "out", "flags"):
        assert shot(**{name: None}) == C["AVSL_E_ARG"] and "null" in message(), name
    assert shot(fps=fake + 4) == C["AVSL_E_ALIGN"] and shot(shots=fake + 4) == C["AVSL_E_ALIGN"]


def test_launch_wrappers_refuse_host_tensors_and_bad_arguments():
    from avsum_amd import loss
    s, y = torch.rand(9), torch.rand(9)
    with pytest.raises(ValueError, match="no CPU fallback"):
        loss.rank_loss(s, y, [0, 4, 9])
    with pytest.raises(ValueError, match="no CPU fallback"):
        loss.shot_targets(torch.rand(5), [0, 5], [(0, 30)], [0, 1], 30)
    for bad in (dict(kind="softmax"), dict(scale=0.0), dict(scale=float("inf")), dict(margin=float("nan"))):
        with pytest.raises(ValueError):
            loss.rank_loss(s, y, [0, 4, 9], **bad)
        with pytest.raises(ValueError):
            loss.rank_loss_host(s.numpy(), y.numpy(), [0, 4, 9], **bad)
    for bad_off in ([0, 4, 8], [1, 9], [0, 4, 4, 9]):
        with pytest.raises(ValueError):
            loss.rank_loss_host(s.numpy(), y.numpy(), bad_off)


# --------------------------------------------------------------------------- the training interface, host side
def _items(with_shots=True):
    from avsum_amd.scripts.train_av_model import SyntheticShotDataset
    ds = SyntheticShotDataset(num_videos=3, shots=(4, 9), seed=5, visual_dim=8, audio_dim=4, with_shots=with_shots)
    return [ds[i] for i in range(len(ds))]


def test_synthetic_shots_partition_the_frames_and_leave_the_items_alone():
    plain, shot = _items(False), _items(True)
    for (fp, sp), (fs, ss) in zip(plain, shot):
        assert "shots" not in fp and torch.equal(fp["visual"], fs["visual"]) and torch.equal(sp, ss)
        table, s = fs["shots"], fs["visual"].shape[0]
        assert table.dtype == torch.int64 and tuple(table.shape) == (s, 2)
        assert table[0, 0] == 0 and table[-1, 1] == 30 * s and torch.equal(table[1:, 0], table[:-1, 1])
        assert (table[:, 1] > table[:, 0]).all()
    lengths = [int((f["shots"][:, 1] - f["shots"][:, 0]).max()) for f, _ in shot]
    assert max(lengths) > 30                                        # ragged: not the uniform 30-frame partition


def test_collate_videos_default_is_unchanged_and_shots_form():
    from avsum_amd.scripts.train_av_model import collate_videos
    from avsum_amd.utils.alignments import align_shots_to_annotations
    items = _items()
    visual, audio, offsets, targets = collate_videos(items)
    lengths = [f["visual"].shape[0] for f, _ in items]
    assert torch.equal(visual, torch.cat([f["visual"] for f, _ in items])) and audio.shape == (sum(lengths), 4)
    assert offsets.dtype == torch.int64 and offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    want = torch.cat([align_shots_to_annotations([(0, n)], sc.numpy(), 30).float().reshape(1)
                      for n, (_, sc) in zip(lengths, items)])
    assert targets.dtype == torch.float32 and torch.equal(targets, want)
    same = collate_videos(items, targets="video")
    assert all(torch.equal(a, b) for a, b in zip(same, (visual, audio, offsets, targets)))
    v2, a2, off2, (ann, ann_off, shots) = collate_videos(items, targets="shots")
    assert torch.equal(v2, visual) and torch.equal(a2, audio) and torch.equal(off2, offsets)
    assert ann.dtype == torch.float32 and torch.equal(ann, torch.cat([sc for _, sc in items]))
    assert ann_off.tolist() == np.concatenate([[0], np.cumsum([30 * n for n in lengths])]).tolist()
    assert shots.dtype == torch.int64 and torch.equal(shots, torch.cat([f["shots"] for f, _ in items]))


def test_collate_videos_shots_refusals():
    from avsum_amd.scripts.train_av_model import collate_videos
    with pytest.raises(ValueError, match="targets must be"):
        collate_videos(_items(), targets="rows")
    with pytest.raises(ValueError, match="needs features\\['shots'\\]"):
        collate_videos(_items(False), targets="shots")
    for spoil in (lambda t: t[:-1], lambda t: t.to(torch.int32), lambda t: t.reshape(-1), lambda t: torch.cat([t, t], 1)):
        items = _items()
        items[1][0]["shots"] = spoil(items[1][0]["shots"])
        with pytest.raises(ValueError, match="video 1"):
            collate_videos(items, targets="shots")
    with pytest.raises(ValueError, match="no video"):
        collate_videos([], targets="shots")


def test_objective_refusals_need_no_device():
    from avsum_amd.scripts import train_av_model as tr
    items = _items()
    for kw in (dict(loss="rank"), dict(loss="mse+rank"), dict(loss="rank", targets="video"), dict(loss="l1"),
               dict(targets="frames")):
        with pytest.raises(ValueError):
            tr.train_step_batch(None, None, items, "cpu", **kw)
    ds = tr.SyntheticShotDataset(num_videos=3, shots=(4, 9), seed=5, visual_dim=8, audio_dim=4, with_shots=True)
    for kw in (dict(targets="shots"), dict(targets="shots", loss="mse+rank"), dict(targets="shots", loss="rank")):
        with pytest.raises(ValueError, match="videos_per_step"):
            tr.train_on_dataset(ds, epochs=1, device="cpu", videos_per_step=1, **kw)
    with pytest.raises(ValueError, match="needs targets='shots'"):
        tr.train_on_dataset(ds, epochs=1, device="cpu", videos_per_step=4, loss="rank")


def test_save_features_writes_shots_only_when_given(tmp_path):
    from avsum_amd.data.dataset import BaseDataset, save_features
    visual, audio = np.zeros((3, 4096), np.float32), np.zeros((3, 296), np.float32)
    save_features(str(tmp_path), "a", visual, audio)
    save_features(str(tmp_path), "b", visual, audio, shots=[(0, 10), (10, 25), (25, 90)])
    for vid in ("a", "b"):
        np.save(os.path.join(str(tmp_path), vid, "scores.npy"), np.ones(90, np.float32))
    ds = BaseDataset(str(tmp_path))
    assert sorted(os.listdir(os.path.join(str(tmp_path), "a"))) == ["audio.npy", "scores.npy", "visual.npy"]
    assert set(ds[0][0]) == {"visual", "audio"} and set(ds[1][0]) == {"visual", "audio", "shots"}
    assert ds[1][0]["shots"].dtype == torch.int64 and ds[1][0]["shots"].tolist() == [[0, 10], [10, 25], [25, 90]]
    with pytest.raises(ValueError, match="shot table"):
        save_features(str(tmp_path), "c", visual, audio, shots=[(0, 10)])
