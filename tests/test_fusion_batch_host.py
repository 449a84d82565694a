"""Batched fusion on the host: the table builder (ops.FusionTables on device="cpu"), the argument checks of the batched
C entries (they return before any launch), and the properties of the GPU tests' inputs the batched kernels rely on.
No GPU needed."""
import numpy as np
import pytest
import torch

import fusion_batch_inputs as fbi
from oracle import fusion as ofu

ARG, SHAPE, WORKSPACE = -1, -2, -5   # AVS_E_ARG, AVS_E_SHAPE, AVS_E_WORKSPACE


def test_tables_offsets_classes_tiles_workspace():
    from avsum_amd import ops
    # five pairs, a gap of 10 visual / 3 audio rows before the second, classes 1, 0, 0, 0, 2 (by min(n, m): 300, 1, 31,
    # 5, 1100 against the boundaries 64 and 512)
    pairs = [(0, 700, 0, 300), (710, 1, 303, 1), (711, 33, 304, 31), (744, 5, 335, 9), (749, 1500, 344, 1100)]
    tb = ops.FusionTables(pairs, "cpu")
    assert tb.npairs == 5 and tb.max_n == 1500
    assert tb.cell_off.tolist() == [0, 210000, 210001, 211024, 211069] and tb.cells == 211069 + 1500 * 1100
    assert tb.path_cap.tolist() == [999, 1, 63, 13, 2599]                 # n + m - 1
    assert tb.path_off.tolist() == [0, 999, 1000, 1063, 1076] and tb.path_rows == 3675
    assert tb.row_off.tolist() == [0, 700, 701, 734, 739] and tb.rows == 2239
    assert tb.cls.tolist() == [1, 0, 0, 0, 2]
    assert tb.class_count == [3, 1, 1] and tb.class_max_l == [31, 300, 1100]
    # class 0 first, inside a class the most anti-diagonals first: (33,31), (5,9), (1,1); then (700,300); then (1500,1100)
    assert tb.order.tolist() == [2, 3, 1, 0, 4]
    # 32x32 cost tiles: 22*10 + 1 + 2*1 + 1*1 + 47*35
    assert tb.ntiles == 220 + 1 + 2 + 1 + 1645 and tb.tiles.shape == (1869, 3) and tb.tiles.dtype == np.int32
    assert tb.tiles[:11].tolist() == [[0, 0, j] for j in range(10)] + [[0, 1, 0]]
    assert tb.tiles[220:224].tolist() == [[1, 0, 0], [2, 0, 0], [2, 1, 0], [3, 0, 0]] and tb.tiles[-1].tolist() == [4, 46, 34]
    # every cell of every pair is covered by exactly one tile
    for p, (_, n, _, m) in enumerate(pairs):
        t = tb.tiles[tb.tiles[:, 0] == p]
        assert len(t) == -(-n // 32) * -(-m // 32) and len({(i, j) for _, i, j in t.tolist()}) == len(t)
    from avsum_amd import _abi
    assert tb.workspace_bytes == _abi.lib().avs_dtw_batch_workspace_bytes(tb.cells) == (tb.cells + 255) // 256 * 256
    table = tb.pairs.numpy()
    assert table.shape == (5, 8) and table.dtype == np.int64
    assert table[4].tolist() == [749, 1500, 344, 1100, 211069, 1076, 739, 0]
    assert tb.row_pair.numpy().tolist() == [0] * 700 + [1] + [2] * 33 + [3] * 5 + [4] * 1500
    assert tb.v_rows_needed == 2249 and tb.a_rows_needed == 1444
    # the fused output: min(n, target_length) rows per pair
    off, total = tb.out_offsets(None)
    assert off.tolist() == [0, 700, 701, 734, 739, 2239] and total == 2239
    off, total = tb.out_offsets(40)
    assert off.tolist() == [0, 40, 41, 74, 79, 119] and total == 119


def test_tables_refuse_bad_pairs():
    from avsum_amd import ops
    ops.FusionTables([(0, 6400, 0, 3)], "cpu")
    for bad in ([(0, 6401, 0, 3)], [(0, 0, 0, 3)], [(0, 3, 0, 0)], [(0, 5, 0, 5), (-1, 2, 0, 2)]):
        with pytest.raises(ValueError):
            ops.FusionTables(bad, "cpu")
    empty = ops.FusionTables([], "cpu")
    assert empty.npairs == 0 and empty.cells == 0 and empty.ntiles == 0 and empty.class_count == [0, 0, 0]


def test_batch_entries_validate_before_launch():
    from avsum_amd import _abi
    lib = _abi.lib()
    fake = 1 << 20   # a 16-byte aligned non-null address; never read, the calls return before any HIP call
    assert lib.avs_dtw_batch_workspace_bytes(0) == 0 and lib.avs_dtw_batch_workspace_bytes(-5) == 0
    assert lib.avs_dtw_batch_workspace_bytes(1) == 256 and lib.avs_dtw_batch_workspace_bytes(257) == 512
    # cost matrices
    assert lib.avs_cdist_batch_f64(fake, 10, fake, 10, 0, fake, 1, fake, 1, fake, 100, None) == SHAPE      # d = 0
    assert lib.avs_cdist_batch_f64(fake, 10, fake, 10, 8, fake, -1, fake, 1, fake, 100, None) == SHAPE
    assert lib.avs_cdist_batch_f64(fake, 10, fake, 10, 8, fake, 3, fake, 2, fake, 100, None) == SHAPE      # tiles < pairs
    assert lib.avs_cdist_batch_f64(fake, 0, fake, 10, 8, fake, 1, fake, 1, fake, 100, None) == SHAPE       # no rows
    assert lib.avs_cdist_batch_f64(None, 10, fake, 10, 8, fake, 1, fake, 1, fake, 100, None) == ARG
    assert b"null" in lib.avs_last_error()
    assert lib.avs_cdist_batch_f64(fake, 10, fake, 10, 8, fake, 1, None, 1, fake, 100, None) == ARG
    assert lib.avs_cdist_batch_f64(None, 0, None, 0, 8, None, 0, None, 0, None, 0, None) == 0              # nothing to do
    # DTW: (cost, cells, pairs, npairs, order, n_small, n_mid, n_large, max_l x 3, max_n, ws, ws_bytes, path, len, total, rc)
    def dtw(counts=(1, 1, 1), max_l=(64, 512, 6400), max_n=6400, cells=1000, npairs=3, ws=1024, ptr=fake, rc=fake):
        return lib.avs_dtw_batch_f64(ptr, cells, fake, npairs, fake, *counts, *max_l, max_n, fake, ws, fake, fake, fake, rc, None)
    assert dtw(max_n=6401) == SHAPE and b"6400" in lib.avs_last_error()
    assert dtw(counts=(1, 1, 2)) == SHAPE                      # classes do not add up to the pairs
    assert dtw(max_l=(65, 512, 6400)) == SHAPE                 # a class-0 pair needs one lane per diagonal cell
    assert dtw(max_l=(64, 513, 6400)) == SHAPE
    assert dtw(max_l=(64, 512, 6401)) == SHAPE
    assert dtw(max_l=(64, 64, 6400)) == SHAPE                  # a pair in a class it does not belong to
    assert dtw(ws=768) == WORKSPACE and b"workspace" in lib.avs_last_error()   # 1000 cells need 1024 bytes
    assert dtw(counts=(0, 0, 3), max_l=(0, 0, 600), ws=1023) == WORKSPACE
    assert dtw(ptr=None) == ARG and dtw(rc=None) == ARG
    assert dtw(counts=(0, 0, 0), npairs=0, cells=0, ptr=None) == 0
    # gather: (x, ldx, d, pairs, npairs, row_pair, nrows, out_off, rowcount, path_len, target_length, out)
    assert lib.avs_fused_gather_batch_f32(fake, 8, 16, fake, 1, fake, 4, fake, fake, fake, 4, fake, None) == SHAPE   # ldx < d
    assert lib.avs_fused_gather_batch_f32(fake, 16, 16, fake, 5, fake, 4, fake, fake, fake, 4, fake, None) == SHAPE  # rows < pairs
    assert lib.avs_fused_gather_batch_f32(fake, 16, 16, fake, 1, fake, 4, fake, fake, fake, -1, fake, None) == SHAPE
    assert lib.avs_fused_gather_batch_f32(fake, 16, 16, fake, 1, None, 4, fake, fake, fake, 4, fake, None) == ARG
    assert lib.avs_fused_gather_batch_f32(None, 16, 16, None, 0, None, 0, None, None, None, 4, None, None) == 0


def _gpu_test_pairs():
    return (fbi.walk_batch(fbi.BATCH_D24, 24) + fbi.walk_batch(fbi.BATCH_D512, 512), fbi.oracle_batch("d24") + fbi.oracle_batch("d512"))


def test_inputs_paths_do_not_sit_on_rounding_ties():
    """Every random-walk pair of the GPU tests keeps its oracle path when the cost is summed in reversed k order: a
    kernel whose cost differs from SciPy's in the last bit still has ONE right path to find."""
    pairs, refs = _gpu_test_pairs()
    warp_rows = warp_cols = 0
    for (v, a), (cost, path) in zip(pairs, refs):
        rev = fbi.cost_reversed(v, a)
        assert np.allclose(rev, cost, rtol=1e-12, atol=0)
        assert np.array_equal(ofu.compute_optimal_path(rev), path), tuple(cost.shape)
        warp_rows = max(warp_rows, np.bincount(path[:, 0]).max())
        warp_cols = max(warp_cols, np.bincount(path[:, 1]).max())
    assert warp_rows >= 8 and warp_cols >= 8     # the paths warp both ways: not the near-diagonal of plain Gaussian rows


def test_rowcount_identity():
    """What lets the batched gather drop unique() and the host round trip: a path visits every row 0..n-1, and
    interpolate_features is v * float32(rowcount / L), bit for bit."""
    pairs, refs = _gpu_test_pairs()
    small, small_refs = fbi.small_batch()[:200], fbi.oracle_batch("small")[:200]
    for (v, a), (_, path) in zip(pairs + small, refs + small_refs):
        n = v.shape[0]
        assert np.array_equal(np.unique(path[:, 0]), np.arange(n))
        rowcount = np.bincount(path[:, 0], minlength=n)
        w = (rowcount.astype(np.float64) / np.float64(len(path))).astype(np.float32)
        for tl in (40, n):
            assert torch.equal(ofu.interpolate_features(v, path, tl), (v * torch.from_numpy(w)[:, None])[:tl])


def test_tie_inputs_take_all_three_steps():
    lens = [len(path) for _, path in fbi.oracle_batch("tie")]
    for (n, m), (cost, path) in zip(fbi.TIE_SHAPES, fbi.oracle_batch("tie")):
        steps = np.diff(path, axis=0)
        assert {tuple(s) for s in steps.tolist()} == {(1, 0), (0, 1), (1, 1)}, (n, m)
    assert all(max(n, m) <= ln <= n + m - 1 for (n, m), ln in zip(fbi.TIE_SHAPES, lens))
