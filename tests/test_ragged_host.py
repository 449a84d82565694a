"""The host plans of the ragged-batch layers (avsum_amd.ragged), pinned without a GPU.  tests/golden/
ragged_tables_host.json holds what ops.EvalTables, ops.SeqTable, ops.ShotTables and ops.FusionTables built or refused
over a corpus of offsets and pair lists BEFORE they were rebuilt on one validated offsets table; every attribute and
every refusal's type must still be the same (tests/golden/make_ragged_tables_golden.py records the file and defines the
replay)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PREFIX = {"EvalTables": "eval_counts: ", "SeqTable": "SeqTable: ", "ShotTables": "ShotTables: ",
          "FusionTables": "fusion_batch: "}
# one refusal per rule and class: (case id, words of which the message holds one)
RULES = {
    "EvalTables": {"entry count": ("EvalTables | []", ("V + 1",)),
                   "start": ("EvalTables | [-2, 5]", ("negative",)),
                   "order": ("EvalTables | [0, 5, 3]", ("decrease",)),
                   "shortest segment": ("EvalTables | [0, 1]", ("at least 2",)),
                   "longest segment": ("EvalTables | [0, 32769]", ("32768",)),
                   "total": ("EvalTables | [2147483638, 2147483658]", ("2^31",))},
    "SeqTable": {"entry count": ("SeqTable rows=None | [0]", ("V + 1",)),
                 "start": ("SeqTable rows=None | [1, 4]", ("start at 0",)),
                 "order": ("SeqTable rows=None | [0, 5, 3]", ("decrease", "increase")),
                 "shortest segment": ("SeqTable rows=None | [0, 5, 5]", ("empty", "at least 1")),
                 "total": ("SeqTable rows=None | [0, 2147483648]", ("2^31",)),
                 "rows mismatch": ("SeqTable rows=last + 1 | [0, 2]", ("the batch has 3 rows",))},
    "ShotTables": {"entry count": ("ShotTables min_scene_len=15 | [0]", ("V + 1",)),
                   "start": ("ShotTables min_scene_len=15 | [1, 4]", ("start at 0",)),
                   "order": ("ShotTables min_scene_len=15 | [0, 5, 3]", ("decrease", "ascend")),
                   "shortest segment": ("ShotTables min_scene_len=15 | [0, 5, 5]", ("empty", "at least 1")),
                   "total": ("ShotTables min_scene_len=15 | [0, 16777217]", ("2^24",)),
                   "min_scene_len": ("ShotTables min_scene_len=0 | [0, 2]", ("min_scene_len",))},
    "FusionTables": {"empty pair": ("FusionTables | n = 0", ("empty",)),
                     "start": ("FusionTables | negative v_row0", ("negative",)),
                     "longest segment": ("FusionTables | n = 6401", ("6400",))},
}


def _recorder():
    spec = importlib.util.spec_from_file_location("make_ragged_tables_golden",
                                                  os.path.join(GOLDEN, "make_ragged_tables_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replayed():
    """(recorded results, results of the tree under test), the corpus replayed once."""
    from avsum_amd import ops
    rec = _recorder()
    with open(os.path.join(GOLDEN, "ragged_tables_host.json")) as f:
        corpus = json.load(f)
    want = rec.expand(corpus)
    return want, rec.replay(ops, corpus, want)


def test_plans_build_and_refuse_as_recorded(replayed):
    want, got = replayed
    assert list(got) == list(want) and len(want) > 500
    wrong = []
    for key, w in want.items():
        g = got[key]
        if "ok" in w:
            if "ok" not in g:
                wrong.append((key, "refused", g))
            else:
                wrong += [(key, name, g["ok"][name], value) for name, value in w["ok"].items() if g["ok"][name] != value]
        elif g.get("error") != w["error"]:
            wrong.append((key, g.get("error", "accepted"), w["error"]))
        elif not g["message"].startswith(PREFIX[key.split(" ")[0]]):
            wrong.append((key, "message", g["message"]))
    assert not wrong, f"{len(wrong)} differences, first: {wrong[:5]}"


def test_corpus_reaches_every_rule(replayed):
    want, got = replayed
    for cls, rules in RULES.items():
        assert any("ok" in r for key, r in want.items() if key.startswith(cls + " ")), cls
        for rule, (key, words) in rules.items():
            assert want[key] == {"error": "ValueError"}, (cls, rule)
            assert any(word in got[key]["message"] for word in words), (cls, rule, got[key]["message"])
    # the accepted limits sit next to the refused ones
    for key in ("EvalTables | [0]", "EvalTables | [1, 4]", "EvalTables | [0, 2, 32770]", "SeqTable rows=last | [0, 1]",
                "SeqTable rows=None | [0, 2147483647]", "ShotTables min_scene_len=1 | [0, 16777216]",
                "FusionTables | n = 6400", "FusionTables | empty list"):
        assert "ok" in want[key], key


def test_ops_exports_the_plans_of_ragged():
    from avsum_amd import ops, ragged
    for name in ("FusionTables", "EvalTables", "SeqTable", "ShotTables", "FUSION_MAX_N", "FUSION_SMALL_L", "FUSION_MID_L",
                 "EVAL_MAX_T", "EVAL_TILE", "EVAL_CHUNK", "SHOT_INTERVAL", "SHOT_MAX_FRAMES", "SHOT_MICRO_BATCH"):
        assert getattr(ops, name) is getattr(ragged, name), name
    for cls in (ragged.EvalTables, ragged.SeqTable, ragged.ShotTables):
        assert issubclass(cls, ragged.RaggedOffsets)
    plan = ragged.ShotTables([0, 40, 47], 15, "cpu")
    assert plan.packed_sizes == (4, 3 * 3, 2 * plan.shot_cap, plan.shot_cap + 1, plan.group_cap + 1)
    assert (plan.count, plan.total, plan.max_len) == (plan.nvideos, plan.frames, 40) == (2, 47, 40)


def test_importing_ragged_does_not_load_the_library():
    code = ("import sys, avsum_amd.ragged\n"
            "assert 'avsum_amd.ops' not in sys.modules\n"
            "abi = sys.modules.get('avsum_amd._abi')\n"
            "assert abi is None or abi._lib is None\n"
            "import avsum_amd._abi as abi\n"
            "assert abi._lib is None\n")
    subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), check=True, timeout=120)


def test_exclusive_offsets_and_segment_tiles():
    from avsum_amd.ragged import exclusive_offsets, segment_tiles
    empty = exclusive_offsets([])
    assert empty.dtype == np.int64 and empty.tolist() == [0]
    off = exclusive_offsets([3, 0, 2])
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 3, 5]
    assert exclusive_offsets(np.array([4], dtype=np.int32)).tolist() == [0, 4]
    seg, k = segment_tiles([])
    assert seg.dtype == k.dtype == np.int64 and seg.shape == k.shape == (0,)
    seg, k = segment_tiles([2, 0, 3, 0])
    assert seg.dtype == k.dtype == np.int64
    assert seg.tolist() == [0, 0, 2, 2, 2] and k.tolist() == [0, 1, 0, 1, 2]
    seg, k = segment_tiles([0, 0])
    assert seg.size == 0 and k.size == 0

