"""The launcher's host-side selection, pinned through the three host-only convolution queries (no GPU: they read a
descriptor and launch nothing).  tests/golden/igemm_plan_host.json holds what the library answered BEFORE igemm_launch
was split into igemm_plan + igemm_run, over the ResNet-50 trunk's and Inception-v3's convolution geometries x dtype x
tile / staging variant x input format, and over a list of refusals; every value, error codes included, must still be
the same (tests/golden/make_igemm_plan_golden.py records the file and defines the replay)."""
import importlib.util
import json
import os

from avsum_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_igemm_plan_golden", os.path.join(GOLDEN, "make_igemm_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_queries_answer_as_recorded():
    rec = _recorder()
    with open(os.path.join(GOLDEN, "igemm_plan_host.json")) as f:
        corpus = json.load(f)
    answers, refusal_answers = rec.replay(rec.bind(_abi.LIB_PATH), corpus)
    per_shape = len(corpus["group_frames"]) * len(corpus["dtypes"]) * len(corpus["variants"]) * len(corpus["formats"])
    assert len(answers) == len(corpus["answers"]) == len(corpus["shapes"]) * per_shape
    wrong = [(corpus["shapes"][i // per_shape], i % per_shape, got, want)
             for i, (got, want) in enumerate(zip(answers, corpus["answers"])) if got != want]
    assert not wrong, f"{len(wrong)} of {len(answers)} answers differ, first: {wrong[:5]}"
    wrong = [(case[0], case[1][0], got, want)
             for case, got, want in zip(corpus["refusals"], refusal_answers, corpus["refusal_answers"]) if got != want]
    assert not wrong, wrong
    # the corpus is worth replaying only while it reaches every kind of answer: sizes, tile rows and each refusal status
    flat = [v for a in corpus["answers"] + corpus["refusal_answers"] for v in a]
    assert {-1, -2, -3, -6} <= set(flat) and any(v > 0 for v in flat)
