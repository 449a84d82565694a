"""The launcher's host-side selection, pinned through the three host-only convolution queries (no GPU: they read a
descriptor and launch nothing).  tests/golden/igemm_plan_host.json holds what the library answered BEFORE igemm_launch
was split into igemm_plan + igemm_run, over the ResNet-50 trunk's and Inception-v3's convolution geometries x dtype x
tile / staging variant x input format, and over a list of refusals; every value, error codes included, must still be
the same (tests/golden/make_igemm_plan_golden.py records the file and defines the replay)."""
import importlib.util
import json
import os
import re

from avsum_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "audiovidsum-a-multi-modal-approach-to-video-summarization_amd", "csrc")
# igemm_kernel's head: mangled names, profiles/, tools/resource_usage.py and the dispatch in igemm_lift_* depend on it
IGEMM_KERNEL_HEAD = (
    "template <int ES, int BN, bool ACC64, bool SPATIAL, int ROWB, int EPI, bool PIPE, int WR = 2, bool FASTK = false,\n"
    "          int SPLIT = 0, bool TAP9 = false, bool AP8 = false, bool XIN = false, bool GROUPW = false>\n"
    "__global__ __launch_bounds__(256, (ROWB == 64 && !ACC64 && WR == 2) ? ((BN == 64 && ES == 2) ? 4 : 3) : 2) void igemm_kernel(\n"
    "    IgemmParams p) {\n")


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


def test_the_contraction_kernels_share_one_text_of_their_staging_pieces():
    """The XCD block remap, the LDS slot map and the advance of the scalar tap walk stand once, in igemm_params.h; igemm.hip,
    local224.hip and (remap, slot map) convbn.hip use them and hold no copy of their own, recognised by each piece's
    distinguishing expression.  igemm_kernel's template head is the one every profile and tool knows."""
    sources = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC))
               if name.endswith((".hip", ".h"))}
    once = {"block remap": r"nwg >> 3", "slot map": r">> SH\) & \(CPRR - 1\)",
            "tap-walk advance": r"x_row_stride - \(long long\)p\.KW \* p\.x_px_stride"}
    for what, pattern in once.items():
        found = {name: len(re.findall(pattern, text)) for name, text in sources.items()}
        assert {name: n for name, n in found.items() if n} == {"igemm_params.h": 1}, (what, found)
    header = sources["igemm_params.h"]
    definitions = (r"^__device__ __forceinline__ unsigned avs_xcd_remap\(", r"^#define AVS_LDS_CHUNK\(", r"^#define AVS_LDS_SLOT\(",
                   r"^__device__ __forceinline__ void avs_tap_advance\(")
    assert all(len(re.findall(d, header, flags=re.M)) == 1 for d in definitions)
    for name in ("igemm.hip", "local224.hip", "convbn.hip"):
        text = sources[name]
        assert '#include "igemm_params.h"' in text and "#define AVS_GLDS16" not in text, name
        assert len(re.findall(r"= avs_xcd_remap\(", text)) == 1 and "AVS_LDS_CHUNK(" in text and "AVS_LDS_SLOT(" in text, name
        # (local224.hip spelled the map with its own constants)
        assert not re.search(r">> 2\) & \(L_CPRR - 1\)|xcd \* \(q \+ 1\)", text), name
    for name in ("igemm.hip", "local224.hip"):
        assert len(re.findall(r"\bavs_tap_advance<", sources[name])) == 1 and not re.search(r"\+\+f_kw\b", sources[name]), name
    assert sources["igemm.hip"].count(IGEMM_KERNEL_HEAD) == 1 and len(re.findall(r"\bvoid igemm_kernel\(", sources["igemm.hip"])) == 1
