"""ResNet50Runner.plan(): the trunk's steps pinned as tables (no GPU: the plan reads shapes, the trunk's structure, the
switches and the library's host-only queries, and packs no weights), and the two-stream pipeline's scope of its
unclustered choice.  The tables are the launch sequences the runner recorded before the plan existed, read as steps.

Columns: step, form, input (- finished | raw), output (- finished | def deferred | p8), residual (- none | id identity |
ds finished downsample | def deferred downsample)."""
import pytest
import torch

F16X2_GF4 = """
conv1                     stem_f16x2 -   def -
layer1.0.conv1+downsample gram_pair  raw -   -
layer1.0.conv2            stats      -   def -
layer1.0.conv3            gram       raw p8  ds
layer1.1.conv1            stats      -   def -
layer1.1.conv2            stats      raw def -
layer1.1.conv3            gram       raw p8  id
layer1.2.conv1            stats      -   def -
layer1.2.conv2            stats      raw def -
layer1.2.conv3            gram       raw -   id
layer2.0.conv1            stats      -   -   -
layer2.0.conv2            stats      -   def -
layer2.0.downsample       stats      -   def -
layer2.0.conv3            gram       raw p8  def
layer2.1.conv1            stats      -   def -
layer2.1.conv2            stats      raw def -
layer2.1.conv3            gram       raw p8  id
layer2.2.conv1            stats      -   def -
layer2.2.conv2            stats      raw def -
layer2.2.conv3            gram       raw p8  id
layer2.3.conv1            stats      -   def -
layer2.3.conv2            stats      raw def -
layer2.3.conv3            gram       raw -   id
layer3.0.conv1            cluster    -   -   -
layer3.0.conv2            cluster    -   -   -
layer3.0.downsample       cluster    -   -   -
layer3.0.conv3            cluster    -   -   ds
layer3.1.conv1            cluster    -   -   -
layer3.1.conv2            cluster    -   -   -
layer3.1.conv3            cluster    -   -   id
layer3.2.conv1            cluster    -   -   -
layer3.2.conv2            cluster    -   -   -
layer3.2.conv3            cluster    -   -   id
layer3.3.conv1            cluster    -   -   -
layer3.3.conv2            cluster    -   -   -
layer3.3.conv3            cluster    -   -   id
layer3.4.conv1            cluster    -   -   -
layer3.4.conv2            cluster    -   -   -
layer3.4.conv3            cluster    -   -   id
layer3.5.conv1            cluster    -   -   -
layer3.5.conv2            cluster    -   -   -
layer3.5.conv3            cluster    -   -   id
layer4.0.conv1            cluster    -   -   -
layer4.0.conv2            local      -   -   -
layer4.0.downsample       local      -   -   -
layer4.0.conv3            local      -   -   ds
layer4.1.conv1            local      -   -   -
layer4.1.conv2            local      -   -   -
layer4.1.conv3            local      -   -   id
layer4.2.conv1            local      -   -   -
layer4.2.conv2            local      -   -   -
layer4.2.conv3            local      -   -   id
"""

F16X2_GF1 = """
conv1                     stem_f16x2 -   def -
layer1.0.conv1+downsample gram_pair  raw -   -
layer1.0.conv2            stats      -   def -
layer1.0.conv3            gram       raw p8  ds
layer1.1.conv1            stats      -   def -
layer1.1.conv2            stats      raw def -
layer1.1.conv3            gram       raw p8  id
layer1.2.conv1            stats      -   def -
layer1.2.conv2            stats      raw def -
layer1.2.conv3            gram       raw -   id
layer2.0.conv1            stats      -   -   -
layer2.0.conv2            stats      -   def -
layer2.0.downsample       stats      -   def -
layer2.0.conv3            gram       raw p8  def
layer2.1.conv1            stats      -   def -
layer2.1.conv2            stats      raw def -
layer2.1.conv3            gram       raw p8  id
layer2.2.conv1            stats      -   def -
layer2.2.conv2            stats      raw def -
layer2.2.conv3            gram       raw p8  id
layer2.3.conv1            stats      -   def -
layer2.3.conv2            stats      raw def -
layer2.3.conv3            gram       raw -   id
layer3.0.conv1            cluster    -   -   -
layer3.0.conv2            local      -   -   -
layer3.0.downsample       local      -   -   -
layer3.0.conv3            local      -   -   ds
layer3.1.conv1            local      -   -   -
layer3.1.conv2            local      -   -   -
layer3.1.conv3            local      -   -   id
layer3.2.conv1            local      -   -   -
layer3.2.conv2            local      -   -   -
layer3.2.conv3            local      -   -   id
layer3.3.conv1            local      -   -   -
layer3.3.conv2            local      -   -   -
layer3.3.conv3            local      -   -   id
layer3.4.conv1            local      -   -   -
layer3.4.conv2            local      -   -   -
layer3.4.conv3            local      -   -   id
layer3.5.conv1            local      -   -   -
layer3.5.conv2            local      -   -   -
layer3.5.conv3            local      -   -   id
layer4.0.conv1            local      -   -   -
layer4.0.conv2            local      -   -   -
layer4.0.downsample       local      -   -   -
layer4.0.conv3            local      -   -   ds
layer4.1.conv1            local      -   -   -
layer4.1.conv2            local      -   -   -
layer4.1.conv3            local      -   -   id
layer4.2.conv1            local      -   -   -
layer4.2.conv2            local      -   -   -
layer4.2.conv3            local      -   -   id
"""

SPLIT = """
conv1               split      -   -   -
layer1.0.conv1      split      -   -   -
layer1.0.conv2      split      -   -   -
layer1.0.downsample split      -   -   -
layer1.0.conv3      split      -   -   ds
layer1.1.conv1      split      -   -   -
layer1.1.conv2      split      -   -   -
layer1.1.conv3      split      -   -   id
layer1.2.conv1      split      -   -   -
layer1.2.conv2      split      -   -   -
layer1.2.conv3      split      -   -   id
layer2.0.conv1      split      -   -   -
layer2.0.conv2      split      -   -   -
layer2.0.downsample split      -   -   -
layer2.0.conv3      split      -   -   ds
layer2.1.conv1      split      -   -   -
layer2.1.conv2      split      -   -   -
layer2.1.conv3      split      -   -   id
layer2.2.conv1      split      -   -   -
layer2.2.conv2      split      -   -   -
layer2.2.conv3      split      -   -   id
layer2.3.conv1      split      -   -   -
layer2.3.conv2      split      -   -   -
layer2.3.conv3      split      -   -   id
layer3.0.conv1      split      -   -   -
layer3.0.conv2      split      -   -   -
layer3.0.downsample split      -   -   -
layer3.0.conv3      split      -   -   ds
layer3.1.conv1      split      -   -   -
layer3.1.conv2      split      -   -   -
layer3.1.conv3      split      -   -   id
layer3.2.conv1      split      -   -   -
layer3.2.conv2      split      -   -   -
layer3.2.conv3      split      -   -   id
layer3.3.conv1      split      -   -   -
layer3.3.conv2      split      -   -   -
layer3.3.conv3      split      -   -   id
layer3.4.conv1      split      -   -   -
layer3.4.conv2      split      -   -   -
layer3.4.conv3      split      -   -   id
layer3.5.conv1      split      -   -   -
layer3.5.conv2      split      -   -   -
layer3.5.conv3      split      -   -   id
layer4.0.conv1      split      -   -   -
layer4.0.conv2      split      -   -   -
layer4.0.downsample split      -   -   -
layer4.0.conv3      split      -   -   ds
layer4.1.conv1      split      -   -   -
layer4.1.conv2      split      -   -   -
layer4.1.conv3      split      -   -   id
layer4.2.conv1      split      -   -   -
layer4.2.conv2      split      -   -   -
layer4.2.conv3      split      -   -   id
"""

BF16_GF1 = """
conv1                     stem_bf16  -   def -
layer1.0.conv1+downsample gram_pair  raw -   -
layer1.0.conv2            stats      -   def -
layer1.0.conv3            gram       raw -   ds
layer1.1.conv1            stats      -   -   -
layer1.1.conv2            stats      -   def -
layer1.1.conv3            gram       raw -   id
layer1.2.conv1            stats      -   -   -
layer1.2.conv2            stats      -   def -
layer1.2.conv3            gram       raw -   id
layer2.0.conv1            stats      -   -   -
layer2.0.conv2            stats      -   def -
layer2.0.downsample       stats      -   def -
layer2.0.conv3            gram       raw -   def
layer2.1.conv1            stats      -   -   -
layer2.1.conv2            stats      -   def -
layer2.1.conv3            gram       raw -   id
layer2.2.conv1            stats      -   -   -
layer2.2.conv2            stats      -   def -
layer2.2.conv3            gram       raw -   id
layer2.3.conv1            stats      -   -   -
layer2.3.conv2            stats      -   def -
layer2.3.conv3            gram       raw -   id
layer3.0.conv1            stats      -   -   -
layer3.0.conv2            local      -   -   -
layer3.0.downsample       local      -   -   -
layer3.0.conv3            local      -   -   ds
layer3.1.conv1            local      -   -   -
layer3.1.conv2            local      -   -   -
layer3.1.conv3            local      -   -   id
layer3.2.conv1            local      -   -   -
layer3.2.conv2            local      -   -   -
layer3.2.conv3            local      -   -   id
layer3.3.conv1            local      -   -   -
layer3.3.conv2            local      -   -   -
layer3.3.conv3            local      -   -   id
layer3.4.conv1            local      -   -   -
layer3.4.conv2            local      -   -   -
layer3.4.conv3            local      -   -   id
layer3.5.conv1            local      -   -   -
layer3.5.conv2            local      -   -   -
layer3.5.conv3            local      -   -   id
layer4.0.conv1            local      -   -   -
layer4.0.conv2            local      -   -   -
layer4.0.downsample       local      -   -   -
layer4.0.conv3            local      -   -   ds
layer4.1.conv1            local      -   -   -
layer4.1.conv2            local      -   -   -
layer4.1.conv3            local      -   -   id
layer4.2.conv1            local      -   -   -
layer4.2.conv2            local      -   -   -
layer4.2.conv3            local      -   -   id
"""

BF16_GF4 = """
conv1                     stem_bf16  -   def -
layer1.0.conv1+downsample gram_pair  raw -   -
layer1.0.conv2            stats      -   def -
layer1.0.conv3            gram       raw -   ds
layer1.1.conv1            stats      -   -   -
layer1.1.conv2            stats      -   def -
layer1.1.conv3            gram       raw -   id
layer1.2.conv1            stats      -   -   -
layer1.2.conv2            stats      -   def -
layer1.2.conv3            gram       raw -   id
layer2.0.conv1            stats      -   -   -
layer2.0.conv2            stats      -   def -
layer2.0.downsample       stats      -   def -
layer2.0.conv3            gram       raw -   def
layer2.1.conv1            stats      -   -   -
layer2.1.conv2            stats      -   def -
layer2.1.conv3            gram       raw -   id
layer2.2.conv1            stats      -   -   -
layer2.2.conv2            stats      -   def -
layer2.2.conv3            gram       raw -   id
layer2.3.conv1            stats      -   -   -
layer2.3.conv2            stats      -   def -
layer2.3.conv3            gram       raw -   id
layer3.0.conv1            stats      -   -   -
layer3.0.conv2            stats      -   -   -
layer3.0.downsample       stats      -   -   -
layer3.0.conv3            stats      -   -   ds
layer3.1.conv1            stats      -   -   -
layer3.1.conv2            stats      -   -   -
layer3.1.conv3            stats      -   -   id
layer3.2.conv1            stats      -   -   -
layer3.2.conv2            stats      -   -   -
layer3.2.conv3            stats      -   -   id
layer3.3.conv1            stats      -   -   -
layer3.3.conv2            stats      -   -   -
layer3.3.conv3            stats      -   -   id
layer3.4.conv1            stats      -   -   -
layer3.4.conv2            stats      -   -   -
layer3.4.conv3            stats      -   -   id
layer3.5.conv1            stats      -   -   -
layer3.5.conv2            stats      -   -   -
layer3.5.conv3            stats      -   -   id
layer4.0.conv1            stats      -   -   -
layer4.0.conv2            local      -   -   -
layer4.0.downsample       local      -   -   -
layer4.0.conv3            local      -   -   ds
layer4.1.conv1            local      -   -   -
layer4.1.conv2            local      -   -   -
layer4.1.conv3            local      -   -   id
layer4.2.conv1            local      -   -   -
layer4.2.conv2            local      -   -   -
layer4.2.conv3            local      -   -   id
"""

FP32_SPLIT = """
conv1               stats      -   -   -
layer1.0.conv1      stats      -   -   -
layer1.0.conv2      stats      -   -   -
layer1.0.downsample stats      -   -   -
layer1.0.conv3      stats      -   -   ds
layer1.1.conv1      stats      -   -   -
layer1.1.conv2      stats      -   -   -
layer1.1.conv3      stats      -   -   id
layer1.2.conv1      stats      -   -   -
layer1.2.conv2      stats      -   -   -
layer1.2.conv3      stats      -   -   id
layer2.0.conv1      stats      -   -   -
layer2.0.conv2      stats      -   -   -
layer2.0.downsample stats      -   -   -
layer2.0.conv3      stats      -   -   ds
layer2.1.conv1      stats      -   -   -
layer2.1.conv2      stats      -   -   -
layer2.1.conv3      stats      -   -   id
layer2.2.conv1      stats      -   -   -
layer2.2.conv2      stats      -   -   -
layer2.2.conv3      stats      -   -   id
layer2.3.conv1      stats      -   -   -
layer2.3.conv2      stats      -   -   -
layer2.3.conv3      stats      -   -   id
layer3.0.conv1      stats      -   -   -
layer3.0.conv2      stats      -   -   -
layer3.0.downsample stats      -   -   -
layer3.0.conv3      stats      -   -   ds
layer3.1.conv1      stats      -   -   -
layer3.1.conv2      stats      -   -   -
layer3.1.conv3      stats      -   -   id
layer3.2.conv1      stats      -   -   -
layer3.2.conv2      stats      -   -   -
layer3.2.conv3      stats      -   -   id
layer3.3.conv1      stats      -   -   -
layer3.3.conv2      stats      -   -   -
layer3.3.conv3      stats      -   -   id
layer3.4.conv1      stats      -   -   -
layer3.4.conv2      stats      -   -   -
layer3.4.conv3      stats      -   -   id
layer3.5.conv1      stats      -   -   -
layer3.5.conv2      stats      -   -   -
layer3.5.conv3      stats      -   -   id
layer4.0.conv1      stats      -   -   -
layer4.0.conv2      stats      -   -   -
layer4.0.downsample stats      -   -   -
layer4.0.conv3      stats      -   -   ds
layer4.1.conv1      stats      -   -   -
layer4.1.conv2      stats      -   -   -
layer4.1.conv3      stats      -   -   id
layer4.2.conv1      stats      -   -   -
layer4.2.conv2      stats      -   -   -
layer4.2.conv3      stats      -   -   id
"""

FOLDED = """
conv1               folded     -   -   -
layer1.0.conv1      folded     -   -   -
layer1.0.conv2      folded     -   -   -
layer1.0.downsample folded     -   -   -
layer1.0.conv3      folded     -   -   ds
layer1.1.conv1      folded     -   -   -
layer1.1.conv2      folded     -   -   -
layer1.1.conv3      folded     -   -   id
layer1.2.conv1      folded     -   -   -
layer1.2.conv2      folded     -   -   -
layer1.2.conv3      folded     -   -   id
layer2.0.conv1      folded     -   -   -
layer2.0.conv2      folded     -   -   -
layer2.0.downsample folded     -   -   -
layer2.0.conv3      folded     -   -   ds
layer2.1.conv1      folded     -   -   -
layer2.1.conv2      folded     -   -   -
layer2.1.conv3      folded     -   -   id
layer2.2.conv1      folded     -   -   -
layer2.2.conv2      folded     -   -   -
layer2.2.conv3      folded     -   -   id
layer2.3.conv1      folded     -   -   -
layer2.3.conv2      folded     -   -   -
layer2.3.conv3      folded     -   -   id
layer3.0.conv1      folded     -   -   -
layer3.0.conv2      folded     -   -   -
layer3.0.downsample folded     -   -   -
layer3.0.conv3      folded     -   -   ds
layer3.1.conv1      folded     -   -   -
layer3.1.conv2      folded     -   -   -
layer3.1.conv3      folded     -   -   id
layer3.2.conv1      folded     -   -   -
layer3.2.conv2      folded     -   -   -
layer3.2.conv3      folded     -   -   id
layer3.3.conv1      folded     -   -   -
layer3.3.conv2      folded     -   -   -
layer3.3.conv3      folded     -   -   id
layer3.4.conv1      folded     -   -   -
layer3.4.conv2      folded     -   -   -
layer3.4.conv3      folded     -   -   id
layer3.5.conv1      folded     -   -   -
layer3.5.conv2      folded     -   -   -
layer3.5.conv3      folded     -   -   id
layer4.0.conv1      folded     -   -   -
layer4.0.conv2      folded     -   -   -
layer4.0.downsample folded     -   -   -
layer4.0.conv3      folded     -   -   ds
layer4.1.conv1      folded     -   -   -
layer4.1.conv2      folded     -   -   -
layer4.1.conv3      folded     -   -   id
layer4.2.conv1      folded     -   -   -
layer4.2.conv2      folded     -   -   -
layer4.2.conv3      folded     -   -   id
"""

ABBR = {"-": None, "raw": "raw", "def": "deferred", "p8": "p8", "id": "identity", "ds": "downsample"}


def _rows(table):
    out = []
    for line in table.strip().splitlines():
        name, form, inp, outp, res = line.split()
        out.append((name, form, "raw" if inp == "raw" else "finished", ABBR[outp] or "finished",
                    {"-": "none", "def": "deferred"}.get(res, ABBR[res])))
    return out


def _runner(mode):
    from avsum_amd.cnn import ResNet50Runner, resnet50_trunk
    torch.manual_seed(0)
    trunk = resnet50_trunk()
    return {"f16x2": lambda: ResNet50Runner(trunk, torch.float32, f32_split="f16x2"),
            "bf16": lambda: ResNet50Runner(trunk, torch.bfloat16),
            "fp32": lambda: ResNet50Runner(trunk, torch.float32),
            "fp32-split": lambda: ResNet50Runner(trunk, torch.float32, f32_split=True),
            "folded": lambda: ResNet50Runner(trunk, torch.float32, bn_mode="folded")}[mode]()


def _pass_15048():
    # the headline run's pass size: its 45 143 frames in 4-frame groups through bench.py's f16x2 chunk of 16 384 frames
    from avsum_amd.pipeline import FrameScoringPipeline
    n = FrameScoringPipeline._pass_frames(45143, 16384, 4)
    assert n == 15048
    return n


CASES = [
    ("f16x2", 16, list(range(0, 17, 4)), F16X2_GF4),
    ("f16x2", 168, list(range(0, 169, 4)), F16X2_GF4),
    ("f16x2", None, 4, F16X2_GF4),
    ("f16x2", 16, None, F16X2_GF1),
    ("f16x2", 8, [0, 4, 7, 8], SPLIT),
    ("bf16", 16, None, BF16_GF1),
    ("bf16", 16, list(range(0, 17, 4)), BF16_GF4),
    ("fp32", 8, [0, 4, 8], SPLIT),
    ("fp32-split", 8, [0, 4, 8], FP32_SPLIT),
    ("folded", 8, [0, 4, 8], FOLDED),
]


@pytest.mark.parametrize("mode,n,groups,table", CASES,
                         ids=["f16x2-gf4-16", "f16x2-gf4-168", "f16x2-gf4-headline", "f16x2-gf1", "f16x2-ragged", "bf16-gf1",
                              "bf16-gf4", "fp32", "fp32-split", "folded"])
def test_plan_pins_the_launch_sequence(mode, n, groups, table):
    if n is None:
        n = _pass_15048()
        groups = list(range(0, n + 1, groups))
    r = _runner(mode)
    got = [(s.name, s.form, s.inp, s.out, s.res) for s in r.plan(n, groups)]
    assert got == _rows(table)
    assert r._w is None     # no weights were packed


def test_plan_follows_the_switches():
    """A switch flipped between two calls takes effect (the plan cache key holds every switch the plan reads)."""
    r = _runner("f16x2")
    gf = list(range(0, 17, 4))
    forms = lambda: [s.form for s in r.plan(16, gf)]
    assert forms().count("cluster") == 20
    r.bn_cluster = False
    assert "cluster" not in forms()
    r.bn_cluster = True
    assert "cluster" not in [s.form for s in r.plan(16, gf, bn_cluster=False)]     # the per-call choice
    r.p8_blocks = ()
    assert all(s.out != "p8" for s in r.plan(16, gf))
    r.fold_input_bn = False
    assert all(not (s.name.endswith("conv2") and s.inp == "raw") for s in r.plan(16, gf))


def test_two_stream_pipeline_leaves_the_runner_alone():
    """FrameScoringPipeline(streams=2) keeps its unclustered choice to its overlapped passes: the shared runner's switch
    stays as it was."""
    from avsum_amd.pipeline import FrameScoringPipeline

    class Extractor:
        _resnet_runner = _runner("f16x2")

    ext = Extractor()
    FrameScoringPipeline(ext, None, use_inception=False, frames_per_group=4, streams=2)
    assert ext._resnet_runner.bn_cluster is True
