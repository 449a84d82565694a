#!/usr/bin/env python3
"""Records igemm_plan_host.json: what the three host-only convolution queries of libavsum_hip.so
(avs_conv2d_bnstats_workspace_bytes, avs_conv2d_bnlocal_tile_rows, avs_conv2d_bncluster_workspace_bytes) answer over a
corpus of shapes and options - error codes included.  tests/test_igemm_plan_host.py replays the file against the
library under test, so record it from the library whose selection is to be kept (a build of the commit BEFORE a change
to the launcher's rules), never from the tree being changed:

    python tests/golden/make_igemm_plan_golden.py path/to/libavsum_hip.so

No GPU is needed: the queries read a descriptor and launch nothing."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from avsum_amd import _abi  # noqa: E402

# (h, w, cin, kh, kw, stride, pad, cout): the ResNet-50 trunk (stride on the 3x3, as torchvision builds it)
RESNET50 = [(224, 224, 3, 7, 7, 2, 3, 64)]
for _hw, _cin, _mid, _stride in ((56, 64, 64, 1), (56, 256, 128, 2), (28, 512, 256, 2), (14, 1024, 512, 2)):
    _out = _hw // _stride
    RESNET50 += [
        (_hw, _hw, _cin, 1, 1, 1, 0, _mid),                # block 0: conv1
        (_hw, _hw, _mid, 3, 3, _stride, 1, _mid),          #          conv2 (carries the stage's stride)
        (_out, _out, _mid, 1, 1, 1, 0, 4 * _mid),          #          conv3
        (_hw, _hw, _cin, 1, 1, _stride, 0, 4 * _mid),      #          downsample
        (_out, _out, 4 * _mid, 1, 1, 1, 0, _mid),          # later blocks: conv1
        (_out, _out, _mid, 3, 3, 1, 1, _mid),              #               conv2
    ]
# Inception-v3's factorised and 3x3 filters on its 17 x 17 and 35 x 35 grids, the output widths that leave a 128-wide
# column tile partly empty
INCEPTION = [(hw, hw, cin, kh, kw, 1, (kh // 2, kw // 2), cout)
             for hw in (17, 35) for (kh, kw) in ((1, 7), (7, 1), (3, 3))
             for (cin, cout) in ((96, 96), (128, 160), (160, 192), (192, 288))]
DTYPES = [_abi.AVS_F32, _abi.AVS_BF16, _abi.AVS_F32_SPLIT, _abi.AVS_F16X2]
VARIANTS = [t | g for t in (_abi.TILE_AUTO, _abi.TILE_128, _abi.TILE_256, _abi.TILE_224) for g in (0, _abi.STAGING_GENERIC)]
FORMATS = [0, _abi.X_F16P8]
GROUP_FRAMES = [1, 4]
N = 4


def desc_fields(n, shape, dtype, variant, formats):
    """The 24 fields of avs_conv_desc for a dense NHWC input and output, in _abi.ConvDesc's order."""
    h, w, cin, kh, kw, s, pad, cout = shape
    ph, pw = pad if isinstance(pad, tuple) else (pad, pad)
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    return [dtype, n, h, w, cin, kh, kw, s, s, ph, pw, ho, wo, cout, h * w * cin, w * cin, cin, kh * kw * cin, cout,
            _abi.ACT_NONE, 1.0, _abi.AVS_W_ROWS, variant, formats]


def refusals():
    """[label, descriptor fields, rows_per_group, cluster]: one thing wrong at a time, on a shape every form takes."""
    base = (14, 14, 256, 3, 3, 1, 1, 256)
    out = []
    for dtype in DTYPES:
        good = desc_fields(N, base, dtype, 0, 0)
        out.append(["n = 0", desc_fields(0, base, dtype, 0, 0), 4 * 196, 4])
        out.append(["rows_per_group = 63", good, 63, 3])
        out.append(["cin = 12", desc_fields(N, (14, 14, 12, 3, 3, 1, 1, 256), dtype, 0, 0), 4 * 196, 4])
        out.append(["cluster = 1", good, 196, 1])
        out.append(["cluster = 17", good, 17 * 196, 17])
        neg = list(good)
        neg[7] = -1
        out.append(["sh = -1", neg, 4 * 196, 4])
        neg = list(good)
        neg[15] = -neg[15]
        out.append(["x_row_stride < 0", neg, 4 * 196, 4])
        odd = list(good)
        odd[16] += 1
        out.append(["x_px_stride = cin + 1", odd, 4 * 196, 4])
    return out


def ask(lib, fields, rpg, cluster):
    d = _abi.ConvDesc(*fields)
    return [int(lib.avs_conv2d_bnstats_workspace_bytes(ctypes.byref(d), rpg)),
            int(lib.avs_conv2d_bnlocal_tile_rows(ctypes.byref(d), rpg)),
            int(lib.avs_conv2d_bncluster_workspace_bytes(ctypes.byref(d), rpg, cluster))]


def replay(lib, corpus):
    """The answers of `lib` over the corpus, in the layout of the recording's "answers" / "refusal_answers"."""
    answers = []
    for shape in corpus["shapes"]:
        shape = [tuple(v) if isinstance(v, list) else v for v in shape]
        for gf in corpus["group_frames"]:
            for dtype in corpus["dtypes"]:
                for variant in corpus["variants"]:
                    for formats in corpus["formats"]:
                        f = desc_fields(corpus["n"], shape, dtype, variant, formats)
                        answers.append(ask(lib, f, gf * f[11] * f[12], max(gf, 2)))
    return answers, [ask(lib, f, rpg, cl) for _, f, rpg, cl in corpus["refusals"]]


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("avs_conv2d_bnstats_workspace_bytes", "avs_conv2d_bnlocal_tile_rows", "avs_conv2d_bncluster_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _abi._SIGNATURES[name]
    return lib


def main():
    lib = bind(os.path.abspath(sys.argv[1]))
    corpus = {"n": N, "shapes": [list(s) for s in RESNET50 + INCEPTION], "group_frames": GROUP_FRAMES, "dtypes": DTYPES,
              "variants": VARIANTS, "formats": FORMATS, "refusals": refusals()}
    corpus = json.loads(json.dumps(corpus))
    corpus["answers"], corpus["refusal_answers"] = replay(lib, corpus)
    with open(os.path.join(HERE, "igemm_plan_host.json"), "w") as f:
        json.dump(corpus, f, separators=(",", ":"))
        f.write("\n")
    vals = corpus["answers"] + corpus["refusal_answers"]
    print(len(vals), "cases,", sum(1 for v in vals for x in v if x < 0), "negative answers of", 3 * len(vals))


if __name__ == "__main__":
    main()
