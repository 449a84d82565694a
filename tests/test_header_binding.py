"""The binding is derived from include/avsum_hip.h (host only): the reader on small header texts, pinned signatures and
the descriptor on the real header, the bound library, and the sizes the host tables share with the kernels - each
defined once, in the header."""
import ctypes
import glob
import os
import re
import subprocess
import sys
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint, c_void_p

import pytest

from avsum_amd import _abi, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = c_void_p


# ---- the reader, on synthetic header text ------------------------------------------------------------------------------
def test_reader_prototypes():
    h = _header.Header("""
        typedef void* stream_t;
        /* a comment with a call(in, it); */
        int f(const float* d_x, int64_t n, void* d_y, unsigned mask,
              const int64_t* d_off, double t, size_t bytes, uint32_t epoch, float alpha, stream_t stream);
        const char* msg(void);   // trailing comment; with(a call)
        size_t bytes_of(int a, int b);
    """)
    assert h.prototypes == {
        "f": ("int", ["float*", "int64_t", "void*", "unsigned", "int64_t*", "double", "size_t", "uint32_t", "float",
                      "stream_t"]),
        "msg": ("char*", []),
        "bytes_of": ("size_t", ["int", "int"])}
    assert h.signatures() == {
        "f": (c_int, [P, c_int64, P, c_uint, P, c_double, c_size_t, c_uint, c_float, P]),
        "msg": (c_char_p, []),
        "bytes_of": (c_size_t, [c_int, c_int])}


def test_reader_enums_and_defines():
    h = _header.Header("""
        #ifndef GUARD_H
        #define GUARD_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VERSION 5
        #define WIDE 0x40     /* hexadecimal */
        #define RATIO 0.5
        #define NAME "text"
        #define TWICE(x) (2 * (x))
        #define SUM (VERSION + 1)
        enum {
          OK = 0,
          E_ARG = -1,       /* null pointer, bad enum   */
          E_SHAPE = -2,     // sizes
          E_LAST = -6 /* no comma */
        };
        enum { A, B, C = 7, D };
        int after(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert h.constants == {"VERSION": 5, "WIDE": 64, "OK": 0, "E_ARG": -1, "E_SHAPE": -2, "E_LAST": -6,
                           "A": 0, "B": 1, "C": 7, "D": 8}
    assert h.prototypes == {"after": ("int", [])}


def test_reader_struct():
    h = _header.Header("""
        typedef struct {
          int dtype;            /* first */
          int n, h, w;          /* three on a line */
          int64_t stride;
          float alpha;
          const void* next;
        } desc_t;
        int take(const desc_t* d, int k);
    """)
    assert h.structs == {"desc_t": [("dtype", "int"), ("n", "int"), ("h", "int"), ("w", "int"), ("stride", "int64_t"),
                                    ("alpha", "float"), ("next", "void*")]}
    assert h.fields("desc_t") == [("dtype", c_int), ("n", c_int), ("h", c_int), ("w", c_int), ("stride", c_int64),
                                  ("alpha", c_float), ("next", P)]

    class Desc(ctypes.Structure):
        _fields_ = h.fields("desc_t")
    assert h.signatures({"desc_t": Desc})["take"] == (c_int, [POINTER(Desc), c_int])
    assert h.signatures()["take"] == (c_int, [P, c_int])


@pytest.mark.parametrize("text, named", [
    ("int f(long n);", "f()"),                                   # an unknown scalar
    ("int f(uint8_t flag);", "f()"),                             # a scalar the map does not hold
    ("int f(const thing_t* p);", "thing_t"),                     # a pointer to nothing known
    ("int f(float** rows);", "float**"),
    ("void f(int n);", "f()"),
    ("int f(int);", "f()"),                                      # a parameter without a name
    ("int f();", "f()"),
    ("int f(int a, );", "f()"),
    ("int f(int a", "int f(int a"),                              # never closed
    ("f(int a);", "f(int a)"),                                   # no return type
    ("int x;", "int x"),                                         # not a prototype at all
    ("int f(int (*callback)(int));", "f()"),
    ("typedef int handle_t;", "handle_t"),
    ("typedef struct { short s; } d_t;", "struct d_t"),          # a struct field of an unmapped type
    ("typedef struct { int a b; } d_t;", "struct d_t"),
    ("enum { A = 1 << 3 };", "A = 1 << 3"),                      # an enumerator that is no literal
    ("enum { A = 1 };\n#define A 2", "A"),                       # one name, two values
    ("int f(void);\nint f(void);", "f()"),
    ('extern "C" {\nint f(void);', "extern"),
])
def test_reader_refuses_what_it_does_not_know(text, named):
    with pytest.raises(_header.HeaderError) as err:
        _header.Header(text)
    assert named in str(err.value)


# ---- the real header -----------------------------------------------------------------------------------------------
CD = POINTER(_abi.ConvDesc)
PINNED = {
    "avs_abi_version": (c_int, []),
    "avs_last_error": (c_char_p, []),
    "avs_device_info": (c_int, [c_int, P, P, P, P, c_int]),
    "avs_gemm_nt": (c_int, [c_int, c_int, c_int, c_int, P, c_int64, c_int64, P, c_int64, c_int64, P, c_int64, c_int64, P,
                            c_int, c_int64, c_float, c_int, c_int, P]),
    "avs_conv2d_nhwc": (c_int, [CD, P, P, P, P, P]),
    "avs_conv2d_bnstats_workspace_bytes": (c_int64, [CD, c_int64]),
    "avs_conv2d_nhwc_bncluster": (c_int, [CD, P, P, P, c_int64, c_int, P, P, c_float, P, c_int64, P, c_int64, c_uint, P]),
    "avs_lstm_f32": (c_int, [P, P, c_int, c_int, c_uint, P, c_int, P, c_int64, c_int, c_int, P]),
    "avs_lstm_split_workspace_bytes": (c_size_t, [c_int, c_int]),
    "avs_lstm_split_f32": (c_int, [P, P, c_int, c_int, c_uint, P, c_int, P, c_int64, c_int, P, P, P, c_size_t, c_uint, P]),
    "avs_shot_cuts_batch": (c_int, [P, c_int64, P, c_int, c_double, c_double, c_int, P, P, P, P]),
    "avs_kts_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "avs_kts_dp_f64": (c_int, [P, c_int, c_int, c_int, c_int64, c_int, P, P, c_size_t, c_int64, c_int64, c_int64, c_int64,
                               c_int64, P, P, P, P, P, P, P, P]),
    "avs_stft_mel_shots_f32": (c_int, [P, c_int64, P, P, c_int, P, c_int, P, P, P, P, P, P, c_int, P, c_int, P, P, P,
                                       c_float, P, c_int64, P, c_int64, P, c_int64, P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    assert _abi._SIGNATURES[name] == PINNED[name]


def test_every_prototype_is_read():
    names = _abi.declared_symbols()
    assert len(names) == 96 == len(_abi._SIGNATURES) and names == sorted(_abi._SIGNATURES)
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER_PATH).read(), flags=re.S)
    assert names == sorted(set(re.findall(r"\b(avs_[a-z0-9_]+)\s*\(", text)))      # the earlier, name-only reading
    assert _header.load() is _header.load()                                       # read once per process


def test_conv_desc_layout():
    assert _abi.ConvDesc._fields_ == [
        ("dtype", c_int),
        ("n", c_int), ("h", c_int), ("w", c_int),
        ("cin", c_int), ("kh", c_int), ("kw", c_int),
        ("sh", c_int), ("sw", c_int), ("ph", c_int), ("pw", c_int),
        ("ho", c_int), ("wo", c_int), ("cout", c_int),
        ("x_img_stride", c_int64), ("x_row_stride", c_int64), ("x_px_stride", c_int64),
        ("w_row_stride", c_int64), ("y_px_stride", c_int64),
        ("act", c_int), ("alpha", c_float), ("w_layout", c_int), ("variant", c_int), ("formats", c_int),
    ]
    assert ctypes.sizeof(_abi.ConvDesc) == 120


def test_enum_values_are_the_headers():
    got = {n: getattr(_abi, n) for n in (
        "AVS_F32 AVS_BF16 AVS_F32_ACC64 AVS_F32_SPLIT AVS_F16X2 AVS_W_ROWS AVS_W_KSTEP32 TILE_AUTO TILE_128 TILE_256 "
        "TILE_224 STAGING_GENERIC CLUSTER_PACKED X_F16P8 Y_F16P8 RES_F16P8 LSTM_AUTO LSTM_STREAM LSTM_RESIDENT_20_8 "
        "LSTM_RESIDENT_16_8 LSTM_SPLIT4 ACT_NONE ACT_RELU BIAS_NONE BIAS_COL BIAS_ROW E_UNSUPPORTED ABI_VERSION").split()}
    assert got == {
        "AVS_F32": 0, "AVS_BF16": 1, "AVS_F32_ACC64": 2, "AVS_F32_SPLIT": 3, "AVS_F16X2": 4, "AVS_W_ROWS": 0,
        "AVS_W_KSTEP32": 1, "TILE_AUTO": 0, "TILE_128": 1, "TILE_256": 2, "TILE_224": 3, "STAGING_GENERIC": 4,
        "CLUSTER_PACKED": 8, "X_F16P8": 1, "Y_F16P8": 2, "RES_F16P8": 4, "LSTM_AUTO": 0, "LSTM_STREAM": 1,
        "LSTM_RESIDENT_20_8": 2, "LSTM_RESIDENT_16_8": 3, "LSTM_SPLIT4": 4, "ACT_NONE": 0, "ACT_RELU": 1, "BIAS_NONE": 0,
        "BIAS_COL": 1, "BIAS_ROW": 2, "E_UNSUPPORTED": -6, "ABI_VERSION": 5}
    constants = _header.load().constants
    for name, value in got.items():
        if name != "LSTM_SPLIT4":                                # (a host-side choice: not in the header)
            assert constants[name if name.startswith("AVS_") else "AVS_" + name] == value, name


def test_library_functions_carry_the_headers_types():
    lib = _abi.lib()
    prototypes = _header.load().prototypes
    for name in _abi.declared_symbols():
        fn = getattr(lib, name)
        assert fn.restype is _abi._SIGNATURES[name][0] and fn.restype is not None, name
        assert len(fn.argtypes) == len(prototypes[name][1]), name
        assert list(fn.argtypes) == _abi._SIGNATURES[name][1], name


def test_host_pointers_pass_as_addresses():
    """The host-side out-parameters are plain addresses now: byref(...), ctypes arrays and string buffers go through
    a c_void_p parameter unchanged (avs_device_info fills them before it asks the runtime about the device)."""
    for arg in (ctypes.byref(c_int()), (c_float * 3)(1.0, 2.0, 3.0), ctypes.create_string_buffer(8), None, 0):
        c_void_p.from_param(arg)
    buf = (c_float * 3)(1.0, 2.0, 3.0)
    out = (c_float * 3)()
    memcpy = ctypes.CDLL(None).memcpy
    memcpy.restype, memcpy.argtypes = c_void_p, [c_void_p, c_void_p, c_size_t]
    memcpy(out, buf, ctypes.sizeof(buf))
    assert list(out) == [1.0, 2.0, 3.0]
    n = c_int64()
    memcpy(ctypes.byref(n), ctypes.byref(c_int64(1 << 40)), 8)
    assert n.value == 1 << 40


# ---- the sizes the host and the kernels share --------------------------------------------------------------------------
def _shared():
    from avsum_amd import audio, ops, ragged, vggish
    from avsum_amd.features import extractors, kts
    return {
        "AVS_FUSION_MAX_N": (6400, [ragged.FUSION_MAX_N, ops.FUSION_MAX_N]),
        "AVS_FUSION_SMALL_L": (64, [ragged.FUSION_SMALL_L, ops.FUSION_SMALL_L]),
        "AVS_FUSION_MID_L": (512, [ragged.FUSION_MID_L, ops.FUSION_MID_L]),
        "AVS_FUSION_TILE": (32, [ragged._FUSION_TILE]),
        "AVS_FUSION_PAIR_COLS": (8, [ragged._FUSION_PAIR_COLS, ops.FusionTables([(0, 2, 0, 3)], "cpu").pairs.shape[1]]),
        "AVS_EVAL_MAX_T": (32768, [ragged.EVAL_MAX_T, ops.EVAL_MAX_T]),
        "AVS_EVAL_TILE": (256, [ragged.EVAL_TILE, ops.EVAL_TILE]),
        "AVS_EVAL_CHUNK": (1024, [ragged.EVAL_CHUNK, ops.EVAL_CHUNK]),
        "AVS_EVAL_COLS": (10, [ragged.EVAL_COLS, len(ops.EVAL_COLUMNS)]),
        "AVS_SHOT_INTERVAL": (3, [ragged.SHOT_INTERVAL, ops.SHOT_INTERVAL, extractors.FRAME_INTERVAL]),
        "AVS_SHOT_MAX_FRAMES": (100, [ragged.SHOT_MAX_FRAMES, ops.SHOT_MAX_FRAMES, extractors.MAX_FRAMES]),
        "AVS_SHOT_MICRO_BATCH": (4, [ragged.SHOT_MICRO_BATCH, ops.SHOT_MICRO_BATCH, extractors.MICRO_BATCH]),
        "AVS_SUMMARY_MAX_CAPACITY": (8191, [ragged.SUMMARY_MAX_CAPACITY, ops.SUMMARY_MAX_CAPACITY]),
        "AVS_KTS_MAX_SAMPLES": (2048, [kts.KTS_MAX_SAMPLES, ragged.KTS_MAX_SAMPLES, ops.KTS_MAX_SAMPLES]),
        "AVS_KTS_TILE": (64, [ragged.KTS_TILE]),
        "AVS_KTS_MAX_VIDEOS": (65535, [ragged.KTS_MAX_VIDEOS]),
        "AVS_KTS_VIDEO_COLS": (10, [ragged._KTS_VIDEO_COLS, ops.KtsTables([0, 5], 1, device="cpu").videos.shape[1]]),
        "AVS_FUSED_NFFT": (400, [audio.N_FFT]),
        "AVS_FUSED_HOP": (200, [audio.HOP]),
        "AVS_FUSED_COLS": (208, [audio.FUSED_COLS]),
        "AVS_FUSED_RE_ROWS": (204, [audio.FUSED_RE_ROWS]),
        "AVS_FUSED_IM_ROWS": (200, [audio.FUSED_IM_ROWS]),
        "AVS_VGG_WINDOW": (400, [vggish.WINDOW]),
        "AVS_VGG_HOP": (160, [vggish.HOP]),
        "AVS_VGG_BINS": (257, [vggish.NUM_BINS, vggish.FFT_LEN // 2 + 1]),
        "AVS_VGG_FRAMES": (96, [vggish.EXAMPLE_FRAMES]),
    }


def test_shared_sizes_keep_their_values_and_python_follows_the_header():
    constants = _header.load().constants
    for name, (value, python_side) in _shared().items():
        assert constants[name] == value, name                       # values do not change
        assert all(type(p) is int and p == value for p in python_side), (name, python_side)


def test_shared_sizes_are_defined_once_in_the_header():
    """Exactly one #define of every shared name across include/ and csrc/, the header's: a kernel file that defines
    its own copy again compiles (or warns) and can then disagree with the tables the host builds."""
    pkg = os.path.dirname(os.path.dirname(_abi.LIB_PATH))
    sources = [_abi.HEADER_PATH] + sorted(glob.glob(os.path.join(pkg, "csrc", "*")))
    assert len(sources) > 20
    defined = {}
    for path in sources:
        for name in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", open(path).read(), flags=re.M):
            defined.setdefault(name, []).append(path)
    for name in _shared():
        assert defined.get(name) == [_abi.HEADER_PATH], (name, defined.get(name))


def test_kts_definitions_import_without_torch():
    """features/kts.py: pure numpy, importable without torch and without the kernel library - the header reader it takes
    its limit from must not pull either in."""
    code = ("import sys; sys.path.insert(0, %r); sys.modules['torch'] = None; import avsum_amd.features.kts as k; "
            "import avsum_amd._header as h; assert k.KTS_MAX_SAMPLES == 2048; "
            "assert 'numpy' in sys.modules and 'avsum_amd._abi' not in sys.modules; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-500:]
    code = ("import sys; sys.path.insert(0, %r); sys.modules['numpy'] = None; sys.modules['torch'] = None; "
            "import avsum_amd._header as h; assert len(h.load().prototypes) == 96; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-500:]
