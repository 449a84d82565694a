"""ctypes binding of libavsum_hip.so, DERIVED from include/avsum_hip.h: the argument types of every entry point, the
fields of ConvDesc, the enum values and the ABI version are what _header.py reads there - none is typed here.

The product path has no CPU fallback: if the library is missing, or a call
returns a non-zero status, this module raises.  Build with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C csrc``.
"""
import ctypes
import os
from ctypes import c_int, c_int64

# torch first: its HIP runtime (torch/lib/libamdhip64) must be the one this process initialises.  Loading
# libavsum_hip.so before torch pulls in /opt/rocm's copy of the same SONAME instead, and the second runtime to come
# up then reports "no ROCm-capable device".
import torch  # noqa: F401  (memory, streams and the HIP runtime come from here)

from ._header import HEADER_PATH, load as _load_header  # noqa: F401  (HEADER_PATH: where the contract lies)

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# AVS_STUDY_LIB=1 loads the kernel-study build (`make study`: the same library with the ablation switches of tools/
# compiled in, plus avs_debug_flags); the product never sets it
# AVS_STUDY_LIB=fp16emu loads the accuracy-study flavour (`make fp16emu`: AVS_F16X2 with the lo halves forced to zero =
# the arithmetic of a plain fp16-storage mode); tools/fp16_storage_study.py only
STUDY = os.environ.get("AVS_STUDY_LIB") == "1"
_FLAVOUR = os.environ.get("AVS_STUDY_LIB")
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libavsum_hip_study.so" if STUDY else
                        "libavsum_hip_fp16emu.so" if _FLAVOUR == "fp16emu" else "libavsum_hip.so")

_HEADER = _load_header()
SHARED = _HEADER.constants     # every enumerator and shared size of the header by its C name


def _enum(names):
    """The header's values of the enumerators AVS_<name>, in the order given."""
    return tuple(_HEADER.constants["AVS_" + n] for n in names.split())


AVS_F32, AVS_BF16, AVS_F32_ACC64, AVS_F32_SPLIT, AVS_F16X2 = _enum("F32 BF16 F32_ACC64 F32_SPLIT F16X2")
AVS_W_ROWS, AVS_W_KSTEP32 = _enum("W_ROWS W_KSTEP32")
TILE_AUTO, TILE_128, TILE_256, TILE_224 = _enum("TILE_AUTO TILE_128 TILE_256 TILE_224")    # avs_conv_desc.variant
STAGING_GENERIC, CLUSTER_PACKED = _enum("STAGING_GENERIC CLUSTER_PACKED")                  # ... its bits 2 and 3
X_F16P8, Y_F16P8, RES_F16P8 = _enum("X_F16P8 Y_F16P8 RES_F16P8")                           # avs_conv_desc.formats
LSTM_AUTO, LSTM_STREAM, LSTM_RESIDENT_20_8, LSTM_RESIDENT_16_8 = _enum(
    "LSTM_AUTO LSTM_STREAM LSTM_RESIDENT_20_8 LSTM_RESIDENT_16_8")
LSTM_SPLIT4 = 4   # (host-side choice: the avs_lstm*_split_f32 entry points - one recurrence over four CUs)
ACT_NONE, ACT_RELU = _enum("ACT_NONE ACT_RELU")
BIAS_NONE, BIAS_COL, BIAS_ROW = _enum("BIAS_NONE BIAS_COL BIAS_ROW")
E_UNSUPPORTED, = _enum("E_UNSUPPORTED")
ABI_VERSION, = _enum("ABI_VERSION")


class AvsError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = _HEADER.fields("avs_conv_desc")


# name -> (restype, [argtypes]) of every entry point the header declares; every pointer but the descriptor's is an
# address (c_void_p: a tensor's data_ptr(), byref(...), a ctypes array or None)
_SIGNATURES = _HEADER.signatures({"avs_conv_desc": ConvDesc})

_lib = None


def declared_symbols():
    """Names of every function include/avsum_hip.h declares."""
    return sorted(_HEADER.prototypes)


def lib():
    """Load libavsum_hip.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AvsError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run __graft_entry__.build() or `make -C <package>/csrc`). There is no CPU fallback."
        )
    handle = ctypes.CDLL(LIB_PATH)
    if STUDY:   # the kernel-study build's ablation switches and rule setters (tools/ only)
        handle.avs_debug_flags.restype = None
        handle.avs_debug_flags.argtypes = [c_int]
        for name, args in (("avs_tune_short_reduction_bytes", [c_int]), ("avs_tune_tall_rule", [c_int, c_int]),
                           ("avs_tune_pipeline", [c_int]), ("avs_tune_bnlocal", [c_int]),
                           ("avs_tune_convbn_narrow", [c_int])):
            getattr(handle, name).restype = None
            getattr(handle, name).argtypes = args
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.avs_abi_version() != ABI_VERSION:
        raise AvsError(f"ABI version mismatch: library reports {handle.avs_abi_version()}, the header says "
                       f"{ABI_VERSION}")
    if STUDY and os.environ.get("AVS_TUNE_CONVBN_NARROW") is not None:
        handle.avs_tune_convbn_narrow(int(os.environ["AVS_TUNE_CONVBN_NARROW"]))
    if STUDY and os.environ.get("AVS_TUNE_PIPELINE") is not None:  # kernel-study override of the library default
        handle.avs_tune_pipeline(int(os.environ["AVS_TUNE_PIPELINE"]))
    _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().avs_last_error()
        raise AvsError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")


def device_info(dev=0):
    cu, clk, mem = c_int(), c_int(), c_int64()
    arch = ctypes.create_string_buffer(64)
    check(lib().avs_device_info(dev, ctypes.byref(cu), ctypes.byref(clk), ctypes.byref(mem), arch, 64),
          "avs_device_info")
    return {"cu_count": cu.value, "clock_khz": clk.value, "hbm_bytes": mem.value, "arch": arch.value.decode()}
