"""ctypes binding of libavsum_yuv.so, the planar / semi-planar / 10-bit YUV 4:2:0 entry points, DERIVED from
include/avsum_yuv.h with the reader of _header.py exactly as _ingest_abi.py derives libavsum_ingest.so's: argument types,
enumerators, shared sizes (the order of the surface description among them) and the ABI version are what the header
says - none is typed here.  The library shares nothing with the other six.

No CPU fallback: a missing library, or a non-zero status, raises.
"""
import ctypes
import functools
import os

# torch first, for the reason _abi.py gives: its HIP runtime must be the one this process initialises
import torch  # noqa: F401

from ._header import Header

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "avsum_yuv.h")
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libavsum_yuv.so")


@functools.lru_cache(maxsize=None)
def load_header():
    """include/avsum_yuv.h, read and parsed once per process."""
    with open(HEADER_PATH) as f:
        return Header(f.read())


_HEADER = load_header()
SHARED = _HEADER.constants     # every enumerator and shared size of the header by its C name
ABI_VERSION = SHARED["AVSY_ABI_VERSION"]
SHIFT = SHARED["AVSY_SHIFT"]
MAX_COEF = SHARED["AVSY_MAX_COEF"]
MATRIX_INTS = SHARED["AVSY_MATRIX_INTS"]
MAX_DIFF_FRAMES = SHARED["AVSY_MAX_DIFF_FRAMES"]
SURFACE_INTS = SHARED["AVSY_SURFACE_INTS"]
RESIZE_BAND = SHARED["AVSY_RESIZE_BAND"]
RESIZE_LDS_BYTES = SHARED["AVSY_RESIZE_LDS_BYTES"]
E_UNSUPPORTED = SHARED["AVSY_E_UNSUPPORTED"]
# the fields of h_surface in the header's order: AVSY_S_PITCH_Y -> "pitch_y"
SURFACE_FIELDS = tuple(name[len("AVSY_S_"):].lower() for name, _ in
                       sorted(((n, v) for n, v in SHARED.items() if n.startswith("AVSY_S_")), key=lambda nv: nv[1]))
assert len(SURFACE_FIELDS) == SURFACE_INTS
_SIGNATURES = _HEADER.signatures()


class AvsyError(RuntimeError):
    pass


_lib = None


def declared_symbols():
    """Names of every function include/avsum_yuv.h declares."""
    return sorted(_HEADER.prototypes)


def lib():
    """Load libavsum_yuv.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AvsyError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                        "(run __graft_entry__.build() or `make -C <package>/csrc`). There is no CPU fallback.")
    handle = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.avsy_abi_version() != ABI_VERSION:
        raise AvsyError(f"ABI version mismatch: libavsum_yuv.so reports {handle.avsy_abi_version()}, the header "
                        f"says {ABI_VERSION}")
    _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().avsy_last_error()
        raise AvsyError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
