"""ctypes binding of libavsum_render.so, the summary-rendering entry points (frame list, BGR -> YUV 4:2:0, repack, audio
cut), DERIVED from include/avsum_render.h with the reader of _header.py exactly as _yuv_abi.py derives libavsum_yuv.so's:
argument types, enumerators, shared sizes (the tile of the index and the order of the surface description among them)
and the ABI version are what the header says - none is typed here.  The library shares nothing with the other seven.

No CPU fallback: a missing library, or a non-zero status, raises.
"""
import ctypes
import functools
import os

# torch first, for the reason _abi.py gives: its HIP runtime must be the one this process initialises
import torch  # noqa: F401

from ._header import Header

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "avsum_render.h")
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libavsum_render.so")


@functools.lru_cache(maxsize=None)
def load_header():
    """include/avsum_render.h, read and parsed once per process."""
    with open(HEADER_PATH) as f:
        return Header(f.read())


_HEADER = load_header()
SHARED = _HEADER.constants     # every enumerator and shared size of the header by its C name
ABI_VERSION = SHARED["AVSR_ABI_VERSION"]
SHIFT = SHARED["AVSR_SHIFT"]
MAX_ROW_SUM = SHARED["AVSR_MAX_ROW_SUM"]
FORWARD_INTS = SHARED["AVSR_FORWARD_INTS"]
SURFACE_INTS = SHARED["AVSR_SURFACE_INTS"]
TILE = SHARED["AVSR_TILE"]
TILE_COLS = SHARED["AVSR_TILE_COLS"]
MAX_FRAMES = SHARED["AVSR_MAX_FRAMES"]
TOTAL_COLS = SHARED["AVSR_TOTAL_COLS"]
AUDIO_TILE = SHARED["AVSR_AUDIO_TILE"]
AUDIO_COLS = SHARED["AVSR_AUDIO_COLS"]
E_UNSUPPORTED = SHARED["AVSR_E_UNSUPPORTED"]
# the fields of h_surface in the header's order: AVSR_S_PITCH_Y -> "pitch_y"
SURFACE_FIELDS = tuple(name[len("AVSR_S_"):].lower() for name, _ in
                       sorted(((n, v) for n, v in SHARED.items() if n.startswith("AVSR_S_")), key=lambda nv: nv[1]))
assert len(SURFACE_FIELDS) == SURFACE_INTS
_SIGNATURES = _HEADER.signatures()


class AvsrError(RuntimeError):
    pass


_lib = None


def declared_symbols():
    """Names of every function include/avsum_render.h declares."""
    return sorted(_HEADER.prototypes)


def lib():
    """Load libavsum_render.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AvsrError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                        "(run __graft_entry__.build() or `make -C <package>/csrc`). There is no CPU fallback.")
    handle = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.avsr_abi_version() != ABI_VERSION:
        raise AvsrError(f"ABI version mismatch: libavsum_render.so reports {handle.avsr_abi_version()}, the header "
                        f"says {ABI_VERSION}")
    _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().avsr_last_error()
        raise AvsrError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
