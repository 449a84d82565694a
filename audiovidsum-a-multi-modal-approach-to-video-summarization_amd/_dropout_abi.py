"""ctypes binding of libavsum_dropout.so, the counter-based Dropout entry points, DERIVED from include/avsum_dropout.h
with the reader of _header.py exactly as _attn_abi.py derives libavsum_attn.so's: argument types, enumerators, launch
constants, limits and the ABI version are what the header says - none is typed here.  The library shares nothing with
the other four.

No CPU fallback: a missing library, or a non-zero status, raises.
"""
import ctypes
import functools
import os

# torch first, for the reason _abi.py gives: its HIP runtime must be the one this process initialises
import torch  # noqa: F401

from ._header import Header

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "avsum_dropout.h")
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libavsum_dropout.so")


@functools.lru_cache(maxsize=None)
def load_header():
    """include/avsum_dropout.h, read and parsed once per process."""
    with open(HEADER_PATH) as f:
        return Header(f.read())


_HEADER = load_header()
SHARED = _HEADER.constants     # every enumerator, launch constant and limit of the header by its C name
ABI_VERSION = SHARED["AVSD_ABI_VERSION"]
VEC = SHARED["AVSD_VEC"]
BLOCK = SHARED["AVSD_BLOCK"]
MAX_GROUPS = SHARED["AVSD_MAX_GROUPS"]
MAX_SEQ = SHARED["AVSD_MAX_SEQ"]
MAX_ROWS = SHARED["AVSD_MAX_ROWS"]
_SIGNATURES = _HEADER.signatures()


class AvsdError(RuntimeError):
    pass


_lib = None


def declared_symbols():
    """Names of every function include/avsum_dropout.h declares."""
    return sorted(_HEADER.prototypes)


def lib():
    """Load libavsum_dropout.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AvsdError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                        "(run __graft_entry__.build() or `make -C <package>/csrc`). There is no CPU fallback.")
    handle = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.avsd_abi_version() != ABI_VERSION:
        raise AvsdError(f"ABI version mismatch: libavsum_dropout.so reports {handle.avsd_abi_version()}, the header "
                        f"says {ABI_VERSION}")
    _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().avsd_last_error()
        raise AvsdError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
