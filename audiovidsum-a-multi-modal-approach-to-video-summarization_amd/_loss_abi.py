"""ctypes binding of libavsum_loss.so, the per-shot targets and the pairwise ranking loss, DERIVED from
include/avsum_loss.h with the reader of _header.py exactly as _dropout_abi.py derives libavsum_dropout.so's: argument
types, enumerators, launch constants, limits and the ABI version are what the header says - none is typed here.  The
library shares nothing with the other five.

No CPU fallback: a missing library, or a non-zero status, raises.
"""
import ctypes
import functools
import os

# torch first, for the reason _abi.py gives: its HIP runtime must be the one this process initialises
import torch  # noqa: F401

from ._header import Header

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "avsum_loss.h")
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libavsum_loss.so")


@functools.lru_cache(maxsize=None)
def load_header():
    """include/avsum_loss.h, read and parsed once per process."""
    with open(HEADER_PATH) as f:
        return Header(f.read())


_HEADER = load_header()
SHARED = _HEADER.constants     # every enumerator, launch constant and limit of the header by its C name
ABI_VERSION = SHARED["AVSL_ABI_VERSION"]
TILE = SHARED["AVSL_TILE"]
CHUNK = SHARED["AVSL_CHUNK"]
BLOCK = SHARED["AVSL_BLOCK"]
MAX_T = SHARED["AVSL_MAX_T"]
MAX_ROWS = SHARED["AVSL_MAX_ROWS"]
KINDS = {"logistic": SHARED["AVSL_LOGISTIC"], "hinge": SHARED["AVSL_HINGE"]}
_SIGNATURES = _HEADER.signatures()


class AvslError(RuntimeError):
    pass


_lib = None


def declared_symbols():
    """Names of every function include/avsum_loss.h declares."""
    return sorted(_HEADER.prototypes)


def lib():
    """Load libavsum_loss.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AvslError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                        "(run __graft_entry__.build() or `make -C <package>/csrc`). There is no CPU fallback.")
    handle = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.avsl_abi_version() != ABI_VERSION:
        raise AvslError(f"ABI version mismatch: libavsum_loss.so reports {handle.avsl_abi_version()}, the header "
                        f"says {ABI_VERSION}")
    _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().avsl_last_error()
        raise AvslError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
