"""ctypes binding of the paged KV cache's split step call (include/sage_kvlsplit_gfx950.h), exported by the same ``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi`, :mod:`_cabi_kvstep` and :mod:`_cabi_kvlist`, whose symbol tables and ABI versions stay what their
headers say.  This one loads after ``_cabi.load()`` (one library handle) and, like them, raises if the library does not match -- there is no
fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_KVLSPLIT_ABI_VERSION

# every symbol include/sage_kvlsplit_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
SYMBOLS = {
    "sage_kvlsplit_abi_version": (c_int, []),
    "sage_kvlsplit_ws_bytes": (c_int64, [_I, _I, _I, _I, _I]),
    "sage_kvlsplit_attn": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                                   _L, _L, _L, _L, _L, _L, _L, _L, _I, _F, _I, _I, _P, _P, _P, _L]),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the split step call bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_kvlsplit_abi_version", ABI_VERSION, "paged KV cache split step-call ABI")
    return lib
