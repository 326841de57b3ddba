"""ctypes binding of the appendable KV cache's entry points (include/sage_kvcache_gfx950.h), exported by the same ``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi`: that module's symbol table and ABI version are the main header's, entry for entry, and stay so.
This one loads after ``_cabi.load()`` (one library handle) and, like it, raises if the library does not match -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_KVCACHE_ABI_VERSION

# every symbol include/sage_kvcache_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L = c_void_p, c_int, c_int64
SYMBOLS = {
    "sage_kvcache_abi_version": (c_int, []),
    "sage_kvcache_append": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _L, _L, _L, _L, _L, _L, _I, _P]),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the cache's entry points bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_kvcache_abi_version", ABI_VERSION, "KV cache ABI")
    return lib
