"""ctypes binding of the appendable quantised latent of the absorbed MLA decode route (include/sage_mlacache_gfx950.h), exported by the same
``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi_mla` and :mod:`_cabi_mlasplit`, whose symbol tables and ABI versions stay what their headers say.  It
loads after ``_cabi.load()`` (one library handle) and, like them, raises if the library does not match -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_MLACACHE_ABI_VERSION

# every symbol include/sage_mlacache_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L = c_void_p, c_int, c_int64
SYMBOLS = {
    "sage_mlacache_abi_version": (c_int, []),
    "sage_mlacache_stats": (c_int, [_P, _P, _P, _P, _P, _L, _I, _I, _L, _L, _I, _I, _P]),
    "sage_mlacache_append": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _L, _L, _I, _I, _P]),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the cache's entries bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_mlacache_abi_version", ABI_VERSION, "MLA latent cache ABI")
    return lib
