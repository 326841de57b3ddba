"""ctypes binding of the exact split of the key range for the absorbed MLA decode route (include/sage_mlasplit_gfx950.h), exported by the same
``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi_mla`, whose symbol table and ABI version stay what its header says.  It loads after ``_cabi.load()`` (one
library handle) and, like its neighbours, raises if the library does not match -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_MLASPLIT_ABI_VERSION

# every symbol include/sage_mlasplit_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
SYMBOLS = {
    "sage_mlasplit_abi_version": (c_int, []),
    "sage_mlasplit_ws_bytes": (c_int64, [_I, _I, _I, _I]),
    # sage_mla_attn's arguments, then num_splits, ws, ws_bytes
    "sage_mlasplit_attn": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _L, _F, _I, _P, _I, _P, _L]),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the split's entries bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_mlasplit_abi_version", ABI_VERSION, "MLA decode split ABI")
    return lib
