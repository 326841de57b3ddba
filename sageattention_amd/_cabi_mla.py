"""ctypes binding of the FP8-PV route for the absorbed MLA decode shape, 576-wide Q / K against the latent's first 512 channels as V
(include/sage_mla_gfx950.h), exported by the same ``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi`, :mod:`_cabi_hd256`, :mod:`_cabi_qk192` and the ``_cabi_kv*`` modules, whose symbol tables and ABI
versions stay what their headers say.  It loads after ``_cabi.load()`` (one library handle) and, like them, raises if the library does not
match -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_MLA_ABI_VERSION

# every symbol include/sage_mla_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
SYMBOLS = {
    "sage_mla_abi_version": (c_int, []),
    "sage_mla_ws_floats": (c_int64, [_I, _I]),
    "sage_mla_prepass": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _L, _L, _I, _I, _P]),
    "sage_mla_attn": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _L, _F, _I, _P]),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the route's entries bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_mla_abi_version", ABI_VERSION, "MLA decode ABI")
    return lib
