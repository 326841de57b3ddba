"""ctypes binding of the packed (variable-length) FP8-PV route for 192-wide Q / K and 128-wide V (include/sage_qk192v_gfx950.h), exported by the
same ``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi_qk192`, whose symbol table and ABI version stay what its header says.  It loads after ``_cabi.load()``
(one library handle) and, like the others, raises if the library does not match -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_QK192V_ABI_VERSION
MASK_NONE, MASK_TOP_LEFT, MASK_BOTTOM_RIGHT = 0, 1, 2

# every symbol include/sage_qk192v_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
SYMBOLS = {
    "sage_qk192v_abi_version": (c_int, []),
    "sage_qk192v_ws_bytes": (c_int64, [_I, _I, _I, _I]),
    "sage_qk192v_prepass": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L, _L, _I, _I, _I, _P]),
    "sage_qk192v_attn": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L, _L, _I, _F, _I, _P]),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the route's entries bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_qk192v_abi_version", ABI_VERSION, "qk192v ABI")
    return lib
