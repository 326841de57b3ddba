"""ctypes binding of the paged KV cache's page pool (include/sage_kvpool_gfx950.h), exported by the same ``libsage_gfx950.so``.

A binding of its own beside :mod:`_cabi` and the seven ``_cabi_kv*`` modules, whose symbol tables and ABI versions stay what their headers
say.  This one loads after ``_cabi.load()`` (one library handle) and, like them, raises if the library does not match -- there is no fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p

from . import _cabi

ABI_VERSION = 1       # SAGE_KVPOOL_ABI_VERSION

# every symbol include/sage_kvpool_gfx950.h declares: name -> (restype, argtypes)
_P, _I, _L = c_void_p, c_int, c_int64
_GEOM = [_P, _L, _P, _L, _I, _I, _I, _I]          # pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B
_RESERVE = _GEOM + [_P, _P, _I, _P, _I, _I, _P]
_RELEASE = _GEOM + [_P, _P, _I]
_FORK = _GEOM + [_P, _P, _P, _P, _I, _P, _P]
SYMBOLS = {
    "sage_kvpool_abi_version": (c_int, []),
    "sage_kvpool_ws_bytes": (c_int64, [_I, _I]),
    "sage_kvpool_init": (c_int, [_P, _L, _I, _I, _P]),
    "sage_kvpool_init_host": (c_int, [_P, _L, _I, _I]),
    "sage_kvpool_reserve": (c_int, _RESERVE + [_P]),
    "sage_kvpool_reserve_host": (c_int, _RESERVE),
    "sage_kvpool_release": (c_int, _RELEASE + [_P]),
    "sage_kvpool_release_host": (c_int, _RELEASE),
    "sage_kvpool_fork_prepare": (c_int, _FORK + [_P]),
    "sage_kvpool_fork_prepare_host": (c_int, _FORK),
}


def load() -> ctypes.CDLL:
    """The library of ``_cabi.load()`` with the page pool's entries bound (once, by ``_cabi.bind``)."""
    lib = _cabi.load()
    _cabi.bind(lib, SYMBOLS, "sage_kvpool_abi_version", ABI_VERSION, "paged KV cache page pool ABI")
    return lib
