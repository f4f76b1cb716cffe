"""CPU-only: gpcc_debug_pool_in_use refuses null arguments like its neighbours of the debug block."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from mpeg_pcc_tmc13_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_pool_in_use_refuses_null_arguments(lib):
    fn = lib.gpcc_debug_pool_in_use
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 2)(-7, -7)
    assert fn(None, out) == -1
    assert lib.gpcc_last_error()
    assert list(out) == [-7, -7]
    # (the context is not looked at before both pointers are known to be there)
    not_a_context = C.cast((C.c_char * 64)(), C.c_void_p)
    assert fn(not_a_context, None) == -1
    assert lib.gpcc_last_error()
    # ... as gpcc_debug_alloc_events does
    lib.gpcc_debug_alloc_events.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert lib.gpcc_debug_alloc_events(None, (C.c_longlong * 4)()) == -1
