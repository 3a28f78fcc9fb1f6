"""CPU-side checks of the context-tensor calls (fvta_context_fwd / _bwd, model_v2.py:863-914): exported and bound, bad
descriptors and pointers come back as FVTA_ERR_INVALID_ARG with a message before anything is launched (there is no GPU
here, so a call that got as far as a launch would fail differently), and the Python surface refuses to run without a GPU."""
import ctypes
import os

import pytest
import torch

from fvta_memexqa_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _desc(N, M, Js, w, K=None):
    d = _lib.ContextDesc(N, len(Js) if K is None else K, M, w)
    for k, J in enumerate(Js[:_lib.CTX_KMAX]):
        d.J[k] = J
    return d


def _fake(K):
    """K non-NULL, 16-byte aligned addresses that are never dereferenced: every call below is refused by validation"""
    return (ctypes.c_void_p * max(K, 1))(*[0x1000 * (i + 1) for i in range(max(K, 1))])


def test_symbols_are_exported_and_bound(lib):
    for name in ("fvta_context_fwd", "fvta_context_bwd"):
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)
    assert ctypes.sizeof(_lib.ContextDesc) == 48 and _lib.ContextDesc.J.offset == 16      # twelve int32, as the header says
    assert _lib.CTX_KMAX == 8


BAD = {
    "K = 0": (_desc(2, 1, [], 8), b"K must be in 1..8"),
    "K = 9": (_desc(2, 1, [3] * 8, 8, K=9), b"K must be in 1..8"),
    "J[k] = 0": (_desc(2, 1, [3, 0, 2], 8), b"J[1] must be >= 1"),
    "N = 0": (_desc(0, 1, [3], 8), b"N, M, w must be >= 1"),
    "w = 0": (_desc(1, 1, [3], 0), b"N, M, w must be >= 1"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_descriptors_are_refused_both_ways(lib, name):
    d, msg = BAD[name]
    p = _fake(8)
    hall = ctypes.c_void_p(0x100000)
    assert lib.fvta_context_fwd(ctypes.byref(d), p, None, hall, None, None) == -1
    assert msg in lib.fvta_last_error() and b"context_fwd" in lib.fvta_last_error()
    assert lib.fvta_context_bwd(ctypes.byref(d), hall, p, None) == -1
    assert msg in lib.fvta_last_error() and b"context_bwd" in lib.fvta_last_error()


def test_null_pointers_are_refused(lib):
    d = _desc(2, 1, [3, 5], 8)
    p, hall, hm = _fake(2), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000)
    assert lib.fvta_context_fwd(ctypes.byref(d), p, None, None, None, None) == -1            # a NULL hall
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_context_fwd(ctypes.byref(d), None, None, hall, None, None) == -1          # no stream table
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_context_fwd(ctypes.byref(d), p, _fake(2), hall, None, None) == -1         # masks without hall_mask
    assert b"go together" in lib.fvta_last_error()
    assert lib.fvta_context_fwd(ctypes.byref(d), p, None, hall, hm, None) == -1               # hall_mask without masks
    assert b"go together" in lib.fvta_last_error()
    holes = (ctypes.c_void_p * 2)(0x1000, None)
    assert lib.fvta_context_fwd(ctypes.byref(d), holes, None, hall, None, None) == -1         # a NULL stream
    assert b"streams[1] is null" in lib.fvta_last_error()
    assert lib.fvta_context_fwd(ctypes.byref(d), p, holes, hall, hm, None) == -1              # a NULL mask
    assert b"masks[1] is null" in lib.fvta_last_error()
    assert lib.fvta_context_fwd(None, p, None, hall, None, None) == -1
    assert lib.fvta_context_bwd(ctypes.byref(d), None, p, None) == -1                          # a NULL d_hall
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_context_bwd(ctypes.byref(d), hall, None, None) == -1
    assert b"null pointer" in lib.fvta_last_error()


def test_a_backward_with_every_stream_skipped_launches_nothing(lib):
    """d_streams[k] == NULL is skipped; with all of them NULL there is nothing to write, so the call succeeds without a
    launch -- which is why it can be made here, where a launch would fail."""
    d = _desc(2, 1, [3, 5], 8)
    none = (ctypes.c_void_p * 2)(None, None)
    assert lib.fvta_context_bwd(ctypes.byref(d), ctypes.c_void_p(0x100000), none, None) == 0


def test_python_surface_refuses_bad_lists_and_runs_only_on_a_gpu():
    from fvta_memexqa_amd import functional as Fn
    s = lambda J, N=2, M=1, w=8: torch.zeros(N, M, J, w)
    with pytest.raises(ValueError, match="K = 9"):
        Fn.context_tensor([s(2)] * 9)
    with pytest.raises(ValueError, match="K = 0"):
        Fn.context_tensor([])
    with pytest.raises(ValueError, match="must agree"):
        Fn.context_tensor([s(2), s(3, w=4)])
    with pytest.raises(ValueError, match="must agree"):
        Fn.context_tensor([s(2), s(3, N=3)])
    with pytest.raises(ValueError, match="must agree"):
        Fn.context_tensor([s(2), s(3, M=2)])
    with pytest.raises(ValueError, match="1 masks for 2 streams"):
        Fn.context_tensor([s(2), s(3)], [torch.ones(2, 1, 2, dtype=torch.bool)])
    with pytest.raises(ValueError, match="mask 1"):
        Fn.context_tensor([s(2), s(3)], [torch.ones(2, 1, 2, dtype=torch.bool), torch.ones(2, 1, 2, dtype=torch.bool)])
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.FvtaError, match="no CPU fallback"):
        Fn.context_tensor([s(2), s(3)])
    with pytest.raises(_lib.FvtaError, match="no CPU fallback"):
        Fn.time_warp_raw(torch.zeros(1, 1, 3, 4), torch.zeros(1, 4), torch.zeros(8, 4), torch.zeros(4), torch.zeros(4, 1),
                         torch.zeros(1))
    from fvta_memexqa_amd import nn as fnn
    for make in (lambda: fnn.TimeWarp(8), lambda: fnn.TokenEmbedding(7, 12), lambda: fnn.PhotoFeatures(24, 10)):
        with pytest.raises(_lib.FvtaError, match="no CPU fallback"):
            make()
