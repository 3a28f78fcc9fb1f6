"""Scorer, weight decay and Adadelta entry points, the part that needs no GPU: bad arguments come back as the library's
invalid-argument code (-1) with a message in fvta_last_error() before anything is launched."""
import ctypes

import pytest

from fvta_memexqa_amd import _lib

INVALID_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _desc(N=6, C=4, w=64, eu=0, tanh=0, xent_grad=0):
    return _lib.ScorerDesc(N, C, w, eu, tanh, xent_grad)


def _fwd(lib, d):
    # every pointer is null: a call that got past the descriptor check would stop at the null-pointer check, and the
    # message tells the two apart
    return lib.fvta_scorer_ce_fwd(ctypes.byref(d) if d is not None else None, None, None, None, None, None, None, None,
                                  None, None, None)


def _bwd(lib, d):
    return lib.fvta_scorer_ce_bwd(ctypes.byref(d) if d is not None else None, None, None, None, None, None, None, None,
                                  None, 1.0, None, None, None, None, None, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_scorer_rejects_a_bad_descriptor(lib, call):
    for kw in (dict(C=0), dict(C=65), dict(N=0), dict(w=0), dict(C=-1), dict(N=-3)):
        assert call(lib, _desc(**kw)) == INVALID_ARG, kw
        assert b"bad descriptor" in lib.fvta_last_error(), kw
    assert call(lib, None) == INVALID_ARG and b"bad descriptor" in lib.fvta_last_error()
    assert call(lib, _desc(xent_grad=2)) == INVALID_ARG and b"xent_grad" in lib.fvta_last_error()
    assert call(lib, _desc(xent_grad=-1)) == INVALID_ARG and b"xent_grad" in lib.fvta_last_error()
    # the limits themselves are accepted: C = 1, C = 64 and xent_grad = 1 get as far as the pointer check
    for kw in (dict(C=1), dict(C=64), dict(xent_grad=1), dict(N=1, w=1)):
        assert call(lib, _desc(**kw)) == INVALID_ARG, kw
        assert b"null pointer" in lib.fvta_last_error(), kw


def test_weight_decay_and_adadelta_reject_bad_arguments(lib):
    # the buffers are host memory that no kernel ever sees: every call returns at its argument check
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert lib.fvta_weight_decay(p, p, 0, 0.014, None, None) == INVALID_ARG
    assert b"weight_decay" in lib.fvta_last_error()
    assert lib.fvta_weight_decay(p, p, -4, 0.014, None, None) == INVALID_ARG
    assert lib.fvta_weight_decay(p, None, 8, 0.014, None, None) == INVALID_ARG       # grad and loss both null
    assert b"weight_decay" in lib.fvta_last_error()
    assert lib.fvta_weight_decay(None, None, 8, 0.014, None, None) == INVALID_ARG
    assert lib.fvta_adadelta_step(p, p, p, p, 0, 0.5, 0.95, 1e-8, 1.0, None) == INVALID_ARG
    assert b"adadelta_step" in lib.fvta_last_error()
    assert lib.fvta_adadelta_step(p, p, p, p, -1, 0.5, 0.95, 1e-8, 1.0, None) == INVALID_ARG
    assert lib.fvta_adadelta_step(None, None, None, None, 8, 0.5, 0.95, 1e-8, 1.0, None) == INVALID_ARG
