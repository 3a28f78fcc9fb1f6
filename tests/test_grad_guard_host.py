"""Gradient guard, the part that needs no GPU: the new entry points load, the workspace query answers, bad arguments
come back as -1 with a message before anything is launched, the two new structs have the library's layout, and the
Trainer validates its three config keys (all off by default)."""
import ctypes
import math
import os

import pytest

from fvta_memexqa_amd import _lib

NEW = ("fvta_grad_guard_workspace_bytes", "fvta_grad_guard", "fvta_adadelta_step_guarded", "fvta_adam_step_guarded")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_new_symbols_load(lib):
    for name in NEW:
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name), name


def test_workspace_query_is_positive_and_non_decreasing(lib):
    sizes = [lib.fvta_grad_guard_workspace_bytes(n) for n in (1, 3, 255, 256, 257, 1024, 1025, 4099, 1 << 20, (1 << 21) + 1,
                                                              1 << 23, 1 << 28, 1 << 33)]
    assert sizes[0] > 0
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] == sizes[-2]                   # the grid is capped: the partials stop growing
    assert lib.fvta_grad_guard_workspace_bytes(0) == 0 and b"positive" in lib.fvta_last_error()
    assert lib.fvta_grad_guard_workspace_bytes(-5) == 0


def test_struct_sizes_match_their_mirrors(lib):
    assert lib.fvta_abi_struct_bytes(6) == ctypes.sizeof(_lib.GuardDesc) == 32
    assert lib.fvta_abi_struct_bytes(7) == ctypes.sizeof(_lib.GuardCtl) == 56
    assert _lib.GuardCtl.norm.offset == 24 and _lib.GuardCtl.applied.offset == 40
    assert lib.fvta_abi_struct_bytes(8) == -1


def _desc(**kw):
    d = dict(grad_scale=1.0, clip_value=0.0, clip_norm=0.0, skip_nonfinite=0, adam=0, lr=0.0, beta1=0.0, beta2=0.0)
    d.update(kw)
    return _lib.GuardDesc(**d)


def test_bad_arguments_return_minus_one_with_a_message(lib):
    # every call returns at its argument check: the buffers are host memory that no kernel ever sees
    grad = (ctypes.c_float * 8)()
    ws = (ctypes.c_double * 64)()
    ctl = _lib.GuardCtl()
    g, w, c = ctypes.addressof(grad), ctypes.addressof(ws), ctypes.addressof(ctl)

    def call(d, g=g, n=8, w=w, c=c):
        return lib.fvta_grad_guard(ctypes.byref(d) if d is not None else None, g, n, w, c, None)
    ok = _desc()
    for kw in (dict(d=None), dict(d=ok, g=None), dict(d=ok, w=None), dict(d=ok, c=None)):
        assert call(**kw) == -1 and b"null pointer" in lib.fvta_last_error(), kw
    assert call(ok, n=0) == -1 and b"n must be positive" in lib.fvta_last_error()
    assert call(ok, n=-3) == -1
    assert call(_desc(clip_norm=-1.0)) == -1 and b"clip_norm" in lib.fvta_last_error()
    assert call(_desc(clip_norm=math.nan)) == -1 and b"clip_norm" in lib.fvta_last_error()
    assert call(_desc(clip_value=-0.5)) == -1 and b"clip_value" in lib.fvta_last_error()
    assert call(_desc(clip_value=math.nan)) == -1 and b"clip_value" in lib.fvta_last_error()
    assert call(_desc(clip_norm=math.inf)) == -1
    assert call(_desc(skip_nonfinite=2)) == -1 and b"skip_nonfinite" in lib.fvta_last_error()
    assert call(_desc(adam=1, lr=1e-3, beta1=1.0, beta2=0.999)) == -1 and b"beta1" in lib.fvta_last_error()
    assert call(ok, g=g + 2) == -1 and b"alignment" in lib.fvta_last_error()
    # the guarded steps
    assert lib.fvta_adadelta_step_guarded(g, g, g, g, 8, 0.5, 0.95, 1e-8, None, None) == -1
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_adadelta_step_guarded(g, g, g, g, 0, 0.5, 0.95, 1e-8, c, None) == -1
    assert b"n must be positive" in lib.fvta_last_error()
    assert lib.fvta_adam_step_guarded(g, None, g, g, 8, 0.9, 0.999, 1e-8, c, None) == -1
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_adam_step_guarded(g, g, g, g, 0, 0.9, 0.999, 1e-8, c, None) == -1


def test_trainer_validates_the_config_keys():
    from types import SimpleNamespace
    from fvta_memexqa_amd.trainer import Trainer
    t = Trainer(object(), {})
    assert not t.guard_on and t.guard_ctl is None
    assert (t.clip_value, t.clip_norm, t.skip_nonfinite) == (0.0, 0.0, False)
    for bad in (dict(clip_global_norm=-1), dict(clip_global_norm=math.nan), dict(clip_gradient_value=-0.1),
                dict(clip_gradient_value=math.inf), dict(clip_global_norm="big"), dict(skip_nonfinite="yes"),
                dict(skip_nonfinite=2), dict(clip_global_norm=True)):
        with pytest.raises(ValueError):
            Trainer(object(), bad)
        with pytest.raises(ValueError):
            Trainer(object(), SimpleNamespace(**bad))
    assert Trainer(object(), dict(clip_global_norm=5)).guard_on
    assert Trainer(object(), dict(clip_gradient_value=0.1)).guard_on
    assert Trainer(object(), SimpleNamespace(skip_nonfinite=True)).guard_on
    assert not Trainer(object(), dict(clip_global_norm=0, clip_gradient_value=None, skip_nonfinite=False)).guard_on
    st = Trainer(object(), dict(skip_nonfinite=True, optimizer="adam")).guard_stats()     # no device yet: the counters
    assert st["applied"] == 0 and st["skipped"] == 0
