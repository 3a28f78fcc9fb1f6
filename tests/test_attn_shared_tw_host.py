"""CPU checks of the shared-context focal attention under the time warp, on every shape tests/test_gpu_attn_shared_tw.py
runs: the factorisation the kernels compute (tests/_attn_shared_tw_ref.factored: the warp as one scalar per (question,
position), its energy taken per album) IS the definition (gather, time_warp_closed, attention_3d) in fp64; evaluated in
fp32 it stays inside the GPU tolerances (a shape that does not is ill conditioned: then the shape changes, never the
tolerance); the scales come in both signs; and the C ABI's host side (descriptor, size query, argument checks)."""
import ctypes

import pytest
import torch

from tests import _attn_shared_tw_ref as TW
from tests._album_attn_host import lib  # noqa: F401

ALL = TW.NAMES + TW.EXTRA
_REF = {}


def _case(name):
    if name not in _REF:
        c = TW.build_case(name)
        _REF[name] = (c, TW.reference(c, block=100))
    return _REF[name]


@pytest.mark.parametrize("name", ALL)
def test_factored_is_the_definition_in_fp64(name):
    c, (ref_ha, ref_a, ref_s) = _case(name)
    ha, a, s = TW.factored(c, torch.float64)
    for got, want, what in ((ha, ref_ha, "h_a"), (a, ref_a, "a_logits"), (s, ref_s, "scale")):
        assert torch.isfinite(got).all(), what
        err = float((got - want).abs().max())
        assert err <= 1e-9 * max(1.0, float(want[want > -1e29].abs().max())), (what, err)
    assert torch.equal(a <= -1e29, ref_a <= -1e29)                              # the same entries are masked


@pytest.mark.parametrize("name", ALL)
def test_factored_in_fp32_stays_inside_the_gpu_tolerances(name):
    c, (ref_ha, ref_a, ref_s) = _case(name)
    ha, a, s = TW.factored(c, torch.float32)
    for got, want, what in ((ha, ref_ha, "h_a"), (a, ref_a, "a_logits"), (s, ref_s, "scale")):
        ok, ratio = TW.within(got, want, what)
        print("%s %s: worst |err| / (atol + rtol |ref|) = %.3f" % (name, what, ratio))
        assert ok, (what, ratio)


def test_scales_come_in_both_signs():
    """the sign flip of the cosine form, and of s against s^2 in the bilinear form, is exercised"""
    neg = tot = 0
    for name in ALL:
        s = _case(name)[1][2]
        neg += int((s < 0).sum())
        tot += s.numel()
        assert bool((s != 0).all()), name
    share = neg / tot
    print("share of negative scales: %.3f" % share)
    assert 0.2 <= share <= 0.8, share
    c, (_, _, s) = _case("mix-simi4-masked")
    assert 0.2 <= float((s < 0).float().mean()) <= 0.8


def test_zero_rows_case_has_zero_rows_behind_the_mask():
    for name in ("zero-rows-simi2", "zero-rows-simi4"):
        c, (ha, a, s) = _case(name)
        assert not bool(c["hm"][0, 0].any()) and float(c["h"][0, 0].abs().max()) == 0.0
        assert float(c["h"][0][~c["hm"][0]].abs().max()) == 0.0 and float(c["h"][1][~c["hm"][1]].abs().max()) > 0.0
        assert torch.isfinite(ha).all() and torch.isfinite(s).all()


def test_energy_is_per_album():
    """what the factorisation rests on: the energy of a gathered question equals its album's"""
    c, _ = _case("mix-simi2-masked")
    e = TW.energy(c)
    assert e.shape == (c["A"], c["T"])
    sub = dict(c, h=c["h"][c["album"]])
    assert torch.allclose(TW.energy(sub), e[c["album"]], rtol=0, atol=1e-12)


# ------------------------------------------------------------------ the C ABI, host side
def _desc(A=2, NQ=3, K=2, T=50, JQ=10, w=64, simi=2, tanh=1, warp_type=5, window_t=2.3):
    from fvta_memexqa_amd import _lib
    return _lib.AttnSharedTwDesc(_lib.AttnSharedDesc(A, NQ, K, T, JQ, w, simi, tanh), warp_type, window_t)


def test_descriptor_and_workspace_query(lib):
    from fvta_memexqa_amd import _lib
    assert lib.fvta_abi_struct_bytes(13) == ctypes.sizeof(_lib.AttnSharedTwDesc) == 40
    d = _desc()
    nb = lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(d))
    base = lib.fvta_attn_shared_workspace_bytes(ctypes.byref(d.shape))
    assert base > 0 and nb >= base + 4 * (d.shape.NQ * d.shape.T + d.shape.w)   # the shared call's, scale [NQ,T], v [w]
    for K in (9, 64):                                                           # the attention's K limit, not the warp's 8
        assert lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(_desc(K=K))) > 0
    assert lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(_desc(K=65))) == 0


@pytest.mark.parametrize("warp_type", [0, 6, 9, -1])
def test_bad_warp_type_fails_like_the_reference(lib, warp_type):
    d = _desc(warp_type=warp_type)
    assert lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(d)) == 0
    assert b"time warping type not implemented" in lib.fvta_last_error()
    assert lib.fvta_attn_shared_energy(ctypes.byref(d), None, None, None, None, None, None) == -1
    assert b"time warping type not implemented" in lib.fvta_last_error()
    assert lib.fvta_attn_shared_fwd_tw(ctypes.byref(d), *([None] * 17)) == -1
    assert b"time warping type not implemented" in lib.fvta_last_error()


def test_argument_checks_come_back_as_status(lib):
    d = _desc()
    assert lib.fvta_attn_shared_energy(ctypes.byref(d), None, None, None, None, None, None) == -1
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_attn_shared_fwd_tw(ctypes.byref(d), *([None] * 17)) == -1
    assert b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_attn_shared_fwd_tw(None, *([None] * 17)) == -1
    bad = _desc(w=100)
    assert lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(bad)) == 0 and b"unsupported" in lib.fvta_last_error()
    assert lib.fvta_attn_shared_fwd_tw(ctypes.byref(bad), *([None] * 17)) == -3
    assert lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(_desc(simi=5))) == 0
    assert b"similarity matrix not implemented" in lib.fvta_last_error()
    assert lib.fvta_attn_shared_tw_workspace_bytes(ctypes.byref(_desc(window_t=-1.0))) == 0


def test_python_surface_validates_on_the_host():
    """the checks that need neither a GPU nor the library"""
    from fvta_memexqa_amd import functional as Fn
    h, q, lq = torch.zeros(2, 2, 5, 64), torch.zeros(3, 4, 64), torch.zeros(3, 64)
    W, b = torch.zeros(128, 1), torch.zeros(1)
    tw = (torch.zeros(128, 64), torch.zeros(64), torch.zeros(64, 1), torch.zeros(1))
    with pytest.raises(Exception, match="time warping type not implemented"):
        Fn.attention_3d_shared_warped_raw(h, q, [0, 1, 1], lq, W, b, *tw, simiMatrix=2, warp_type=7)
    with pytest.raises(ValueError, match="lq"):
        Fn.attention_3d_shared_warped_raw(h, q, [0, 1, 1], lq[:2], W, b, *tw, simiMatrix=2, warp_type=5)
    with pytest.raises(ValueError, match="album index"):
        Fn.attention_3d_shared_warped_raw(h, q, [0, 1, 2], lq, W, b, *tw, simiMatrix=2, warp_type=5)
    with pytest.raises(ValueError, match="energy"):
        Fn.attention_3d_shared_warped_raw(h, q, [0, 1, 1], lq, W, b, *tw, simiMatrix=2, warp_type=5, energy=torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_shared_warped_raw(h, q.clone().requires_grad_(), [0, 1, 1], lq, W, b, *tw, simiMatrix=2, warp_type=5)
