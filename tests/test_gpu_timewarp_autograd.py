"""The time warp (model_v2.py:953-1009) under torch.autograd: autograd.time_warp, functional.time_warp /
time_indication_func, nn.TimeWarp, and its `scale` fed into the focal attention as C [N,T], against the fp64 oracle.

Tolerances: the warp's own quantities use what tests/test_gpu_timewarp.py applies to the same kernels (rtol 2e-4, atol
2e-5 x max(1, |ref|max)); the attention's quantities use tests/test_gpu_autograd.py's RTOL / ATOL."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_autograd import ATOL, RTOL, _close

pytestmark = pytest.mark.gpu

NAMES = ("hall", "lq", "WH/W", "WH/b", "WC/W", "WC/b")


def _wclose(got, want, msg=""):
    wv = want.detach().cpu().double().numpy()
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), wv, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(wv).max()),
                               err_msg=msg)


def _cu(t):
    return t.cuda().contiguous()


def _case(N, K, T, w, seed):
    """hall, lq, WH_W, WH_b, WC_W [w,1], WC_b scaled so that tanh stays off its flat ends, and the two upstream gradients"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    leaves = (r(N, K, T, w) * 0.5, r(N, w) * 0.5, r(2 * w, w) * 0.05, r(w) * 0.05, r(w, 1) * 0.1, r(1) * 0.05)
    return leaves, r(N, K, T, w), r(N, T)


def _cnt(T, warp_type, window_t):
    from oracle import fvta_fused as F
    return F.time_indication_band(T, warp_type, window_t, torch.float64).sum(1)


@functools.lru_cache(maxsize=None)
def _reference(N, K, T, w, warp_type, window_t, seed):
    """warp_h, scale and the six gradients for upstream gradients on both outputs / warp_h only / scale only (fp64)"""
    from oracle import fvta_fused as F
    leaves, G1, G2 = _case(N, K, T, w, seed)
    out = {}
    for which in ("both", "warp", "scale"):
        L = [t.double().requires_grad_() for t in leaves]
        warp, c = F.time_warp_closed(*L, warp_type=warp_type, window_t=window_t)
        scale = c * _cnt(T, warp_type, window_t)[None, :]
        loss = 0.0
        if which != "scale":
            loss = loss + (warp * G1.double()).sum()
        if which != "warp":
            loss = loss + (scale * G2.double()).sum()
        loss.backward()
        out[which] = [t.grad for t in L]
    return warp.detach(), scale.detach(), out


def _check_grads(got, ref, w, tag):
    for g, r, name in zip(got, ref, NAMES):
        _wclose(g.reshape(r.shape), r, "%s: d %s" % (tag, name))
    assert bool((got[2].reshape(2 * w, w)[w:] == 0).all()), "%s: rows w..2w of d WH/W see a zero feature" % tag


SHAPES = [((2, 3, 17, 64), wt, 1.4) for wt in (1, 2, 3, 4, 5)] + [((1, 2, 3, 8), wt, 3.0) for wt in (3, 4, 5)]


@pytest.mark.parametrize("shape,warp_type,window_t", SHAPES)
def test_autograd_time_warp(shape, warp_type, window_t):
    """window 1.4 -> 2 rows either side (the band matters); window 3.0 on T = 3: wider than the sequence, both ends clamp"""
    from fvta_memexqa_amd import autograd as ag
    N, K, T, w = shape
    seed = 100 * warp_type + T
    ref_warp, ref_scale, ref_grads = _reference(N, K, T, w, warp_type, window_t, seed)
    leaves, G1, G2 = _case(N, K, T, w, seed)
    for which in ("both", "warp", "scale"):
        L = [_cu(t).requires_grad_() for t in leaves]
        warp, scale = ag.time_warp(*L, warp_type=warp_type, window_t=window_t)
        assert warp.shape == (N, K, T, w) and scale.shape == (N, T)
        _wclose(warp, ref_warp, "warp_h")
        _wclose(scale, ref_scale, "scale")
        outs = [warp, scale] if which == "both" else [warp] if which == "warp" else [scale]
        gs = [_cu(G1), _cu(G2)] if which == "both" else [_cu(G1)] if which == "warp" else [_cu(G2)]
        torch.autograd.backward(outs, gs)
        _check_grads([t.grad for t in L], ref_grads[which], w, "type %d, upstream on %s" % (warp_type, which))
    # nothing requires grad: the same kernels, no graph, the same bits
    plain_w, plain_s = ag.time_warp(*[_cu(t) for t in leaves], warp_type=warp_type, window_t=window_t)
    assert plain_w.grad_fn is None and plain_s.grad_fn is None
    assert torch.equal(plain_w, warp.detach()) and torch.equal(plain_s, scale.detach())


def _set_warp_vars(Fn, leaves, scope="time_warp"):
    Fn.reset_default_graph()
    vs = [_cu(t).requires_grad_() for t in leaves[2:]]
    for tail, v in zip(("WH/W", "WH/b", "WC/W", "WC/b"), vs):
        Fn.variables["%s/%s" % (scope, tail)] = v
    return vs


@pytest.mark.parametrize("shape", [(2, 2, 9, 100), (1, 1, 5, 6)])        # w = 6: zero padded to 8 outside the kernels
def test_functional_time_warp(shape):
    """warp_type 5 with the window read from the store's time_warp_C/time_warp_window_t (3.0); hall given 5-D"""
    from fvta_memexqa_amd import functional as Fn
    N, K, T, w = shape
    seed = 7 + w
    ref_warp, ref_scale, ref_grads = _reference(N, K, T, w, 5, 3.0, seed)
    leaves, G1, G2 = _case(N, K, T, w, seed)
    try:
        vs = _set_warp_vars(Fn, leaves)
        hall, lq = _cu(leaves[0]).reshape(N, K, 1, T, w).requires_grad_(), _cu(leaves[1]).requires_grad_()
        warp, scale = Fn.time_warp(hall, lq, warp_type=5)
        win = Fn.variables["time_warp/time_warp_C/time_warp_window_t"]
        assert win.dim() == 0 and float(win) == 3.0 and not win.requires_grad
        assert warp.shape == hall.shape and scale.shape == (N, T)
        _wclose(warp.reshape(N, K, T, w), ref_warp, "warp_h")
        _wclose(scale, ref_scale, "scale")
        torch.autograd.backward([warp, scale], [_cu(G1).reshape(hall.shape), _cu(G2)])
        _check_grads([hall.grad.reshape(N, K, T, w), lq.grad] + [v.grad for v in vs], ref_grads["both"], w, "functional")
        with torch.no_grad():
            again_w, again_s = Fn.time_warp(hall, lq, warp_type=5, window_t=3.0)
        assert again_w.grad_fn is None and torch.equal(again_w, warp.detach()) and torch.equal(again_s, scale.detach())
    finally:
        Fn.reset_default_graph()


def test_functional_time_warp_creates_the_reference_variables():
    from fvta_memexqa_amd import functional as Fn
    Fn.reset_default_graph()
    try:
        h, lq = torch.randn(1, 2, 4, 12, device="cuda"), torch.randn(1, 12, device="cuda")
        Fn.time_warp(h, lq, warp_type=3, scope="tw")
        assert {k: tuple(v.shape) for k, v in Fn.variables.items()} == {
            "tw/WH/W": (24, 12), "tw/WH/b": (12,), "tw/WC/W": (12, 1), "tw/WC/b": (1,)}
        assert float(Fn.variables["tw/WH/b"].abs().max()) == 0 and float(Fn.variables["tw/WC/W"].abs().max()) > 0
        Fn.time_warp(h, lq, warp_type=5)
        assert tuple(Fn.variables["time_warp/time_warp_C/time_warp_window_t"].shape) == ()
        with pytest.raises(Exception, match="time warping type not implemented"):
            Fn.time_warp(h, lq, warp_type=6)
        with pytest.raises(Exception, match="time warping type not implemented"):
            Fn.time_indication_func(torch.zeros(1, 4, 4, device="cuda"), warp_type=0)
    finally:
        Fn.reset_default_graph()


def test_module_applied_twice_sums_the_parameter_gradients():
    from fvta_memexqa_amd import nn as fnn
    from oracle import fvta_fused as F
    N, K, T, w, wt, win = 2, 3, 17, 64, 5, 1.4
    leaves, G1, G2 = _case(N, K, T, w, 41)
    other, _, _ = _case(N, K, T, w, 42)
    mod = fnn.TimeWarp(w, warp_type=wt, window_t=win, seed=3)
    sd = mod.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "WH/W": (2 * w, w), "WH/b": (w,), "WC/W": (w, 1), "WC/b": (1,), "time_warp_C/time_warp_window_t": ()}
    assert abs(float(sd["time_warp_C/time_warp_window_t"]) - win) < 1e-6
    assert set(dict(mod.named_parameters())) == {"WH/W", "WH/b", "WC/W", "WC/b"}      # the window never gets a gradient
    with torch.no_grad():
        for name, t in zip(NAMES[2:], leaves[2:]):
            mod.p(name).copy_(_cu(t))
    P = [t.double().requires_grad_() for t in leaves[2:]]
    loss = 0.0
    for h, lq in ((leaves[0], leaves[1]), (other[0], other[1])):
        warp, c = F.time_warp_closed(h.double(), lq.double(), *P, warp_type=wt, window_t=win)
        loss = loss + (warp * G1.double()).sum() + (c * _cnt(T, wt, win)[None] * G2.double()).sum()
    loss.backward()
    w1, s1 = mod(_cu(leaves[0]), _cu(leaves[1]))
    w2, s2 = mod(_cu(other[0]), _cu(other[1]))
    torch.autograd.backward([w1, s1, w2, s2], [_cu(G1), _cu(G2), _cu(G1), _cu(G2)])
    for name, ref in zip(NAMES[2:], P):
        _wclose(mod.p(name).grad, ref.grad, "d %s over two calls" % name)
    with pytest.raises(Exception, match="time warping type not implemented"):
        fnn.TimeWarp(w, warp_type=7)
    # the window lives in the state dict: a twin loaded from it warps alike
    twin = fnn.TimeWarp(w, warp_type=wt, window_t=9.0)
    twin.load_state_dict(mod.state_dict())
    with torch.no_grad():
        tw, ts = twin(_cu(leaves[0]), _cu(leaves[1]))
    assert torch.equal(tw, w1.detach()) and torch.equal(ts, s1.detach())


def _att_inputs(N, K, T, JQ, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(N, JQ, w) * 0.5, r(2 * w, 1) * 0.1, r(1) * 0.1, r(N, w), r(N, K, T, JQ)


def test_chained_with_the_attention():
    """functional.time_warp -> functional.attention_3d(time_warp_att=True, C=scale), loss <G1,h_a> + <G2,a_logits>: the
    gradient reaches hall, lq and the four warp parameters through the warped rows AND through the scale."""
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, K, T, JQ, w, wt, win = 2, 2, 12, 5, 64, 5, 1.4
    leaves, _, _ = _case(N, K, T, w, 77)
    hq, W, b, G1, G2 = _att_inputs(N, K, T, JQ, w, 78)
    L = [t.double().requires_grad_() for t in leaves + (hq, W, b)]
    warp, c = F.time_warp_closed(*L[:6], warp_type=wt, window_t=win)
    C = c[:, :, None] * F.time_indication_band(T, wt, win, torch.float64)[None]
    ra, rl = F.attention_3d(warp, L[6], L[7], L[8], None, None, simiMatrix=2, add_tanh=True, time_warp_att=True, C=C)
    torch.autograd.backward([ra, rl], [G1.double(), G2.double()])
    try:
        vs = _set_warp_vars(Fn, leaves)
        Wc, bc = _cu(W).requires_grad_(), _cu(b).requires_grad_()
        Fn.variables["attention_2vector/att_logits/W"], Fn.variables["attention_2vector/att_logits/b"] = Wc, bc
        hall, lq, q = (_cu(t).requires_grad_() for t in (leaves[0], leaves[1], hq))
        wh, scale = Fn.time_warp(hall, lq, warp_type=wt, window_t=win)
        ha, a = Fn.attention_3d(wh, q, simiMatrix=2, add_tanh=True, time_warp_att=True, C=scale)
        _close(ha, ra, rtol=RTOL, atol=ATOL, msg="h_a")
        _close(a, rl, rtol=RTOL, atol=ATOL, msg="a_logits")
        torch.autograd.backward([ha, a], [_cu(G1), _cu(G2)])
        for got, ref, nm in zip((hall, lq, q, Wc, bc), (L[0], L[1], L[6], L[7], L[8]), ("hall", "lq", "hq", "att W", "att b")):
            _close(got.grad, ref.grad, rtol=RTOL, atol=ATOL, msg="d " + nm)
        for v, ref, nm in zip(vs, L[2:6], NAMES[2:]):
            _wclose(v.grad, ref.grad, "d " + nm)
        assert float(L[2].grad[:w].abs().max()) > 0 and bool((vs[0].grad[w:] == 0).all())
    finally:
        Fn.reset_default_graph()


def test_attention_3d_takes_the_row_sums_in_place_of_C():
    from fvta_memexqa_amd import functional as Fn
    from fvta_memexqa_amd import nn as fnn
    N, K, T, JQ, w = 2, 2, 12, 5, 64
    g = torch.Generator().manual_seed(5)
    h, C = torch.randn(N, K, T, w, generator=g) * 0.5, torch.rand(N, T, T, generator=g) / T + 0.02
    hq, W, b, _, _ = _att_inputs(N, K, T, JQ, w, 6)
    try:
        Fn.reset_default_graph()
        Fn.variables["attention_2vector/att_logits/W"], Fn.variables["attention_2vector/att_logits/b"] = _cu(W), _cu(b)
        dense, a3 = Fn.attention_3d(_cu(h), _cu(hq), simiMatrix=2, add_tanh=True, time_warp_att=True, C=_cu(C))
        rows, a2 = Fn.attention_3d(_cu(h), _cu(hq), simiMatrix=2, add_tanh=True, time_warp_att=True, C=_cu(C.sum(2)))
        _close(rows, dense, rtol=RTOL, atol=ATOL, msg="h_a")
        assert torch.equal(a2, a3)
        mod = fnn.FocalAttention3D(w, simiMatrix=2, add_tanh=True, seed=1)
        m3, _ = mod(_cu(h), _cu(hq), C=_cu(C))
        m2, _ = mod(_cu(h), _cu(hq), C=_cu(C.sum(2)))
        _close(m2, m3, rtol=RTOL, atol=ATOL, msg="module h_a")
    finally:
        Fn.reset_default_graph()


@pytest.mark.parametrize("warp_type", [1, 2, 3, 4, 5])
def test_time_indication_func(warp_type):
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, T, win = 2, 9, 1.4
    g = torch.Generator().manual_seed(warp_type)
    C, G = torch.randn(N, T, T, generator=g), torch.randn(N, T, T, generator=g)
    band = F.time_indication_band(T, warp_type, win)
    Cc = _cu(C).requires_grad_()
    for _ in range(2):                                                    # the second call reuses the band
        out, wt = Fn.time_indication_func(Cc, warp_type=warp_type, window_t=win)
        np.testing.assert_allclose(out.detach().cpu().numpy(), (C * band[None]).numpy(), rtol=1e-6, atol=0)
    assert (wt == win) if warp_type == 5 else (wt is None)
    out.backward(_cu(G))
    np.testing.assert_allclose(Cc.grad.cpu().numpy(), (G * band[None]).numpy(), rtol=1e-6, atol=0)
