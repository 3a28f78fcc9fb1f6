"""GPU parity of the time warp (model_v2.py:953-1009, closed form) forward and backward vs the oracle
(whose closed form is itself checked against the literal O(T^2) restatement in tests/test_oracle_cross.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# every warp type on: the separate kernels (w = 64), the fused G4 = 1, 2 and 4 (the last with K = TW_KMAX), the fused forward
# G4 = 8 with the separate backward (w = 2048), and K > TW_KMAX at a width the fused kernels would otherwise take
_TW_SHAPES = [(2, 3, 17, 64), (3, 6, 50, 256), (1, 2, 9, 512), (1, 8, 5, 1024), (1, 2, 5, 2048), (1, 9, 5, 256)]
# N T = 2200 > the 2048 wave slots of the fused kernels: some waves run two positions, n = pos / T changes inside a wave's
# stride.  Types 2 and 5 only: 1 / 3 / 4 scale every row by a count of up to 1100, and the tolerance on warp_h would then be
# judging the fp32 rounding of c near zero, not the loop
_TW_CASES = [s + (wt,) for wt in (1, 2, 3, 4, 5) for s in _TW_SHAPES] + [(2, 2, 1100, 256, wt) for wt in (2, 5)]


def _tw_inputs(N, K, T, w, warp_type):
    """hall [N,K,1,T,w], lq, WH_W, WH_b, WC_W [w,1], WC_b, the upstream gradient on warp_h and -- drawn last -- the one on
    scale [N,T] (what the attention hands back under use_time_warp_att)"""
    g = torch.Generator().manual_seed(warp_type * 100 + T)
    hall = torch.randn(N, K, 1, T, w, generator=g) * 0.5
    lq = torch.randn(N, w, generator=g) * 0.5
    WH_W = torch.randn(2 * w, w, generator=g) * (0.3 / w ** 0.5)
    WH_b = torch.randn(w, generator=g) * 0.1
    WC_W = torch.randn(w, 1, generator=g) * (0.5 / w ** 0.5)
    WC_b = torch.randn(1, generator=g) * 0.1
    gout = torch.randn(N, K, 1, T, w, generator=g)
    g2 = torch.randn(N, T, generator=g)
    return (hall, lq, WH_W, WH_b, WC_W, WC_b), gout, g2


@pytest.mark.parametrize("N,K,T,w,warp_type", _TW_CASES)
def test_timewarp_forward_backward(warp_type, N, K, T, w):
    from fvta_memexqa_amd import ops
    from oracle import fvta_fused as F
    (hall, lq, WH_W, WH_b, WC_W, WC_b), gout, _ = _tw_inputs(N, K, T, w, warp_type)
    leaves = [t.double().requires_grad_() for t in (hall, lq, WH_W, WH_b, WC_W, WC_b)]
    ref, c = F.time_warp_closed(*leaves, warp_type=warp_type, window_t=2.3)
    (ref * gout.double()).sum().backward()
    cu = lambda t: t.cuda().contiguous()
    op = ops.TimeWarp(N, K, T, w, warp_type, 2.3)
    hd, lqd, WHd, WHbd, WCd, WCbd = cu(hall.reshape(N, K, T, w)), cu(lq), cu(WH_W), cu(WH_b), cu(WC_W.reshape(-1)), cu(WC_b)
    warp = torch.empty_like(hd)
    op.forward(hd, lqd, WHd, WHbd, WCd, WCbd, warp)
    np.testing.assert_allclose(warp.cpu().numpy(), ref.detach().reshape(N, K, T, w).numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(op.c.cpu().numpy(), c.detach().numpy(), rtol=1e-4, atol=1e-6)
    d_hall = torch.empty_like(hd)
    d_lq = torch.zeros_like(lqd)
    dWH, dWHb, dWC, dWCb = torch.zeros_like(WHd), torch.zeros_like(WHbd), torch.zeros_like(WCd), torch.zeros_like(WCbd)
    op.backward(hd, lqd, WHd, WHbd, WCd, WCbd, cu(gout.reshape(N, K, T, w)), d_hall, d_lq, dWH, dWHb, dWC, dWCb)
    for got, want, name in [(d_hall, leaves[0].grad.reshape(N, K, T, w), "d_hall"), (d_lq, leaves[1].grad, "d_lq"),
                            (dWH, leaves[2].grad, "dWH_W"), (dWHb, leaves[3].grad, "dWH_b"),
                            (dWC, leaves[4].grad.reshape(-1), "dWC_W"), (dWCb, leaves[5].grad, "dWC_b")]:
        wv = want.numpy()
        np.testing.assert_allclose(got.cpu().numpy(), wv, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(wv).max()), err_msg=name)


_TW_GRADS = ("d_hall", "d_lq", "dWH_W", "dWH_b", "dWC_W", "dWC_b")


@functools.lru_cache(maxsize=2)          # (neighbouring cases of one parametrisation share an entry; the long ones are 36 MB a tensor)
def _tw_reference(N, K, T, w, warp_type, window_t, modes, seed_type=None):
    """fp64 oracle on _tw_inputs: warp_h [N,K,T,w], c, scale = c * the band's row sums, and for each of `modes` the six
    gradients (in the kernels' layout) of  <warp_h, gout>  ("warp"),  <scale, g2>  ("scale": what d_scale_att alone
    brings in) or their sum ("both").  Shared between tests: read only."""
    from oracle import fvta_fused as F
    leaves, gout, g2 = _tw_inputs(N, K, T, w, seed_type or warp_type)
    L = [t.double().requires_grad_() for t in leaves]
    warp, c = F.time_warp_closed(*L, warp_type=warp_type, window_t=window_t)
    scale = c * F.time_indication_band(T, warp_type, window_t, torch.float64).sum(1)
    loss = {"warp": (warp * gout.double()).sum(), "scale": (scale * g2.double()).sum()}
    loss["both"] = loss["warp"] + loss["scale"]
    grads = {}
    for m in modes:
        gs = torch.autograd.grad(loss[m], L, retain_graph=True)
        grads[m] = [gs[0].reshape(N, K, T, w), gs[1], gs[2], gs[3], gs[4].reshape(-1), gs[5]]
    return warp.detach().reshape(N, K, T, w), c.detach(), scale.detach(), grads


def _tw_on_device(N, K, T, w, warp_type):
    """_tw_inputs as the kernels take them: the six operands, d_warp and d_scale_att"""
    cu = lambda t: t.cuda().contiguous()
    (hall, lq, WH_W, WH_b, WC_W, WC_b), gout, g2 = _tw_inputs(N, K, T, w, warp_type)
    dev = (cu(hall.reshape(N, K, T, w)), cu(lq), cu(WH_W), cu(WH_b), cu(WC_W.reshape(-1)), cu(WC_b))
    return dev, cu(gout.reshape(N, K, T, w)), cu(g2)


def _tw_forward(N, K, T, w, warp_type, window_t, dev):
    from fvta_memexqa_amd import ops
    op = ops.TimeWarp(N, K, T, w, warp_type, window_t)
    warp = torch.full_like(dev[0], float("nan"))
    op.forward(*dev, warp)
    return op, warp


def _tw_backward(op, dev, d_warp, d_scale_att, prefill=0.0):
    """d_hall (prefilled with NaN: it is stored) and the five accumulated gradients on top of `prefill`"""
    outs = [torch.full_like(dev[0], float("nan"))] + [torch.full_like(t, prefill) for t in dev[1:]]
    op.backward(*dev, d_warp, *outs, d_scale_att=d_scale_att)
    return outs


def _tw_check_forward(op, warp, ref, tag):
    np.testing.assert_allclose(warp.cpu().numpy(), ref[0].numpy(), rtol=1e-4, atol=1e-5, err_msg=tag + ": warp_h")
    np.testing.assert_allclose(op.c.cpu().numpy(), ref[1].numpy(), rtol=1e-4, atol=1e-6, err_msg=tag + ": c")
    np.testing.assert_allclose(op.scale.cpu().numpy(), ref[2].numpy(), rtol=1e-4, atol=1e-5, err_msg=tag + ": scale")


def _tw_check_grads(outs, want, tag, on_top_of=0.0):
    for got, ref, name in zip(outs, want, _TW_GRADS):
        wv = ref.numpy()
        assert bool(torch.isfinite(got).all()), "%s: %s is not finite" % (tag, name)
        np.testing.assert_allclose(got.cpu().numpy(), wv + (0.0 if name == "d_hall" else on_top_of), rtol=2e-4,
                                   atol=2e-5 * max(1.0, np.abs(wv).max()), err_msg="%s: %s" % (tag, name))
    w = outs[2].shape[1]
    assert bool((outs[2][w:] == on_top_of).all()), "%s: rows w..2w of dWH_W see a zero feature and are never touched" % tag


def _tw_same_bits(a, b, tag, names=("warp_h", "c", "scale") + _TW_GRADS):
    for x, y, name in zip(a, b, names):
        assert x.dtype == torch.float32 and torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: %s" % (tag, name)


# Every loop of the kernels past its first round.  Types 2 and 5 only, as for the long case above.
#   (3,3,300,64)    separate kernels: 2700 rows > the 2048 workgroups of tw_apply_bwd_kernel (n changes inside a workgroup's stride, dvacc
#                   carries over two rows), four blocks of tw_dz_kernel, T > 256 in tw_reduce_kernel's dsq
#   (1,9,250,256)   K > TW_KMAX at a fused width: the separate kernels at w = 256, 2250 rows
#   (2,1,1100,2048) the G4 = 8 forward past its 2048 wave slots; the separate backward with both rounds of c0 += 1024, 2200 rows
#   (2,2,1100,512), (2,2,1100,1024)   G4 = 2 and 4, forward and backward, past the wave slots
_TW_LONG = [(3, 3, 300, 64), (1, 9, 250, 256), (2, 1, 1100, 2048), (2, 2, 1100, 512), (2, 2, 1100, 1024)]


@pytest.mark.parametrize("N,K,T,w,warp_type,att", [s + (wt, att) for s in _TW_LONG for wt in (2, 5) for att in (False, True)])
def test_timewarp_loops_past_one_round(N, K, T, w, warp_type, att):
    ref = _tw_reference(N, K, T, w, warp_type, 2.3, ("warp", "both"))
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, warp_type)
    op, warp = _tw_forward(N, K, T, w, warp_type, 2.3, dev)
    _tw_check_forward(op, warp, ref, "forward")
    outs = _tw_backward(op, dev, d_warp, g2 if att else None)
    _tw_check_grads(outs, ref[3]["both" if att else "warp"], "backward with d_scale_att" if att else "backward")


# N > 256: the second round of n += 256 in tw_param_bwd_kernel (dWC_W and d_lq [N,w] are what it feeds), o past w + 256 in
# tw_vec_kernel, w + N blocks of tw_reduce_kernel
@pytest.mark.parametrize("N,K,T,w,warp_type", [s + (wt,) for s in [(300, 1, 3, 64), (260, 2, 2, 256)] for wt in (1, 2, 3, 4, 5)])
def test_timewarp_many_questions(N, K, T, w, warp_type):
    ref = _tw_reference(N, K, T, w, warp_type, 2.3, ("both",))
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, warp_type)
    op, warp = _tw_forward(N, K, T, w, warp_type, 2.3, dev)
    _tw_check_forward(op, warp, ref, "N = %d" % N)
    _tw_check_grads(_tw_backward(op, dev, d_warp, g2), ref[3]["both"], "N = %d" % N)


@pytest.mark.parametrize("N,K,T,w,warp_type",
                         [s + (wt,) for s in [(2, 3, 17, 256), (1, 2, 9, 512), (1, 8, 5, 1024)] for wt in (1, 2, 3, 4, 5)])
def test_timewarp_scale_gradient_through_the_fused_backward(N, K, T, w, warp_type):
    """d_scale_att enters tw_bwd_fused_kernel (G4 = 1, 2, 4) in a line of its own.  The second run has it as the ONLY upstream
    gradient (d_warp = 0: d_hall is 2 v h dz alone), so its sign and scale cannot hide behind the larger row term."""
    ref = _tw_reference(N, K, T, w, warp_type, 2.3, ("both", "scale"))
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, warp_type)
    op, warp = _tw_forward(N, K, T, w, warp_type, 2.3, dev)
    _tw_check_forward(op, warp, ref, "forward")
    _tw_check_grads(_tw_backward(op, dev, d_warp, g2), ref[3]["both"], "upstream on warp_h and scale")
    _tw_check_grads(_tw_backward(op, dev, torch.zeros_like(d_warp), g2), ref[3]["scale"], "upstream on scale only")


# tw_count at its edges, on the separate and the fused kernels: a single position (every count is 1), and for the band a window
# of 0 (the diagonal), an integer window (ceil must not add one) and one wider than the sequence (both ends clamp at every t)
_TW_EDGES = [(2, 2, 1, w, wt, 2.3) for w in (64, 256) for wt in (1, 2, 3, 4, 5)] + \
            [(2, 2, 6, w, 5, win) for w in (64, 256) for win in (0.0, 1.0, 7.5)]


@pytest.mark.parametrize("N,K,T,w,warp_type,window_t", _TW_EDGES)
def test_timewarp_count_edges(N, K, T, w, warp_type, window_t):
    ref = _tw_reference(N, K, T, w, warp_type, window_t, ("both",))
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, warp_type)
    op, warp = _tw_forward(N, K, T, w, warp_type, window_t, dev)
    _tw_check_forward(op, warp, ref, "window %g" % window_t)
    _tw_check_grads(_tw_backward(op, dev, d_warp, g2), ref[3]["both"], "window %g" % window_t)


@pytest.mark.parametrize("w", [64, 256])
@pytest.mark.parametrize("window_t,same_as", [(0.0, 2), (7.5, 1)])
def test_timewarp_band_at_its_ends_is_the_diagonal_and_all_time(window_t, same_as, w):
    """On T = 6 the band of window 0.0 counts what type 2 counts and the band of window 7.5 what type 1 counts: equal floats into
    the same arithmetic, so warp_h, c, scale and every gradient have the same bits."""
    N, K, T = 2, 2, 6
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, 5)
    runs = []
    for warp_type, win in ((5, window_t), (same_as, 2.3)):
        op, warp = _tw_forward(N, K, T, w, warp_type, win, dev)
        runs.append([warp, op.c, op.scale] + _tw_backward(op, dev, d_warp, g2))
    _tw_same_bits(runs[0], runs[1], "type 5 with window %g against type %d" % (window_t, same_as))


# What the kernels' comments promise, one shape per path: the separate kernels past one round, the fused G4 = 1, 2, 4, and
# w = 2048 (fused forward, separate backward).  Type 5 with d_scale_att.
_TW_PATHS = [(3, 3, 300, 64), (2, 3, 17, 256), (1, 2, 9, 512), (1, 8, 5, 1024), (1, 2, 5, 2048)]


def _tw_plain_run(N, K, T, w):
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, 5)
    op, warp = _tw_forward(N, K, T, w, 5, 2.3, dev)
    return dev, d_warp, g2, op, [warp, op.c, op.scale] + _tw_backward(op, dev, d_warp, g2)


@pytest.mark.parametrize("N,K,T,w", _TW_PATHS)
def test_timewarp_backward_owes_nothing_to_the_workspace(N, K, T, w):
    """The backward recomputes v, s0 and sq, and every wave slot or workgroup stores its dv partials -- those without work
    zeros: with the workspace overwritten by 0xFF bytes (NaN to any reader) after the forward, and again before a second
    backward, every output has the bits of the run that left the workspace alone."""
    dev, d_warp, g2, _, plain = _tw_plain_run(N, K, T, w)
    op, warp = _tw_forward(N, K, T, w, 5, 2.3, dev)
    for which in ("first", "second"):
        op.work.view(torch.uint8).fill_(0xFF)
        _tw_same_bits([warp, op.c, op.scale] + _tw_backward(op, dev, d_warp, g2), plain, which + " backward on a refilled workspace")


@pytest.mark.parametrize("N,K,T,w", _TW_PATHS)
def test_timewarp_backward_is_repeatable(N, K, T, w):
    """no atomics anywhere: fixed partial sums folded in a fixed order"""
    dev, d_warp, g2, op, plain = _tw_plain_run(N, K, T, w)
    _tw_same_bits(_tw_backward(op, dev, d_warp, g2), plain[3:], "a second backward", _TW_GRADS)


@pytest.mark.parametrize("N,K,T,w", _TW_PATHS)
def test_timewarp_backward_stores_d_hall_and_accumulates_the_rest(N, K, T, w):
    """d_hall comes back finite from a NaN prefill; d_lq and the four parameter gradients come back as prefill + gradient, rows
    w..2w of dWH_W as the prefill exactly"""
    ref = _tw_reference(N, K, T, w, 5, 2.3, ("both",))
    dev, d_warp, g2 = _tw_on_device(N, K, T, w, 5)
    op, _ = _tw_forward(N, K, T, w, 5, 2.3, dev)
    _tw_check_grads(_tw_backward(op, dev, d_warp, g2, prefill=0.5), ref[3]["both"], "on top of 0.5", on_top_of=0.5)


def test_unknown_warp_type_raises_like_the_reference():
    from fvta_memexqa_amd import ops
    with pytest.raises(Exception, match="time warping type not implemented"):
        ops.TimeWarp(1, 1, 4, 64, 9)


def _close(a, b, rtol=1e-4, atol=1e-5):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale)


def _tw_att_case(seed, N, K, T, JQ, w, simi, tanh, neg_scale, ties, all_masked_k=None):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, K, T, w, generator=g) * 0.5
    q = torch.randn(N, JQ, w, generator=g) * 0.5
    F_ = {1: 3, 2: 2, 3: 4}[simi]
    W = torch.randn(F_ * w, 1, generator=g) * 0.1
    b = torch.randn(1, generator=g) * 0.1
    lens = torch.randint(1, T + 1, (N, K), generator=g)
    hm = torch.arange(T)[None, None, :] < lens[:, :, None]
    if all_masked_k is not None:
        hm[:, all_masked_k] = False
    qm = torch.arange(JQ)[None, :] < torch.randint(1, JQ + 1, (N,), generator=g)[:, None]
    scale = torch.rand(N, T, generator=g) * 1.5 + 0.2
    if neg_scale:
        scale = torch.where(torch.rand(N, T, generator=g) < 0.4, -scale, scale)
    if ties:                       # the rows that are padding for every k share one scale (same c[n,t], same count)
        allpad = ~hm.any(1)
        scale = torch.where(allpad, torch.full_like(scale, -2.37), scale)
        # ... and, as in the model, they are zero rows (LSTM outputs past the length; the warp keeps zeros zero).  With
        # non-zero tied rows TF also pushes gradient through the MASKED logits (DESIGN.md deviation (b)), which the
        # kernels do not; partially padded positions keep random values (their scales differ: one winner, d z = 0)
        h = h * (~allpad)[:, None, :, None]
    return h, q, W, b, hm, qm, scale


@pytest.mark.parametrize("N,K,T,JQ,w,simi,tanh,neg,ties,amk", [
    (3, 3, 40, 5, 64, 2, True, False, False, None), (3, 3, 40, 5, 64, 2, True, True, False, None),
    (4, 2, 70, 7, 128, 1, False, True, True, None), (2, 4, 300, 30, 256, 3, True, True, True, 1),
    (2, 6, 1200, 30, 1024, 2, True, True, True, None)])
def test_attention_3d_time_warp_att_forward_backward(N, K, T, JQ, w, simi, tanh, neg, ties, amk):
    """fvta_attn_fwd_tw / fvta_attn_bwd_tw against the fp64 oracle: positive scales, negative scales on masked rows
    (they take the softmax), tied masked rows, a fully masked modality; h_a, and the gradients w.r.t. hinfo, hq, W, b
    and the scale itself."""
    from fvta_memexqa_amd import ops
    from oracle import fvta_fused as F
    h, q, W, b, hm, qm, scale = _tw_att_case(N * 7 + T, N, K, T, JQ, w, simi, tanh, neg, ties, amk)
    leaves = [t.double().requires_grad_() for t in (h, q, W, b, scale)]
    C = torch.diag_embed(leaves[4])                                       # [N,T,T] with row sums = scale
    ref, _ = F.attention_3d(leaves[0], leaves[1], leaves[2], leaves[3], hm, qm, simiMatrix=simi, add_tanh=tanh,
                            time_warp_att=True, C=C)
    gout = torch.randn(N, w, generator=torch.Generator().manual_seed(5)).double()
    (ref * gout).sum().backward()
    op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
    cu = lambda t: t.float().cuda().contiguous()
    hd, qd, Wd, bd, sd = cu(h), cu(q), cu(W).reshape(-1), cu(b), cu(scale)
    hmd, qmd = ops.as_mask_u8(hm).cuda(), ops.as_mask_u8(qm).cuda()
    ha, _ = op.forward(hd, qd, hmd, qmd, Wd, bd, tscale=sd)
    _close(ha, ref.detach(), rtol=1e-4, atol=2e-5)
    d_h, d_q = torch.empty_like(hd), torch.empty_like(qd)
    dW, db, dsc = torch.zeros_like(Wd), torch.zeros_like(bd), torch.zeros_like(sd)
    op.backward(hd, qd, hmd, qmd, Wd, bd, cu(gout), d_h, d_q, dW, db, accumulate=0, tscale=sd, d_tscale=dsc)
    _close(d_h, leaves[0].grad, rtol=2e-4, atol=2e-5)
    _close(d_q, leaves[1].grad, rtol=2e-4, atol=2e-5)
    _close(dW, leaves[2].grad.reshape(-1), rtol=2e-4, atol=2e-5)
    _close(db, leaves[3].grad, rtol=2e-4, atol=2e-5)
    # d scale: rows that take the whole softmax carry 0 * 1e30-scale terms; compare where the oracle's is finite and sane
    gs = leaves[4].grad
    ok = gs.abs() < 1e6
    _close(dsc.cpu().double()[ok], gs[ok], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("warp_type", [1, 5])
def test_model_with_time_warp_att(warp_type):
    """--use_time_warp --use_time_warp_att through the Model: forward and every parameter gradient vs the oracle."""
    from fvta_memexqa_amd.model_v2 import Model
    from fvta_memexqa_amd.synth import SynthSpec, make_inputs, make_params, to_dtype
    from oracle import fvta_fused as F
    spec = SynthSpec(N=3, A=2, P=3, S=2, L=5, d=32, SA=1, dense=False, text_in=12, img_in=8)
    params, inputs = make_params(spec), make_inputs(spec)
    g = torch.Generator().manual_seed(17)
    w = spec.w
    params.update(WH_W=torch.randn(2 * w, w, generator=g) * 0.05, WH_b=torch.randn(w, generator=g) * 0.05,
                  WC_W=torch.randn(w, 1, generator=g) * 0.1, WC_b=torch.randn(1, generator=g) * 0.05)
    cfg = dict(spec.cfg(), use_time_warp=True, use_time_warp_att=True, warp_type=warp_type, window_t=1.4)
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    ref = F.fvta_forward(dict(p64, window_t=1.4), to_dtype(inputs, torch.float64), cfg)
    ref["loss"].backward()
    assert (ref["c_warp"] < 0).any()
    model = Model(dict(cfg, batch_size=spec.N), text_in=spec.text_in, img_in=spec.img_in)
    model.set_oracle_params(params)
    L = model.load_inputs(inputs, training=True)
    model.zero_grad()
    yp = model.forward(L)
    model.backward(L)
    d, dp = model.d, model.dp
    unpad = lambda t: torch.cat([t[..., :d], t[..., dp:dp + d]], -1)
    _close(unpad(L.g1), ref["g1_all"].detach(), rtol=1e-4, atol=2e-5)
    _close(yp, ref["yp"].detach(), rtol=1e-4, atol=1e-5)
    grads = model.get_oracle_grads()
    for k, v in p64.items():
        if v.grad is not None:
            _close(torch.from_numpy(grads[k]).reshape(v.grad.shape), v.grad, rtol=2e-4, atol=2e-5)
    with pytest.raises(NameError):
        Model(dict(spec.cfg(), use_time_warp_att=True, batch_size=spec.N), text_in=spec.text_in, img_in=spec.img_in)


# (the last case: N T = 4200 > the 4096 waves of the shadow forward, two to three positions per wave in the shadow backward;
#  the last positions of a wave's stride take the clamped table prefetch; K = 1: every lane >= 2 of the table load re-reads an
#  entry; (1,8,5,1024): the heaviest instantiation, G4 = 4 with all TW_KMAX streams)
@pytest.mark.parametrize("N,K,T,w,warp_type",
                         [s + (wt,) for wt in (1, 3, 5) for s in [(2, 3, 17, 512), (3, 6, 50, 1024), (1, 8, 9, 512), (2, 1, 9, 512),
                                                                  (1, 8, 5, 1024)]] +
                         [(2, 3, 2100, 512, 5)])
def test_timewarp_over_shadow_rows(warp_type, N, K, T, w):
    """fvta_timewarp_fwd_shadow / _bwd_shadow (the bf16 engine: the context tensor is never stored in fp32) against the
    fp32-row kernels on the SAME bf16-valued rows: c / scale equal, the warped rows = bf16 of the fp32 kernel's, and every
    gradient equal up to summation order; rows whose table entries point at the shared zero half-row are zero rows."""
    from fvta_memexqa_amd import ops
    from tests.test_gpu_shadow import _shadow_table
    g = torch.Generator().manual_seed(warp_type * 10 + T + w)
    hb = (torch.randn(N * K * T, w, generator=g) * 0.5).clamp(-1, 1).bfloat16().cuda()
    zero_rows = torch.arange(0, N * K * T, 7, device="cuda")
    hb[zero_rows] = 0
    table, keep = _shadow_table(hb, zero_rows, warp_type + T)
    h32 = hb.float().view(N, K, T, w).contiguous()
    cu = lambda t: t.cuda().contiguous()
    lq = cu(torch.randn(N, w, generator=g) * 0.5)
    WH = cu(torch.randn(2 * w, w, generator=g) * (0.3 / w ** 0.5))
    WHb = cu(torch.randn(w, generator=g) * 0.1)
    WC = cu(torch.randn(w, generator=g) * (0.5 / w ** 0.5))
    WCb = cu(torch.randn(1, generator=g) * 0.1)
    ref_op, op = ops.TimeWarp(N, K, T, w, warp_type, 2.3), ops.TimeWarp(N, K, T, w, warp_type, 2.3)
    warp32 = torch.empty_like(h32)
    ref_op.forward(h32, lq, WH, WHb, WC, WCb, warp32)
    warp_b = torch.full((N * K * T, w), 7.0, dtype=torch.bfloat16, device="cuda")
    op.forward_shadow(table, lq, WH, WHb, WC, WCb, warp_b)
    np.testing.assert_allclose(op.c.cpu().numpy(), ref_op.c.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(op.scale.cpu().numpy(), ref_op.scale.cpu().numpy(), rtol=1e-5, atol=1e-6)
    # bf16 of the same product (c differs in the last fp32 bits between the two reductions: allow one bf16 ulp)
    np.testing.assert_allclose(warp_b.float().cpu().numpy(), warp32.view(-1, w).bfloat16().float().cpu().numpy(), rtol=2.0 ** -7, atol=1e-30)
    assert float(warp_b[zero_rows].float().abs().max()) == 0.0
    d_warp = cu(torch.randn(N, K, T, w, generator=g))
    outs = []
    for which in (0, 1):
        d_hall = torch.full_like(h32, float("nan"))
        d_lq = torch.zeros_like(lq)
        grads = [torch.zeros_like(WH), torch.zeros_like(WHb), torch.zeros_like(WC), torch.zeros_like(WCb)]
        if which == 0:
            ref_op.backward(h32, lq, WH, WHb, WC, WCb, d_warp, d_hall, d_lq, *grads)
        else:
            op.backward_shadow(table, lq, WH, WHb, WC, WCb, d_warp, d_hall, d_lq, *grads)
        outs.append([d_hall, d_lq] + grads)
    for a, b, name in zip(outs[1], outs[0], ("d_hall", "d_lq", "dWH_W", "dWH_b", "dWC_W", "dWC_b")):
        assert torch.isfinite(a).all(), name
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-5 * max(1.0, float(b.abs().max())), err_msg=name)


# (warp types 1 / 3 / 5 of the kernels themselves: test_timewarp_over_shadow_rows.  At the model level only the published type:
#  type 1 scales every row by T, the attention's tanh saturates, and two bf16 runs a rounding apart no longer agree in the
#  warp's own -- vanishing -- parameter gradients)
@pytest.mark.parametrize("cfgname,N,warp_type", [("plumbing_w512", None, 5), ("metric", 2, 5)])
def test_model_time_warp_on_shadow_rows_is_the_same_train_step(cfgname, N, warp_type):
    """--use_time_warp under precision = bf16 with and without shadow rows (the published flag set's regime): the warp and the
    attention read the encoders' bf16 rows instead of an fp32 context tensor -- yp / loss within the bf16 engine's tolerance of
    the plain bf16 run, every gradient within a few percent (relative L2), the vis tensors hall / warp_h served on demand."""
    from fvta_memexqa_amd.model_v2 import Model
    from fvta_memexqa_amd.synth import CONFIGS, SynthSpec, make_inputs, make_params
    cfg = dict(CONFIGS["plumbing"], d=256) if cfgname == "plumbing_w512" else dict(CONFIGS[cfgname])
    if N:
        cfg["N"] = N
    spec = SynthSpec(dense=False, **cfg)
    params, inputs = make_params(spec), make_inputs(spec)
    g = torch.Generator().manual_seed(17)
    w = spec.w
    params.update(WH_W=torch.randn(2 * w, w, generator=g) * (0.3 / w ** 0.5), WH_b=torch.randn(w, generator=g) * 0.05,
                  WC_W=torch.randn(w, 1, generator=g) * (0.5 / w ** 0.5), WC_b=torch.randn(1, generator=g) * 0.05)
    res = {}
    for shadow in (False, True):
        model = Model(dict(spec.cfg(), batch_size=spec.N, precision="bf16", shadow_rows=shadow, use_time_warp=True,
                           warp_type=warp_type, window_t=2.4), text_in=spec.text_in, img_in=spec.img_in)
        model.set_oracle_params(params)
        L = model.load_inputs(inputs, training=True)
        assert L.shadow == shadow
        model.zero_grad()
        yp = model.forward(L).cpu().double()
        model.backward(L, need_dx=True)
        grads = {k: torch.from_numpy(np.asarray(v)).double() for k, v in model.get_oracle_grads().items()}
        res[shadow] = dict(yp=yp, loss=model.loss.cpu().double(), grads=grads, hall=model.hall.clone(), warp=model.warp_h.clone(),
                           c=model.C.clone())
        model.forward(L, want_logits=True)
        res[shadow]["yp2"] = model.yp.cpu().double()
    a, b = res[True], res[False]
    assert torch.equal(a["hall"], b["hall"].bfloat16().float()), "hall"
    np.testing.assert_allclose(a["c"].cpu().numpy(), b["c"].cpu().numpy(), rtol=0, atol=2e-2)
    np.testing.assert_allclose(a["warp"].cpu().numpy(), b["warp"].cpu().numpy(), rtol=3e-2, atol=3e-2 * float(b["warp"].abs().max()))
    np.testing.assert_allclose(a["yp"].numpy(), b["yp"].numpy(), rtol=0, atol=1e-2)
    np.testing.assert_allclose(a["yp2"].numpy(), a["yp"].numpy(), rtol=0, atol=1e-3)
    np.testing.assert_allclose(a["loss"].numpy(), b["loss"].numpy(), rtol=0, atol=1e-2)
    for k, gb in b["grads"].items():
        ga = a["grads"][k]
        if float(gb.norm()) < 1e-6:
            assert float(ga.abs().max()) < 1e-5, k
            continue
        err = float((ga - gb).norm() / (gb.norm() + 1e-30))
        # (the attention logits' parameters hang off arg-max positions, and the warp's off a tanh of sums over every row)
        assert err < (0.3 if (k.startswith("att_") or k.startswith("W")) else 5e-2), "grad %s: relative L2 %.4f" % (k, err)
