"""GPU parity of the autograd layer (fvta_memexqa_amd/autograd.py, functional.py, nn.py) and of the two kernels it adds
(fvta_attn_cube_bwd, fvta_softsel_bwd): gradients vs torch autograd on the fp64 fused oracle.

Inputs are continuous random, so the oracle's max over the question has no exact tie (tests/test_autograd_host.py checks
that for the seeds used here), and every (n,k) of an `h_a` case keeps at least one valid row: the two places where the
kernels deviate from TensorFlow's gradient on purpose are not touched.

Tolerances: the exact-fp32 class of DESIGN.md section 2 / tests/test_gpu_backward.py -- rtol 1e-4, atol 2e-5 x
max(1, max|ref|); bf16x3 2e-4 / 5e-5; bf16 4e-2 relative L2 per gradient tensor.
"""
import ctypes
import functools

import pytest
import torch

from tests.test_gpu_backward import _close
from tests.test_gpu_forward import _att_case

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def _dbl(*ts):
    return [None if t is None else t.double().requires_grad_() for t in ts]


# ------------------------------------------------------------------ 1. the cube gradient through the C ABI
CUBE_SHAPES = [(2, 3, 50, 10, 64), (2, 6, 333, 30, 1024), (1, 2, 70, 60, 2048), (2, 1, 1100, 5, 128), (3, 2, 16, 1, 256)]


def cube_case(N, K, T, JQ, w, simi, tanh, masked):
    h, q, W, b, hm, qm = _att_case(N, K, T, JQ, w, simi, tanh, masked, seed=N * 1000 + T + w + 7 * simi + 3)
    G = torch.randn(N, K, T, JQ, generator=torch.Generator().manual_seed(T + JQ))      # every entry, masked ones included
    return h, q, W, b, hm, qm, G


@pytest.mark.parametrize("N,K,T,JQ,w", CUBE_SHAPES)
@pytest.mark.parametrize("simi,tanh", [(1, False), (2, True), (3, True)])
@pytest.mark.parametrize("masked", [True, False])
def test_attn_cube_bwd_matches_autograd(N, K, T, JQ, w, simi, tanh, masked):
    """dA random on every entry (the masked case has a fully masked (n,k): _att_case masks hinfo[0,0]); accumulate 0 over
    7.0, accumulate 1 on top of ones, and a second run bitwise equal to the first."""
    from fvta_memexqa_amd import _lib
    from fvta_memexqa_amd._lib import AttnDesc, check, ptr, stream_ptr
    from oracle import fvta_fused as F
    h, q, W, b, hm, qm, G = cube_case(N, K, T, JQ, w, simi, tanh, masked)
    if masked:
        assert not bool(hm[0, 0].any())
    hd, qd, Wd, bd = _dbl(h, q, W, b)
    _, a = F.attention_3d(hd, qd, Wd, bd, hm, qm, simiMatrix=simi, add_tanh=tanh)
    a.backward(G.double())

    lib = _lib.load()
    desc = AttnDesc(N, K, T, JQ, w, simi, 0, int(tanh), 0)
    nb = lib.fvta_attn_cube_bwd_workspace_bytes(ctypes.byref(desc))
    assert nb > 0
    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
    hc, qc, Wc, bc, Gc = _cu(h), _cu(q), _cu(W.reshape(-1)), _cu(b), _cu(G)

    def run(dh, dq, dW, db, acc):
        check(lib.fvta_attn_cube_bwd(ctypes.byref(desc), ptr(hc), ptr(qc), ptr(Wc), ptr(bc), ptr(Gc), ptr(dh), ptr(dq),
                                     ptr(dW), ptr(db), acc, ptr(work), stream_ptr()), "fvta_attn_cube_bwd")

    dh, dq = torch.full_like(hc, 7.0), torch.full_like(qc, 7.0)
    dW, db = torch.zeros_like(Wc), torch.zeros(1, device="cuda")
    run(dh, dq, dW, db, 0)
    _close(dh, hd.grad, rtol=RTOL, atol=ATOL, msg="d_hinfo")
    _close(dq, qd.grad, rtol=RTOL, atol=ATOL, msg="d_hq")
    _close(dW, Wd.grad.reshape(-1), rtol=RTOL, atol=ATOL, msg="dW")
    _close(db, bd.grad, rtol=RTOL, atol=ATOL, msg="db")
    dh2, dq2 = torch.full_like(hc, float("nan")), torch.full_like(qc, float("nan"))
    dW2, db2 = torch.zeros_like(Wc), torch.zeros(1, device="cuda")
    run(dh2, dq2, dW2, db2, 0)
    for x, y in ((dh, dh2), (dq, dq2), (dW, dW2), (db, db2)):
        assert torch.equal(x, y), "two runs differ"
    dh3, dq3 = torch.ones_like(hc), torch.ones_like(qc)
    run(dh3, dq3, dW, db, 1)
    _close(dh3 - 1.0, hd.grad, rtol=RTOL, atol=ATOL, msg="d_hinfo accumulate")
    _close(dq3 - 1.0, qd.grad, rtol=RTOL, atol=ATOL, msg="d_hq accumulate")
    _close(dW, 2 * Wd.grad.reshape(-1), rtol=RTOL, atol=ATOL, msg="dW accumulates")
    _close(db, 2 * bd.grad, rtol=RTOL, atol=ATOL, msg="db accumulates")


def test_attn_cube_bwd_hinfo_stride_is_the_dense_call_on_a_stream_of_an_arena():
    """K = 1 with desc.hinfo_stride: the rows of one stream inside a wider [N][all streams' rows] arena; the same bits as
    the dense call, and nothing outside the stream is written"""
    from fvta_memexqa_amd import _lib
    from fvta_memexqa_amd._lib import AttnDesc, check, ptr, stream_ptr
    N, T, JQ, w, lead, tail = 2, 40, 6, 64, 5, 3
    h, q, W, b, _, _, G = cube_case(N, 1, T, JQ, w, 2, True, False)
    lib = _lib.load()
    hc, qc, Wc, bc, Gc = _cu(h), _cu(q), _cu(W.reshape(-1)), _cu(b), _cu(G)
    arena = torch.randn(N, lead + T + tail, w, device="cuda")
    arena[:, lead:lead + T] = hc[:, 0]
    outs = []
    for stride in (0, (lead + T + tail) * w):
        desc = AttnDesc(N, 1, T, JQ, w, 2, 0, 1, stride)
        work = torch.empty(lib.fvta_attn_cube_bwd_workspace_bytes(ctypes.byref(desc)), dtype=torch.uint8, device="cuda")
        src = arena[:, lead:] if stride else hc
        dh = torch.full_like(arena, 7.0) if stride else torch.empty_like(hc)
        dq, dW, db = torch.empty_like(qc), torch.zeros_like(Wc), torch.zeros(1, device="cuda")
        dst = dh[:, lead:] if stride else dh
        check(lib.fvta_attn_cube_bwd(ctypes.byref(desc), ptr(src), ptr(qc), ptr(Wc), ptr(bc), ptr(Gc), ptr(dst), ptr(dq),
                                     ptr(dW), ptr(db), 0, ptr(work), stream_ptr()), "fvta_attn_cube_bwd")
        outs.append((dh, dq, dW, db))
    (dh0, dq0, dW0, db0), (dh1, dq1, dW1, db1) = outs
    assert torch.equal(dh1[:, lead:lead + T], dh0[:, 0])
    assert torch.equal(dq0, dq1) and torch.equal(dW0, dW1) and torch.equal(db0, db1)
    assert float((dh1[:, :lead] - 7.0).abs().max()) == 0.0 and float((dh1[:, lead + T:] - 7.0).abs().max()) == 0.0


# ------------------------------------------------------------------ 2. softsel
@pytest.mark.parametrize("lead,J,d,masked_row", [((3, 2), 7, 33, False), ((5,), 300, 256, True), ((2, 3, 4), 1, 5, False)])
def test_softsel_backward(lead, J, d, masked_row):
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    g = torch.Generator().manual_seed(J + d)
    target = torch.randn(*lead, J, d, generator=g)
    logits = torch.randn(*lead, J, generator=g) * 2
    mask = torch.ones(*lead, J, dtype=torch.bool)
    if masked_row:
        mask[0] = False                         # a fully exp-masked row: uniform weights
        mask[1, J // 2:] = False
    gout = torch.randn(*lead, d, generator=g)
    td, ld = _dbl(target, logits)
    ref = F.softsel(td, F.exp_mask(ld, mask))
    ref.backward(gout.double())
    tc, lc = _cu(target).requires_grad_(), _cu(logits).requires_grad_()
    out = Fn.softsel(tc, Fn.exp_mask(lc, mask.cuda()))
    assert out.grad_fn is not None
    _close(out, ref, rtol=RTOL, atol=ATOL, msg="softsel")
    out.backward(_cu(gout))
    _close(tc.grad, td.grad, rtol=RTOL, atol=ATOL, msg="d_target")
    _close(lc.grad, ld.grad, rtol=RTOL, atol=ATOL, msg="d_logits")


# ------------------------------------------------------------------ 3. attention_3d / attention under autograd
def att_case(N, K, T, JQ, w, simi, tanh, masked, seed):
    """_att_case with every (n,k) keeping a valid row and every batch row a valid question position"""
    h, q, W, b, hm, qm = _att_case(N, K, T, JQ, w, simi, tanh, masked, seed=seed)
    if masked:
        hm[0, 0, :3] = True
        if N > 1:
            qm[N - 1, :2] = True
    return h, q, W, b, hm, qm


ATT_CASES = {                       # name -> (N, K, T, JQ, w, simi, tanh, masked, seed)
    "plain": (2, 3, 50, 10, 64, 1, False, True, 11),
    "tanh_w100": (2, 2, 40, 7, 100, 2, True, True, 12),
    "timewarp": (2, 2, 24, 5, 64, 3, False, False, 13),
    "cosine": (2, 2, 30, 6, 64, 4, False, True, 14),
    "bidirect": (2, 1, 20, 6, 64, 1, False, True, 15),
}


def _set_att_vars(Fn, W, b, scope="attention_2vector"):
    Fn.reset_default_graph()
    if W is None:
        return None, None
    Wc, bc = _cu(W).requires_grad_(), _cu(b).requires_grad_()
    Fn.variables["%s/att_logits/W" % scope] = Wc
    Fn.variables["%s/att_logits/b" % scope] = bc
    return Wc, bc


def _grads(ts):
    return [None if t is None else t.grad for t in ts]


@pytest.mark.parametrize("which", ["both", "h_a", "a"])
@pytest.mark.parametrize("name", ["plain", "tanh_w100"])
def test_attention_3d_autograd(name, which):
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, K, T, JQ, w, simi, tanh, masked, seed = ATT_CASES[name]
    h, q, W, b, hm, qm = att_case(*ATT_CASES[name])
    g = torch.Generator().manual_seed(seed)
    G1, G2 = torch.randn(N, w, generator=g), torch.randn(N, K, T, JQ, generator=g)
    leaves = _dbl(h, q, W, b)
    ra, rl = F.attention_3d(*leaves, hm, qm, simiMatrix=simi, add_tanh=tanh)
    outs, gs = {"both": ([ra, rl], [G1, G2]), "h_a": ([ra], [G1]), "a": ([rl], [G2])}[which]
    torch.autograd.backward(outs, [x.double() for x in gs])
    hc, qc = _cu(h).requires_grad_(), _cu(q).requires_grad_()
    Wc, bc = _set_att_vars(Fn, W, b)
    try:
        ha, a = Fn.attention_3d(hc, qc, _cu(hm), _cu(qm), simiMatrix=simi, add_tanh=tanh)
        assert ha.grad_fn is not None and a.grad_fn is not None
        _close(ha, ra, rtol=RTOL, atol=ATOL, msg="h_a")
        outs, gs = {"both": ([ha, a], [G1, G2]), "h_a": ([ha], [G1]), "a": ([a], [G2])}[which]
        torch.autograd.backward(outs, [_cu(x) for x in gs])
        for got, ref, nm in zip(_grads([hc, qc, Wc, bc]), _grads(leaves), ("d_hinfo", "d_hq", "dW", "db")):
            _close(got, ref, rtol=RTOL, atol=ATOL, msg=nm)
    finally:
        Fn.reset_default_graph()


def test_attention_3d_without_grad_is_the_plain_call():
    """nothing requires grad: no grad_fn, and the outputs are bit for bit those of the handle called directly and those of
    the call that does record a graph"""
    from fvta_memexqa_amd import functional as Fn, ops
    N, K, T, JQ, w, simi, tanh, masked, seed = ATT_CASES["plain"]
    h, q, W, b, hm, qm = att_case(*ATT_CASES["plain"])
    hc, qc = _cu(h), _cu(q)
    Wc, bc = _set_att_vars(Fn, W, b)
    try:
        Wc.requires_grad_(False), bc.requires_grad_(False)
        ha, a = Fn.attention_3d(hc, qc, _cu(hm), _cu(qm), simiMatrix=simi, add_tanh=tanh)
        assert ha.grad_fn is None and a.grad_fn is None and not ha.requires_grad and not a.requires_grad
        op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
        ha0, a0 = op.forward(hc, qc, _cu(ops.as_mask_u8(hm)), _cu(ops.as_mask_u8(qm)), Wc.reshape(-1).contiguous(), bc,
                             want_logits=True)
        assert torch.equal(ha, ha0) and torch.equal(a, a0)
        ha1, a1 = Fn.attention_3d(hc.clone().requires_grad_(), qc, _cu(hm), _cu(qm), simiMatrix=simi, add_tanh=tanh)
        assert ha1.grad_fn is not None
        assert torch.equal(ha, ha1.detach()) and torch.equal(a, a1.detach())
    finally:
        Fn.reset_default_graph()


def test_attention_3d_time_warp_att_gradient_reaches_C():
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, K, T, JQ, w, simi, tanh, masked, seed = ATT_CASES["timewarp"]
    h, q, W, b, hm, qm = att_case(*ATT_CASES["timewarp"])
    g = torch.Generator().manual_seed(seed)
    C = torch.rand(N, T, T, generator=g) / T + 0.02
    G1, G2 = torch.randn(N, w, generator=g), torch.randn(N, K, T, JQ, generator=g)
    leaves = _dbl(h, q, W, b, C)
    ra, rl = F.attention_3d(*leaves[:4], None, None, simiMatrix=simi, add_tanh=tanh, time_warp_att=True, C=leaves[4])
    torch.autograd.backward([ra, rl], [G1.double(), G2.double()])
    hc, qc, Cc = _cu(h).requires_grad_(), _cu(q).requires_grad_(), _cu(C).requires_grad_()
    Wc, bc = _set_att_vars(Fn, W, b)
    try:
        ha, a = Fn.attention_3d(hc, qc, simiMatrix=simi, add_tanh=tanh, time_warp_att=True, C=Cc)
        _close(ha, ra, rtol=RTOL, atol=ATOL, msg="h_a")
        torch.autograd.backward([ha, a], [_cu(G1), _cu(G2)])
        for got, ref, nm in zip(_grads([hc, qc, Wc, bc, Cc]), _grads(leaves), ("d_hinfo", "d_hq", "dW", "db", "dC")):
            _close(got, ref, rtol=RTOL, atol=ATOL, msg=nm)
    finally:
        Fn.reset_default_graph()


def test_attention_3d_cosine_h_a_gradient_and_cube_refusal():
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, K, T, JQ, w, simi, tanh, masked, seed = ATT_CASES["cosine"]
    h, q, _, _, hm, qm = att_case(*ATT_CASES["cosine"])
    G1 = torch.randn(N, w, generator=torch.Generator().manual_seed(seed))
    hd, qd = _dbl(h, q)
    ra, _ = F.attention_3d(hd, qd, None, None, hm, qm, simiMatrix=4)
    ra.backward(G1.double())
    Fn.reset_default_graph()
    hc, qc = _cu(h).requires_grad_(), _cu(q).requires_grad_()
    ha, a = Fn.attention_3d(hc, qc, _cu(hm), _cu(qm), simiMatrix=4)
    ha.backward(_cu(G1), retain_graph=True)
    _close(hc.grad, hd.grad, rtol=RTOL, atol=ATOL, msg="d_hinfo")
    _close(qc.grad, qd.grad, rtol=RTOL, atol=ATOL, msg="d_hq")
    with pytest.raises(NotImplementedError, match="simiMatrix 4"):
        a.backward(torch.ones_like(a))


def test_attention_bidirect_autograd():
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, K, T, JQ, w, simi, tanh, masked, seed = ATT_CASES["bidirect"]
    h, q, W, b, hm, qm = att_case(*ATT_CASES["bidirect"])
    G1 = torch.randn(N, 2 * w, generator=torch.Generator().manual_seed(seed))
    leaves = _dbl(h.reshape(N, T, w), q, W, b)
    ra, _ = F.attention(*leaves, hm.reshape(N, T), qm, simiMatrix=simi, add_tanh=tanh, bidirect=True)
    ra.backward(G1.double())
    hc, qc = _cu(h.reshape(N, T, w)).requires_grad_(), _cu(q).requires_grad_()
    Wc, bc = _set_att_vars(Fn, W, b)
    try:
        ha, _ = Fn.attention(hc, qc, _cu(hm.reshape(N, T)), _cu(qm), simiMatrix=simi, add_tanh=tanh, bidirect=True)
        _close(ha, ra, rtol=RTOL, atol=ATOL, msg="[h_a, q_a]")
        ha.backward(_cu(G1))
        for got, ref, nm in zip(_grads([hc, qc, Wc, bc]), _grads(leaves), ("d_hinfo", "d_hq", "dW", "db")):
            _close(got, ref, rtol=RTOL, atol=ATOL, msg=nm)
    finally:
        Fn.reset_default_graph()


def test_question_attention_module_is_the_functional_attention():
    """nn.QuestionAttention (K = 1, bidirect) against functional.attention with the same weights: same bits, and its
    parameters receive gradients"""
    from fvta_memexqa_amd import functional as Fn, nn as fnn
    N, K, T, JQ, w, simi, tanh, masked, seed = ATT_CASES["bidirect"]
    h, q, W, b, hm, qm = att_case(*ATT_CASES["bidirect"])
    mod = fnn.QuestionAttention(w, simiMatrix=simi, add_tanh=tanh, bidirect=True)
    assert mod.state_dict()["att_logits/W"].shape == (3 * w, 1)
    with torch.no_grad():
        mod.p("att_logits/W").copy_(W)
        mod.p("att_logits/b").copy_(b)
    hc, qc = _cu(h.reshape(N, T, w)), _cu(q)
    ha, a = mod(hc, qc, _cu(hm.reshape(N, T)), _cu(qm))
    _set_att_vars(Fn, W, b)
    try:
        ha0, a0 = Fn.attention(hc, qc, _cu(hm.reshape(N, T)), _cu(qm), simiMatrix=simi, add_tanh=tanh, bidirect=True)
    finally:
        Fn.reset_default_graph()
    assert ha.shape == (N, 2 * w) and torch.equal(ha.detach(), ha0.detach()) and torch.equal(a.detach(), a0.detach())
    ha.sum().backward()
    assert mod.p("att_logits/W").grad is not None and float(mod.p("att_logits/W").grad.abs().max()) > 0.0
    assert mod.p("att_logits/b").grad is not None


# ------------------------------------------------------------------ 4. bi-LSTM
LSTM_SHAPE = (5, 7, 12, 32)
LSTM_LENS = (0, 7, 3, 1, 5)


def _lstm_inputs(seed=5):
    B, J, din, d = LSTM_SHAPE
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, J, din, generator=g)
    ks = [torch.randn(din + d, 4 * d, generator=g) * 0.2 for _ in range(2)]
    bs = [torch.randn(4 * d, generator=g) * 0.1 for _ in range(2)]
    G_out, G_last = torch.randn(B, J, 2 * d, generator=g), torch.randn(B, 2 * d, generator=g)
    return x, ks, bs, G_out, G_last


def _mode_outs(out, last, G_out, G_last, mode, conv):
    return {"out": ([out], [conv(G_out)]), "last": ([last], [conv(G_last)]),
            "both": ([out, last], [conv(G_out), conv(G_last)])}[mode]


@functools.lru_cache(maxsize=None)
def _lstm_reference(shared, mode):
    from oracle import fvta_fused as F
    B, J, din, d = LSTM_SHAPE
    x, ks, bs, G_out, G_last = _lstm_inputs()
    lens = torch.tensor(LSTM_LENS)
    mask = torch.arange(J)[None, :] < lens[:, None]
    leaves = _dbl(x, ks[0], bs[0]) + (_dbl(ks[1], bs[1]) if not shared else [None, None])
    out, last = F.encode_stream(leaves[0], mask, leaves[1], leaves[2], leaves[3], leaves[4])
    torch.autograd.backward(*_mode_outs(out, last, G_out, G_last, mode, lambda t: t.double()))
    return out.detach(), last.detach(), [None if t is None else t.grad.clone() for t in leaves]


def _run_bilstm(shared, mode, precision):
    from fvta_memexqa_amd import autograd as A
    x, ks, bs, G_out, G_last = _lstm_inputs()
    leaves = [_cu(x).requires_grad_(), _cu(ks[0]).requires_grad_(), _cu(bs[0]).requires_grad_()]
    leaves += [None, None] if shared else [_cu(ks[1]).requires_grad_(), _cu(bs[1]).requires_grad_()]
    out, last = A.bilstm(leaves[0], torch.tensor(LSTM_LENS).cuda(), leaves[1], leaves[2], leaves[3], leaves[4], precision=precision)
    torch.autograd.backward(*_mode_outs(out, last, G_out, G_last, mode, _cu))
    return out, last, _grads(leaves)


@pytest.mark.parametrize("precision,rtol,atol", [("f32", RTOL, ATOL), ("bf16x3", 2e-4, 5e-5)])
@pytest.mark.parametrize("mode", ["out", "last", "both"])
@pytest.mark.parametrize("shared", [True, False])
def test_bilstm_autograd(shared, mode, precision, rtol, atol):
    """ragged batch with one empty and one full-length sequence; gradient from either output alone and from both"""
    ro, rl, rg = _lstm_reference(shared, mode)
    out, last, grads = _run_bilstm(shared, mode, precision)
    _close(out, ro, rtol=rtol, atol=atol, msg="out")
    _close(last, rl, rtol=rtol, atol=atol, msg="last")
    for got, ref, nm in zip(grads, rg, ("dx", "dkernel_fw", "dbias_fw", "dkernel_bw", "dbias_bw")):
        if ref is not None:
            _close(got, ref, rtol=rtol, atol=atol, msg=nm)


def test_bilstm_autograd_bf16():
    """the bf16 engine at the project's bf16 bound: 4e-2 relative L2 per gradient tensor"""
    ro, rl, rg = _lstm_reference(True, "both")
    out, last, grads = _run_bilstm(True, "both", "bf16")
    for got, ref, nm in zip([out, last] + grads, [ro, rl] + rg, ("out", "last", "dx", "dkernel_fw", "dbias_fw")):
        err = float((got.detach().cpu().double() - ref).norm() / ref.norm())
        print("bf16 %s: relative L2 %.3e" % (nm, err))
        assert err <= 4e-2, "%s: relative L2 %.3e" % (nm, err)


def test_bilstm_module_applied_twice_sums_the_weight_gradient():
    """one module, two inputs, one backward(): the shared weight's gradient is the oracle's sum over both calls"""
    from fvta_memexqa_amd import nn as fnn
    from oracle import fvta_fused as F
    B, J, din, d = LSTM_SHAPE
    x, ks, bs, G_out, G_last = _lstm_inputs()
    x2 = torch.randn(3, 4, din, generator=torch.Generator().manual_seed(8))
    lens, lens2 = torch.tensor(LSTM_LENS), torch.tensor([4, 2, 3])
    G2 = torch.randn(3, 2 * d, generator=torch.Generator().manual_seed(9))
    xd, x2d, kd, bd = _dbl(x, x2, ks[0], bs[0])
    o1, _ = F.encode_stream(xd, torch.arange(J)[None, :] < lens[:, None], kd, bd)
    _, l2 = F.encode_stream(x2d, torch.arange(4)[None, :] < lens2[:, None], kd, bd)
    ((o1 * G_out.double()).sum() + (l2 * G2.double()).sum()).backward()
    enc = fnn.BiLSTMEncoder(din, d)
    with torch.no_grad():
        enc.p("fw/basic_lstm_cell/kernel").copy_(ks[0])
        enc.p("fw/basic_lstm_cell/bias").copy_(bs[0])
    xc, x2c = _cu(x).requires_grad_(), _cu(x2).requires_grad_()
    c1, _ = enc(xc, lens.cuda())
    _, c2 = enc(x2c, lens2.cuda())
    ((c1 * _cu(G_out)).sum() + (c2 * _cu(G2)).sum()).backward()
    _close(xc.grad, xd.grad, rtol=RTOL, atol=ATOL, msg="dx (first call)")
    _close(x2c.grad, x2d.grad, rtol=RTOL, atol=ATOL, msg="dx (second call)")
    _close(enc.p("fw/basic_lstm_cell/kernel").grad, kd.grad, rtol=RTOL, atol=ATOL, msg="dkernel = sum of both calls")
    _close(enc.p("fw/basic_lstm_cell/bias").grad, bd.grad, rtol=RTOL, atol=ATOL, msg="dbias = sum of both calls")


# ------------------------------------------------------------------ 5. the small helpers, one case each
def test_linear_autograd():
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    g = torch.Generator().manual_seed(21)
    x, W, b, G = torch.randn(3, 5, 37, generator=g), torch.randn(37, 70, generator=g) * 0.2, torch.randn(70, generator=g), \
        torch.randn(3, 5, 70, generator=g)
    xd, Wd, bd = _dbl(x, W, b)
    ref = F.linear(xd, Wd, bd, add_tanh=True)
    ref.backward(G.double())
    Fn.reset_default_graph()
    xc = _cu(x).requires_grad_()
    Fn.variables["lin/W"], Fn.variables["lin/b"] = _cu(W).requires_grad_(), _cu(b).requires_grad_()
    try:
        y = Fn.linear(xc, 70, scope="lin", add_tanh=True)
        _close(y, ref, rtol=RTOL, atol=ATOL, msg="y")
        y.backward(_cu(G))
        _close(xc.grad, xd.grad, rtol=RTOL, atol=ATOL, msg="dx")
        _close(Fn.variables["lin/W"].grad, Wd.grad, rtol=RTOL, atol=ATOL, msg="dW")
        _close(Fn.variables["lin/b"].grad, bd.grad, rtol=RTOL, atol=ATOL, msg="db")
        y2 = Fn.linear_raw(xc.detach(), _cu(W), None)                 # no bias, nothing requires grad
        assert y2.grad_fn is None
    finally:
        Fn.reset_default_graph()


def test_softmax_and_exp_mask_autograd():
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    g = torch.Generator().manual_seed(22)
    x, G = torch.randn(4, 3, 130, generator=g) * 3, torch.randn(4, 3, 130, generator=g)
    mask = torch.rand(4, 3, 130, generator=g) < 0.7
    mask[..., 0] = True
    xd, = _dbl(x)
    ref = F.softmax(F.exp_mask(xd, mask))
    ref.backward(G.double())
    xc = _cu(x).requires_grad_()
    m = Fn.exp_mask(xc, mask.cuda())
    assert m.grad_fn is not None
    p = Fn.softmax(m)
    _close(p, ref, rtol=RTOL, atol=ATOL, msg="softmax")
    p.backward(_cu(G))
    _close(xc.grad, xd.grad, rtol=RTOL, atol=ATOL, msg="dx")
    x2 = _cu(x).requires_grad_()                                         # exp_mask alone: the identity on val
    Fn.exp_mask(x2, mask.cuda()).backward(_cu(G))
    assert torch.equal(x2.grad, _cu(G))


@pytest.mark.parametrize("eu,tanh", [(False, False), (True, True)])
def test_scorer_ce_autograd(eu, tanh):
    from fvta_memexqa_amd import autograd as A
    from oracle import fvta_fused as F
    N, C, w = 5, 4, 48
    g = torch.Generator().manual_seed(23)
    gq, g1, gch = torch.randn(N, w, generator=g), torch.randn(N, w, generator=g), torch.randn(N, C, w, generator=g)
    W, b = torch.randn((7 if eu else 5) * w, 1, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1
    y = torch.zeros(N, C, dtype=torch.bool)
    y[torch.arange(N - 1), torch.tensor([1, 0, 3, 2])] = True            # the last row has no label (a padded row)
    leaves = _dbl(gq, g1, gch, W, b)
    logits, yp = F.scorer(*leaves, use_eu_output=eu, add_tanh=tanh)
    ref = F.softmax_cross_entropy_mean(logits, y, tf_grad=True)
    (ref * 0.7).backward()
    cl = [_cu(t).requires_grad_() for t in (gq, g1, gch, W, b)]
    loss, lg, p = A.scorer_ce(*cl, y.cuda(), use_eu_output=eu, add_tanh=tanh)
    assert loss.grad_fn is not None and not lg.requires_grad and not p.requires_grad
    _close(loss, ref, rtol=RTOL, atol=ATOL, msg="loss")
    _close(lg, logits, rtol=RTOL, atol=ATOL, msg="logits")
    _close(p, yp, rtol=RTOL, atol=ATOL, msg="yp")
    (loss * 0.7).backward()
    for got, ref_, nm in zip(_grads(cl), _grads(leaves), ("dgq", "dg1", "dgch", "dW", "db")):
        _close(got, ref_, rtol=RTOL, atol=ATOL, msg=nm)


def test_attention_tgif_autograd():
    from fvta_memexqa_amd import functional as Fn
    from oracle import fvta_fused as F
    N, V, w, mlp = 3, 9, 24, 16
    g = torch.Generator().manual_seed(24)
    hinfo, lq = torch.randn(N, V, w, generator=g), torch.randn(N, 2 * mlp, generator=g)
    shapes = dict(q_W=(2 * mlp, mlp), q_b=(mlp,), h_W=(w, mlp), h_b=(mlp,), p_W=(mlp, 1), p_b=(1,), f_W=(w, 2 * mlp), f_b=(2 * mlp,))
    p = {k: torch.randn(*s, generator=g) * 0.3 for k, s in shapes.items()}
    G1, G2 = torch.randn(N, 2 * mlp, generator=g), torch.randn(N, V, generator=g)
    hd, ld = _dbl(hinfo, lq)
    pd = {k: v.double().requires_grad_() for k, v in p.items()}
    rf, ratt = F.attention_tgif(hd, ld, pd)
    torch.autograd.backward([rf, ratt], [G1.double(), G2.double()])
    Fn.reset_default_graph()
    names = dict(q="mlp_q", h="mlp_h", p="preatt", f="final")
    for k, v in p.items():
        Fn.variables["tgif/%s/%s" % (names[k[0]], k[2])] = _cu(v).requires_grad_()
    hc, lc = _cu(hinfo).requires_grad_(), _cu(lq).requires_grad_()
    try:
        final, att = Fn.attention_tgif(hc, lc, mlp_dim=mlp, scope="tgif")
        _close(final, rf, rtol=RTOL, atol=ATOL, msg="logits")
        torch.autograd.backward([final, att], [_cu(G1), _cu(G2)])
        _close(hc.grad, hd.grad, rtol=RTOL, atol=ATOL, msg="d_hinfo")
        _close(lc.grad, ld.grad, rtol=RTOL, atol=ATOL, msg="d_lq")
        for k in p:
            _close(Fn.variables["tgif/%s/%s" % (names[k[0]], k[2])].grad, pd[k].grad, rtol=RTOL, atol=ATOL, msg=k)
    finally:
        Fn.reset_default_graph()


# ------------------------------------------------------------------ 6. end to end with nn.py
E2E = dict(N=2, K=2, T=12, JQ=4, C=3, JC=3, din=10, hidden=50)


class _TinyModel(torch.nn.Module):
    """two encoders, the focal attention and the scorer: what a user composes from fvta_memexqa_amd.nn"""

    def __init__(self, din, hidden):
        from fvta_memexqa_amd import nn as fnn
        super().__init__()
        self.text = fnn.BiLSTMEncoder(din, hidden, seed=1)
        self.photo = fnn.BiLSTMEncoder(din, hidden, share_fw_bw=False, seed=2)
        self.att = fnn.FocalAttention3D(2 * hidden, simiMatrix=2, add_tanh=True, seed=3)
        self.out = fnn.AnswerScorer(2 * hidden, seed=4)

    def forward(self, xq, qlen, xc, clen, xch, chlen, y):
        N, K, T = clen.shape[0] // E2E["K"], E2E["K"], xc.shape[1]
        hq, lq = self.text(xq, qlen)
        hall, _ = self.photo(xc, clen)
        _, lch = self.text(xch, chlen)
        ar = lambda J, ln: torch.arange(J, device=ln.device)[None, :] < ln[:, None]
        h_a, a = self.att(hall.reshape(N, K, T, -1), hq, ar(T, clen).reshape(N, K, T), ar(xq.shape[1], qlen))
        return self.out(lq, h_a, lch.reshape(N, -1, lch.shape[-1]), y)[0]


def _e2e_inputs():
    c = E2E
    g = torch.Generator().manual_seed(31)
    xq = torch.randn(c["N"], c["JQ"], c["din"], generator=g)
    xc = torch.randn(c["N"] * c["K"], c["T"], c["din"], generator=g)
    xch = torch.randn(c["N"] * c["C"], c["JC"], c["din"], generator=g)
    qlen, clen, chlen = torch.tensor([4, 2]), torch.tensor([12, 5, 1, 9]), torch.tensor([3, 1, 2, 2, 3, 1])
    y = torch.zeros(c["N"], c["C"], dtype=torch.bool)
    y[0, 1] = y[1, 2] = True
    return xq, qlen, xc, clen, xch, chlen, y


def _e2e_oracle(sd, inputs):
    from oracle import fvta_fused as F
    c = E2E
    xq, qlen, xc, clen, xch, chlen, y = inputs
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in sd.items()}
    ar = lambda J, ln: torch.arange(J)[None, :] < ln[:, None]
    tk, tb = P["text.fw/basic_lstm_cell/kernel"], P["text.fw/basic_lstm_cell/bias"]
    hq, lq = F.encode_stream(xq.double(), ar(c["JQ"], qlen), tk, tb)
    hall, _ = F.encode_stream(xc.double(), ar(c["T"], clen), P["photo.fw/basic_lstm_cell/kernel"], P["photo.fw/basic_lstm_cell/bias"],
                              P["photo.bw/basic_lstm_cell/kernel"], P["photo.bw/basic_lstm_cell/bias"])
    _, lch = F.encode_stream(xch.double(), ar(c["JC"], chlen), tk, tb)
    h_a, _ = F.attention_3d(hall.reshape(c["N"], c["K"], c["T"], -1), hq, P["att.att_logits/W"], P["att.att_logits/b"],
                            ar(c["T"], clen).reshape(c["N"], c["K"], c["T"]), ar(c["JQ"], qlen), simiMatrix=2, add_tanh=True)
    logits, _ = F.scorer(lq, h_a, lch.reshape(c["N"], c["C"], -1), P["out.choicelogits/W"], P["out.choicelogits/b"])
    loss = F.softmax_cross_entropy_mean(logits, y, tf_grad=True)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in P.items()}


def test_end_to_end_model_from_nn_trains():
    c = E2E
    inputs = _e2e_inputs()
    dev = [t.cuda() for t in inputs]
    model = _TinyModel(c["din"], c["hidden"])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert sd["text.fw/basic_lstm_cell/kernel"].shape == (c["din"] + c["hidden"], 4 * c["hidden"])      # the reference's shapes
    assert sd["att.att_logits/W"].shape == (2 * 2 * c["hidden"], 1) and sd["out.choicelogits/W"].shape == (5 * 2 * c["hidden"], 1)
    ref_loss, ref_grads = _e2e_oracle(sd, inputs)
    loss = model(*dev)
    _close(loss, ref_loss, rtol=RTOL, atol=ATOL, msg="loss")
    loss.backward()
    params = dict(model.named_parameters())
    assert set(params) == set(ref_grads)
    for k, p in params.items():
        _close(p.grad, ref_grads[k], rtol=RTOL, atol=ATOL, msg=k)
    opt = torch.optim.Adadelta(model.parameters(), lr=0.5)
    first = float(loss.detach())
    for _ in range(3):
        opt.zero_grad()
        step_loss = model(*dev)
        step_loss.backward()
        opt.step()
    with torch.no_grad():
        after = model(*dev)
    assert after.grad_fn is None
    assert float(after) < first, "three Adadelta steps did not lower the loss: %.6f -> %.6f" % (first, float(after))
    twin = _TinyModel(c["din"], c["hidden"])
    twin.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(twin(*dev), after)
