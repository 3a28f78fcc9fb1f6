"""GPU parity of the differentiable attention_keeprank1 (fvta_attn_bwd_u under autograd._KeepRank1,
functional.attention_keeprank1[_raw], nn.ChoicesAttention): gradients vs torch autograd on the fp64 fused oracle's
attention_keeprank1, and vs the K = 1 route at batch N*M that the fused model trains.

Shapes (N, M, V, JQ, w) are the smallest that reach each path of the backward: one workgroup per (n,m); several workgroups
on one (n,m) (bsplit > 1); the batch where the ORDINARY backward groups several k into a workgroup (gk > 1 -- the
per-stream entry runs one k per workgroup there); the 1024-wide and the two-float4-per-thread kernels.  The regime is
asserted through fvta_attn_plan.

The oracle comparisons keep a valid row in every (n,m), a valid position in every question and no exact tie in the max
over the question (tests/test_keeprank_host.py checks the seeds): the two deliberate deviations from TensorFlow's gradient
 are pinned by the comparison with the K = 1 route instead, which shares them.

Tolerance: the exact-fp32 class (tests/test_gpu_autograd.py): rtol 1e-4, atol 2e-5 x max(1, max|ref|).
"""
import ctypes
import functools

import pytest
import torch

from tests.test_gpu_autograd import ATOL, RTOL, _cu, _dbl, _grads, att_case
from tests.test_gpu_backward import _close

pytestmark = pytest.mark.gpu

# name -> (N, M, V, JQ, w, simi, masked, seed, bidirect)
SMALL = {"a64_s%d_%s" % (s, "m" if m else "u"): (2, 4, 5, 3, 64, s, m, 40 + 2 * s + m, False) for s in (1, 2, 3) for m in (True, False)}
SMALL.update({"a100_s%d_%s" % (s, "m" if m else "u"): (2, 3, 7, 4, 100, s, m, 50 + 2 * s + m, False) for s in (1, 2, 3) for m in (True, False)})
SPLIT = {"b1100": (1, 2, 1100, 5, 64, 1, True, 61, False), "b600": (1, 2, 600, 5, 64, 3, True, 62, False)}
GROUPED = {"c_m": (260, 4, 6, 3, 64, 2, True, 63, False), "c_u": (260, 4, 6, 3, 64, 1, False, 64, False)}
WIDE = {"d2048": (1, 2, 40, 4, 2048, 3, True, 65, False), "d1024": (1, 2, 33, 4, 1024, 1, True, 66, False)}
BIDIRECT = {"e_bidirect": (2, 3, 6, 4, 64, 2, True, 67, True)}
ORACLE_CASES = dict(SMALL, **SPLIT, **GROUPED, **WIDE, **BIDIRECT)
# the backward plan of the ORDINARY attention at these shapes (fvta_attn_plan's bsplit, gk): what the shape is there for.
# (attn_shape: bsplit = min(ceil(1024 / (N K)), ceil(T / 256)), at least ceil(T / 960) -- 5 and 3 workgroups per (n,m))
PLAN = {"b1100": ("bsplit", 5), "b600": ("bsplit", 3), "c_m": ("gk", 2), "c_u": ("gk", 2)}


def kr_case(N, M, V, JQ, w, simi, masked, seed):
    """att_case (a valid question position in every batch row) with a valid row in EVERY (n,m) list"""
    h, q, W, b, hm, qm = att_case(N, M, V, JQ, w, simi, False, masked, seed)
    if masked:
        hm[..., 0] |= ~hm.any(-1)
    return h, q, W, b, hm, qm


def kr_grad_out(name):
    N, M, V, JQ, w, simi, masked, seed, bidirect = ORACLE_CASES[name]
    return torch.randn(N, M, 2 * w if bidirect else w, generator=torch.Generator().manual_seed(seed + 1000))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(u, [d_hinfo, d_hq, dW, db]) of the fp64 oracle, computed once per case"""
    from oracle import fvta_fused as F
    N, M, V, JQ, w, simi, masked, seed, bidirect = ORACLE_CASES[name]
    h, q, W, b, hm, qm = kr_case(N, M, V, JQ, w, simi, masked, seed)
    leaves = _dbl(h, q, W, b)
    ref = F.attention_keeprank1(*leaves, hm, qm, simiMatrix=simi, bidirect=bidirect)
    ref.backward(kr_grad_out(name).double())
    return ref.detach(), [t.grad for t in leaves]


def _assert_plan(name):
    from fvta_memexqa_amd import ops
    N, M, V, JQ, w, simi, masked, seed, bidirect = ORACLE_CASES[name]
    if name in PLAN:
        key, want = PLAN[name]
        p = ops.FocalAttention(N, M, V, JQ, w, simi, False, feat_order=1).plan(masked)
        assert p[key] == want and want > 1, "%s: fvta_attn_plan says %r, the case is there for %s = %d" % (name, p, key, want)


def _check_against_oracle(name):
    from fvta_memexqa_amd import functional as Fn
    N, M, V, JQ, w, simi, masked, seed, bidirect = ORACLE_CASES[name]
    _assert_plan(name)
    ref, ref_grads = _reference(name)
    h, q, W, b, hm, qm = kr_case(N, M, V, JQ, w, simi, masked, seed)
    leaves = [_cu(t).requires_grad_() for t in (h, q, W, b)]
    out = Fn.attention_keeprank1_raw(*leaves, _cu(hm), _cu(qm), simiMatrix=simi, bidirect=bidirect)
    assert out.grad_fn is not None and tuple(out.shape) == tuple(ref.shape)
    _close(out, ref, rtol=RTOL, atol=ATOL, msg="u")
    out.backward(_cu(kr_grad_out(name)))
    for got, want, nm in zip(_grads(leaves), ref_grads, ("d_hinfo", "d_hq", "dW", "db")):
        assert got is not None, nm
        _close(got, want, rtol=RTOL, atol=ATOL, msg="%s: %s" % (name, nm))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_keeprank1_gradient_small(name):
    """(a): w = 64 and w = 100 (padded to 128), masked and unmasked, simiMatrix 1-3: forward u and all four gradients"""
    _check_against_oracle(name)


@pytest.mark.parametrize("name", sorted(SPLIT))
def test_keeprank1_gradient_several_workgroups_per_stream(name):
    """(b): the row list of one (n,m) is split over bsplit backward workgroups, their dQs slabs folded afterwards"""
    _check_against_oracle(name)


@pytest.mark.parametrize("name", sorted(GROUPED))
def test_keeprank1_gradient_where_the_ordinary_backward_groups_k(name):
    """(c): N*M >= 1024 with short lists -- fvta_attn_bwd puts gk = 2 streams into a workgroup here; fvta_attn_bwd_u runs
    them one per workgroup, each with its own gradient vector."""
    _check_against_oracle(name)


@pytest.mark.parametrize("name", sorted(WIDE))
def test_keeprank1_gradient_wide_rows(name):
    """(d): w = 2048 (two float4 per thread and row) and w = 1024 with a row count that is no multiple of the tile"""
    _check_against_oracle(name)


def test_keeprank1_bidirect_gradient():
    """(e): [N,M,2w] = concat([u, q_a]) through the variable store: g_u (fvta_attn_bwd_u) and g_a (fvta_attn_cube_bwd at
    K = M, accumulated on top) in one backward"""
    from fvta_memexqa_amd import functional as Fn
    name = "e_bidirect"
    N, M, V, JQ, w, simi, masked, seed, bidirect = ORACLE_CASES[name]
    ref, ref_grads = _reference(name)
    h, q, W, b, hm, qm = kr_case(N, M, V, JQ, w, simi, masked, seed)
    hc, qc = _cu(h).requires_grad_(), _cu(q).requires_grad_()
    Fn.reset_default_graph()
    Wc, bc = _cu(W).requires_grad_(), _cu(b).requires_grad_()
    Fn.variables["kr/att_logits/W"], Fn.variables["kr/att_logits/b"] = Wc, bc
    try:
        out = Fn.attention_keeprank1(hc, qc, _cu(hm), _cu(qm), simiMatrix=simi, bidirect=True, scope="kr")
        assert out.grad_fn is not None and tuple(out.shape) == (N, M, 2 * w)
        _close(out, ref, rtol=RTOL, atol=ATOL, msg="[u, q_a]")
        out.backward(_cu(kr_grad_out(name)))
        for got, want, nm in zip(_grads([hc, qc, Wc, bc]), ref_grads, ("d_hinfo", "d_hq", "dW", "db")):
            _close(got, want, rtol=RTOL, atol=ATOL, msg=nm)
    finally:
        Fn.reset_default_graph()


@pytest.mark.parametrize("simi", [1, 2, 3])
def test_keeprank1_is_the_k1_route_at_batch_n_times_m(simi):
    """(f): the route the fused model trains -- attention at K = 1 on hinfo [N*M,1,V,w] with hq expanded per m, model.py's
    feature order.  One (n,m) list is fully masked (nothing reaches its logits, its rows take the uniform softmax's share)
    and one question has two identical positions (an exact tie in the max over the question: the first takes all) --
    both routes are the same fp32 kernels with the same deviations, so they agree at the fp32 tolerance."""
    from fvta_memexqa_amd import functional as Fn
    from tests.test_gpu_forward import _att_case
    N, M, V, JQ, w = 2, 4, 9, 5, 64
    h, q, W, b, hm, qm = _att_case(N, M, V, JQ, w, simi, False, True, seed=70 + simi)
    assert not bool(hm[0, 0].any())                      # the fully masked list
    qm[N - 1, :2] = True
    qm[0, :2] = True
    q[0, 1] = q[0, 0]                                    # an exact tie wherever position 0 / 1 is the maximum
    G = torch.randn(N, M, w, generator=torch.Generator().manual_seed(80 + simi))
    hmc, qmc = _cu(hm), _cu(qm)

    a = [_cu(t).requires_grad_() for t in (h, q, W, b)]
    u = Fn.attention_keeprank1_raw(*a, hmc, qmc, simiMatrix=simi)
    u.backward(_cu(G))

    r = [_cu(t).requires_grad_() for t in (h, q, W, b)]
    hq_rep = r[1][:, None].expand(N, M, JQ, w).reshape(N * M, JQ, w)
    qm_rep = qmc[:, None].expand(N, M, JQ).reshape(N * M, JQ)
    h_a, _ = Fn.attention_raw(r[0].reshape(N * M, 1, V, w), hq_rep, r[2], r[3], hmc.reshape(N * M, 1, V), qm_rep,
                              simiMatrix=simi, add_tanh=False, feat_order=1)
    h_a.backward(_cu(G).reshape(N * M, w))
    _close(u, h_a.reshape(N, M, w), rtol=RTOL, atol=ATOL, msg="u")
    assert float(a[0].grad[0, 0].abs().max()) > 0.0      # the fully masked list still gets p * g on its rows
    for got, want, nm in zip(_grads(a), _grads(r), ("d_hinfo", "d_hq", "dW", "db")):
        _close(got, want, rtol=RTOL, atol=ATOL, msg=nm)


def test_keeprank1_without_grad_is_the_plain_call():
    """(g) nothing requires grad: no grad_fn, bit for bit the handle called directly and the call that records a graph"""
    from fvta_memexqa_amd import functional as Fn, ops
    N, M, V, JQ, w, simi, masked, seed, _ = ORACLE_CASES["a64_s2_m"]
    h, q, W, b, hm, qm = kr_case(N, M, V, JQ, w, simi, masked, seed)
    hc, qc, Wc, bc, hmc, qmc = (_cu(t) for t in (h, q, W, b, hm, qm))
    u = Fn.attention_keeprank1_raw(hc, qc, Wc, bc, hmc, qmc, simiMatrix=simi)
    assert u.grad_fn is None and not u.requires_grad
    op = ops.FocalAttention(N, M, V, JQ, w, simi, False, feat_order=1)
    op.forward(hc, qc, ops.as_mask_u8(hmc), ops.as_mask_u8(qmc), Wc.reshape(-1).contiguous(), bc, want_logits=False)
    assert torch.equal(u, op.read_u())
    u1 = Fn.attention_keeprank1_raw(hc.clone().requires_grad_(), qc, Wc, bc, hmc, qmc, simiMatrix=simi)
    assert u1.grad_fn is not None and torch.equal(u, u1.detach())


def test_choices_attention_module_applied_twice_sums_the_weight_gradient():
    """(g) one nn.ChoicesAttention, two inputs, one backward(): the weight gradient is the oracle's sum over both calls"""
    from fvta_memexqa_amd import nn as fnn
    from oracle import fvta_fused as F
    w, simi = 64, 3
    c1 = kr_case(2, 4, 5, 3, w, simi, True, 91)
    c2 = kr_case(3, 2, 7, 4, w, simi, True, 92)
    W, b = c1[2], c1[3]
    G1 = torch.randn(2, 4, w, generator=torch.Generator().manual_seed(93))
    G2 = torch.randn(3, 2, w, generator=torch.Generator().manual_seed(94))
    h1d, q1d, h2d, q2d, Wd, bd = _dbl(c1[0], c1[1], c2[0], c2[1], W, b)
    r1 = F.attention_keeprank1(h1d, q1d, Wd, bd, c1[4], c1[5], simiMatrix=simi)
    r2 = F.attention_keeprank1(h2d, q2d, Wd, bd, c2[4], c2[5], simiMatrix=simi)
    ((r1 * G1.double()).sum() + (r2 * G2.double()).sum()).backward()
    mod = fnn.ChoicesAttention(w, simiMatrix=simi)
    assert mod.state_dict()["att_logits/W"].shape == (4 * w, 1)
    with torch.no_grad():
        mod.p("att_logits/W").copy_(W)
        mod.p("att_logits/b").copy_(b)
    h1, q1, h2, q2 = (_cu(t).requires_grad_() for t in (c1[0], c1[1], c2[0], c2[1]))
    o1 = mod(h1, q1, _cu(c1[4]), _cu(c1[5]))
    o2 = mod(h2, q2, _cu(c2[4]), _cu(c2[5]))
    ((o1 * _cu(G1)).sum() + (o2 * _cu(G2)).sum()).backward()
    _close(h1.grad, h1d.grad, rtol=RTOL, atol=ATOL, msg="d_hinfo (first call)")
    _close(q2.grad, q2d.grad, rtol=RTOL, atol=ATOL, msg="d_hq (second call)")
    _close(mod.p("att_logits/W").grad, Wd.grad, rtol=RTOL, atol=ATOL, msg="dW = sum of both calls")
    _close(mod.p("att_logits/b").grad, bd.grad, rtol=RTOL, atol=ATOL, msg="db = sum of both calls")


@pytest.mark.parametrize("name", ["a64_s3_m", "c_u"])
def test_attn_bwd_u_accumulates_and_repeats_bitwise(name):
    """(g) through the C ABI: accumulate = 0 over 7.0 (masked rows of d_hinfo become zeros), a second run bitwise equal,
    accumulate = 1 on top of ones = that result plus one, dW / db accumulated"""
    from fvta_memexqa_amd import ops
    N, M, V, JQ, w, simi, masked, seed, _ = ORACLE_CASES[name]
    _, ref_grads = _reference(name)
    h, q, W, b, hm, qm = kr_case(N, M, V, JQ, w, simi, masked, seed)
    hc, qc, Wc, bc = _cu(h), _cu(q), _cu(W.reshape(-1)), _cu(b)
    hmc, qmc = _cu(ops.as_mask_u8(hm)), _cu(ops.as_mask_u8(qm))
    Gc = _cu(kr_grad_out(name))
    op = ops.FocalAttention(N, M, V, JQ, w, simi, False, feat_order=1)
    op.forward(hc, qc, hmc, qmc, Wc, bc)

    def run(fill, acc, dW, db):
        dh, dq = torch.full_like(hc, fill), torch.full_like(qc, fill)
        op.backward_u(hc, qc, hmc, qmc, Wc, bc, Gc, dh, dq, dW, db, acc)
        return dh, dq

    dW, db = torch.zeros_like(Wc), torch.zeros(1, device="cuda")
    dh, dq = run(7.0, 0, dW, db)
    for got, want, nm in zip((dh, dq, dW, db), ref_grads, ("d_hinfo", "d_hq", "dW", "db")):
        _close(got, want.reshape(got.shape), rtol=RTOL, atol=ATOL, msg=nm)
    if masked:
        assert float(dh[~_cu(hm)].abs().max()) == 0.0, "masked rows of d_hinfo are zeros under accumulate = 0"
    dW2, db2 = torch.zeros_like(Wc), torch.zeros(1, device="cuda")
    dh2, dq2 = run(float("nan"), 0, dW2, db2)
    for x, y in ((dh, dh2), (dq, dq2), (dW, dW2), (db, db2)):
        assert torch.equal(x, y), "two runs differ"
    dh3, dq3 = run(1.0, 1, dW, db)
    _close(dh3, dh + 1.0, rtol=RTOL, atol=ATOL, msg="d_hinfo accumulate")
    _close(dq3, dq + 1.0, rtol=RTOL, atol=ATOL, msg="d_hq accumulate")
    _close(dW, 2 * dW2, rtol=RTOL, atol=ATOL, msg="dW accumulates")
    _close(db, 2 * db2, rtol=RTOL, atol=ATOL, msg="db accumulates")


def test_attn_bwd_u_rejects_what_it_does_not_cover():
    """(h) simiMatrix 4, a non-zero hinfo_stride, accumulate = 2: a negative status and a message, nothing launched"""
    from fvta_memexqa_amd import _lib
    from fvta_memexqa_amd._lib import AttnDesc, ptr, stream_ptr
    lib = _lib.load()
    N, T, JQ, w = 2, 8, 3, 64
    x = torch.zeros(N * T * w, device="cuda")
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def call(desc, acc):
        return lib.fvta_attn_bwd_u(ctypes.byref(desc), ptr(x), ptr(x), None, None, ptr(x), ptr(x), ptr(x), ptr(buf), ptr(x),
                                   ptr(x), ptr(x), ptr(x), acc, ptr(buf), stream_ptr())

    assert call(AttnDesc(N, 1, T, JQ, w, 4, 0, 0, 0), 0) < 0 and b"simiMatrix 4" in lib.fvta_last_error()
    assert lib.fvta_attn_bwd_u_workspace_bytes(ctypes.byref(AttnDesc(N, 1, T, JQ, w, 4, 0, 0, 0))) == 0
    assert call(AttnDesc(N, 1, T, JQ, w, 1, 0, 0, 2 * T * w), 0) < 0 and b"hinfo_stride" in lib.fvta_last_error()
    assert call(AttnDesc(N, 1, T, JQ, w, 1, 0, 0, 0), 2) < 0 and b"accumulate" in lib.fvta_last_error()
    torch.cuda.synchronize()


def test_keeprank1_refuses_a_batch_the_backward_does_not_cover_in_the_forward():
    """N * M = 65536 lists: without a gradient the forward runs; with one it is refused there, not in backward()"""
    from fvta_memexqa_amd import functional as Fn
    from fvta_memexqa_amd._lib import FvtaError
    N, M, V, JQ, w = 16384, 4, 1, 2, 64
    g = torch.Generator().manual_seed(95)
    h, q = torch.randn(N, M, V, w, generator=g).cuda(), torch.randn(N, JQ, w, generator=g).cuda()
    W, b = torch.randn(3 * w, 1, generator=g).cuda() * 0.1, torch.zeros(1).cuda()
    u = Fn.attention_keeprank1_raw(h, q, W, b)
    assert tuple(u.shape) == (N, M, w) and u.grad_fn is None
    with pytest.raises(FvtaError, match="65535"):
        Fn.attention_keeprank1_raw(h.requires_grad_(), q, W, b)
