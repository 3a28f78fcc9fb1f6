"""The pieces fvta_memexqa_amd.model (the model.py graph) adds to the C ABI: the strided 1-D attention
(fvta_attn_desc.hinfo_stride: one stream of an [N][all streams] arena, model.py:836-846 / :929-944) and the two shape ops
(fvta_rows_reduce / fvta_rows_broadcast = reduce_mean / tile and each other's backward)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,simi", [(64, 1), (128, 2), (256, 3)])
@pytest.mark.parametrize("masked", [True, False])
def test_strided_attention_equals_dense_on_the_gathered_stream(w, simi, masked):
    """forward and backward on a slice [N, V, w] of a wider [N, Vtot, w] arena == the same kernel on a dense copy
    (bitwise: same kernel, same order), in overwrite and accumulate mode; rows outside the slice are never touched"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    g = torch.Generator().manual_seed(5)
    N, V, off, Vtot, JQ = 5, 37, 11, 70, 9
    F = {1: 3, 2: 2, 3: 4}[simi]
    arena = torch.randn(N, Vtot, w, generator=g).to(dev)
    hq = torch.randn(N, JQ, w, generator=g).to(dev)
    W = (torch.randn(F * w, generator=g) * 0.1).to(dev)
    b = torch.zeros(1, device=dev)
    hm = (torch.rand(N, V, generator=g) > 0.3).to(torch.uint8).to(dev) if masked else None
    qm = (torch.rand(N, JQ, generator=g) > 0.2).to(torch.uint8).to(dev) if masked else None
    if masked:
        hm[:, 0] = 1
        qm[:, 0] = 1
    dense_h = arena[:, off:off + V].contiguous()
    op_d = ops.FocalAttention(N, 1, V, JQ, w, simi, False, feat_order=1)
    op_s = ops.FocalAttention(N, 1, V, JQ, w, simi, False, feat_order=1, hinfo_stride=Vtot * w)
    ha_d, lg_d = op_d.forward(dense_h, hq, hm, qm, W, b, True)
    ha_s, lg_s = op_s.forward(arena.view(-1)[off * w:], hq, hm, qm, W, b, True)
    assert torch.equal(ha_d, ha_s) and torch.equal(lg_d, lg_s)
    d_ha = torch.randn(N, w, generator=g).to(dev)
    for acc in (0, 1):
        base = torch.randn(N, Vtot, w, generator=g).to(dev)
        d_dense = base[:, off:off + V].contiguous()
        d_hq_d = torch.ones(N, JQ, w, device=dev)
        dW_d, db_d = torch.zeros(F * w, device=dev), torch.zeros(1, device=dev)
        op_d.backward(dense_h, hq, hm, qm, W, b, d_ha, d_dense, d_hq_d, dW_d, db_d, accumulate=acc)
        d_arena = base.clone()
        d_hq_s = torch.ones(N, JQ, w, device=dev)
        dW_s, db_s = torch.zeros(F * w, device=dev), torch.zeros(1, device=dev)
        op_s.backward(arena.view(-1)[off * w:], hq, hm, qm, W, b, d_ha, d_arena.view(-1)[off * w:], d_hq_s, dW_s, db_s,
                      accumulate=acc)
        assert torch.equal(d_arena[:, off:off + V], d_dense), acc
        assert torch.equal(d_arena[:, :off], base[:, :off]) and torch.equal(d_arena[:, off + V:], base[:, off + V:]), acc
        assert torch.equal(d_hq_d, d_hq_s) and torch.equal(dW_d, dW_s) and torch.equal(db_d, db_s)


def test_strided_attention_argument_checks():
    from fvta_memexqa_amd import _lib, ops
    ops.require_gpu()
    with pytest.raises(_lib.FvtaError):
        ops.FocalAttention(2, 3, 8, 4, 64, 1, False, hinfo_stride=8 * 64 * 3)      # K must be 1
    with pytest.raises(_lib.FvtaError):
        ops.FocalAttention(2, 1, 8, 4, 64, 1, False, hinfo_stride=4 * 64)          # shorter than the stream


def test_rows_reduce_and_broadcast():
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    g = torch.Generator().manual_seed(9)
    R, J, d, K = 7, 5, 300, 3
    x = torch.randn(R, J, d, generator=g).to(dev)
    out = torch.randn(R, K, d, generator=g).to(dev)
    want = out.clone()
    want[:, 1] = x.mean(1)
    ops.rows_reduce(x, out.view(-1)[d:], R, J, d, K * d, 1.0 / J)                   # into slot 1 of a [R,K,d] stack
    torch.testing.assert_close(out, want, rtol=1e-6, atol=1e-6)
    ops.rows_reduce(x, out.view(-1)[d:], R, J, d, K * d, 2.0, accumulate=True)
    want[:, 1] += 2.0 * x.sum(1)
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-5)
    v = torch.randn(R, K, d, generator=g).to(dev)
    y = torch.randn(R, J, d, generator=g).to(dev)
    wanty = v[:, 2][:, None, :].expand(R, J, d) * 0.25
    ops.rows_broadcast(v.view(-1)[2 * d:], y, R, J, d, K * d, 0.25)
    assert torch.equal(y, wanty.contiguous())
    ops.rows_broadcast(v.view(-1)[2 * d:], y, R, J, d, K * d, 1.0, accumulate=True)
    torch.testing.assert_close(y, wanty + v[:, 2][:, None, :], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("tanh", [False, True])
def test_linear_bwd_against_autograd(tanh):
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    g = torch.Generator().manual_seed(2)
    M, din, dout = 77, 130, 70
    x = torch.randn(M, din, generator=g).to(dev)
    W = (torch.randn(din, dout, generator=g) * 0.1).to(dev)
    b = torch.randn(dout, generator=g).to(dev)
    dy = torch.randn(M, dout, generator=g).to(dev)
    y = torch.empty(M, dout, device=dev)
    ops.linear_fwd(x, W, b, y, M, din, dout, tanh)
    xr, Wr, br = (t.double().cpu().requires_grad_() for t in (x, W, b))
    yr = xr @ Wr + br
    yr = torch.tanh(yr) if tanh else yr
    torch.testing.assert_close(y.cpu().double(), yr.detach(), rtol=1e-5, atol=1e-5)
    yr.backward(dy.double().cpu())
    dx = torch.full((M, din), 0.5, device=dev)
    dW, db = torch.ones(din, dout, device=dev), torch.ones(dout, device=dev)
    ops.linear_bwd(x, W, y, dy, dx, dW, db, M, din, dout, tanh, accumulate_dx=True)
    torch.testing.assert_close(dx.cpu().double(), xr.grad + 0.5, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dW.cpu().double(), Wr.grad + 1.0, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db.cpu().double(), br.grad + 1.0, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("simi", [1, 2, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_bidirect_attention_forward_backward(simi, masked):
    """attention(..., bidirect=True) -> [h_a ; q_a] (model.py:169-177) through fvta_attn_fwd + fvta_attn_qside_fwd, and its
    gradient through fvta_attn_bwd (max-pooled half) + fvta_attn_qside_bwd + fvta_attn_logits_bwd (dense half), against
    autograd of the fp64 oracle.

    db is analytically ZERO here: the bias shifts every logit alike and both halves are softmaxes over the logits, so the
    oracle's br.grad is rounding noise (<= 1e-14) and the db assertion below only says that the kernels' db is small.  The
    per-n bias partials and their fold (attn_logits_bwd_kernel's pb[n], the params kernel's db[0] += acc) are really
    checked in tests/test_gpu_attn_dense.py::test_logits_bwd_arbitrary_dA, under a dA that is no softmax gradient
    (db = sum(dA), |db| > 1)."""
    from fvta_memexqa_amd import ops
    from oracle import fvta_fused as F
    dev = ops.require_gpu()
    g = torch.Generator().manual_seed(11)
    N, V, JQ, w = 4, 9, 7, 64
    nf = {1: 3, 2: 2, 3: 4}[simi]
    h = torch.randn(N, V, w, generator=g)
    q = torch.randn(N, JQ, w, generator=g)
    W = torch.randn(nf * w, 1, generator=g) * 0.1
    b = torch.randn(1, generator=g) * 0.1
    hm = (torch.rand(N, V, generator=g) > 0.3) if masked else None
    qm = (torch.rand(N, JQ, generator=g) > 0.3) if masked else None
    if masked:
        hm[:, 0] = True
        qm[:, 0] = True
        # (no batch row without ANY valid context row: fvta_attn_bwd passes no gradient into the logits of a fully masked
        # (n, k), DESIGN.md section 2 deviation (b); masked context rows -- uniform over the question -- are covered)
    hr, qr, Wr, br = (t.double().requires_grad_() for t in (h, q, W, b))
    ref, _ = F.attention(hr, qr, Wr, br, hm, qm, simiMatrix=simi, feat_order="v1", bidirect=True)
    go = torch.randn(N, 2 * w, generator=g)
    ref.backward(go.double())
    hd, qd, Wd, bd = (t.to(dev).contiguous() for t in (h, q, W.reshape(-1), b))
    hmd = hm.to(torch.uint8).to(dev) if masked else None
    qmd = qm.to(torch.uint8).to(dev) if masked else None
    op = ops.FocalAttention(N, 1, V, JQ, w, simi, False, feat_order=1)
    h_a, lg = op.forward(hd, qd, hmd, qmd, Wd, bd, True)
    q_a = torch.empty(N, w, device=dev)
    ops.attn_qside_fwd(lg, qd, q_a, N, V, JQ, w)
    torch.testing.assert_close(torch.cat([h_a, q_a], 1).cpu().double(), ref.detach(), rtol=1e-4, atol=1e-5)
    god = go.to(dev)
    d_h, d_q = torch.zeros(N, V, w, device=dev), torch.zeros(N, JQ, w, device=dev)
    dW, db = torch.zeros(nf * w, device=dev), torch.zeros(1, device=dev)
    op.backward(hd, qd, hmd, qmd, Wd, bd, god[:, :w].contiguous(), d_h, d_q, dW, db, accumulate=0)
    dA = torch.empty(N, V, JQ, device=dev)
    ops.attn_qside_bwd(lg, qd, god[:, w:].contiguous(), dA, d_q, N, V, JQ, w)
    op.logits_bwd(hd, qd, Wd, dA, d_h, d_q, dW, db)
    torch.testing.assert_close(d_h.cpu().double(), hr.grad, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(d_q.cpu().double(), qr.grad, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(dW.cpu().double(), Wr.grad.reshape(-1), rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(db.cpu().double(), br.grad, rtol=2e-4, atol=2e-5)


def test_blocked_linear_wsum_softmax_backward():
    """the _blk / _ld forms on one stream of an [N][all streams] arena, and fvta_softmax_bwd / fvta_wsum_bwd, vs autograd"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    g = torch.Generator().manual_seed(4)
    N, V, off, Vtot, w, dout = 3, 11, 5, 23, 48, 20
    arena = torch.randn(N, Vtot, w, generator=g).to(dev)
    W = (torch.randn(w, dout, generator=g) * 0.2).to(dev)
    b = torch.randn(dout, generator=g).to(dev)
    xs = arena[:, off:off + V]
    y = torch.empty(N * V, dout, device=dev)
    ops.linear_fwd(arena.view(-1)[off * w:], W, b, y, N * V, w, dout, blk=(V, Vtot * w))
    torch.testing.assert_close(y.view(N, V, dout), xs @ W + b, rtol=1e-5, atol=1e-5)
    dy = torch.randn(N * V, dout, generator=g).to(dev)
    d_arena = torch.ones(N, Vtot, w, device=dev)
    dW, db = torch.zeros(w, dout, device=dev), torch.zeros(dout, device=dev)
    ops.linear_bwd(arena.view(-1)[off * w:], W, None, dy, d_arena.view(-1)[off * w:], dW, db, N * V, w, dout, accumulate_dx=True,
                   blk=(V, Vtot * w))
    want = torch.ones(N, Vtot, w, device=dev)
    want[:, off:off + V] += (dy @ W.t()).view(N, V, w)
    torch.testing.assert_close(d_arena, want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dW, xs.reshape(-1, w).t() @ dy, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db, dy.sum(0), rtol=1e-5, atol=1e-5)
    # softmax backward
    x = torch.randn(N, V, generator=g).to(dev)
    p = torch.empty_like(x)
    ops.softmax_fwd(x, p, N, V)
    dp = torch.randn(N, V, generator=g).to(dev)
    dx = torch.empty_like(x)
    ops.softmax_bwd(p, dp, dx, N, V)
    xr = x.double().cpu().requires_grad_()
    torch.softmax(xr, -1).backward(dp.double().cpu())
    torch.testing.assert_close(dx.cpu().double(), xr.grad, rtol=1e-5, atol=1e-6)
    # weighted sum over the stream's rows and its backward
    out = torch.empty(N, w, device=dev)
    ops.wsum_fwd(arena.view(-1)[off * w:], p, out, N, V, w, target_ld=Vtot * w)
    torch.testing.assert_close(out, (xs * p[..., None]).sum(1), rtol=1e-5, atol=1e-5)
    go = torch.randn(N, w, generator=g).to(dev)
    dwt = torch.empty(N, V, device=dev)
    d_arena = torch.zeros(N, Vtot, w, device=dev)
    ops.wsum_bwd(arena.view(-1)[off * w:], p, go, dwt, d_arena.view(-1)[off * w:], N, V, w, target_ld=Vtot * w)
    torch.testing.assert_close(dwt, (xs * go[:, None, :]).sum(-1), rtol=1e-5, atol=1e-5)
    want = torch.zeros(N, Vtot, w, device=dev)
    want[:, off:off + V] = p[..., None] * go[:, None, :]
    torch.testing.assert_close(d_arena, want, rtol=1e-5, atol=1e-6)
