"""Focal attention at LARGE BATCH against the fp64 oracle: the regimes of attn_shape() (csrc/attn_common.h) that the
other kernel tests, all at N <= 8, never reach.

  * grouped backward (gk > 1: N*K >= 1024, T <= 512, bsplit == 1): one workgroup of attn_bwd_main takes gk consecutive
    streams of an album -- concatenated row lists, one LDS sort, one dQs slab, per-stream scalars picked by t / T; a short
    last group; the sort exactly full at gk * T == 1024; the slab folds over ng * bsplit * RH slots;
  * forward planning at large batch: nsplit at its floor, one workgroup per album (G = 1) dealt every item of the album,
    the plain deal on ragged albums (N > 64: no balance table);
  * the write modes of d_hinfo the models use (accumulate = 2 and 3, the latter also under time_warp_att);
  * the shadow-row backward (bf16 half-rows through an address table) under the grouped plan.

Every test first asserts the plan it means to exercise, read from the library (fvta_attn_plan), so that a retuned
threshold cannot silently move a shape out of the regime.  Each check prints its measured maximum error (pytest -s).

Masks: _att_case's, with the two fix-ups of test_attention_3d_backward_matches_autograd (an album whose question is
fully masked passes gradient into its masked logits in TF / the oracle and not in the kernels: DESIGN.md).  A fully
masked STREAM beside a live one is no such case -- its weight in the softmax over k is exp(-1e30 - M) = 0 exactly, in
fp64 as in fp32, so every gradient through it vanishes on both sides -- and one is planted inside a group (hm[1, 1]),
rows left non-zero: the kernel walks all T rows of it with that stream's own scalars."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (N, K, T, JQ, w), simi, tanh, masked, the plan {nsplit, bsplit, gk, ng} the case is there for
CASES = {
    # even groups, G = 1, attn_bwd_prep with 256 threads
    "gk2_w64": ((256, 4, 24, 5, 64), 1, False, True, (1, 1, 2, 2)),
    # last group short (3 + 2), prep with 1024 threads (K > 4)
    "gk3_short_w128": ((320, 5, 16, 6, 128), 3, True, True, (1, 1, 3, 2)),
    # cosine variant, attn_bwd_cosine_q_kernel over ng * RH slots
    "gk3_cosine_w128": ((320, 5, 16, 6, 128), 4, False, False, (1, 1, 3, 2)),
    # gk * T == 1024: the LDS sort exactly full (unmasked: every row is listed)
    "gk2_full_sort_w64": ((512, 2, 512, 2, 64), 2, True, False, (3, 1, 2, 1)),
    # w = 512 tile, short last group (2 + 1), pair16 forward with G = 1, N > 64 masked (no balance table)
    "gk2_short_w512": ((342, 3, 12, 4, 512), 2, True, True, (1, 1, 2, 2)),
    # w = 1024 tile (RH = 1), pair16 forward with G = 1
    "gk2_w1024": ((256, 4, 8, 3, 1024), 2, True, True, (1, 1, 2, 2)),
    # ungrouped, one workgroup per stream; keeps _att_case's fully masked stream hm[0, 0] (modes 2 / 3 write all of its rows)
    "small": ((3, 3, 50, 10, 64), 2, True, True, (1, 1, 1, 3)),
}


def _close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    """tests/test_gpu_backward.py's _close (atol relative to the reference's scale), printing what it measured"""
    from tests.test_gpu_backward import _close as close
    err = float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max()) if a.numel() else 0.0
    print("  %-28s max |err| %.3e   |ref|max %.3e" % (msg, err, float(b.detach().abs().max()) if b.numel() else 0.0))
    close(a, b, rtol=rtol, atol=atol, msg=msg)


def _oracle(h, q, W, b, hm, qm, simi, tanh, gout, scale=None, dtype=torch.float64, chunk=64):
    """attention_3d + autograd in `dtype`, album slice by album slice (albums are independent; W and b are shared leaves
    whose .grad accumulates over the slices): h_a and the gradients of sum(h_a * gout)"""
    from oracle import fvta_fused as F
    N = h.shape[0]
    Wd = None if W is None else W.to(dtype).requires_grad_()
    bd = None if b is None else b.to(dtype).requires_grad_()
    out = dict(ha=[], dh=[], dq=[], dsc=[])
    for n0 in range(0, N, chunk):
        sl = slice(n0, min(N, n0 + chunk))
        hd, qd = h[sl].to(dtype).requires_grad_(), q[sl].to(dtype).requires_grad_()
        kw = {}
        if scale is not None:
            sd = scale[sl].to(dtype).requires_grad_()
            kw = dict(time_warp_att=True, C=torch.diag_embed(sd))          # [n,T,T] with row sums = scale
        ha, _ = F.attention_3d(hd, qd, Wd, bd, None if hm is None else hm[sl], None if qm is None else qm[sl],
                               simiMatrix=simi, add_tanh=tanh, **kw)
        (ha * gout[sl].to(dtype)).sum().backward()
        out["ha"].append(ha.detach())
        out["dh"].append(hd.grad)
        out["dq"].append(qd.grad)
        if scale is not None:
            out["dsc"].append(sd.grad)
    res = {k: torch.cat(v) for k, v in out.items() if v}
    res["dW"] = None if Wd is None else Wd.grad.reshape(-1)
    res["db"] = None if bd is None else bd.grad
    return res


ARGMAX_GAP = 2e-4


def _settle_argmax(h, q, W, b, hm, qm, simi, tanh, seed, post=lambda rows: rows, chunk=64):
    """Makes the two arg-max decisions of attention_3d unambiguous, in place.  The gradient is discontinuous in them: the
    max over question positions sends a row's gradient to ONE position, the max over a stream's rows sends the stream's
    softmax-over-k gradient to ONE row.  Where the two leading logits lie closer than the kernels' fp32 rounding, kernel
    and fp64 oracle may pick different ones and differ by O(1) in that row -- no error of either.  Among a few rows that
    does not happen; among the 5e5 rows of these shapes it does (the oracle ITSELF evaluated in float32 misses the
    tolerances on such inputs).  So every valid row whose two leading logits over j, and every stream whose two leading
    rows, lie closer than ARGMAX_GAP = 10 x the absolute tolerance the project holds its logits to (2e-5,
    test_attention_3d_forward_matches_oracle) is drawn again until none is left."""
    from oracle import fvta_fused as F
    N, K, T, w = h.shape
    g = torch.Generator().manual_seed(seed)
    dd = lambda t: None if t is None else t.double()
    for _ in range(20):
        near = []
        with torch.no_grad():
            for n0 in range(0, N, chunk):
                sl = slice(n0, min(N, n0 + chunk))
                a = F.simi_logits(dd(h[sl]), dd(q[sl])[:, None], dd(W), dd(b), simi, tanh)            # [n,K,T,JQ]
                rows = torch.ones(a.shape[:3], dtype=torch.bool)
                if hm is not None:
                    a = F.exp_mask(a, hm[sl][..., None] & qm[sl][:, None, None, :])
                    rows = hm[sl] & qm[sl].any(1)[:, None, None]
                top = a.topk(min(2, a.shape[-1]), -1).values
                bad = rows & (top[..., 0] - top[..., -1] < ARGMAX_GAP) if a.shape[-1] > 1 else torch.zeros_like(rows)
                amax = torch.where(rows, top[..., 0], torch.full_like(top[..., 0], -float("inf")))
                if T > 1:
                    t2 = amax.topk(2, -1)
                    close_t = (t2.values[..., 0] - t2.values[..., 1] < ARGMAX_GAP) & torch.isfinite(t2.values[..., 1])
                    bad |= torch.zeros_like(rows).scatter_(2, t2.indices[..., 1:], close_t[..., None])
                near.append(bad)
        near = torch.cat(near)
        if not near.any():
            return
        h[near] = post(torch.randn(int(near.sum()), w, generator=g) * 0.5)
    raise AssertionError("arg-max positions still ambiguous")


def _case(name):
    """inputs + fp64 reference of a case; the two cases that more than one test uses are built once and never written to"""
    return _case_shared(name) if name in ("gk2_w64", "small") else _case_build(name)


@functools.lru_cache(maxsize=None)
def _case_shared(name):
    return _case_build(name)


def _case_build(name):
    from tests.test_gpu_forward import _att_case
    (N, K, T, JQ, w), simi, tanh, masked, _ = CASES[name]
    h, q, W, b, hm, qm = _att_case(N, K, T, JQ, w, simi, tanh, masked, seed=N * 100 + T + w + simi + 1)
    if masked:
        qm[N - 1, :2] = True          # no album with a fully masked question (see the module docstring)
        if name != "small":
            hm[0, 0, :3] = True
            hm[1, 1] = False          # a stream without a valid row inside a group, beside live ones
    _settle_argmax(h, q, W, b, hm, qm, simi, tanh, seed=N + T)
    gout = torch.randn(N, w, generator=torch.Generator().manual_seed(99))
    ref = _oracle(h, q, W, b, hm, qm, simi, tanh, gout)
    return dict(h=h, q=q, W=W, b=b, hm=hm, qm=qm, gout=gout, ref=ref)


def _assert_plan(op, masked, want, what):
    p = op.plan(masked)
    assert (p["nsplit"], p["bsplit"], p["gk"], p["ng"]) == tuple(want), "%s: fvta_attn_plan says %r, the case is there for %r" % (what, p, want)


def _device_args(c):
    from fvta_memexqa_amd import ops
    cu = lambda t: None if t is None else t.cuda().contiguous()
    return (cu(c["h"]), cu(c["q"]), cu(ops.as_mask_u8(c["hm"])), cu(ops.as_mask_u8(c["qm"])),
            None if c["W"] is None else cu(c["W"].reshape(-1)), cu(c["b"])), cu(c["gout"])


def _row_sets(hmc, qmc, N, K, T):
    """(valid, dead, written) [N,K,T] on the device: dead = masked rows of live streams (zeros under modes 0 / 3), written
    = the rows mode 2 stores: valid rows, and every row of a stream without a valid (t, j) pair (uniform over all T)"""
    valid = hmc.view(N, K, T).bool()
    qany = qmc.view(N, -1).bool().any(1).view(N, 1, 1)
    allm = ~valid.any(2, keepdim=True) | ~qany
    return valid, (~valid & ~allm), (valid | allm).expand_as(valid)


def _grads(args, fill_h, fill_q):
    hc, qc, _, _, Wc, _ = args
    return [torch.full_like(hc, fill_h), torch.full_like(qc, fill_q), None if Wc is None else torch.zeros_like(Wc),
            None if Wc is None else torch.zeros(1, device="cuda")]


@pytest.mark.parametrize("name", [n for n in CASES if n != "small"])
def test_large_batch_forward_backward_match_oracle(name, attn_select):
    """h_a; the overwrite mode into NaN-filled d_hinfo / d_hq (a row the kernel missed stays NaN, a masked row of a live
    stream must come back exactly 0); the accumulate mode on top of 1.0 (dW, db accumulate: twice the oracle's); and the
    exact-fp32 forward kernel (launch_main at nsplit == 1) where it is not what ran by default."""
    from fvta_memexqa_amd import ops
    (N, K, T, JQ, w), simi, tanh, masked, plan = CASES[name]
    op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
    _assert_plan(op, masked, plan, name)
    c = _case(name)
    ref = c["ref"]
    args, g = _device_args(c)
    print("\n%s  N %d K %d T %d JQ %d w %d simi %d" % (name, N, K, T, JQ, w, simi))
    ha, _ = op.forward(*args)
    _close(ha, ref["ha"], msg="h_a")

    def params(dW, db, times, atol):
        if dW is not None:
            _close(dW, times * ref["dW"], atol=atol, msg="dW x%d" % times)
            _close(db, times * ref["db"], atol=atol, msg="db x%d" % times)

    dh, dq, dW, db = _grads(args, float("nan"), float("nan"))
    op.backward(*args, g, dh, dq, dW, db, accumulate=0)
    assert torch.isfinite(dh).all() and torch.isfinite(dq).all(), "rows left unwritten"
    _close(dh, ref["dh"], msg="d_hinfo")
    _close(dq, ref["dq"], msg="d_hq")
    params(dW, db, 1, 1e-5)
    if masked:
        _, dead, _ = _row_sets(args[2], args[3], N, K, T)
        assert dead.any() and float(dh[dead].abs().max()) == 0.0, "masked rows of a live stream are not exactly zero"
    del dh
    dh1, dq1, _, _ = _grads(args, 1.0, 1.0)
    op.backward(*args, g, dh1, dq1, dW, db, accumulate=1)
    dh1 -= 1.0
    _close(dh1, ref["dh"], atol=2e-5, msg="d_hinfo accumulate")
    _close(dq1 - 1.0, ref["dq"], atol=2e-5, msg="d_hq accumulate")
    params(dW, db, 2, 3e-5)
    del dh1
    if w in (64, 128, 1024):
        attn_select.exact()
        ha_exact, _ = op.forward(*args)
        _close(ha_exact, ref["ha"], msg="h_a (exact-fp32 kernel)")


@pytest.mark.parametrize("name", ["gk2_w64", "small"])
def test_write_modes_2_and_3_match_oracle(name):
    """accumulate = 2 (the fused model's: plain stores to the rows of the compacted lists, everything else untouched, d_hq
    accumulated) and 3 (the time-warp model's: d_hinfo overwritten, zeros on masked rows, d_hq accumulated) against
    mode 0 of the same call sequence -- the same kernel instantiation: bitwise -- and against the oracle."""
    from fvta_memexqa_amd import ops
    (N, K, T, JQ, w), simi, tanh, masked, plan = CASES[name]
    op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
    _assert_plan(op, masked, plan, name)
    c = _case(name)
    ref = c["ref"]
    args, g = _device_args(c)
    print("\n%s  N %d K %d T %d JQ %d w %d simi %d" % (name, N, K, T, JQ, w, simi))
    valid, dead, written = _row_sets(args[2], args[3], N, K, T)
    assert dead.any() and (written & ~valid).any()          # both kinds of masked rows occur
    op.forward(*args)
    d0, dq0, dW0, db0 = _grads(args, float("nan"), float("nan"))
    op.backward(*args, g, d0, dq0, dW0, db0, accumulate=0)
    assert torch.isfinite(d0).all()
    _close(dq0, ref["dq"], msg="d_hq (mode 0)")
    # mode 2
    op.forward(*args)
    d2, dq2, dW2, db2 = _grads(args, 5.0, 1.0)
    op.backward(*args, g, d2, dq2, dW2, db2, accumulate=2)
    assert bool((d2[~written] == 5.0).all()), "mode 2 wrote a masked row of a live stream"
    assert torch.equal(d2[written], d0[written]), "mode 2: written rows differ from mode 0's"
    if name != "small":
        _close(d2[written], ref["dh"].cuda()[written], msg="d_hinfo (mode 2, written rows)")
    _close(dq2 - 1.0, ref["dq"], atol=2e-5, msg="d_hq (mode 2) - prefill")
    _close(dW2, ref["dW"], msg="dW (mode 2)")
    # mode 3
    op.forward(*args)
    d3, dq3, dW3, db3 = _grads(args, float("nan"), 1.0)
    op.backward(*args, g, d3, dq3, dW3, db3, accumulate=3)
    assert torch.isfinite(d3).all(), "mode 3 left rows unwritten"
    assert float(d3[dead].abs().max()) == 0.0, "mode 3: masked rows of a live stream are not exactly zero"
    assert torch.equal(d3, d0), "mode 3 differs from mode 0"
    _close(dq3 - 1.0, ref["dq"], atol=2e-5, msg="d_hq (mode 3) - prefill")
    _close(dW3, ref["dW"], msg="dW (mode 3)")


@pytest.mark.parametrize("N,K,T,JQ,w,plan", [(3, 3, 40, 5, 64, (1, 1, 1, 3)), (256, 4, 24, 5, 64, (1, 1, 2, 2))])
def test_write_mode_3_under_time_warp_att(N, K, T, JQ, w, plan):
    """The time-warp model's call: accumulate = 3 with tscale (negative scales: masked rows take the softmax, and
    attn_bwd_pad_kernel adds their direct term to rows mode 3 has zeroed), into a NaN-filled d_hinfo, a prefilled d_hq
    and a prefilled d_tscale (accumulated into) -- every gradient against the fp64 oracle, ungrouped and grouped."""
    from fvta_memexqa_amd import ops
    from tests.test_gpu_timewarp import _close as close_tw, _tw_att_case
    simi, tanh = 2, True
    op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
    _assert_plan(op, True, plan, "time_warp_att N %d" % N)
    h, q, W, b, hm, qm, scale = _tw_att_case(N * 7 + T, N, K, T, JQ, w, simi, tanh, True, False)
    _settle_argmax(h, q, W, b, hm, qm, simi, tanh, seed=N + T)
    gout = torch.randn(N, w, generator=torch.Generator().manual_seed(5))
    ref = _oracle(h, q, W, b, hm, qm, simi, tanh, gout, scale=scale)
    assert (scale < 0).any() and not hm.all()
    cu = lambda t: t.float().cuda().contiguous()
    hd, qd, Wd, bd, sd = cu(h), cu(q), cu(W).reshape(-1), cu(b), cu(scale)
    hmd, qmd = ops.as_mask_u8(hm).cuda(), ops.as_mask_u8(qm).cuda()
    print("\ntime_warp_att  N %d K %d T %d JQ %d w %d" % (N, K, T, JQ, w))

    def close(a, r, rtol, atol, what):
        a, r = a.detach().cpu().double(), r.detach().cpu().double()
        print("  %-28s max |err| %.3e   |ref|max %.3e" % (what, float((a - r).abs().max()), float(r.abs().max())))
        close_tw(a, r, rtol=rtol, atol=atol)

    ha, _ = op.forward(hd, qd, hmd, qmd, Wd, bd, tscale=sd)
    close(ha, ref["ha"], 1e-4, 2e-5, "h_a")
    d_h, d_q = torch.full_like(hd, float("nan")), torch.ones_like(qd)
    dW, db, dsc = torch.zeros_like(Wd), torch.zeros_like(bd), torch.full_like(sd, 0.25)
    op.backward(hd, qd, hmd, qmd, Wd, bd, cu(gout), d_h, d_q, dW, db, accumulate=3, tscale=sd, d_tscale=dsc)
    assert torch.isfinite(d_h).all(), "mode 3 left rows unwritten"
    close(d_h, ref["dh"], 2e-4, 2e-5, "d_hinfo")
    close(d_q - 1.0, ref["dq"], 2e-4, 2e-5, "d_hq - prefill")
    close(dW, ref["dW"], 2e-4, 2e-5, "dW")
    close(db, ref["db"], 2e-4, 2e-5, "db")
    # d scale: rows that take the whole softmax carry 0 * 1e30-scale terms; compare where the oracle's is finite and sane
    gs = ref["dsc"]
    ok = gs.abs() < 1e6
    assert ok.any()
    close((dsc.cpu().double() - 0.25)[ok], gs[ok], 2e-4, 2e-5, "d_tscale - prefill")


def test_shadow_rows_under_the_grouped_backward(attn_select):
    """forward_shadow / backward_shadow (modes 0 and 2) at gk == 2 -- the shadow variant indexes its address table with
    the group's flat row -- against forward / backward on the bf16-rounded fp32 rows under the exact-fp32 kernel, which
    test_large_batch_forward_backward_match_oracle ties to the oracle at this N*K."""
    from fvta_memexqa_amd import ops
    from tests.test_gpu_forward import _att_case
    from tests.test_gpu_shadow import _close as close_sh, _shadow_table
    N, K, T, JQ, w, simi, tanh = 256, 4, 8, 3, 512, 2, True
    op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
    assert op.plan(True)["gk"] == 2 and op.plan(True)["bsplit"] == 1, op.plan(True)
    h, q, W, b, hm, qm = _att_case(N, K, T, JQ, w, simi, tanh, True, seed=8512)
    hm[1, 1] = False                                            # a stream without a valid row inside a group
    rounded = lambda rows: rows.clamp(-1, 1).bfloat16().float()   # encoder outputs lie in (-1, 1)
    h = rounded(h)
    _settle_argmax(h, q, W, b, hm, qm, simi, tanh, seed=8512, post=rounded)   # (the two forward kernels round their logits differently)
    cu = lambda t: t.cuda().contiguous()
    hmu = cu(ops.as_mask_u8(hm))
    hb = cu(h).bfloat16() * hmu.view(N, K, T, 1).to(torch.bfloat16)               # zero rows where masked
    zero_rows = (hmu.view(-1) == 0).nonzero().view(-1)
    table, keep = _shadow_table(hb.view(N * K * T, w), zero_rows, 8512)
    h32 = hb.float().contiguous()
    rest = (cu(q), hmu, cu(ops.as_mask_u8(qm)), cu(W.reshape(-1)), cu(b))
    g = torch.randn(N, w, generator=torch.Generator().manual_seed(3)).cuda()
    mk = lambda fh, fq: [torch.full((N, K, T, w), fh, device="cuda"), torch.full((N, JQ, w), fq, device="cuda"),
                         torch.zeros_like(rest[3]), torch.zeros(1, device="cuda")]
    sh = op.forward_shadow(table, *rest)
    grads_sh = mk(float("nan"), float("nan"))
    op.backward_shadow(table, *rest, g, *grads_sh, accumulate=0)
    assert torch.isfinite(sh).all() and torch.isfinite(grads_sh[0]).all() and torch.isfinite(grads_sh[1]).all(), "rows left unwritten"
    op.forward_shadow(table, *rest)
    d2, dq2, dW2, db2 = mk(5.0, 0.0)
    op.backward_shadow(table, *rest, g, d2, dq2, dW2, db2, accumulate=2)
    attn_select.exact()
    exact, _ = op.forward(h32, *rest)
    grads_ex = mk(float("nan"), float("nan"))
    op.backward(h32, *rest, g, *grads_ex, accumulate=0)

    def close(a, r, rtol, atol, what):
        print("  %-28s max |err| %.3e   |ref|max %.3e" % (what, float((a - r).abs().max()), float(r.abs().max())))
        close_sh(a, r, rtol=rtol, atol=atol, msg=what)

    print("\nshadow rows, grouped  N %d K %d T %d JQ %d w %d" % (N, K, T, JQ, w))
    close(sh, exact, 5e-5, 5e-6, "h_a")
    for name, a_, b_ in zip(("d_hinfo", "d_hq", "dW", "db"), grads_sh, grads_ex):
        close(a_, b_, 2e-4, 2e-5 * max(1.0, float(b_.abs().max())), name + " (mode 0)")
    valid, dead, written = _row_sets(hmu, rest[2], N, K, T)
    assert dead.any() and (written & ~valid).any()
    assert bool((d2[~written] == 5.0).all()), "masked rows written under accumulate=2"
    assert torch.equal(d2[written], grads_sh[0][written]), "mode 2: written rows differ from mode 0's"
    close(d2[written], grads_ex[0][written], 2e-4, 2e-5 * max(1.0, float(grads_ex[0].abs().max())), "d_hinfo (mode 2, written rows)")
    for name, a_, b_ in zip(("d_hq", "dW", "db"), (dq2, dW2, db2), grads_ex[1:]):
        close(a_, b_, 2e-4, 2e-5 * max(1.0, float(b_.abs().max())), name + " (mode 2)")
