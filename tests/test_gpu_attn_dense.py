"""The reversed ("bidirect") half of the 1-D attentions (csrc/attn_dense.hip, csrc/attn_bwd_shared.h) and the stand-alone
helpers the fallback route chains together (csrc/elementwise.hip, fvta_softsel_bwd), at the shapes where their loops turn
over and their LDS tiles fill up -- the other tests reach them at one small shape each (w <= 128, V * JQ <= 66).

  1. fvta_attn_logits_bwd under an ARBITRARY dA (no softmax gradient, so db = sum(dA) is far from zero: the pb[n] fold
     across the four waves and the `db[0] += acc` of the params kernel are checked against a real number), against autograd
     of the fp64 oracle's simi_logits; accumulate contract on all four outputs; one stream of a wider arena (hinfo_stride);
  2. fvta_attn_qside_fwd / _bwd on logits with fully masked rows and columns, against fp64 torch;
  3. both sides of the route switch in functional.bidirect_q_a (fused backward / each launch's own);
  4. fvta_softmax_bwd, fvta_wsum_fwd_ld, fvta_wsum_bwd, softsel forward and backward where their strided loops wrap;
  5. the refusals: a shape above a kernel's limit is turned away on the host and no output is touched.

Every case asserts the property it was chosen for, so that a later change of the limits cannot silently move it to
another branch, and every kernel result is produced twice and must come out bitwise equal (fixed summation orders).

Tolerances are the ones these ops carry in tests/test_gpu_v1_ops.py: forward rtol 1e-4 / atol 1e-5, gradients rtol 2e-4 /
atol 2e-5, atol of the parameter gradients scaled by max(1, max |ref|).  Every check prints the fraction of its tolerance
it used (pytest -s).  A case that needs more gets max(that tolerance, 4 x the error of the float32 reference against the
float64 one), entered in F32_REF_FRACTION with the measured figure; none did."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD = dict(rtol=1e-4, atol=1e-5)
GRAD = dict(rtol=2e-4, atol=2e-5)
NEG = -1e30                     # what exp_mask leaves in a masked logit (fp32: val + -1e30 == -1e30)
DENSE_MAX, ROWS_MAX = 8192, 2048   # csrc/attn_dense.hip: the V * JQ LDS tile, s_rs
# (check name) -> fraction of its tolerance the float32 reference itself uses against float64, where 4 x that exceeds 1
F32_REF_FRACTION = {}


def _fraction(got, ref, rtol, atol, scale=False):
    """max over elements of |got - ref| / (atol [* max(1, max |ref|)] + rtol |ref|); NaN / inf in `got` count as inf"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    a = atol * (max(1.0, float(ref.abs().max())) if scale else 1.0)
    return float(((got - ref).abs() / (a + rtol * ref.abs())).max())


class _Checks:
    """collects every comparison of a test before failing, so that one run shows all figures"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def close(self, name, got, ref, tol, scale=False):
        f = _fraction(got, ref, scale=scale, **tol)
        allowed = max(1.0, 4.0 * F32_REF_FRACTION.get("%s:%s" % (self.case, name), 0.0))
        print("  %-34s %-8s uses %.3f of its tolerance (|ref|max %.3e)" % (self.case, name, f, float(ref.abs().max())))
        if not f <= allowed:
            self.bad.append("%s: %.3f > %.3f" % (name, f, allowed))

    def equal(self, name, a, b):
        if not torch.equal(a, b):
            self.bad.append("%s: not bitwise equal" % name)

    def done(self):
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))


# ------------------------------------------------------------------------------------------ 1. fvta_attn_logits_bwd
# name: (N, T, JQ, w), simiMatrix, feat_order, the branch the shape is there for
LOGITS_CASES = {
    "tile_full": ((3, 128, 64, 512), 3, 0, lambda N, T, JQ, w: T * JQ == DENSE_MAX and JQ == 64 and w == 2 * 256),
    "rows_full": ((2, 2048, 4, 64), 2, 1, lambda N, T, JQ, w: T == ROWS_MAX and T == 8 * 256 and T * JQ <= DENSE_MAX),
    "one_row": ((2, 1, 64, 1024), 1, 0, lambda N, T, JQ, w: T == 1 and JQ == 64 and w == 4 * 256),
    "one_question_token": ((2, 7, 1, 64), 2, 0, lambda N, T, JQ, w: JQ == 1),
    "rows_ragged": ((3, 300, 27, 256), 3, 1, lambda N, T, JQ, w: 256 < T < 512 and T % 256 != 0 and T * JQ <= DENSE_MAX),
    "five_partials": ((5, 130, 63, 128), 1, 1, lambda N, T, JQ, w: N > 4 and JQ == 63 and T * JQ <= DENSE_MAX),
}
FEAT_ORDER = {0: "v2", 1: "v1"}


def _logits_inputs(shape, simi, seed):
    N, T, JQ, w = shape
    g = torch.Generator().manual_seed(seed)
    nf = {1: 3, 2: 2, 3: 4}[simi]
    inp = dict(h=torch.randn(N, T, w, generator=g), q=torch.randn(N, JQ, w, generator=g),
               W=torch.randn(nf * w, generator=g) * 0.1,
               dA=torch.randn(N, T, JQ, generator=g) + 0.5)        # no softmax gradient: its sum is far from zero
    inp["pat"] = dict(dh=torch.randn(N, T, w, generator=g), dq=torch.randn(N, JQ, w, generator=g),
                      dW=torch.randn(nf * w, generator=g), db=torch.full((1,), 3.0))
    return inp


def _logits_ref(inp, simi, feat_order, dtype=torch.float64):
    """the gradients of sum(simi_logits * dA) by autograd in `dtype`"""
    from oracle import fvta_fused as F
    h, q, W = (inp[k].to(dtype).clone().requires_grad_() for k in ("h", "q", "W"))
    b = torch.zeros(1, dtype=dtype, requires_grad=True)
    a = F.simi_logits(h, q, W, b, simi, False, FEAT_ORDER[feat_order])
    (a * inp["dA"].to(dtype)).sum().backward()
    return dict(dh=h.grad, dq=q.grad, dW=W.grad, db=b.grad)


def _logits_run(op, inp, dev, hinfo=None, d_hinfo=None):
    """one fvta_attn_logits_bwd into buffers prefilled with the pattern; `hinfo` / `d_hinfo`: views into an arena"""
    pat = inp["pat"]
    dq, dW, db = (pat[k].to(dev) for k in ("dq", "dW", "db"))
    dh = pat["dh"].to(dev) if d_hinfo is None else d_hinfo
    op.logits_bwd(inp["h"].to(dev) if hinfo is None else hinfo, inp["q"].to(dev), inp["W"].to(dev), inp["dA"].to(dev),
                  dh, dq, dW, db)
    torch.cuda.synchronize()
    return dict(dh=dh, dq=dq, dW=dW, db=db)


def _logits_compare(ck, got, inp, ref):
    for k in ("dh", "dq", "dW", "db"):
        ck.close(k, got[k], inp["pat"][k].double() + ref[k], GRAD, scale=k in ("dW", "db"))


@pytest.mark.parametrize("case", sorted(LOGITS_CASES))
def test_logits_bwd_arbitrary_dA(case):
    """d_hinfo, d_hq, dW, db of sum(a_logits * dA) for a random dA, accumulated onto a non-zero pattern"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    shape, simi, fo, branch = LOGITS_CASES[case]
    N, T, JQ, w = shape
    assert branch(*shape), "the shape no longer reaches the branch it was chosen for"
    inp = _logits_inputs(shape, simi, seed=21)
    ref = _logits_ref(inp, simi, fo)
    assert abs(float(ref["db"])) > 1.0 and abs(float(ref["db"]) - float(inp["dA"].double().sum())) < 1e-9
    op = ops.FocalAttention(N, 1, T, JQ, w, simi, False, feat_order=fo)
    got, again = _logits_run(op, inp, dev), _logits_run(op, inp, dev)
    ck = _Checks("logits_bwd/" + case)
    _logits_compare(ck, got, inp, ref)
    for k in got:
        ck.equal(k + " (second run)", got[k], again[k])
    ck.done()


def test_logits_bwd_on_a_stream_of_the_arena():
    """hinfo_stride != 0 with a non-trivial dA (as model.py calls it): bitwise the dense call on the gathered copy, and the
    arena's rows outside the stream stay bitwise untouched"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    (N, V, JQ, w), off, Vtot, simi, fo = (3, 37, 9, 64), 11, 70, 2, 1
    inp = _logits_inputs((N, V, JQ, w), simi, seed=22)
    g = torch.Generator().manual_seed(23)
    arena = torch.randn(N, Vtot, w, generator=g)
    arena[:, off:off + V] = inp["h"]
    base = torch.randn(N, Vtot, w, generator=g)
    base[:, off:off + V] = inp["pat"]["dh"]
    arena = arena.to(dev)
    op_d = ops.FocalAttention(N, 1, V, JQ, w, simi, False, feat_order=fo)
    op_s = ops.FocalAttention(N, 1, V, JQ, w, simi, False, feat_order=fo, hinfo_stride=Vtot * w)
    assert op_s.desc.hinfo_stride == Vtot * w != V * w
    dense = _logits_run(op_d, inp, dev)
    ck = _Checks("logits_bwd/arena_stream")
    _logits_compare(ck, dense, inp, _logits_ref(inp, simi, fo))
    for _ in range(2):
        d_arena = base.to(dev)
        got = _logits_run(op_s, inp, dev, hinfo=arena.view(-1)[off * w:], d_hinfo=d_arena.view(-1)[off * w:])
        ck.equal("d_hinfo of the stream", d_arena[:, off:off + V].contiguous(), dense["dh"])
        ck.equal("arena rows before the stream", d_arena[:, :off].cpu(), base[:, :off])
        ck.equal("arena rows behind the stream", d_arena[:, off + V:].cpu(), base[:, off + V:])
        for k in ("dq", "dW", "db"):
            ck.equal(k, got[k], dense[k])
    ck.done()


# ----------------------------------------------------------------------------------- 2. fvta_attn_qside_fwd / _bwd
# name: (R, V, JQ, w), the branch the shape is there for
QSIDE_CASES = {
    "tile_full": ((3, 128, 64, 320), lambda R, V, JQ, w: V * JQ == DENSE_MAX and JQ == 64 and w % 256 != 0 and w > 256),
    "rows_2048": ((2, 2048, 4, 64), lambda R, V, JQ, w: V == 2048 and V * JQ == DENSE_MAX),
    "one_row": ((2, 1, 64, 512), lambda R, V, JQ, w: V == 1 and JQ == 64 and w == 2 * 256),
    "one_question_token": ((2, 7, 1, 64), lambda R, V, JQ, w: JQ == 1 and V % 4 != 0),
    "ragged": ((3, 300, 27, 256), lambda R, V, JQ, w: V * JQ <= DENSE_MAX and 0 < JQ < 64),
    "five_rows": ((5, 130, 63, 128), lambda R, V, JQ, w: R > 4 and V % 4 != 0 and JQ == 63),
}


@functools.lru_cache(maxsize=None)
def _qside_inputs(shape, seed=31):
    """random logits with rows and columns exp-masked as attention() leaves them; d_q_a scaled by V / sqrt(w), so that dA
    (which carries 1 / V) stays O(1) and the absolute tolerance does not swallow it"""
    R, V, JQ, w = shape
    g = torch.Generator().manual_seed(seed)
    hm = torch.rand(R, V, generator=g) > 0.3
    qm = torch.rand(R, JQ, generator=g) > 0.3
    hm[:, 0] = True
    qm[:, 0] = True
    if V > 1:
        hm[:, 1] = False                                   # a fully masked row next to a valid one
    else:
        hm[0, 0] = False                                   # the only row fully masked: uniform over the question
    mask = hm[:, :, None] & qm[:, None, :]
    a = torch.randn(R, V, JQ, generator=g) * 2 + (1 - mask.float()) * NEG
    assert bool((a[~mask] == NEG).all()) and bool((a[:, 1 if V > 1 else 0] == NEG).all(-1).any())
    return dict(a=a, hq=torch.randn(R, JQ, w, generator=g), go=torch.randn(R, w, generator=g) * (V / w ** 0.5),
                pat=torch.randn(R, JQ, w, generator=g))


def _qside_ref(inp, dtype=torch.float64):
    """q_a = mean_v softmax(a[v, :]) @ hq and the gradients of sum(q_a * go), plain torch in `dtype`"""
    a, hq = (inp[k].to(dtype).clone().requires_grad_() for k in ("a", "hq"))
    q_a = torch.einsum("rj,rjc->rc", torch.softmax(a, -1).mean(1), hq)
    (q_a * inp["go"].to(dtype)).sum().backward()
    return dict(q_a=q_a.detach(), dA=a.grad, dq=hq.grad)


@functools.lru_cache(maxsize=None)
def _qside_ref64(shape):
    return _qside_ref(_qside_inputs(shape))


def _qside_run(inp, dev):
    from fvta_memexqa_amd import ops
    R, V, JQ = inp["a"].shape
    w = inp["hq"].shape[-1]
    a, hq, go = (inp[k].to(dev) for k in ("a", "hq", "go"))
    q_a = torch.full((R, w), float("nan"), device=dev)
    ops.attn_qside_fwd(a, hq, q_a, R, V, JQ, w)
    dA = torch.full((R, V, JQ), float("nan"), device=dev)           # overwritten
    dq = inp["pat"].to(dev)                                         # accumulated
    ops.attn_qside_bwd(a, hq, go, dA, dq, R, V, JQ, w)
    torch.cuda.synchronize()
    return dict(q_a=q_a, dA=dA, dq=dq)


@pytest.mark.parametrize("case", sorted(QSIDE_CASES))
def test_qside_forward_backward(case):
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    shape, branch = QSIDE_CASES[case]
    assert branch(*shape), "the shape no longer reaches the branch it was chosen for"
    inp, ref = _qside_inputs(shape), _qside_ref64(shape)
    got, again = _qside_run(inp, dev), _qside_run(inp, dev)
    ck = _Checks("qside/" + case)
    ck.close("q_a", got["q_a"], ref["q_a"], FWD)
    ck.close("dA", got["dA"], ref["dA"], GRAD)
    ck.close("d_hq", got["dq"], inp["pat"].double() + ref["dq"], GRAD)
    for k in got:
        ck.equal(k + " (second run)", got[k], again[k])
    ck.done()


# ------------------------------------------------------------------------ 3. the route switch of bidirect_q_a
def _graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


def _route_run(fn, inp, dev):
    a, hq = (inp[k].to(dev).requires_grad_() for k in ("a", "hq"))
    q_a = fn(a, hq)
    nodes = _graph_nodes(q_a)
    q_a.backward(inp["go"].to(dev))
    torch.cuda.synchronize()
    return dict(q_a=q_a.detach(), dA=a.grad, dq=hq.grad), nodes


def _is_fused(nodes):
    fused, chained = "_AttnQSideBackward" in nodes, "_WsumBackward" in nodes and "_SoftmaxBackward" in nodes
    assert fused != chained, nodes
    return fused


def _route_compare(ck, tag, got, ref):
    ck.close(tag + " q_a", got["q_a"], ref["q_a"], FWD)
    ck.close(tag + " dA", got["dA"], ref["dA"], GRAD)
    ck.close(tag + " d_hq", got["dq"], ref["dq"], GRAD)


@pytest.mark.parametrize("inside,outside,w", [((2, 5, 64), (2, 5, 65), 64), ((2, 128, 64), (2, 130, 64), 64),
                                              ((2, 128, 64), (2, 130, 64), 320)])
def test_bidirect_q_a_route_switch(inside, outside, w):
    """functional.bidirect_q_a on each side of JQ <= 64 and of V * JQ <= 8192: the fused backward (fvta_attn_qside_bwd)
    inside, each launch's own backward outside, both against fp64 torch; and the chained route on the inside inputs agrees
    with the fused one"""
    from fvta_memexqa_amd import functional, ops
    dev = ops.require_gpu()
    ck = _Checks("route/%s|%s/w%d" % ("x".join(map(str, inside)), "x".join(map(str, outside)), w))
    assert inside[2] <= 64 and inside[1] * inside[2] <= DENSE_MAX
    assert outside[2] == 65 or outside[1] * outside[2] > DENSE_MAX
    inp_in, inp_out = _qside_inputs(inside + (w,)), _qside_inputs(outside + (w,))
    got_in, nodes = _route_run(functional.bidirect_q_a, inp_in, dev)
    assert _is_fused(nodes), nodes
    _route_compare(ck, "fused", got_in, _qside_ref64(inside + (w,)))
    got_out, nodes = _route_run(functional.bidirect_q_a, inp_out, dev)
    assert not _is_fused(nodes), nodes
    _route_compare(ck, "chained", got_out, _qside_ref64(outside + (w,)))
    # the chained route on the inside inputs: the same numbers as the fused one
    N = inside[0]
    got_ch, nodes = _route_run(lambda a, hq: functional._bidirect_q_a(a, hq, (N,)), inp_in, dev)
    assert not _is_fused(nodes), nodes
    _route_compare(ck, "chained vs fused", got_ch, {k: v.cpu().double() for k, v in got_in.items()})
    if outside[2] == 65:
        # through the switch itself: a 65th question token that is masked changes nothing, and takes the chained route.
        # (Only where a row keeps a valid token: a fully masked row attends all 65 uniformly.  Those rows are drawn anew.)
        a = inp_in["a"].clone()
        dead = (a == NEG).all(-1)
        assert bool(dead.any())
        a[dead] = torch.randn(int(dead.sum()), 64, generator=torch.Generator().manual_seed(32))
        live = dict(inp_in, a=a)
        got_live, nodes = _route_run(functional.bidirect_q_a, live, dev)
        assert _is_fused(nodes), nodes
        pad = dict(a=torch.cat([a, torch.full(inside[:2] + (1,), NEG)], 2), go=inp_in["go"],
                   hq=torch.cat([inp_in["hq"], torch.ones(N, 1, w)], 1))
        got_pad, nodes = _route_run(functional.bidirect_q_a, pad, dev)
        assert not _is_fused(nodes), nodes
        ck.equal("masked token: dA", got_pad["dA"][:, :, 64], torch.zeros_like(got_pad["dA"][:, :, 64]))
        ck.equal("masked token: d_hq", got_pad["dq"][:, 64], torch.zeros_like(got_pad["dq"][:, 64]))
        cut = dict(q_a=got_pad["q_a"], dA=got_pad["dA"][:, :, :64], dq=got_pad["dq"][:, :64])
        _route_compare(ck, "padded vs fused", cut, {k: v.cpu().double() for k, v in got_live.items()})
    ck.done()


# ------------------------------------------------------------------------------------ 4. the helper kernels
@pytest.mark.parametrize("J", [1, 64, 65, 300])
def test_softmax_bwd_rows_and_lanes(J):
    """a wave per row, four rows per workgroup (rows not a multiple of 4), lanes striding J by 64"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    ck = _Checks("softmax_bwd/J%d" % J)
    g = torch.Generator().manual_seed(41)
    for rows in (1, 5, 9):
        assert rows % 4 != 0
        p = torch.softmax(torch.randn(rows, J, generator=g).double() * 2, -1).float()
        dp = torch.randn(rows, J, generator=g)
        ref = p.double() * (dp.double() - (p.double() * dp.double()).sum(-1, keepdim=True))
        outs = []
        for _ in range(2):
            dx = torch.full((rows + 1, J), float("nan"), device=dev)      # one row more: the kernel stops at `rows`
            ops.softmax_bwd(p.to(dev), dp.to(dev), dx, rows, J)
            torch.cuda.synchronize()
            outs.append(dx)
        ck.close("rows%d" % rows, outs[0][:rows], ref, GRAD)
        assert bool(torch.isnan(outs[0][rows]).all()), "wrote past the last row"
        ck.equal("rows%d (second run)" % rows, outs[0][:rows], outs[1][:rows])
    ck.done()


@pytest.mark.parametrize("d", [1, 64, 65, 300, 600])
def test_wsum_ld_forward_backward(d):
    """fvta_wsum_fwd_ld / fvta_wsum_bwd with target rows target_ld > J * d apart: the forward's c += 256 loop wraps at
    d = 300 and 600, the backward's c += 64 loop from d = 65 on; J not a multiple of the four waves; the gap between two rows of
    d_target is never written; d_target = None and d_weights = None"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    ck = _Checks("wsum/d%d" % d)
    g = torch.Generator().manual_seed(42)
    rows, gap = 3, 5
    for J in (1, 4, 5, 9):
        ld = J * d + gap
        assert ld > J * d
        arena = torch.randn(rows, ld, generator=g)
        wts = torch.randn(rows, J, generator=g)
        go = torch.randn(rows, d, generator=g)
        base = torch.randn(rows, ld, generator=g)
        tgt = arena[:, :J * d].reshape(rows, J, d).double()
        ref_out = (tgt * wts.double()[..., None]).sum(1)
        ref_dw = (tgt * go.double()[:, None, :]).sum(-1)
        ref_dt = base[:, :J * d].reshape(rows, J, d).double() + wts.double()[..., None] * go.double()[:, None, :]
        ad, wd, god = arena.to(dev), wts.to(dev), go.to(dev)
        res = []
        for _ in range(2):
            out = torch.full((rows, d), float("nan"), device=dev)
            ops.wsum_fwd(ad, wd, out, rows, J, d, target_ld=ld)
            dw = torch.full((rows, J), float("nan"), device=dev)       # overwritten
            dt = base.to(dev)                                          # accumulated
            ops.wsum_bwd(ad, wd, god, dw, dt, rows, J, d, target_ld=ld)
            torch.cuda.synchronize()
            res.append((out, dw, dt))
        out, dw, dt = res[0]
        ck.close("J%d out" % J, out, ref_out, FWD)
        ck.close("J%d d_weights" % J, dw, ref_dw, GRAD)
        ck.close("J%d d_target" % J, dt[:, :J * d].reshape(rows, J, d), ref_dt, GRAD)
        ck.equal("J%d gap rows of d_target" % J, dt[:, J * d:].cpu(), base[:, J * d:])
        for k, name in enumerate(("out", "d_weights", "d_target")):
            ck.equal("J%d %s (second run)" % (J, name), res[0][k], res[1][k])
        # one output only: the other one comes out as with both
        dw1 = torch.full((rows, J), float("nan"), device=dev)
        ops.wsum_bwd(ad, wd, god, dw1, None, rows, J, d, target_ld=ld)
        dt1 = base.to(dev)
        ops.wsum_bwd(ad, wd, god, None, dt1, rows, J, d, target_ld=ld)
        torch.cuda.synchronize()
        ck.equal("J%d d_weights alone" % J, dw1, dw)
        ck.equal("J%d d_target alone" % J, dt1, dt)
    ck.done()


SOFTSEL_MAX_J = 16000          # fvta_softsel_fwd / _bwd: J floats of dynamic LDS next to 16 bytes of static


@pytest.mark.parametrize("rows,J,d,spread", [(2, 16000, 8, 3.0), (3, 257, 300, 1.0)])
def test_softsel_forward_backward_at_the_limit(rows, J, d, spread):
    """softsel and its backward at J = 16000 (64016 of the 65536 bytes of LDS a workgroup may ask for) and where both the
    j += 256 and the c += 256 loops wrap with a ragged last pass.  `spread` widens the logits at J = 16000 so that the
    weights do not all shrink to 1 / J, below the absolute tolerance."""
    from fvta_memexqa_amd import functional, ops
    dev = ops.require_gpu()
    if J == SOFTSEL_MAX_J:
        assert J * 4 + 16 == 64016 <= 65536
    else:
        assert J > 256 and J % 256 != 0 and d > 256 and d % 256 != 0
    g = torch.Generator().manual_seed(43)
    t, l = torch.randn(rows, J, d, generator=g), torch.randn(rows, J, generator=g) * spread
    go = torch.randn(rows, d, generator=g)
    tr, lr = t.double().requires_grad_(), l.double().requires_grad_()
    ref = (torch.softmax(lr, -1)[..., None] * tr).sum(1)
    ref.backward(go.double())
    res = []
    for _ in range(2):
        td, ld = t.to(dev).requires_grad_(), l.to(dev).requires_grad_()
        out = functional.softsel(td, ld)
        out.backward(go.to(dev))
        torch.cuda.synchronize()
        res.append((out.detach(), td.grad, ld.grad))
    ck = _Checks("softsel/%dx%dx%d" % (rows, J, d))
    ck.close("out", res[0][0], ref.detach(), FWD)
    ck.close("d_target", res[0][1], tr.grad, GRAD)
    ck.close("d_logits", res[0][2], lr.grad, GRAD)
    for k, name in enumerate(("out", "d_target", "d_logits")):
        ck.equal(name + " (second run)", res[0][k], res[1][k])
    ck.done()


# ------------------------------------------------------------------------------------------------- 5. refusals
def _refused(match, call, outputs):
    """`call` raises FvtaError naming `match`, and leaves every prefilled output bitwise as it was"""
    from fvta_memexqa_amd import _lib
    before = [o.clone() for o in outputs]
    with pytest.raises(_lib.FvtaError, match=match):
        call()
    torch.cuda.synchronize()
    for o, b in zip(outputs, before):
        assert torch.equal(o, b), "a refused call wrote into an output (%s)" % match


@pytest.mark.parametrize("V,JQ,match", [(2, 65, "JQ=65"), (8193, 1, "V\\*JQ=8193")])
def test_qside_refuses_what_its_tile_cannot_hold(V, JQ, match):
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    assert JQ > 64 or V * JQ == DENSE_MAX + 1
    R, w = 2, 64
    a, hq, go = torch.zeros(R, V, JQ, device=dev), torch.ones(R, JQ, w, device=dev), torch.ones(R, w, device=dev)
    q_a, dA, dq = (torch.full(s, 7.0, device=dev) for s in ((R, w), (R, V, JQ), (R, JQ, w)))
    _refused(match, lambda: ops.attn_qside_fwd(a, hq, q_a, R, V, JQ, w), [q_a])
    _refused(match, lambda: ops.attn_qside_bwd(a, hq, go, dA, dq, R, V, JQ, w), [dA, dq])


@pytest.mark.parametrize("K,T,simi,tanh,match", [(1, 2049, 1, False, "T=2049"), (2, 8, 1, False, "K=2"),
                                                 (1, 8, 1, True, "add_tanh=1"), (1, 8, 4, False, "simi=4")])
def test_logits_bwd_refuses(K, T, simi, tanh, match):
    """one row more than s_rs holds (T * JQ itself fits), K > 1, tanh on the logits, the cosine similarity"""
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    N, JQ, w = 2, 3, 64
    assert T * JQ <= DENSE_MAX and JQ <= 64
    op = ops.FocalAttention(N, K, T, JQ, w, simi, tanh)
    h, q, W = torch.ones(N, K, T, w, device=dev), torch.ones(N, JQ, w, device=dev), torch.ones(4 * w, device=dev)
    dA = torch.ones(N, K, T, JQ, device=dev)
    outs = [torch.full((N, K, T, w), 7.0, device=dev), torch.full((N, JQ, w), 7.0, device=dev),
            torch.full((4 * w,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)]
    _refused(match, lambda: op.logits_bwd(h, q, W, dA, *outs), outs)


def test_softsel_refuses_more_logits_than_lds_holds():
    from fvta_memexqa_amd import _lib, ops
    from fvta_memexqa_amd._lib import check, ptr, stream_ptr
    dev = ops.require_gpu()
    lib = _lib.load()
    rows, J, d = 1, SOFTSEL_MAX_J + 1, 2
    t, l, go = torch.ones(rows, J, d, device=dev), torch.zeros(rows, J, device=dev), torch.ones(rows, d, device=dev)
    out, dt, dl = (torch.full(s, 7.0, device=dev) for s in ((rows, d), (rows, J, d), (rows, J)))
    _refused("J=16001", lambda: check(lib.fvta_softsel_fwd(ptr(t), ptr(l), ptr(out), rows, J, d, stream_ptr()),
                                      "fvta_softsel_fwd"), [out])
    _refused("J=16001", lambda: check(lib.fvta_softsel_bwd(ptr(t), ptr(l), ptr(go), ptr(dt), ptr(dl), rows, J, d, stream_ptr()),
                                      "fvta_softsel_bwd"), [dt, dl])
