"""GPU parity of the shared-context focal attention's training calls UNDER THE TIME WARP (fvta_attn_shared_fwd_tw_train /
fvta_attn_shared_bwd_tw, ops.SharedWarpedFocalAttention.forward_train / backward, autograd.shared_warped_focal_attention,
functional.attention_3d_shared_warped_raw(differentiable=True), nn.FocalAttention3D.forward_shared_warped) against fp64
autograd of the definition -- time_warp_closed -> attention_3d on h[album] (tests/_attn_shared_tw_bwd_ref.py).

Tolerances, rtol / atol x max(1, max|ref|): d_hinfo, d_hq, dW, db at 1e-4 / 1e-5 (tests/test_gpu_attn_shared_bwd.py's);
d_lq, dWH_W, dWH_b, dWC_W, dWC_b at 2e-4 / 2e-5 (tests/test_gpu_timewarp.py's for the same gradients); h_a at 1e-4 / 1e-5.

The shapes are tests/test_gpu_attn_shared_bwd.py's -- every loop of the plan, the row pass and the question pass turned
over, LOOP_SPECS asserting their regime before any launch -- with the warp on: type 5 throughout, type 2 on `mix`, types
1 / 3 / 4 at T = 1, 7, 9, the windows 0.5, 3.0 and one wider than T, zero rows behind a mask.  The pinned seeds keep every
arg-max clear in fp64 (tests/test_attn_shared_tw_bwd_host.py); the first test also holds the GPU's own logits to a quarter
of the case's smallest gap.

Measured on the MI355X, worst |err| / (atol max(1, max|ref|) + rtol |ref|) over all 51 cases: d_hinfo 0.02, d_hq 0.01,
d_lq 0.02, dW 0.03, db 0.03, dWH_W 0.01, dWH_b 0.02, dWC_W 0.15, dWC_b 0.11.  db is the one output that needed care: as the
plain sum of dx it cancels from summands of order 1 to a few 1e-3 (0 without tanh) and kept 4e-6 to 1.1e-5 of fp32 noise --
1.08 and 1.05 of its tolerance at cols-jq1-w512 and cols-jq64-w512, and up to 0.69 on the per-question route on the same
inputs.  The kernels sum -damax x^2 instead (tests/test_attn_shared_tw_bwd_host.py holds the identity)."""
import pytest
import torch

from tests import _attn_shared_ref as R
from tests import _attn_shared_tw_bwd_ref as TB
from tests._album_attn_gpu import TrainRun, case, check_grads, close_scaled, cu, modules, output_names, tol_of, want_of

pytestmark = pytest.mark.gpu

NAMES = output_names("shared", True)                             # backward()'s nine outputs, in order
OVERWRITTEN, ACCUMULATED = NAMES[:3], NAMES[3:]


def _case(name):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(TB, name)


def _check_grads(name, got, ref, what=""):
    check_grads(name, got, ref, NAMES, TB.TOL, TB.within, what)


@pytest.mark.parametrize("name", TB.CASE_IDS)
def test_gradients_match_fp64_autograd(name):
    c, ref = _case(name)
    run = TrainRun(c, "shared", True)
    from fvta_memexqa_amd import ops
    plan = ops.SharedFocalAttention(c["A"], c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"]).plan()
    R.loop_regime(name, c, plan, run.op.bwd_plan())              # a LOOP_SPECS case reaches its loop, before any launch
    ha, a, s = run.forward_train()
    # the arg-max the backward routes through is the reference's: the GPU's logits are within a quarter of the smallest gap
    jgap, tgap, _ = TB.conditions(c, ref["a_logits"])
    v = TB.valid_mask(c)
    err = float((a.cpu().double() - ref["a_logits"])[v].abs().max())
    print("%s: max |a_logits - fp64| over valid entries %.3g, smallest gap %.3g" % (name, err, min(jgap, tgap)))
    assert err < min(jgap, tgap) / 4, (err, jgap, tgap)
    close_scaled(ha, ref["h_a"], msg="h_a")
    close_scaled(s, ref["scale"], msg="scale")
    got = run.backward()                                         # d_hinfo / d_hq / d_lq prefilled with 7.0: overwritten
    _check_grads(name, got, ref)
    empty = torch.bincount(c["album"], minlength=c["A"]) == 0
    if bool(empty.any()):                                        # albums without a question: exactly zero, not the 7.0
        assert float(got[0].cpu()[empty].abs().max()) == 0.0
    again = run.backward(acc=got[3:], fill=-3.0)                 # a second call: the parameter gradients accumulate ...
    for n, g in zip(ACCUMULATED, again[3:]):
        rtol, atol = tol_of(TB.TOL, n)
        close_scaled(g, 2 * want_of(ref, n, g), rtol=rtol, atol=2 * atol, msg=n + " accumulates")
    for n, g in zip(OVERWRITTEN, again[:3]):                     # ... the others do not
        rtol, atol = tol_of(TB.TOL, n)
        close_scaled(g, want_of(ref, n, g), rtol=rtol, atol=atol, msg=n + " overwritten")


def test_same_result_as_the_per_question_route(attn_select):
    """The masked `mix` case as make_case leaves it: a fully masked (album, k), a single-row (album, k), a fully masked
    question and an album without a question.  The contract is the expanded per-question route: index_select,
    ops.TimeWarp, ops.FocalAttention forward + backward (accumulate = 0), TimeWarp.backward, index_add_ of the row
    gradient.  The project's tolerances apply."""
    from fvta_memexqa_amd import ops
    c = TB.build_case(TB.MIX_MASKED, parity=False)
    run = TrainRun(c, "shared", True)
    run.forward_train(want_logits=False)
    got = run.backward()
    attn_select.exact()
    al64 = run.al.long()
    he, hme = run.rows.index_select(0, al64), run.mask.index_select(0, al64)
    tw = ops.TimeWarp(c["NQ"], c["K"], c["T"], c["w"], c["warp_type"], c["window_t"])
    warped = torch.empty_like(he)
    tw.forward(he, run.lq, run.WH, run.WHb, run.WC, run.WCb, warped)
    op = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"])
    op.forward(warped, run.q, hme, run.qm, run.W, run.b)
    dwarp, dqe = torch.full_like(he, 7.0), torch.full_like(run.q, 7.0)
    dWe, dbe = torch.zeros_like(run.W), torch.zeros(1, device="cuda")
    op.backward(warped, run.q, hme, run.qm, run.W, run.b, run.g, dwarp, dqe, dWe, dbe, 0)
    dhe, dlqe = torch.empty_like(he), torch.zeros_like(run.lq)
    dWH, dWHb, dWC, dWCb = torch.zeros_like(run.WH), torch.zeros_like(run.WHb), torch.zeros_like(run.WC), torch.zeros_like(run.WCb)
    tw.backward(he, run.lq, run.WH, run.WHb, run.WC, run.WCb, dwarp, dhe, dlqe, dWH, dWHb, dWC, dWCb)
    dh_ref = torch.zeros_like(run.rows).index_add_(0, al64, dhe)
    want = dict(dh=dh_ref, dq=dqe, dlq=dlqe, dW=dWe, db=dbe, dWH_W=dWH, dWH_b=dWHb, dWC_W=dWC, dWC_b=dWCb)
    _check_grads("per-question", got, {k: v.cpu().double() for k, v in want.items()}, what="against the expanded route: ")
    cnt = torch.bincount(c["album"], minlength=c["A"])
    empty = int((cnt == 0).nonzero()[0])
    assert float(got[0][empty].abs().max()) == 0.0               # the album without a question: exactly zero
    fully_masked_q = (~c["qm"].any(-1)).nonzero().reshape(-1)
    assert fully_masked_q.numel() == 1
    assert float(got[1][int(fully_masked_q[0])].abs().max()) == 0.0   # nothing passes into a fully masked question's hq


@pytest.mark.parametrize("name", ["mix-simi2-masked", "cols-jq33-w128", "rows-T333", "wide2048", "short-T9-warp3"])
def test_forward_train_has_the_bits_of_the_inference_forward(name):
    c, _ = _case(name)
    run = TrainRun(c, "shared", True)
    ha_t, a_t, s_t = run.forward_train()
    ha_i, a_i, s_i = run.forward()
    assert torch.equal(ha_t, ha_i) and torch.equal(a_t, a_i) and torch.equal(s_t, s_i)
    ha_n, none, s_n = run.forward_train(want_logits=False)
    assert none is None and torch.equal(ha_n, ha_i) and torch.equal(s_n, s_i)


@pytest.mark.parametrize("name", ["mix-simi3-masked", "rows-T333", "cols-jq64-w512", "many", "heavy", "tiles-w64", "splits9"])
def test_two_backward_calls_are_bitwise_equal(name):
    """all nine outputs; `many` and `heavy`: an album's questions span several batches of the ordered plan"""
    c, _ = _case(name)
    outs = []
    for _ in range(2):
        run = TrainRun(c, "shared", True)                        # a fresh handle: plan, saved and workspace anew
        run.forward_train(want_logits=False)
        outs.append(run.backward())
    assert len(outs[0]) == 9
    for n, x, y in zip(NAMES, outs[0], outs[1]):
        assert torch.equal(x, y), n


def test_a_questions_gradient_does_not_depend_on_its_company():
    """d_lq of a question in a full group and d_hq / d_lq of a question whose group has the same count in both calls are the
    same BITS alone with its album and in company: every sum behind them is the question's own, in an order the descriptor
    fixes (T = 50: one T split in both calls).  d_hq's dQs sum is the one exception by design: a group of fewer than G
    questions spreads a question's rows over the free accumulator regions, so its ORDER follows
    the group's count -- the question that is alone here but one of G in company is held to the tolerance instead."""
    c, _ = _case("mix-simi3-masked")
    G, _ = R.host_plan(c["JQ"], c["w"])
    big = int(torch.bincount(c["album"], minlength=c["A"]).argmax())          # the album with 2G+1 questions
    members = torch.nonzero(c["album"] == big).reshape(-1)                     # ascending: groups of G, G and 1
    assert members.numel() == 2 * G + 1
    run = TrainRun(c, "shared", True)
    run.forward_train(want_logits=False)
    got_all = run.backward()
    others = [a for a in range(c["A"]) if a != big]
    for i, same_count in ((int(members[2 * G]), True), (int(members[G]), False)):
        one = TrainRun(c, "shared", True, rows=[i])
        one.forward_train(want_logits=False)
        got_one = one.backward()
        assert torch.equal(got_one[2][0], got_all[2][i]), "d_lq alone against in company"
        if same_count:
            assert torch.equal(got_one[1][0], got_all[1][i]), "d_hq alone against in company"
        else:
            close_scaled(got_one[1][0], got_all[1][i], msg="d_hq alone against in company, another group count")
        assert float(got_one[0][others].abs().max()) == 0.0                    # and it reaches its own album only


def _module_grads(att, tw):
    return [att.p("att_logits/W").grad, att.p("att_logits/b").grad, tw.p("WH/W").grad, tw.p("WH/b").grad, tw.p("WC/W").grad,
            tw.p("WC/b").grad]


def test_functional_and_nn_surface():
    from fvta_memexqa_amd import functional as Fn, nn
    c, ref = _case("rows-TRb+1")                                               # w = 256
    keys = ("h", "q", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b")
    t = {k: cu(c[k]).requires_grad_() for k in keys}
    hm, qm, g = cu(c["hm"]), cu(c["qm"]), cu(c["gout"])
    kw = dict(simiMatrix=c["simi"], add_tanh=c["tanh"], warp_type=c["warp_type"], window_t=c["window_t"])
    args = lambda d: (d["h"], d["q"], c["album"], d["lq"], d["W"], d["b"], d["WH_W"], d["WH_b"], d["WC_W"], d["WC_b"], hm, qm)
    ha, a, s = Fn.attention_3d_shared_warped_raw(*args(t), differentiable=True, **kw)
    assert ha.requires_grad and not a.requires_grad and not s.requires_grad
    (ha * g).sum().backward()
    close_scaled(ha, ref["h_a"])
    grads = [t[k].grad for k in ("h", "q", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b")]
    assert tuple(grads[5].shape) == (2 * c["w"], c["w"]) and float(grads[5][c["w"]:].abs().max()) == 0.0
    grads[3], grads[7] = grads[3].reshape(-1), grads[7].reshape(-1)
    _check_grads("functional", [grads[0], grads[1], grads[2], grads[3], grads[4], grads[5], grads[6], grads[7], grads[8]], ref)
    # a held energy and energy=None: the same bits, forward and backward
    with torch.no_grad():
        e = Fn.album_energy(t["h"], t["WH_W"], t["WC_W"])
    t2 = {k: cu(c[k]).requires_grad_() for k in keys}
    ha2, a2, s2 = Fn.attention_3d_shared_warped_raw(*args(t2), energy=e, differentiable=True, **kw)
    (ha2 * g).sum().backward()
    assert torch.equal(ha2, ha) and torch.equal(a2, a) and torch.equal(s2, s)
    for k in keys:
        assert torch.equal(t2[k].grad, t[k].grad), k
    with pytest.raises(RuntimeError, match="forward-only"):                    # the default still refuses under gradient mode
        Fn.attention_3d_shared_warped_raw(*args(t), **kw)
    with pytest.raises(NotImplementedError):
        Fn.attention_3d_shared_warped_raw(t["h"], t["q"], c["album"], t["lq"], None, None, t["WH_W"], t["WH_b"], t["WC_W"],
                                          t["WC_b"], hm, qm, simiMatrix=4, warp_type=5, differentiable=True)

    # nn: forward_shared_warped against the per-question nn path, at the end-to-end 2e-4 of tests/test_gpu_attn_shared_tw.py
    att, tw = modules(c)
    h1, q1, lq1 = (cu(c[k]).requires_grad_() for k in ("h", "q", "lq"))
    ha_s, a_s = att.forward_shared_warped(h1, q1, c["album"], lq1, tw, hm, qm)
    assert ha_s.requires_grad and not a_s.requires_grad
    (ha_s * g).sum().backward()
    shared = [h1.grad, q1.grad, lq1.grad] + [x.clone() for x in _module_grads(att, tw)]
    att.zero_grad(set_to_none=True)
    tw.zero_grad(set_to_none=True)
    h2, q2, lq2 = (cu(c[k]).requires_grad_() for k in ("h", "q", "lq"))
    al = c["album"].cuda()
    warped, _ = tw(h2.index_select(0, al), lq2)[:2]
    ha_e, _ = att(warped, q2, hm.index_select(0, al), qm)
    (ha_e * g).sum().backward()
    each = [h2.grad, q2.grad, lq2.grad] + _module_grads(att, tw)
    close_scaled(ha_s, ha_e, rtol=2e-4, atol=2e-4, msg="nn h_a")
    for n, x, y in zip(NAMES, shared, each):
        assert x is not None and y is not None, n
        close_scaled(x.reshape(y.shape), y, rtol=2e-4, atol=2e-4, msg="nn " + n)
    with pytest.raises(NotImplementedError, match="forward_shared_warped"):    # the inference call's refusal names the new one
        att.forward_shared(h2, q2, c["album"], hm, qm, differentiable=True, time_warp=tw, lq=lq2)
    with pytest.raises(NotImplementedError):
        nn.FocalAttention3D(c["w"], simiMatrix=4).forward_shared_warped(h2, q2, c["album"], lq2, tw, hm, qm)


def test_unpadded_width_goes_through_channel_padding():
    from fvta_memexqa_amd import functional as Fn
    c = TB.odd_width_case()                                                    # w = 100 -> the 128-wide kernels
    ref = TB.reference(c)
    assert TB.qualifies(c, ref["a_logits"])
    keys = ("h", "q", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b")
    t = {k: cu(c[k]).requires_grad_() for k in keys}
    ha, a, s = Fn.attention_3d_shared_warped_raw(t["h"], t["q"], c["album"], t["lq"], t["W"], t["b"], t["WH_W"], t["WH_b"], t["WC_W"],
                                                 t["WC_b"], cu(c["hm"]), cu(c["qm"]), simiMatrix=c["simi"], add_tanh=c["tanh"],
                                                 warp_type=c["warp_type"], window_t=c["window_t"], differentiable=True)
    assert tuple(ha.shape) == (c["NQ"], 100)
    (ha * cu(c["gout"])).sum().backward()
    close_scaled(ha, ref["h_a"])
    close_scaled(s, ref["scale"])
    grads = [t[k].grad for k in ("h", "q", "lq")] + [t["W"].grad.reshape(-1), t["b"].grad, t["WH_W"].grad, t["WH_b"].grad,
                                                     t["WC_W"].grad.reshape(-1), t["WC_b"].grad]
    assert tuple(grads[5].shape) == (200, 100) and float(grads[5][100:].abs().max()) == 0.0
    _check_grads("odd-width", grads, ref)
