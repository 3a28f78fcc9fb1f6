"""GPU parity of the pooled focal attention's training calls UNDER THE TIME WARP (fvta_attn_pool_fwd_tw_train /
fvta_attn_pool_bwd_tw, ops.PooledWarpedFocalAttention.forward_train / backward, autograd.pooled_warped_focal_attention,
functional.attention_3d_pooled_warped_raw(differentiable=True), nn.FocalAttention3D.forward_pooled_warped) against fp64
autograd of the definition -- expand -> time_warp_closed -> attention_3d (tests/_attn_pool_tw_bwd_ref.py).

Tolerances are tests/_attn_shared_tw_bwd_ref.TOL, rtol / atol x max(1, max|ref|): d_pool, d_hq, dW, db and h_a at 1e-4 /
1e-5; d_lq, dWH_W, dWH_b, dWC_W, dWC_b at 2e-4 / 2e-5.

The shapes are tests/test_gpu_attn_pool_bwd.py's with the warp on (type 5 at window 2.3: on `mix` the band crosses both
slot boundaries), plus `mix` under type 2, types 1 / 3 / 4 where M JX <= 9, the windows 0.5, 3.0 and one wider than M JX,
JX = 260 (de's second block) and zero rows behind the masks.  The pinned seeds keep every arg-max clear in fp64
(tests/test_attn_pool_tw_bwd_host.py); the first test also holds the GPU's own logits to a quarter of the case's smallest
gap.

Measured on the MI355X, worst |err| / (atol max(1, max|ref|) + rtol |ref|) over the 49 parametrised cases and the
odd-width one: d_pool 0.02 (heavy), d_hq 0.01, d_lq 0.01, dW 0.05 (many), db 0.06, dWH_W 0.01, dWH_b 0.07, dWC_W 0.02,
dWC_b 0.42 (short-M1-JX7-warp3: counts up to 7 at M JX = 7; 0.01 at most outside the short cases).  The GPU's a_logits
stay within 0.7 % of the smallest arg-max gap.
Against the per-question route on `mix-simi2-masked` the nine gradients differ by at most 4e-7 of their largest value."""
import pytest
import torch

from tests import _attn_pool_tw_bwd_ref as TB
from tests._album_attn_gpu import (TrainRun, case, check_grads, close_scaled, cu, gather, listed, modules, nan_fill, output_names,
                                   tol_of, want_of)

pytestmark = pytest.mark.gpu

NAMES = output_names("pooled", True)                             # backward()'s nine outputs, in order
OVERWRITTEN, ACCUMULATED = NAMES[:3], NAMES[3:]


def _case(name):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(TB, name)


def _check_grads(name, got, ref, what=""):
    check_grads(name, got, ref, NAMES, TB.TOL, TB.within, what)


@pytest.mark.parametrize("name", TB.CASE_IDS)
def test_gradients_match_fp64_autograd(name):
    from fvta_memexqa_amd import ops
    c, ref = _case(name)
    plan, bwd_plan = TB.plans_of(c)                              # the host-only plans: no device yet
    TB.loop_regime(name, c, plan, bwd_plan)                      # a past-one-round case reaches its loop, before any launch
    run = TrainRun(c, "pooled", True)
    unwarped = ops.PooledFocalAttention(c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"], c["simi"], c["tanh"])
    assert run.op.plan() == unwarped.plan() == plan and run.op.bwd_plan() == unwarped.bwd_plan() == bwd_plan   # the warp changes none
    ha, a, s = run.forward_train()
    # the arg-max the backward routes through is the reference's: the GPU's logits are within a quarter of the smallest gap
    jgap, tgap, _ = TB.conditions(c, ref["a_logits"])
    v = TB.valid_mask(c)
    err = float((a.cpu().double() - ref["a_logits"])[v].abs().max())
    print("%s: max |a_logits - fp64| over valid entries %.3g, smallest gap %.3g" % (name, err, min(jgap, tgap)))
    assert err < min(jgap, tgap) / 4, (err, jgap, tgap)
    close_scaled(ha, ref["h_a"], msg="h_a")
    close_scaled(s, ref["scale"], msg="scale")
    got = run.backward()                                         # d_pool / d_hq / d_lq prefilled with 7.0: overwritten
    _check_grads(name, got, ref)
    unlisted = listed(c) == 0
    if bool(unlisted.any()):                                     # albums nobody lists: exactly zero, not the 7.0
        assert float(got[0].cpu()[unlisted].abs().max()) == 0.0
    nothing = (c["albums"] < 0).all(1)
    if bool(nothing.any()):                                      # a question that lists nothing: exactly zero, not the 7.0
        assert float(got[1].cpu()[nothing].abs().max()) == 0.0 and float(got[2].cpu()[nothing].abs().max()) == 0.0
    again = run.backward(acc=got[3:], fill=-3.0)                 # a second call: the parameter gradients accumulate ...
    for n, g in zip(ACCUMULATED, again[3:]):
        rtol, atol = tol_of(TB.TOL, n)
        close_scaled(g, 2 * want_of(ref, n, g), rtol=rtol, atol=2 * atol, msg=n + " accumulates")
    for n, g in zip(OVERWRITTEN, again[:3]):                     # ... the others do not
        rtol, atol = tol_of(TB.TOL, n)
        close_scaled(g, want_of(ref, n, g), rtol=rtol, atol=atol, msg=n + " overwritten")


@pytest.mark.parametrize("name", ["mix-simi2-masked", "cols-jq33-w128", "rows-JX260", "wide2048", "all-empty-simi3",
                                  "short-M3-JX3-warp3"])
def test_forward_train_has_the_bits_of_the_inference_forward(name):
    c, _ = _case(name)
    run = TrainRun(c, "pooled", True)
    ha_t, a_t, s_t = run.forward_train()
    ha_i, a_i, s_i = run.forward()
    assert torch.equal(ha_t, ha_i) and torch.equal(a_t, a_i) and torch.equal(s_t, s_i)
    ha_n, none, s_n = run.forward_train(want_logits=False)
    assert none is None and torch.equal(ha_n, ha_i) and torch.equal(s_n, s_i)


def _shared_run(c, album):
    """ops.SharedWarpedFocalAttention on (A = P, T = JX) with album [NQ]: -> forward outputs, the nine gradients, saved"""
    from fvta_memexqa_amd import ops
    w = c["w"]
    sh = ops.SharedWarpedFocalAttention(c["P"], c["NQ"], c["K"], c["JX"], c["JQ"], w, c["simi"], c["tanh"], c["warp_type"],
                                        c["window_t"])
    pool, pm, q, qm = cu(c["pool"]), cu(ops.as_mask_u8(c["pm"])), cu(c["q"]), cu(ops.as_mask_u8(c["qm"]))
    lq, al = cu(c["lq"]), ops.check_album_index(album, c["P"]).cuda()
    W, b = cu(c["W"].reshape(-1)), cu(c["b"])
    WH, WHb, WC, WCb = cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"].reshape(-1)), cu(c["WC_b"])
    e = sh.album_energy(pool, WH, WC)
    fwd = sh.forward_train(pool, pm, e, q, qm, lq, al, W, b, WHb, WC, WCb, want_logits=True, want_scale=True)
    dh, dq, dlq = torch.full_like(pool, 7.0), torch.full_like(q, 7.0), torch.full_like(lq, 7.0)
    acc = (torch.zeros_like(W), torch.zeros(1, device="cuda"), torch.zeros(w, w, device="cuda"), torch.zeros(w, device="cuda"),
           torch.zeros(w, device="cuda"), torch.zeros(1, device="cuda"))
    sh.backward(pool, pm, q, qm, lq, al, W, b, WH, WHb, WC, WCb, cu(c["gout"]), dh, dq, dlq, *acc)
    return fwd, (dh, dq, dlq) + acc, sh.saved


@pytest.mark.parametrize("name", ["single-simi1", "single-simi2", "mix-simi2-masked", "cols-jq64-w512", "rows-JX260", "wide2048",
                                  "short-M3-JX3-warp3", "many"])
def test_one_slot_has_the_bits_of_the_shared_warped_pair(name):
    """M = 1, lists album[:, None] (`single` is M = 1 as it stands; the others are a shared warped case: every question
    keeps its first album): the forward outputs, `saved` and all nine gradients are ops.SharedWarpedFocalAttention's on the
    same inputs, bit for bit"""
    c, _ = _case(name)
    album = c["albums"][:, 0].clamp(min=0)
    c1 = dict(c, albums=album[:, None], M=1, T=c["JX"])
    run = TrainRun(c1, "pooled", True)
    fwd = run.forward_train()
    got = run.backward()
    fwd_s, got_s, saved_s = _shared_run(c1, album)
    for x, y, what in zip(fwd, fwd_s, ("h_a", "a_logits", "scale")):
        assert torch.equal(x, y), what
    assert run.op.saved.numel() == saved_s.numel()
    for x, y, what in zip(got, got_s, NAMES):
        assert torch.equal(x, y), what
    # `saved`: every byte a launch writes is the shared call's; what no launch writes (alignment gaps, the r2 rows of an
    # album without a question) is compared after both were prefilled alike
    a, b = run.op.saved, saved_s
    a.fill_(0x5A), b.fill_(0x5A)
    run.forward_train(want_logits=False)
    _shared_run_forward_only(c1, album, b)
    assert torch.equal(a, b), "saved"


def _shared_run_forward_only(c, album, saved):
    from fvta_memexqa_amd import ops
    sh = ops.SharedWarpedFocalAttention(c["P"], c["NQ"], c["K"], c["JX"], c["JQ"], c["w"], c["simi"], c["tanh"], c["warp_type"],
                                        c["window_t"])
    sh.saved = saved
    pool, pm, q, qm = cu(c["pool"]), cu(ops.as_mask_u8(c["pm"])), cu(c["q"]), cu(ops.as_mask_u8(c["qm"]))
    WH, WHb, WC, WCb = cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"].reshape(-1)), cu(c["WC_b"])
    e = sh.album_energy(pool, WH, WC)
    sh.forward_train(pool, pm, e, q, qm, cu(c["lq"]), ops.check_album_index(album, c["P"]).cuda(), cu(c["W"].reshape(-1)),
                     cu(c["b"]), WHb, WC, WCb)


@pytest.mark.parametrize("name", ["mix-simi3-masked", "rows-JX260", "cols-jq64-w512", "many", "heavy", "tiles", "slots9"])
def test_two_backward_calls_are_bitwise_equal(name):
    """all nine outputs; `many` and `heavy`: an album's references span several batches of the ordered plan; `slots9`: the
    fold sums nine slots per question"""
    c, _ = _case(name)
    outs = []
    for _ in range(2):
        run = TrainRun(c, "pooled", True)                        # a fresh handle: plan, saved and workspace anew
        run.forward_train(want_logits=False)
        outs.append(run.backward())
    assert len(outs[0]) == 9
    for n, x, y in zip(NAMES, outs[0], outs[1]):
        assert torch.equal(x, y), n


@pytest.mark.parametrize("name", ["mix-simi1-masked", "mix-simi2-masked", "mix-simi3-masked", "all-empty-simi1", "all-empty-simi3"])
def test_nothing_is_read_that_no_launch_wrote(name):
    """The empty-slot rule.  No row pass visits the positions of an empty slot, so their ds / dbt / dx s in the workspace
    (and lin in `saved`) are whatever the memory held.  With `saved` prefilled with a NaN pattern before the forward and
    the backward's workspace before the backward -- every byte no launch writes is then a NaN -- the nine outputs are
    finite and the bits of an ordinary run."""
    c, _ = _case(name)
    assert bool((c["albums"] < 0).any())
    base = TrainRun(c, "pooled", True)
    base.forward_train(want_logits=False)
    want = base.backward()
    run = TrainRun(c, "pooled", True)
    run.forward_train(want_logits=False)                         # allocates op.saved
    run.backward()                                               # ... and op.work_bwd
    nan_fill(run.op.saved)
    run.forward_train(want_logits=False)                         # rewrites what it writes; the rest stays NaN
    nan_fill(run.op.work_bwd)
    got = run.backward()
    for n, x, y in zip(NAMES, got, want):
        assert bool(torch.isfinite(x).all()), n
        assert torch.equal(x, y), n


def _apart_from(c, i):
    """the questions that share no album with question i (one that lists nothing among them)"""
    al = c["albums"].tolist()
    mine = {p for p in al[i] if p >= 0}
    return [j for j, row in enumerate(al) if j != i and not (mine & {p for p in row if p >= 0})]


@pytest.mark.parametrize("name,i", [("mix-simi3-masked", 2), ("mix-simi3-masked", 11), ("all-empty-simi3", 0), ("all-empty-simi3", 2),
                                    ("rows-JXRb+1", 2)])
def test_a_questions_gradient_bits_do_not_depend_on_its_company(name, i):
    """The call without the questions that share no album with question i (on `all-empty`: the one that lists nothing;
    on `mix`: three questions that list album 3 alone; question 11 of `mix` and 2 of `all-empty` have an empty slot).  Every
    album that i lists keeps its references, their order and so its groups' counts -- the question pass's spreading and
    the fold's slot order are what they were -- and JX here leaves one split of the rows in either call: d_hq[i] and
    d_lq[i] are the same BITS, and so are the d_pool rows of the albums i lists, whose every reference is still there."""
    c, _ = _case(name)
    drop = _apart_from(c, i)
    assert drop and any(p >= 0 for p in c["albums"][i].tolist())
    keep = [j for j in range(c["NQ"]) if j not in drop]
    run = TrainRun(c, "pooled", True)
    assert run.op.bwd_plan()["tsplit"] == 1
    run.forward_train(want_logits=False)
    got_all = run.backward()
    sub = TrainRun(c, "pooled", True, rows=keep)
    assert sub.op.bwd_plan()["tsplit"] == 1
    sub.forward_train(want_logits=False)
    got_sub = sub.backward()
    at = keep.index(i)
    assert torch.equal(got_sub[1][at], got_all[1][i]), "d_hq in other company"
    assert torch.equal(got_sub[2][at], got_all[2][i]), "d_lq in other company"
    mine = sorted({p for p in c["albums"][i].tolist() if p >= 0})
    shared_with_kept = set(p for j in keep for p in c["albums"][j].tolist() if p >= 0)
    assert torch.equal(got_sub[0][mine], got_all[0][mine]), "d_pool of the albums it lists"
    gone = [p for p in range(c["P"]) if p not in shared_with_kept]
    if gone:                                                     # albums only the dropped questions list: zeros now
        assert float(got_sub[0][gone].abs().max()) == 0.0


def test_a_question_alone_keeps_its_d_lq_bits():
    """A question alone with the pool: every sum behind d_lq is the question's own over its M JX positions in a fixed
    order -- the same BITS as in company.  Its albums' reference counts DO change here, and with them the question pass's
    spreading of a reference's rows over free accumulator regions, so d_hq's dQs sum has
    another order: held to the tolerance in this one case.  Its d_pool reaches the albums it lists only."""
    c, _ = _case("mix-simi3-masked")
    run = TrainRun(c, "pooled", True)
    run.forward_train(want_logits=False)
    got_all = run.backward()
    i = next(i for i, row in enumerate(c["albums"].tolist()) if min(row) >= 0 and len(set(row)) > 1)
    one = TrainRun(c, "pooled", True, rows=[i])
    one.forward_train(want_logits=False)
    got_one = one.backward()
    assert torch.equal(got_one[2][0], got_all[2][i]), "d_lq alone against in company"
    close_scaled(got_one[1][0], got_all[1][i], msg="d_hq alone against in company, other group counts")
    mine = set(c["albums"][i].tolist())
    others = [p for p in range(c["P"]) if p not in mine]
    assert others and float(got_one[0][others].abs().max()) == 0.0
    assert all(float(got_one[0][p].abs().max()) > 0.0 for p in mine)


def test_same_result_as_the_per_question_route(attn_select):
    """The masked `mix` case as make_case leaves it: a fully masked (album, k), a single-row (album, k), a fully masked
    question, an empty slot, an album twice in one list and an album nobody lists.  The per-question route at module
    level: gather of the listed albums' rows and mask, nn.TimeWarp, nn.FocalAttention3D.forward, backward() -- autograd
    does the index_add_ into the pool.  Each route is held to fp64 at the project's tolerances, so the two agree within
    the sum of their bounds: twice the tolerance of each output."""
    c = TB.build_case(TB.MIX_MASKED, parity=False)
    assert bool((c["albums"] < 0).any())
    run = TrainRun(c, "pooled", True)
    run.forward_train(want_logits=False)
    got = run.backward()
    attn_select.exact()
    att, tw = modules(c)
    pool, q, lq = (cu(c[k]).requires_grad_() for k in ("pool", "q", "lq"))
    rows, mask = gather(pool, cu(c["pm"]), run.al)
    warped = tw(rows, lq)[0]
    h_a, _ = att(warped, q, mask, cu(c["qm"]))
    (h_a * run.g).sum().backward()
    want = (pool.grad, q.grad, lq.grad, att.p("att_logits/W").grad.reshape(-1), att.p("att_logits/b").grad, tw.p("WH/W").grad,
            tw.p("WH/b").grad, tw.p("WC/W").grad.reshape(-1), tw.p("WC/b").grad)
    for n, g, wnt in zip(NAMES, got, want):
        rtol, atol = tol_of(TB.TOL, n)
        assert wnt is not None, n
        wnt = wnt[:g.shape[0]] if n == "dWH_W" else wnt
        print("per-question %s: max |diff| %.3g, max |ref| %.3g" % (n, float((g - wnt).abs().max()), float(wnt.abs().max())))
        close_scaled(g, wnt, rtol=2 * rtol, atol=2 * atol, msg=n + " against the per-question route")
    unlisted = (listed(c) == 0).nonzero().reshape(-1)
    assert unlisted.numel() == 1 and float(got[0][int(unlisted[0])].abs().max()) == 0.0
    fully_masked_q = (~c["qm"].any(-1)).nonzero().reshape(-1)
    assert fully_masked_q.numel() == 1
    assert float(got[1][int(fully_masked_q[0])].abs().max()) == 0.0   # nothing passes into a fully masked question's hq


LEAVES = ("pool", "q", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b")


def _leaf_grads(t):
    g = [t[k].grad for k in LEAVES]
    g[3], g[7] = g[3].reshape(-1), g[7].reshape(-1)
    return g


def test_public_surface_matches_the_ops_level_result():
    from fvta_memexqa_amd import autograd, functional as Fn, nn, ops
    c, ref = _case("rows-JXRb+1")                                              # w = 256, an empty slot
    run = TrainRun(c, "pooled", True)
    ha_o, a_o, s_o = run.forward_train()
    got = run.backward()
    lists = c["albums"].tolist()                                               # a list of lists
    pm, qm, g = cu(c["pm"]), cu(c["qm"]), cu(c["gout"])
    kw = dict(simiMatrix=c["simi"], add_tanh=c["tanh"], warp_type=c["warp_type"], window_t=c["window_t"])
    args = lambda d: (d["pool"], d["q"], lists, d["lq"], d["W"], d["b"], d["WH_W"], d["WH_b"], d["WC_W"], d["WC_b"], pm, qm)
    # functional
    t = {k: cu(c[k]).requires_grad_() for k in LEAVES}
    ha, a, s = Fn.attention_3d_pooled_warped_raw(*args(t), differentiable=True, **kw)
    assert ha.requires_grad and not a.requires_grad and not s.requires_grad
    assert tuple(a.shape) == (c["NQ"], c["K"], c["T"], c["JQ"]) and tuple(s.shape) == (c["NQ"], c["T"])
    (ha * g).sum().backward()
    assert torch.equal(ha, ha_o) and torch.equal(a, a_o) and torch.equal(s, s_o)
    grads = _leaf_grads(t)
    assert tuple(grads[5].shape) == (2 * c["w"], c["w"]) and float(grads[5][c["w"]:].abs().max()) == 0.0
    for n, x, y in zip(NAMES, grads, got):
        assert torch.equal(x[:y.shape[0]] if n == "dWH_W" else x, y), "functional " + n
    _check_grads("functional", grads, ref)
    # a held energy is a cache of the forward; the gradient through e flows all the same: the same bits
    with torch.no_grad():
        e = Fn.album_energy(t["pool"], t["WH_W"], t["WC_W"])
    assert tuple(e.shape) == (c["P"], c["JX"])
    t2 = {k: cu(c[k]).requires_grad_() for k in LEAVES}
    ha2, a2, s2 = Fn.attention_3d_pooled_warped_raw(*args(t2), energy=e, differentiable=True, **kw)
    (ha2 * g).sum().backward()
    assert torch.equal(ha2, ha) and torch.equal(a2, a) and torch.equal(s2, s)
    for k in LEAVES:
        assert torch.equal(t2[k].grad, t[k].grad), k
    with pytest.raises(RuntimeError, match="forward-only"):                    # the default still refuses under gradient mode
        Fn.attention_3d_pooled_warped_raw(*args(t), **kw)
    with torch.no_grad():                                                      # and under no_grad it is the inference call
        ha_i, _, _ = Fn.attention_3d_pooled_warped_raw(*args(t), **kw)
    assert torch.equal(ha_i, ha.detach())
    # autograd
    t3 = {k: cu(c[k]).requires_grad_() for k in LEAVES}
    ha3, a3, s3 = autograd.pooled_warped_focal_attention(
        t3["pool"], t3["q"], t3["lq"], run.al, t3["W"].reshape(-1), t3["b"], t3["WH_W"], t3["WH_b"], t3["WC_W"], t3["WC_b"],
        ops.as_mask_u8(pm), ops.as_mask_u8(qm), c["simi"], c["tanh"], c["warp_type"], c["window_t"])
    assert not a3.requires_grad and not s3.requires_grad
    (ha3 * g).sum().backward()
    for n, x, y in zip(NAMES, _leaf_grads(t3), got):
        assert torch.equal(x[:y.shape[0]] if n == "dWH_W" else x, y), "autograd " + n
    # nn
    att, tw = modules(c)
    p4, q4, lq4 = (cu(c[k]).requires_grad_() for k in ("pool", "q", "lq"))
    ha4, a4 = att.forward_pooled_warped(p4, q4, lists, lq4, tw, pm, qm)
    assert ha4.requires_grad and not a4.requires_grad
    (ha4 * g).sum().backward()
    mod = [p4.grad, q4.grad, lq4.grad, att.p("att_logits/W").grad.reshape(-1), att.p("att_logits/b").grad, tw.p("WH/W").grad,
           tw.p("WH/b").grad, tw.p("WC/W").grad.reshape(-1), tw.p("WC/b").grad]
    assert torch.equal(ha4, ha_o)
    for n, x, y in zip(NAMES, mod, got):
        assert torch.equal(x[:y.shape[0]] if n == "dWH_W" else x, y), "nn " + n
    with pytest.raises(NotImplementedError, match="forward_pooled_warped"):    # the inference call's refusal names the new one
        att.forward_pooled(p4, q4, lists, pm, qm, time_warp=tw, lq=lq4, differentiable=True)
    with pytest.raises(NotImplementedError):
        nn.FocalAttention3D(c["w"], simiMatrix=4).forward_pooled_warped(p4, q4, lists, lq4, tw, pm, qm)


def test_unpadded_width_goes_through_channel_padding():
    from fvta_memexqa_amd import functional as Fn
    c = TB.odd_width_case()                                                    # w = 50 -> the 64-wide kernels
    ref = TB.reference(c)
    assert TB.qualifies(c, ref["a_logits"])
    t = {k: cu(c[k]).requires_grad_() for k in LEAVES}
    ha, a, s = Fn.attention_3d_pooled_warped_raw(t["pool"], t["q"], c["albums"], t["lq"], t["W"], t["b"], t["WH_W"], t["WH_b"],
                                                 t["WC_W"], t["WC_b"], cu(c["pm"]), cu(c["qm"]), simiMatrix=c["simi"],
                                                 add_tanh=c["tanh"], warp_type=c["warp_type"], window_t=c["window_t"],
                                                 differentiable=True)
    assert tuple(ha.shape) == (c["NQ"], 50)
    (ha * cu(c["gout"])).sum().backward()
    assert tuple(t["pool"].grad.shape) == (c["P"], c["K"], c["JX"], 50) and tuple(t["lq"].grad.shape) == (c["NQ"], 50)
    close_scaled(ha, ref["h_a"])
    close_scaled(s, ref["scale"])
    grads = _leaf_grads(t)
    assert tuple(grads[5].shape) == (100, 50) and float(grads[5][50:].abs().max()) == 0.0
    _check_grads("odd-width", grads, ref)
