"""GPU parity of the pooled focal attention's training calls (fvta_attn_pool_fwd_train / fvta_attn_pool_bwd,
ops.PooledFocalAttention.forward_train / backward, autograd.pooled_focal_attention,
functional.attention_3d_pooled_raw(differentiable=True), nn.FocalAttention3D.forward_pooled(differentiable=True)) against
fp64 autograd of the oracle through the concatenated contexts (tests/_attn_pool_bwd_ref.py), at the tolerance of
tests/test_gpu_backward.py: rtol 1e-4, atol 1e-5 x max(1, max|ref|).

The shapes are the smallest that turn every loop over: references per album G+1, 1, 0, 2G+1 and G with an empty slot and
an album twice in one list, JX around the row pass's tile (fvta_attn_pool_bwd_plan), JQ = 1, 30, 32, 33, 64, widths 64 to
2048, M = 9, K = 6, P = NQ = M = 1, a question that lists nothing; and, past one round of the plan's and the row pass's
loops, `many` (P = 1500, 1600 references), `heavy` ([150, 0, 50]: 19 groups of one album) and `tiles` (two row tiles per
workgroup), each asserting its regime from the plans' words before any launch.  The pinned seeds keep every arg-max clear
in fp64 (tests/test_attn_pool_bwd_host.py); the first test also holds the GPU's own logits to a quarter of the smallest
gap."""
import pytest
import torch

from tests import _attn_pool_bwd_ref as B
from tests._album_attn_gpu import TrainRun, case, close_scaled, cu, gather, listed

pytestmark = pytest.mark.gpu


def _case(name):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(B, name)


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_gradients_match_fp64_autograd(name):
    c, ref = _case(name)
    run = TrainRun(c, "pooled")
    B.loop_regime(name, c, run.op.plan(), run.op.bwd_plan())    # a past-one-round case reaches its loop, before any launch
    ha, a = run.forward_train()
    # the arg-max the backward routes through is the reference's: the GPU's logits are within a quarter of the smallest gap
    jgap, tgap, _ = B.conditions(c, ref["a_logits"])
    v = B.valid_mask(c)
    err = float((a.cpu().double() - ref["a_logits"])[v].abs().max())
    print("%s: max |a_logits - fp64| over valid entries %.3g, smallest gap %.3g" % (name, err, min(jgap, tgap)))
    assert err < min(jgap, tgap) / 4, (err, jgap, tgap)
    close_scaled(ha, ref["h_a"], msg="h_a")
    dp, dq, dW, db = run.backward()                              # d_pool / d_hq prefilled with 7.0: overwritten
    for got, key in ((dp, "dpool"), (dq, "dq"), (dW, "dW"), (db, "db")):
        print("%s %s: max |got - ref| %.3g, max |ref| %.3g" % (name, key, float((got.cpu().double() - ref[key]).abs().max()),
                                                               float(ref[key].abs().max())))
    close_scaled(dp, ref["dpool"], msg="d_pool")
    close_scaled(dq, ref["dq"], msg="d_hq")
    close_scaled(dW, ref["dW"], msg="dW")
    close_scaled(db, ref["db"], msg="db")
    unlisted = listed(c) == 0
    if bool(unlisted.any()):                                     # albums nobody lists: exactly zero, not the 7.0
        assert float(dp.cpu()[unlisted].abs().max()) == 0.0
    nothing = (c["albums"] < 0).all(1)
    if bool(nothing.any()):                                      # a question that lists nothing: exactly zero, not the 7.0
        assert float(dq.cpu()[nothing].abs().max()) == 0.0
    dp2, dq2, dW2, db2 = run.backward(acc=(dW, db), fill=-3.0)   # a second call: dW / db accumulate, the others do not
    close_scaled(dW2, 2 * ref["dW"], atol=2e-5, msg="dW accumulates")
    close_scaled(db2, 2 * ref["db"], atol=2e-5, msg="db accumulates")
    close_scaled(dp2, ref["dpool"], msg="d_pool overwritten")
    close_scaled(dq2, ref["dq"], msg="d_hq overwritten")


def test_exact_zeros():
    """masked `mix`, every question partly valid: the album nobody lists and every masked row hold exactly 0"""
    c, _ = _case("mix-simi3-masked")
    run = TrainRun(c, "pooled")
    run.forward_train(want_logits=False)
    dp = run.backward()[0].cpu()
    unlisted = listed(c) == 0
    assert int(unlisted.sum()) == 1 and float(dp[unlisted].abs().max()) == 0.0
    assert bool((~c["pm"]).any()) and float(dp[~c["pm"]].abs().max()) == 0.0
    assert float(dp[c["pm"] & ~unlisted[:, None, None]].abs().max()) > 0.0


def _scatter(dhe, al, Pn):
    """index_add_ of the per-question row gradient [NQ,K,M JX,w] by reference, empty slots skipped -> [P,K,JX,w]"""
    NQ, M = al.shape
    K, w = dhe.shape[1], dhe.shape[3]
    JX = dhe.shape[2] // M
    per_ref = dhe.reshape(NQ, K, M, JX, w).permute(0, 2, 1, 3, 4).reshape(NQ * M, K, JX, w)
    flat = al.reshape(-1).long()
    keep = (flat >= 0).nonzero().reshape(-1)
    return torch.zeros(Pn, K, JX, w, device=dhe.device).index_add_(0, flat[keep], per_ref[keep])


def test_same_result_as_the_per_question_route(attn_select):
    """The masked `mix` case as make_case leaves it: a fully masked (album, k), a single-row (album, k), a fully masked
    question, an empty slot, an album twice in one list and an album nobody lists.  The contract is the expanded
    per-question route: gather, ops.FocalAttention forward + backward (accumulate = 0), scatter-add by reference.  Zeros:
    the unlisted album's rows, and every masked row -- except where fvta_attn_bwd itself writes one: a fully masked
    QUESTION's softmax is uniform over all rows it lists, masked ones included (p r g, no logit gradient)."""
    from fvta_memexqa_amd import ops
    c = B.build_case(B.MIX_MASKED, parity=False)
    assert bool((c["albums"] < 0).any())                                         # the empty slot
    run = TrainRun(c, "pooled")
    run.forward_train(want_logits=False)
    dp, dq, dW, db = run.backward()
    attn_select.exact()
    pool, pm, q, qm, al, W, b = run.args
    he, hme = gather(pool, pm, al)
    op = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"])
    op.forward(he, q, hme, qm, W, b)
    dhe, dqe = torch.full_like(he, 7.0), torch.full_like(q, 7.0)
    dWe, dbe = torch.zeros_like(W), torch.zeros(1, device="cuda")
    op.backward(he, q, hme, qm, W, b, run.g, dhe, dqe, dWe, dbe, 0)
    close_scaled(dp, _scatter(dhe, al, c["P"]), msg="d_pool against the scatter-add of the per-question gradient")
    close_scaled(dq, dqe, msg="d_hq")
    close_scaled(dW, dWe, msg="dW")
    close_scaled(db, dbe, msg="db")
    unlisted = (listed(c) == 0).nonzero().reshape(-1)
    assert unlisted.numel() == 1 and float(dp[int(unlisted[0])].abs().max()) == 0.0
    fully_masked_q = (~c["qm"].any(-1)).nonzero().reshape(-1)
    assert fully_masked_q.numel() == 1
    spread = set(p for p in c["albums"][fully_masked_q].reshape(-1).tolist() if p >= 0)
    checked = 0
    for p in range(c["P"]):
        if p in spread:
            continue
        masked_rows = ~c["pm"][p]                                                # [K,JX]
        assert float(dp[p].cpu()[masked_rows].abs().max()) == 0.0
        checked += int(masked_rows.sum())
    assert checked > 0
    assert float(dq[int(fully_masked_q[0])].abs().max()) == 0.0                  # nothing passes into a fully masked question


@pytest.mark.parametrize("name", ["mix-simi2-masked", "cols-jq33-w128", "rows-JX200", "wide2048", "all-empty-simi3"])
def test_forward_train_has_the_bits_of_the_inference_forward(name):
    c, _ = _case(name)
    run = TrainRun(c, "pooled")
    ha_t, a_t = run.forward_train()
    ha_i, a_i = run.forward()
    assert torch.equal(ha_t, ha_i) and torch.equal(a_t, a_i)
    ha_n, none = run.forward_train(want_logits=False)
    assert none is None and torch.equal(ha_n, ha_i)


@pytest.mark.parametrize("name", ["mix-simi2-masked", "cols-jq64-w512", "rows-JX200", "wide2048", "many"])
def test_one_slot_has_the_bits_of_the_shared_backward(name):
    """M = 1, lists album[:, None]: d_pool, d_hq, dW and db are ops.SharedFocalAttention's on the same inputs, bit for bit"""
    from fvta_memexqa_amd import ops
    c, _ = _case(name)
    album = c["albums"][:, 0].clamp(min=0)
    c1 = dict(c, albums=album[:, None], M=1, T=c["JX"])
    run = TrainRun(c1, "pooled")
    run.forward_train(want_logits=False)
    got = run.backward()
    pool, pm, q, qm, _, W, b = run.args
    sh = ops.SharedFocalAttention(c["P"], c["NQ"], c["K"], c["JX"], c["JQ"], c["w"], c["simi"], c["tanh"])
    al = ops.check_album_index(album, c["P"]).cuda()
    sh.forward_train(pool, pm, q, qm, al, W, b)
    dh, dq = torch.full_like(pool, 7.0), torch.full_like(q, 7.0)
    dW, db = torch.zeros_like(W), torch.zeros(1, device="cuda")
    sh.backward(pool, pm, q, qm, al, W, b, run.g, dh, dq, dW, db)
    for x, y, what in zip(got, (dh, dq, dW, db), ("d_pool", "d_hq", "dW", "db")):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("name", ["mix-simi3-masked", "many", "heavy", "slots9"])
def test_three_backward_calls_are_bitwise_equal(name):
    """`many` and `heavy`: an album's references span several batches of the ordered plan, whose promise this is;
    `slots9`: the fold sums nine slots per question"""
    c, _ = _case(name)
    outs = []
    for _ in range(3):
        run = TrainRun(c, "pooled")                              # a fresh handle: plan, saved and workspace anew
        run.forward_train(want_logits=False)
        outs.append(run.backward())
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["mix-simi2-masked", "heavy"])
def test_a_relabelled_pool_gives_the_same_bits(name):
    """albums permuted, lists renamed to match: an album's references keep their order and their groups' composition, so
    d_pool's rows under the permutation and d_hq are bitwise equal; dW / db sum in album order: at tolerance"""
    c, ref = _case(name)
    perm = torch.randperm(c["P"], generator=torch.Generator().manual_seed(3))   # new album perm[p] holds old album p
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(c["P"])
    assert perm.tolist() != list(range(c["P"]))
    al = c["albums"]
    al2 = torch.where(al >= 0, perm[al.clamp(min=0)], al)
    base = TrainRun(c, "pooled")
    base.forward_train(want_logits=False)
    dp, dq, dW, db = base.backward()
    moved = TrainRun(c, "pooled", pool=c["pool"][inv], pm=None if c["pm"] is None else c["pm"][inv], albums=al2)
    moved.forward_train(want_logits=False)
    dp2, dq2, dW2, db2 = moved.backward()
    assert torch.equal(dp2[perm.cuda()], dp) and torch.equal(dq2, dq)
    close_scaled(dW2, ref["dW"], msg="dW after relabelling")
    close_scaled(db2, ref["db"], msg="db after relabelling")


def test_a_questions_gradient_does_not_depend_on_its_company():
    c, _ = _case("mix-simi3-masked")
    run = TrainRun(c, "pooled")
    run.forward_train(want_logits=False)
    _, dq_all, _, _ = run.backward()
    i = next(i for i, row in enumerate(c["albums"].tolist()) if min(row) >= 0 and len(set(row)) > 1)
    one = TrainRun(c, "pooled", rows=[i])
    one.forward_train(want_logits=False)
    dp_one, dq_one, _, _ = one.backward()
    close_scaled(dq_one[0], dq_all[i], msg="d_hq alone against in company")
    mine = set(c["albums"][i].tolist())
    others = [p for p in range(c["P"]) if p not in mine]
    assert others and float(dp_one[others].abs().max()) == 0.0                 # and it reaches the albums it lists only
    assert all(float(dp_one[p].abs().max()) > 0.0 for p in mine)


def test_functional_and_nn_surface():
    from fvta_memexqa_amd import functional as Fn, nn
    c, ref = _case("rows-JXRb+1")                                              # w = 256, an empty slot
    lists = c["albums"].tolist()                                               # a list of lists
    pool, q, W, b = (cu(c[k]).requires_grad_() for k in ("pool", "q", "W", "b"))
    pm, qm, g = cu(c["pm"]), cu(c["qm"]), cu(c["gout"])
    ha, a = Fn.attention_3d_pooled_raw(pool, q, lists, W, b, pm, qm, simiMatrix=c["simi"], add_tanh=c["tanh"],
                                       differentiable=True)
    assert ha.requires_grad and not a.requires_grad
    assert tuple(a.shape) == (c["NQ"], c["K"], c["T"], c["JQ"])
    (ha * g).sum().backward()
    close_scaled(ha, ref["h_a"])
    close_scaled(pool.grad, ref["dpool"], msg="functional d_pool")
    close_scaled(q.grad, ref["dq"], msg="functional d_hq")
    close_scaled(W.grad.reshape(-1), ref["dW"], msg="functional dW")
    close_scaled(b.grad, ref["db"], msg="functional db")
    with pytest.raises(RuntimeError, match="forward-only"):                    # the default still refuses under gradient mode
        Fn.attention_3d_pooled_raw(pool, q, lists, W, b, pm, qm, simiMatrix=c["simi"], add_tanh=c["tanh"])
    with torch.no_grad():                                                      # and under no_grad it is the inference call
        ha_i, _ = Fn.attention_3d_pooled_raw(pool, q, lists, W, b, pm, qm, simiMatrix=c["simi"], add_tanh=c["tanh"])
    assert torch.equal(ha_i, ha.detach())

    att = nn.FocalAttention3D(c["w"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    with torch.no_grad():
        att.p("att_logits/W").copy_(cu(c["W"]))
        att.p("att_logits/b").copy_(cu(c["b"]))
    p2, q2 = cu(c["pool"]).requires_grad_(), cu(c["q"]).requires_grad_()
    ha2, a2 = att.forward_pooled(p2, q2, lists, pm, qm, differentiable=True)
    assert not a2.requires_grad
    (ha2 * g).sum().backward()
    close_scaled(p2.grad, ref["dpool"], msg="nn d_pool")
    close_scaled(q2.grad, ref["dq"], msg="nn d_hq")
    close_scaled(att.p("att_logits/W").grad.reshape(-1), ref["dW"], msg="nn dW")
    close_scaled(att.p("att_logits/b").grad, ref["db"], msg="nn db")
    with pytest.raises(RuntimeError, match="forward-only"):
        att.forward_pooled(p2, q2, lists, pm, qm)


def test_unpadded_width_goes_through_channel_padding():
    from fvta_memexqa_amd import functional as Fn
    c = B.odd_width_case()                                                     # w = 100 -> the 128-wide kernels
    ref = B.reference(c)
    assert B.qualifies(c, ref["a_logits"])
    pool, q, W, b = (cu(c[k]).requires_grad_() for k in ("pool", "q", "W", "b"))
    ha, a = Fn.attention_3d_pooled_raw(pool, q, c["albums"], W, b, cu(c["pm"]), cu(c["qm"]), simiMatrix=c["simi"],
                                       add_tanh=c["tanh"], differentiable=True)
    assert tuple(ha.shape) == (c["NQ"], 100)
    (ha * cu(c["gout"])).sum().backward()
    assert tuple(pool.grad.shape) == (c["P"], c["K"], c["JX"], 100) and tuple(q.grad.shape) == (c["NQ"], c["JQ"], 100)
    close_scaled(ha, ref["h_a"])
    close_scaled(pool.grad, ref["dpool"], msg="d_pool")
    close_scaled(q.grad, ref["dq"], msg="d_hq")
    close_scaled(W.grad.reshape(-1), ref["dW"], msg="dW")
    close_scaled(b.grad, ref["db"], msg="db")
