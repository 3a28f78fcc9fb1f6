"""GPU parity of the focal attention over per-question album lists from one album pool (fvta_attn_pool_fwd,
ops.PooledFocalAttention, functional.attention_3d_pooled_raw, nn.FocalAttention3D.forward_pooled, nn.AlbumPool) against
the fp64 reference of tests/_attn_pooled_ref.py, at the tolerances of tests/test_gpu_attn_shared.py: against fp64 h_a
rtol 1e-4 / atol 1e-5 and a_logits rtol 1e-4 / atol 2e-5; against another fp32 route rtol 2e-5 / atol 2e-6.

The shapes (SPECS there) are the smallest that turn every loop over: 0, 1, G, G+1 and 2G+1 references to an album, empty
slots, an album twice in one list, row tiles at JX = 1, 7, R-1, R, R+1, 200, question columns at JQ = 1, 30, 32, 33, 64,
widths up to 2048, nine slots, K = 6, P = NQ = M = 1, a question without any album; G and R are read from
fvta_attn_pool_plan.  LOOP_SPECS goes past one round of the plan's and the weighted sum's loops, each case asserting its
regime through the plan's words before it launches.  Every index given to a GPU call is valid."""
import pytest
import torch

from tests import _attn_pooled_ref as R
from tests import _attn_shared_ref as S
from tests._album_attn_gpu import case, close, cu, handle, infer

pytestmark = pytest.mark.gpu

FP32 = dict(rtol=2e-5, atol=2e-6)


def _case(name, simi, tanh, masked):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(R, (name, simi, tanh, masked), lambda key: R.build_case(name, simi, masked), lambda c: R.reference(c, tanh))


def _loop_case(name):
    return case(R, name, R.loop_case, lambda c: R.reference(c, c["tanh"]))


def _op(c, tanh):
    return handle(c, "pooled", tanh=tanh)


def _run(c, tanh, **kw):
    """ops.PooledFocalAttention on case c; rows: a subset of the questions (an index list); albums / pool / pm: in place
    of the case's own"""
    return infer(c, "pooled", tanh=tanh, **kw)


def _report(name, ha, a, ref_ha, ref_a):
    live = ref_a > -1e29
    print("%s h_a: max |got - ref| %.3g, max |ref| %.3g; a_logits: max |got - ref| over valid entries %.3g"
          % (name, float((ha.cpu().double() - ref_ha).abs().max()), float(ref_ha.abs().max()),
             float((a.cpu().double() - ref_a)[live].abs().max()) if bool(live.any()) else 0.0))


# ---- against the fp64 reference
@pytest.mark.parametrize("name,simi,tanh,masked", R.CASES, ids=R.CASE_IDS)
def test_matches_the_fp64_reference(name, simi, tanh, masked):
    c, (ref_ha, ref_a) = _case(name, simi, tanh, masked)
    ha, a = _run(c, tanh)
    _report(name, ha, a, ref_ha, ref_a)
    close(ha, ref_ha, msg="h_a")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")
    if name == "all-empty":                                                 # a question without any album: exactly 0
        assert c["albums"][1].tolist() == [-1, -1]
        assert torch.equal(ha[1].cpu(), torch.zeros(c["w"])) and bool((a[1] == R.NEG).all())


def test_plan_is_what_the_shapes_assume():
    c, _ = _case("mix", 1, False, True)
    op = _op(c, False)
    p = op.plan()
    assert p == R.host_plan_words(c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"])
    assert p["G"] >= 8 and (p["G"], p["rows"]) == R.host_plan(10, 64) == S.host_plan(10, 64)


# ---- past one round of the plan and weighted-sum loops
@pytest.mark.parametrize("name", R.LOOP_IDS)
def test_loop_cases_match_the_fp64_reference(name):
    c, (ref_ha, ref_a) = _loop_case(name)
    R.loop_regime(name, c, _op(c, c["tanh"]).plan())                         # before anything is launched
    ha, a = _run(c, c["tanh"])
    _report(name, ha, a, ref_ha, ref_a)
    close(ha, ref_ha, msg="h_a")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")
    ha2, a2 = _run(c, c["tanh"])                                             # the plan's cursor atomics race: no bit moves
    assert torch.equal(ha, ha2) and torch.equal(a, a2)


# ---- M = 1 is the shared call
@pytest.mark.parametrize("simi,tanh,masked", [(1, False, True), (2, True, False), (4, False, True)])
def test_one_slot_is_the_shared_call_bit_for_bit(simi, tanh, masked):
    from fvta_memexqa_amd import ops
    c = S.build_case("mix", simi, masked)
    args = (cu(c["h"]), cu(ops.as_mask_u8(c["hm"])), cu(c["q"]), cu(ops.as_mask_u8(c["qm"])))
    Wb = (None if c["W"] is None else cu(c["W"].reshape(-1)), cu(c["b"]))
    shared = ops.SharedFocalAttention(c["A"], c["NQ"], c["K"], c["T"], c["JQ"], c["w"], simi, tanh)
    ha_s, a_s = shared.forward(*args, ops.check_album_index(c["album"], c["A"]).cuda(), *Wb, want_logits=True)
    pooled = ops.PooledFocalAttention(c["A"], c["NQ"], 1, c["K"], c["T"], c["JQ"], c["w"], simi, tanh)
    assert pooled.plan() == shared.plan()
    ha_p, a_p = pooled.forward(*args, ops.check_album_lists(c["album"][:, None], c["A"], masked).cuda(), *Wb, want_logits=True)
    assert torch.equal(ha_p, ha_s) and torch.equal(a_p, a_s)


# ---- the per-question kernel on the gathered rows
@pytest.mark.parametrize("name,simi,tanh,masked", [("mix", 2, True, True), ("rows4", 1, False, True)])
def test_same_result_as_the_per_question_kernel(name, simi, tanh, masked, attn_select):
    from fvta_memexqa_amd import ops
    c, _ = _case(name, simi, tanh, masked)
    if name == "rows4":
        assert c["JX"] == R.host_plan(c["JQ"], c["w"])[1] + 1                # R + 1
    h, m = R.expand(c)                                                       # [NQ,K,T,w]: what the pooled call never builds
    attn_select.exact()
    op = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], simi, tanh)
    ref_ha, ref_a = op.forward(cu(h), cu(c["q"]), cu(ops.as_mask_u8(m)), cu(ops.as_mask_u8(c["qm"])),
                               cu(c["W"].reshape(-1)), cu(c["b"]), want_logits=True)
    ha, a = _run(c, tanh)
    print("%s against the per-question exact kernel: max |h_a diff| %.3g, max |a_logits diff| %.3g"
          % (name, float((ha - ref_ha).abs().max()), float((a - ref_a).abs().max())))
    close(ha, ref_ha, msg="h_a against the per-question exact kernel", **FP32)
    close(a, ref_a, msg="a_logits against the per-question exact kernel", **FP32)


# ---- placement changes no bit
def test_placement_changes_no_bit():
    c, _ = _case("mix", 3, True, True)
    ha, a = _run(c, True)
    ha2, a2 = _run(c, True)
    assert torch.equal(ha, ha2) and torch.equal(a, a2)                       # the same call twice
    perm = torch.tensor([3, 0, 4, 1, 2])                                     # new label of album p: perm[p]
    pool, pm = torch.empty_like(c["pool"]), torch.empty_like(c["pm"])
    pool[perm], pm[perm] = c["pool"], c["pm"]
    al = torch.where(c["albums"] >= 0, perm[c["albums"].clamp(min=0)], c["albums"])
    ha3, a3 = _run(c, True, albums=al, pool=pool, pm=pm)
    assert torch.equal(ha, ha3) and torch.equal(a, a3)                       # the pool relabelled: other groups, the same bits
    ha4, none = _run(c, True, want_logits=False)
    assert none is None and torch.equal(ha, ha4)                             # want_logits changes no bit of h_a


def test_a_question_does_not_depend_on_its_company():
    c, _ = _case("mix", 3, True, True)
    ha, a = _run(c, True)
    twice = next(i for i, r in enumerate(c["albums"].tolist()) if min(r) >= 0 and len(set(r)) < len(r))
    for i in (0, twice, c["NQ"] - 1):                                        # the last: the one with the empty slot, fully masked
        ha_one, a_one = _run(c, True, rows=[i])
        close(ha_one[0], ha[i], msg="alone against in company, question %d" % i, **FP32)
        close(a_one[0], a[i], **FP32)


def test_slot_order_permutes_the_logit_blocks():
    c, _ = _case("mix", 2, True, True)
    JX = c["JX"]
    i = next(i for i, r in enumerate(c["albums"].tolist()) if min(r) >= 0 and len(set(r)) == len(r))
    ha, a = _run(c, True)
    al = c["albums"].clone()
    order = [2, 0, 1]
    al[i] = c["albums"][i][order]
    assert al[i].tolist() != c["albums"][i].tolist()
    ha2, a2 = _run(c, True, albums=al)
    blocks = a[i].reshape(c["K"], c["M"], JX, c["JQ"])[:, order].reshape(c["K"], c["T"], c["JQ"])
    assert torch.equal(a2[i], blocks)                                        # its blocks move with the slots, bit for bit
    close(ha2[i], ha[i], msg="the merge order moves", **FP32)
    keep = [j for j in range(c["NQ"]) if j != i]
    assert torch.equal(ha2[keep], ha[keep]) and torch.equal(a2[keep], a[keep])


# ---- the surface
def test_functional_and_nn_surface():
    from fvta_memexqa_amd import functional as Fn, nn
    c, (ref_ha, ref_a) = _case("rows1", 2, True, True)                       # w = 256, simiMatrix 2, tanh
    ha_ops, a_ops = _run(c, True)
    pool, q, W, b, pm, qm = cu(c["pool"]), cu(c["q"]), cu(c["W"]), cu(c["b"]), cu(c["pm"]), cu(c["qm"])
    with torch.no_grad():
        ha, a = Fn.attention_3d_pooled_raw(pool, q, c["albums"], W, b, pm, qm, simiMatrix=2, add_tanh=True)
    assert torch.equal(ha, ha_ops) and torch.equal(a, a_ops)
    att = nn.FocalAttention3D(c["w"], simiMatrix=2, add_tanh=True)
    with torch.no_grad():
        att.p("att_logits/W").copy_(W)
        att.p("att_logits/b").copy_(b)
        ha_n, a_n = att.forward_pooled(pool, q, c["albums"].tolist(), pm, qm)            # a list of lists
        mem = nn.AlbumPool(pool, pm)
        ha_m, a_m = mem.attend(att, q, qm, c["albums"])
    assert len(mem) == c["P"]
    assert torch.equal(ha_n, ha_ops) and torch.equal(a_n, a_ops) and torch.equal(ha_m, ha_ops) and torch.equal(a_m, a_ops)
    with pytest.raises(RuntimeError, match="forward-only"):                  # the parameters require grad
        att.forward_pooled(pool, q, c["albums"], pm, qm)
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_pooled_raw(pool, q.clone().requires_grad_(), c["albums"], W, b, pm, qm, simiMatrix=2)
    with torch.no_grad():                                                    # gradient mode off: allowed
        ha2, _ = Fn.attention_3d_pooled_raw(pool, q.clone().requires_grad_(), c["albums"], W, b, pm, qm, simiMatrix=2,
                                            add_tanh=True)
    assert torch.equal(ha2, ha_ops)


def test_functional_pads_the_width():
    """w = 100 runs at the kernels' 128: zero channels add nothing to any feature of any similarity form"""
    from fvta_memexqa_amd import functional as Fn
    w = 100
    c = R.make_case(R.lists_from_counts([3, 1, 2], 2, 7, True), 3, 2, 9, 5, w, 3, True, 71)
    ref_ha, ref_a = R.reference(c, True)
    with torch.no_grad():
        ha, a = Fn.attention_3d_pooled_raw(cu(c["pool"]), cu(c["q"]), c["albums"], cu(c["W"]), cu(c["b"]), cu(c["pm"]),
                                           cu(c["qm"]), simiMatrix=3, add_tanh=True)
    assert tuple(ha.shape) == (c["NQ"], w) and tuple(a.shape) == (c["NQ"], c["K"], c["T"], c["JQ"])
    close(ha, ref_ha, msg="h_a")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")


def test_from_context_agrees_with_the_per_question_forward(attn_select):
    from fvta_memexqa_amd import nn
    g = torch.Generator().manual_seed(11)
    N, K, M, JX, JQ, w = 3, 2, 4, 6, 5, 64
    hall = (torch.randn(N, K, M, JX, w, generator=g) * 0.5).cuda()
    mask = (torch.rand(N, K, M, JX, generator=g) < 0.6).cuda()
    hq = (torch.randn(N, JQ, w, generator=g) * 0.5).cuda()
    qm = torch.ones(N, JQ, dtype=torch.bool).cuda()
    att = nn.FocalAttention3D(w, simiMatrix=2, add_tanh=True, seed=5)
    attn_select.exact()                                                      # the fp32 route of the per-question kernel
    with torch.no_grad():
        ha_f, a_f = att.forward(hall, hq, mask, qm)
        mem, albums = nn.AlbumPool.from_context(hall, mask)
        assert len(mem) == N * M and tuple(albums.shape) == (N, M)
        ha_p, a_p = mem.attend(att, hq, qm, albums)
    print("from_context against forward(): max |h_a diff| %.3g, max |a_logits diff| %.3g"
          % (float((ha_p - ha_f).abs().max()), float((a_p - a_f).abs().max())))
    close(ha_p, ha_f, msg="h_a: the pool cut from the context against forward() on the context", **FP32)
    close(a_p, a_f, msg="a_logits", **FP32)
