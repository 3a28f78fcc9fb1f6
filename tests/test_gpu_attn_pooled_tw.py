"""GPU parity of the pooled focal attention under the time warp (fvta_attn_pool_energy / fvta_attn_pool_fwd_tw,
ops.PooledWarpedFocalAttention, functional.attention_3d_pooled_warped_raw, nn.FocalAttention3D.forward_pooled(time_warp=),
nn.AlbumPool.attend(time_warp=)) against the fp64 definition of tests/_attn_pooled_tw_ref.py (expand, time_warp_closed,
attention_3d), at the tolerances of tests/_attn_shared_tw_ref.TOL: h_a rtol 1e-4 / atol 1e-5, a_logits rtol 1e-4 / atol
2e-5, scale rtol 1e-4 / atol 1e-5.  tests/test_attn_pooled_tw_host.py holds every case to these tolerances on the CPU
(the kernels' factorisation evaluated in fp32), so a failure here is the kernels'.  Every index given to a GPU call is
valid."""
import pytest
import torch

from tests import _attn_pooled_ref as R
from tests import _attn_pooled_tw_ref as PT
from tests._album_attn_gpu import album_energy, case, check_forward, close, cu, handle, infer, modules, warp_args

pytestmark = pytest.mark.gpu

FP32 = dict(rtol=2e-5, atol=2e-5)      # two fp32 routes under the band's scales (|scale| <= 7): tests/test_gpu_attn_shared_tw.py's


def _case(name):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(PT, name)


def _op(c, NQ=None, M=None):
    return handle(c, "pooled", True, NQ=NQ, M=M)


def _energy(c, op=None):
    return album_energy(c, "pooled", op)


def _run(c, **kw):
    """ops.PooledWarpedFocalAttention on case c -> (h_a, a_logits, scale); rows: a subset of the questions (an index list);
    albums / pool / pm: in place of the case's own; sentinels: the outputs hold NaN before the call"""
    return infer(c, "pooled", True, **kw)


def _check(name, got, ref):
    check_forward(name, got, ref, PT.within)


# ------------------------------------------------------------------ against the fp64 definition
@pytest.mark.parametrize("name", PT.NAMES)
def test_matches_the_fp64_definition(name):
    c, ref = _case(name)
    got = _run(c, sentinels=True)
    _check(name, got, ref)
    if name.startswith("all-empty"):                                            # a question without any album: exactly 0
        assert c["albums"][1].tolist() == [-1, -1]
        assert torch.equal(got[0][1].cpu(), torch.zeros(c["w"])) and bool((got[1][1] == R.NEG).all())


@pytest.mark.parametrize("name", PT.LOOP_NAMES)
def test_loop_cases_match_the_fp64_definition(name):
    c, ref = _case(name)
    R.loop_regime(name, c, _op(c).plan())                                       # before anything is launched
    _check(name, _run(c, sentinels=True), ref)


def test_energy_is_the_shared_call_s_bit_for_bit():
    """fvta_attn_pool_energy makes fvta_attn_shared_energy's two launches with A = P, T = JX"""
    from fvta_memexqa_amd import functional as Fn, ops
    for name in ("mix-simi2-masked", "k9", "wide2048-simi3", "rows5"):
        c, _ = _case(name)
        e = _energy(c)
        assert tuple(e.shape) == (c["P"], c["JX"])
        close(e, PT.energy(c), rtol=1e-4, atol=1e-5, msg="energy of %s" % name)
        shared = ops.SharedWarpedFocalAttention(c["P"], 1, c["K"], c["JX"], 1, c["w"], 1, False, 1)
        assert torch.equal(e, shared.album_energy(cu(c["pool"]), cu(c["WH_W"]), cu(c["WC_W"].reshape(-1))))
        assert torch.equal(e, _energy(c, _op(c, 1, 1)))                         # NQ and M do not enter
        with torch.no_grad():
            assert torch.equal(e, Fn.album_energy(cu(c["pool"]), cu(c["WH_W"]), cu(c["WC_W"])))      # a 4-D pool


# ------------------------------------------------------------------ M = 1 is the shared call under the warp
@pytest.mark.parametrize("simi,masked", [(1, True), (2, False), (4, True)])
def test_one_slot_is_the_shared_call_bit_for_bit(simi, masked):
    from tests import _attn_shared_tw_ref as TW
    from fvta_memexqa_amd import ops
    c = TW.build_case("mix-simi%d-%s" % (simi, "masked" if masked else "open"))
    rows = (cu(c["h"]), cu(ops.as_mask_u8(c["hm"])))
    Wb = (None if c["W"] is None else cu(c["W"].reshape(-1)), cu(c["b"]))
    wargs = (cu(c["WH_b"]), cu(c["WC_W"].reshape(-1)), cu(c["WC_b"]))
    shared = ops.SharedWarpedFocalAttention(c["A"], c["NQ"], c["K"], c["T"], c["JQ"], c["w"], simi, c["tanh"], 5, c["window_t"])
    e = shared.album_energy(rows[0], cu(c["WH_W"]), wargs[1])
    ha_s, a_s, s_s = shared.forward(*rows, e, cu(c["q"]), cu(ops.as_mask_u8(c["qm"])), cu(c["lq"]),
                                    ops.check_album_index(c["album"], c["A"]).cuda(), *Wb, *wargs, want_logits=True, want_scale=True)
    pooled = ops.PooledWarpedFocalAttention(c["A"], c["NQ"], 1, c["K"], c["T"], c["JQ"], c["w"], simi, c["tanh"], 5, c["window_t"])
    assert pooled.plan() == shared_plan(c, simi)
    e_p = pooled.album_energy(rows[0], cu(c["WH_W"]), wargs[1])
    ha_p, a_p, s_p = pooled.forward(*rows, e_p, cu(c["q"]), cu(ops.as_mask_u8(c["qm"])), cu(c["lq"]),
                                    ops.check_album_lists(c["album"][:, None], c["A"], masked).cuda(), *Wb, *wargs,
                                    want_logits=True, want_scale=True)
    assert torch.equal(e_p, e) and torch.equal(s_p, s_s) and torch.equal(a_p, a_s) and torch.equal(ha_p, ha_s)


def shared_plan(c, simi):
    from fvta_memexqa_amd import ops
    return ops.SharedFocalAttention(c["A"], c["NQ"], c["K"], c["T"], c["JQ"], c["w"], simi, c["tanh"]).plan()


# ------------------------------------------------------------------ the shared call on the expanded contexts
@pytest.mark.parametrize("name", ["mix-simi2-masked", "mix-simi3-open"])
def test_logits_and_scale_are_the_expanded_shared_call_s_bits(name):
    """one context per question (A = NQ, T = M JX, album = arange) through ops.SharedWarpedFocalAttention: a column's chain
    and a row's terms do not depend on tile or group, so a_logits and scale are the same bits; h_a's merge order differs"""
    from fvta_memexqa_amd import ops
    c, _ = _case(name)
    h, m = R.expand(c)
    NQ, T = c["NQ"], c["T"]
    shared = ops.SharedWarpedFocalAttention(NQ, NQ, c["K"], T, c["JQ"], c["w"], c["simi"], c["tanh"], c["warp_type"], c["window_t"])
    e = shared.album_energy(cu(h), cu(c["WH_W"]), cu(c["WC_W"].reshape(-1)))
    ha_s, a_s, s_s = shared.forward(cu(h), cu(ops.as_mask_u8(m)), e, cu(c["q"]), cu(ops.as_mask_u8(c["qm"])), cu(c["lq"]),
                                    torch.arange(NQ, dtype=torch.int32).cuda(), None if c["W"] is None else cu(c["W"].reshape(-1)),
                                    cu(c["b"]), *warp_args(c), want_logits=True, want_scale=True)
    ha, a, s = _run(c)
    assert torch.equal(s, s_s) and torch.equal(a, a_s)
    close(ha, ha_s, msg="h_a against the shared call on the expanded contexts", **FP32)


# ------------------------------------------------------------------ the per-question route
@pytest.mark.parametrize("name", ["mix-simi2-masked", "rows4"])
def test_same_result_as_the_per_question_route(name):
    """gather -> ops.TimeWarp -> ops.FocalAttention, at the sum of the two routes' own bounds against fp64"""
    from fvta_memexqa_amd import ops
    c, _ = _case(name)
    h, m = R.expand(c)                                                          # [NQ,K,T,w]: what the pooled call never builds
    rows = cu(h)
    tw = ops.TimeWarp(c["NQ"], c["K"], c["T"], c["w"], c["warp_type"], c["window_t"])
    warped = torch.empty_like(rows)
    tw.forward(rows, cu(c["lq"]), cu(c["WH_W"]), *warp_args(c), warped)
    per_q = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"])
    ref_ha, ref_a = per_q.forward(warped, cu(c["q"]), cu(ops.as_mask_u8(m)), cu(ops.as_mask_u8(c["qm"])),
                                  cu(c["W"].reshape(-1)), cu(c["b"]), want_logits=True)
    ha, a, s = _run(c)
    close(s, tw.scale, rtol=2e-4, atol=2e-5, msg="scale")
    close(a, ref_a, rtol=2e-4, atol=4e-5, msg="a_logits")
    close(ha, ref_ha, rtol=2e-4, atol=2e-5, msg="h_a")


# ------------------------------------------------------------------ placement changes no bit
def test_two_calls_and_a_relabelled_pool_give_the_same_bits():
    c, _ = _case("mix-simi3-masked")
    first = _run(c)
    for x, y in zip(_run(c), first):                                            # fresh handles: workspace, plan and energy anew
        assert torch.equal(x, y)
    perm = torch.tensor([3, 0, 4, 1, 2])                                        # new label of album p: perm[p]
    pool, pm = torch.empty_like(c["pool"]), torch.empty_like(c["pm"])
    pool[perm], pm[perm] = c["pool"], c["pm"]
    al = torch.where(c["albums"] >= 0, perm[c["albums"].clamp(min=0)], c["albums"])
    for x, y in zip(_run(c, albums=al, pool=pool, pm=pm), first):               # other groups, the same bits
        assert torch.equal(x, y)
    ha_nol, none, s_nol = _run(c, want_logits=False)
    assert none is None and torch.equal(ha_nol, first[0]) and torch.equal(s_nol, first[2])


def test_a_question_does_not_depend_on_its_company():
    """JX = 17 is one split of the weighted sum whatever NQ, so h_a keeps its order of sums too: all three outputs, bit for bit"""
    c, _ = _case("mix-simi3-masked")
    assert _op(c).plan()["tsplit"] == 1 == _op(c, 1).plan()["tsplit"]
    ha, a, s = _run(c)
    twice = next(i for i, r in enumerate(c["albums"].tolist()) if min(r) >= 0 and len(set(r)) < len(r))
    for rows in ([0], [twice], [c["NQ"] - 1], [twice, 0, 3]):                   # the last: the empty slot, fully masked
        ha_r, a_r, s_r = _run(c, rows=rows)
        assert torch.equal(ha_r, ha[rows]) and torch.equal(a_r, a[rows]) and torch.equal(s_r, s[rows]), rows


def test_the_count_runs_over_the_whole_list():
    """a list's slots permuted: the blocks of tanh(z) move with their albums, the count stays with the position -- past (3)
    and future (4) tell the global t = m JX + j from the album's own j"""
    for name in ("short-M3-JX3-warp3-simi2", "short-M3-JX3-warp4-simi3"):
        c, _ = _case(name)
        order = [2, 0, 1]
        cp = dict(c, albums=c["albums"][:, order])
        s, sp = _run(c)[2].cpu().double(), _run(cp)[2].cpu()
        cnt = PT.TW._count(c["T"], c["warp_type"], c["window_t"], torch.float64)
        JX = c["JX"]
        moved = torch.cat([(s / cnt)[:, m * JX:(m + 1) * JX] for m in order], 1) * cnt
        close(sp, moved, rtol=1e-5, atol=1e-6, msg="scale after permuting the slots")
        close(sp, PT.scale_of(cp), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ the Python surface
def test_functional_nn_and_album_pool_give_the_ops_result():
    from fvta_memexqa_amd import functional as Fn, nn
    c, ref = _case("mix-simi2-masked")
    ha_ops, a_ops, s_ops = _run(c)
    pool, q, lq, pm, qm = cu(c["pool"]), cu(c["q"]), cu(c["lq"]), cu(c["pm"]), cu(c["qm"])
    wargs = (cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"]), cu(c["WC_b"]))
    kw = dict(pool_mask=pm, hq_mask=qm, simiMatrix=c["simi"], add_tanh=c["tanh"], warp_type=c["warp_type"], window_t=c["window_t"])
    with torch.no_grad():
        ha, a, s = Fn.attention_3d_pooled_warped_raw(pool, q, c["albums"], lq, cu(c["W"]), cu(c["b"]), *wargs, **kw)
        e = Fn.album_energy(pool, wargs[0], wargs[2])
        ha2, a2, s2 = Fn.attention_3d_pooled_warped_raw(pool, q, c["albums"].tolist(), lq, cu(c["W"]), cu(c["b"]), *wargs,
                                                        energy=e, **kw)
    for got in ((ha, a, s), (ha2, a2, s2)):
        assert torch.equal(got[0], ha_ops) and torch.equal(got[1], a_ops) and torch.equal(got[2], s_ops)
    att, tw = modules(c)
    with torch.no_grad():
        ha_n, a_n = att.forward_pooled(pool, q, c["albums"], pm, qm, time_warp=tw, lq=lq)
        mem = nn.AlbumPool(pool, pm)
        ha_m, a_m = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)
        ha_m2, _ = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)    # the kept energy
        ha_plain, _ = mem.attend(att, q, qm, c["albums"])                      # the defaults: today's call
        ha_unwarped, _ = att.forward_pooled(pool, q, c["albums"], pm, qm)
    assert torch.equal(ha_n, ha_ops) and torch.equal(a_n, a_ops)
    assert torch.equal(ha_m, ha_ops) and torch.equal(a_m, a_ops) and torch.equal(ha_m2, ha_ops)
    assert torch.equal(ha_plain, ha_unwarped) and not torch.equal(ha_plain, ha_ops)
    close(ha_m, ref[0], msg="AlbumPool.attend against the fp64 definition")


def test_a_padded_width_goes_through():
    """w = 40 is zero padded to the kernel width 64: the energy, WC . lq and the logits gain nothing from a zero channel"""
    from fvta_memexqa_amd import functional as Fn
    c = R.make_case(R.lists_from_counts([3, 1, 2], 2, 7, True), 3, 2, 9, 5, 40, 2, True, 77)
    c = PT.TW.add_warp(dict(c, tanh=True), 77, 5)
    ref = PT.reference(c)
    with torch.no_grad():
        got = Fn.attention_3d_pooled_warped_raw(cu(c["pool"]), cu(c["q"]), c["albums"], cu(c["lq"]), cu(c["W"]), cu(c["b"]),
                                                cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"]), cu(c["WC_b"]), cu(c["pm"]),
                                                cu(c["qm"]), simiMatrix=2, add_tanh=True, warp_type=5, window_t=c["window_t"])
    assert tuple(got[0].shape) == (c["NQ"], 40) and tuple(got[2].shape) == (c["NQ"], c["T"])
    _check("w40", got, ref)


def test_album_pool_never_serves_a_stale_energy():
    from fvta_memexqa_amd import nn
    c, _ = _case("mix-simi2-masked")
    att, tw = modules(c)
    pool, q, lq, pm, qm = cu(c["pool"]), cu(c["q"]), cu(c["lq"]), cu(c["pm"]), cu(c["qm"])
    mem = nn.AlbumPool(pool, pm)
    with torch.no_grad():
        ha0, _ = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)
        e0 = mem.energy(tw)
        assert mem.energy(tw) is e0 and tuple(e0.shape) == (c["P"], c["JX"])   # kept
        tw.p("WC/W").mul_(1.5)                                                 # an in-place change of WC/W ...
        ha1, _ = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)
        assert mem.energy(tw) is not e0                                        # ... is seen by the next attend
        c15 = dict(c, WC_W=c["WC_W"] * 1.5)
        close(ha1, PT.reference(c15)[0], msg="after the in-place update")
        assert not torch.equal(ha1, ha0)
        sd = {k: v.clone() for k, v in tw.state_dict().items()}
        sd["WH/W"] = sd["WH/W"] * 0.5
        tw.load_state_dict(sd)                                                 # load_state_dict writes in place as well
        ha2, _ = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)
        close(ha2, PT.reference(dict(c15, WH_W=c["WH_W"] * 0.5))[0], msg="after load_state_dict")
        _, tw_b = modules(c)                                                  # another module, the first weights again
        ha3, _ = mem.attend(att, q, qm, c["albums"], time_warp=tw_b, lq=lq)
        assert torch.equal(ha3, ha0)


def test_refusals():
    from fvta_memexqa_amd import _lib, functional as Fn, ops
    c, _ = _case("mix-simi2-masked")
    att, tw = modules(c)
    pool, q, lq, pm, qm = cu(c["pool"]), cu(c["q"]), cu(c["lq"]), cu(c["pm"]), cu(c["qm"])
    with pytest.raises(RuntimeError, match="forward-only.*per-question time_warp"):  # gradient mode on, the parameters require grad
        att.forward_pooled(pool, q, c["albums"], pm, qm, time_warp=tw, lq=lq)
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_pooled_warped_raw(pool, q.clone().requires_grad_(), c["albums"], lq, cu(c["W"]), cu(c["b"]),
                                          cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"]), cu(c["WC_b"]), pm, qm, simiMatrix=2,
                                          warp_type=5)
    with pytest.raises(_lib.FvtaError, match="time warping type not implemented"):
        ops.PooledWarpedFocalAttention(2, 3, 2, 2, 9, 5, 64, 2, True, 9)
    with torch.no_grad(), pytest.raises(ValueError, match="needs both masks"):
        att.forward_pooled(pool, q, c["albums"], None, None, time_warp=tw, lq=lq)


def test_from_context_agrees_with_the_per_question_time_warp_and_forward(attn_select):
    from fvta_memexqa_amd import nn
    g = torch.Generator().manual_seed(13)
    N, K, M, JX, JQ, w = 3, 2, 4, 6, 5, 64
    hall = (torch.randn(N, K, M, JX, w, generator=g) * 0.5).cuda()
    mask = (torch.rand(N, K, M, JX, generator=g) < 0.6).cuda()
    hq = (torch.randn(N, JQ, w, generator=g) * 0.5).cuda()
    lq = (torch.randn(N, w, generator=g) * 0.5).cuda()
    qm = torch.ones(N, JQ, dtype=torch.bool).cuda()
    att = nn.FocalAttention3D(w, simiMatrix=2, add_tanh=True, seed=5)
    tw = nn.TimeWarp(w, warp_type=5, window_t=2.3, seed=7)
    attn_select.exact()                                                      # the fp32 route of the per-question kernel
    with torch.no_grad():
        tw.p("WH/W").mul_(0.3 / 0.1 / w ** 0.5)                              # the tests' recipe for the warp's weights
        tw.p("WC/W").mul_(0.5 / 0.1 / w ** 0.5)
        tw.p("WH/b").copy_(torch.randn(w, generator=g) * 0.1)
        warped, scale = tw(hall, lq)
        ha_f, a_f = att.forward(warped, hq, mask, qm)
        mem, albums = nn.AlbumPool.from_context(hall, mask)
        ha_p, a_p = mem.attend(att, hq, qm, albums, time_warp=tw, lq=lq)
    print("from_context under the warp against TimeWarp + forward(): max |h_a diff| %.3g, max |a_logits diff| %.3g"
          % (float((ha_p - ha_f).abs().max()), float((a_p - a_f).abs().max())))
    # each route's own bound against fp64, added (tests/test_gpu_attn_shared_tw.py's end-to-end test)
    close(ha_p, ha_f, rtol=2e-4, atol=2e-5, msg="h_a: the pool cut from the context against TimeWarp + forward()")
    close(a_p, a_f, rtol=2e-4, atol=4e-5, msg="a_logits")
