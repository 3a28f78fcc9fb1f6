"""GPU parity of the shared-context focal attention under the time warp (fvta_attn_shared_energy / fvta_attn_shared_fwd_tw,
ops.SharedWarpedFocalAttention, functional.attention_3d_shared_warped_raw, nn.FocalAttention3D.forward_shared(time_warp=),
nn.AlbumMemory.attend(time_warp=)) against the fp64 definition of tests/_attn_shared_tw_ref.py -- gather, time_warp_closed,
attention_3d -- at the tolerances of tests/test_gpu_attn_shared.py, compared with tests/_album_attn_gpu.py's close:
h_a 1e-4 / 1e-5, a_logits 1e-4 / 2e-5, scale 1e-4 / 1e-5.

Conditioning: warp types 1, 3 and 4 multiply the rows by counts up to T, so the fp32 rounding of the warped rows' logits
grows with T while the a_logits tolerance stays absolute; types 2 and 5 scale by at most 2 ceil(window_t) + 1.  So types
1/3/4 come at T in {1, 7, 9}, types 2/5 at every shape, and the tolerance is not loosened.  The fp32 evaluation of the
same factorisation on the CPU (tests/test_attn_shared_tw_host.py) stays inside every tolerance on every shape here; on
the MI355X the worst ratio |err| / (atol + rtol |ref|) over all cases was 0.47 (a_logits at w = 1024), printed per case.

Shapes (tests/_attn_shared_tw_ref.SPECS): `mix` (groups of G+1, 1, 0, 2G+1, G questions) on all four similarities masked
and open; T = 1, 7, 9 on warp types 1, 3, 4; the tile edges T = R-1, R, R+1, 333 (the row -> scale index at tile
boundaries, the band clipped at both ends); windows 0.5, 3.0 and one wider than T; JQ = 32, 33, 64 at w = 128, 512;
w = 1024 and 2048 (two float4 per thread in the weighted sum, the energy's channel loop); K = 9 (past the time warp's own
fused-kernel limit of 8); LOOP_SPECS' `chunks` (the weighted sum's second, ragged staging round, with scales); zero rows
behind the mask, cosine included."""
import pytest
import torch

from tests import _attn_shared_ref as R
from tests import _attn_shared_tw_ref as TW
from tests._album_attn_gpu import album_energy, case, check_forward, close, cu, handle, infer, modules, warp_args

pytestmark = pytest.mark.gpu


def _case(name):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(TW, name, reference=lambda c: TW.reference(c, block=100))


def _energy(c, op=None):
    return album_energy(c, "shared", op)


def _run(c, **kw):
    """ops.SharedWarpedFocalAttention on case c -> (h_a, a_logits, scale); rows: a subset of the questions (an index list)"""
    return infer(c, "shared", True, **kw)


def _check(name, got, ref):
    check_forward(name, got, ref, TW.within)


@pytest.mark.parametrize("name", TW.NAMES + TW.EXTRA)
def test_matches_the_fp64_definition(name):
    c, ref = _case(name)
    if name == "chunks":
        from fvta_memexqa_amd import ops
        plan = ops.SharedFocalAttention(c["A"], c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"]).plan()
        R.loop_regime(name, c, plan)
    _check(name, _run(c), ref)


def test_energy_matches_and_is_the_album_s_alone():
    c, _ = _case("mix-simi2-masked")
    e = _energy(c)
    close(e, TW.energy(c), rtol=1e-4, atol=1e-5, msg="energy")
    assert torch.equal(e, _energy(c, handle(c, "shared", True, NQ=1)))                                # NQ does not enter
    c9, _ = _case("k9")
    close(_energy(c9), TW.energy(c9), rtol=1e-4, atol=1e-5, msg="energy, K = 9")
    cw, _ = _case("wide2048")
    close(_energy(cw), TW.energy(cw), rtol=1e-4, atol=1e-5, msg="energy, w = 2048")


def test_three_calls_are_bitwise_equal():
    c, _ = _case("mix-simi3-masked")
    outs = [_run(c) for _ in range(3)]                                          # fresh handles: workspace, plan and energy anew
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(x, y)
    ha_nol, none, s_nol = _run(c, want_logits=False)
    assert none is None and torch.equal(ha_nol, outs[0][0]) and torch.equal(s_nol, outs[0][2])


def test_a_question_does_not_depend_on_its_company():
    c, _ = _case("mix-simi3-masked")
    G, _ = R.host_plan(c["JQ"], c["w"])
    big = int(torch.bincount(c["album"], minlength=c["A"]).argmax())
    members = torch.nonzero(c["album"] == big).reshape(-1)
    assert members.numel() == 2 * G + 1
    ha_all, a_all, s_all = _run(c)
    i = int(members[G])
    ha_one, a_one, s_one = _run(c, rows=[i])
    # 2e-5, relative and absolute: another NQ is another split of T in the weighted sum, so another order of the same fp32
    # sum; the unwarped test's absolute 2e-6 times the largest |scale| of the band (2 * 3 + 1 = 7), rounded up
    close(ha_one[0], ha_all[i], rtol=2e-5, atol=2e-5, msg="alone against in company")
    close(a_one[0], a_all[i], rtol=2e-5, atol=2e-5)
    assert torch.equal(s_one[0], s_all[i])


def test_one_energy_serves_two_question_sets():
    c, _ = _case("mix-simi2-masked")
    e = _energy(c)
    ha_all, a_all, s_all = _run(c, energy=e)
    first, second = list(range(0, c["NQ"], 2)), list(range(1, c["NQ"], 2))
    for rows in (first, second):
        ha, a, s = _run(c, rows=rows, energy=e)
        close(ha, ha_all[rows], rtol=2e-5, atol=2e-5, msg="h_a of a question set against the whole call")
        close(a, a_all[rows], rtol=2e-5, atol=2e-5)
        assert torch.equal(s, s_all[rows])


def test_same_result_as_the_per_question_route():
    """index_select -> ops.TimeWarp -> ops.FocalAttention, at the sum of the two routes' own bounds against fp64"""
    from fvta_memexqa_amd import ops
    c, _ = _case("mix-simi2-masked")
    al = c["album"].cuda()
    rows = cu(c["h"]).index_select(0, al)
    hm = cu(ops.as_mask_u8(c["hm"])).index_select(0, al)
    tw = ops.TimeWarp(c["NQ"], c["K"], c["T"], c["w"], c["warp_type"], c["window_t"])
    warped = torch.empty_like(rows)
    tw.forward(rows, cu(c["lq"]), cu(c["WH_W"]), *warp_args(c), warped)
    per_q = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"])
    ref_ha, ref_a = per_q.forward(warped, cu(c["q"]), hm, cu(ops.as_mask_u8(c["qm"])), cu(c["W"].reshape(-1)), cu(c["b"]),
                                  want_logits=True)
    ha, a, s = _run(c)
    close(s, tw.scale, rtol=2e-4, atol=4e-5, msg="scale")
    close(a, ref_a, rtol=2e-4, atol=4e-5, msg="a_logits")
    close(ha, ref_ha, rtol=2e-4, atol=4e-5, msg="h_a")


# ------------------------------------------------------------------ the Python surface
def test_functional_nn_and_album_memory_give_the_ops_result():
    from fvta_memexqa_amd import functional as Fn, nn
    c, ref = _case("mix-simi2-masked")
    ha_ops, a_ops, s_ops = _run(c)
    h, q, lq, hm, qm = cu(c["h"]), cu(c["q"]), cu(c["lq"]), cu(c["hm"]), cu(c["qm"])
    wargs = (cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"]), cu(c["WC_b"]))
    kw = dict(simiMatrix=c["simi"], add_tanh=c["tanh"], warp_type=c["warp_type"], window_t=c["window_t"])
    with torch.no_grad():
        ha, a, s = Fn.attention_3d_shared_warped_raw(h, q, c["album"], lq, cu(c["W"]), cu(c["b"]), *wargs, hm, qm, **kw)
        e = Fn.album_energy(h, wargs[0], wargs[2])
        ha2, a2, s2 = Fn.attention_3d_shared_warped_raw(h, q, c["album"], lq, cu(c["W"]), cu(c["b"]), *wargs, hm, qm,
                                                        energy=e, **kw)
    for got in ((ha, a, s), (ha2, a2, s2)):
        assert torch.equal(got[0], ha_ops) and torch.equal(got[1], a_ops) and torch.equal(got[2], s_ops)
    att, tw = modules(c)
    with torch.no_grad():
        ha_n, a_n = att.forward_shared(h, q, c["album"], hm, qm, time_warp=tw, lq=lq)
        mem = nn.AlbumMemory(h, hm)
        ha_m, a_m = mem.attend(att, q, qm, c["album"], time_warp=tw, lq=lq)
        ha_m2, _ = mem.attend(att, q, qm, c["album"], time_warp=tw, lq=lq)     # the kept energy
        ha_plain, _ = mem.attend(att, q, qm, c["album"])                       # the defaults: today's call
        ha_unwarped, _ = att.forward_shared(h, q, c["album"], hm, qm)
    assert torch.equal(ha_n, ha_ops) and torch.equal(a_n, a_ops)
    assert torch.equal(ha_m, ha_ops) and torch.equal(a_m, a_ops) and torch.equal(ha_m2, ha_ops)
    assert torch.equal(ha_plain, ha_unwarped) and not torch.equal(ha_plain, ha_ops)
    close(ha_m, ref[0], msg="AlbumMemory.attend against the fp64 definition")


def test_a_padded_width_goes_through():
    """w = 40 is zero padded to the kernel width 64: the energy, WC . lq and the logits gain nothing from a zero channel"""
    from fvta_memexqa_amd import functional as Fn
    c = TW.add_warp(dict(R.make_case([3, 2], 2, 9, 5, 40, 2, True, 77), tanh=True), 77, 5)
    ref_ha, ref_a, ref_s = TW.reference(c)
    with torch.no_grad():
        ha, a, s = Fn.attention_3d_shared_warped_raw(cu(c["h"]), cu(c["q"]), c["album"], cu(c["lq"]), cu(c["W"]), cu(c["b"]),
                                                     cu(c["WH_W"]), cu(c["WH_b"]), cu(c["WC_W"]), cu(c["WC_b"]), cu(c["hm"]),
                                                     cu(c["qm"]), simiMatrix=2, add_tanh=True, warp_type=5, window_t=c["window_t"])
    assert ha.shape == (5, 40)
    _check("w40", (ha, a, s), (ref_ha, ref_a, ref_s))


def test_album_memory_never_serves_a_stale_energy():
    from fvta_memexqa_amd import nn
    c, _ = _case("mix-simi2-masked")
    att, tw = modules(c)
    h, q, lq, hm, qm = cu(c["h"]), cu(c["q"]), cu(c["lq"]), cu(c["hm"]), cu(c["qm"])
    mem = nn.AlbumMemory(h, hm)
    with torch.no_grad():
        ha0, _ = mem.attend(att, q, qm, c["album"], time_warp=tw, lq=lq)
        e0 = mem.energy(tw)
        assert mem.energy(tw) is e0                                            # kept
        tw.p("WH/W").mul_(1.5)                                                 # an in-place change of WH/W ...
        ha1, _ = mem.attend(att, q, qm, c["album"], time_warp=tw, lq=lq)
        assert mem.energy(tw) is not e0                                        # ... is seen by the next attend
        c15 = dict(c, WH_W=c["WH_W"] * 1.5)
        close(ha1, TW.reference(c15)[0], msg="after the in-place update")
        assert not torch.equal(ha1, ha0)
        sd = {k: v.clone() for k, v in tw.state_dict().items()}
        sd["WC/W"] = sd["WC/W"] * 0.5
        tw.load_state_dict(sd)                                                 # load_state_dict writes in place as well
        ha2, _ = mem.attend(att, q, qm, c["album"], time_warp=tw, lq=lq)
        close(ha2, TW.reference(dict(c15, WC_W=c["WC_W"] * 0.5))[0], msg="after load_state_dict")
        _, tw_b = modules(c)                                                  # another module, the first weights again
        ha3, _ = mem.attend(att, q, qm, c["album"], time_warp=tw_b, lq=lq)
        assert torch.equal(ha3, ha0)


def test_refusals():
    from fvta_memexqa_amd import _lib, functional as Fn, nn, ops
    c, _ = _case("mix-simi2-masked")
    att, tw = modules(c)
    h, q, lq, hm, qm = cu(c["h"]), cu(c["q"]), cu(c["lq"]), cu(c["hm"]), cu(c["qm"])
    with pytest.raises(RuntimeError, match="forward-only"):                    # gradient mode on, the parameters require grad
        att.forward_shared(h, q, c["album"], hm, qm, time_warp=tw, lq=lq)
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_shared_warped_raw(h, q.clone().requires_grad_(), c["album"], lq, cu(c["W"]), cu(c["b"]), cu(c["WH_W"]),
                                          cu(c["WH_b"]), cu(c["WC_W"]), cu(c["WC_b"]), hm, qm, simiMatrix=2, warp_type=5)
    with pytest.raises(_lib.FvtaError, match="time warping type not implemented"):
        ops.SharedWarpedFocalAttention(2, 3, 2, 9, 5, 64, 2, True, 9)
    with pytest.raises(Exception, match="time warping type not implemented"):
        nn.TimeWarp(64, warp_type=0)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        att.forward_shared(h, q, c["album"], hm, qm, differentiable=True, time_warp=tw, lq=lq)


def test_lq_errors_are_raised_before_any_library_call(monkeypatch):
    from fvta_memexqa_amd import nn, ops
    c, _ = _case("mix-simi2-masked")
    att, tw = modules(c)
    h, q, lq, hm, qm = cu(c["h"]), cu(c["q"]), cu(c["lq"]), cu(c["hm"]), cu(c["qm"])
    mem = nn.AlbumMemory(h, hm)

    def boom(*a, **k):
        raise AssertionError("the library was reached with invalid arguments")
    for cls in (ops.SharedFocalAttention, ops.SharedWarpedFocalAttention):
        for meth in ("__init__", "forward"):
            monkeypatch.setattr(cls, meth, boom)
    monkeypatch.setattr(ops.SharedWarpedFocalAttention, "album_energy", boom)
    with torch.no_grad():
        for bad in (None, lq[:-1], lq[:, :-1], lq[None], lq.tolist()):
            with pytest.raises(ValueError, match="lq"):
                mem.attend(att, q, qm, c["album"], time_warp=tw, lq=bad)
            with pytest.raises(ValueError, match="lq"):
                att.forward_shared(h, q, c["album"], hm, qm, time_warp=tw, lq=bad)
        with pytest.raises(ValueError, match="time_warp"):                     # lq without the time warp
            mem.attend(att, q, qm, c["album"], lq=lq)
        with pytest.raises(ValueError, match="time_warp"):
            att.forward_shared(h, q, c["album"], hm, qm, lq=lq)
        with pytest.raises(ValueError):                                        # the index checks still come first
            mem.attend(att, q, qm, c["album"] + c["A"], time_warp=tw, lq=lq)


def test_end_to_end_many_questions_under_the_time_warp():
    """tests/_attn_shared_ref.E2E plus nn.TimeWarp(warp_type=5): two albums encoded once, five questions through
    AlbumMemory.attend(time_warp=), QuestionAttention and the scorer, against the per-question nn path (index_select,
    TimeWarp, FocalAttention3D) at 2e-4"""
    from fvta_memexqa_amd import functional as Fn, nn, ops
    c = R.e2e_case()
    A, M, w = c["A"], c["M"], 2 * c["hidden"]
    wp = TW.add_warp(dict(w=w, NQ=c["NQ"]), c["seed"], 5)                      # the warp's weights and lq: the tests' recipe
    lq = wp["lq"].cuda()
    with torch.no_grad():
        streams, masks = [], []
        for x, ln, k, b in zip(c["x"], c["lens"], c["lstm_k"], c["lstm_b"]):
            enc = nn.BiLSTMEncoder(c["din"], c["hidden"], share_fw_bw=True)
            enc.p("fw/basic_lstm_cell/kernel").copy_(k)
            enc.p("fw/basic_lstm_cell/bias").copy_(b)
            out, _ = enc(x.cuda(), ln.cuda())
            streams.append(out.reshape(A, M, x.shape[1], w))
            masks.append((torch.arange(x.shape[1])[None, :] < ln[:, None]).reshape(A, M, -1).cuda())
        hall, hall_mask = Fn.context_tensor(streams, masks)
        att = nn.FocalAttention3D(w, simiMatrix=c["simi"], add_tanh=c["tanh"])
        qatt = nn.QuestionAttention(w, simiMatrix=c["simi"], add_tanh=c["tanh"])
        for mod, W, b in ((att, c["att_W"], c["att_b"]), (qatt, c["qatt_W"], c["qatt_b"])):
            mod.p("att_logits/W").copy_(W)
            mod.p("att_logits/b").copy_(b)
        tw = nn.TimeWarp(w, warp_type=5, window_t=wp["window_t"])
        for name, key in (("WH/W", "WH_W"), ("WH/b", "WH_b"), ("WC/W", "WC_W"), ("WC/b", "WC_b")):
            tw.p(name).copy_(wp[key])
        hq = c["hq"].cuda()
        qmask = (torch.arange(c["JQ"])[None, :] < c["qlen"][:, None]).cuda()
        ones = torch.ones(c["NQ"], 1, dtype=torch.bool, device="cuda")
        gch, oW, ob = c["gch"].cuda(), c["out_W"].reshape(-1).cuda(), c["out_b"].cuda()

        def head(g1):
            gq, _ = qatt(hq, g1[:, None, :].contiguous(), qmask, ones)
            return ops.scorer_ce_fwd(gq.contiguous(), g1.contiguous(), gch, oW, ob)[0]

        mem = nn.AlbumMemory(hall, hall_mask)
        g1_shared, a_shared = mem.attend(att, hq, qmask, c["album"], time_warp=tw, lq=lq)
        al = c["album"].cuda()
        warped, scale = tw(hall.index_select(0, al), lq)
        g1_each, a_each = att(warped, hq, hall_mask.index_select(0, al), qmask)
        assert bool((scale < 0).any()) and bool((scale > 0).any())
        # 2e-4 of the largest magnitude: each route's own 1e-4 against fp64 (BASELINE.json north_star), added
        close(g1_shared, g1_each, rtol=2e-4, atol=2e-4 * float(g1_each.abs().max()), msg="g1")
        close(a_shared, a_each, rtol=2e-4, atol=4e-5, msg="a_logits")
        logits_s, logits_e = head(g1_shared), head(g1_each)
    close(logits_s, logits_e, rtol=2e-4, atol=2e-4 * float(logits_e.abs().max()), msg="shared-warped against per-question")
