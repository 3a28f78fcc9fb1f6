"""GPU parity of the shared-context focal attention (fvta_attn_shared_fwd, ops.SharedFocalAttention,
functional.attention_3d_shared_raw, nn.FocalAttention3D.forward_shared, nn.AlbumMemory) against the fp64 reference of
tests/_attn_shared_ref.py, at the tolerances of tests/test_gpu_forward.py (BASELINE.json north_star: 1e-4 relative).

The shapes (tests/_attn_shared_ref.py SPECS) are the smallest that turn every loop over: groups of 1, G, G+1 and 2G+1
questions and an album without one, row tiles at T = 1, 7, R-1, R, R+1, 333, question columns at JQ = 1, 30, 32, 33, 64,
every width from 64 to 2048, A = NQ = 1, K = 6; G and R are read from fvta_attn_shared_plan.

LOOP_SPECS there goes past one round of the plan's and the weighted sum's loops, on the training recipe (W scaled by
sqrt(64 / w), partly valid masks), each case asserting its regime through the plans' words before it launches: `many`
A = 1500 / NQ = 1284 (two albums per plan thread, 21 ordered batches, strided loops, ngmax clamped), `heavy` [150, 0, 50]
questions (19 groups of one album), `chunks` [2] x 120 at T = 200 (67 rows per split of the weighted sum: 64 + 3), and the
backward's `tiles-w64` / `-w512` / `-w2048` (T = 260 / 220 / 360), `k17`, `k64`."""
import pytest
import torch

from tests import _attn_shared_ref as R
from tests._album_attn_gpu import TrainRun, case, close, cu, infer

pytestmark = pytest.mark.gpu


def _case(name, simi, tanh, masked):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(R, (name, simi, tanh, masked), lambda key: R.build_case(name, simi, masked), lambda c: R.reference(c, tanh))


def _run(c, tanh, **kw):
    """ops.SharedFocalAttention on case c; rows: a subset of the questions (an index list), else all of them"""
    return infer(c, "shared", tanh=tanh, **kw)


def _expanded(c, tanh, want_logits=False):
    """today's route: index_select of the rows to [NQ,...], then the per-question kernel"""
    from fvta_memexqa_amd import ops
    al = c["album"].cuda()
    h = cu(c["h"]).index_select(0, al)
    hm = None if c["hm"] is None else cu(ops.as_mask_u8(c["hm"])).index_select(0, al)
    op = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], tanh)
    return op.forward(h, cu(c["q"]), hm, cu(ops.as_mask_u8(c["qm"])), None if c["W"] is None else cu(c["W"].reshape(-1)),
                      cu(c["b"]), want_logits=want_logits)


@pytest.mark.parametrize("name,simi,tanh,masked", R.CASES, ids=R.CASE_IDS)
def test_matches_the_fp64_reference(name, simi, tanh, masked):
    c, (ref_ha, ref_a) = _case(name, simi, tanh, masked)
    ha, a = _run(c, tanh)
    close(ha, ref_ha, msg="h_a")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")


def test_plan_is_what_the_shapes_assume():
    from fvta_memexqa_amd import ops
    p = ops.SharedFocalAttention(5, 40, 2, 50, 10, 64, 1, False).plan()
    assert p["G"] >= 8 and (p["G"], p["rows"]) == R.host_plan(10, 64)
    from tests import _attn_shared_bwd_ref as B
    op = ops.SharedFocalAttention(120, 240, 3, 200, 5, 64, 1, False)           # the handle's words are the host calls'
    assert op.plan() == R.host_plan_words(120, 240, 3, 200, 5, 64) and op.plan()["rows_per_split"] >= 1
    assert op.bwd_plan() == B.host_bwd_plan_words(120, 240, 3, 200, 5, 64) and op.bwd_plan()["tiles_per_wg"] >= 1
    assert ops.SharedFocalAttention(2, 5, 2, 40, 33, 128, 1, False).plan()["G"] >= 4


@pytest.mark.parametrize("name,simi,tanh,masked", [("mix", 2, True, True), ("rows5", 2, True, True)])
def test_same_result_as_the_per_question_kernel(name, simi, tanh, masked, attn_select):
    c, _ = _case(name, simi, tanh, masked)
    attn_select.exact()
    ref_ha, _ = _expanded(c, tanh)
    ha, _ = _run(c, tanh, want_logits=False)
    close(ha, ref_ha, rtol=2e-5, atol=2e-6, msg="h_a against the per-question exact kernel")


def test_a_question_does_not_depend_on_its_company():
    c, _ = _case("mix", 3, True, True)
    G, _ = R.host_plan(c["JQ"], c["w"])
    big = int(torch.bincount(c["album"], minlength=c["A"]).argmax())          # the album with 2G+1 questions
    members = torch.nonzero(c["album"] == big).reshape(-1)
    assert members.numel() == 2 * G + 1
    ha_all, a_all = _run(c, True)
    again_ha, again_a = _run(c, True)
    assert torch.equal(ha_all, again_ha) and torch.equal(a_all, again_a)       # the same call twice: the same bits
    i = int(members[G])
    ha_one, a_one = _run(c, True, rows=[i])
    close(ha_one[0], ha_all[i], rtol=2e-5, atol=2e-6, msg="alone against in company")
    close(a_one[0], a_all[i], rtol=2e-5, atol=2e-6)
    ha_nol, none = _run(c, True, want_logits=False)
    assert none is None and torch.equal(ha_nol, ha_all)                        # want_logits changes no bit of h_a


# ---- past one round of the plan and tile loops (R.LOOP_SPECS): many albums, many questions
def _loop_case(name):
    """a LOOP_SPECS case (the training recipe and, where the backward runs it too, its pinned seed) and its fp64 reference,
    evaluated in blocks of questions; once per session, never written to"""
    from tests import _attn_shared_bwd_ref as B
    return case(R, name, lambda n: R.loop_case(n, R.CHUNKS_SEED) if n in R.FORWARD_ONLY else B.build_case(n),
                lambda c: R.reference(c, c["tanh"], block=100))


@pytest.mark.parametrize("name", R.LOOP_IDS)
def test_loop_cases_match_the_fp64_reference(name):
    c, (ref_ha, ref_a) = _loop_case(name)
    run = TrainRun(c, "shared")                                  # the regime the case is named for: asserted before any launch
    R.loop_regime(name, c, run.op.plan(), None if name in R.FORWARD_ONLY else run.op.bwd_plan())
    ha, a = run.forward()
    live = ref_a > -1e29
    print("%s h_a: max |got - ref| %.3g, max |ref| %.3g" % (name, float((ha.cpu().double() - ref_ha).abs().max()),
                                                            float(ref_ha.abs().max())))
    print("%s a_logits: max |got - ref| over valid entries %.3g" % (name, float((a.cpu().double() - ref_a)[live].abs().max())))
    close(ha, ref_ha, msg="h_a")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")
    ha_t, a_t = run.forward_train()                              # the ordered plan: other places, the same bits
    assert torch.equal(ha_t, ha) and torch.equal(a_t, a)


@pytest.mark.parametrize("name", ["many", "heavy"])
def test_loop_cases_three_forward_calls_are_bitwise_equal(name):
    """the unordered plan's cursor atomics race across the waves of its workgroup here (NQ > 64): where a question lands
    changes no bit"""
    c, _ = _loop_case(name)
    outs = []
    for _ in range(3):
        outs.append(TrainRun(c, "shared").forward())             # a fresh handle: workspace and plan anew
    for ha, a in outs[1:]:
        assert torch.equal(ha, outs[0][0]) and torch.equal(a, outs[0][1])


def test_many_a_question_does_not_depend_on_its_company():
    c, _ = _loop_case("many")
    G, _ = R.host_plan(c["JQ"], c["w"])
    cnt = torch.bincount(c["album"], minlength=c["A"])
    ha_all, a_all = _run(c, c["tanh"])
    for size in (1, G, 2 * G + 1):                               # one question each of a 1-, a G- and a 2G+1-album
        album = int((cnt == size).nonzero()[-1])
        members = torch.nonzero(c["album"] == album).reshape(-1)
        assert members.numel() == size
        i = int(members[size // 2])
        ha_one, a_one = _run(c, c["tanh"], rows=[i])
        close(ha_one[0], ha_all[i], rtol=2e-5, atol=2e-6, msg="alone against in company, album of %d" % size)
        close(a_one[0], a_all[i], rtol=2e-5, atol=2e-6)


def test_functional_and_nn_surface():
    from fvta_memexqa_amd import functional as Fn, nn
    c, (ref_ha, ref_a) = _case("rows4", 1, False, True)                       # w = 256, simiMatrix 1, no tanh
    ha_ops, a_ops = _run(c, False)
    h, q, W, b = cu(c["h"]), cu(c["q"]), cu(c["W"]), cu(c["b"])
    hm, qm = cu(c["hm"]), cu(c["qm"])
    with torch.no_grad():
        ha, a = Fn.attention_3d_shared_raw(h, q, c["album"], W, b, hm, qm, simiMatrix=1, add_tanh=False)
    assert torch.equal(ha, ha_ops) and torch.equal(a, a_ops)
    qg = q.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="attention_3d"):
        Fn.attention_3d_shared_raw(h, qg, c["album"], W, b, hm, qm, simiMatrix=1)
    with torch.no_grad():                                                      # gradient mode off: allowed, nothing to detach
        ha2, _ = Fn.attention_3d_shared_raw(h, qg, c["album"], W, b, hm, qm, simiMatrix=1)
    assert torch.equal(ha2, ha_ops)
    with pytest.raises(ValueError):
        Fn.attention_3d_shared_raw(h, q, c["album"] + c["A"], W, b, hm, qm, simiMatrix=1)
    att = nn.FocalAttention3D(c["w"], simiMatrix=1, add_tanh=False)
    with torch.no_grad():
        att.p("att_logits/W").copy_(W)
        att.p("att_logits/b").copy_(b)
        al = c["album"].cuda()
        ha_f, a_f = att.forward(h.index_select(0, al), q, hm.index_select(0, al), qm)
        ha_s, a_s = att.forward_shared(h, q, c["album"], hm, qm)
    close(ha_s, ha_f, msg="forward_shared against forward")
    close(a_s, a_f, rtol=1e-4, atol=2e-5)
    close(ha_s, ref_ha)
    with pytest.raises(RuntimeError):                                          # the parameters require grad
        att.forward_shared(h, q, c["album"], hm, qm)


def test_album_memory_validates_before_any_library_call(monkeypatch):
    from fvta_memexqa_amd import nn, ops
    c, _ = _case("single", 1, False, True)
    mem = nn.AlbumMemory(cu(c["h"]), cu(c["hm"]))
    assert len(mem) == c["A"] and mem.hall.is_contiguous() and mem.hall.dtype == torch.float32
    assert not isinstance(mem, torch.nn.Module)                                # no parameters, no encoder
    att = nn.FocalAttention3D(c["w"], simiMatrix=1)

    def boom(*a, **k):
        raise AssertionError("the library was reached with an invalid index")
    monkeypatch.setattr(ops.SharedFocalAttention, "forward", boom)
    monkeypatch.setattr(ops.SharedFocalAttention, "__init__", boom)
    with torch.no_grad():
        for bad in (torch.tensor([c["A"]]), torch.tensor([-1]), torch.tensor([0.0]), torch.tensor([[0]])):
            with pytest.raises(ValueError):
                mem.attend(att, cu(c["q"]), cu(c["qm"]), bad)
        with pytest.raises(ValueError):
            mem.attend(att, cu(c["q"]), cu(c["qm"]), torch.tensor([0, 0]))   # two indices for one question


def test_end_to_end_many_questions_over_encoded_albums():
    """A = 2 albums encoded ONCE (two bi-LSTM streams -> context tensor), NQ = 5 questions through AlbumMemory,
    QuestionAttention and the scorer, against the per-question graph on the expanded context and the fp64 oracle."""
    from fvta_memexqa_amd import functional as Fn, nn, ops
    c = R.e2e_case()
    ref_logits, ref_yp = R.e2e_reference(c)
    margin = R.top2_margin(ref_yp)
    assert bool((margin > c["margin"]).all()), margin                          # the argmax check below excludes nothing
    A, M, w = c["A"], c["M"], 2 * c["hidden"]
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
        hq = c["hq"].cuda()
        qmask = (torch.arange(c["JQ"])[None, :] < c["qlen"][:, None]).cuda()
        ones = torch.ones(c["NQ"], 1, dtype=torch.bool, device="cuda")
        gch, oW, ob = c["gch"].cuda(), c["out_W"].reshape(-1).cuda(), c["out_b"].cuda()

        def head(g1):
            gq, _ = qatt(hq, g1[:, None, :].contiguous(), qmask, ones)
            logits, yp, _ = ops.scorer_ce_fwd(gq.contiguous(), g1.contiguous(), gch, oW, ob)
            return logits, yp

        mem = nn.AlbumMemory(hall, hall_mask)
        assert len(mem) == A
        g1_shared, _ = mem.attend(att, hq, qmask, c["album"])
        al = c["album"].cuda()
        g1_each, _ = att(hall.index_select(0, al), hq, hall_mask.index_select(0, al), qmask)
        logits_s, yp_s = head(g1_shared)
        logits_e, yp_e = head(g1_each)
    close(logits_s, logits_e, msg="shared against per-question")
    close(logits_s, ref_logits, msg="shared against the fp64 oracle")
    clear = margin > c["margin"]
    assert torch.equal(yp_s.argmax(-1).cpu()[clear], ref_yp.argmax(-1)[clear])
    assert torch.equal(yp_s.argmax(-1), yp_e.argmax(-1))
