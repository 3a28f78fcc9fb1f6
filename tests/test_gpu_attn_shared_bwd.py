"""GPU parity of the shared-context focal attention's training calls (fvta_attn_shared_fwd_train / fvta_attn_shared_bwd,
ops.SharedFocalAttention.forward_train / backward, autograd.shared_focal_attention, functional.attention_3d_shared[_raw],
nn.FocalAttention3D.forward_shared(differentiable=True)) against fp64 autograd of the oracle on h[album]
(tests/_attn_shared_bwd_ref.py), at the tolerance of tests/test_gpu_backward.py: rtol 1e-4, atol 1e-5 x max(1, max|ref|).

The shapes are the smallest that turn every loop over: groups of G+1, 1, 0, 2G+1 and G questions, T around the row pass's
tile (fvta_attn_shared_bwd_plan) and across a T split of the question pass, JQ = 1, 30, 32, 33, 64, every width from 64 to
2048, A = NQ = 1, K = 6; and, past one round of the plan's and the row pass's loops (tests/_attn_shared_ref.py LOOP_SPECS,
each asserting its regime through the two plans' words): `many` A = 1500 / NQ = 1284, `heavy` [150, 0, 50] questions,
`tiles-w64` / `-w512` / `-w2048` with two row tiles per workgroup (T = 260 / 220 / 360), `k17`, `k64`, `splits9` (nine T
splits of the question pass: the fold's eight-in-flight slot sum and its remainder).  The pinned seeds keep every arg-max clear in fp64 (tests/test_attn_shared_bwd_host.py); the
first test also holds the GPU's own logits to a quarter of the case's smallest gap."""
import pytest
import torch

from tests import _attn_shared_bwd_ref as B
from tests import _attn_shared_ref as R
from tests._album_attn_gpu import TrainRun, case, close_scaled, cu

pytestmark = pytest.mark.gpu


def _case(name):
    """the case and its fp64 reference, computed once per session and never written to"""
    return case(B, name)


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_gradients_match_fp64_autograd(name):
    c, ref = _case(name)
    run = TrainRun(c, "shared")
    R.loop_regime(name, c, run.op.plan(), run.op.bwd_plan())    # a LOOP_SPECS case reaches its loop, before any launch
    ha, a = run.forward_train()
    # the arg-max the backward routes through is the reference's: the GPU's logits are within a quarter of the smallest gap
    jgap, tgap, _ = B.conditions(c, ref["a_logits"])
    v = B.valid_mask(c)
    err = float((a.cpu().double() - ref["a_logits"])[v].abs().max())
    print("%s: max |a_logits - fp64| over valid entries %.3g, smallest gap %.3g" % (name, err, min(jgap, tgap)))
    assert err < min(jgap, tgap) / 4, (err, jgap, tgap)
    close_scaled(ha, ref["h_a"], msg="h_a")
    dh, dq, dW, db = run.backward()                              # d_hinfo / d_hq prefilled with 7.0: overwritten
    for got, key in ((dh, "dh"), (dq, "dq"), (dW, "dW"), (db, "db")):
        print("%s %s: max |got - ref| %.3g, max |ref| %.3g" % (name, key, float((got.cpu().double() - ref[key]).abs().max()),
                                                               float(ref[key].abs().max())))
    close_scaled(dh, ref["dh"], msg="d_hinfo")
    close_scaled(dq, ref["dq"], msg="d_hq")
    close_scaled(dW, ref["dW"], msg="dW")
    close_scaled(db, ref["db"], msg="db")
    empty = torch.bincount(c["album"], minlength=c["A"]) == 0
    if bool(empty.any()):                                        # albums without a question: exactly zero, not the 7.0
        assert float(dh.cpu()[empty].abs().max()) == 0.0
    dh2, dq2, dW2, db2 = run.backward(acc=(dW, db), fill=-3.0)   # a second call: dW / db accumulate, the others do not
    close_scaled(dW2, 2 * ref["dW"], atol=2e-5, msg="dW accumulates")
    close_scaled(db2, 2 * ref["db"], atol=2e-5, msg="db accumulates")
    close_scaled(dh2, ref["dh"], msg="d_hinfo overwritten")
    close_scaled(dq2, ref["dq"], msg="d_hq overwritten")


def test_same_result_as_the_per_question_route(attn_select):
    """The masked `mix` case as make_case leaves it: a fully masked (album, k), a single-row (album, k), a fully masked
    question and an album without a question.  The contract is the expanded per-question route: index_select,
    ops.FocalAttention forward + backward (accumulate = 0), index_add_ of the row gradient.  Zeros: the question-less
    album's rows, and every masked row -- except where fvta_attn_bwd itself writes one: a fully masked QUESTION's
    softmax is uniform over all T rows of every k of its album, masked ones included (p r g, no logit gradient), so
    that album's masked rows hold exactly that term and are compared like all others."""
    from fvta_memexqa_amd import ops
    c = B.build_case(B.MIX_MASKED, parity=False)
    run = TrainRun(c, "shared")
    run.forward_train(want_logits=False)
    dh, dq, dW, db = run.backward()
    attn_select.exact()
    h, hm, q, qm, al, W, b = run.args
    al64 = al.long()
    he, hme = h.index_select(0, al64), hm.index_select(0, al64)
    op = ops.FocalAttention(c["NQ"], c["K"], c["T"], c["JQ"], c["w"], c["simi"], c["tanh"])
    op.forward(he, q, hme, qm, W, b)
    dhe, dqe = torch.full_like(he, 7.0), torch.full_like(q, 7.0)
    dWe, dbe = torch.zeros_like(W), torch.zeros(1, device="cuda")
    op.backward(he, q, hme, qm, W, b, run.g, dhe, dqe, dWe, dbe, 0)
    dh_ref = torch.zeros_like(h).index_add_(0, al64, dhe)
    close_scaled(dh, dh_ref, msg="d_hinfo against index_add_ of the per-question gradient")
    close_scaled(dq, dqe, msg="d_hq")
    close_scaled(dW, dWe, msg="dW")
    close_scaled(db, dbe, msg="db")
    cnt = torch.bincount(c["album"], minlength=c["A"])
    empty = int((cnt == 0).nonzero()[0])
    assert float(dh[empty].abs().max()) == 0.0                   # the album without a question: exactly zero
    fully_masked_q = (~c["qm"].any(-1)).nonzero().reshape(-1)
    assert fully_masked_q.numel() == 1
    spread = set(c["album"][fully_masked_q].tolist())            # albums whose masked rows carry a uniform softmax
    checked = 0
    for a in range(c["A"]):
        if a in spread:
            continue
        masked_rows = ~c["hm"][a]                                # [K,T]
        assert float(dh[a].cpu()[masked_rows].abs().max()) == 0.0
        checked += int(masked_rows.sum())
    assert checked > 0
    assert float(dq[int(fully_masked_q[0])].abs().max()) == 0.0  # nothing passes into a fully masked question


@pytest.mark.parametrize("name", ["mix-simi2-masked", "cols-jq33-w128", "rows-T333", "wide2048"])
def test_forward_train_has_the_bits_of_the_inference_forward(name):
    c, _ = _case(name)
    run = TrainRun(c, "shared")
    ha_t, a_t = run.forward_train()
    ha_i, a_i = run.forward()
    assert torch.equal(ha_t, ha_i) and torch.equal(a_t, a_i)
    ha_n, none = run.forward_train(want_logits=False)
    assert none is None and torch.equal(ha_n, ha_i)


@pytest.mark.parametrize("name", ["mix-simi3-masked", "rows-T333", "cols-jq64-w512", "many", "heavy", "tiles-w64", "splits9"])
def test_three_backward_calls_are_bitwise_equal(name):
    """`many` and `heavy`: an album's questions span several batches of the ordered plan, whose promise this is;
    `splits9`: the fold sums nine slots per question, eight of them in flight at a time"""
    c, _ = _case(name)
    outs = []
    for _ in range(3):
        run = TrainRun(c, "shared")                              # a fresh handle: plan, saved and workspace anew
        run.forward_train(want_logits=False)
        outs.append(run.backward())
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)


def test_a_questions_gradient_does_not_depend_on_its_company():
    c, _ = _case("mix-simi3-masked")
    G, _ = R.host_plan(c["JQ"], c["w"])
    big = int(torch.bincount(c["album"], minlength=c["A"]).argmax())          # the album with 2G+1 questions
    members = torch.nonzero(c["album"] == big).reshape(-1)
    assert members.numel() == 2 * G + 1
    run = TrainRun(c, "shared")
    run.forward_train(want_logits=False)
    _, dq_all, _, _ = run.backward()
    i = int(members[G])
    one = TrainRun(c, "shared", rows=[i])
    one.forward_train(want_logits=False)
    dh_one, dq_one, _, _ = one.backward()
    close_scaled(dq_one[0], dq_all[i], msg="d_hq alone against in company")
    others = [a for a in range(c["A"]) if a != big]
    assert float(dh_one[others].abs().max()) == 0.0                            # and it reaches its own album only


def test_functional_and_nn_surface():
    from fvta_memexqa_amd import functional as Fn, nn
    c, ref = _case("rows-TRb+1")                                               # w = 256
    h, q, W, b = (cu(c[k]).requires_grad_() for k in ("h", "q", "W", "b"))
    hm, qm, g = cu(c["hm"]), cu(c["qm"]), cu(c["gout"])
    ha, a = Fn.attention_3d_shared_raw(h, q, c["album"], W, b, hm, qm, simiMatrix=c["simi"], add_tanh=c["tanh"],
                                       differentiable=True)
    assert ha.requires_grad and not a.requires_grad
    (ha * g).sum().backward()
    close_scaled(ha, ref["h_a"])
    close_scaled(h.grad, ref["dh"], msg="functional d_hinfo")
    close_scaled(q.grad, ref["dq"], msg="functional d_hq")
    close_scaled(W.grad.reshape(-1), ref["dW"], msg="functional dW")
    close_scaled(b.grad, ref["db"], msg="functional db")
    with pytest.raises(RuntimeError, match="attention_3d"):                    # the default still refuses under gradient mode
        Fn.attention_3d_shared_raw(h, q, c["album"], W, b, hm, qm, simiMatrix=c["simi"], add_tanh=c["tanh"])
    with pytest.raises(NotImplementedError):
        Fn.attention_3d_shared_raw(h, q, c["album"], None, None, hm, qm, simiMatrix=4, differentiable=True)

    att = nn.FocalAttention3D(c["w"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    with torch.no_grad():
        att.p("att_logits/W").copy_(cu(c["W"]))
        att.p("att_logits/b").copy_(cu(c["b"]))
    h2, q2 = cu(c["h"]).requires_grad_(), cu(c["q"]).requires_grad_()
    ha2, a2 = att.forward_shared(h2, q2, c["album"], hm, qm, differentiable=True)
    assert not a2.requires_grad
    (ha2 * g).sum().backward()
    close_scaled(h2.grad, ref["dh"], msg="nn d_hinfo")
    close_scaled(q2.grad, ref["dq"], msg="nn d_hq")
    close_scaled(att.p("att_logits/W").grad.reshape(-1), ref["dW"], msg="nn dW")
    close_scaled(att.p("att_logits/b").grad, ref["db"], msg="nn db")
    with pytest.raises(RuntimeError):
        att.forward_shared(h2, q2, c["album"], hm, qm)
    with pytest.raises(NotImplementedError):
        nn.FocalAttention3D(c["w"], simiMatrix=4).forward_shared(h2, q2, c["album"], hm, qm, differentiable=True)

    # the scope's att_logits variables, as attention_3d has them: the same variables, the same result
    Fn.reset_default_graph()
    try:
        with torch.no_grad():
            al = c["album"].cuda()
            ha_each, _ = Fn.attention_3d(cu(c["h"]).index_select(0, al), cu(c["q"]), hm.index_select(0, al), qm,
                                         simiMatrix=c["simi"], add_tanh=c["tanh"], scope="att")
        names = set(Fn.variables)
        h3 = cu(c["h"]).requires_grad_()
        ha3, a3 = Fn.attention_3d_shared(h3, cu(c["q"]), c["album"], hm, qm, simiMatrix=c["simi"], add_tanh=c["tanh"],
                                         scope="att")
        assert set(Fn.variables) == names and any(n.endswith("att_logits/W") for n in names)
        assert ha3.requires_grad and not a3.requires_grad
        close_scaled(ha3, ha_each, msg="attention_3d_shared against attention_3d on gathered rows")
        ha3.sum().backward()
        assert h3.grad is not None and float(h3.grad.abs().max()) > 0
    finally:
        Fn.reset_default_graph()


def test_unpadded_width_goes_through_channel_padding():
    from fvta_memexqa_amd import functional as Fn
    c = B.odd_width_case()                                                     # w = 100 -> the 128-wide kernels
    ref = B.reference(c)
    assert B.qualifies(c, ref["a_logits"])
    h, q, W, b = (cu(c[k]).requires_grad_() for k in ("h", "q", "W", "b"))
    ha, a = Fn.attention_3d_shared_raw(h, q, c["album"], W, b, cu(c["hm"]), cu(c["qm"]), simiMatrix=c["simi"],
                                       add_tanh=c["tanh"], differentiable=True)
    assert tuple(ha.shape) == (c["NQ"], 100)
    (ha * cu(c["gout"])).sum().backward()
    close_scaled(ha, ref["h_a"])
    close_scaled(h.grad, ref["dh"], msg="d_hinfo")
    close_scaled(q.grad, ref["dq"], msg="d_hq")
    close_scaled(W.grad.reshape(-1), ref["dW"], msg="dW")
    close_scaled(b.grad, ref["db"], msg="db")


def test_end_to_end_training_over_albums_encoded_once():
    """A = 2 albums encoded ONCE by two bi-LSTM encoders -> context tensor -> shared differentiable attention (NQ = 5)
    -> question attention -> scorer loss -> backward(); every parameter gradient and hq.grad against the same graph on
    hall.index_select(0, album) through forward()."""
    from fvta_memexqa_amd import functional as Fn, nn
    c = R.e2e_case()
    A, M, w = c["A"], c["M"], 2 * c["hidden"]
    y = torch.zeros(c["NQ"], c["C"])
    y[torch.arange(c["NQ"]), torch.randint(0, c["C"], (c["NQ"],), generator=torch.Generator().manual_seed(11))] = 1.0
    encs = [nn.BiLSTMEncoder(c["din"], c["hidden"], share_fw_bw=True) for _ in c["x"]]
    att = nn.FocalAttention3D(w, simiMatrix=c["simi"], add_tanh=c["tanh"])
    qatt = nn.QuestionAttention(w, simiMatrix=c["simi"], add_tanh=c["tanh"])
    scorer = nn.AnswerScorer(w)
    with torch.no_grad():
        for enc, k, b in zip(encs, c["lstm_k"], c["lstm_b"]):
            enc.p("fw/basic_lstm_cell/kernel").copy_(k)
            enc.p("fw/basic_lstm_cell/bias").copy_(b)
        for mod, W, b in ((att, c["att_W"], c["att_b"]), (qatt, c["qatt_W"], c["qatt_b"])):
            mod.p("att_logits/W").copy_(W)
            mod.p("att_logits/b").copy_(b)
        scorer.p("choicelogits/W").copy_(c["out_W"])
        scorer.p("choicelogits/b").copy_(c["out_b"])
    mods = encs + [att, qatt, scorer]
    qmask = (torch.arange(c["JQ"])[None, :] < c["qlen"][:, None]).cuda()
    ones = torch.ones(c["NQ"], 1, dtype=torch.bool, device="cuda")
    al = c["album"].cuda()

    def step(shared):
        for m in mods:
            m.zero_grad(set_to_none=True)
        hq = c["hq"].cuda().requires_grad_()
        streams, masks = [], []
        for enc, x, ln in zip(encs, c["x"], c["lens"]):
            out, _ = enc(x.cuda(), ln.cuda())
            streams.append(out.reshape(A, M, x.shape[1], w))
            masks.append((torch.arange(x.shape[1])[None, :] < ln[:, None]).reshape(A, M, -1).cuda())
        hall, hall_mask = Fn.context_tensor(streams, masks)
        if shared:
            g1, _ = att.forward_shared(hall, hq, c["album"], hall_mask, qmask, differentiable=True)
        else:
            g1, _ = att(hall.index_select(0, al), hq, hall_mask.index_select(0, al), qmask)
        gq, _ = qatt(hq, g1[:, None, :].contiguous(), qmask, ones)
        loss = scorer(gq, g1, c["gch"].cuda(), y.cuda())[0]
        loss.sum().backward()
        grads = {"hq": hq.grad.clone(), "loss": loss.detach().clone()}
        for i, m in enumerate(mods):
            for n, p in m.named_parameters():
                assert p.grad is not None, (i, n)
                grads["%d/%s" % (i, n)] = p.grad.clone()
        return grads

    each, shared = step(False), step(True)
    assert set(each) == set(shared) and len(each) >= 2 + 2 * len(encs) + 6
    for key in each:
        close_scaled(shared[key], each[key], msg=key)
    assert float(each["0/" + next(n for n, _ in encs[0].named_parameters())].abs().max()) > 0
