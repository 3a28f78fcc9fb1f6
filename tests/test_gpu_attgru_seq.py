"""GPU parity of the AttentionGRU over a whole fact sequence (fvta_attgru_seq_fwd / _bwd) and of the differentiable DMN+
episodic memory built on it (autograd.attgru_seq / dmn_features / relu, functional.generate_episode / episodic_memory,
nn.AttentionGRU / EpisodicMemory) against fp64 autograd of the oracle: oracle.fvta_fused.attention_gru_cell looped F times,
and oracle.fvta_fused.dmn_memory.

Tolerances are those of tests/test_gpu_attgru.py: outputs rtol 2e-4 / atol 2e-5, every gradient tensor
|a - b|_2 <= 2e-4 |b|_2 + 1e-5.  Inputs: facts 0.5 randn, gates rand masked by random lengths that include F, 0 and 1,
h0 0.5 randn, weights randn 0.5 / sqrt(d), biases 0.1 randn."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRADS = ("d_facts", "d_gate", "d_h0", "dWg", "dbg", "dWc", "dWi", "dbi")
# (17, 3, 131), regime B: a last k-chunk of 3 columns, a last column tile of 3 units, a second row tile with one live row
SHAPES = [(5, 1, 16), (17, 2, 100), (33, 9, 80), (6, 33, 64), (1, 3, 64), (9, 5, 136), (65, 4, 256), (17, 3, 131)]


def _close_out(got, want, tag):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=2e-4, atol=2e-5, err_msg=tag)


def _close_grad(got, want, tag):
    assert got is not None, "%s: no gradient" % tag
    a, b = got.detach().cpu().double().numpy(), want.detach().double().numpy()
    err, ref = np.linalg.norm(a - b), np.linalg.norm(b)
    assert err <= 2e-4 * ref + 1e-5, "%s: |a-b| %.3g, |b| %.3g" % (tag, err, ref)


@functools.lru_cache(maxsize=None)
def _case(N, F, d, with_h0):
    """inputs (fp32, CPU) and the fp64 reference of one shape, computed once and shared"""
    from oracle import fvta_fused as O
    g = torch.Generator().manual_seed(100000 * N + 1000 * F + 2 * d + int(with_h0))
    facts = torch.randn(N, F, d, generator=g) * 0.5
    lens = torch.randint(0, F + 1, (N,), generator=g)
    special = [F, 0, 1][:N]
    lens[:len(special)] = torch.tensor(special)
    gate = torch.rand(N, F, generator=g) * (torch.arange(F)[None, :] < lens[:, None]).float()
    h0 = torch.randn(N, d, generator=g) * 0.5 if with_h0 else None
    s = 0.5 / d ** 0.5
    P = [torch.randn(2 * d, d, generator=g) * s, torch.randn(d, generator=g) * 0.1, torch.randn(d, d, generator=g) * s,
         torch.randn(d, d, generator=g) * s, torch.randn(d, generator=g) * 0.1]
    gout = torch.randn(N, d, generator=g)
    f64, g64 = facts.double().requires_grad_(), gate.double().requires_grad_()
    h64 = h0.double().requires_grad_() if with_h0 else None
    P64 = [p.double().requires_grad_() for p in P]
    state = h64 if with_h0 else torch.zeros(N, d, dtype=torch.float64)
    for t in range(F):
        state = O.attention_gru_cell(torch.cat([f64[:, t], g64[:, t:t + 1]], 1), state, *P64)
    (state * gout.double()).sum().backward()
    ref = dict(zip(GRADS, [f64.grad, g64.grad, h64.grad if with_h0 else None] + [p.grad for p in P64]))
    return dict(facts=facts, gate=gate, h0=h0, P=P, gout=gout, h_last=state.detach(), grads=ref)


def _run_autograd(c):
    """h_last and the gradients through autograd.attgru_seq (the accumulate = 0 path of the C ABI)"""
    from fvta_memexqa_amd import autograd
    leaf = lambda t: None if t is None else t.cuda().requires_grad_()
    facts, gate, h0 = leaf(c["facts"]), leaf(c["gate"]), leaf(c["h0"])
    P = [leaf(p) for p in c["P"]]
    h = autograd.attgru_seq(facts, gate, h0, *P)
    h.backward(c["gout"].cuda())
    return h, dict(zip(GRADS, [facts.grad, gate.grad, None if h0 is None else h0.grad] + [p.grad for p in P]))


def _check_case(N, F, d, with_h0):
    c = _case(N, F, d, with_h0)
    h, grads = _run_autograd(c)
    tag = "(%d,%d,%d,h0=%s)" % (N, F, d, with_h0)
    _close_out(h, c["h_last"], "h_last " + tag)
    for k in GRADS:
        if c["grads"][k] is not None:
            _close_grad(grads[k], c["grads"][k], k + " " + tag)
    return c, h, grads


@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("N,F,d", SHAPES)
def test_sequence_op_matches_the_oracle(N, F, d, with_h0):
    """h_last and all eight gradients with and without h0; accumulate = 0 (through autograd) and accumulate = 1 onto
    non-zero buffers (through ops.AttentionGRUSeq), d_facts / d_gate / d_h0 overwritten either way."""
    from fvta_memexqa_amd import ops
    if (N, F, d) == (17, 3, 131):
        assert ops.attgru_seq_plan(N, F, d)["regime"] == "B"
    c, _, _ = _check_case(N, F, d, with_h0)
    cu = lambda t: None if t is None else t.cuda().contiguous()
    facts, gate, h0, P = cu(c["facts"]), cu(c["gate"]), cu(c["h0"]), [cu(p) for p in c["P"]]
    op = ops.AttentionGRUSeq(N, F, d, training=True)
    h = op.forward(facts, gate, h0, *P)
    _close_out(h, c["h_last"], "h_last (ops)")
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(p.shape, generator=g) for p in c["P"]]
    acc = [cu(b.clone()) for b in base]
    junk = lambda *s: torch.full(s, 7.0, device="cuda")
    d_facts, d_gate, d_h0 = junk(N, F, d), junk(N, F), (junk(N, d) if with_h0 else None)
    op.backward(facts, gate, P[0], P[2], P[3], cu(c["gout"]), d_facts, d_gate, d_h0, *acc, accumulate=True)
    _close_grad(d_facts, c["grads"]["d_facts"], "d_facts (accumulate)")
    _close_grad(d_gate, c["grads"]["d_gate"], "d_gate (accumulate)")
    if with_h0:
        _close_grad(d_h0, c["grads"]["d_h0"], "d_h0 (accumulate)")
    for k, got, b in zip(GRADS[3:], acc, base):
        _close_grad(got, b.double() + c["grads"][k], k + " (accumulate)")


def test_plan_regimes_and_tile_edges():
    """N around the row tile the plan reports at d = 80, and both sides of the regime edge the plan reports."""
    from fvta_memexqa_amd import ops
    for d in (16, 64, 80, 100):
        assert ops.attgru_seq_plan(17, 3, d)["regime"] == "A", d
    RT = ops.attgru_seq_plan(17, 3, 80)["row_tile"]
    assert RT >= 1
    for N in (RT - 1, RT, RT + 1):
        if N >= 1:
            _check_case(N, 3, 80, True)
    edge = next((d for d in range(101, 514) if ops.attgru_seq_plan(17, 3, d)["regime"] == "B"), None)
    assert edge is not None, "no regime B up to d = 513"
    assert ops.attgru_seq_plan(17, 3, edge - 1)["regime"] == "A"
    _check_case(17, 3, edge - 1, True)
    _check_case(17, 3, edge, True)


def test_launch_counts_of_the_plan():
    """Regime A: the launches do not grow with F.  Regime B: F = 1 -> 48 adds at most 47 launches each way (one fused
    launch per step).  tools/bench_attgru_seq.py's kernel trace is the independent record of these counts."""
    from fvta_memexqa_amd import ops
    a2, a48 = ops.attgru_seq_plan(64, 2, 80), ops.attgru_seq_plan(64, 48, 80)
    assert a2["regime"] == a48["regime"] == "A"
    assert a2["fwd_launches"] == a48["fwd_launches"] and a2["bwd_launches"] == a48["bwd_launches"]
    b1, b48 = ops.attgru_seq_plan(64, 1, 512), ops.attgru_seq_plan(64, 48, 512)
    assert b1["regime"] == b48["regime"] == "B"
    assert 0 < b48["fwd_launches"] - b1["fwd_launches"] <= 47
    assert 0 < b48["bwd_launches"] - b1["bwd_launches"] <= 47


@pytest.mark.parametrize("N,F,d", [(33, 9, 80), (9, 5, 136)])
def test_runs_are_bitwise_repeatable(N, F, d):
    """two forward + backward runs agree bit for bit; a second backward over a retained graph equals the first (the
    backward only reads `saved`)."""
    from fvta_memexqa_amd import autograd
    c = _case(N, F, d, True)
    h1, g1 = _run_autograd(c)
    h2, g2 = _run_autograd(c)
    assert torch.equal(h1, h2)
    for k in GRADS:
        assert torch.equal(g1[k], g2[k]), k
    leaves = [t.cuda().requires_grad_() for t in [c["facts"], c["gate"], c["h0"]] + c["P"]]
    h = autograd.attgru_seq(*leaves)
    first = torch.autograd.grad(h, leaves, c["gout"].cuda(), retain_graph=True)
    second = torch.autograd.grad(h, leaves, c["gout"].cuda(), retain_graph=True)
    for k, a, b, r in zip(GRADS, first, second, [g1[k] for k in GRADS]):
        assert torch.equal(a, b) and torch.equal(a, r), k


def _episode64(mem, q, facts, lens, p):
    """model_dmnplus.py:113-136 in torch (any dtype) over oracle.fvta_fused.attention_gru_cell; p: fc1_W .. bi"""
    from oracle import fvta_fused as O
    N, F, d = facts.shape
    q3, m3 = q[:, None, :], mem[:, None, :]
    feats = torch.cat([facts * q3, facts * m3, (facts - q3).abs(), (facts - m3).abs()], 2)
    a1 = torch.tanh(feats @ p["fc1_W"] + p["fc1_b"])
    att = torch.softmax((a1 @ p["fc2_W"] + p["fc2_b"])[..., 0], 1)
    g = att * (torch.arange(F)[None, :] < lens[:, None]).to(facts.dtype)
    state = torch.zeros(N, d, dtype=facts.dtype)
    for t in range(F):
        state = O.attention_gru_cell(torch.cat([facts[:, t], g[:, t:t + 1]], 1), state, p["Wg"], p["bg"], p["Wc"], p["Wi"], p["bi"])
    return state


def test_generate_episode_gradient_flows():
    """functional.generate_episode over two hops with requires_grad on the facts, the question, the memory and the nine
    variables: every gradient exists and matches fp64 autograd.  (Before the episode ran on autograd.attgru_seq /
    dmn_features the result had no grad_fn towards the facts, the question, the memory and the cell.)"""
    from fvta_memexqa_amd import functional as Fn
    Fn.reset_default_graph()
    g = torch.Generator().manual_seed(9)
    N, F, d = 5, 11, 64
    facts = torch.randn(N, F, d, generator=g) * 0.5
    q = torch.randn(N, d, generator=g) * 0.5
    mem = torch.randn(N, d, generator=g) * 0.5
    lens = torch.tensor([11, 7, 1, 4, 11])
    go = [torch.randn(N, d, generator=g) for _ in range(2)]
    with torch.no_grad():                                       # creates the nine variables
        Fn.generate_episode(mem.cuda(), q.cuda(), facts.cuda(), lens, 0, d, scope="memory")
    names = dict(fc1_W="memory/attention/fc1/weights", fc1_b="memory/attention/fc1/biases", fc2_W="memory/attention/fc2/weights",
                 fc2_b="memory/attention/fc2/biases", Wg="memory/attention_gru/attention_gru_cell/gates/weights",
                 bg="memory/attention_gru/attention_gru_cell/gates/biases", Wc="memory/attention_gru/attention_gru_cell/candidate/weights",
                 Wi="memory/attention_gru/attention_gru_cell/input/weights", bi="memory/attention_gru/attention_gru_cell/input/biases")
    assert sorted(names.values()) == sorted(Fn.variables)
    for k, n in names.items():
        if k.endswith("_b") or k in ("bg", "bi"):
            Fn.variables[n].copy_((torch.randn(Fn.variables[n].shape, generator=g) * 0.1).cuda())
        Fn.variables[n].requires_grad_()
    f_c, q_c, m_c = (t.cuda().requires_grad_() for t in (facts, q, mem))
    ep1 = Fn.generate_episode(m_c, q_c, f_c, lens, 0, d, scope="memory")
    ep2 = Fn.generate_episode(ep1, q_c, f_c, lens, 1, d, scope="memory")
    assert len(Fn.variables) == 9
    ((ep1 * go[0].cuda()).sum() + (ep2 * go[1].cuda()).sum()).backward()
    p64 = {k: Fn.variables[n].detach().cpu().double().requires_grad_() for k, n in names.items()}
    f64, q64, m64 = (t.double().requires_grad_() for t in (facts, q, mem))
    r1 = _episode64(m64, q64, f64, lens, p64)
    r2 = _episode64(r1, q64, f64, lens, p64)
    ((r1 * go[0].double()).sum() + (r2 * go[1].double()).sum()).backward()
    _close_out(ep1, r1, "episode 1")
    _close_out(ep2, r2, "episode 2")
    _close_grad(f_c.grad, f64.grad, "d_facts")
    _close_grad(q_c.grad, q64.grad, "d_question")
    _close_grad(m_c.grad, m64.grad, "d_memory")
    for k, n in names.items():
        _close_grad(Fn.variables[n].grad, p64[k].grad, n)
    Fn.reset_default_graph()


def test_episodic_memory_module_and_functional():
    """nn.EpisodicMemory and functional.episodic_memory at (6, 9, 64), 3 hops, non-zero biases: output and the 13 + 2
    gradients against autograd of oracle.fvta_fused.dmn_memory; state_dict() keys; one Adadelta step moves every
    parameter.  (fc2's bias shifts every logit of the softmax alike, so its true gradient is 0 and a plain step leaves it
    where it is to the last bit: the step runs with weight decay, which every parameter that the optimizer reaches
    feels; that the gradients themselves are right is what the comparison above it checks.)"""
    from fvta_memexqa_amd import dmn, functional as Fn, nn
    from oracle import fvta_fused as O
    g = torch.Generator().manual_seed(21)
    N, F, d, hops = 6, 9, 64, 3
    facts = torch.randn(N, F, d, generator=g) * 0.5
    gq = torch.randn(N, d, generator=g) * 0.5
    lens = torch.tensor([9, 5, 1, 9, 3, 7])
    d_out = torch.randn(N, d, generator=g)
    mod = nn.EpisodicMemory(d, hops, seed=3)
    want_keys = sorted(k[len("memory/"):] for k in dmn.EpisodicMemory(d, hops, seed=3).params)
    assert sorted(mod.state_dict()) == want_keys and len(want_keys) == 9 + 2 * hops
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("biases") or k.endswith("bias"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).cuda())
    p64 = {"memory/" + k: p.detach().cpu().double().requires_grad_() for k, p in mod.named_parameters()}
    gq64, f64 = gq.double().requires_grad_(), facts.double().requires_grad_()
    ref = O.dmn_memory(gq64, f64, lens, p64, hops)
    (ref * d_out.double()).sum().backward()

    # ---- the module
    gq_c, f_c = gq.cuda().requires_grad_(), facts.cuda().requires_grad_()
    out = mod(gq_c, f_c, lens)
    out.backward(d_out.cuda())
    _close_out(out, ref, "nn.EpisodicMemory")
    _close_grad(gq_c.grad, gq64.grad, "d_gq")
    _close_grad(f_c.grad, f64.grad, "d_facts")
    for k, p in mod.named_parameters():
        _close_grad(p.grad, p64["memory/" + k].grad, k)

    # ---- the functional form on the same values (its cell lives under attention_gru/attention_gru_cell, without "rnn")
    Fn.reset_default_graph()
    with torch.no_grad():
        Fn.episodic_memory(gq.cuda(), facts.cuda(), lens, hops, d)
    assert len(Fn.variables) == 9 + 2 * hops
    fn_name = lambda k: "memory/" + k.replace("attention_gru/rnn/", "attention_gru/")
    for k, p in mod.named_parameters():
        Fn.variables[fn_name(k)].copy_(p.detach())
        Fn.variables[fn_name(k)].requires_grad_()
    gq_c2, f_c2 = gq.cuda().requires_grad_(), facts.cuda().requires_grad_()
    out2 = Fn.episodic_memory(gq_c2, f_c2, lens, hops, d)
    out2.backward(d_out.cuda())
    assert len(Fn.variables) == 9 + 2 * hops
    _close_out(out2, ref, "functional.episodic_memory")
    _close_grad(gq_c2.grad, gq64.grad, "d_gq (functional)")
    _close_grad(f_c2.grad, f64.grad, "d_facts (functional)")
    for k, p in mod.named_parameters():
        _close_grad(Fn.variables[fn_name(k)].grad, p64["memory/" + k].grad, fn_name(k))
    Fn.reset_default_graph()

    # ---- one optimizer step
    before = {k: p.detach().clone() for k, p in mod.named_parameters()}
    opt = torch.optim.Adadelta(mod.parameters(), lr=1.0, weight_decay=1e-2)
    opt.step()
    for k, p in mod.named_parameters():
        assert p.grad is not None and not torch.equal(p.detach(), before[k]), k


@pytest.mark.parametrize("N,F,d", [(17, 2, 100), (9, 5, 136)])
def test_no_grad_path_keeps_nothing(N, F, d, monkeypatch):
    """with nothing requiring grad the forward gives the same bits, runs with training = 0 and allocates no `saved`"""
    from fvta_memexqa_amd import autograd, ops
    made = []

    class Spy(ops.AttentionGRUSeq):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(ops, "AttentionGRUSeq", Spy)
    c = _case(N, F, d, True)
    args = [t.cuda() for t in [c["facts"], c["gate"], c["h0"]] + c["P"]]
    plain = autograd.attgru_seq(*args)
    assert plain.grad_fn is None and not plain.requires_grad
    args[0].requires_grad_()
    tracked = autograd.attgru_seq(*args)
    assert tracked.grad_fn is not None
    assert torch.equal(plain, tracked.detach())
    assert len(made) == 2
    assert made[0].desc.training == 0 and made[0].saved is None
    assert made[1].desc.training == 1 and made[1].saved is not None
    with pytest.raises(Exception):
        made[0].backward(*([None] * 14))
