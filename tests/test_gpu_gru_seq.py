"""GPU parity of the GRU over a whole sequence (fvta_gru_seq_fwd / _bwd, ops.GRUSeq, autograd.gru_seq) and of the modules
built on it (nn.GRUEncoder / BiGRUFusion / DMNPlusHead) against fp64 autograd of tests/_gru_ref.py -- TF's GRUCell under
dynamic_rnn, written from the formulas with the literal concats -- and, for the head, of that composed with
oracle.fvta_fused.dmn_memory.

Tolerances are those of tests/test_gpu_attgru_seq.py (the same arithmetic class, exact-fp32 MFMA recurrences): outputs
rtol 2e-4 / atol 2e-5, every gradient tensor |a - b|_2 <= 2e-4 |b|_2 + 1e-5.  Inputs: x and h0 0.5 randn, kernels
0.5 / sqrt(in + d) randn, bg = 1 + 0.1 randn, bc = 0.1 randn, lengths random in [0, T] with T, 0 and 1 in the first rows."""
import functools

import numpy as np
import pytest
import torch

from tests import _gru_ref as R

pytestmark = pytest.mark.gpu

GRADS = ("d_x", "d_h0", "dWg", "dbg", "dWc", "dbc")
SHAPES_A = [(1, 1, 4, 16), (5, 3, 7, 16), (17, 2, 37, 100), (33, 9, 24, 80), (6, 33, 12, 64), (16, 4, 100, 100)]
# (17, 3, 5, 131): a last k-chunk of 3 columns, a last column tile of 3 units, a second row tile with one live row
SHAPES_B = [(9, 5, 20, 136), (65, 4, 48, 256), (17, 3, 5, 131)]


def _close_out(got, want, tag):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=2e-4, atol=2e-5, err_msg=tag)


def _close_grad(got, want, tag):
    assert got is not None, "%s: no gradient" % tag
    a, b = got.detach().cpu().double().numpy(), want.detach().double().numpy()
    err, ref = np.linalg.norm(a - b), np.linalg.norm(b)
    assert err <= 2e-4 * ref + 1e-5, "%s: |a-b| %.3g, |b| %.3g" % (tag, err, ref)


def _cell_params(g, din, d):
    s = 0.5 / (din + d) ** 0.5
    return [torch.randn(din + d, 2 * d, generator=g) * s, 1 + 0.1 * torch.randn(2 * d, generator=g),
            torch.randn(din + d, d, generator=g) * s, 0.1 * torch.randn(d, generator=g)]


@functools.lru_cache(maxsize=None)
def _case(N, T, din, d, reverse, with_h0, use="both", full=False):
    """inputs (fp32, CPU) and the fp64 reference of one case, computed once and shared.  use: which outputs the loss
    reads ("both", "out", "last"); full: lens = None"""
    g = torch.Generator().manual_seed(1000003 * N + 10007 * T + 101 * din + 2 * d + int(with_h0))
    x = torch.randn(N, T, din, generator=g) * 0.5
    lens = torch.randint(0, T + 1, (N,), generator=g)
    special = [T, 0, 1][:N]
    lens[:len(special)] = torch.tensor(special)
    h0 = torch.randn(N, d, generator=g) * 0.5 if with_h0 else None
    P = _cell_params(g, din, d)
    g_out, g_last = torch.randn(N, T, d, generator=g), torch.randn(N, d, generator=g)
    x64 = x.double().requires_grad_()
    h64 = h0.double().requires_grad_() if with_h0 else None
    P64 = [p.double().requires_grad_() for p in P]
    out, last = R.gru_seq(x64, None if full else lens, h64, *P64, reverse=reverse)
    loss = 0
    if use in ("both", "out"):
        loss = loss + (out * g_out.double()).sum()
    if use in ("both", "last"):
        loss = loss + (last * g_last.double()).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    ref = dict(zip(GRADS, [zero(x64), zero(h64) if with_h0 else None] + [zero(p) for p in P64]))
    return dict(x=x, lens=None if full else lens, h0=h0, P=P, g_out=g_out, g_last=g_last, out=out.detach(), last=last.detach(),
                grads=ref, reverse=reverse, use=use)


def _run_autograd(c):
    """outputs and gradients through autograd.gru_seq (the accumulate = 0 path of the C ABI)"""
    from fvta_memexqa_amd import autograd
    leaf = lambda t: None if t is None else t.cuda().requires_grad_()
    x, h0, P = leaf(c["x"]), leaf(c["h0"]), [leaf(p) for p in c["P"]]
    out, last = autograd.gru_seq(x, c["lens"], h0, *P, reverse=c["reverse"])
    loss = 0
    if c["use"] in ("both", "out"):
        loss = loss + (out * c["g_out"].cuda()).sum()
    if c["use"] in ("both", "last"):
        loss = loss + (last * c["g_last"].cuda()).sum()
    loss.backward()
    return out, last, dict(zip(GRADS, [x.grad, None if h0 is None else h0.grad] + [p.grad for p in P]))


def _check_case(*key, **kw):
    c = _case(*key, **kw)
    out, last, grads = _run_autograd(c)
    tag = str(key) + str(kw)
    _close_out(out, c["out"], "out " + tag)
    _close_out(last, c["last"], "h_last " + tag)
    for k in GRADS:
        if c["grads"][k] is not None:
            _close_grad(grads[k], c["grads"][k], k + " " + tag)
    return c, out, last, grads


@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("N,T,din,d", SHAPES_A + SHAPES_B)
def test_sequence_op_matches_the_reference(N, T, din, d, reverse, with_h0):
    """out, h_last and all six gradients from a loss on both outputs"""
    from fvta_memexqa_amd import ops
    assert ops.gru_seq_plan(N, T, din, d)["regime"] == ("A" if (N, T, din, d) in SHAPES_A else "B")
    c, out, _, _ = _check_case(N, T, din, d, reverse, with_h0)
    pad = torch.arange(T)[None, :] >= c["lens"][:, None]
    assert out.detach().cpu()[pad].abs().sum().item() == 0          # padded rows are exactly zero


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("use", ["out", "last"])
def test_one_output_unused(use, reverse):
    """(17,2,37,100) with only `out`, and only `h_last`, in the loss: the other gradient goes down as NULL"""
    from fvta_memexqa_amd import ops
    seen = []
    orig = ops.GRUSeq.backward

    def spy(self, x, lens, Wg, Wc, d_out, d_h_last, *rest, **kw):
        seen.append((d_out is None, d_h_last is None))
        return orig(self, x, lens, Wg, Wc, d_out, d_h_last, *rest, **kw)

    ops.GRUSeq.backward = spy
    try:
        _check_case(17, 2, 37, 100, reverse, True, use=use)
    finally:
        ops.GRUSeq.backward = orig
    assert seen == [(use == "last", use == "out")]


@pytest.mark.parametrize("N,T,din,d,reverse", [(17, 2, 37, 100, False), (33, 9, 24, 80, True), (9, 5, 20, 136, True)])
def test_accumulate_onto_nonzero_buffers(N, T, din, d, reverse):
    """accumulate = 1 through ops.GRUSeq: the parameter gradients are added to random buffers, d_x / d_h0 (pre-filled with
    7.0) are overwritten"""
    from fvta_memexqa_amd import ops
    c = _case(N, T, din, d, reverse, True)
    cu = lambda t: t.cuda().contiguous()
    x, h0, P = cu(c["x"]), cu(c["h0"]), [cu(p) for p in c["P"]]
    lens = c["lens"].to(torch.int32).cuda()
    op = ops.GRUSeq(N, T, din, d, reverse=reverse, training=True)
    out, last = op.forward(x, lens, h0, *P)
    _close_out(out, c["out"], "out (ops)")
    _close_out(last, c["last"], "h_last (ops)")
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(p.shape, generator=g) for p in c["P"]]
    acc = [cu(b.clone()) for b in base]
    d_x, d_h0 = torch.full((N, T, din), 7.0, device="cuda"), torch.full((N, d), 7.0, device="cuda")
    op.backward(x, lens, P[0], P[2], cu(c["g_out"]), cu(c["g_last"]), d_x, d_h0, *acc, accumulate=True)
    _close_grad(d_x, c["grads"]["d_x"], "d_x (accumulate)")
    _close_grad(d_h0, c["grads"]["d_h0"], "d_h0 (accumulate)")
    for k, got, b in zip(GRADS[2:], acc, base):
        _close_grad(got, b.double() + c["grads"][k], k + " (accumulate)")


def test_row_tile_and_regime_edges():
    """N around the row tile the plan reports, and both sides of the regime edge it reports"""
    from fvta_memexqa_amd import ops
    RT = ops.gru_seq_plan(17, 3, 24, 80)["row_tile"]
    assert RT >= 1
    for N in (RT - 1, RT, RT + 1):
        if N >= 1:
            _check_case(N, 3, 24, 80, N % 2 == 0, True)
    edge = next((d for d in range(101, 514) if ops.gru_seq_plan(17, 3, 24, d)["regime"] == "B"), None)
    assert edge is not None, "no regime B up to d = 513"
    assert ops.gru_seq_plan(17, 3, 24, edge - 1)["regime"] == "A"
    for reverse in (False, True):
        _check_case(17, 3, 24, edge - 1, reverse, True)
        _check_case(17, 3, 24, edge, reverse, True)


@pytest.mark.parametrize("N,T,din,d", [(17, 2, 37, 100), (9, 5, 20, 136)])
@pytest.mark.parametrize("reverse", [False, True])
def test_lens_none_is_full_length(N, T, din, d, reverse):
    """lens = None equals lens = T bit for bit, and matches the reference"""
    from fvta_memexqa_amd import autograd
    c, out, last, grads = _check_case(N, T, din, d, reverse, True, full=True)
    leaf = lambda t: t.cuda().requires_grad_()
    x, h0, P = leaf(c["x"]), leaf(c["h0"]), [leaf(p) for p in c["P"]]
    out2, last2 = autograd.gru_seq(x, torch.full((N,), T), h0, *P, reverse=reverse)
    ((out2 * c["g_out"].cuda()).sum() + (last2 * c["g_last"].cuda()).sum()).backward()
    assert torch.equal(out, out2) and torch.equal(last, last2)
    for k, t in zip(GRADS, [x, h0] + P):
        assert torch.equal(grads[k], t.grad), k


@pytest.mark.parametrize("N,T,din,d,reverse", [(33, 9, 24, 80, False), (17, 2, 37, 100, True), (9, 5, 20, 136, True)])
def test_runs_are_bitwise_repeatable(N, T, din, d, reverse, monkeypatch):
    """two forward + backward runs agree bit for bit; a second backward over a retained graph equals the first; the
    no-grad forward gives the training forward's bits, with training = 0 and no `saved`"""
    from fvta_memexqa_amd import autograd, ops
    c = _case(N, T, din, d, reverse, True)
    o1, l1, g1 = _run_autograd(c)
    o2, l2, g2 = _run_autograd(c)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    for k in GRADS:
        assert torch.equal(g1[k], g2[k]), k
    leaves = [t.cuda().requires_grad_() for t in [c["x"], c["h0"]] + c["P"]]
    out, last = autograd.gru_seq(leaves[0], c["lens"], leaves[1], *leaves[2:], reverse=reverse)
    go = (c["g_out"].cuda(), c["g_last"].cuda())
    first = torch.autograd.grad((out, last), leaves, go, retain_graph=True)
    second = torch.autograd.grad((out, last), leaves, go, retain_graph=True)
    for k, a, b in zip(GRADS, first, second):
        assert torch.equal(a, b) and torch.equal(a, g1[k]), k
    made = []

    class Spy(ops.GRUSeq):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(ops, "GRUSeq", Spy)
    plain = autograd.gru_seq(c["x"].cuda(), c["lens"], c["h0"].cuda(), *[p.cuda() for p in c["P"]], reverse=reverse)
    assert plain[0].grad_fn is None and not plain[1].requires_grad
    assert torch.equal(plain[0], o1.detach()) and torch.equal(plain[1], l1.detach())
    assert len(made) == 1 and made[0].desc.training == 0 and made[0].saved is None
    with pytest.raises(Exception):
        made[0].backward(*([None] * 12))


def test_gru_encoder_module():
    """nn.GRUEncoder on [2,3,T,in] inputs with lens [2,3]: outputs, every gradient, the variable names and initial values"""
    from fvta_memexqa_amd import nn
    g = torch.Generator().manual_seed(31)
    T, din, d = 5, 12, 20
    x = torch.randn(2, 3, T, din, generator=g) * 0.5
    lens = torch.tensor([[5, 0, 1], [3, 5, 2]])
    g_out, g_last = torch.randn(2, 3, T, d, generator=g), torch.randn(2, 3, d, generator=g)
    mod = nn.GRUEncoder(din, d, seed=7)
    assert sorted(mod.state_dict()) == sorted("gru_cell/%s/%s" % (a, b) for a in ("gates", "candidate") for b in ("kernel", "bias"))
    sd = mod.state_dict()
    assert tuple(sd["gru_cell/gates/kernel"].shape) == (din + d, 2 * d) and tuple(sd["gru_cell/candidate/kernel"].shape) == (din + d, d)
    assert torch.equal(sd["gru_cell/gates/bias"].cpu(), torch.ones(2 * d)) and torch.equal(sd["gru_cell/candidate/bias"].cpu(), torch.zeros(d))
    with torch.no_grad():
        mod.p("gru_cell/gates/bias").add_((0.1 * torch.randn(2 * d, generator=g)).cuda())
        mod.p("gru_cell/candidate/bias").add_((0.1 * torch.randn(d, generator=g)).cuda())
    names = ["gru_cell/gates/kernel", "gru_cell/gates/bias", "gru_cell/candidate/kernel", "gru_cell/candidate/bias"]
    P64 = [mod.p(n).detach().cpu().double().requires_grad_() for n in names]
    x64 = x.double().requires_grad_()
    ro, rl = R.gru_seq(x64.reshape(6, T, din), lens.reshape(-1), None, *P64)
    ((ro * g_out.reshape(6, T, d).double()).sum() + (rl * g_last.reshape(6, d).double()).sum()).backward()
    xc = x.cuda().requires_grad_()
    out, last = mod(xc, lens)
    assert tuple(out.shape) == (2, 3, T, d) and tuple(last.shape) == (2, 3, d)
    ((out * g_out.cuda()).sum() + (last * g_last.cuda()).sum()).backward()
    _close_out(out.reshape(6, T, d), ro, "GRUEncoder out")
    _close_out(last.reshape(6, d), rl, "GRUEncoder last")
    _close_grad(xc.grad.reshape(6, T, din), x64.grad.reshape(6, T, din), "GRUEncoder d_x")
    for n, p64 in zip(names, P64):
        _close_grad(mod.p(n).grad, p64.grad, n)


def _randomise_biases(mod, g):
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("bias") or k.endswith("biases") or k.endswith("/b"):
                p.add_((0.1 * torch.randn(p.shape, generator=g)).cuda())


def _gru_vars(p64, prefix):
    return tuple(p64[prefix + n] for n in ("gru_cell/gates/kernel", "gru_cell/gates/bias", "gru_cell/candidate/kernel",
                                           "gru_cell/candidate/bias"))


def test_bigru_fusion_module():
    """nn.BiGRUFusion against the reference's two directions summed"""
    from fvta_memexqa_amd import nn
    g = torch.Generator().manual_seed(41)
    N, F, d = 7, 6, 24
    f_in = torch.randn(N, F, d, generator=g) * 0.5
    lens = torch.tensor([6, 0, 1, 4, 6, 2, 5])
    go = torch.randn(N, F, d, generator=g)
    mod = nn.BiGRUFusion(d, seed=3)
    assert sorted(mod.state_dict()) == sorted("%s/gru_cell/%s/%s" % (dr, a, b) for dr in ("fw", "bw") for a in ("gates", "candidate")
                                              for b in ("kernel", "bias"))
    assert not torch.equal(mod.p("fw/gru_cell/gates/kernel"), mod.p("bw/gru_cell/gates/kernel"))
    _randomise_biases(mod, g)
    p64 = {k: p.detach().cpu().double().requires_grad_() for k, p in mod.named_parameters()}
    f64 = f_in.double().requires_grad_()
    ref = R.bigru_sum(f64, lens, _gru_vars(p64, "fw/"), _gru_vars(p64, "bw/"))
    (ref * go.double()).sum().backward()
    fc = f_in.cuda().requires_grad_()
    out = mod(fc, lens)
    out.backward(go.cuda())
    _close_out(out, ref, "BiGRUFusion")
    _close_grad(fc.grad, f64.grad, "BiGRUFusion d_f_in")
    for k, p in mod.named_parameters():
        _close_grad(p.grad, p64[k].grad, k)


@pytest.mark.parametrize("N,F,d,hops", [(5, 6, 16, 2), (17, 9, 100, 3)])
def test_dmnplus_head(N, F, d, hops):
    """nn.DMNPlusHead: logits and every parameter / input gradient against the reference composed from tests/_gru_ref.py
    and oracle.fvta_fused.dmn_memory; three Adam steps lower a soft-label cross-entropy"""
    from fvta_memexqa_amd import nn
    from oracle import fvta_fused as O
    g = torch.Generator().manual_seed(51 + d)
    C = 4
    lq = torch.randn(N, d, generator=g) * 0.5
    lch = torch.randn(N, C, d, generator=g) * 0.5
    f_in = torch.randn(N, F, d, generator=g) * 0.5
    lens = torch.randint(1, F + 1, (N,), generator=g)
    lens[:3] = torch.tensor([F, 1, 2])
    go = torch.randn(N, C, generator=g)
    mod = nn.DMNPlusHead(d, hops, num_choice=C, seed=11)
    keys = sorted(mod.state_dict())
    assert len(keys) == 8 + 9 + 2 * hops + 2
    assert "input_facts/fw/gru_cell/gates/kernel" in keys and "memory/hop_0/dense/kernel" in keys and "output/choicelogits/W" in keys
    _randomise_biases(mod, g)
    p64 = {k: p.detach().cpu().double().requires_grad_() for k, p in mod.named_parameters()}
    lq64, lch64, f64 = (t.double().requires_grad_() for t in (lq, lch, f_in))

    def ref_logits():
        facts = R.bigru_sum(f64, lens, _gru_vars(p64, "input_facts/fw/"), _gru_vars(p64, "input_facts/bw/"))
        output = O.dmn_memory(lq64, facts, lens, p64, hops)
        cat = torch.cat([lq64[:, None, :].expand(-1, C, -1), output[:, None, :].expand(-1, C, -1), lch64], 2)
        return (cat @ p64["output/choicelogits/W"] + p64["output/choicelogits/b"])[..., 0]

    ref = ref_logits()
    (ref * go.double()).sum().backward()
    lq_c, lch_c, f_c = (t.cuda().requires_grad_() for t in (lq, lch, f_in))
    logits = mod(lq_c, lch_c, f_c, lens)
    assert tuple(logits.shape) == (N, C)
    (logits * go.cuda()).sum().backward()
    _close_out(logits, ref, "logits")
    _close_grad(lq_c.grad, lq64.grad, "d_lq")
    _close_grad(lch_c.grad, lch64.grad, "d_lchoices")
    _close_grad(f_c.grad, f64.grad, "d_f_in")
    for k, p in mod.named_parameters():
        _close_grad(p.grad, p64[k].grad, k)

    # ---- training: a soft-label cross-entropy goes down over three Adam steps
    y = torch.softmax(torch.randn(N, C, generator=g) * 2, 1).cuda()
    opt = torch.optim.Adam(mod.parameters(), lr=1e-2)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = -(y * torch.log_softmax(mod(lq.cuda(), lch.cuda(), f_in.cuda(), lens), 1)).sum(1).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[3] < losses[0], losses
