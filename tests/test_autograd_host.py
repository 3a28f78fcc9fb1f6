"""Host-side checks of the autograd layer: what must hold without a GPU."""
import pytest
import torch


def test_nn_imports_and_refuses_to_run_without_a_gpu(monkeypatch):
    import fvta_memexqa_amd.nn as fnn
    from fvta_memexqa_amd._lib import FvtaError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for make in (lambda: fnn.BiLSTMEncoder(12, 50), lambda: fnn.FocalAttention3D(100), lambda: fnn.QuestionAttention(100),
                 lambda: fnn.AnswerScorer(100)):
        with pytest.raises(FvtaError, match="no CPU fallback"):
            make()


def test_padding_helpers_are_differentiable_and_match_the_models_layout():
    """nn.BiLSTMEncoder pads with model_v2.pad_lstm_kernel / pad_blocks: zero everywhere but the reference's entries, and the
    gradient of the padded tensor flows back to exactly those entries"""
    from fvta_memexqa_amd.model_v2 import pad_blocks, pad_lstm_kernel, padded_hidden
    din, dinp, d = 12, 16, 50
    dp = padded_hidden(d)
    assert dp == 64
    k = torch.randn(din + d, 4 * d, requires_grad=True)
    kp = pad_lstm_kernel(k, din, dinp, d, dp)
    assert kp.shape == (dinp + dp, 4 * dp) and int((kp != 0).sum()) == int((k != 0).sum())
    assert torch.equal(kp.detach()[:din, dp:dp + d], k.detach()[:din, d:2 * d])              # input rows of gate j
    assert torch.equal(kp.detach()[dinp:dinp + d, 3 * dp:3 * dp + d], k.detach()[din:, 3 * d:])  # hidden rows of gate o
    kp.sum().backward()
    assert torch.equal(k.grad, torch.ones_like(k))
    b = torch.randn(4 * d, requires_grad=True)
    bp = pad_blocks(b, 4, d, dp)
    assert bp.shape == (4 * dp,) and torch.equal(bp.detach().reshape(4, dp)[:, :d].reshape(-1), b.detach())
    (bp * 2).sum().backward()
    assert torch.equal(b.grad, torch.full_like(b, 2.0))


def test_oracle_has_no_exact_tie_in_the_gpu_tests_attention_cases():
    """tests/test_gpu_autograd.py compares the `h_a` gradient with the oracle's default (TensorFlow's tie splitting); the
    kernels send a tie to the first arg-max.  The two agree only without exact ties: every valid row of every case there
    must have a unique maximum over the question, and every (n,k) a unique maximum over its rows."""
    from oracle import fvta_fused as F
    from tests.test_gpu_autograd import ATT_CASES, att_case
    for name, spec in ATT_CASES.items():
        N, K, T, JQ, w, simi, tanh, masked, seed = spec
        h, q, W, b, hm, qm = att_case(*spec)
        dbl = lambda t: None if t is None else t.double()
        _, a = F.attention_3d(dbl(h), dbl(q), dbl(W), dbl(b), hm, qm, simiMatrix=simi, add_tanh=tanh)
        valid = hm if hm is not None else torch.ones(N, K, T, dtype=torch.bool)
        assert bool(valid.reshape(N * K, T).any(1).all()), "%s: an (n,k) without a valid row" % name
        amax = a.amax(-1, keepdim=True)
        assert int(((a == amax).sum(-1) > 1)[valid].sum()) == 0, "%s: a tie in the max over the question" % name
        top = torch.where(valid, amax[..., 0], torch.full_like(amax[..., 0], -float("inf")))
        assert int(((top == top.amax(-1, keepdim=True)).sum(-1) > 1).sum()) == 0, "%s: a tie in the max over the rows" % name
