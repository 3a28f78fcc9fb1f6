"""The front-end under autograd: nn.TokenEmbedding (model_v2.py:524-620) and nn.PhotoFeatures (:634-645) against the
oracle's embed_tokens / image_features, with the tolerances tests/test_gpu_embed.py applies to the same kernels."""
import pytest
import torch

from tests.test_gpu_embed import RTOL, _close

pytestmark = pytest.mark.gpu

VW, G, VC, W, HEIGHT, CDIM, CWDIM, WDIM = 7, 5, 11, 6, 5, 8, 16, 12
# 0, VW - 1 (the last trainable row), VW (the first frozen row), VW + G - 1 (the last one), and repeats: rows 0 and 6 are
# each read twice, so their gradient is a sum
IDS = torch.tensor([[0, VW - 1, VW], [VW + G - 1, VW - 1, 0]], dtype=torch.int32)


def _load(mod, values):
    with torch.no_grad():
        for k, v in values.items():
            mod.p(k).copy_(v.cuda())


def test_token_embedding_with_char_cnn():
    from fvta_memexqa_amd import nn as fnn
    from oracle import fvta_fused as F
    g = torch.Generator().manual_seed(1)
    vals = {"word/var/word_emb_mat": torch.randn(VW, WDIM, generator=g), "var/char_emb": torch.randn(VC, CDIM, generator=g),
            "conv/conv1d/filter": torch.randn(1, HEIGHT, CDIM, CWDIM, generator=g) * 0.3,
            "conv/conv1d/bias": torch.randn(CWDIM, generator=g) * 0.2}
    fixed = torch.randn(G, WDIM, generator=g)
    chars = torch.randint(0, VC, (2, 3, W), generator=g, dtype=torch.int32)
    chars[1, 1] = chars[0, 1]                                             # the same word twice: the same char rows twice
    gout = torch.randn(2, 3, CWDIM + WDIM, generator=g)
    mod = fnn.TokenEmbedding(VW, WDIM, VC=VC, cdim=CDIM, cwdim=CWDIM, W=W, height=HEIGHT, seed=2)
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == {k: tuple(v.shape) for k, v in vals.items()}
    _load(mod, vals)
    p64 = {k: v.double().requires_grad_() for k, v in vals.items()}
    ref = F.embed_tokens(IDS, chars, p64["word/var/word_emb_mat"], fixed.double(), p64["var/char_emb"],
                         p64["conv/conv1d/filter"], p64["conv/conv1d/bias"])
    (ref * gout.double()).sum().backward()
    existing = fixed.cuda().requires_grad_()
    x = mod(IDS.cuda(), chars.cuda(), existing)
    assert x.shape == (2, 3, CWDIM + WDIM)
    _close(x, ref, msg="x = [char part | word part]")
    x.backward(gout.cuda())
    for k in vals:
        _close(mod.p(k).grad, p64[k].grad, atol=1e-4, msg="d " + k)
    assert float(p64["word/var/word_emb_mat"].grad[VW - 1].abs().max()) > 0
    assert existing.grad is None                                          # the pre-trained table is frozen (model_v2.py:590)
    # no grad: no graph, the same rows; and a second call with other ids before one backward keeps its own argpos
    with torch.no_grad():
        again = mod(IDS.cuda(), chars.cuda(), fixed.cuda())
    assert again.grad_fn is None and torch.equal(again, x.detach())
    mod.zero_grad()
    x1 = mod(IDS.cuda(), chars.cuda(), fixed.cuda())
    x2 = mod(IDS.flip(0).cuda(), chars.flip(0).cuda(), fixed.cuda())
    torch.autograd.backward([x1, x2], [gout.cuda(), gout.flip(0).cuda()])
    for k in vals:
        _close(mod.p(k).grad, 2 * p64[k].grad, atol=2e-4, msg="two calls, d " + k)


def test_token_embedding_words_only():
    from fvta_memexqa_amd import nn as fnn
    from oracle import fvta_fused as F
    g = torch.Generator().manual_seed(3)
    table, fixed = torch.randn(VW, WDIM, generator=g), torch.randn(G, WDIM, generator=g)
    gout = torch.randn(2, 3, WDIM, generator=g)
    mod = fnn.TokenEmbedding(VW, WDIM)
    assert list(mod.state_dict()) == ["word/var/word_emb_mat"]
    _load(mod, {"word/var/word_emb_mat": table})
    t64 = table.double().requires_grad_()
    ref = F.embed_tokens(IDS, None, t64, fixed.double(), None, None, None)
    (ref * gout.double()).sum().backward()
    existing = fixed.cuda().requires_grad_()
    x = mod(IDS.cuda(), None, existing)
    assert x.shape == (2, 3, WDIM)
    _close(x, ref, msg="x")
    x.backward(gout.cuda())
    _close(mod.p("word/var/word_emb_mat").grad, t64.grad, atol=1e-4, msg="d word_emb_mat")
    assert existing.grad is None


def test_token_embedding_limits_surface_as_the_library_error():
    from fvta_memexqa_amd import _lib
    from fvta_memexqa_amd import nn as fnn
    mod = fnn.TokenEmbedding(VW, WDIM, VC=VC, cdim=CDIM, cwdim=CWDIM, W=3, height=HEIGHT)          # W < height
    with pytest.raises(_lib.FvtaError, match="unsupported char-CNN shape"):
        mod(IDS.cuda(), torch.zeros(2, 3, 3, dtype=torch.int32, device="cuda"), torch.zeros(G, WDIM, device="cuda"))


def test_photo_features():
    from fvta_memexqa_amd import nn as fnn
    from oracle import fvta_fused as F
    P, idim, tdim = 9, 24, 10
    g = torch.Generator().manual_seed(4)
    pis = torch.randint(0, P, (2, 2, 3), generator=g, dtype=torch.int32)
    pis[0, 0, 0], pis[1, 1, 2] = 0, P - 1
    pis[1, 0] = pis[0, 1]                                                 # repeats
    mat = torch.randn(P, idim, generator=g)
    Wt, bt = torch.randn(idim, tdim, generator=g) * 0.2, torch.randn(tdim, generator=g) * 0.1
    gout = torch.randn(2, 2, 3, tdim, generator=g)
    mod = fnn.PhotoFeatures(idim, tdim=tdim, add_tanh=True, seed=5)
    names = ("image_transform/image_trans_linear/W", "image_transform/image_trans_linear/b")
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == {names[0]: (idim, tdim), names[1]: (tdim,)}
    _load(mod, dict(zip(names, (Wt, bt))))
    W64, b64 = Wt.double().requires_grad_(), bt.double().requires_grad_()
    ref = F.image_features(pis, mat.double(), W64, b64, add_tanh=True)
    (ref * gout.double()).sum().backward()
    feats = mat.cuda().requires_grad_()
    x = mod(pis.cuda(), feats)
    assert x.shape == (2, 2, 3, tdim)
    _close(x, ref, msg="x")
    x.backward(gout.cuda())
    _close(mod.p(names[0]).grad, W64.grad, atol=1e-4, msg="dW")
    _close(mod.p(names[1]).grad, b64.grad, atol=1e-4, msg="db")
    assert feats.grad is None                                             # a placeholder in the reference
    # without the transform: the gather itself, no parameters
    plain = fnn.PhotoFeatures(idim)
    assert list(plain.parameters()) == [] and len(plain.state_dict()) == 0
    got = plain(pis.cuda(), mat.cuda())
    assert got.grad_fn is None and torch.equal(got.cpu(), mat[pis.long()])
    with pytest.raises(ValueError):
        plain(pis.cuda(), torch.zeros(P, idim + 1, device="cuda"))
