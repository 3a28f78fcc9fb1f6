"""The published FVTA configuration (--use_char, --use_image_trans, --use_time_warp --warp_type 5, simiMatrix 2,
--add_tanh, --use_question_att, time_warp_att) composed from fvta_memexqa_amd.nn / .functional alone, from token ids to
the loss: loss and every parameter gradient against the same graph written with the fp64 oracle's functions, three
torch.optim steps, and a twin loaded from state_dict()."""
import numpy as np
import pytest
import torch

from tests.test_gpu_autograd import ATOL, RTOL, _close

pytestmark = pytest.mark.gpu

N, M, HID, JQ, NCH, JC = 2, 2, 50, 4, 3, 3
JI, JXP = 2, 3
VW, G, VC, W, CDIM, CWDIM, WDIM = 7, 5, 11, 6, 8, 16, 12
P_IMG, IDIM, TDIM = 9, 24, 10
WARP_TYPE, WINDOW_T = 5, 1.4
ORDER = ("at", "ad", "when", "where", "pts", "pis")            # model_v2.py:910


def _mask(J, lens):
    return torch.arange(J, device=lens.device).expand(*lens.shape, J) < lens[..., None]


class _PublishedFVTA(torch.nn.Module):
    def __init__(self):
        from fvta_memexqa_amd import nn as fnn
        super().__init__()
        w = 2 * HID
        self.emb = fnn.TokenEmbedding(VW, WDIM, VC=VC, cdim=CDIM, cwdim=CWDIM, W=W, seed=1)
        self.photo = fnn.PhotoFeatures(IDIM, tdim=TDIM, add_tanh=True, seed=2)
        self.text = fnn.BiLSTMEncoder(CWDIM + WDIM, HID, seed=3)
        self.image = fnn.BiLSTMEncoder(TDIM, HID, seed=4)
        self.warp = fnn.TimeWarp(w, warp_type=WARP_TYPE, window_t=WINDOW_T, seed=5)
        self.att = fnn.FocalAttention3D(w, simiMatrix=2, add_tanh=True, seed=6)
        self.qatt = fnn.QuestionAttention(w, simiMatrix=2, add_tanh=True, seed=7)
        self.out = fnn.AnswerScorer(w, seed=8)

    def _encode(self, enc, x, lens):
        """x [..., J, in], lens [...] -> (h [..., J, 2 hidden], last [..., 2 hidden])"""
        lead, J = tuple(lens.shape), x.shape[-2]
        h, last = enc(x.reshape(-1, J, x.shape[-1]), lens.reshape(-1))
        return h.reshape(lead + (J, h.shape[-1])), last.reshape(lead + (last.shape[-1],))

    def forward(self, b):
        from fvta_memexqa_amd import functional as Fn
        E = b["existing_emb_mat"]
        text = lambda s: self._encode(self.text, self.emb(s["ids"], s["chars"], E), s["lens"])
        hq, lq = text(b["q"])
        _, lch = text(b["choices"])
        streams, masks = [], []
        for name in ORDER[:4]:
            streams.append(text(b[name])[0])                                         # [N,M,J,w]
            masks.append(_mask(b[name]["ids"].shape[-1], b[name]["lens"]))
        hpts = text(b["pts"])[0]                                                     # [N,M,JI,JXP,w]
        streams.append(hpts.reshape(N, M, JI * JXP, -1))                             # model_v2.py:886
        masks.append(_mask(JXP, b["pts"]["lens"]).reshape(N, M, JI * JXP))
        streams.append(self._encode(self.image, self.photo(b["pis"]["ids"], b["image_emb_mat"]), b["pis"]["lens"])[0])
        masks.append(_mask(JI, b["pis"]["lens"]))
        hall, hall_mask = Fn.context_tensor(streams, masks)                          # [N,6,M,6,w]
        warp_h, scale = self.warp(hall, lq)
        qmask = _mask(JQ, b["q"]["lens"])
        g1, _ = self.att(warp_h, hq, hall_mask, qmask, C=scale)
        gq, _ = self.qatt(hq, g1[:, None, :], qmask, torch.ones(N, 1, dtype=torch.bool, device=g1.device))
        return self.out(gq, g1, lch, b["y"])[0]


def _batch():
    g = torch.Generator().manual_seed(23)

    def text(lead, J, lens):
        return dict(ids=torch.randint(0, VW + G, lead + (J,), generator=g, dtype=torch.int32),
                    chars=torch.randint(0, VC, lead + (J, W), generator=g, dtype=torch.int32), lens=torch.tensor(lens))

    b = dict(at=text((N, M), 3, [[3, 1], [2, 3]]), ad=text((N, M), 4, [[4, 2], [1, 3]]), when=text((N, M), 2, [[2, 1], [1, 2]]),
             where=text((N, M), 2, [[1, 0], [2, 1]]),                                # one empty row
             pts=text((N, M, JI), JXP, [[[3, 1], [2, 0]], [[1, 3], [2, 2]]]),
             q=text((N,), JQ, [4, 2]), choices=text((N, NCH), JC, [[3, 1, 2], [2, 3, 1]]),
             pis=dict(ids=torch.randint(0, P_IMG, (N, M, JI), generator=g, dtype=torch.int32), lens=torch.tensor([[2, 1], [1, 2]])),
             existing_emb_mat=torch.randn(G, WDIM, generator=g), image_emb_mat=torch.randn(P_IMG, IDIM, generator=g))
    b["at"]["ids"][0, 0] = torch.tensor([0, VW - 1, VW + G - 1])                    # both tables, both ends
    y = torch.zeros(N, NCH, dtype=torch.bool)
    y[0, 1] = y[1, 2] = True
    b["y"] = y
    return b


def _to_cuda(b):
    return {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in b.items()}


def _oracle(sd, b):
    """_PublishedFVTA.forward with the oracle's functions in fp64"""
    from oracle import fvta_fused as F
    Pm = {k: v.detach().cpu().double().requires_grad_() for k, v in sd.items() if k != "warp.time_warp_C/time_warp_window_t"}
    E, img = b["existing_emb_mat"].double(), b["image_emb_mat"].double()
    tk, tb = Pm["text.fw/basic_lstm_cell/kernel"], Pm["text.fw/basic_lstm_cell/bias"]

    def text(s):
        x = F.embed_tokens(s["ids"], s["chars"], Pm["emb.word/var/word_emb_mat"], E, Pm["emb.var/char_emb"],
                           Pm["emb.conv/conv1d/filter"], Pm["emb.conv/conv1d/bias"])
        return F.encode_stream(x, _mask(s["ids"].shape[-1], s["lens"]), tk, tb)

    hq, lq = text(b["q"])
    _, lch = text(b["choices"])
    hs = [text(b[n])[0] for n in ORDER[:4]]
    ms = [_mask(b[n]["ids"].shape[-1], b[n]["lens"]) for n in ORDER[:4]]
    hs.append(text(b["pts"])[0].reshape(N, M, JI * JXP, -1))
    ms.append(_mask(JXP, b["pts"]["lens"]).reshape(N, M, JI * JXP))
    xi = F.image_features(b["pis"]["ids"], img, Pm["photo.image_transform/image_trans_linear/W"],
                          Pm["photo.image_transform/image_trans_linear/b"], add_tanh=True)
    hs.append(F.encode_stream(xi, _mask(JI, b["pis"]["lens"]), Pm["image.fw/basic_lstm_cell/kernel"],
                              Pm["image.fw/basic_lstm_cell/bias"])[0])
    ms.append(_mask(JI, b["pis"]["lens"]))
    hall, hall_mask = F.context_tensor(hs, ms)
    warp_h, c = F.time_warp_closed(hall, lq, Pm["warp.WH/W"], Pm["warp.WH/b"], Pm["warp.WC/W"], Pm["warp.WC/b"],
                                   warp_type=WARP_TYPE, window_t=WINDOW_T)
    C = c[:, :, None] * F.time_indication_band(c.shape[1], WARP_TYPE, WINDOW_T, torch.float64)[None]
    qmask = _mask(JQ, b["q"]["lens"])
    g1, _ = F.attention_3d(warp_h, hq, Pm["att.att_logits/W"], Pm["att.att_logits/b"], hall_mask, qmask, simiMatrix=2,
                           add_tanh=True, time_warp_att=True, C=C)
    gq, _ = F.attention(hq, g1[:, None, :], Pm["qatt.att_logits/W"], Pm["qatt.att_logits/b"], qmask,
                        torch.ones(N, 1, dtype=torch.bool), simiMatrix=2, add_tanh=True)
    logits, _ = F.scorer(gq, g1, lch, Pm["out.choicelogits/W"], Pm["out.choicelogits/b"])
    loss = F.softmax_cross_entropy_mean(logits, b["y"], tf_grad=True)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in Pm.items()}, (hall.detach(), c.detach())


def _tolerance(name):
    """(rtol, atol, atol scaled by max(1, |ref|max)): each parameter with its op-level test's"""
    if name.startswith("warp."):
        return 2e-4, 2e-5, True                                  # tests/test_gpu_timewarp.py
    if name.startswith("emb."):
        return 1e-4, 1e-4, False                                 # tests/test_gpu_embed.py
    return RTOL, ATOL, True                                      # tests/test_gpu_autograd.py


def test_published_model_from_ids_to_loss_trains():
    b = _batch()
    dev = _to_cuda(b)
    model = _PublishedFVTA()
    # The reference scales the max-pooled logits AFTER exp_mask (model_v2.py:269-275), so a padded position whose c[n,t] is
    # negative takes the whole softmax over t and hands on its zero row: with most of T padding, as here, one negative
    # c[n,:] would cut every parameter below the attention off from the loss (tests/test_gpu_timewarp.py covers those
    # rows at the kernel).  c = tanh(K (lq . WC/W + WC/b) + ...): a small WC/W and a positive WC/b keep it positive.
    with torch.no_grad():
        model.warp.p("WC/W").mul_(0.1)
        model.warp.p("WC/b").fill_(0.1)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    w = 2 * HID
    assert sd["warp.time_warp_C/time_warp_window_t"].shape == () and sd["warp.WH/W"].shape == (2 * w, w)
    assert sd["emb.conv/conv1d/filter"].shape == (1, 5, CDIM, CWDIM) and sd["att.att_logits/W"].shape == (2 * w, 1)
    ref_loss, ref_grads, (ref_hall, ref_c) = _oracle(sd, b)
    assert ref_hall.shape == (N, 6, M, 6, w) and ref_c.shape == (N, 12) and bool((ref_c > 0.1).all())
    loss = model(dev)
    print("\nloss %.7f (oracle %.7f)" % (float(loss.detach()), float(ref_loss)))
    _close(loss, ref_loss, rtol=RTOL, atol=ATOL, msg="loss")
    loss.backward()
    params = dict(model.named_parameters())
    assert set(params) == set(ref_grads)
    failures = []
    for k, p in params.items():
        assert p.grad is not None, k
        ref = ref_grads[k].numpy()
        got = p.grad.detach().cpu().double().numpy()
        rtol, atol, scaled = _tolerance(k)
        atol = atol * max(1.0, float(np.abs(ref).max())) if scaled else atol
        err = float(np.max(np.abs(got - ref) - rtol * np.abs(ref)))
        print("%-48s |ref|max %.3e  worst |err| - rtol |ref| %.3e  (atol %.1e)" % (k, np.abs(ref).max(), err, atol))
        # (the scorer's bias shifts every logit of a row alike: its gradient is zero by construction)
        assert float(np.abs(ref).max()) > 1e-9 or k == "out.choicelogits/b", "%s: the test does not reach it" % k
        if not err <= atol:
            failures.append(k)
    assert not failures, "gradients outside their tolerance: %s" % failures
    opt = torch.optim.Adadelta(model.parameters(), lr=0.5)
    first = float(loss.detach())
    for _ in range(3):
        opt.zero_grad()
        step_loss = model(dev)
        step_loss.backward()
        opt.step()
    with torch.no_grad():
        after = model(dev)
    assert after.grad_fn is None
    assert float(after) < first, "three Adadelta steps did not lower the loss: %.6f -> %.6f" % (first, float(after))
    twin = _PublishedFVTA()
    twin.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(twin(dev), after)
