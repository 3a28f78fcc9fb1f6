"""Thin `torch.nn.Module`s over the autograd layer (autograd.py): the pieces of the reference's graph a user composes
into a model of their own and trains with `torch.optim`.

Parameters are `nn.Parameter`s in the REFERENCE's shapes, named like the reference's variables below their scope
(`fw/basic_lstm_cell/kernel`, `att_logits/W`, `choicelogits/W`: the tails of `Model.N_*`) and initialised like them, so
`state_dict()` holds what a reference checkpoint holds.  Any hidden size is accepted: the forward zero pads to the sizes
the kernels run at with the padding `Model` uses (model_v2.padded_hidden, pad_lstm_kernel, pad_blocks -- exact, and the
gradient of a padded entry is dropped by the slicing's own backward).

There is no CPU path: constructing a module without a GPU raises FvtaError.
"""
import zlib

import torch

from . import autograd, functional, ops
from .model_v2 import pad_blocks, pad_lstm_kernel, padded_hidden
from .synth import _glorot, _trunc_normal

_DIRS = ("fw", "bw")


def _gen(name, seed):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) if seed is None else int(seed))


class _Module(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._dev = ops.require_gpu()

    def _param(self, name, value):
        self.register_parameter(name, torch.nn.Parameter(value.to(torch.float32).to(self._dev)))

    def p(self, name):
        return self._parameters[name]


class BiLSTMEncoder(_Module):
    """One bidirectional_dynamic_rnn over BasicLSTMCell (model_v2.py:652-661, 694-823): x [B,J,in_dim], lens [B] ->
    (out [B,J,2*hidden] = [fw | bw] with rows t >= len zeroed, last [B,2*hidden]).  Parameters
    `{fw,bw}/basic_lstm_cell/{kernel [in_dim+hidden, 4*hidden], bias [4*hidden]}` (Glorot uniform / zeros, as
    tf.get_variable's defaults); share_fw_bw: TF >= 1.2 cell reuse, only `fw/...` exists."""

    def __init__(self, in_dim, hidden, share_fw_bw=True, precision="f32", seed=None):
        super().__init__()
        self.in_dim, self.hidden, self.share_fw_bw, self.precision = int(in_dim), int(hidden), bool(share_fw_bw), precision
        self.in_p = (self.in_dim + 7) // 8 * 8
        self.dp = padded_hidden(self.hidden)
        for i, dr in enumerate(_DIRS[:1 if share_fw_bw else 2]):
            name = "%s/basic_lstm_cell/kernel" % dr
            self._param(name, _glorot(_gen(name, None if seed is None else seed + i), self.in_dim + self.hidden, 4 * self.hidden))
            self._param("%s/basic_lstm_cell/bias" % dr, torch.zeros(4 * self.hidden))

    def _padded(self, dr):
        k = pad_lstm_kernel(self.p("%s/basic_lstm_cell/kernel" % dr), self.in_dim, self.in_p, self.hidden, self.dp)
        return k, pad_blocks(self.p("%s/basic_lstm_cell/bias" % dr), 4, self.hidden, self.dp)

    def forward(self, x, lens):
        d, dp = self.hidden, self.dp
        x = torch.nn.functional.pad(x.to(torch.float32), (0, self.in_p - self.in_dim))
        kf, bf = self._padded("fw")
        kb, bb = (None, None) if self.share_fw_bw else self._padded("bw")
        out, last = autograd.bilstm(x, lens, kf, bf, kb, bb, precision=self.precision)
        if dp != d:
            out = torch.cat([out[..., :d], out[..., dp:dp + d]], -1)
            last = torch.cat([last[..., :d], last[..., dp:dp + d]], -1)
        return out, last


class _AttLogits(_Module):
    """the `att_logits` linear inside the attentions: W [F*w, 1] truncated normal(0.1), b [1] zeros (model_v2.py:88)"""

    def __init__(self, w, simiMatrix, add_tanh, seed):
        super().__init__()
        if simiMatrix not in (1, 2, 3, 4):
            raise ValueError("similarity matrix not implemented")
        self.w, self.simiMatrix, self.add_tanh = int(w), int(simiMatrix), bool(add_tanh)
        F = {1: 3, 2: 2, 3: 4, 4: 0}[self.simiMatrix]
        if F:
            self._param("att_logits/W", _trunc_normal(_gen("att_logits/W", seed), (F * self.w, 1)))
            self._param("att_logits/b", torch.zeros(1))

    def _wb(self):
        if self.simiMatrix == 4:
            return None, None
        return self.p("att_logits/W"), self.p("att_logits/b")


class FocalAttention3D(_AttLogits):
    """attention_3d (model_v2.py:210-298): hinfo [N,K,...,w], hq [N,JQ,w], masks -> (h_a [N,w], a_logits [N,K,T,JQ]), both
    differentiable.  With C [N,T,T] the max-pooled logits are scaled by its row sums (time_warp_att)."""

    def __init__(self, w, simiMatrix=1, add_tanh=False, seed=None):
        super().__init__(w, simiMatrix, add_tanh, seed)

    def forward(self, hinfo, hq, hinfo_mask=None, hq_mask=None, C=None):
        N, K = hinfo.shape[0], hinfo.shape[1]
        tscale = None
        if C is not None:
            T = C.shape[-1]
            ones = torch.ones(T, 1, dtype=torch.float32, device=C.device)
            tscale = functional.linear_raw(C.to(torch.float32).reshape(N * T, T), ones, None).reshape(N, T)
        W, b = self._wb()
        return functional.attention_raw(hinfo.reshape(N, K, -1, self.w), hq, W, b, hinfo_mask, hq_mask, self.simiMatrix,
                                        self.add_tanh, 0, tscale)


class QuestionAttention(_AttLogits):
    """attention (model_v2.py:125-201), the K = 1 form `question_emb/question_att` uses: hinfo [N,...,w] flattened to
    [N,V,w] -> (h_a [N,w], a_logits [N,V,JQ]); with bidirect h_a is [N,2w] = concat([h_a, q_a])."""

    def __init__(self, w, simiMatrix=1, add_tanh=False, bidirect=False, seed=None):
        super().__init__(w, simiMatrix, add_tanh, seed)
        self.bidirect = bool(bidirect)

    def forward(self, hinfo, hq, hinfo_mask=None, hq_mask=None):
        N = hinfo.shape[0]
        h = hinfo.reshape(N, 1, -1, self.w)
        hm = hinfo_mask.reshape(N, 1, -1) if hinfo_mask is not None else None
        W, b = self._wb()
        h_a, a = functional.attention_raw(h, hq, W, b, hm, hq_mask, self.simiMatrix, self.add_tanh, 0)
        a = a.reshape(N, h.shape[2], hq.shape[1])
        if self.bidirect:
            h_a = torch.cat([h_a, functional.bidirect_q_a(a, hq)], 1)
        return h_a, a


class ChoicesAttention(_AttLogits):
    """attention_keeprank1 (model.py:247-314), what `use_choices_att` runs (:966-968): hinfo [N,M,...,w], hq [N,JQ,w] ->
    h_a [N,M,w], every (n,m) attended on its own; with bidirect [N,M,2w] = concat([h_a, q_a]).  model.py's feature order
    ([(h-q)^2, h*q] under simiMatrix 2), simiMatrix 1-3, no tanh on the logits.  Training needs N * M <= 65535; the
    backward's workspace is sized in functional.attention_keeprank1_raw's docstring."""

    def __init__(self, w, simiMatrix=1, bidirect=False, seed=None):
        if simiMatrix not in (1, 2, 3):
            raise ValueError("similarity matrix not implemented")          # model.py:283-285
        super().__init__(w, simiMatrix, False, seed)
        self.bidirect = bool(bidirect)

    def forward(self, hinfo, hq, hinfo_mask=None, hq_mask=None):
        W, b = self._wb()
        return functional.attention_keeprank1_raw(hinfo, hq, W, b, hinfo_mask, hq_mask, self.simiMatrix, self.bidirect)


class AnswerScorer(_Module):
    """model_v2.py:1053-1096: gq, g1 [N,w], gch [N,C,w], y [N,C] -> (loss, logits [N,C], yp [N,C]); `choicelogits/W`
    [5w, 1] (7w with use_eu_output) truncated normal(0.1), `choicelogits/b` [1] zeros.  Only the loss is differentiable."""

    def __init__(self, w, use_eu_output=False, add_tanh=False, tf_xent_grad=True, seed=None):
        super().__init__()
        self.w, self.use_eu_output, self.add_tanh, self.tf_xent_grad = int(w), bool(use_eu_output), bool(add_tanh), bool(tf_xent_grad)
        self._param("choicelogits/W", _trunc_normal(_gen("choicelogits/W", seed), ((7 if use_eu_output else 5) * self.w, 1)))
        self._param("choicelogits/b", torch.zeros(1))

    def forward(self, gq, g1, gch, y):
        return autograd.scorer_ce(gq, g1, gch, self.p("choicelogits/W"), self.p("choicelogits/b"), y,
                                  use_eu_output=self.use_eu_output, add_tanh=self.add_tanh, tf_xent_grad=self.tf_xent_grad)
