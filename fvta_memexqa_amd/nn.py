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
    differentiable.  With C [N,T,T] the max-pooled logits are scaled by its row sums (time_warp_att); C [N,T] is taken as
    those row sums already (TimeWarp's `scale`)."""

    def __init__(self, w, simiMatrix=1, add_tanh=False, seed=None):
        super().__init__(w, simiMatrix, add_tanh, seed)

    def forward(self, hinfo, hq, hinfo_mask=None, hq_mask=None, C=None):
        N, K = hinfo.shape[0], hinfo.shape[1]
        tscale = functional._tscale_of(C, N) if C is not None else None
        W, b = self._wb()
        return functional.attention_raw(hinfo.reshape(N, K, -1, self.w), hq, W, b, hinfo_mask, hq_mask, self.simiMatrix,
                                        self.add_tanh, 0, tscale)

    def forward_shared(self, hinfo, hq, album, hinfo_mask=None, hq_mask=None, differentiable=False, time_warp=None, lq=None,
                       energy=None):
        """forward() for NQ questions over A albums held once: hinfo [A,K,...,w], hq [NQ,JQ,w], album [NQ] in [0, A) ->
        (h_a [NQ,w], a_logits [NQ,K,T,JQ]) with this module's att_logits/{W,b} (functional.attention_3d_shared_raw).
        differentiable=False is the inference call: under gradient mode the parameters require grad and the call raises;
        use it under torch.no_grad().  differentiable=True trains over the shared rows (simiMatrix 1-3; 4 raises
        NotImplementedError): h_a's gradient reaches hinfo [A,K,...,w], hq and the parameters, a_logits carries none.
        time_warp (an nn.TimeWarp) with lq [NQ,w], the questions' last states: the attention over the rows warped per
        question -- forward(time_warp(hinfo[album], lq)[0], ...) -- with the rows still held once
        (functional.attention_3d_shared_warped_raw; inference only here -- forward_shared_warped() is the training call).
        Its parameters and its window buffer are used; energy [A,T]: functional.album_energy of (hinfo, WH/W, WC/W) when
        the caller keeps it, else computed here."""
        return self._album_forward(
            "forward_shared", False, differentiable, hinfo, hq, album, hinfo_mask, hq_mask, time_warp, lq, energy,
            "forward_shared: under the time warp this call is the inference one; "
            "forward_shared_warped(hinfo, hq, album, lq, time_warp, ...) trains over the shared rows")

    def forward_shared_warped(self, hinfo, hq, album, lq, time_warp, hinfo_mask=None, hq_mask=None, energy=None):
        """The training call under the time warp: forward(time_warp(hinfo[album], lq)[0], hq, ...) for NQ questions over A
        albums held once -> (h_a [NQ,w], a_logits [NQ,K,T,JQ]); no [NQ,K,T,w] tensor in either direction
        (functional.attention_3d_shared_warped_raw(differentiable=True); simiMatrix 1-3, 4 raises NotImplementedError).
        h_a's gradient reaches hinfo [A,K,...,w] (summed over each album's questions), hq, lq, this module's att_logits/{W,b}
        and time_warp's WH/{W,b}, WC/{W,b}; a_logits carries none.  energy [A,T]: a cached functional.album_energy, used
        for the forward; the gradient through it is taken all the same."""
        return self._album_forward("forward_shared_warped", False, True, hinfo, hq, album, hinfo_mask, hq_mask, time_warp, lq,
                                   energy)

    def forward_pooled(self, pool, hq, albums, pool_mask=None, hq_mask=None, time_warp=None, lq=None, energy=None,
                       differentiable=False):
        """forward() for NQ questions that each list M albums of one pool: pool [P,K,JX,w], hq [NQ,JQ,w], albums [NQ,M]
        (entries in [0, P), -1 an empty slot -- which needs both masks) -> (h_a [NQ,w], a_logits [NQ,K,M*JX,JQ]) with this
        module's att_logits/{W,b} (functional.attention_3d_pooled_raw): forward() on each question's albums laid end to
        end, with no such tensor built.  differentiable=False is the inference call: under gradient mode the parameters
        require grad and the call raises; use it under torch.no_grad().  differentiable=True trains over the pool
        (simiMatrix 1-3; 4 raises NotImplementedError): h_a's gradient reaches pool [P,K,JX,w] -- summed over every
        (question, slot) that names the album -- hq and the parameters, a_logits carries none.  Under the time warp this
        call is the inference one: with time_warp and differentiable=True it raises NotImplementedError (the per-question
        route is not needed: forward_pooled_warped() trains over the pool).
        time_warp (an nn.TimeWarp) with lq [NQ,w], the questions' last states: the attention over each question's albums
        laid end to end and warped for that question -- forward(time_warp(hinfo_i, lq)[0], ...) -- with the pool still
        held once (functional.attention_3d_pooled_warped_raw).  Its parameters and its window buffer are used; energy
        [P,JX]: functional.album_energy of (pool, WH/W, WC/W) when the caller keeps it, else computed here.
        A pool held in torch.bfloat16 passes through the inference calls as it is: no fp32 copy, and the result is that of
        the same call on pool.float(), bit for bit; differentiable=True widens it."""
        refusal = ("forward_pooled: under the time warp this call is the inference one; "
                   "forward_pooled_warped(pool, hq, albums, lq, time_warp, ...) trains over the pool (as "
                   "does the per-question route: forward() on time_warp's warp of each question's "
                   "gathered rows)")
        if time_warp is not None and differentiable:          # (this call refuses it before it looks at lq)
            raise NotImplementedError(refusal)
        return self._album_forward("forward_pooled", True, differentiable, pool, hq, albums, pool_mask, hq_mask, time_warp, lq,
                                   energy, refusal)

    def forward_pooled_warped(self, pool, hq, albums, lq, time_warp, pool_mask=None, hq_mask=None, energy=None):
        """The training call over the pool under the time warp: forward(time_warp(hinfo_i, lq)[0], hq, ...) for NQ questions
        that each list M albums of one pool, hinfo_i the question's albums laid end to end -> (h_a [NQ,w], a_logits
        [NQ,K,M*JX,JQ]); no [NQ,K,M*JX,w] tensor in either direction
        (functional.attention_3d_pooled_warped_raw(differentiable=True); simiMatrix 1-3, 4 raises NotImplementedError).
        h_a's gradient reaches pool [P,K,JX,w] (summed over every (question, slot) that names the album), hq, lq, this
        module's att_logits/{W,b} and time_warp's WH/{W,b}, WC/{W,b}; a_logits carries none.  energy [P,JX]: a cached
        functional.album_energy, used for the forward; the gradient through it is taken all the same."""
        return self._album_forward("forward_pooled_warped", True, True, pool, hq, albums, pool_mask, hq_mask, time_warp, lq,
                                   energy)

    def _album_forward(self, name, pooled, differentiable, rows, hq, index, rows_mask, hq_mask, time_warp, lq, energy,
                       inference=None):
        """What forward_shared / forward_pooled (pooled: a pool with album lists) and their _warped training calls share,
        each under its own `name`: the refusals, the time warp's parameters unpacked, the functional call.  inference:
        on the calls that are the inference ones under the time warp, the NotImplementedError they answer differentiable
        with there; None on the training calls, which take lq and time_warp by position."""
        W, b = self._wb()
        if time_warp is None:
            if lq is not None or energy is not None:
                raise ValueError("%s: lq / energy belong to the time warp; pass time_warp (an nn.TimeWarp) with them" % name)
            raw = functional.attention_3d_pooled_raw if pooled else functional.attention_3d_shared_raw
            return raw(rows, hq, index, W, b, rows_mask, hq_mask, self.simiMatrix, self.add_tanh, differentiable=differentiable)
        if inference is not None and lq is None:
            raise ValueError("%s: the time warp needs lq [NQ,w], the questions' last states" % name)
        if not torch.is_tensor(lq) or tuple(lq.shape) != (hq.shape[0], self.w):
            raise ValueError("%s: lq must be [%d, %d], got %s"
                             % (name, hq.shape[0], self.w, tuple(lq.shape) if torch.is_tensor(lq) else type(lq).__name__))
        if inference is not None and differentiable:
            raise NotImplementedError(inference)
        tw = time_warp
        raw = functional.attention_3d_pooled_warped_raw if pooled else functional.attention_3d_shared_warped_raw
        h_a, a, _ = raw(rows, hq, index, lq, W, b, tw.p("WH/W"), tw.p("WH/b"), tw.p("WC/W"), tw.p("WC/b"), rows_mask, hq_mask,
                        self.simiMatrix, self.add_tanh, tw.warp_type, tw.window_t(), energy, differentiable=differentiable)
        return h_a, a


class _EnergyCache:
    """The rows' share of the time warp, functional.album_energy(rows, WH/W, WC/W), kept by whoever holds the rows
    (AlbumMemory, AlbumPool): recomputed when either parameter is another tensor or has been written to since (its version
    counter)"""

    def __init__(self):
        self._kept = None                # (key of the time warp's weights, the energy)

    def get(self, rows, time_warp):
        WH, WC = time_warp.p("WH/W"), time_warp.p("WC/W")
        key = tuple((id(t), t.data_ptr(), t._version) for t in (WH, WC))
        if self._kept is None or self._kept[0] != key:
            self._kept = (key, functional.album_energy(rows, WH, WC))
        return self._kept[1]


class _AlbumRows:
    """What nn.AlbumMemory and nn.AlbumPool share: rows held once (`_held`), asked with an index per question (an album,
    or -- `_pooled` -- a list of albums), and the rows' energy under a time warp's weights, kept."""
    _pooled = False

    def __init__(self):
        self._energy = _EnergyCache()    # e [A,T] / [P,JX] under a time warp's weights: see energy()

    def _attend(self, attention, hq, hq_mask, index, time_warp, lq):
        rows, mask = self._held()
        if self._pooled:
            idx = ops.check_album_lists(index, len(self), mask is not None and hq_mask is not None)
        else:
            idx = ops.check_album_index(index, len(self))
        if idx.shape[0] != hq.shape[0]:
            raise ValueError(("album lists: %d lists for %d questions" if self._pooled else
                              "album index: %d entries for %d questions") % (idx.shape[0], hq.shape[0]))
        forward = attention.forward_pooled if self._pooled else attention.forward_shared
        if time_warp is None:
            if lq is not None:
                raise ValueError("attend: lq belongs to the time warp; pass time_warp (an nn.TimeWarp) with it")
            return forward(rows, hq, idx, mask, hq_mask)
        if lq is None:
            raise ValueError("attend: the time warp needs lq [NQ,w], the questions' last states")
        if not torch.is_tensor(lq) or tuple(lq.shape) != (hq.shape[0], rows.shape[-1]):
            raise ValueError("attend: lq must be [%d, %d], got %s"
                             % (hq.shape[0], rows.shape[-1], tuple(lq.shape) if torch.is_tensor(lq) else type(lq).__name__))
        return forward(rows, hq, idx, mask, hq_mask, time_warp=time_warp, lq=lq, energy=self.energy(time_warp))

    def energy(self, time_warp):
        """e [A,T] (a pool's: [P,JX]) of functional.album_energy for the held rows and time_warp's WH/W, WC/W: kept, and
        recomputed when either parameter is another tensor or has been written to since (its version counter)"""
        return self._energy.get(self._held()[0], time_warp)


class AlbumPool(_AlbumRows):
    """P encoded albums, each kept ONCE for any number of questions and any album lists: pool [P,K,JX,w] and pool_mask
    [P,K,JX], held contiguous fp32 (dtype=torch.float32, the default) or bf16 (dtype=torch.bfloat16) / u8 on the device
    and detached.  In bf16 the rows take half the bytes (`nbytes`) and every read of a row moves half the bytes; attend()
    and energy() return what an fp32 AlbumPool of the same (rounded) rows returns, bit for bit -- the kernels widen in
    registers and compute in fp32.  The rounding (to nearest even, once, here) is the only loss, and there is none when
    the rows came from the bf16 engine (the project's default, whose context rows are bf16: DESIGN.md 3, shadow rows):
    those values are bf16 already.  Where nn.AlbumMemory keeps one context per distinct
    LIST of albums, this keeps one block of rows per ALBUM and every question names the albums it reads (MemexQA's
    album_ids).  No parameters, no encoder.  It stays a detached inference holder: no gradient reaches the rows it was
    built from.  Training over a pool goes through nn.FocalAttention3D.forward_pooled(differentiable=True) -- under the time
    warp forward_pooled_warped() -- on a pool tensor that requires grad."""
    _pooled = True

    def __init__(self, pool, pool_mask=None, dtype=torch.float32):
        super().__init__()
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("AlbumPool: dtype must be torch.float32 or torch.bfloat16, got %s" % (dtype,))
        dev = ops.require_gpu()
        if pool.dim() != 4:
            raise ValueError("AlbumPool: expected [P,K,JX,w], got shape %s" % (tuple(pool.shape),))
        self.pool = pool.detach().to(dev, dtype).contiguous()
        self.pool_mask = None if pool_mask is None else ops.as_mask_u8(pool_mask.detach().to(dev))
        if self.pool_mask is not None and tuple(self.pool_mask.shape) != tuple(self.pool.shape[:3]):
            raise ValueError("AlbumPool: mask %s does not match the rows %s" % (tuple(pool_mask.shape), tuple(pool.shape)))

    def __len__(self):
        return self.pool.shape[0]

    def _held(self):
        return self.pool, self.pool_mask

    @property
    def nbytes(self):
        """the bytes the rows take on the device (the mask is P*K*JX more)"""
        return self.pool.numel() * self.pool.element_size()

    @classmethod
    def from_context(cls, hall, hall_mask=None, dtype=torch.float32):
        """The context tensor functional.context_tensor produces, hall [N,K,M,JX,w] / hall_mask [N,K,M,JX], cut into its
        albums: (pool of P = N*M albums, albums [N,M] = arange(N*M): question n's own M albums in order).  dtype: as the
        constructor's."""
        if hall.dim() != 5:
            raise ValueError("AlbumPool.from_context: expected [N,K,M,JX,w], got shape %s" % (tuple(hall.shape),))
        N, K, M, JX, w = hall.shape
        pool = hall.detach().permute(0, 2, 1, 3, 4).reshape(N * M, K, JX, w)
        mask = None if hall_mask is None else hall_mask.detach().reshape(N, K, M, JX).permute(0, 2, 1, 3).reshape(N * M, K, JX)
        return cls(pool, mask, dtype), torch.arange(N * M, dtype=torch.int32).reshape(N, M)

    def attend(self, attention, hq, hq_mask, albums, time_warp=None, lq=None):
        """(h_a [NQ,w], a_logits [NQ,K,M*JX,JQ]) of `attention` (an nn.FocalAttention3D) for questions hq [NQ,JQ,w] that list
        albums [NQ,M] of this pool; a bad list raises ValueError before anything reaches the library.
        time_warp (an nn.TimeWarp) with lq [NQ,w]: the attention over each question's albums laid end to end and warped
        for that question, the pool still held once.  The albums' share of the warp, the energy [P,JX], is computed on
        first use and kept; it is recomputed when WH/W or WC/W of the time warp have changed since (an in-place update,
        load_state_dict, another module)."""
        return self._attend(attention, hq, hq_mask, albums, time_warp, lq)


class AlbumMemory(_AlbumRows):
    """The context of A encoded albums, kept for any number of questions: hall [A,K,T,w] (or [A,K,M,JX,w]) and hall_mask
    [A,K,T] as functional.context_tensor returns them, held contiguous fp32 / u8 on the device and detached.  No
    parameters, no encoder: the caller encodes each album once and asks with attend()."""

    def __init__(self, hall, hall_mask=None):
        super().__init__()
        dev = ops.require_gpu()
        A, K, w = hall.shape[0], hall.shape[1], hall.shape[-1]
        self.hall = hall.detach().to(dev, torch.float32).reshape(A, K, -1, w).contiguous()
        self.hall_mask = None if hall_mask is None else ops.as_mask_u8(hall_mask.detach().to(dev).reshape(A, K, -1))
        if self.hall_mask is not None and tuple(self.hall_mask.shape) != tuple(self.hall.shape[:3]):
            raise ValueError("AlbumMemory: mask %s does not match the rows %s" % (tuple(hall_mask.shape), tuple(hall.shape)))

    def __len__(self):
        return self.hall.shape[0]

    def _held(self):
        return self.hall, self.hall_mask

    def attend(self, attention, hq, hq_mask, album, time_warp=None, lq=None):
        """(h_a [NQ,w], a_logits [NQ,K,T,JQ]) of `attention` (an nn.FocalAttention3D) for questions hq [NQ,JQ,w] about
        albums album [NQ]; a bad index raises ValueError before anything reaches the library.
        time_warp (an nn.TimeWarp) with lq [NQ,w]: the attention over the rows warped per question, the rows still held
        once.  The albums' share of the warp, the energy [A,T], is computed on first use and kept; it is recomputed when
        WH/W or WC/W of the time warp have changed since (an in-place update, load_state_dict, another module)."""
        return self._attend(attention, hq, hq_mask, album, time_warp, lq)


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


class TimeWarp(_Module):
    """The time warp of the context tensor (model_v2.py:953-1009): forward(hall [N,K,M,JX,w] or [N,K,T,w], lq [N,w]) ->
    (warp_h in hall's shape, scale [N,T]); `scale` feeds FocalAttention3D(..., C=scale).  Parameters `WH/W` [2w,w], `WC/W`
    [w,1] truncated normal(0.1), `WH/b` [w], `WC/b` [1] zeros; the buffer `time_warp_C/time_warp_window_t` (a 0-d tensor,
    the reference's variable of that name) is in state_dict() and never receives a gradient (tf.ceil, :335)."""

    def __init__(self, w, warp_type=1, window_t=3.0, seed=None):
        super().__init__()
        functional._check_warp_type(warp_type)
        self.w, self.warp_type = int(w), int(warp_type)
        shapes = (("WH/W", (2 * self.w, self.w)), ("WH/b", (self.w,)), ("WC/W", (self.w, 1)), ("WC/b", (1,)))
        for i, (name, shape) in enumerate(shapes):
            if name.endswith("/b"):
                self._param(name, torch.zeros(shape))
            else:
                self._param(name, _trunc_normal(_gen(name, None if seed is None else seed + i), shape))
        self.register_buffer("time_warp_C/time_warp_window_t", torch.tensor(float(window_t), dtype=torch.float32, device=self._dev))
        self._win = None

    def window_t(self):
        """the window as a host number, read back from the buffer only after it changed (load_state_dict)"""
        buf = self._buffers["time_warp_C/time_warp_window_t"]
        if self._win is None or self._win[0] != (buf._version, buf.data_ptr()):
            self._win = ((buf._version, buf.data_ptr()), float(buf))
        return self._win[1]

    def forward(self, hall, lq):
        return functional.time_warp_raw(hall, lq, self.p("WH/W"), self.p("WH/b"), self.p("WC/W"), self.p("WC/b"),
                                        self.warp_type, self.window_t())


def _glorot_any(gen, shape):
    """tf.get_variable's default initialiser as Model.init_parameters applies it to the front-end's variables"""
    fan = (shape[-3] * shape[-2], shape[-1]) if len(shape) >= 3 else (shape[0], shape[-1])
    lim = (6.0 / (fan[0] + fan[1])) ** 0.5
    return (torch.rand(shape, generator=gen) * 2 - 1) * lim


class TokenEmbedding(_Module):
    """The text front-end (model_v2.py:524-620): forward(word_ids [...], char_ids [..., W] | None, existing_emb_mat
    [G,wdim]) -> x [..., cwdim + wdim] = [char-CNN part | word part].  Ids < VW read `word/var/word_emb_mat` [VW,wdim]
    (trainable, N(0,1) rows as main.py:308), ids >= VW read existing_emb_mat[id - VW], the frozen pre-trained table: it
    gets no gradient.  With cwdim > 0 the char-CNN: `var/char_emb` [VC,cdim], `conv/conv1d/filter` [1,height,cdim,cwdim],
    `conv/conv1d/bias` [cwdim] (tf.get_variable's default, as Model initialises them).  The limits of fvta_embed_desc
    (cwdim <= 128, height <= W <= 64, VC <= 1024, ...) surface as the library's own error.  No char dropout here."""

    def __init__(self, VW, wdim, VC=0, cdim=0, cwdim=0, W=0, height=5, seed=None):
        super().__init__()
        self.VW, self.wdim, self.VC, self.cdim, self.cwdim, self.W, self.height = (int(v) for v in (VW, wdim, VC, cdim, cwdim, W, height))
        sd = lambda i: None if seed is None else seed + i
        self._param("word/var/word_emb_mat", torch.randn(self.VW, self.wdim, generator=_gen("word/var/word_emb_mat", sd(0))))
        if self.cwdim > 0:
            self._param("var/char_emb", _glorot_any(_gen("var/char_emb", sd(1)), (self.VC, self.cdim)))
            self._param("conv/conv1d/filter", _glorot_any(_gen("conv/conv1d/filter", sd(2)), (1, self.height, self.cdim, self.cwdim)))
            self._param("conv/conv1d/bias", _glorot_any(_gen("conv/conv1d/bias", sd(3)), (self.cwdim,)))

    def forward(self, word_ids, char_ids, existing_emb_mat):
        if self.cwdim > 0:
            if char_ids is None or char_ids.shape[-1] != self.W or tuple(char_ids.shape[:-1]) != tuple(word_ids.shape):
                raise ValueError("TokenEmbedding: char_ids must be word_ids' shape + [%d]" % self.W)
            return autograd.token_embed(word_ids, char_ids, self.p("word/var/word_emb_mat"), existing_emb_mat,
                                        self.p("var/char_emb"), self.p("conv/conv1d/filter"), self.p("conv/conv1d/bias"))
        return autograd.token_embed(word_ids, None, self.p("word/var/word_emb_mat"), existing_emb_mat)


class PhotoFeatures(_Module):
    """The photo front-end (model_v2.py:634-645): forward(pis [...], image_emb_mat [P,idim]) -> [..., tdim or idim].  With
    tdim: `image_transform/image_trans_linear/{W [idim,tdim] truncated normal(0.1), b [tdim] zeros}` (+ tanh with add_tanh);
    without, the gathered rows and no parameters.  image_emb_mat is the reference's placeholder: no gradient flows into it."""

    def __init__(self, idim, tdim=None, add_tanh=False, seed=None):
        super().__init__()
        self.idim, self.tdim, self.add_tanh = int(idim), (None if tdim is None else int(tdim)), bool(add_tanh)
        if self.tdim is not None:
            name = "image_transform/image_trans_linear/W"
            self._param(name, _trunc_normal(_gen(name, seed), (self.idim, self.tdim)))
            self._param("image_transform/image_trans_linear/b", torch.zeros(self.tdim))

    def forward(self, pis, image_emb_mat):
        if image_emb_mat.shape[-1] != self.idim:
            raise ValueError("PhotoFeatures: image_emb_mat is %s, idim %d" % (tuple(image_emb_mat.shape), self.idim))
        if self.tdim is None:
            return autograd.photo_features(pis, image_emb_mat)
        return autograd.photo_features(pis, image_emb_mat, self.p("image_transform/image_trans_linear/W"),
                                       self.p("image_transform/image_trans_linear/b"), self.add_tanh)


class AttentionGRU(_Module):
    """The AttentionGRUCell (attention_gru_cell.py:50-70) run over a whole fact sequence, the state carried:
    forward(facts [N,F,hidden], gate [N,F], h0 [N,hidden] | None) -> h_last [N,hidden] (autograd.attgru_seq, one library
    call each way).  A gate of 0 copies the state through, so a caller masks the gates of steps past a row's length.
    Parameters `attention_gru_cell/{gates/weights [2h,h], gates/biases [h], candidate/weights [h,h], input/weights [h,h],
    input/biases [h]}`: Glorot uniform / zeros (bias_start 0.0, :72)."""

    def __init__(self, hidden, seed=None):
        super().__init__()
        self.hidden = int(hidden)
        for i, (name, shape) in enumerate(functional._CELL_VARS):
            name = "attention_gru_cell/" + name
            sh = shape(self.hidden)
            self._param(name, torch.zeros(sh) if name.endswith("biases") else
                        _glorot(_gen(name, None if seed is None else seed + i), *sh))

    def forward(self, facts, gate, h0=None):
        if facts.shape[-1] != self.hidden:
            raise ValueError("AttentionGRU: facts %s do not fit hidden size %d" % (tuple(facts.shape), self.hidden))
        return autograd.attgru_seq(facts, gate, h0, *(self.p("attention_gru_cell/" + name) for name, _ in functional._CELL_VARS))


class EpisodicMemory(_Module):
    """The DMN+ episodic memory (model_dmnplus.py:503-516 over `_generate_episode` :113-136): forward(gq [N,hidden],
    facts [N,F,hidden], facts_length [N]) -> [N,hidden], differentiable in everything.  Parameters under dmn.py's names
    without the `memory/` scope -- `attention/fc{1,2}/{weights,biases}`, `attention_gru/rnn/attention_gru_cell/...`,
    `hop_<i>/dense/{kernel,bias}` -- and initialised like dmn.EpisodicMemory (the same draws for the same seed)."""

    def __init__(self, hidden, num_hops, seed=None):
        super().__init__()
        from . import dmn
        self.hidden, self.num_hops = int(hidden), int(num_hops)
        seed = zlib.crc32(b"memory") if seed is None else int(seed)
        for k, v in dmn.init_params(self.hidden, self.num_hops, seed).items():
            self._param(k[len("memory/"):], v)

    def forward(self, gq, facts, facts_length):
        from . import dmn
        if gq.shape[-1] != self.hidden or facts.shape[-1] != self.hidden:
            raise ValueError("EpisodicMemory: gq %s / facts %s do not fit hidden size %d" % (tuple(gq.shape), tuple(facts.shape), self.hidden))
        return functional.episodic_memory_raw(gq, facts, facts_length, *dmn.split_params(self._parameters, self.num_hops, prefix=""))


_GRU_VARS = ("gru_cell/gates/kernel", "gru_cell/gates/bias", "gru_cell/candidate/kernel", "gru_cell/candidate/bias")


def _gru_cell_init(in_dim, hidden, prefix, seed):
    """tf.nn.rnn_cell.GRUCell's four variables as TF creates them: Glorot uniform kernels (tf.get_variable's default), the
    gate bias 1, the candidate bias 0"""
    sd = lambda name, i: _gen(name, None if seed is None else seed + i)
    gk, ck = prefix + _GRU_VARS[0], prefix + _GRU_VARS[2]
    return {gk: _glorot(sd(gk, 0), in_dim + hidden, 2 * hidden), prefix + _GRU_VARS[1]: torch.ones(2 * hidden),
            ck: _glorot(sd(ck, 1), in_dim + hidden, hidden), prefix + _GRU_VARS[3]: torch.zeros(hidden)}


class GRUEncoder(_Module):
    """One dynamic_rnn over tf.nn.rnn_cell.GRUCell (the uni-directional encoders of model_dmnplus.py:344-440):
    forward(x [..., T, in_dim], lens [...]) -> (out [..., T, hidden] with rows t >= len zero, last [..., hidden]), one
    autograd.gru_seq over all leading axes flattened.  Parameters `gru_cell/gates/{kernel [in_dim+hidden, 2*hidden], bias
    [2*hidden]}` and `gru_cell/candidate/{kernel [in_dim+hidden, hidden], bias [hidden]}`: Glorot uniform kernels, the gate
    bias 1, the candidate bias 0 (TF's initialisers).  reverse=True walks every row from its last valid step down."""

    def __init__(self, in_dim, hidden, reverse=False, seed=None):
        super().__init__()
        self.in_dim, self.hidden, self.reverse = int(in_dim), int(hidden), bool(reverse)
        for k, v in _gru_cell_init(self.in_dim, self.hidden, "", seed).items():
            self._param(k, v)

    def forward(self, x, lens=None, h0=None):
        if x.shape[-1] != self.in_dim:
            raise ValueError("GRUEncoder: x %s does not fit in_dim %d" % (tuple(x.shape), self.in_dim))
        lead, T = tuple(x.shape[:-2]), x.shape[-2]
        out, last = autograd.gru_seq(x.reshape(-1, T, self.in_dim), None if lens is None else torch.as_tensor(lens).reshape(-1),
                                     None if h0 is None else h0.reshape(-1, self.hidden), *(self.p(n) for n in _GRU_VARS),
                                     reverse=self.reverse)
        return out.reshape(lead + (T, self.hidden)), last.reshape(lead + (self.hidden,))


def _bigru_sum(f_in, lens, fw_vars, bw_vars):
    """bidirectional_dynamic_rnn over two GRUCells, the two output sequences summed (model_dmnplus.py:478-486)"""
    fw, _ = autograd.gru_seq(f_in, lens, None, *fw_vars, reverse=False)
    bw, _ = autograd.gru_seq(f_in, lens, None, *bw_vars, reverse=True)
    return fw + bw


class BiGRUFusion(_Module):
    """The fusion of the facts (model_dmnplus.py:470-486): forward(f_in [N,F,hidden], lens [N]) -> [N,F,hidden] = the
    forward GRU's outputs + the backward GRU's, rows past a length zero.  Two autograd.gru_seq calls and one torch add.
    Parameters `{fw,bw}/gru_cell/{gates,candidate}/{kernel,bias}`, initialised as in GRUEncoder."""

    def __init__(self, hidden, seed=None):
        super().__init__()
        self.hidden = int(hidden)
        for i, dr in enumerate(_DIRS):
            for k, v in _gru_cell_init(self.hidden, self.hidden, dr + "/", None if seed is None else seed + 2 * i).items():
                self._param(k, v)

    def forward(self, f_in, lens=None):
        if f_in.dim() != 3 or f_in.shape[-1] != self.hidden:
            raise ValueError("BiGRUFusion: f_in %s does not fit hidden size %d" % (tuple(f_in.shape), self.hidden))
        return _bigru_sum(f_in, lens, *(tuple(self.p("%s/%s" % (dr, n)) for n in _GRU_VARS) for dr in _DIRS))


class DMNPlusHead(_Module):
    """The DMN+ baseline from the stacked facts to the choice logits (model_dmnplus.py:460-537): forward(lq [N,hidden],
    lchoices [N,C,hidden], f_in [N,F,hidden], facts_length [N]) -> logits [N,C].  The bi-directional GRU fusion of the
    facts (`input_facts/{fw,bw}/gru_cell/...`, as BiGRUFusion), the episodic memory over them with gq = lq (`memory/...`,
    as EpisodicMemory), then linear(concat([tile(gq), tile(output), gchoices]), 1) under `output/choicelogits/{W [3h,1]
    truncated normal(0.1), b [1] zeros}`.  Tiling and concat are torch plumbing; every product runs in the library.
    The loss is the caller's (the reference takes softmax cross-entropy of these logits), and there is no dropout: the
    reference's two tf.nn.dropout calls (:491, :521) are left out."""

    def __init__(self, hidden, num_hops, num_choice=4, seed=None):
        super().__init__()
        from . import dmn
        self.hidden, self.num_hops, self.num_choice = int(hidden), int(num_hops), int(num_choice)
        for i, dr in enumerate(_DIRS):
            pre = "input_facts/%s/" % dr
            for k, v in _gru_cell_init(self.hidden, self.hidden, pre, None if seed is None else seed + 2 * i).items():
                self._param(k, v)
        for k, v in dmn.init_params(self.hidden, self.num_hops, zlib.crc32(b"memory") if seed is None else int(seed) + 4).items():
            self._param(k, v)
        name = "output/choicelogits/W"
        self._param(name, _trunc_normal(_gen(name, None if seed is None else seed + 5), (3 * self.hidden, 1)))
        self._param("output/choicelogits/b", torch.zeros(1))

    def forward(self, lq, lchoices, f_in, facts_length):
        from . import dmn
        h, C = self.hidden, self.num_choice
        if lq.shape[-1] != h or f_in.shape[-1] != h or tuple(lchoices.shape[1:]) != (C, h):
            raise ValueError("DMNPlusHead: lq %s / lchoices %s / f_in %s do not fit hidden size %d, %d choices"
                             % (tuple(lq.shape), tuple(lchoices.shape), tuple(f_in.shape), h, C))
        facts = _bigru_sum(f_in, facts_length, *(tuple(self.p("input_facts/%s/%s" % (dr, n)) for n in _GRU_VARS) for dr in _DIRS))
        gq = lq.to(torch.float32)
        output = functional.episodic_memory_raw(gq, facts, facts_length, *dmn.split_params(self._parameters, self.num_hops))
        cat = torch.cat([gq[:, None, :].expand(-1, C, -1), output[:, None, :].expand(-1, C, -1), lchoices.to(torch.float32)], 2)
        logits = functional.linear_raw(cat.contiguous(), self.p("output/choicelogits/W"), self.p("output/choicelogits/b"))
        return logits.reshape(-1, C)


_MCB_TABLES = ("rand_h_1", "rand_s_1", "rand_h_2", "rand_s_2")


def _register_tables(mod, prefix, d1, d2, D, seeds=(1, 3, 5, 7)):
    """the layer's four count sketch tables, drawn as the reference draws them, as buffers of `mod` (its own copies:
    load_state_dict writes into them)"""
    for name, t in zip(_MCB_TABLES, ops.upload_sketch_tables(*ops.count_sketch_tables(d1, d2, D, seeds), d1, d2, D)):
        mod.register_buffer(prefix + name, t)


class CompactBilinearPooling(_Module):
    """compact_bilinear_pooling_layer (model_mcb.py:1254-1363) as a module: forward(bottom1 [B,H,W,d1], bottom2 [B,H,W,d2]
    or [B,1,1,d2]) -> [B,H,W,output_dim] (sum_pool=True: [B,output_dim]); with normalize the l2_normalize(sqrt|.|) of :645
    is fused behind the pooling (and sum_pool is refused: the reference normalises the un-pooled rows).  The four count
    sketch tables are BUFFERS (`rand_h_1`, `rand_s_1`, `rand_h_2`, `rand_s_2`), drawn from `seeds` exactly as the
    reference draws them (ops.count_sketch_tables), so they travel in state_dict(); no parameters."""

    def __init__(self, d1, d2, output_dim, normalize=False, sum_pool=False, seeds=(1, 3, 5, 7)):
        super().__init__()
        self.d1, self.d2, self.output_dim = int(d1), int(d2), int(output_dim)
        self.normalize, self.sum_pool = bool(normalize), bool(sum_pool)
        if self.normalize and self.sum_pool:
            raise ValueError("CompactBilinearPooling: normalize applies to the un-pooled rows, not with sum_pool")
        _register_tables(self, "", self.d1, self.d2, self.output_dim, seeds)

    def forward(self, bottom1, bottom2):
        if bottom1.dim() != 4 or bottom2.dim() != 4 or bottom1.shape[-1] != self.d1 or bottom2.shape[-1] != self.d2:
            raise ValueError("CompactBilinearPooling: bottoms %s / %s do not fit d1 = %d, d2 = %d"
                             % (tuple(bottom1.shape), tuple(bottom2.shape), self.d1, self.d2))
        return functional.compact_bilinear_pooling_raw(bottom1, bottom2, tuple(self._buffers[n] for n in _MCB_TABLES),
                                                       self.output_dim, sum_pool=self.sum_pool, normalize=self.normalize)


def _mcb_attention_init(mod, prefix, idim, qdim, mcb_outdim, conv1_out, seed):
    """the variables and tables of `mcb_attention` (model_mcb.py:641-664) on module `mod`, below `prefix`"""
    _register_tables(mod, prefix, idim, qdim, mcb_outdim)
    for i, (name, shape) in enumerate((("filter_conv1", (mcb_outdim, conv1_out)), ("filter_conv2", (conv1_out, 1)))):
        mod._param(prefix + name, _trunc_normal(_gen(prefix + name, None if seed is None else seed + i), shape, std=0.02))


def _mcb_attention(mod, prefix, hpis, gq):
    tabs = tuple(mod._buffers[prefix + n] for n in _MCB_TABLES)
    return functional.mcb_attention_raw(hpis, gq, tabs, mod.p(prefix + "filter_conv1"), mod.p(prefix + "filter_conv2"))


class MCBAttention(_Module):
    """The MCB attention over the photos (model_mcb.py:623-672): forward(hpis [N,M,JI,idim], gq [N,qdim]) -> (attended
    [N,idim], att [N, M*JI]) through functional.mcb_attention_raw.  Parameters `filter_conv1` [mcb_outdim, conv1_out] and
    `filter_conv2` [conv1_out, 1], truncated normal(0.02): the reference's [1,1,in,out] 1x1 convolution filters without
    their two leading axes.  The count sketch tables are buffers, drawn as the reference draws them (seeds 1/3/5/7).
    No dropout (:649) and no NaN scrubs, as functional.mcb_attention_raw says."""

    def __init__(self, idim, qdim, mcb_outdim=16000, conv1_out=512, seed=None):
        super().__init__()
        self.idim, self.qdim, self.mcb_outdim, self.conv1_out = int(idim), int(qdim), int(mcb_outdim), int(conv1_out)
        _mcb_attention_init(self, "", self.idim, self.qdim, self.mcb_outdim, self.conv1_out, seed)

    def forward(self, hpis, gq):
        if hpis.dim() != 4 or hpis.shape[-1] != self.idim or gq.dim() != 2 or gq.shape[-1] != self.qdim:
            raise ValueError("MCBAttention: hpis %s / gq %s do not fit idim = %d, qdim = %d"
                             % (tuple(hpis.shape), tuple(gq.shape), self.idim, self.qdim))
        return _mcb_attention(self, "", hpis, gq)


class MCBHead(_Module):
    """The MCB baseline from the encoders' outputs to the choice logits (model_mcb.py:614-748): forward(lq [N,hidden2],
    g1 [N,hidden2], hpis [N,M,JI,idim], lchoices [N,C,hidden2]) -> logits [N,C]; the attention weights of the call are
    kept as `.att` [N, M*JI].  hidden2 is the reference's 2d (a bi-LSTM's last state).  gq = lq attends the raw photo rows
    (`mcb_attention/{filter_conv1, filter_conv2}` and the table buffers, as MCBAttention), the attended row goes through `mcb_attention/g_mcb_trans/{W [idim,hidden2],
    b}` (:681), and `output/att_logits/{W [7*hidden2, 1], b}` scores concat([gq, g1, g_mcb, gchoices, gq*g1, gq*g_mcb,
    gq*gchoices]) per choice (:740); both linears truncated normal(0.1) / zeros, with tanh under add_tanh.  g1 is the
    mean-pooled text representation of :700-717, torch plumbing the caller writes.  Tiling, concat and
    the three element-wise products are torch; every matrix product runs in the library.
    Left out: the tf.nn.dropout of :649, the forward NaN scrubs of :621 / :635 / :646 / :715 (inputs are taken to be
    finite) and the loss (the reference takes softmax cross-entropy of these logits)."""

    def __init__(self, idim, hidden2, mcb_outdim=16000, num_choice=4, add_tanh=False, conv1_out=512, seed=None):
        super().__init__()
        self.idim, self.hidden2, self.num_choice, self.add_tanh = int(idim), int(hidden2), int(num_choice), bool(add_tanh)
        self.mcb_outdim, self.conv1_out = int(mcb_outdim), int(conv1_out)
        _mcb_attention_init(self, "mcb_attention/", self.idim, self.hidden2, self.mcb_outdim, self.conv1_out, seed)
        sd = lambda i: None if seed is None else seed + i
        for i, (name, shape) in enumerate((("mcb_attention/g_mcb_trans/W", (self.idim, self.hidden2)),
                                           ("output/att_logits/W", (7 * self.hidden2, 1)))):
            self._param(name, _trunc_normal(_gen(name, sd(2 + i)), shape))
            self._param(name[:-1] + "b", torch.zeros(shape[1]))
        self.att = None

    def forward(self, lq, g1, hpis, lchoices):
        h, C = self.hidden2, self.num_choice
        if lq.shape[-1] != h or g1.shape[-1] != h or tuple(lchoices.shape[1:]) != (C, h):
            raise ValueError("MCBHead: lq %s / g1 %s / lchoices %s do not fit hidden2 = %d, %d choices"
                             % (tuple(lq.shape), tuple(g1.shape), tuple(lchoices.shape), h, C))
        gq, g1, gch = lq.to(torch.float32), g1.to(torch.float32), lchoices.to(torch.float32)
        if hpis.dim() != 4 or hpis.shape[-1] != self.idim:
            raise ValueError("MCBHead: hpis %s does not fit [N,M,JI,%d]" % (tuple(hpis.shape), self.idim))
        attended, att = _mcb_attention(self, "mcb_attention/", hpis, gq)
        self.att = att.detach()
        g_mcb = functional.linear_raw(attended, self.p("mcb_attention/g_mcb_trans/W"), self.p("mcb_attention/g_mcb_trans/b"),
                                      self.add_tanh)
        tile = lambda t: t[:, None, :].expand(-1, C, -1)
        q_t, g1_t, m_t = tile(gq), tile(g1), tile(g_mcb)
        cat = torch.cat([q_t, g1_t, m_t, gch, q_t * g1_t, q_t * m_t, q_t * gch], 2)
        logits = functional.linear_raw(cat.contiguous(), self.p("output/att_logits/W"), self.p("output/att_logits/b"), self.add_tanh)
        return logits.reshape(-1, C)
