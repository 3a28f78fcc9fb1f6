"""Thin host-side handles over the C ABI (include/fvta_hip.h).

These classes own the descriptor + scratch/saved buffers of one kernel family
and pass raw device pointers to libfvta_hip.so.  No arithmetic happens here and
there is no CPU path: every call needs a GPU and the built library.
"""
import ctypes

import torch

from . import _lib
from ._lib import (F32, BF16, AttGruSeqDesc, AttnDesc, EmbedDesc, GruSeqDesc, ImgTransDesc, LstmDesc, ScorerDesc, TimewarpDesc, check,
                   ptr, stream_ptr)


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.FvtaError("fvta_memexqa_amd needs an MI355X (no GPU visible); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _f32c(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expected a contiguous float32 CUDA tensor"
    return t


def _bytes(n, dev):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=dev)


def _sized(op, query, prefix, *args):
    """a buffer of the bytes the library's size query names for op.desc; 0 is its refusal, raised with its message"""
    nb = getattr(op.lib, query)(ctypes.byref(op.desc), *args)
    if nb == 0:
        raise _lib.FvtaError(prefix + op.lib.fvta_last_error().decode())
    return _bytes(nb, op.dev)


# ------------------------------------------------------------------ side stream
def concurrency_ratio(main, cand, spin_us=400, repeats=3, others=()):
    """time(one spin wave on each of the streams main, others..., cand) / time(one spin wave on `main`): about 1 when
    they all run concurrently, 2 or more when HIP mapped some of them onto the same hardware queue."""
    import time
    lib = _lib.load()

    def run(streams):
        best = float("inf")
        for _ in range(repeats):
            for s in streams:
                s.synchronize()
            t0 = time.perf_counter()
            for s in streams:
                check(lib.fvta_probe_spin(spin_us, ctypes.c_void_p(s.cuda_stream)), "fvta_probe_spin")
            for s in streams:
                s.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    group = [main] + list(others) + [cand]
    run(group)                              # first use creates the hardware queues
    return run(group) / run([main])


def pick_side_stream(dev, main=None, candidates=8, others=(), priority=0):
    """A HIP stream that really runs beside `main` (and beside every stream in `others`).  HIP maps streams onto a small pool of hardware queues
    (GPU_MAX_HW_QUEUES, 4 by default) and two streams on one queue serialise; which streams collide depends on how
    many were created before -- an RCCL communicator created ahead of the model moved the side stream onto the main
    stream's queue and the training step lost the photo-cell overlap (21.9 ms instead of 15.7 ms,
    tools/dist_probe.py).  So the choice is measured: candidates are tried in turn with fvta_probe_spin and the
    first one that overlaps with `main` wins.  Rejected candidates stay referenced until the search ends so that the
    next one is mapped to another queue."""
    main = main if main is not None else torch.cuda.current_stream(dev)
    tried, best = [], None
    for _ in range(candidates):
        cand = torch.cuda.Stream(device=dev, priority=priority)
        r = concurrency_ratio(main, cand, others=others)
        tried.append(cand)
        if best is None or r < best[0]:
            best = (r, cand)
        if r < 1.4:
            break
    return best[1], best[0]


# ------------------------------------------------------------------ test hook
def test_gemm(A, B, layout, precision=F32):
    lib = _lib.load()
    require_gpu()
    if layout == 0:
        M, K = A.shape
        N = B.shape[1]
    elif layout in (1, 3):      # row images (3: the split engine's two-term il32 rows)
        M, K = A.shape
        N = B.shape[0]
    else:                       # k-major images (4: split engine)
        K, M = A.shape
        N = B.shape[1]
    C = torch.empty(M, N, device=A.device, dtype=torch.float32)
    check(lib.fvta_test_gemm(precision, layout, M, N, K, ptr(_f32c(A)), ptr(_f32c(B)), ptr(C), stream_ptr()), "test_gemm")
    return C


# ------------------------------------------------------------------- encoders
class BiLstm:
    """One bi-LSTM call group (all sequences sharing a cell): model_v2.py:694-823.

    x_off/out_off: int64 [B] element offsets of each sequence's first row in the
    x / out arenas; seq_J: padded length per sequence; out_ld: output row stride.
    """

    def __init__(self, B, J, in_dim, d, x_off, out_off, seq_J, out_ld, share_fw_bw=True, precision=F32,
                 training=False, prof_tag=0, x_bw_delta=0, dx_overwrite=False, out_pads_persist=False, out_skip=0):
        """x_bw_delta > 0: the backward direction reads x (writes dx) that many elements behind the forward direction's
        -- x = [x_fw | x_bw], the two dropped copies of DropoutWrapper's inputs (dropout_pair_fwd).
        dx_overwrite: backward() writes dx (zeros at padded positions) instead of adding to it: no memset by the caller.
        out_pads_persist: the caller leaves `out` alone between forward calls: only rows that turn into padding are zeroed.
        out_skip (bf16 engine): output half-rows at element offsets below it are not stored in fp32 -- their readers take
        the bf16 shadow rows (shadow_rows; FocalAttention.forward_shadow / backward_shadow)."""
        self.x_bw_delta = int(x_bw_delta)
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.desc = LstmDesc(B, J, in_dim, d, int(share_fw_bw), precision, int(training), int(prof_tag), int(dx_overwrite), int(out_pads_persist),
                             int(out_skip))
        self.B, self.J, self.in_dim, self.d = B, J, in_dim, d
        self.x_off = x_off.to(self.dev, torch.int64).contiguous()
        self.out_off = out_off.to(self.dev, torch.int64).contiguous()
        self.seq_J = seq_J.to(self.dev, torch.int32).contiguous()
        self.out_ld = int(out_ld)
        r = ctypes.byref(self.desc)
        self.plan = _bytes(self.lib.fvta_lstm_plan_bytes(r), self.dev).zero_()   # (no stale plan state: out_pads_persist)
        self.saved = _bytes(self.lib.fvta_lstm_saved_bytes(r), self.dev)
        self.work = _bytes(self.lib.fvta_lstm_workspace_bytes(r), self.dev)
        self.training = training
        self.share = share_fw_bw

    def make_plan(self, lens):
        lens = lens.to(self.dev, torch.int32).contiguous()
        check(self.lib.fvta_lstm_plan_xdir(ctypes.byref(self.desc), ptr(lens), ptr(self.seq_J), ptr(self.x_off),
                                           ptr(self.out_off), self.out_ld, self.x_bw_delta, ptr(self.plan), stream_ptr()),
              "fvta_lstm_plan")

    def forward(self, x, out, kernel_fw, bias_fw, kernel_bw=None, bias_bw=None):
        check(self.lib.fvta_bilstm_fwd(ctypes.byref(self.desc), ptr(self.plan), ptr(_f32c(x)), ptr(_f32c(out)),
                                       ptr(_f32c(kernel_fw)), ptr(_f32c(bias_fw)), ptr(kernel_bw), ptr(bias_bw),
                                       ptr(self.saved), ptr(self.work), stream_ptr()), "fvta_bilstm_fwd")

    def shadow_rows(self, table, nrows):
        """table int64 [2, nrows] (device): the addresses of this call's bf16 output half-rows, by output row (out offset //
        out_ld) -- only the rows t < len of this plan's sequences are written, see fvta_lstm_shadow_rows.  After forward()."""
        assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() == 2 * nrows
        check(self.lib.fvta_lstm_shadow_rows(ctypes.byref(self.desc), ptr(self.plan), ptr(self.saved), int(nrows), ptr(table),
                                             stream_ptr()), "fvta_lstm_shadow_rows")

    def set_active_hint(self, lens_host):
        """What the host knows about the lengths of the NEXT plan (a numpy / list of the B lengths, or None): the backward
        recurrence sizes each step's launch by its active sequences (fvta_bilstm_bwd_hint).  Optional; a stale hint costs
        time, never correctness."""
        if lens_host is None:
            self.active_hint = None
            return
        import numpy as np
        ln = np.clip(np.asarray(lens_host, dtype=np.int64).reshape(-1), 0, self.J)
        below = np.cumsum(np.bincount(ln, minlength=self.J + 1))[:self.J]      # sequences with len <= t
        self.active_hint = np.ascontiguousarray(ln.size - below, dtype=np.int32)   # nactive[t] = #(len > t)

    def backward(self, x, out, d_out, kernel_fw, kernel_bw, dx, dk_fw, db_fw, dk_bw=None, db_bw=None, side_stream=None):
        """side_stream (a torch stream, bf16 engine): dx and the per-step-group weight gradients run there, beside the
        recurrence (fvta_bilstm_bwd_overlap); the current stream has joined it again when this returns."""
        side = ctypes.c_void_p(side_stream.cuda_stream) if side_stream is not None else None
        hint = getattr(self, "active_hint", None)
        hp = hint.ctypes.data_as(ctypes.c_void_p) if hint is not None else None
        check(self.lib.fvta_bilstm_bwd_hint(ctypes.byref(self.desc), ptr(self.plan), ptr(x), ptr(out), ptr(_f32c(d_out)),
                                            ptr(kernel_fw), ptr(kernel_bw), ptr(self.saved), ptr(dx), ptr(dk_fw),
                                            ptr(db_fw), ptr(dk_bw), ptr(db_bw), ptr(self.work), stream_ptr(), side, hp),
              "fvta_bilstm_bwd")

    def last_state(self, out, s0, count, dst):
        check(self.lib.fvta_lstm_last_state(ctypes.byref(self.desc), ptr(self.plan), ptr(out), s0, count, ptr(dst),
                                            stream_ptr()), "fvta_lstm_last_state")

    def last_state_bwd(self, d_dst, s0, count, d_out):
        check(self.lib.fvta_lstm_last_state_bwd(ctypes.byref(self.desc), ptr(self.plan), ptr(_f32c(d_dst)), s0, count,
                                                ptr(d_out), stream_ptr()), "fvta_lstm_last_state_bwd")


def rows_from_shadow(table, nrows, d, out_ld, out):
    """out [nrows, out_ld] fp32 <- the bf16 rows behind a shadow table (inspection outputs, tests)"""
    check(_lib.load().fvta_rows_from_shadow(ptr(table), int(nrows), int(d), int(out_ld), ptr(out), stream_ptr()),
          "fvta_rows_from_shadow")


def dropout_pair_fwd(x, x2, keep_prob, seed):
    """x2 [2, numel(x)] = the forward / backward direction's dropped copy of x (DropoutWrapper, model_v2.py:657-661)"""
    check(_lib.load().fvta_dropout_pair_fwd(ptr(x), ptr(x2), x.numel(), float(keep_prob), int(seed) & (2 ** 64 - 1), stream_ptr()),
          "fvta_dropout_pair_fwd")


def dropout_pair_bwd(dx2, dx, keep_prob, seed, accumulate=False):
    check(_lib.load().fvta_dropout_pair_bwd(ptr(dx2), ptr(dx), dx.numel(), float(keep_prob), int(seed) & (2 ** 64 - 1),
                                            int(accumulate), stream_ptr()), "fvta_dropout_pair_bwd")


def bilstm_simple(x, lens, kernel_fw, bias_fw, kernel_bw=None, bias_bw=None, training=False, precision=F32):
    """x [B,J,in] dense, lens [B] -> out [B,J,2d], last [B,2d] (test/convenience form)."""
    B, J, din = x.shape
    d = kernel_fw.shape[1] // 4
    ar = torch.arange(B, dtype=torch.int64)
    op = BiLstm(B, J, din, d, ar * J * din, ar * J * 2 * d, torch.full((B,), J, dtype=torch.int32), 2 * d,
                share_fw_bw=kernel_bw is None, precision=precision, training=training)
    op.make_plan(lens)
    out = torch.empty(B, J, 2 * d, device=x.device, dtype=torch.float32)
    op.forward(x.contiguous(), out, kernel_fw, bias_fw, kernel_bw, bias_bw)
    last = torch.empty(B, 2 * d, device=x.device, dtype=torch.float32)
    op.last_state(out, 0, B, last)
    return out, last, op


# ------------------------------------------------------------------ attention
class FocalAttention:
    """attention_3d (model_v2.py:210-298) / attention (125-201, K=1) handle."""

    def __init__(self, N, K, T, JQ, w, simi, add_tanh, feat_order=0, hinfo_stride=0):
        """hinfo_stride (K == 1): floats between consecutive batch rows of hinfo / d_hinfo, for a stream that lives
        inside a wider arena; the tensors handed to forward / backward then start at the stream's first row."""
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.desc = AttnDesc(N, K, T, JQ, w, simi, feat_order, int(add_tanh), int(hinfo_stride))
        r = ctypes.byref(self.desc)
        sb = self.lib.fvta_attn_saved_bytes(r)
        if sb == 0:
            raise _lib.FvtaError("attention: " + self.lib.fvta_last_error().decode())
        self.saved = _bytes(sb, self.dev)
        self.work = _bytes(self.lib.fvta_attn_workspace_bytes(r), self.dev)
        self.N, self.K, self.T, self.JQ, self.w = N, K, T, JQ, w

    def plan(self, use_mask=True):
        """{nsplit, bsplit, gk, ng}: how the kernels split this shape's work (fvta_attn_plan; host only)"""
        out = (ctypes.c_int32 * 4)()
        check(self.lib.fvta_attn_plan(ctypes.byref(self.desc), int(bool(use_mask)), out), "fvta_attn_plan")
        return dict(zip(("nsplit", "bsplit", "gk", "ng"), (int(v) for v in out)))

    def forward(self, hinfo, hq, hmask, qmask, W, b, want_logits=False, tscale=None):
        """tscale [N,T] (time_warp_att, model_v2.py:269-275): the softmax over t runs on amax * tscale."""
        h_a = torch.empty(self.N, self.w, device=self.dev, dtype=torch.float32)
        a_logits = torch.empty(self.N, self.K, self.T, self.JQ, device=self.dev, dtype=torch.float32) if want_logits else None
        check(self.lib.fvta_attn_fwd_tw(ctypes.byref(self.desc), ptr(_f32c(hinfo)), ptr(_f32c(hq)), ptr(hmask), ptr(qmask),
                                        ptr(W), ptr(b), ptr(tscale), ptr(h_a), ptr(a_logits), ptr(self.saved),
                                        ptr(self.work), stream_ptr()), "fvta_attn_fwd")
        return h_a, a_logits

    def forward_shadow(self, table, hq, hmask, qmask, W, b):
        """forward() over the encoders' bf16 shadow rows: table int64 [2, N*K*T] (BiLstm.shadow_rows)"""
        h_a = torch.empty(self.N, self.w, device=self.dev, dtype=torch.float32)
        check(self.lib.fvta_attn_fwd_shadow(ctypes.byref(self.desc), ptr(table), ptr(_f32c(hq)), ptr(hmask), ptr(qmask),
                                            ptr(W), ptr(b), ptr(h_a), ptr(self.saved), ptr(self.work), stream_ptr()),
              "fvta_attn_fwd_shadow")
        return h_a

    def backward_shadow(self, table, hq, hmask, qmask, W, b, d_h_a, d_hinfo, d_hq, dW, db, accumulate):
        check(self.lib.fvta_attn_bwd_shadow(ctypes.byref(self.desc), ptr(table), ptr(hq), ptr(hmask), ptr(qmask), ptr(W),
                                            ptr(b), ptr(_f32c(d_h_a)), ptr(self.saved), ptr(d_hinfo), ptr(d_hq),
                                            ptr(dW), ptr(db), int(accumulate), ptr(self.work), stream_ptr()),
              "fvta_attn_bwd_shadow")

    def backward(self, hinfo, hq, hmask, qmask, W, b, d_h_a, d_hinfo, d_hq, dW, db, accumulate, tscale=None,
                 d_tscale=None):
        check(self.lib.fvta_attn_bwd_tw(ctypes.byref(self.desc), ptr(hinfo), ptr(hq), ptr(hmask), ptr(qmask), ptr(W),
                                        ptr(b), ptr(tscale), ptr(_f32c(d_h_a)), ptr(self.saved), ptr(d_hinfo), ptr(d_hq),
                                        ptr(dW), ptr(db), ptr(d_tscale), int(accumulate), ptr(self.work), stream_ptr()),
              "fvta_attn_bwd")

    def backward_u(self, hinfo, hq, hmask, qmask, W, b, d_u, d_hinfo, d_hq, dW, db, accumulate):
        """the backward of forward() + fvta_attn_read_u from d_u [N,K,w]: every (n,k) an attention of its own
        (fvta_attn_bwd_u; simiMatrix 1-3, accumulate 0 | 1, N * K <= 65535).  Its workspace is sized by its own query and
        allocated on first use: one dQs slab set per (n,k), 136 MB at N K = 1040 and w = 64."""
        if getattr(self, "work_u", None) is None:
            nb = self.lib.fvta_attn_bwd_u_workspace_bytes(ctypes.byref(self.desc))
            if nb == 0:
                raise _lib.FvtaError("attention: " + self.lib.fvta_last_error().decode())
            self.work_u = _bytes(nb, self.dev)
        check(self.lib.fvta_attn_bwd_u(ctypes.byref(self.desc), ptr(hinfo), ptr(hq), ptr(hmask), ptr(qmask), ptr(W), ptr(b),
                                       ptr(_f32c(d_u)), ptr(self.saved), ptr(d_hinfo), ptr(d_hq), ptr(dW), ptr(db),
                                       int(accumulate), ptr(self.work_u), stream_ptr()), "fvta_attn_bwd_u")

    def read_u(self):
        """u [N,K,w]: the per-(n,k) softsel result the last forward() left in `saved` (fvta_attn_read_u)"""
        u = torch.empty(self.N, self.K, self.w, dtype=torch.float32, device=self.dev)
        check(self.lib.fvta_attn_read_u(ctypes.byref(self.desc), ptr(self.saved), ptr(u), stream_ptr()), "fvta_attn_read_u")
        return u


# ------------------------------------------------------------------ attention, many questions over one album
def check_album_index(album, A):
    """Host-side validation of a question -> album index, before it is uploaded (the kernels only clamp it): one
    dimension, an integer dtype, every value in [0, A).  Returns it as a contiguous int32 CPU tensor.  Pure host: no GPU,
    no library."""
    t = album if torch.is_tensor(album) else torch.as_tensor(album)
    if t.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError("album index: an integer dtype is needed, got %s" % t.dtype)
    if t.dim() != 1:
        raise ValueError("album index: expected one dimension [NQ], got shape %s" % (tuple(t.shape),))
    t = t.detach().cpu()
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= int(A)):
        raise ValueError("album index: values must lie in [0, %d), got [%d, %d]" % (int(A), int(t.min()), int(t.max())))
    return t.to(torch.int32).contiguous()


class _AlbumAttention:
    """What the four classes of this section share: context rows held ONCE ([A,K,T,w] per album, or a pool [P,K,JX,w]),
    an int32 index on the device that says which of them a question reads (album [NQ], or albums [NQ,M]), and the library's
    entry points under one prefix (fvta_attn_shared / fvta_attn_pool).  A subclass's constructor names the prefix, the
    FvtaError prefix, the descriptor, the rows' and the index's shape and the positions per question (T, or M*JX)."""
    _tw, _sep = "", " "               # the warped pair: "_tw" in its size queries, ", " in its messages

    def _setup(self, sym, what, desc, rows_shape, index_shape, positions):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self._sym, self._what, self.desc = sym, what, desc
        self._shape_desc = desc.shape if self._tw else desc
        self._rows, self._index, self._TO = tuple(rows_shape), tuple(index_shape), int(positions)
        # (under the warp a refusal may be a bad warp type: "time warping type not implemented", model_v2.py:341)
        self.work = _sized(self, sym + self._tw + "_workspace_bytes", what + ": ")

    def _call(self, name, *args):
        check(getattr(self.lib, name)(ctypes.byref(self.desc), *args, stream_ptr()), name)

    def _rows_arg(self, rows):
        """(suffix of the entry point's name, the rows' pointer) of an inference call.  A pool held as a contiguous
        torch.bfloat16 tensor goes to the pooled calls' _bf16 entry points AS IT IS -- no fp32 copy; their result is the
        fp32 call's on the widened rows, bit for bit.  Anything else must be contiguous fp32, as ever."""
        if rows.dtype == torch.bfloat16 and self._sym == "fvta_attn_pool":
            assert rows.is_cuda and rows.is_contiguous(), "expected a contiguous bfloat16 CUDA tensor"
            return "_bf16", ptr(rows)
        return "", ptr(_f32c(rows))

    def _words(self, name, keys):
        out = (ctypes.c_int32 * 4)()
        check(getattr(self.lib, name)(ctypes.byref(self._shape_desc), out), name)
        return dict(zip(keys, (int(v) for v in out)))

    def plan(self):
        """{G, rows, tsplit, rows_per_split}: questions (references) per group, rows per logits tile, splits of T (JX) in
        the weighted sum and the rows of one split (fvta_attn_{shared,pool}_plan; host only; the warp changes none)"""
        return self._words(self._sym + "_plan", ("G", "rows", "tsplit", "rows_per_split"))

    def bwd_plan(self):
        """{rows, tsplit, channels, tiles_per_wg}: rows per tile of the backward's row pass, T (JX) splits and channels per
        slice of its question pass, row tiles per workgroup of the row pass (fvta_attn_{shared,pool}_bwd_plan; host only,
        simiMatrix 1-3; the warp changes none)"""
        return self._words(self._sym + "_bwd_plan", ("rows", "tsplit", "channels", "tiles_per_wg"))

    def _check_inputs(self, rows, rows_mask, hq, qmask, index):
        assert tuple(rows.shape) == self._rows and tuple(hq.shape) == (self.NQ, self.JQ, self.w)
        assert index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and tuple(index.shape) == self._index
        assert rows_mask is None or (rows_mask.dtype == torch.uint8 and tuple(rows_mask.shape) == self._rows[:3])
        assert qmask is None or (qmask.dtype == torch.uint8 and tuple(qmask.shape) == (self.NQ, self.JQ))

    def _run(self, train, rows, rows_mask, hq, qmask, index, W, b, want_logits, warp=None, want_scale=False):
        """the forward call: -> (h_a [NQ,w], a_logits [NQ,K,positions,JQ] | None), under the warp also scale
        [NQ,positions] | None.  train: leaves in self.saved (allocated on first use) what backward() reads.
        warp: (energy, lq, WH_b, WC_W, WC_b), which the entry points under the time warp take between the others"""
        self._check_inputs(rows, rows_mask, hq, qmask, index)
        if warp is not None:
            energy, lq, WH_b, WC_W, WC_b = warp
            assert tuple(energy.shape) == (self._rows[0], self._rows[2]) and tuple(lq.shape) == (self.NQ, self.w)
            assert WH_b.numel() == self.w and WC_W.numel() == self.w and WC_b.numel() == 1
        if train and getattr(self, "saved", None) is None:
            self.saved = _sized(self, self._sym + self._tw + "_saved_bytes", self._what + self._sep + "saved: ")
        h_a = torch.empty(self.NQ, self.w, device=self.dev, dtype=torch.float32)
        a_logits = torch.empty(self.NQ, self.K, self._TO, self.JQ, device=self.dev, dtype=torch.float32) if want_logits else None
        scale = torch.empty(self.NQ, self._TO, device=self.dev, dtype=torch.float32) if want_scale else None
        W = _f32c(W) if train else W                                 # (inference: simiMatrix 4 takes no W)
        e, q, wb, sc = [], [], [], []                                # the warp's arguments, where the entry points take them
        if warp is not None:
            e, q, sc = [ptr(_f32c(energy))], [ptr(_f32c(lq))], [ptr(scale)]
            wb = [ptr(_f32c(WH_b)), ptr(_f32c(WC_W)), ptr(_f32c(WC_b))]
        bf16, rows_ptr = ("", ptr(_f32c(rows))) if train else self._rows_arg(rows)   # (training: fp32 rows only)
        args = [rows_ptr, ptr(rows_mask)] + e + [ptr(_f32c(hq)), ptr(qmask)] + q + [ptr(index), ptr(W), ptr(b)] + wb + \
            [ptr(h_a), ptr(a_logits)] + sc + ([ptr(self.saved)] if train else []) + [ptr(self.work)]
        self._call(self._sym + "_fwd" + self._tw + ("_train" if train else "") + bf16, *args)
        return (h_a, a_logits) if warp is None else (h_a, a_logits, scale)

    def forward(self, rows, rows_mask, hq, qmask, index, W, b, want_logits=False):
        """the inference call (fvta_attn_{shared,pool}_fwd): nothing kept"""
        return self._run(False, rows, rows_mask, hq, qmask, index, W, b, want_logits)

    def forward_train(self, rows, rows_mask, hq, qmask, index, W, b, want_logits=False):
        """forward() -- the same bits -- that leaves in self.saved (allocated on first use) what backward() reads
        (fvta_attn_{shared,pool}_fwd_train; simiMatrix 1-3)"""
        return self._run(True, rows, rows_mask, hq, qmask, index, W, b, want_logits)

    def _begin_backward(self, rows, rows_mask, hq, qmask, index, d_h_a, d_rows, d_hq, *grads):
        """what every backward starts with: the saved state, the workspace (allocated on first use), the arguments"""
        if getattr(self, "saved", None) is None:
            raise _lib.FvtaError(self._what + ": backward() needs a forward_train() first")
        if getattr(self, "work_bwd", None) is None:
            self.work_bwd = _sized(self, self._sym + self._tw + "_bwd_workspace_bytes",
                                   self._what + self._sep + "backward workspace: ")
        self._check_inputs(rows, rows_mask, hq, qmask, index)
        assert tuple(d_rows.shape) == self._rows and tuple(d_hq.shape) == (self.NQ, self.JQ, self.w)
        assert tuple(d_h_a.shape) == (self.NQ, self.w)
        for t in (d_rows, d_hq) + grads:
            assert t.is_contiguous() and t.dtype == torch.float32, "gradient outputs are written in place"

    def backward(self, rows, rows_mask, hq, qmask, index, W, b, d_h_a, d_rows, d_hq, dW, db):
        """After forward_train() with the same arguments: d_rows (the rows' shape) and d_hq [NQ,JQ,w] are overwritten, dW
        [F] and db [1] accumulated into (fvta_attn_{shared,pool}_bwd).  Its workspace is allocated on first use."""
        self._begin_backward(rows, rows_mask, hq, qmask, index, d_h_a, d_rows, d_hq, dW, db)
        self._call(self._sym + "_bwd", ptr(_f32c(rows)), ptr(rows_mask), ptr(_f32c(hq)), ptr(qmask), ptr(index), ptr(_f32c(W)),
                   ptr(b), ptr(_f32c(d_h_a)), ptr(self.saved), ptr(d_rows), ptr(d_hq), ptr(_f32c(dW)), ptr(_f32c(db)),
                   ptr(self.work_bwd))


class _WarpedAlbumAttention(_AlbumAttention):
    """_AlbumAttention under the time warp: the descriptor with the warp's type and window, the energy of the rows
    (album_energy: once per album set), forward calls that take it with the warp's other arguments, and the backward with
    the warp's parameters and their gradients."""
    _tw, _sep = "_tw", ", "

    def _album_energy(self, rows, WH_W, WC_W):
        assert tuple(rows.shape) == self._rows
        assert WH_W.numel() >= self.w * self.w and WC_W.numel() == self.w
        energy = torch.empty(self._rows[0], self._rows[2], device=self.dev, dtype=torch.float32)
        bf16, rows_ptr = self._rows_arg(rows)
        self._call(self._sym + "_energy" + bf16, rows_ptr, ptr(_f32c(WH_W)), ptr(_f32c(WC_W)), ptr(energy), ptr(self.work))
        return energy

    def forward(self, rows, rows_mask, energy, hq, qmask, lq, index, W, b, WH_b, WC_W, WC_b, want_logits=False, want_scale=False):
        """-> (h_a [NQ,w], a_logits [NQ,K,positions,JQ] | None, scale [NQ,positions] | None); scale is TimeWarp's, per
        question over its positions (T, or the M*JX of its albums laid end to end)"""
        return self._run(False, rows, rows_mask, hq, qmask, index, W, b, want_logits, (energy, lq, WH_b, WC_W, WC_b), want_scale)

    def forward_train(self, rows, rows_mask, energy, hq, qmask, lq, index, W, b, WH_b, WC_W, WC_b, want_logits=False,
                      want_scale=False):
        """forward() -- the same bits -- that leaves in self.saved (allocated on first use) what backward() reads
        (fvta_attn_{shared,pool}_fwd_tw_train; simiMatrix 1-3)"""
        return self._run(True, rows, rows_mask, hq, qmask, index, W, b, want_logits, (energy, lq, WH_b, WC_W, WC_b), want_scale)

    def backward(self, rows, rows_mask, hq, qmask, lq, index, W, b, WH_W, WH_b, WC_W, WC_b, d_h_a, d_rows, d_hq, d_lq, dW, db,
                 dWH_W, dWH_b, dWC_W, dWC_b):
        """After forward_train() with the same arguments: d_rows (the rows' shape: [A,K,T,w], or [P,K,JX,w] -- the sum over
        every (question, slot) that names the album), d_hq [NQ,JQ,w] and d_lq [NQ,w] are overwritten; dW [F], db [1], dWH_W
        (its first w rows, [w,w]), dWH_b [w], dWC_W [w] and dWC_b [1] accumulated into (fvta_attn_{shared,pool}_bwd_tw).
        WH_W: [2w,w] or its first w rows.  Its workspace is allocated on first use."""
        self._begin_backward(rows, rows_mask, hq, qmask, index, d_h_a, d_rows, d_hq, d_lq, dW, db, dWH_W, dWH_b, dWC_W, dWC_b)
        assert tuple(d_lq.shape) == (self.NQ, self.w)
        assert WH_W.numel() >= self.w * self.w and dWH_W.numel() >= self.w * self.w
        assert dWH_b.numel() == self.w and dWC_W.numel() == self.w and dWC_b.numel() == 1
        self._call(self._sym + "_bwd_tw", ptr(_f32c(rows)), ptr(rows_mask), ptr(_f32c(hq)), ptr(qmask), ptr(_f32c(lq)), ptr(index),
                   ptr(_f32c(W)), ptr(b), ptr(_f32c(WH_W)), ptr(_f32c(WH_b)), ptr(_f32c(WC_W)), ptr(_f32c(WC_b)),
                   ptr(_f32c(d_h_a)), ptr(self.saved), ptr(d_rows), ptr(d_hq), ptr(d_lq), ptr(dW), ptr(db), ptr(dWH_W),
                   ptr(dWH_b), ptr(dWC_W), ptr(dWC_b), ptr(self.work_bwd))


class SharedFocalAttention(_AlbumAttention):
    """attention_3d (model_v2.py:210-298) of NQ questions over A albums whose context rows are held ONCE: hinfo [A,K,T,w],
    hmask [A,K,T], hq [NQ,JQ,w], qmask [NQ,JQ], album [NQ] int32 on the device (validate it with check_album_index before
    the upload).  Question i gets FocalAttention's result on album[i]'s rows.  forward() is the inference call
    (fvta_attn_shared_fwd, nothing kept); forward_train() / backward() are the training pair (simiMatrix 1-3), whose
    d_hinfo stays [A,K,T,w]: the sum of the per-question row gradients over each album's questions."""

    def __init__(self, A, NQ, K, T, JQ, w, simi, add_tanh):
        self.A, self.NQ, self.K, self.T, self.JQ, self.w = int(A), int(NQ), int(K), int(T), int(JQ), int(w)
        desc = _lib.AttnSharedDesc(self.A, self.NQ, self.K, self.T, self.JQ, self.w, int(simi), int(bool(add_tanh)))
        self._setup("fvta_attn_shared", "shared attention", desc, (self.A, self.K, self.T, self.w), (self.NQ,), self.T)


# ------------------------------------------------------------------ attention, per-question album lists over one pool
def check_album_lists(albums, P, masked):
    """Host-side validation of per-question album lists, before they are uploaded (the kernels only clamp them): a
    [NQ,M] integer tensor / array, or a list of lists -- ragged lists are padded with -1 (an empty slot) to the longest.
    Every entry lies in [-1, P); -1 needs masked=True (an empty slot is masked rows, and the attention masks only when
    both masks are given).  Returns a contiguous int32 CPU tensor [NQ,M].  Pure host: no GPU, no library."""
    if not torch.is_tensor(albums) and not hasattr(albums, "shape"):
        rows = [list(r) if isinstance(r, (list, tuple)) else r for r in list(albums)]
        if len(rows) == 0:
            raise ValueError("album lists: no question")
        if all(isinstance(r, list) for r in rows):
            M = max(len(r) for r in rows)
            rows = [r + [-1] * (M - len(r)) for r in rows]
        albums = rows
    t = albums if torch.is_tensor(albums) else torch.as_tensor(albums)
    if t.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        if t.numel() == 0:
            raise ValueError("album lists: empty (shape %s)" % (tuple(t.shape),))
        raise ValueError("album lists: an integer dtype is needed, got %s" % t.dtype)
    if t.dim() != 2:
        raise ValueError("album lists: expected two dimensions [NQ,M], got shape %s" % (tuple(t.shape),))
    if t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError("album lists: empty (NQ = %d, M = %d)" % (t.shape[0], t.shape[1]))
    t = t.detach().cpu()
    lo, hi = int(t.min()), int(t.max())
    if lo < -1 or hi >= int(P):
        raise ValueError("album lists: values must lie in [-1, %d) (-1: an empty slot), got [%d, %d]" % (int(P), lo, hi))
    if lo < 0 and not masked:
        raise ValueError("album lists: an empty slot (-1) needs both masks: without them the attention masks nothing, "
                         "and an empty slot is masked rows")
    return t.to(torch.int32).contiguous()


class PooledFocalAttention(_AlbumAttention):
    """attention_3d (model_v2.py:210-298) of NQ questions that each list M albums of ONE pool of P encoded albums: pool
    [P,K,JX,w], pool_mask [P,K,JX], hq [NQ,JQ,w], qmask [NQ,JQ], albums [NQ,M] int32 on the device (validate them with
    check_album_lists before the upload; -1 is an empty slot).  Question i gets FocalAttention's result on its albums' rows
    laid end to end, [K, M*JX, w], which is never built.  forward() is the inference call (fvta_attn_pool_fwd, nothing
    kept); forward_train() / backward() are the training pair (simiMatrix 1-3), whose d_pool stays [P,K,JX,w]: the sum of
    the per-question row gradients over every (question, slot) that refers to the album.
    forward() also takes the pool as a contiguous torch.bfloat16 tensor (fvta_attn_pool_fwd_bf16): half the bytes held
    and read, no fp32 copy made, and the result is forward()'s on pool.float(), bit for bit.  The training pair takes fp32
    rows."""

    def __init__(self, P, NQ, M, K, JX, JQ, w, simi, add_tanh):
        self.P, self.NQ, self.M, self.K, self.JX, self.JQ, self.w = int(P), int(NQ), int(M), int(K), int(JX), int(JQ), int(w)
        desc = _lib.AttnPoolDesc(self.P, self.NQ, self.M, self.K, self.JX, self.JQ, self.w, int(simi), int(bool(add_tanh)))
        self._setup("fvta_attn_pool", "pooled attention", desc, (self.P, self.K, self.JX, self.w), (self.NQ, self.M),
                    self.M * self.JX)


class SharedWarpedFocalAttention(_WarpedAlbumAttention):
    """SharedFocalAttention under the time warp (model_v2.py:953-1009, use_time_warp without use_time_warp_att):
    question i gets FocalAttention's result on TimeWarp's warp of (hinfo[album[i]], lq[i]), from the rows
    [A,K,T,w] as they are held -- the warp is one scalar per (question, position), and the only term of it that reads the
    rows, the energy e [A,T], belongs to the album: album_energy() computes it once per album set, forward() takes it.
    forward_train() / backward() are the training pair (simiMatrix 1-3), whose d_hinfo stays [A,K,T,w]."""

    def __init__(self, A, NQ, K, T, JQ, w, simi, add_tanh, warp_type, window_t=3.0):
        self.A, self.NQ, self.K, self.T, self.JQ, self.w = int(A), int(NQ), int(K), int(T), int(JQ), int(w)
        shape = _lib.AttnSharedDesc(self.A, self.NQ, self.K, self.T, self.JQ, self.w, int(simi), int(bool(add_tanh)))
        self._setup("fvta_attn_shared", "shared attention under the time warp",
                    _lib.AttnSharedTwDesc(shape, int(warp_type), float(window_t)), (self.A, self.K, self.T, self.w), (self.NQ,), self.T)

    def album_energy(self, hinfo, WH_W, WC_W):
        """e [A,T] = sum_k sum_c (WH_W[:w] WC_W)[c] hinfo[a,k,t,c]^2 (fvta_attn_shared_energy): a function of the rows and
        of WH/W, WC/W alone -- keep it as long as those stay what they are.  WH_W [2w,w] or its first w rows, WC_W [w]"""
        return self._album_energy(hinfo, WH_W, WC_W)


class PooledWarpedFocalAttention(_WarpedAlbumAttention):
    """PooledFocalAttention under the time warp (model_v2.py:953-1009, use_time_warp without use_time_warp_att):
    question i gets FocalAttention's result on TimeWarp's warp of (its albums' rows laid end to end, lq[i]),
    from the pool [P,K,JX,w] as it is held -- the warp is one scalar per (question, position t = m*JX + j of its M*JX), and
    the only term of it that reads the rows, the energy e [P,JX], belongs to the pooled album: album_energy() computes it
    once per pool, forward() takes it.  The count of a position runs over the question's whole M*JX positions.
    forward_train() / backward() are the training pair (fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw; simiMatrix
    1-3), whose d_pool stays [P,K,JX,w]: the sum -- the attention's row gradient and the energy's -- over every (question,
    slot) that refers to the album.
    album_energy() and forward() also take the pool as a contiguous torch.bfloat16 tensor (fvta_attn_pool_energy_bf16 /
    fvta_attn_pool_fwd_tw_bf16): no fp32 copy, and the results are those on pool.float(), bit for bit.  The training pair
    takes fp32 rows."""

    def __init__(self, P, NQ, M, K, JX, JQ, w, simi, add_tanh, warp_type, window_t=3.0):
        self.P, self.NQ, self.M, self.K, self.JX, self.JQ, self.w = int(P), int(NQ), int(M), int(K), int(JX), int(JQ), int(w)
        shape = _lib.AttnPoolDesc(self.P, self.NQ, self.M, self.K, self.JX, self.JQ, self.w, int(simi), int(bool(add_tanh)))
        self._setup("fvta_attn_pool", "pooled attention under the time warp",
                    _lib.AttnPoolTwDesc(shape, int(warp_type), float(window_t)), (self.P, self.K, self.JX, self.w),
                    (self.NQ, self.M), self.M * self.JX)

    def album_energy(self, pool, WH_W, WC_W):
        """e [P,JX] = sum_k sum_c (WH_W[:w] WC_W)[c] pool[p,k,j,c]^2 (fvta_attn_pool_energy): a function of the pool and of
        WH/W, WC/W alone -- keep it as long as those stay what they are.  WH_W [2w,w] or its first w rows, WC_W [w]"""
        return self._album_energy(pool, WH_W, WC_W)


def linear_fwd(x, W, b, y, M, din, dout, add_tanh=False, blk=None):
    """y [M,dout] = x [M,din] W [din,dout] + b (+ tanh); blk = (rows_per_blk, blk_stride): x rows in blocks"""
    rpb, bs = blk if blk else (M, 0)
    check(_lib.load().fvta_linear_fwd_blk(ptr(x), ptr(W), ptr(b), ptr(y), M, din, dout, int(add_tanh), rpb, bs, stream_ptr()),
          "fvta_linear_fwd")


def linear_bwd(x, W, y, dy, dx, dW, db, M, din, dout, add_tanh=False, accumulate_dx=False, blk=None):
    """dx = dyt W^T (overwritten / added to), dW += x^T dyt, db += sum dyt; dyt = dy (1 - y^2) under add_tanh"""
    rpb, bs = blk if blk else (M, 0)
    check(_lib.load().fvta_linear_bwd_blk(ptr(x), ptr(W), ptr(y), ptr(dy), ptr(dx), ptr(dW), ptr(db), M, din, dout,
                                          int(add_tanh), int(accumulate_dx), rpb, bs, stream_ptr()), "fvta_linear_bwd")


def softmax_fwd(x, p, rows, J):
    check(_lib.load().fvta_softmax_fwd(ptr(x), ptr(p), rows, J, stream_ptr()), "fvta_softmax_fwd")


def softmax_bwd(p, dp, dx, rows, J):
    check(_lib.load().fvta_softmax_bwd(ptr(p), ptr(dp), ptr(dx), rows, J, stream_ptr()), "fvta_softmax_bwd")


def exp_mask(val, mask, out, n):
    check(_lib.load().fvta_exp_mask(ptr(val), ptr(mask), ptr(out), n, stream_ptr()), "fvta_exp_mask")


def wsum_fwd(target, weights, out, rows, J, d, target_ld=None):
    check(_lib.load().fvta_wsum_fwd_ld(ptr(target), ptr(weights), ptr(out), rows, J, d, J * d if target_ld is None else target_ld,
                                       stream_ptr()), "fvta_wsum_fwd")


def wsum_bwd(target, weights, d_out, d_weights, d_target, rows, J, d, target_ld=None):
    check(_lib.load().fvta_wsum_bwd(ptr(target), ptr(weights), ptr(d_out), ptr(d_weights), ptr(d_target), rows, J, d,
                                    J * d if target_ld is None else target_ld, stream_ptr()), "fvta_wsum_bwd")


def attn_qside_fwd(a_logits, hq, q_a, R, V, JQ, w):
    """q_a [R,w] = mean_v softsel(hq [R,JQ,w], a_logits [R,V,JQ])  (the bidirect branch, model.py:169-177)"""
    check(_lib.load().fvta_attn_qside_fwd(ptr(a_logits), ptr(hq), ptr(q_a), R, V, JQ, w, stream_ptr()), "fvta_attn_qside_fwd")


def attn_qside_bwd(a_logits, hq, d_q_a, dA, d_hq, R, V, JQ, w):
    """dA [R,V,JQ] overwritten, d_hq accumulated"""
    check(_lib.load().fvta_attn_qside_bwd(ptr(a_logits), ptr(hq), ptr(d_q_a), ptr(dA), ptr(d_hq), R, V, JQ, w, stream_ptr()),
          "fvta_attn_qside_bwd")


def rows_reduce(x, out, rows, J, d, out_ld=None, scale=1.0, accumulate=False):
    """out[r, :] (+)= scale * sum_j x[r, j, :]; `out` rows out_ld floats apart (fvta_rows_reduce)"""
    check(_lib.load().fvta_rows_reduce(ptr(x), ptr(out), rows, J, d, d if out_ld is None else out_ld, float(scale),
                                       int(accumulate), stream_ptr()), "fvta_rows_reduce")


def rows_broadcast(v, out, rows, J, d, v_ld=None, scale=1.0, accumulate=False):
    """out[r, j, :] (+)= scale * v[r, :]; `v` rows v_ld floats apart (fvta_rows_broadcast)"""
    check(_lib.load().fvta_rows_broadcast(ptr(v), ptr(out), rows, J, d, d if v_ld is None else v_ld, float(scale),
                                          int(accumulate), stream_ptr()), "fvta_rows_broadcast")


def _focal_logits_bwd(self, hinfo, hq, W, dA, d_hinfo, d_hq, dW, db):
    """dense logit gradient dA [N,T,JQ] of this K = 1 attention -> d_hinfo, d_hq (accumulated), dW, db (accumulated)"""
    if getattr(self, "dense_work", None) is None:
        self.dense_work = _bytes(self.lib.fvta_attn_logits_bwd_workspace_bytes(ctypes.byref(self.desc)), self.dev)
    check(self.lib.fvta_attn_logits_bwd(ctypes.byref(self.desc), ptr(hinfo), ptr(hq), ptr(W), ptr(dA), ptr(d_hinfo), ptr(d_hq),
                                        ptr(dW), ptr(db), ptr(self.dense_work), stream_ptr()), "fvta_attn_logits_bwd")


FocalAttention.logits_bwd = _focal_logits_bwd


def as_mask_u8(m):
    if m is None:
        return None
    return m.to(torch.uint8).contiguous()


# --------------------------------------------------------------------- scorer
def scorer_ce_fwd(gq, g1, gch, W, b, y=None, use_eu_output=False, add_tanh=False):
    lib = _lib.load()
    N, C, w = gch.shape
    desc = ScorerDesc(N, C, w, int(use_eu_output), int(add_tanh), 0)
    logits = torch.empty(N, C, device=gq.device, dtype=torch.float32)
    yp = torch.empty_like(logits)
    loss = torch.zeros(1, device=gq.device, dtype=torch.float32) if y is not None else None
    check(lib.fvta_scorer_ce_fwd(ctypes.byref(desc), ptr(_f32c(gq)), ptr(_f32c(g1)), ptr(_f32c(gch)), ptr(W), ptr(b),
                                 ptr(y), ptr(logits), ptr(yp), ptr(loss), stream_ptr()), "fvta_scorer_ce_fwd")
    return logits, yp, loss


def scorer_ce_bwd(gq, g1, gch, W, b, y, logits, yp, loss_scale, dW, db, use_eu_output=False, add_tanh=False,
                  tf_xent_grad=True):
    """tf_xent_grad: d logits = softmax - labels on every row (TF-1's kernel; all-False label rows still carry
    gradient); False: the gradient of -sum(y log softmax) proper."""
    lib = _lib.load()
    N, C, w = gch.shape
    desc = ScorerDesc(N, C, w, int(use_eu_output), int(add_tanh), 0 if tf_xent_grad else 1)
    dgq, dg1, dgch = torch.empty_like(gq), torch.empty_like(g1), torch.empty_like(gch)
    check(lib.fvta_scorer_ce_bwd(ctypes.byref(desc), ptr(gq), ptr(g1), ptr(gch), ptr(W), ptr(b), ptr(y), ptr(logits),
                                 ptr(yp), float(loss_scale), ptr(dgq), ptr(dg1), ptr(dgch), ptr(dW), ptr(db),
                                 stream_ptr()), "fvta_scorer_ce_bwd")
    return dgq, dg1, dgch


# ----------------------------------------------------------------- optimisers
def adadelta_step(var, grad, accum, accum_update, lr, rho=0.95, eps=1e-8, grad_scale=1.0):
    check(_lib.load().fvta_adadelta_step(ptr(var), ptr(grad), ptr(accum), ptr(accum_update), var.numel(), lr, rho, eps,
                                         grad_scale, stream_ptr()), "fvta_adadelta_step")


def adam_step(var, grad, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    check(_lib.load().fvta_adam_step(ptr(var), ptr(grad), ptr(m), ptr(v), var.numel(), lr, beta1, beta2, eps, int(t),
                                     grad_scale, stream_ptr()), "fvta_adam_step")


# ------------------------------------------------------------ gradient guard
def guard_ctl_new(dev, applied=0, skipped=0):
    """A zeroed control block (fvta_guard_ctl) on `dev` with its running counters preset; a uint8 tensor."""
    host = _lib.GuardCtl(applied=int(applied), skipped=int(skipped))
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)


def guard_ctl_read(ctl):
    """The control block as a dict -- ONE device-to-host copy, which waits for the stream."""
    host = _lib.GuardCtl.from_buffer_copy(ctl.cpu().numpy().tobytes())
    return {name: getattr(host, name) for name, _ in _lib.GuardCtl._fields_}


def grad_guard_workspace(n, dev):
    nbytes = _lib.load().fvta_grad_guard_workspace_bytes(int(n))
    if nbytes == 0:
        check(-1, "fvta_grad_guard_workspace_bytes")
    return _bytes(nbytes, dev)


def grad_guard(grad, ctl, workspace=None, grad_scale=1.0, clip_value=0.0, clip_norm=0.0, skip_nonfinite=False, adam=None):
    """Statistics of the flat gradient and the decision of this step into the device control block `ctl`
    (guard_ctl_new), asynchronously on the current stream; follow it with adadelta_step_guarded / adam_step_guarded.
    grad: 1-D float32, any 4-byte aligned start (a slice is fine).  adam = (lr, beta1, beta2) also computes lr_t."""
    assert grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous(), "expected a contiguous float32 CUDA tensor"
    assert ctl.is_cuda and ctl.dtype == torch.uint8 and ctl.numel() == ctypes.sizeof(_lib.GuardCtl)
    if workspace is None:
        workspace = grad_guard_workspace(grad.numel(), grad.device)
    lr, b1, b2 = adam if adam is not None else (0.0, 0.0, 0.0)
    d = _lib.GuardDesc(float(grad_scale), float(clip_value), float(clip_norm), int(bool(skip_nonfinite)),
                       int(adam is not None), float(lr), float(b1), float(b2))
    check(_lib.load().fvta_grad_guard(ctypes.byref(d), ptr(grad), grad.numel(), ptr(workspace), ptr(ctl), stream_ptr()),
          "fvta_grad_guard")
    return ctl


def adadelta_step_guarded(var, grad, accum, accum_update, ctl, lr, rho=0.95, eps=1e-8):
    check(_lib.load().fvta_adadelta_step_guarded(ptr(var), ptr(grad), ptr(accum), ptr(accum_update), var.numel(), lr, rho,
                                                 eps, ptr(ctl), stream_ptr()), "fvta_adadelta_step_guarded")


def adam_step_guarded(var, grad, m, v, ctl, beta1=0.9, beta2=0.999, eps=1e-8):
    """lr, the step count and the bias correction come from ctl (grad_guard(..., adam=(lr, beta1, beta2)))"""
    check(_lib.load().fvta_adam_step_guarded(ptr(var), ptr(grad), ptr(m), ptr(v), var.numel(), beta1, beta2, eps,
                                             ptr(ctl), stream_ptr()), "fvta_adam_step_guarded")


def weight_decay(var, grad, coef, loss):
    """add_wd (model_v2.py:347-354) for one variable: loss += coef/2 * sum(var^2), grad += coef * var (either may be None)."""
    check(_lib.load().fvta_weight_decay(ptr(var), ptr(grad) if grad is not None else None, var.numel(), float(coef),
                                        ptr(loss) if loss is not None else None, stream_ptr()), "fvta_weight_decay")


# ------------------------------------------------------------ AttentionGRUCell
def attgru_fwd(inputs, state, Wg, bg, Wc, Wi, bi):
    """attention_gru_cell.py:50-70, one step.  inputs [B,d+1] (last column = gate), state [B,d]."""
    lib = _lib.load()
    B, d = state.shape
    new_h = torch.empty_like(state)
    saved = torch.empty(B, 3 * d, device=state.device, dtype=torch.float32)
    check(lib.fvta_attgru_fwd(B, d, ptr(_f32c(inputs)), ptr(_f32c(state)), ptr(_f32c(Wg)), ptr(_f32c(bg)), ptr(_f32c(Wc)),
                              ptr(_f32c(Wi)), ptr(_f32c(bi)), ptr(new_h), ptr(saved), stream_ptr()), "fvta_attgru_fwd")
    return new_h, saved


def attgru_bwd(inputs, state, Wg, Wc, Wi, saved, d_new_h, dWg, dbg, dWc, dWi, dbi):
    """Gradients of one AttentionGRUCell step; parameter gradients are accumulated into."""
    lib = _lib.load()
    B, d = state.shape
    d_inputs = torch.empty_like(inputs)
    d_state = torch.empty_like(state)
    ws = torch.empty(B, 4 * d, device=state.device, dtype=torch.float32)
    check(lib.fvta_attgru_bwd(B, d, ptr(inputs), ptr(state), ptr(Wg), ptr(Wc), ptr(Wi), ptr(saved), ptr(_f32c(d_new_h)),
                              ptr(d_inputs), ptr(d_state), ptr(dWg), ptr(dbg), ptr(dWc), ptr(dWi), ptr(dbi), ptr(ws),
                              stream_ptr()), "fvta_attgru_bwd")
    return d_inputs, d_state


def attgru_seq_plan(N, F, d):
    """How the library runs the AttentionGRU over F facts at this shape (fvta_attgru_seq_plan; a host query, no GPU):
    regime "A" (the whole recurrence in one launch) or "B" (one fused launch per step), kernel launches of a forward and
    of a backward, rows of a workgroup tile."""
    out = (ctypes.c_int32 * 4)()
    check(_lib.load().fvta_attgru_seq_plan(ctypes.byref(AttGruSeqDesc(N, F, d, 1)), out), "fvta_attgru_seq_plan")
    return dict(regime="AB"[out[0]], fwd_launches=out[1], bwd_launches=out[2], row_tile=out[3])


class AttentionGRUSeq:
    """F steps of the AttentionGRUCell with the state carried (dynamic_rnn over the facts, model_dmnplus.py:123-134):
    facts [N,F,d], gate [N,F], h0 [N,d] | None -> h_last [N,d].  training=False keeps nothing (`saved` stays None)."""

    def __init__(self, N, F, d, training=True):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.N, self.F, self.d = int(N), int(F), int(d)
        self.desc = AttGruSeqDesc(self.N, self.F, self.d, int(bool(training)))
        self.saved = None

    def forward(self, facts, gate, h0, Wg, bg, Wc, Wi, bi):
        h_last = torch.empty(self.N, self.d, dtype=torch.float32, device=self.dev)
        work = _sized(self, "fvta_attgru_seq_workspace_bytes", "attgru_seq: ", 0)
        if self.desc.training:
            self.saved = _bytes(self.lib.fvta_attgru_seq_saved_bytes(ctypes.byref(self.desc)), self.dev)
        check(self.lib.fvta_attgru_seq_fwd(ctypes.byref(self.desc), ptr(_f32c(facts)), ptr(_f32c(gate)),
                                           ptr(None if h0 is None else _f32c(h0)), ptr(_f32c(Wg)), ptr(_f32c(bg)),
                                           ptr(_f32c(Wc)), ptr(_f32c(Wi)), ptr(_f32c(bi)), ptr(h_last), ptr(self.saved),
                                           ptr(work), stream_ptr()), "fvta_attgru_seq_fwd")
        return h_last

    def backward(self, facts, gate, Wg, Wc, Wi, d_h_last, d_facts, d_gate, d_h0, dWg, dbg, dWc, dWi, dbi, accumulate=False):
        """d_facts, d_gate, d_h0 (may be None) are overwritten; the parameter gradients stored, or added to under
        `accumulate`.  `saved` is only read: the call may be repeated."""
        if self.saved is None:
            raise _lib.FvtaError("AttentionGRUSeq.backward: no training forward ran")
        work = _sized(self, "fvta_attgru_seq_workspace_bytes", "attgru_seq: ", 1)
        check(self.lib.fvta_attgru_seq_bwd(ctypes.byref(self.desc), ptr(facts), ptr(gate), ptr(Wg), ptr(Wc), ptr(Wi),
                                           ptr(self.saved), ptr(_f32c(d_h_last)), ptr(d_facts), ptr(d_gate), ptr(d_h0),
                                           ptr(dWg), ptr(dbg), ptr(dWc), ptr(dWi), ptr(dbi), int(accumulate), ptr(work),
                                           stream_ptr()), "fvta_attgru_seq_bwd")


def gru_seq_plan(N, T, in_dim, d):
    """How the library runs the GRU over T steps at this shape (fvta_gru_seq_plan; a host query, no GPU): regime "A" (the
    whole recurrence in one launch) or "B" (two fused launches per step), kernel launches of a forward and of a backward,
    rows of a workgroup tile."""
    out = (ctypes.c_int32 * 4)()
    check(_lib.load().fvta_gru_seq_plan(ctypes.byref(GruSeqDesc(N, T, in_dim, d, 0, 1)), out), "fvta_gru_seq_plan")
    return dict(regime="AB"[out[0]], fwd_launches=out[1], bwd_launches=out[2], row_tile=out[3])


def _i32c(t):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), "expected a contiguous int32 CUDA tensor"
    return t


class GRUSeq:
    """TF's GRUCell under dynamic_rnn(sequence_length) (model_dmnplus.py:344-345, 470-471): x [N,T,in_dim], lens int32 [N]
    | None (all T), h0 [N,d] | None -> (out [N,T,d] with padded rows zero, h_last [N,d]); reverse=True is the backward half
    of bidirectional_dynamic_rnn.  training=False keeps nothing (`saved` stays None)."""

    def __init__(self, N, T, in_dim, d, reverse=False, training=True):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.N, self.T, self.in_dim, self.d = int(N), int(T), int(in_dim), int(d)
        self.desc = GruSeqDesc(self.N, self.T, self.in_dim, self.d, int(bool(reverse)), int(bool(training)))
        self.saved = None

    def forward(self, x, lens, h0, Wg, bg, Wc, bc, want_out=True):
        out = torch.empty(self.N, self.T, self.d, dtype=torch.float32, device=self.dev) if want_out else None
        h_last = torch.empty(self.N, self.d, dtype=torch.float32, device=self.dev)
        work = _sized(self, "fvta_gru_seq_workspace_bytes", "gru_seq: ", 0)
        if self.desc.training:
            self.saved = _bytes(self.lib.fvta_gru_seq_saved_bytes(ctypes.byref(self.desc)), self.dev)
        check(self.lib.fvta_gru_seq_fwd(ctypes.byref(self.desc), ptr(_f32c(x)), ptr(None if lens is None else _i32c(lens)),
                                        ptr(None if h0 is None else _f32c(h0)), ptr(_f32c(Wg)), ptr(_f32c(bg)), ptr(_f32c(Wc)),
                                        ptr(_f32c(bc)), ptr(out), ptr(h_last), ptr(self.saved), ptr(work), stream_ptr()),
              "fvta_gru_seq_fwd")
        return out, h_last

    def backward(self, x, lens, Wg, Wc, d_out, d_h_last, d_x, d_h0, dWg, dbg, dWc, dbc, accumulate=False):
        """d_out / d_h_last: either may be None, not both.  d_x, d_h0 (may be None) are overwritten; the parameter
        gradients stored, or added to under `accumulate`.  `saved` is only read: the call may be repeated."""
        if self.saved is None:
            raise _lib.FvtaError("GRUSeq.backward: no training forward ran")
        work = _sized(self, "fvta_gru_seq_workspace_bytes", "gru_seq: ", 1)
        check(self.lib.fvta_gru_seq_bwd(ctypes.byref(self.desc), ptr(x), ptr(lens), ptr(Wg), ptr(Wc), ptr(self.saved),
                                        ptr(None if d_out is None else _f32c(d_out)),
                                        ptr(None if d_h_last is None else _f32c(d_h_last)), ptr(d_x), ptr(d_h0), ptr(dWg),
                                        ptr(dbg), ptr(dWc), ptr(dbc), int(accumulate), ptr(work), stream_ptr()),
              "fvta_gru_seq_bwd")


# ------------------------------------------------------------------ compact bilinear pooling
def count_sketch_tables(d1, d2, D, seeds=(1, 3, 5, 7)):
    """The four count-sketch tables compact_bilinear_pooling_layer draws (model_mcb.py:1313-1326), as numpy arrays
    (h1 [d1], s1 [d1], h2 [d2], s2 [d2]): `np.random.seed(s); np.random.randint(D, size=d)` for the indices and
    `2 * np.random.randint(2, size=d) - 1` for the signs.  np.random.RandomState(s) is that legacy stream and is stable
    across numpy versions, so a checkpoint the reference trained meets the same hash.  A host function: no GPU."""
    import numpy as np
    sh1, ss1, sh2, ss2 = (int(s) for s in seeds)
    draw_h = lambda s, d: np.random.RandomState(s).randint(int(D), size=int(d))
    draw_s = lambda s, d: 2 * np.random.RandomState(s).randint(2, size=int(d)) - 1
    return draw_h(sh1, d1), draw_s(ss1, d1), draw_h(sh2, d2), draw_s(ss2, d2)


def check_sketch_tables(h1, s1, h2, s2, d1, d2, D):
    """Host-side validation of user-supplied tables, before they are uploaded (the kernels trust them): lengths d1 / d2,
    integer indices in [0, D), signs +1 / -1.  Returns them as numpy (int32, float32, int32, float32)."""
    import numpy as np
    out = []
    for name, t, d, is_h in (("rand_h_1", h1, d1, True), ("rand_s_1", s1, d1, False), ("rand_h_2", h2, d2, True),
                             ("rand_s_2", s2, d2, False)):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        if a.ndim != 1 or a.shape[0] != int(d):
            raise ValueError("%s: expected %d entries, got shape %s" % (name, int(d), tuple(a.shape)))
        if is_h:
            if not (np.issubdtype(a.dtype, np.integer) or np.all(a == np.floor(a))):
                raise ValueError("%s: indices must be integers" % name)
            if a.min() < 0 or a.max() >= int(D):
                raise ValueError("%s: indices must lie in [0, %d), got [%d, %d]" % (name, int(D), int(a.min()), int(a.max())))
            out.append(np.ascontiguousarray(a, dtype=np.int32))
        else:
            if not np.all(np.abs(a) == 1):
                raise ValueError("%s: signs must be +1 or -1" % name)
            out.append(np.ascontiguousarray(a, dtype=np.float32))
    return tuple(out)


def upload_sketch_tables(h1, s1, h2, s2, d1, d2, D):
    """validated tables as device tensors (h1 int32, s1 float32, h2 int32, s2 float32)"""
    dev = require_gpu()
    return tuple(torch.from_numpy(a).to(dev) for a in check_sketch_tables(h1, s1, h2, s2, d1, d2, D))


class CompactBilinear:
    """compact_bilinear_pooling_layer without its sum pool (model_mcb.py:1254-1363), optionally with the
    l2_normalize(sqrt|.|) of :645 fused: x [N*P, d1], q [N, d2] (shared by the P rows of its n) -> [N*P, D].  The tables are
    device tensors from upload_sketch_tables (validated there: the kernels trust them).  training=False keeps nothing."""

    def __init__(self, N, P, d1, d2, D, normalize=False, training=True):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.N, self.P, self.d1, self.d2, self.D = int(N), int(P), int(d1), int(d2), int(D)
        self.desc = _lib.CbpDesc(self.N, self.P, self.d1, self.d2, self.D, int(bool(normalize)), int(bool(training)))
        self.saved = None

    def forward(self, x, q, h1, s1, h2, s2):
        work = _sized(self, "fvta_cbp_workspace_bytes", "compact_bilinear: ", 0)
        out = torch.empty(self.N * self.P, self.D, dtype=torch.float32, device=self.dev)
        if self.desc.training:
            self.saved = _bytes(self.lib.fvta_cbp_saved_bytes(ctypes.byref(self.desc)), self.dev)
        check(self.lib.fvta_cbp_fwd(ctypes.byref(self.desc), ptr(_f32c(x)), ptr(_f32c(q)), ptr(_i32c(h1)), ptr(_f32c(s1)),
                                    ptr(_i32c(h2)), ptr(_f32c(s2)), ptr(out), ptr(self.saved), ptr(work), stream_ptr()),
              "fvta_cbp_fwd")
        return out

    def backward(self, x, q, h1, s1, h2, s2, dy, dx, dq, accumulate=False):
        """dx [N*P, d1] / dq [N, d2]: either may be None, not both; stored, or added to under `accumulate`.  `saved` is only
        read: the call may be repeated."""
        if self.saved is None:
            raise _lib.FvtaError("CompactBilinear.backward: no training forward ran")
        work = _sized(self, "fvta_cbp_workspace_bytes", "compact_bilinear: ", 1)
        check(self.lib.fvta_cbp_bwd(ctypes.byref(self.desc), ptr(_f32c(x)), ptr(_f32c(q)), ptr(_i32c(h1)), ptr(_f32c(s1)),
                                    ptr(_i32c(h2)), ptr(_f32c(s2)), ptr(self.saved), ptr(_f32c(dy)), ptr(dx), ptr(dq),
                                    int(accumulate), ptr(work), stream_ptr()), "fvta_cbp_bwd")


# ------------------------------------------------------------------ time warp
class TimeWarp:
    """model_v2.py:953-1009 (closed form): warp_h = hall * c[n,t] * cnt(t)."""

    def __init__(self, N, K, T, w, warp_type, window_t=3.0):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.desc = TimewarpDesc(N, K, T, w, int(warp_type), float(window_t))
        nb = self.lib.fvta_timewarp_workspace_bytes(ctypes.byref(self.desc))
        if nb == 0:
            raise Exception(self.lib.fvta_last_error().decode())     # "time warping type not implemented" (model_v2.py:341)
        self.work = _bytes(nb, self.dev)
        self.c = torch.empty(N, T, device=self.dev, dtype=torch.float32)
        self.scale = torch.empty(N, T, device=self.dev, dtype=torch.float32)

    def forward(self, hall, lq, WH_W, WH_b, WC_W, WC_b, warp_h):
        check(self.lib.fvta_timewarp_fwd(ctypes.byref(self.desc), ptr(_f32c(hall)), ptr(_f32c(lq)), ptr(WH_W), ptr(WH_b),
                                         ptr(WC_W), ptr(WC_b), ptr(_f32c(warp_h)), ptr(self.c), ptr(self.scale),
                                         ptr(self.work), stream_ptr()), "fvta_timewarp_fwd")

    def backward(self, hall, lq, WH_W, WH_b, WC_W, WC_b, d_warp, d_hall, d_lq, dWH_W, dWH_b, dWC_W, dWC_b,
                 d_scale_att=None):
        """d_scale_att [N,T]: the attention's gradient w.r.t. the per-position scale (use_time_warp_att)."""
        check(self.lib.fvta_timewarp_bwd_att(ctypes.byref(self.desc), ptr(hall), ptr(lq), ptr(WH_W), ptr(WH_b), ptr(WC_W),
                                             ptr(WC_b), ptr(self.c), ptr(_f32c(d_warp)), ptr(d_scale_att), ptr(d_hall),
                                             ptr(d_lq), ptr(dWH_W), ptr(dWH_b), ptr(dWC_W), ptr(dWC_b), ptr(self.work),
                                             stream_ptr()), "fvta_timewarp_bwd")


    def forward_shadow(self, table, lq, WH_W, WH_b, WC_W, WC_b, warp_rows):
        """forward() over the encoders' bf16 shadow rows: table int64 [2, N*K*T] (BiLstm.shadow_rows), warp_rows bf16
        [N*K*T, w] receives the warped rows (the focal attention reads them through a table of addresses into it)."""
        check(self.lib.fvta_timewarp_fwd_shadow(ctypes.byref(self.desc), ptr(table), ptr(_f32c(lq)), ptr(WH_W), ptr(WH_b),
                                                ptr(WC_W), ptr(WC_b), ptr(warp_rows), ptr(self.c), ptr(self.scale),
                                                ptr(self.work), stream_ptr()), "fvta_timewarp_fwd_shadow")

    def backward_shadow(self, table, lq, WH_W, WH_b, WC_W, WC_b, d_warp, d_hall, d_lq, dWH_W, dWH_b, dWC_W, dWC_b):
        check(self.lib.fvta_timewarp_bwd_shadow(ctypes.byref(self.desc), ptr(table), ptr(lq), ptr(WH_W), ptr(WH_b), ptr(WC_W),
                                                ptr(WC_b), ptr(self.c), ptr(_f32c(d_warp)), ptr(d_hall), ptr(d_lq),
                                                ptr(dWH_W), ptr(dWH_b), ptr(dWC_W), ptr(dWC_b), ptr(self.work),
                                                stream_ptr()), "fvta_timewarp_bwd_shadow")


# ------------------------------------------------------------ context tensor
def _ptr_table(tensors, K):
    """a HOST array of K device pointers (None -> NULL); the kernels take the pointers by value, nothing is copied"""
    return (ctypes.c_void_p * K)(*[None if t is None else t.data_ptr() for t in tensors])


def _context_desc(N, M, Js, w):
    if not 1 <= len(Js) <= _lib.CTX_KMAX:
        raise ValueError("context_tensor: K must be in 1..%d (got %d)" % (_lib.CTX_KMAX, len(Js)))
    d = _lib.ContextDesc(int(N), len(Js), int(M), int(w))
    for k, J in enumerate(Js):
        d.J[k] = int(J)
    return d


def context_fwd(streams, masks, hall, hall_mask):
    """model_v2.py:863-914: streams[k] [N,M,J_k,w] f32 (masks[k] [N,M,J_k] u8, or masks = hall_mask = None) ->
    hall [N,K,M,JMAX,w], hall_mask [N,K,M,JMAX] u8; every element written once (fvta_context_fwd, one launch)."""
    N, M, _, w = streams[0].shape
    K = len(streams)
    d = _context_desc(N, M, [s.shape[2] for s in streams], w)
    check(_lib.load().fvta_context_fwd(ctypes.byref(d), _ptr_table([_f32c(s) for s in streams], K),
                                       None if masks is None else _ptr_table(masks, K), ptr(_f32c(hall)), ptr(hall_mask),
                                       stream_ptr()), "fvta_context_fwd")


def context_bwd(d_hall, d_streams, N, M, Js, w):
    """d_streams[k] [N,M,J_k,w] <- d_hall[:, k, :, :J_k] (overwritten; a None entry is skipped; fvta_context_bwd)"""
    d = _context_desc(N, M, Js, w)
    check(_lib.load().fvta_context_bwd(ctypes.byref(d), ptr(_f32c(d_hall)), _ptr_table(d_streams, len(Js)), stream_ptr()),
          "fvta_context_bwd")


# ------------------------------------------------------- embedding front-end
class TokenEmbed:
    """model_v2.py:524-620 for all text tokens of a batch: char-CNN + word lookup, rows written at tok_off.

    word_ids [ntok] i32, char_ids [ntok, W] i32 (None without the char-CNN), tok_off [ntok] i64 element offsets."""

    def __init__(self, ntok, W, cdim, cwdim, wdim, VW, VT, VC, height=5):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.desc = EmbedDesc(ntok, W, cdim, cwdim, wdim, VW, VT, VC, height)
        nb = self.lib.fvta_embed_workspace_bytes(ctypes.byref(self.desc))
        if nb == 0:
            raise _lib.FvtaError("embed: " + self.lib.fvta_last_error().decode())
        self.work = _bytes(nb, self.dev)
        self.argpos = torch.empty(max(ntok * cwdim, 1), dtype=torch.uint8, device=self.dev)
        self.cwdim = cwdim

    def set_dropout(self, keep_prob, seed):
        """conv1d's dropout of the gathered char embeddings for the NEXT forward / backward pair (model_v2.py:58-62,
        training only); keep_prob 1.0 switches it off."""
        self.desc.keep_prob = float(keep_prob)
        self.desc.dropout_seed = int(seed) & (2 ** 64 - 1)

    def forward(self, word_ids, char_ids, tok_off, word_emb, fixed_emb, char_emb, filt, bias, x):
        check(self.lib.fvta_embed_fwd(ctypes.byref(self.desc), ptr(word_ids), ptr(char_ids), ptr(tok_off), ptr(word_emb),
                                      ptr(fixed_emb), ptr(char_emb), ptr(filt), ptr(bias), ptr(x), ptr(self.argpos),
                                      stream_ptr()), "fvta_embed_fwd")

    def backward(self, word_ids, char_ids, tok_off, char_emb, filt, dx, d_word_emb, d_char_emb, d_filt, d_bias):
        check(self.lib.fvta_embed_bwd(ctypes.byref(self.desc), ptr(word_ids), ptr(char_ids), ptr(tok_off), ptr(char_emb),
                                      ptr(filt), ptr(self.argpos), ptr(dx), ptr(d_word_emb), ptr(d_char_emb),
                                      ptr(d_filt), ptr(d_bias), ptr(self.work), stream_ptr()), "fvta_embed_bwd")


class ImageTrans:
    """model_v2.py:634-645: photo feature lookup (+ image_trans_linear); rows written at row_off."""

    def __init__(self, M, idim, tdim, add_tanh):
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.desc = ImgTransDesc(M, idim, tdim, int(add_tanh))
        self.work = torch.empty(M * tdim, dtype=torch.float32, device=self.dev)

    def forward(self, pidx, row_off, image_emb_mat, W, b, x):
        check(self.lib.fvta_image_trans_fwd(ctypes.byref(self.desc), ptr(pidx), ptr(row_off), ptr(_f32c(image_emb_mat)),
                                            ptr(W), ptr(b), ptr(x), stream_ptr()), "fvta_image_trans_fwd")

    def backward(self, pidx, row_off, image_emb_mat, x, dx, dW, db):
        check(self.lib.fvta_image_trans_bwd(ctypes.byref(self.desc), ptr(pidx), ptr(row_off), ptr(image_emb_mat), ptr(x),
                                            ptr(dx), ptr(dW), ptr(db), ptr(self.work), stream_ptr()),
              "fvta_image_trans_bwd")
