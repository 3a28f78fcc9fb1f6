"""torch.autograd over the C ABI: one `torch.autograd.Function` per op of the functional surface and of the encoders.

Forward and backward are each one (or a few) calls into libfvta_hip.so; no arithmetic happens in Python.  Every Function
is `once_differentiable` (no double backward).  Rules that hold for all of them:

  * tensors are contiguous fp32 CUDA tensors with the channel widths the kernels accept -- zero padding and un-padding
    stay OUTSIDE, as ordinary differentiable torch ops (functional.py, nn.py);
  * a Function may be applied several times before one `backward()` (the reference runs one text cell over five
    streams): whatever the forward leaves for the backward (`saved`, plans) belongs to that call alone;
  * when no input requires grad the same kernels run, nothing is kept, the outputs are bit-identical;
  * parameter gradients are accumulated by the kernels into fresh zero buffers, autograd sums them across calls.

Deviations from TensorFlow's gradients that carry over from the model's backward kernels, on the
`h_a` path of the focal attention and on attention_keeprank1's per-(n,m) vectors (fvta_attn_bwd_u, the same kernels): an
exact tie in the max over the question goes to the FIRST arg-max (TF splits it), and a fully masked (n,k) row list sends
no gradient into its logits.  The `a_logits` path (fvta_attn_cube_bwd) is the plain dense gradient; the additive mask
lets it through to masked entries, as in TF.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import BF16, BF16X3, F32, check, ptr, stream_ptr

_PRECISIONS = {"f32": F32, "bf16": BF16, "bf16x3": BF16X3, F32: F32, BF16: BF16, BF16X3: BF16X3}


def _c(t):
    return None if t is None else t.contiguous()


# ------------------------------------------------------------------ small ops
class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        out = torch.empty_like(logits)
        J = logits.shape[-1]
        check(_lib.load().fvta_softmax_fwd(ptr(logits), ptr(out), logits.numel() // J, J, stream_ptr()), "fvta_softmax_fwd")
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, = ctx.saved_tensors
        dx = torch.empty_like(p)
        ops.softmax_bwd(p, _c(g), dx, p.numel() // p.shape[-1], p.shape[-1])
        return dx


class _Softsel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target, logits):
        J, d = target.shape[-2], target.shape[-1]
        out = torch.empty(*target.shape[:-2], d, dtype=torch.float32, device=target.device)
        check(_lib.load().fvta_softsel_fwd(ptr(target), ptr(logits), ptr(out), logits.numel() // J, J, d, stream_ptr()),
              "fvta_softsel_fwd")
        ctx.save_for_backward(target, logits)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        target, logits = ctx.saved_tensors
        J, d = target.shape[-2], target.shape[-1]
        dt = torch.empty_like(target) if ctx.needs_input_grad[0] else None
        dl = torch.empty_like(logits) if ctx.needs_input_grad[1] else None
        check(_lib.load().fvta_softsel_bwd(ptr(target), ptr(logits), ptr(_c(g)), ptr(dt), ptr(dl), logits.numel() // J, J, d,
                                           stream_ptr()), "fvta_softsel_bwd")
        return dt, dl


class _ExpMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, mask_u8):
        out = torch.empty_like(val)
        check(_lib.load().fvta_exp_mask(ptr(val), ptr(mask_u8), ptr(out), val.numel(), stream_ptr()), "fvta_exp_mask")
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return g, None          # the mask is additive (utils.py:210-213)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, add_tanh):
        din, dout = W.shape
        y = torch.empty(*x.shape[:-1], dout, dtype=torch.float32, device=x.device)
        check(_lib.load().fvta_linear_fwd(ptr(x), ptr(W), ptr(b), ptr(y), x.numel() // din, din, dout, int(add_tanh),
                                          stream_ptr()), "fvta_linear_fwd")
        ctx.add_tanh = bool(add_tanh)
        ctx.has_b = b is not None
        ctx.save_for_backward(x, W, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W, y = ctx.saved_tensors
        din, dout = W.shape
        need_x, need_W, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dW = torch.zeros_like(W) if (need_W or need_b) else None
        db = torch.zeros(dout, dtype=torch.float32, device=x.device) if (ctx.has_b and dW is not None) else None
        ops.linear_bwd(x, W, y, _c(g), dx, dW, db, x.numel() // din, din, dout, add_tanh=ctx.add_tanh)
        return dx, (dW if need_W else None), (db if need_b else None), None


class _Wsum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target, weights):
        rows, J, d = target.shape
        out = torch.empty(rows, d, dtype=torch.float32, device=target.device)
        check(_lib.load().fvta_wsum_fwd(ptr(target), ptr(weights), ptr(out), rows, J, d, stream_ptr()), "fvta_wsum_fwd")
        ctx.save_for_backward(target, weights)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        target, weights = ctx.saved_tensors
        rows, J, d = target.shape
        dt = torch.zeros_like(target) if ctx.needs_input_grad[0] else None       # fvta_wsum_bwd adds into d_target
        dw = torch.empty_like(weights) if ctx.needs_input_grad[1] else None
        ops.wsum_bwd(target, weights, _c(g), dw, dt, rows, J, d)
        return dt, dw


def softmax(logits):
    return _Softmax.apply(logits)


def softsel(target, logits):
    return _Softsel.apply(target, logits)


def exp_mask(val, mask_u8):
    return _ExpMask.apply(val, mask_u8)


def linear(x, W, b, add_tanh=False):
    """x [..., in] (contiguous), W [in, out], b [out] or None"""
    return _Linear.apply(x, W, b, bool(add_tanh))


def wsum(target, weights):
    return _Wsum.apply(target, weights)


# ------------------------------------------------------------ focal attention
class _FocalAttention(torch.autograd.Function):
    """(hinfo [N,K,T,w], hq [N,JQ,w], W [F*w] | None, b [1] | None, tscale [N,T] | None; masks u8 | None) ->
    (h_a [N,w], a_logits [N,K,T,JQ]).  Each call owns its handle and with it the `saved` buffer."""

    @staticmethod
    def forward(ctx, hinfo, hq, W, b, tscale, hmask, qmask, simi, add_tanh, feat_order):
        N, K, T, w = hinfo.shape
        op = ops.FocalAttention(N, K, T, hq.shape[1], w, simi, add_tanh, feat_order=feat_order)
        h_a, a = op.forward(hinfo, hq, hmask, qmask, W, b, want_logits=True, tscale=tscale)
        ctx.set_materialize_grads(False)
        ctx.op = op
        ctx.masks = (hmask, qmask)
        ctx.save_for_backward(hinfo, hq, W, b, tscale)
        return h_a, a

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ha, g_a):
        none = (None,) * 10
        if g_ha is None and g_a is None:
            return none
        hinfo, hq, W, b, tscale = ctx.saved_tensors
        hmask, qmask = ctx.masks
        op = ctx.op
        if g_a is not None and op.desc.simi == 4:
            raise NotImplementedError("attention: no gradient of a_logits under simiMatrix 4 (the cosine cube has no "
                                      "backward kernel); the h_a gradient is available")
        dh, dq = torch.empty_like(hinfo), torch.empty_like(hq)
        dW = torch.zeros_like(W) if W is not None else None
        db = torch.zeros_like(b) if b is not None else None
        dts = torch.zeros_like(tscale) if tscale is not None else None
        if g_ha is not None:
            op.backward(hinfo, hq, hmask, qmask, W, b, _c(g_ha), dh, dq, dW, db, 0, tscale=tscale, d_tscale=dts)
        if g_a is not None:
            r = ctypes.byref(op.desc)
            work = ops._bytes(op.lib.fvta_attn_cube_bwd_workspace_bytes(r), op.dev)
            check(op.lib.fvta_attn_cube_bwd(r, ptr(hinfo), ptr(hq), ptr(W), ptr(b), ptr(_c(g_a)), ptr(dh), ptr(dq), ptr(dW),
                                            ptr(db), 0 if g_ha is None else 1, ptr(work), stream_ptr()), "fvta_attn_cube_bwd")
        need = ctx.needs_input_grad
        return (dh if need[0] else None, dq if need[1] else None, dW if need[2] else None, db if need[3] else None,
                dts if need[4] else None) + (None,) * 5


def focal_attention(hinfo, hq, W, b, hmask=None, qmask=None, simi=1, add_tanh=False, feat_order=0, tscale=None):
    return _FocalAttention.apply(hinfo, hq, W, b, tscale, hmask, qmask, int(simi), bool(add_tanh), int(feat_order))


class _AlbumFocalAttention(torch.autograd.Function):
    """The focal attention over context rows held once (simiMatrix 1-3), by the static word `pooled`:
    False  (hinfo [A,K,T,w], hq [NQ,JQ,w], album int32 [NQ] on the device, W [F*w], b [1]; masks u8 | None) ->
           (h_a [NQ,w], a_logits [NQ,K,T,JQ]): question i over album[i]'s rows (fvta_attn_shared_fwd_train /
           fvta_attn_shared_bwd)
    True   (pool [P,K,JX,w], hq, albums int32 [NQ,M] on the device, ...) -> (h_a, a_logits [NQ,K,M*JX,JQ]): question i over
           its albums' rows laid end to end (fvta_attn_pool_fwd_train / fvta_attn_pool_bwd).  The gradient of pool stays
           [P,K,JX,w]: the sum over every (question, slot) that refers to the album.
    a_logits is not differentiable here.  Each call owns its handle."""

    @staticmethod
    def forward(ctx, rows, hq, index, W, b, rows_mask, qmask, simi, add_tanh, pooled):
        A, K, T, w = rows.shape
        if pooled:
            op = ops.PooledFocalAttention(A, hq.shape[0], index.shape[1], K, T, hq.shape[1], w, simi, add_tanh)
        else:
            op = ops.SharedFocalAttention(A, hq.shape[0], K, T, hq.shape[1], w, simi, add_tanh)
        h_a, a = op.forward_train(rows, rows_mask, hq, qmask, index, W, b, want_logits=True)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(a)
        ctx.op = op
        ctx.aux = (index, rows_mask, qmask)
        ctx.save_for_backward(rows, hq, W, b)
        return h_a, a

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ha, g_a):
        if g_ha is None:
            return (None,) * 10
        rows, hq, W, b = ctx.saved_tensors
        index, rows_mask, qmask = ctx.aux
        dr, dq = torch.empty_like(rows), torch.empty_like(hq)
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        ctx.op.backward(rows, rows_mask, hq, qmask, index, W, b, _c(g_ha), dr, dq, dW, db)
        need = ctx.needs_input_grad
        return (dr if need[0] else None, dq if need[1] else None, None, dW if need[3] else None, db if need[4] else None,
                None, None, None, None, None)


def shared_focal_attention(hinfo, hq, album, W, b, hmask=None, qmask=None, simi=1, add_tanh=False):
    """album: int32 [NQ] on the device, validated by the caller (ops.check_album_index)"""
    if int(simi) == 4:
        raise NotImplementedError("shared_focal_attention: simiMatrix 4 has no shared-context backward; the per-question "
                                  "focal_attention on gathered rows covers it")
    return _AlbumFocalAttention.apply(hinfo, hq, album, W, b, hmask, qmask, int(simi), bool(add_tanh), False)


def pooled_focal_attention(pool, hq, albums, W, b, pool_mask=None, qmask=None, simi=1, add_tanh=False):
    """albums: int32 [NQ,M] on the device, validated by the caller (ops.check_album_lists)"""
    if int(simi) == 4:
        raise NotImplementedError("pooled_focal_attention: simiMatrix 4 has no pooled backward; the per-question "
                                  "focal_attention on gathered rows covers it")
    return _AlbumFocalAttention.apply(_c(pool), _c(hq), albums, _c(W), _c(b), pool_mask, qmask, int(simi), bool(add_tanh), True)


class _AlbumWarpedFocalAttention(torch.autograd.Function):
    """_AlbumFocalAttention under the time warp (simiMatrix 1-3), by the same static word `pooled`:
    False  (hinfo [A,K,T,w], hq [NQ,JQ,w], lq [NQ,w], album int32 [NQ] on the device, W [F*w], b [1], WH_W [2w,w] or its
           first w rows, WH_b [w], WC_W [w], WC_b [1]; masks u8 | None; energy [A,T] | None) -> (h_a [NQ,w], a_logits
           [NQ,K,T,JQ], scale [NQ,T])  (fvta_attn_shared_fwd_tw_train / fvta_attn_shared_bwd_tw)
    True   (pool [P,K,JX,w], hq, lq, albums int32 [NQ,M] on the device, ...; energy [P,JX] | None) -> (h_a, a_logits
           [NQ,K,M*JX,JQ], scale [NQ,M*JX])  (fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw).  The gradient of pool
           stays [P,K,JX,w]: the sum over every (question, slot) that refers to the album.
    a_logits and scale are not differentiable.  `energy` is a cached value of the forward alone: the gradient through e
    reaches the rows, WH_W and WC_W whether it was given or computed here."""

    @staticmethod
    def forward(ctx, rows, hq, lq, index, W, b, WH_W, WH_b, WC_W, WC_b, rows_mask, qmask, simi, add_tanh, warp_type, window_t,
                energy, pooled):
        A, K, T, w = rows.shape
        if pooled:
            op = ops.PooledWarpedFocalAttention(A, hq.shape[0], index.shape[1], K, T, hq.shape[1], w, simi, add_tanh, warp_type,
                                                window_t)
        else:
            op = ops.SharedWarpedFocalAttention(A, hq.shape[0], K, T, hq.shape[1], w, simi, add_tanh, warp_type, window_t)
        if energy is None:
            energy = op.album_energy(rows, WH_W, WC_W)
        h_a, a, scale = op.forward_train(rows, rows_mask, energy, hq, qmask, lq, index, W, b, WH_b, WC_W, WC_b, want_logits=True,
                                         want_scale=True)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(a, scale)
        ctx.op = op
        ctx.aux = (index, rows_mask, qmask)
        ctx.save_for_backward(rows, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b)
        return h_a, a, scale

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ha, g_a, g_scale):
        if g_ha is None:
            return (None,) * 18
        rows, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b = ctx.saved_tensors
        index, rows_mask, qmask = ctx.aux
        dh, dq, dlq = torch.empty_like(rows), torch.empty_like(hq), torch.empty_like(lq)   # overwritten
        dW, db, dWH_W, dWH_b, dWC_W, dWC_b = (torch.zeros_like(t) for t in (W, b, WH_W, WH_b, WC_W, WC_b))
        ctx.op.backward(rows, rows_mask, hq, qmask, lq, index, W, b, WH_W, WH_b, WC_W, WC_b, _c(g_ha), dh, dq, dlq, dW, db, dWH_W,
                        dWH_b, dWC_W, dWC_b)
        need = ctx.needs_input_grad
        grads = (dh, dq, dlq, None, dW, db, dWH_W, dWH_b, dWC_W, dWC_b)
        return tuple(g if n else None for g, n in zip(grads, need[:10])) + (None,) * 8


def _warped_apply(pooled, rows, hq, lq, index, W, b, WH_W, WH_b, WC_W, WC_b, rows_mask, qmask, simi, add_tanh, warp_type, window_t,
                  energy):
    f = lambda t: t.to(torch.float32).contiguous()
    return _AlbumWarpedFocalAttention.apply(f(rows), f(hq), f(lq), index, f(W), f(b), f(WH_W), f(WH_b), f(WC_W).reshape(-1),
                                            f(WC_b).reshape(-1), rows_mask, qmask, int(simi), bool(add_tanh), int(warp_type),
                                            float(window_t), None if energy is None else f(energy.detach()), pooled)


def shared_warped_focal_attention(hinfo, hq, lq, album, W, b, WH_W, WH_b, WC_W, WC_b, hmask=None, qmask=None, simi=1,
                                  add_tanh=False, warp_type=1, window_t=3.0, energy=None):
    """album: int32 [NQ] on the device, validated by the caller (ops.check_album_index); WC_W [w] (or [w,1]), WC_b [1];
    the width is the kernels' (functional.attention_3d_shared_warped_raw pads any)"""
    if int(simi) == 4:
        raise NotImplementedError("shared_warped_focal_attention: simiMatrix 4 has no shared-context backward; the "
                                  "per-question time_warp + focal_attention on gathered rows cover it")
    return _warped_apply(False, hinfo, hq, lq, album, W, b, WH_W, WH_b, WC_W, WC_b, hmask, qmask, simi, add_tanh, warp_type,
                         window_t, energy)


def pooled_warped_focal_attention(pool, hq, lq, albums, W, b, WH_W, WH_b, WC_W, WC_b, pool_mask=None, qmask=None, simi=1,
                                  add_tanh=False, warp_type=1, window_t=3.0, energy=None):
    """albums: int32 [NQ,M] on the device, validated by the caller (ops.check_album_lists); energy [P,JX] | None; the rest
    as shared_warped_focal_attention (functional.attention_3d_pooled_warped_raw pads any width)"""
    if int(simi) == 4:
        raise NotImplementedError("pooled_warped_focal_attention: simiMatrix 4 has no pooled backward; the per-question "
                                  "time_warp + focal_attention on gathered rows cover it")
    return _warped_apply(True, pool, hq, lq, albums, W, b, WH_W, WH_b, WC_W, WC_b, pool_mask, qmask, simi, add_tanh, warp_type,
                         window_t, energy)


class _KeepRank1(torch.autograd.Function):
    """attention_keeprank1 (model.py:247-314): (hinfo [N,M,V,w], hq [N,JQ,w], W [F*w], b [1]; masks u8 | None) ->
    (u [N,M,w], a_logits [N,M,V,JQ] | None).  Forward: fvta_attn_fwd at K = M in model.py's feature order, then the
    per-(n,m) softsel result read out of `saved` (fvta_attn_read_u); the logits cube only when `want_logits` (the bidirect
    branch) -- asking for it selects the general forward kernel, so the flag keeps `u` what it has always been.
    Backward: fvta_attn_bwd_u for g_u, fvta_attn_cube_bwd at K = M for g_a (on top when both are present).
    fvta_attn_bwd_u takes N * M <= 65535 (a larger batch that requires grad is refused in the forward) and its workspace,
    allocated in backward(), holds one dQs slab set per (n,m): N M bsplit (256 / min(w/4, 256)) 32 ceil(JQ/32) w floats
    (136 MB at N M = 1040, w = 64)."""

    @staticmethod
    def forward(ctx, hinfo, hq, W, b, hmask, qmask, simi, want_logits):
        N, M, V, w = hinfo.shape
        op = ops.FocalAttention(N, M, V, hq.shape[1], w, simi, False, feat_order=1)
        _, a = op.forward(hinfo, hq, hmask, qmask, W, b, want_logits=want_logits)
        u = op.read_u()
        ctx.set_materialize_grads(False)
        if any(ctx.needs_input_grad):
            # what fvta_attn_bwd_u does not cover (N * M > 65535) is refused here, not in backward()
            if op.lib.fvta_attn_bwd_u_workspace_bytes(ctypes.byref(op.desc)) == 0:
                raise _lib.FvtaError("attention_keeprank1: " + op.lib.fvta_last_error().decode())
            ctx.op = op
            ctx.masks = (hmask, qmask)
            ctx.save_for_backward(hinfo, hq, W, b)
        return u, a

    @staticmethod
    @once_differentiable
    def backward(ctx, g_u, g_a):
        none = (None,) * 8
        if g_u is None and g_a is None:
            return none
        hinfo, hq, W, b = ctx.saved_tensors
        hmask, qmask = ctx.masks
        op = ctx.op
        dh, dq = torch.empty_like(hinfo), torch.empty_like(hq)
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        if g_u is not None:
            op.backward_u(hinfo, hq, hmask, qmask, W, b, _c(g_u), dh, dq, dW, db, 0)
        if g_a is not None:
            r = ctypes.byref(op.desc)
            work = ops._bytes(op.lib.fvta_attn_cube_bwd_workspace_bytes(r), op.dev)
            check(op.lib.fvta_attn_cube_bwd(r, ptr(hinfo), ptr(hq), ptr(W), ptr(b), ptr(_c(g_a)), ptr(dh), ptr(dq), ptr(dW),
                                            ptr(db), 0 if g_u is None else 1, ptr(work), stream_ptr()), "fvta_attn_cube_bwd")
        need = ctx.needs_input_grad
        return (dh if need[0] else None, dq if need[1] else None, dW if need[2] else None, db if need[3] else None) + (None,) * 4


def keeprank1(hinfo, hq, W, b, hmask=None, qmask=None, simi=1, want_logits=False):
    return _KeepRank1.apply(hinfo, hq, W, b, hmask, qmask, int(simi), bool(want_logits))


class _AttnQSide(torch.autograd.Function):
    """q_a [R,w] = mean_v softsel(hq[r], a_logits[r,v,:]) (the `bidirect` half, model_v2.py:184-188).  Forward: the three
    launches functional._bidirect_q_a has always made (softmax over JQ, the mean over V of the weights, the weighted sum of
    the question), so results do not depend on whether a gradient is wanted; backward: fvta_attn_qside_bwd (JQ <= 64,
    V * JQ <= 8192).  The logit gradient it returns reaches hinfo, hq, W, b through fvta_attn_cube_bwd."""

    @staticmethod
    def forward(ctx, a_logits, hq):
        R, V, JQ = a_logits.shape
        p = _Softmax.apply(a_logits)
        pbar = _Wsum.apply(p, torch.full((R, V), 1.0 / V, dtype=torch.float32, device=p.device))
        ctx.save_for_backward(a_logits, hq)
        return _Wsum.apply(hq, pbar)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a_logits, hq = ctx.saved_tensors
        R, V, JQ = a_logits.shape
        dA = torch.empty_like(a_logits)
        dq = torch.zeros_like(hq)                       # fvta_attn_qside_bwd adds into d_hq
        ops.attn_qside_bwd(a_logits, hq, _c(g), dA, dq, R, V, JQ, hq.shape[-1])
        return (dA if ctx.needs_input_grad[0] else None), (dq if ctx.needs_input_grad[1] else None)


def attn_qside(a_logits, hq):
    return _AttnQSide.apply(a_logits, hq)


# -------------------------------------------------------------------- bi-LSTM
class _BiLstm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens, kernel_fw, bias_fw, kernel_bw, bias_bw, precision):
        B, J, din = x.shape
        d = kernel_fw.shape[1] // 4
        train = any(ctx.needs_input_grad)               # the descriptor keeps gate activations only when a gradient is needed
        ar = torch.arange(B, dtype=torch.int64)
        op = ops.BiLstm(B, J, din, d, ar * J * din, ar * J * 2 * d, torch.full((B,), J, dtype=torch.int32), 2 * d,
                        share_fw_bw=kernel_bw is None, precision=precision, training=train)
        op.make_plan(lens)
        out = torch.empty(B, J, 2 * d, device=x.device, dtype=torch.float32)
        op.forward(x, out, kernel_fw, bias_fw, kernel_bw, bias_bw)
        last = torch.empty(B, 2 * d, device=x.device, dtype=torch.float32)
        op.last_state(out, 0, B, last)
        ctx.set_materialize_grads(False)
        if train:
            ctx.op = op
            ctx.save_for_backward(x, out, kernel_fw, kernel_bw)
        return out, last

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_last):
        none = (None,) * 7
        if g_out is None and g_last is None:
            return none
        x, out, kernel_fw, kernel_bw = ctx.saved_tensors
        op = ctx.op
        d_out = g_out.contiguous().clone() if g_out is not None else torch.zeros_like(out)
        if g_last is not None:
            op.last_state_bwd(_c(g_last), 0, op.B, d_out)
        need = ctx.needs_input_grad
        dx = torch.zeros_like(x) if need[0] else None
        dk_fw = torch.zeros_like(kernel_fw)
        db_fw = torch.zeros(kernel_fw.shape[1], dtype=torch.float32, device=x.device)
        dk_bw = torch.zeros_like(kernel_bw) if kernel_bw is not None else None
        db_bw = torch.zeros_like(db_fw) if kernel_bw is not None else None
        op.backward(x, out, d_out, kernel_fw, kernel_bw, dx, dk_fw, db_fw, dk_bw, db_bw)
        return (dx, None, dk_fw if need[2] else None, db_fw if need[3] else None,
                dk_bw if kernel_bw is not None and need[4] else None, db_bw if kernel_bw is not None and need[5] else None, None)


def bilstm(x, lens, kernel_fw, bias_fw, kernel_bw=None, bias_bw=None, precision="f32"):
    """model_v2.py:652-661, 694-823: x [B,J,in] dense, lens [B] -> (out [B,J,2d] with rows t >= len zeroed, last [B,2d] =
    concat(fw h at len-1, bw h at 0)).  kernel [in+d, 4d] gate order i,j,f,o, bias [4d]; in % 4 == 0, d % 32 == 0
    (nn.BiLSTMEncoder pads any size).  Without kernel_bw both directions share the cell.  Either output's gradient may be
    absent."""
    if precision not in _PRECISIONS:
        raise ValueError("bilstm: precision %r (f32 | bf16 | bf16x3)" % (precision,))
    ops.require_gpu()
    f = lambda t: None if t is None else t.to(torch.float32).contiguous()
    return _BiLstm.apply(f(x), lens.to(torch.int32), f(kernel_fw), f(bias_fw), f(kernel_bw), f(bias_bw),
                         _PRECISIONS[precision])


# --------------------------------------------------------------------- scorer
class _ScorerCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gq, g1, gch, W, b, y, use_eu_output, add_tanh, tf_xent_grad):
        logits, yp, loss = ops.scorer_ce_fwd(gq, g1, gch, W, b, y, use_eu_output=use_eu_output, add_tanh=add_tanh)
        ctx.flags = (use_eu_output, add_tanh, tf_xent_grad)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(logits, yp)
        ctx.save_for_backward(gq, g1, gch, W, b, y, logits, yp)
        return loss.reshape(()), logits, yp

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_logits, _g_yp):
        if g_loss is None:
            return (None,) * 9
        gq, g1, gch, W, b, y, logits, yp = ctx.saved_tensors
        eu, tanh, tfg = ctx.flags
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        dgq, dg1, dgch = ops.scorer_ce_bwd(gq, g1, gch, W, b, y, logits, yp, 1.0, dW, db, use_eu_output=eu, add_tanh=tanh,
                                           tf_xent_grad=tfg)
        # d loss arrives as a device scalar; fvta_scorer_ce_bwd takes its scale from the host, so the kernel runs at 1 and
        # the five results are scaled here (no host sync)
        need = ctx.needs_input_grad
        outs = [t * g_loss if n else None for t, n in zip((dgq, dg1, dgch, dW, db), need[:5])]
        return tuple(outs) + (None,) * 4


def scorer_ce(gq, g1, gch, W, b, y, use_eu_output=False, add_tanh=False, tf_xent_grad=True):
    """model_v2.py:1053-1096: gq, g1 [N,w], gch [N,C,w], W [5w] (7w with use_eu_output), b [1], y [N,C] labels ->
    (loss scalar, logits [N,C], yp [N,C]); only `loss` is differentiable.  tf_xent_grad: TF-1's cross-entropy gradient
    (softmax - labels on every row, all-False label rows included); False: the gradient of the loss as a function."""
    ops.require_gpu()
    f = lambda t: t.to(torch.float32).contiguous()
    return _ScorerCE.apply(f(gq), f(g1), f(gch), f(W).reshape(-1), f(b), ops.as_mask_u8(y), bool(use_eu_output),
                           bool(add_tanh), bool(tf_xent_grad))


# ------------------------------------------------------------- context tensor
class _ContextTensor(torch.autograd.Function):
    """(K, streams[0..K) [N,M,J_k,w], then masks[0..K) u8 [N,M,J_k] or nothing) -> (hall [N,K,M,JMAX,w], hall_mask
    [N,K,M,JMAX] bool | None): model_v2.py:863-914, one fvta_context_fwd.  The backward is the slice back, one
    fvta_context_bwd, only into the streams that need a gradient."""

    @staticmethod
    def forward(ctx, K, *tensors):
        streams, masks = tensors[:K], (tensors[K:] or None)
        N, M, _, w = streams[0].shape
        Js = [s.shape[2] for s in streams]
        hall = torch.empty(N, K, M, max(Js), w, dtype=torch.float32, device=streams[0].device)
        hall_mask = torch.empty(N, K, M, max(Js), dtype=torch.bool, device=hall.device) if masks else None
        ops.context_fwd(streams, masks, hall, hall_mask)
        ctx.dims = (N, M, Js, w)
        ctx.set_materialize_grads(False)
        if hall_mask is not None:
            ctx.mark_non_differentiable(hall_mask)
        return hall, hall_mask

    @staticmethod
    @once_differentiable
    def backward(ctx, g_hall, _g_mask):
        N, M, Js, w = ctx.dims
        K = len(Js)
        if g_hall is None:
            return (None,) * len(ctx.needs_input_grad)
        need = ctx.needs_input_grad[1:1 + K]
        ds = [torch.empty(N, M, J, w, dtype=torch.float32, device=g_hall.device) if n else None for J, n in zip(Js, need)]
        if any(need):
            ops.context_bwd(_c(g_hall), ds, N, M, Js, w)
        return (None,) + tuple(ds) + (None,) * (len(ctx.needs_input_grad) - 1 - K)


def context_tensor(streams, masks=None):
    """streams: K contiguous fp32 [N,M,J_k,w]; masks: K u8 [N,M,J_k] or None -> (hall, hall_mask bool | None)"""
    K = len(streams)
    return _ContextTensor.apply(K, *streams, *(masks or ()))


# ------------------------------------------------------------------ time warp
class _TimeWarp(torch.autograd.Function):
    """(hall [N,K,T,w], lq [N,w], WH_W [2w,w], WH_b [w], WC_W [w], WC_b [1]; warp_type, window_t) -> (warp_h [N,K,T,w],
    scale [N,T] = c[n,t] cnt(t)): model_v2.py:953-1009 in the closed form of SURVEY 3.4.  Each call owns its ops.TimeWarp
    and with it the saved c.  Backward: fvta_timewarp_bwd_att (g_scale = the attention's d_tscale under time_warp_att)."""

    @staticmethod
    def forward(ctx, hall, lq, WH_W, WH_b, WC_W, WC_b, warp_type, window_t):
        N, K, T, w = hall.shape
        op = ops.TimeWarp(N, K, T, w, warp_type, window_t)
        warp_h = torch.empty_like(hall)
        op.forward(hall, lq, WH_W, WH_b, WC_W, WC_b, warp_h)
        ctx.set_materialize_grads(False)
        if any(ctx.needs_input_grad):
            ctx.op = op
            ctx.save_for_backward(hall, lq, WH_W, WH_b, WC_W, WC_b)
        return warp_h, op.scale

    @staticmethod
    @once_differentiable
    def backward(ctx, g_warp, g_scale):
        if g_warp is None and g_scale is None:
            return (None,) * 8
        hall, lq, WH_W, WH_b, WC_W, WC_b = ctx.saved_tensors
        g_warp = torch.zeros_like(hall) if g_warp is None else _c(g_warp)
        d_hall = torch.empty_like(hall)                 # overwritten; the rest is accumulated into
        d_lq, dWH_W, dWH_b, dWC_W, dWC_b = (torch.zeros_like(t) for t in (lq, WH_W, WH_b, WC_W, WC_b))
        ctx.op.backward(hall, lq, WH_W, WH_b, WC_W, WC_b, g_warp, d_hall, d_lq, dWH_W, dWH_b, dWC_W, dWC_b,
                        d_scale_att=_c(g_scale))
        need = ctx.needs_input_grad
        return tuple(t if n else None for t, n in zip((d_hall, d_lq, dWH_W, dWH_b, dWC_W, dWC_b), need[:6])) + (None, None)


def time_warp(hall, lq, WH_W, WH_b, WC_W, WC_b, warp_type=1, window_t=3.0):
    """hall [N,K,T,w] (w % 4 == 0; functional.time_warp pads any width), lq [N,w], WH_W [2w,w], WH_b [w], WC_W [w] (or
    [w,1]), WC_b [1] -> (warp_h, scale [N,T]).  window_t gets no gradient (tf.ceil, model_v2.py:335)."""
    ops.require_gpu()
    f = lambda t: t.to(torch.float32).contiguous()
    return _TimeWarp.apply(f(hall), f(lq), f(WH_W), f(WH_b), f(WC_W).reshape(-1), f(WC_b).reshape(-1), int(warp_type),
                           float(window_t))


# ------------------------------------------------------------------ front-end
class _TokenEmbed(torch.autograd.Function):
    """(word_ids [ntok] i32, char_ids [ntok,W] i32 | None, word_emb [VW,wdim], fixed_emb [G,wdim], char_emb [VC,cdim] |
    None, filt [height,cdim,cwdim] | None, bias [cwdim] | None) -> x [ntok, cwdim + wdim] = [char part | word part]
    (model_v2.py:524-620, fvta_embed_fwd; rows dense).  Backward: one fvta_embed_bwd into fresh zero buffers; the frozen
    table gets none.  `argpos` lives in the call's own ops.TokenEmbed."""

    @staticmethod
    def forward(ctx, word_ids, char_ids, word_emb, fixed_emb, char_emb, filt, bias):
        ntok = word_ids.numel()
        VW, wdim = word_emb.shape
        cw = 0 if char_emb is None else filt.shape[2]
        W = 0 if char_emb is None else char_ids.shape[1]
        height, cdim = (filt.shape[0], filt.shape[1]) if cw else (5, 0)
        op = ops.TokenEmbed(ntok, W, cdim, cw, wdim, VW, VW + fixed_emb.shape[0], char_emb.shape[0] if cw else 1, height)
        tok_off = torch.arange(ntok, dtype=torch.int64, device=word_emb.device) * (cw + wdim)
        x = torch.empty(ntok, cw + wdim, dtype=torch.float32, device=word_emb.device)
        op.forward(word_ids, char_ids, tok_off, word_emb, fixed_emb if fixed_emb.shape[0] else None, char_emb, filt, bias, x)
        if any(ctx.needs_input_grad):
            ctx.op, ctx.ids = op, (word_ids, char_ids, tok_off)
            ctx.save_for_backward(word_emb, char_emb, filt, bias)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        word_emb, char_emb, filt, bias = ctx.saved_tensors
        word_ids, char_ids, tok_off = ctx.ids
        z = lambda t: None if t is None else torch.zeros_like(t)
        dwe, dce, dfl, dbi = z(word_emb), z(char_emb), z(filt), z(bias)
        ctx.op.backward(word_ids, char_ids, tok_off, char_emb, filt, _c(g), dwe, dce, dfl, dbi)
        need = ctx.needs_input_grad
        return (None, None, dwe if need[2] else None, None, dce if need[4] else None, dfl if need[5] else None,
                dbi if need[6] else None)


def token_embed(word_ids, char_ids, word_emb, fixed_emb, char_emb=None, filt=None, bias=None):
    """ids of any shape [...] (chars [..., W]) -> x [..., cwdim + wdim]; filt [height, cdim, cwdim] (or TF's
    [1, height, cdim, cwdim]).  Ids >= VW read fixed_emb[id - VW].  keep_prob is 1 (no char dropout here)."""
    dev = ops.require_gpu()
    f = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    i32 = lambda t: t.to(dev, torch.int32).contiguous()
    lead = tuple(word_ids.shape)
    if char_emb is not None:
        filt = filt.reshape(filt.shape[-3:])
        char_ids = i32(char_ids).reshape(-1, char_ids.shape[-1])
    else:
        char_ids = filt = bias = None
    x = _TokenEmbed.apply(i32(word_ids).reshape(-1), char_ids, f(word_emb), f(fixed_emb), f(char_emb), f(filt), f(bias))
    return x.reshape(lead + (x.shape[-1],))


class _PhotoFeatures(torch.autograd.Function):
    """(pidx [R] i32, image_emb_mat [P,idim], W [idim,tdim] | None, b [tdim] | None; add_tanh) -> x [R, tdim or idim]
    (model_v2.py:634-645, fvta_image_trans_fwd).  image_emb_mat is a placeholder in the reference: no gradient."""

    @staticmethod
    def forward(ctx, pidx, image_emb_mat, W, b, add_tanh):
        R, idim = pidx.numel(), image_emb_mat.shape[1]
        tdim = idim if W is None else W.shape[1]
        op = ops.ImageTrans(R, idim, tdim, add_tanh and W is not None)
        row_off = torch.arange(R, dtype=torch.int64, device=pidx.device) * tdim
        x = torch.empty(R, tdim, dtype=torch.float32, device=pidx.device)
        op.forward(pidx, row_off, image_emb_mat, W, b, x)
        if W is not None and any(ctx.needs_input_grad):
            ctx.op, ctx.idx = op, (pidx, row_off)
            ctx.save_for_backward(image_emb_mat, W, x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[2] and not ctx.needs_input_grad[3]:
            return (None,) * 5
        image_emb_mat, W, x = ctx.saved_tensors
        pidx, row_off = ctx.idx
        dW = torch.zeros_like(W)
        db = torch.zeros(W.shape[1], dtype=torch.float32, device=W.device)
        ctx.op.backward(pidx, row_off, image_emb_mat, x, _c(g), dW, db)
        need = ctx.needs_input_grad
        return None, None, dW if need[2] else None, db if need[3] else None, None


def photo_features(pis, image_emb_mat, W=None, b=None, add_tanh=False):
    """pis [...] photo indices into image_emb_mat [P,idim] -> [..., tdim] through image_trans_linear W [idim,tdim], b [tdim]
    (+ tanh), or the gathered rows [..., idim] without W."""
    dev = ops.require_gpu()
    f = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    x = _PhotoFeatures.apply(pis.to(dev, torch.int32).contiguous().reshape(-1), f(image_emb_mat).detach(), f(W), f(b),
                             bool(add_tanh))
    return x.reshape(tuple(pis.shape) + (x.shape[-1],))


# ------------------------------------------------------- DMN+ episodic memory
class _AttGruSeq(torch.autograd.Function):
    """(facts [N,F,d], gate [N,F], h0 [N,d] | None, Wg [2d,d], bg [d], Wc [d,d], Wi [d,d], bi [d]) -> h_last [N,d]: the
    AttentionGRUCell (attention_gru_cell.py:50-70) over all F facts with the state carried, one fvta_attgru_seq_fwd.
    Each call owns its ops.AttentionGRUSeq and with it `saved`; the backward (one fvta_attgru_seq_bwd, workspace
    allocated there) only reads it, so a retained graph may be walked again."""

    @staticmethod
    def forward(ctx, facts, gate, h0, Wg, bg, Wc, Wi, bi):
        N, F, d = facts.shape
        need = any(ctx.needs_input_grad)
        op = ops.AttentionGRUSeq(N, F, d, training=need)
        h_last = op.forward(facts, gate, h0, Wg, bg, Wc, Wi, bi)
        ctx.set_materialize_grads(False)
        if need:
            ctx.op = op
            ctx.save_for_backward(facts, gate, Wg, Wc, Wi)
        return h_last

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 8
        facts, gate, Wg, Wc, Wi = ctx.saved_tensors
        N, F, d = facts.shape
        need = ctx.needs_input_grad
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=facts.device)
        d_facts, d_gate = new(N, F, d), new(N, F)
        d_h0 = new(N, d) if need[2] else None
        dWg, dbg, dWc, dWi, dbi = new(2 * d, d), new(d), new(d, d), new(d, d), new(d)     # stored: accumulate = 0
        ctx.op.backward(facts, gate, Wg, Wc, Wi, _c(g), d_facts, d_gate, d_h0, dWg, dbg, dWc, dWi, dbi, accumulate=False)
        return tuple(t if n else None for t, n in zip((d_facts, d_gate, d_h0, dWg, dbg, dWc, dWi, dbi), need))


def attgru_seq(facts, gate, h0, Wg, bg, Wc, Wi, bi):
    """facts [N,F,d], gate [N,F] (the attention times `t < length`: a gate of 0 copies the state through), h0 [N,d] or
    None (zeros), the five cell variables -> h_last [N,d]"""
    ops.require_gpu()
    f = lambda t: None if t is None else t.to(torch.float32).contiguous()
    return _AttGruSeq.apply(f(facts), f(gate), f(h0), f(Wg), f(bg), f(Wc), f(Wi), f(bi))


class _GruSeq(torch.autograd.Function):
    """(x [N,T,in], lens int32 [N] | None, h0 [N,d] | None, Wg [in+d,2d], bg [2d], Wc [in+d,d], bc [d], reverse) ->
    (out [N,T,d], h_last [N,d]): TF's GRUCell under dynamic_rnn, one fvta_gru_seq_fwd.  Each call owns its ops.GRUSeq and
    with it `saved`; the backward (one fvta_gru_seq_bwd) only reads it, so a retained graph may be walked again.  An output
    nobody used arrives as a None gradient and goes down as NULL."""

    @staticmethod
    def forward(ctx, x, lens, h0, Wg, bg, Wc, bc, reverse):
        N, T, din = x.shape
        d = Wc.shape[1]
        need = any(ctx.needs_input_grad)
        op = ops.GRUSeq(N, T, din, d, reverse=reverse, training=need)
        out, h_last = op.forward(x, lens, h0, Wg, bg, Wc, bc)
        ctx.set_materialize_grads(False)
        if need:
            ctx.op = op
            ctx.save_for_backward(x, lens, Wg, Wc)
        return out, h_last

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_last):
        if g_out is None and g_last is None:
            return (None,) * 8
        x, lens, Wg, Wc = ctx.saved_tensors
        N, T, din = x.shape
        d = Wc.shape[1]
        need = ctx.needs_input_grad
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=x.device)
        d_x = new(N, T, din)
        d_h0 = new(N, d) if need[2] else None
        dWg, dbg, dWc, dbc = new(din + d, 2 * d), new(2 * d), new(din + d, d), new(d)     # stored: accumulate = 0
        ctx.op.backward(x, lens, Wg, Wc, _c(g_out), _c(g_last), d_x, d_h0, dWg, dbg, dWc, dbc, accumulate=False)
        grads = (d_x, None, d_h0, dWg, dbg, dWc, dbc, None)
        return tuple(t if n else None for t, n in zip(grads, need))


def gru_seq(x, lens, h0, Wg, bg, Wc, bc, reverse=False):
    """x [N,T,in], lens [N] (any integer tensor or list) or None (every row has length T), h0 [N,d] or None (zeros), TF's
    GRUCell variables gates/{kernel [in+d,2d], bias [2d]} and candidate/{kernel [in+d,d], bias [d]} -> (out [N,T,d] with
    rows t >= lens[n] zero, h_last [N,d]); reverse=True walks every row from lens[n] - 1 down to 0."""
    dev = ops.require_gpu()
    f = lambda t: None if t is None else t.to(torch.float32).contiguous()
    if lens is not None:
        lens = torch.as_tensor(lens).to(dev, torch.int32).contiguous()
    x, Wg, Wc = f(x), f(Wg), f(Wc)
    if x.dim() != 3 or Wc.dim() != 2 or Wc.shape[0] != x.shape[2] + Wc.shape[1] or tuple(Wg.shape) != (Wc.shape[0], 2 * Wc.shape[1]):
        raise ValueError("gru_seq: x %s, gates kernel %s, candidate kernel %s do not fit" % (tuple(x.shape), tuple(Wg.shape), tuple(Wc.shape)))
    return _GruSeq.apply(x, lens, f(h0), Wg, f(bg), Wc, f(bc), bool(reverse))


class _CompactBilinear(torch.autograd.Function):
    """(x [N*P, d1], q [N, d2], device tables h1, s1, h2, s2; D, P, normalize) -> [N*P, D]: one fvta_cbp_fwd.  Each call
    owns its ops.CompactBilinear; the backward (one fvta_cbp_bwd, accumulate = 0) only reads what it kept.  The gradient
    at an exactly zero bucket of the normalised form is 0 (the convention of include/fvta_hip.h; TF gives NaN there)."""

    @staticmethod
    def forward(ctx, x, q, h1, s1, h2, s2, D, P, normalize):
        need = any(ctx.needs_input_grad)
        op = ops.CompactBilinear(q.shape[0], P, x.shape[1], q.shape[1], D, normalize=normalize, training=need)
        out = op.forward(x, q, h1, s1, h2, s2)
        ctx.set_materialize_grads(False)
        if need:
            ctx.op = op
            ctx.save_for_backward(x, q, h1, s1, h2, s2)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 9
        x, q, h1, s1, h2, s2 = ctx.saved_tensors
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dq = torch.empty_like(q) if ctx.needs_input_grad[1] else None
        ctx.op.backward(x, q, h1, s1, h2, s2, _c(g), dx, dq, accumulate=False)
        return (dx, dq) + (None,) * 7


def compact_bilinear(x, q, h1, s1, h2, s2, D, P=1, normalize=False):
    """x [N*P, d1], q [N, d2] (row n of q is shared by rows n*P .. n*P+P-1 of x; P = 1: one q row per x row), the count
    sketch tables as device tensors (ops.upload_sketch_tables validates and uploads them) -> z [N*P, D], the count sketch of
    the outer products, or with normalize its l2-normalised square root of the magnitude (model_mcb.py:645).
    Non-contiguous inputs are made contiguous."""
    ops.require_gpu()
    f = lambda t: t.to(torch.float32).contiguous()
    x, q = f(x), f(q)
    D, P = int(D), int(P)
    if x.dim() != 2 or q.dim() != 2 or P < 1 or x.shape[0] != q.shape[0] * P:
        raise ValueError("compact_bilinear: x %s and q %s do not fit P = %d" % (tuple(x.shape), tuple(q.shape), P))
    if h1.numel() != x.shape[1] or s1.numel() != x.shape[1] or h2.numel() != q.shape[1] or s2.numel() != q.shape[1]:
        raise ValueError("compact_bilinear: the tables do not fit d1 = %d, d2 = %d" % (x.shape[1], q.shape[1]))
    i = lambda t: t.to(x.device, torch.int32).contiguous()
    g = lambda t: t.to(x.device, torch.float32).contiguous()
    return _CompactBilinear.apply(x, q, i(h1), g(s1), i(h2), g(s2), D, P, bool(normalize))


class _DmnFeatures(torch.autograd.Function):
    """(facts [N,F,d], q [N,d], m [N,d]) -> [N,F,4d] = [fact*q, fact*m, |fact-q|, |fact-m|] (model_dmnplus.py:93-98,
    fvta_dmn_features); backward: fvta_dmn_features_bwd into fresh zero buffers (it accumulates)."""

    @staticmethod
    def forward(ctx, facts, q, m):
        N, F, d = facts.shape
        out = torch.empty(N, F, 4 * d, dtype=torch.float32, device=facts.device)
        check(_lib.load().fvta_dmn_features(ptr(facts), ptr(q), ptr(m), ptr(out), N, F, d, stream_ptr()), "fvta_dmn_features")
        ctx.set_materialize_grads(False)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(facts, q, m)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None
        facts, q, m = ctx.saved_tensors
        N, F, d = facts.shape
        d_facts, d_q, d_m = torch.zeros_like(facts), torch.zeros_like(q), torch.zeros_like(m)
        check(_lib.load().fvta_dmn_features_bwd(ptr(facts), ptr(q), ptr(m), ptr(_c(g)), ptr(d_facts), ptr(d_q), ptr(d_m),
                                                N, F, d, stream_ptr()), "fvta_dmn_features_bwd")
        return tuple(t if n else None for t, n in zip((d_facts, d_q, d_m), ctx.needs_input_grad))


def dmn_features(facts, q, m):
    ops.require_gpu()
    f = lambda t: t.to(torch.float32).contiguous()
    return _DmnFeatures.apply(f(facts), f(q), f(m))


class _Relu(torch.autograd.Function):
    """fvta_relu_fwd; the backward reads the OUTPUT (fvta_relu_bwd: dx = dy where y > 0)."""

    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        check(_lib.load().fvta_relu_fwd(ptr(x), ptr(y), x.numel(), stream_ptr()), "fvta_relu_fwd")
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return None
        y, = ctx.saved_tensors
        dx = torch.empty_like(y)
        check(_lib.load().fvta_relu_bwd(ptr(y), ptr(_c(g)), ptr(dx), y.numel(), stream_ptr()), "fvta_relu_bwd")
        return dx


def relu(x):
    ops.require_gpu()
    return _Relu.apply(x.to(torch.float32).contiguous())
