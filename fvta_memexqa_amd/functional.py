"""The reference's functional graph helpers with their own keyword signatures (SURVEY 8b "functional ops"):

    softmax(logits, scope=None)                                                     model_v2.py:23-28
    softsel(target, logits, hard=False, hardK=None, scope=None)                      model_v2.py:39-48
    linear(x, output_size, scope, add_tanh=False, wd=None)                           model_v2.py:75-100
    exp_mask(val, mask)                                                              utils.py:210-213
    attention(hinfo, hq, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None,
              add_tanh=False, bidirect=False, scope=None) -> (h_a, a_logits)         model_v2.py:125-201
    attention_3d(hinfo, hq, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None, add_tanh=False,
                 time_warp_att=False, C=None, bidirect=False, scope=None)            model_v2.py:210-298
    attention_keeprank1(hinfo, hq, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None,
                        bidirect=False, scope=None) -> h_a [N,M,w]                   model.py:247-314
      (attention_raw / attention_keeprank1_raw: the same with explicit W, b instead of the variable store)
    attention_tgif(hinfo, lq, hinfo_mask=None, wd=None, mlp_dim=512, scope=None)     model.py:210-244
    context_tensor(streams, masks=None) -> (hall, hall_mask)                         model_v2.py:863-914
    time_warp(hall, lq, warp_type=1, window_t=None, scope=None) -> (warp_h, scale)   model_v2.py:953-1009
    time_indication_func(C, warp_type=1, window_t=3.0) -> (C_windowed, window_t)     model_v2.py:301-341
    generate_episode(memory, q_vec, fact_vecs, fact_vecs_length, hop_index,
                     hidden_size, scope=None) -> episode [N,d]                       model_dmnplus.py:113-136
    episodic_memory(gq, facts, facts_length, num_hops, hidden_size,
                    scope="memory") -> [N,hidden_size]                               model_dmnplus.py:503-516
      (generate_episode_raw / episodic_memory_raw: the same with explicit variables)
    compact_bilinear_pooling_layer(bottom1, bottom2, output_dim, sum_pool=True, rand_h_1=None, rand_s_1=None,
                                   rand_h_2=None, rand_s_2=None, seed_h_1=1, seed_s_1=3, seed_h_2=5, seed_s_2=7,
                                   sequential=True, compute_size=128)                model_mcb.py:1254-1363
    mcb_attention_raw(hpis, gq, tables, filter_conv1, filter_conv2) -> (attended, att)   model_mcb.py:628-672

Tensors are torch CUDA tensors; every op is one call into libfvta_hip.so, wrapped in a `torch.autograd.Function`
(autograd.py): a tensor that requires grad gets its gradient through the library's backward kernels, and when nothing
requires grad the same forward kernels run and nothing is kept.  The variable store keeps plain tensors;
`variables[name].requires_grad_()` makes one a leaf that receives its gradient.
On the focal attentions' `h_a` path, and on `attention_keeprank1`'s per-(n,m) vectors, two deviations of the model's
backward kernels carry over: an exact tie in the max over the question sends its gradient to the
FIRST arg-max (TensorFlow splits it), and a fully masked (n,k) row list sends no gradient into its logits.  Where the reference creates TF variables (`linear`'s W / b, the
`att_logits` linear inside the attentions) the variable lives in a module-level store under the same scoped name
(`variable_scope("attention")` + `scope="all"` -> "attention/all/att_logits/W"), initialised like the reference
(truncated normal 0.1 / zeros) and reused on the next call, which is what `tf.get_variable` under reuse does.
`wd` appends the l2 terms to `losses` like `add_wd` (model_v2.py:347-354).
"""
import contextlib
import zlib

import torch

from . import _lib, autograd, ops
from ._lib import check, ptr, stream_ptr
from .model_v2 import SUPPORTED_W

variables = {}      # scoped name -> torch tensor (fp32, CUDA)
losses = []         # the "losses" collection: scalar tensors appended by `wd`
_scope = []


@contextlib.contextmanager
def variable_scope(name):
    _scope.append(name)
    try:
        yield
    finally:
        _scope.pop()


def reset_default_graph():
    variables.clear()
    del losses[:]


def _name(*parts):
    return "/".join([p for p in _scope if p] + [p for p in parts if p])


def get_variable(name, shape, init="trunc_normal", seed=None):
    """tf.get_variable under reuse: create on first use, return the same tensor afterwards."""
    if name in variables:
        if tuple(variables[name].shape) != tuple(shape):
            raise ValueError("variable %s exists with shape %s, asked for %s" % (name, tuple(variables[name].shape), tuple(shape)))
        return variables[name]
    dev = ops.require_gpu()
    if init == "zeros":
        v = torch.zeros(*shape, dtype=torch.float32, device=dev)
    elif init == "glorot":          # tf.get_variable's default / xavier_initializer: uniform(+-sqrt(6 / (fan_in + fan_out)))
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()) if seed is None else seed)
        lim = (6.0 / (shape[0] + shape[-1])) ** 0.5
        v = ((torch.rand(*shape, generator=g) * 2 - 1) * lim).to(dev)
    else:
        from .synth import _trunc_normal
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()) if seed is None else seed)
        v = _trunc_normal(g, tuple(shape)).to(dev)                  # truncated_normal(stddev=0.1), model_v2.py:88
    variables[name] = v
    return v


def _add_wd(names, wd):
    """add_wd (model_v2.py:347-354) for the variables of the current call's scope"""
    if wd is None or wd == 0.0:
        return
    for n in names:
        t = torch.zeros(1, dtype=torch.float32, device=variables[n].device)
        ops.weight_decay(variables[n].reshape(-1), None, wd, t)
        losses.append(t)


def _f32(t):
    return t.to(torch.float32).contiguous()


def softmax(logits, scope=None):
    return autograd.softmax(_f32(logits))


def softsel(target, logits, hard=False, hardK=None, scope=None):
    """target [..., J, d], logits [..., J] -> [..., d]  (`hard` / `hardK` are accepted and unused, as in the reference)"""
    target, logits = _f32(target), _f32(logits)
    J, d = target.shape[-2], target.shape[-1]
    if tuple(logits.shape) != tuple(target.shape[:-1]):
        raise ValueError("softsel: logits %s do not match target %s" % (tuple(logits.shape), tuple(target.shape)))
    return autograd.softsel(target, logits)


def exp_mask(val, mask):
    val = _f32(val)
    m = ops.as_mask_u8(mask.expand_as(val) if tuple(mask.shape) != tuple(val.shape) else mask)
    return autograd.exp_mask(val, m)


def linear_raw(x, W, b, add_tanh=False):
    """flatten(x, 1) . W [in, out] + b through fvta_linear_fwd with explicit weights (no variable scope)"""
    return autograd.linear(_f32(x), _f32(W), None if b is None else _f32(b), add_tanh)


def linear(x, output_size, scope, add_tanh=False, wd=None):
    x = _f32(x)
    din = x.shape[-1]
    with variable_scope(scope):
        wn, bn = _name("W"), _name("b")
        W = get_variable(wn, (din, int(output_size)))
        b = get_variable(bn, (int(output_size),), init="zeros")
        _add_wd([wn, bn], wd)
    return autograd.linear(x, W, b, add_tanh)


def _pad_channels(t, wp):
    w = t.shape[-1]
    if w == wp:
        return t.contiguous()
    return torch.nn.functional.pad(t, (0, wp - w))      # (differentiable: the gradient of the padding is dropped)


def attention_raw(hinfo, hq, W, b, hinfo_mask=None, hq_mask=None, simiMatrix=1, add_tanh=False, feat_order=0, tscale=None):
    """The focal attention with explicit weights: hinfo [N,K,T,w], hq [N,JQ,w], W [F*w, 1] (any shape with F*w elements;
    None for simiMatrix 4), b [1] -> (h_a [N,w], a_logits [N,K,T,JQ]).  w is zero padded to a kernel width (exact: a zero
    channel adds nothing to any feature of any similarity), W block-wise with it; both outputs are differentiable
    (h_a: fvta_attn_bwd_tw, a_logits: fvta_attn_cube_bwd)."""
    if simiMatrix not in (1, 2, 3, 4):
        raise ValueError("similarity matrix not implemented")              # model_v2.py:255-257 (sys.exit there)
    hinfo, hq = _f32(hinfo), _f32(hq)
    N, K, T, w = hinfo.shape
    wp = next((c for c in SUPPORTED_W if w <= c), None)
    if wp is None:
        raise ValueError("attention: feature width %d too large (max %d)" % (w, SUPPORTED_W[-1]))
    F = {1: 3, 2: 2, 3: 4, 4: 0}[simiMatrix]
    if F:
        W = _pad_channels(_f32(W).reshape(F, w), wp).reshape(-1)
        b = _f32(b)
    else:
        W = b = None
    ops.require_gpu()
    both = hinfo_mask is not None and hq_mask is not None                  # model_v2.py:146 / 233: only when BOTH are given
    hm = ops.as_mask_u8(hinfo_mask.reshape(N, K, T)) if both else None
    qm = ops.as_mask_u8(hq_mask) if both else None
    h_a, a = autograd.focal_attention(_pad_channels(hinfo, wp), _pad_channels(hq, wp), W, b, hm, qm, simiMatrix, add_tanh,
                                      feat_order, tscale)
    return h_a[:, :w].contiguous(), a


def _album_attention_args(rows, hq, index, W, b, rows_mask, hq_mask, simiMatrix, pooled, differentiable, no_backward,
                          forward_only, warp=None):
    """The preparation the five attention_3d_{shared,pooled}[_warped]_raw functions share, every refusal before any
    library or device call and in one order: the similarity matrix (and warp type), differentiable with simiMatrix 4
    (`no_backward`), gradient mode on a forward-only call (`forward_only`), the shapes, the index, the width.  rows:
    [A,K,T,w] / [A,K,M,JX,w], `pooled`: a pool [P,K,JX,w] with album lists.  warp: None, or (lq, WH_W, WH_b, WC_W, WC_b,
    warp_type, energy).  Without `differentiable` everything is detached, and a `pooled` torch.bfloat16 pool STAYS bf16
    (through the reshape and the zero padding of the width, both exact): the inference ops read it as it is, no fp32 copy.
    With `differentiable`, and for the shared family, bf16 rows are widened as ever.  -> a namespace: rows / hq / lq padded to the
    kernel width wp, idx on the device, W padded block-wise, b, the two uint8 masks (None unless BOTH are given:
    model_v2.py:233), the warp's weights as the kernels read them, energy (detached, or None), and A K T NQ JQ w wp."""
    from types import SimpleNamespace
    if simiMatrix not in (1, 2, 3, 4):
        raise ValueError("similarity matrix not implemented")
    lq, WH_W, WH_b, WC_W, WC_b, warp_type, energy = warp if warp is not None else (None,) * 7
    if warp is not None:
        _check_warp_type(warp_type)
    if differentiable and simiMatrix == 4:
        raise NotImplementedError(no_backward)
    tensors = [t for t in (rows, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b) if torch.is_tensor(t)]
    if not differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(forward_only)
    det = (lambda t: t) if differentiable else (lambda t: t.detach())
    keep_bf16 = pooled and not differentiable and torch.is_tensor(rows) and rows.dtype == torch.bfloat16
    rows, hq = det(rows.contiguous() if keep_bf16 else _f32(rows)), det(_f32(hq))
    lq = None if warp is None else det(_f32(lq))
    if pooled and rows.dim() != 4:
        raise ValueError("album pool: expected [P,K,JX,w], got shape %s" % (tuple(rows.shape),))
    A, K, w = rows.shape[0], rows.shape[1], rows.shape[-1]
    rows = rows.reshape(A, K, -1, w)
    T = rows.shape[2]
    NQ, JQ = hq.shape[0], hq.shape[1]
    if warp is not None and tuple(lq.shape) != (NQ, w):
        raise ValueError("lq: expected the questions' last states [%d, %d], got %s" % (NQ, w, tuple(lq.shape)))
    both = rows_mask is not None and hq_mask is not None
    idx = ops.check_album_lists(index, A, both) if pooled else ops.check_album_index(index, A)
    if idx.shape[0] != NQ:
        raise ValueError(("album lists: %d lists for %d questions" if pooled else "album index: %d entries for %d questions")
                         % (idx.shape[0], NQ))
    if energy is not None and tuple(energy.shape) != (A, T):
        raise ValueError("energy: expected [%d, %d], got %s" % (A, T, tuple(energy.shape)))
    wp = next((c for c in SUPPORTED_W if w <= c), None)
    if wp is None:
        raise ValueError("attention: feature width %d too large (max %d)" % (w, SUPPORTED_W[-1]))
    F = {1: 3, 2: 2, 3: 4, 4: 0}[simiMatrix]
    if F:
        W = _pad_channels(det(_f32(W)).reshape(F, w), wp).reshape(-1)
        b = det(_f32(b))
    else:
        W = b = None
    dev = ops.require_gpu()
    p = SimpleNamespace(A=A, K=K, T=T, NQ=NQ, JQ=JQ, w=w, wp=wp, W=W, b=b, idx=idx.to(dev),
                        rows=_pad_channels(rows, wp), hq=_pad_channels(hq, wp),
                        rm=ops.as_mask_u8(rows_mask.reshape(A, K, T)) if both else None,
                        qm=ops.as_mask_u8(hq_mask) if both else None)
    if warp is not None:
        p.WH, p.WC, p.WHb, p.WCb = _warp_weights(w, wp, WH_W, WC_W, WH_b, WC_b, detach=not differentiable)
        p.lq = _pad_channels(lq, wp)
        p.energy = None if energy is None else _f32(energy).detach().contiguous()
    return p


def _album_attention(p, pooled, differentiable, simiMatrix, add_tanh, warp_type=None, window_t=None):
    """What the four attention_3d_{shared,pooled}[_warped]_raw functions do with the namespace p of _album_attention_args:
    differentiable, the autograd function; else the op built for p's shape and its forward (under the warp, warp_type not
    None, with the energy it computes unless one was given) -> (h_a sliced to w, a_logits[, scale])"""
    M = (p.idx.shape[1],) if pooled else ()
    if warp_type is None:
        if differentiable:
            fn = autograd.pooled_focal_attention if pooled else autograd.shared_focal_attention
            out = fn(p.rows, p.hq, p.idx, p.W, p.b, p.rm, p.qm, simiMatrix, add_tanh)
        else:
            op = (ops.PooledFocalAttention if pooled else ops.SharedFocalAttention)(
                p.A, p.NQ, *M, p.K, p.T, p.JQ, p.wp, simiMatrix, add_tanh)
            out = op.forward(p.rows, p.rm, p.hq, p.qm, p.idx, p.W, p.b, want_logits=True)
    elif differentiable:   # (the gradients come back sliced to w; WH_W's comes back [2w,w] with zeros below row w)
        fn = autograd.pooled_warped_focal_attention if pooled else autograd.shared_warped_focal_attention
        out = fn(p.rows, p.hq, p.lq, p.idx, p.W, p.b, p.WH, p.WHb, p.WC, p.WCb, p.rm, p.qm, simiMatrix, add_tanh, warp_type,
                 float(window_t), p.energy)
    else:
        op = (ops.PooledWarpedFocalAttention if pooled else ops.SharedWarpedFocalAttention)(
            p.A, p.NQ, *M, p.K, p.T, p.JQ, p.wp, simiMatrix, add_tanh, warp_type, float(window_t))
        energy = op.album_energy(p.rows, p.WH, p.WC) if p.energy is None else p.energy
        out = op.forward(p.rows, p.rm, energy, p.hq, p.qm, p.lq, p.idx, p.W, p.b, p.WHb, p.WC, p.WCb, want_logits=True,
                         want_scale=True)
    return (out[0][:, :p.w].contiguous(),) + tuple(out[1:])


def attention_3d_shared_raw(hinfo, hq, album, W, b, hinfo_mask=None, hq_mask=None, simiMatrix=1, add_tanh=False,
                            differentiable=False):
    """attention_3d for NQ questions over A albums held once: hinfo [A,K,T,w] (or [A,K,M,JX,w]), hq [NQ,JQ,w], album [NQ]
    integers in [0, A) (validated on the host before the upload), W / b as attention_raw -> (h_a [NQ,w], a_logits
    [NQ,K,T,JQ]): question i attends album[i]'s rows, with attention_raw's result for that pair.
    differentiable=False (the default) is the inference call (fvta_attn_shared_fwd keeps nothing for a backward): with
    gradient mode on and an argument that requires grad it raises instead of returning a detached result.
    differentiable=True goes through autograd.shared_focal_attention (simiMatrix 1-3; 4 raises NotImplementedError):
    gradients flow from h_a to hinfo -- summed over each album's questions, [A,K,T,w] -- hq, W and b; a_logits carries
    none."""
    p = _album_attention_args(
        hinfo, hq, album, W, b, hinfo_mask, hq_mask, simiMatrix, False, differentiable,
        "attention_3d_shared_raw(differentiable=True): simiMatrix 4 has no shared-context backward; "
        "use the per-question attention_3d (attention_raw) on hinfo.index_select(0, album)",
        "attention_3d_shared_raw is forward-only by default: pass differentiable=True (simiMatrix 1-3), call "
        "it under torch.no_grad(), or use the per-question attention_3d (functional.attention_3d / "
        "attention_raw, nn.FocalAttention3D.forward)")
    return _album_attention(p, False, differentiable, simiMatrix, add_tanh)


def attention_3d_pooled_raw(pool, hq, albums, W, b, pool_mask=None, hq_mask=None, simiMatrix=1, add_tanh=False,
                            differentiable=False):
    """attention_3d for NQ questions that each LIST M albums of one pool of encoded albums: pool [P,K,JX,w], hq [NQ,JQ,w],
    albums [NQ,M] (a tensor, an array or a list of lists -- ragged lists are padded; entries in [0, P), or -1 for an empty
    slot, which needs both masks; validated on the host before the upload), W / b as attention_raw -> (h_a [NQ,w],
    a_logits [NQ,K,M*JX,JQ]): question i attends its albums' rows laid end to end, hinfo_i[k, m*JX + j] =
    pool[albums[i,m], k, j] (an empty slot: JX masked zero rows), with attention_raw's result for that context -- which is
    never built: each pooled album is held once and read once per group of the (question, slot) references that name it
    (fvta_attn_pool_fwd).  A torch.bfloat16 pool is read as it is by the inference call (fvta_attn_pool_fwd_bf16: no fp32
    copy, the bits of the call on pool.float()); differentiable=True widens it, and the gradient reaches it through the
    cast.  differentiable=False (the default) is that inference call: with gradient mode on and an
    argument that requires grad it raises, as attention_3d_shared_raw does.  differentiable=True goes through
    autograd.pooled_focal_attention (simiMatrix 1-3; 4 raises NotImplementedError): gradients flow from h_a to pool --
    summed over every (question, slot) that names the album, [P,K,JX,w] -- hq, W and b; a_logits carries none."""
    p = _album_attention_args(
        pool, hq, albums, W, b, pool_mask, hq_mask, simiMatrix, True, differentiable,
        "attention_3d_pooled_raw(differentiable=True): simiMatrix 4 has no pooled backward; use the "
        "per-question attention_3d (attention_raw) on the gathered rows",
        "attention_3d_pooled_raw is forward-only: call it under torch.no_grad(), or use the per-question "
        "attention_3d (functional.attention_3d / attention_raw, nn.FocalAttention3D.forward) on the "
        "gathered rows")
    return _album_attention(p, True, differentiable, simiMatrix, add_tanh)


def _warp_weights(w, wp, WH_W, WC_W, WH_b=None, WC_b=None, detach=True):
    """the time warp's weights as the shared-context kernels read them: WH_W's first w rows [wp,wp] (the rest sees a zero
    feature), WC_W [wp], and -- where given -- WH_b [wp], WC_b [1], zero padded to the kernel width (exact: a zero channel
    adds nothing to v, s0 or WC . lq); detach=False: with differentiable torch ops"""
    pad = torch.nn.functional.pad
    f = (lambda t: _f32(t).detach()) if detach else _f32
    WH = pad(f(WH_W).reshape(-1, w)[:w], (0, wp - w, 0, wp - w)).contiguous()
    WC = pad(f(WC_W).reshape(w), (0, wp - w)).contiguous()
    WH_b = None if WH_b is None else pad(f(WH_b).reshape(w), (0, wp - w)).contiguous()
    WC_b = None if WC_b is None else f(WC_b).reshape(1)
    return WH, WC, WH_b, WC_b


def album_energy(hinfo, WH_W, WC_W):
    """e [A,T] = sum_k sum_c v[c] hinfo[a,k,t,c]^2, v = WH_W[:w] WC_W: the one term of the time warp's scale that reads the
    rows (fvta_attn_shared_energy).  It belongs to the albums -- attention_3d_shared_warped_raw(energy=) takes it, and it
    holds as long as hinfo, WH/W and WC/W do.  Forward only, detached.
    An album pool [P,K,JX,w] is accepted as it is and gives e [P,JX], the energy attention_3d_pooled_warped_raw(energy=)
    takes (fvta_attn_pool_energy makes the same two launches: the same bits).  A pool held in torch.bfloat16 is read as it
    is (fvta_attn_pool_energy_bf16: no fp32 copy; the bits of the energy of pool.float()); bf16 rows of any other shape
    are widened first."""
    bf16_pool = torch.is_tensor(hinfo) and hinfo.dtype == torch.bfloat16 and hinfo.dim() == 4
    hinfo = (hinfo.contiguous() if bf16_pool else _f32(hinfo)).detach()
    A, K, w = hinfo.shape[0], hinfo.shape[1], hinfo.shape[-1]
    hinfo = hinfo.reshape(A, K, -1, w)
    wp = next((c for c in SUPPORTED_W if w <= c), None)
    if wp is None:
        raise ValueError("attention: feature width %d too large (max %d)" % (w, SUPPORTED_W[-1]))
    ops.require_gpu()
    WH, WC, _, _ = _warp_weights(w, wp, WH_W, WC_W)
    if bf16_pool:
        op = ops.PooledWarpedFocalAttention(A, 1, 1, K, hinfo.shape[2], 1, wp, 1, False, 1)
    else:
        op = ops.SharedWarpedFocalAttention(A, 1, K, hinfo.shape[2], 1, wp, 1, False, 1)
    return op.album_energy(_pad_channels(hinfo, wp), WH, WC)


def attention_3d_shared_warped_raw(hinfo, hq, album, lq, W, b, WH_W, WH_b, WC_W, WC_b, hinfo_mask=None, hq_mask=None,
                                   simiMatrix=1, add_tanh=False, warp_type=1, window_t=3.0, energy=None, differentiable=False):
    """attention_3d_shared_raw under the time warp (use_time_warp without use_time_warp_att): hinfo [A,K,T,w]
    (or [A,K,M,JX,w]) held once, hq [NQ,JQ,w], album [NQ], lq [NQ,w] the questions' last states, W / b as attention_raw,
    the warp's weights as time_warp_raw -> (h_a [NQ,w], a_logits [NQ,K,T,JQ], scale [NQ,T]): for question i, attention_raw
    on time_warp_raw's warp of (hinfo[album[i]], lq[i]), and that warp's scale.  No [NQ,K,T,w] tensor is built: the warp is
    one scalar per (question, position), applied inside the kernels (fvta_attn_shared_fwd_tw).  energy [A,T]: album_energy
    of (hinfo, WH_W, WC_W), None computes it on the spot.
    differentiable=False (the default) is the inference call, forward only: with gradient mode on and an argument that
    requires grad it raises, as attention_3d_shared_raw(differentiable=False) does.
    differentiable=True goes through autograd.shared_warped_focal_attention (simiMatrix 1-3; 4 raises NotImplementedError):
    gradients flow from h_a to hinfo -- summed over each album's questions, [A,K,T,w] -- hq, lq, W, b and the warp's four
    parameters (WH_W's rows w..2w-1 get zeros: they see a zero feature); a_logits and scale carry none.  A given energy is
    used as a cached value of the forward; the gradient through e is taken all the same."""
    p = _album_attention_args(
        hinfo, hq, album, W, b, hinfo_mask, hq_mask, simiMatrix, False, differentiable,
        "attention_3d_shared_warped_raw(differentiable=True): simiMatrix 4 has no shared-context "
        "backward; use the per-question time_warp_raw + attention_raw on hinfo.index_select(0, album)",
        "attention_3d_shared_warped_raw is forward-only: call it under torch.no_grad(), or use the "
        "per-question time_warp + attention_3d (functional.time_warp_raw / attention_raw, nn.TimeWarp / "
        "nn.FocalAttention3D.forward) on hinfo.index_select(0, album)",
        warp=(lq, WH_W, WH_b, WC_W, WC_b, warp_type, energy))
    return _album_attention(p, False, differentiable, simiMatrix, add_tanh, warp_type, window_t)


def attention_3d_pooled_warped_raw(pool, hq, albums, lq, W, b, WH_W, WH_b, WC_W, WC_b, pool_mask=None, hq_mask=None,
                                   simiMatrix=1, add_tanh=False, warp_type=1, window_t=3.0, energy=None, differentiable=False):
    """attention_3d_pooled_raw under the time warp (use_time_warp without use_time_warp_att): pool [P,K,JX,w] held once,
    hq [NQ,JQ,w], albums [NQ,M] as attention_3d_pooled_raw takes them, lq [NQ,w] the questions' last states, W / b as
    attention_raw, the warp's weights as time_warp_raw -> (h_a [NQ,w], a_logits [NQ,K,M*JX,JQ], scale [NQ,M*JX]): for
    question i, attention_raw on time_warp_raw's warp of (its albums' rows laid end to end, lq[i]), and that warp's scale.
    A position's count runs over the question's whole M*JX positions (a band, past or future crosses slot boundaries).
    Neither the [NQ,K,M*JX,w] context nor its warp is built: the warp is one scalar per (question, position), applied
    inside the kernels (fvta_attn_pool_fwd_tw).  energy [P,JX]: album_energy of (pool, WH_W, WC_W), None computes it on the
    spot.  A torch.bfloat16 pool: as attention_3d_pooled_raw (fvta_attn_pool_energy_bf16 / fvta_attn_pool_fwd_tw_bf16).
    differentiable=False (the default) is the inference call, forward only: with gradient mode on and an argument that
    requires grad it raises, as attention_3d_pooled_raw(differentiable=False) does.
    differentiable=True goes through autograd.pooled_warped_focal_attention (simiMatrix 1-3; 4 raises NotImplementedError):
    gradients flow from h_a to pool -- summed over every (question, slot) that names the album, [P,K,JX,w] -- hq, lq, W, b
    and the warp's four parameters (WH_W's rows w..2w-1 get zeros); a_logits and scale carry none.  A given energy is used
    as a cached value of the forward; the gradient through e is taken all the same."""
    p = _album_attention_args(
        pool, hq, albums, W, b, pool_mask, hq_mask, simiMatrix, True, differentiable,
        "attention_3d_pooled_warped_raw(differentiable=True): simiMatrix 4 has no pooled backward; use the "
        "per-question time_warp_raw + attention_raw on the gathered rows",
        "attention_3d_pooled_warped_raw is forward-only by default: pass differentiable=True (simiMatrix 1-3), call "
        "it under torch.no_grad(), or use the per-question time_warp + attention_3d (functional.time_warp_raw / "
        "attention_raw, nn.TimeWarp / nn.FocalAttention3D.forward) on the gathered rows",
        warp=(lq, WH_W, WH_b, WC_W, WC_b, warp_type, energy))
    return _album_attention(p, True, differentiable, simiMatrix, add_tanh, warp_type, window_t)


def attention_3d_shared(hinfo, hq, album, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None, add_tanh=False,
                        scope=None):
    """attention_3d (model_v2.py:210-298) of NQ questions over A albums whose rows are held once, with the `att_logits`
    variables of the scope (the ones attention_3d uses under the same scope); always differentiable (simiMatrix 1-3)."""
    if simiMatrix not in (1, 2, 3, 4):
        raise ValueError("similarity matrix not implemented")
    if simiMatrix == 4:
        raise NotImplementedError("attention_3d_shared: simiMatrix 4 has no shared-context backward; use attention_3d on "
                                  "hinfo.index_select(0, album)")
    w = hinfo.shape[-1]
    F = {1: 3, 2: 2, 3: 4}[simiMatrix]
    with variable_scope(scope or "attention_2vector"):
        wn, bn = _name("att_logits", "W"), _name("att_logits", "b")
        W = get_variable(wn, (F * w, 1))
        b = get_variable(bn, (1,), init="zeros")
        _add_wd([wn, bn], wd)
    return attention_3d_shared_raw(hinfo, hq, album, W, b, hinfo_mask, hq_mask, simiMatrix, add_tanh, differentiable=True)


def _attention(hinfo, hq, hinfo_mask, hq_mask, simiMatrix, wd, add_tanh, scope, feat_order, tscale=None):
    """attention_raw with the `att_logits` variables of the scope (linear(..., output_size=1, scope="att_logits"))"""
    if simiMatrix not in (1, 2, 3, 4):
        raise ValueError("similarity matrix not implemented")
    w = hinfo.shape[-1]
    F = {1: 3, 2: 2, 3: 4, 4: 0}[simiMatrix]
    W = b = None
    with variable_scope(scope):
        if F:
            wn, bn = _name("att_logits", "W"), _name("att_logits", "b")
            W = get_variable(wn, (F * w, 1))
            b = get_variable(bn, (1,), init="zeros")
            _add_wd([wn, bn], wd)
    return attention_raw(hinfo, hq, W, b, hinfo_mask, hq_mask, simiMatrix, add_tanh, feat_order, tscale)


def _tscale_of(C, N):
    """model_v2.py:269-275: a_logits_maxed[n,k,t] * sum_t' C[n,t,t'] -- the row sums of C [N,T,T] as a linear layer with
    an all-ones weight (fvta_linear_fwd); a C [N,T] is taken as those row sums already (time_warp's `scale`)."""
    C = _f32(C)
    if C.dim() == 2:
        return C
    T = C.shape[-1]
    return linear_raw(C.reshape(N * T, T), torch.ones(T, 1, dtype=torch.float32, device=C.device), None).reshape(N, T)


def attention_3d(hinfo, hq, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None, add_tanh=False, time_warp_att=False,
                 C=None, bidirect=False, scope=None):
    """hinfo [N,K,M,JX,w] (or [N,K,T,w]), hq [N,JQ,w], masks [N,K,M,JX] / [N,JQ] -> (h_a [N,w], a_logits [N,K,T,JQ]).
    C: [N,T,T] as in the reference, or its row sums [N,T] (time_warp's `scale`), which skips the N T^2 tensor."""
    if bidirect:
        raise NotImplementedError("bidirect: the 3-D branch cannot run in the reference either (SURVEY 3.5)")
    N, K, w = hinfo.shape[0], hinfo.shape[1], hinfo.shape[-1]
    tscale = None
    if time_warp_att:
        if C is None:
            raise ValueError("time_warp_att needs C [N,T,T] (model_v2.py:269-275)")
        tscale = _tscale_of(C, N)
    return _attention(hinfo.reshape(N, K, -1, w), hq, hinfo_mask, hq_mask, simiMatrix, wd, add_tanh,
                      scope or "attention_2vector", 0, tscale=tscale)


def _wsum(target, weights):
    """sum_j weights[r,j] * target[r,j,:] -> [rows, d] (fvta_wsum_fwd)"""
    return autograd.wsum(_f32(target), _f32(weights))


def _bidirect_q_a(a_logits, hq, lead):
    """the reversed-direction vector of the `bidirect` branch (model_v2.py:184-188, model.py:169-174, 297-304):
    q_a = reduce_mean over the V rows of softsel(q_aug, a_logits), i.e. every row (masked ones included: their logits are
    all -1e30, so they attend the question uniformly) softmaxes its JQ logits and averages the question with them.
    a_logits [*lead, V, JQ], hq [N, JQ, w] -> [*lead, w].  Three launches: softmax over JQ, the mean over V of the
    weights (the average commutes with the weighted sum), the weighted sum of the question vectors."""
    V, JQ = a_logits.shape[-2], a_logits.shape[-1]
    G = int(torch.tensor(lead).prod().item()) if len(lead) else 1
    p = softmax(a_logits)                                                   # [*lead, V, JQ]
    ones = torch.full((G, V), 1.0 / V, dtype=torch.float32, device=p.device)
    pbar = _wsum(p.reshape(G, V, JQ), ones)                                 # [G, JQ]
    N = hq.shape[0]
    per_n = G // N                                                          # (n, m) groups share n's question
    q = _f32(hq)
    if per_n > 1:
        q = q[:, None].expand(N, per_n, JQ, q.shape[-1]).reshape(G, JQ, q.shape[-1])
    return _wsum(q, pbar).reshape(*lead, q.shape[-1])


def bidirect_q_a(a_logits, hq):
    """_bidirect_q_a for the 1-D attention (a_logits [N,V,JQ] -> q_a [N,w]): the same three launches; where
    fvta_attn_qside_bwd covers the shape (JQ <= 64, V * JQ <= 8192) it is their backward, otherwise each launch's own."""
    N, V, JQ = a_logits.shape
    if JQ <= 64 and V * JQ <= 8192:
        return autograd.attn_qside(a_logits.contiguous(), _f32(hq))
    return _bidirect_q_a(a_logits, hq, (N,))


def attention(hinfo, hq, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None, add_tanh=False, bidirect=False, scope=None):
    """hinfo [N,...,w] flattened to [N,V,w] (model_v2.py:133) -> (h_a [N,w], a_logits [N,V,JQ]); with `bidirect`
    h_a is [N,2w] = concat([h_a, q_a]) (model_v2.py:184-192)."""
    N, w = hinfo.shape[0], hinfo.shape[-1]
    h = hinfo.reshape(N, 1, -1, w)
    hm = hinfo_mask.reshape(N, 1, -1) if hinfo_mask is not None else None
    h_a, a = _attention(h, hq, hm, hq_mask, simiMatrix, wd, add_tanh, scope or "attention_2vector", 0)
    a = a.reshape(N, h.shape[2], hq.shape[1])
    if bidirect:
        h_a = torch.cat([h_a, bidirect_q_a(a, hq)], 1)                      # tf.concat: memory layout, no arithmetic
    return h_a, a


def attention_keeprank1_raw(hinfo, hq, W, b, hinfo_mask=None, hq_mask=None, simiMatrix=1, bidirect=False):
    """attention_keeprank1 with explicit weights: hinfo [N,M,...,w], hq [N,JQ,w], W [F*w, 1] (any shape with F*w
    elements), b [1] -> h_a [N,M,w] ([N,M,2w] with `bidirect`).  w is zero padded to a kernel width, W block-wise with it;
    the result is differentiable (fvta_attn_bwd_u; the bidirect half through fvta_attn_cube_bwd).  With a gradient wanted
    N * M is at most 65535, and backward() allocates a workspace of one dQs slab set per (n,m) -- N M bsplit
    (256 / min(w/4, 256)) 32 ceil(JQ/32) w floats, 136 MB at N M = 1040 and w = 64: wide batches of narrow rows cost memory."""
    if simiMatrix not in (1, 2, 3):
        raise ValueError("similarity matrix not implemented")              # model.py:283-285 (sys.exit there)
    hinfo, hq = _f32(hinfo), _f32(hq)
    N, M, w = hinfo.shape[0], hinfo.shape[1], hinfo.shape[-1]
    h = hinfo.reshape(N, M, -1, w)
    V = h.shape[2]
    wp = next((c for c in SUPPORTED_W if w <= c), None)
    if wp is None:
        raise ValueError("attention: feature width %d too large (max %d)" % (w, SUPPORTED_W[-1]))
    F = {1: 3, 2: 2, 3: 4}[simiMatrix]
    W = _pad_channels(_f32(W).reshape(F, w), wp).reshape(-1).contiguous()
    ops.require_gpu()
    both = hinfo_mask is not None and hq_mask is not None
    hm = ops.as_mask_u8(hinfo_mask.reshape(N, M, V)) if both else None
    qm = ops.as_mask_u8(hq_mask) if both else None
    u, a = autograd.keeprank1(_pad_channels(h, wp), _pad_channels(hq, wp), W, _f32(b), hm, qm, simiMatrix,
                              want_logits=bool(bidirect))
    u = u[..., :w].contiguous()
    if bidirect:                                                            # model.py:297-307 -> [N,M,2w]
        u = torch.cat([u, _bidirect_q_a(a, hq, (N, M))], 2)
    return u


def attention_keeprank1(hinfo, hq, hinfo_mask=None, hq_mask=None, simiMatrix=1, wd=None, bidirect=False, scope=None):
    """model.py:247-314: hinfo [N,M,...,w] -> h_a [N,M,w] ([N,M,2w] with `bidirect`), each album attended on its own (softsel over the rows of
    (n, m) with the max-over-question logits; no softmax over m).  That is the inner stage of attention_3d with K = M:
    one fvta_attn_fwd, then the per-(n,k) result is read back out of the saved state; its gradient runs through
    fvta_attn_bwd_u, every (n,m) an attention of its own.  model.py's feature order for simiMatrix 2 is
    [(h-q)^2, h*q] (feat_order 1); no tanh on the logits."""
    if simiMatrix not in (1, 2, 3):
        raise ValueError("similarity matrix not implemented")              # model.py:283-285 (sys.exit there)
    w = hinfo.shape[-1]
    F = {1: 3, 2: 2, 3: 4}[simiMatrix]
    with variable_scope(scope or "attention_2vector"):
        wn, bn = _name("att_logits", "W"), _name("att_logits", "b")
        W = get_variable(wn, (F * w, 1))
        b = get_variable(bn, (1,), init="zeros")
        _add_wd([wn, bn], wd)
    return attention_keeprank1_raw(hinfo, hq, W, b, hinfo_mask, hq_mask, simiMatrix, bidirect)


def attention_tgif(hinfo, lq, hinfo_mask=None, wd=None, mlp_dim=512, scope=None):
    """model.py:210-244 (the TGIF-QA attention baseline): score = linear(linear(lq)[:,None] + linear(hinfo)) ->
    softmax over the rows -> exp_mask applied to the PROBABILITIES (as the reference does: masked rows get weight
    -1e30, harmless only because their h is 0) -> weighted sum -> tanh(linear) + lq.  Returns (logits [N,2*mlp_dim],
    att [N,V]); needs lq.shape[-1] == 2 * mlp_dim like the reference's tf.add."""
    hinfo, lq = _f32(hinfo), _f32(lq)
    N, w = hinfo.shape[0], hinfo.shape[-1]
    h = hinfo.reshape(N, -1, w)
    V = h.shape[1]
    with variable_scope(scope or "attention_2vector"):
        q_in = linear(lq, mlp_dim, scope="mlp_q", wd=None)
        h_in = linear(h, mlp_dim, scope="mlp_h", wd=None)
        preatt = (h_in + q_in[:, None, :]).contiguous()                      # tf.tile + tf.add (plumbing)
        score = linear(preatt, 1, scope="preatt").reshape(N, V)
        att = softmax(score)
        if hinfo_mask is not None:
            att = exp_mask(att, hinfo_mask.reshape(N, V))
        attended = _wsum(h, att)
        final = linear(attended, 2 * mlp_dim, scope="final", add_tanh=True)
        if wd is not None:                                                    # add_wd over the whole scope (:241-242)
            _add_wd([n for n in variables if n.startswith(_name("") )], wd)
    return final + lq, att


# ------------------------------------------------------------------ context tensor (model_v2.py:863-914)
def context_tensor(streams, masks=None):
    """The 12 tf.pad + 2 tf.stack of model_v2.py:863-914 as one library call each way: streams, a list of K <= 8 tensors
    [N,M,J_k,w] (the caller reshapes hpts to [N,M,JI*JXP,w], :886), masks a list of K [N,M,J_k] bool / u8 or None ->
    (hall [N,K,M,JMAX,w], hall_mask [N,K,M,JMAX] bool, or None without masks); JMAX = max_k J_k, rows j >= J_k are zeros /
    False.  Rows are copied whatever their mask bit says, as tf.pad does.  The K order is the caller's (the reference's:
    at, ad, when, where, pts, pis, :910).  The gradient of hall is sliced back into the streams that require one."""
    streams = list(streams)
    K = len(streams)
    if not 1 <= K <= _lib.CTX_KMAX:
        raise ValueError("context_tensor: K = %d streams (1..%d)" % (K, _lib.CTX_KMAX))
    if any(s.dim() != 4 for s in streams):
        raise ValueError("context_tensor: every stream is [N,M,J_k,w]")
    N, M, _, w = streams[0].shape
    for k, s in enumerate(streams):
        if (s.shape[0], s.shape[1], s.shape[3]) != (N, M, w) or s.shape[2] < 1:
            raise ValueError("context_tensor: stream %d is %s, stream 0 is %s: N, M and w must agree and J_k >= 1"
                             % (k, tuple(s.shape), tuple(streams[0].shape)))
    if masks is not None:
        masks = list(masks)
        if len(masks) != K:
            raise ValueError("context_tensor: %d masks for %d streams" % (len(masks), K))
        for k, (m, s) in enumerate(zip(masks, streams)):
            if tuple(m.shape) != tuple(s.shape[:3]):
                raise ValueError("context_tensor: mask %d is %s, its stream %s" % (k, tuple(m.shape), tuple(s.shape)))
    ops.require_gpu()
    return autograd.context_tensor([_f32(s) for s in streams], None if masks is None else [ops.as_mask_u8(m) for m in masks])


# ------------------------------------------------------------------ time warp (model_v2.py:301-341, 953-1009)
_WARP_TYPES = (1, 2, 3, 4, 5)


def _check_warp_type(warp_type):
    if warp_type not in _WARP_TYPES:
        raise Exception("time warping type not implemented")                # model_v2.py:341


def time_warp_raw(hall, lq, WH_W, WH_b, WC_W, WC_b, warp_type=1, window_t=3.0):
    """The time warp with explicit weights: hall [N,K,M,JX,w] or [N,K,T,w], lq [N,w], WH_W [2w,w], WH_b [w], WC_W [w,1],
    WC_b [1] -> (warp_h in hall's shape, scale [N,T] = c[n,t] cnt(t), the row sums of the reference's windowed C).  The
    kernels take w % 4 == 0; another width is zero padded here (exact: the padded channels of WH, WH_b, WC and lq are
    zero) and sliced back, with differentiable torch ops."""
    _check_warp_type(warp_type)
    hall, lq = _f32(hall), _f32(lq)
    shape, w = hall.shape, hall.shape[-1]
    N, K = shape[0], shape[1]
    wp = (w + 3) // 4 * 4
    h = hall.reshape(N, K, -1, w)
    WH_W, WH_b, WC_W = _f32(WH_W), _f32(WH_b), _f32(WC_W).reshape(w)
    if wp != w:
        pad = torch.nn.functional.pad
        h, lq, WH_b, WC_W = pad(h, (0, wp - w)), pad(lq, (0, wp - w)), pad(WH_b, (0, wp - w)), pad(WC_W, (0, wp - w))
        WH_W = pad(WH_W.reshape(2, w, w), (0, wp - w, 0, wp - w)).reshape(2 * wp, wp)
    warp_h, scale = autograd.time_warp(h, lq, WH_W, WH_b, WC_W, _f32(WC_b), warp_type, float(window_t))
    if wp != w:
        warp_h = warp_h[..., :w]
    return warp_h.reshape(shape), scale


def time_warp(hall, lq, warp_type=1, window_t=None, scope=None):
    """model_v2.py:953-1009: hall [N,K,M,JX,w] or [N,K,T,w], lq [N,w] -> (warp_h in hall's shape, scale [N,T]).  The
    variables WH/W [2w,w], WH/b [w], WC/W [w,1], WC/b [1] live below `scope or "time_warp"` (truncated normal 0.1 / zeros);
    for warp_type 5 the window is time_warp_C/time_warp_window_t, a 0-d tensor initialised to 3.0 and used when `window_t`
    is None (it never receives a gradient: tf.ceil, :335).  `scale` is what attention_3d(time_warp_att=True, C=scale)
    takes in place of the reference's C [N,T,T]."""
    _check_warp_type(warp_type)
    w = hall.shape[-1]
    with variable_scope(scope or "time_warp"):
        WH_W = get_variable(_name("WH", "W"), (2 * w, w))
        WH_b = get_variable(_name("WH", "b"), (w,), init="zeros")
        WC_W = get_variable(_name("WC", "W"), (w, 1))
        WC_b = get_variable(_name("WC", "b"), (1,), init="zeros")
        if warp_type == 5:
            wn = _name("time_warp_C", "time_warp_window_t")
            if wn not in variables:
                variables[wn] = torch.full((), 3.0, dtype=torch.float32, device=ops.require_gpu())
            if window_t is None:
                window_t = float(variables[wn])
    return time_warp_raw(hall, lq, WH_W, WH_b, WC_W, WC_b, warp_type, 3.0 if window_t is None else float(window_t))


_bands = {}      # (T, warp_type, win, device) -> the 0/1 band [T,T], built once


def time_indication_func(C, warp_type=1, window_t=3.0):
    """model_v2.py:301-341: C [N,T,T] times the 0/1 indicator of the warp type (1 all, 2 current, 3 past, 4 future, 5 a
    window of ceil(window_t) either side) -> (C_windowed, window_t for type 5 | None).  One fvta_wsum_fwd over the
    elements (J = d = 1: a product) with the band, built once per (T, warp_type, window); differentiable in C.  It
    exists for code written against the reference's signature -- the [N,T] path (time_warp's `scale`) needs no C."""
    import math
    _check_warp_type(warp_type)
    C = _f32(C)
    N, T = C.shape[0], C.shape[-1]
    dev = ops.require_gpu()
    win = int(math.ceil(float(window_t))) if warp_type == 5 else 0
    key = (T, warp_type, win, str(C.device))
    if key not in _bands:
        ones = torch.ones(T, T, dtype=torch.float32)
        band = {1: ones, 2: torch.eye(T), 3: torch.tril(ones), 4: torch.triu(ones),
                5: torch.triu(torch.tril(ones, win), -win)}[warp_type]
        _bands[key] = band.to(C.device)
    band = _bands[key][None].expand(N, T, T).reshape(-1, 1)
    out = autograd.wsum(C.reshape(-1, 1, 1), band).reshape(N, T, T)
    return out, (window_t if warp_type == 5 else None)


# ------------------------------------------------------------------ DMN+ episodic memory (model_dmnplus.py:89-136, 503-516)
_CELL_VARS = (("gates/weights", lambda d: (2 * d, d)), ("gates/biases", lambda d: (d,)), ("candidate/weights", lambda d: (d, d)),
              ("input/weights", lambda d: (d, d)), ("input/biases", lambda d: (d,)))


def get_attention_raw(q_vec, prev_memory, fact_vecs, W1, b1, W2, b2):
    """model_dmnplus.py:89-111 for ALL facts at once with explicit fc1 / fc2 variables: facts [N,F,d] -> logits [N,F].
    Differentiable in the facts, the question, the memory and the four variables."""
    N, F, d = fact_vecs.shape
    feats = autograd.dmn_features(fact_vecs, q_vec, prev_memory)
    a1 = linear_raw(feats, W1, b1, add_tanh=True)
    return linear_raw(a1, W2, b2).reshape(N, F)


def generate_episode_raw(memory, q_vec, fact_vecs, fact_vecs_length, att_vars, cell_vars):
    """model_dmnplus.py:113-136 with explicit variables: att_vars = (fc1 W, fc1 b, fc2 W, fc2 b), cell_vars = (gates W,
    gates b, candidate W, input W, input b).  The ONE episode of the library: generate_episode, episodic_memory,
    nn.EpisodicMemory and dmn.EpisodicMemory all run it."""
    fact_vecs = _f32(fact_vecs)
    N, F, d = fact_vecs.shape
    att = softmax(get_attention_raw(q_vec, memory, fact_vecs, *att_vars))                     # [N,F], over ALL facts (:120)
    live = (torch.arange(F, device=att.device)[None, :] < torch.as_tensor(fact_vecs_length).to(att.device)[:, None])
    g = _wsum(att.reshape(N * F, 1, 1), live.to(torch.float32).reshape(N * F, 1)).reshape(N, F)   # att * (t < length)
    return autograd.attgru_seq(fact_vecs, g, None, *cell_vars)                                # dynamic_rnn, zero state (:127-131)


def episodic_memory_raw(gq, facts, facts_length, att_vars, cell_vars, hop_vars):
    """model_dmnplus.py:503-516, the ONE hop loop of the library: hop_vars = [(kernel [3d,d], bias [d])] per hop."""
    prev = gq = _f32(gq)
    for kernel, bias in hop_vars:
        episode = generate_episode_raw(prev, gq, facts, facts_length, att_vars, cell_vars)
        prev = autograd.relu(linear_raw(torch.cat([prev, episode, gq], 1), kernel, bias))     # :510-514
    return prev


def _get_attention(q_vec, prev_memory, fact_vecs, hidden_size):
    """model_dmnplus.py:89-111 for ALL facts at once (the reference unstacks the facts and reuses the two
    fully_connected layers): facts [N,F,d] -> attention logits [N,F].  Variables attention/fc1/{weights,biases}
    (tanh), attention/fc2/{weights,biases} (tf.contrib.layers.fully_connected: Glorot weights, zero biases)."""
    return get_attention_raw(_f32(q_vec), _f32(prev_memory), _f32(fact_vecs), *_attention_vars(fact_vecs.shape[2], hidden_size))


def _attention_vars(d, hidden_size):
    with variable_scope("attention"):
        W1 = get_variable(_name("fc1", "weights"), (4 * d, hidden_size), init="glorot")
        b1 = get_variable(_name("fc1", "biases"), (hidden_size,), init="zeros")
        W2 = get_variable(_name("fc2", "weights"), (hidden_size, 1), init="glorot")
        b2 = get_variable(_name("fc2", "biases"), (1,), init="zeros")
    return W1, b1, W2, b2


def _cell_vars(d):
    with variable_scope("attention_gru"):
        return tuple(get_variable(_name("attention_gru_cell", n_), sh(d), init="zeros" if n_.endswith("biases") else "glorot")
                     for n_, sh in _CELL_VARS)


def generate_episode(memory, q_vec, fact_vecs, fact_vecs_length, hop_index, hidden_size, scope=None):
    """model_dmnplus.py:113-136 `_generate_episode`: attention over the facts from (question, previous memory), softmax
    over ALL F facts (no mask in the reference), then the AttentionGRUCell (attention_gru_cell.py:50-70) run by
    dynamic_rnn over the facts with sequence_length: the state is carried past a row's length -- which the cell does by
    itself when the attention gate is 0, so the gates of steps >= length are zeroed.  Returns the episode [N,d],
    differentiable in the facts, the question, the memory and the nine variables (autograd.dmn_features, .attgru_seq).
    Variables live under the current scope (hop_index > 0 reuses them, as the reference's reuse flags do)."""
    d = fact_vecs.shape[2]
    with variable_scope(scope):
        att_vars = _attention_vars(d, hidden_size)
        cell_vars = _cell_vars(d)
    return generate_episode_raw(memory, q_vec, fact_vecs, fact_vecs_length, att_vars, cell_vars)


def episodic_memory(gq, facts, facts_length, num_hops, hidden_size, scope="memory"):
    """model_dmnplus.py:503-516: prev_memory = gq; per hop, episode = generate_episode(prev_memory, gq, facts, ...) and
    prev_memory = relu(dense(concat([prev_memory, episode, gq], 1), hidden_size)) with its own `hop_<i>/dense/{kernel,
    bias}` (tf.layers.dense: Glorot / zeros); the attention MLP and the AttentionGRU are shared by the hops.  gq [N,d],
    facts [N,F,d], facts_length [N] -> [N,hidden_size], differentiable in everything."""
    d = facts.shape[2]
    with variable_scope(scope):
        att_vars = _attention_vars(d, hidden_size)
        cell_vars = _cell_vars(d)
        hop_vars = [(get_variable(_name("hop_%d" % i, "dense", "kernel"), (3 * d, hidden_size), init="glorot"),
                     get_variable(_name("hop_%d" % i, "dense", "bias"), (hidden_size,), init="zeros")) for i in range(int(num_hops))]
    return episodic_memory_raw(gq, facts, facts_length, att_vars, cell_vars, hop_vars)


# ------------------------------------------------------------------ MCB (model_mcb.py:623-681, 1254-1363)
_SKETCH_CACHE = {}


def sketch_tables(d1, d2, D, rand_h_1=None, rand_s_1=None, rand_h_2=None, rand_s_2=None, seeds=(1, 3, 5, 7)):
    """The layer's four tables on the device: those the reference draws from `seeds` (ops.count_sketch_tables), each
    replaced by the caller's own where one is given; validated on the host, uploaded, and kept per (sizes, seeds) when all
    four are drawn."""
    given = (rand_h_1, rand_s_1, rand_h_2, rand_s_2)
    key = (int(d1), int(d2), int(D), tuple(int(s) for s in seeds), torch.cuda.current_device())
    if all(t is None for t in given) and key in _SKETCH_CACHE:
        return _SKETCH_CACHE[key]
    drawn = ops.count_sketch_tables(d1, d2, D, seeds)
    tabs = ops.upload_sketch_tables(*(dr if t is None else t for t, dr in zip(given, drawn)), d1, d2, D)
    if all(t is None for t in given):
        _SKETCH_CACHE[key] = tabs
    return tabs


def compact_bilinear_pooling_layer(bottom1, bottom2, output_dim, sum_pool=True, rand_h_1=None, rand_s_1=None, rand_h_2=None,
                                   rand_s_2=None, seed_h_1=1, seed_s_1=3, seed_h_2=5, seed_s_2=7, sequential=True,
                                   compute_size=128):
    """model_mcb.py:1254-1363 with the reference's signature: bottom1 [B,H,W,d1], bottom2 [B,H,W,d2] (one row of it per
    position) or [B,1,1,d2] (one row per b, shared by its H*W positions: what the model's tiled question is) ->
    [B,H,W,output_dim], or its sum over H and W [B,output_dim] with sum_pool (a torch sum).  The count sketch of the outer
    product in exact fp32 (autograd.compact_bilinear), where the reference goes through FFTs; `sequential` and
    `compute_size` steer those FFTs and are accepted and ignored.  Differentiable in both bottoms."""
    if bottom1.dim() != 4 or bottom2.dim() != 4:
        raise ValueError("compact_bilinear_pooling_layer: bottoms must be [B,H,W,d], got %s and %s" % (tuple(bottom1.shape), tuple(bottom2.shape)))
    tabs = sketch_tables(bottom1.shape[-1], bottom2.shape[-1], output_dim, rand_h_1, rand_s_1, rand_h_2, rand_s_2,
                         (seed_h_1, seed_s_1, seed_h_2, seed_s_2))
    return compact_bilinear_pooling_raw(bottom1, bottom2, tabs, output_dim, sum_pool=sum_pool)


def compact_bilinear_pooling_raw(bottom1, bottom2, tables, output_dim, sum_pool=True, normalize=False):
    """compact_bilinear_pooling_layer with explicit device tables (h1, s1, h2, s2); normalize fuses the
    l2_normalize(sqrt|.|) of model_mcb.py:645 behind the un-pooled rows"""
    B, H, W, d1 = bottom1.shape
    d2 = bottom2.shape[-1]
    if tuple(bottom2.shape[:3]) == (B, H, W):
        P = 1
    elif tuple(bottom2.shape[:3]) == (B, 1, 1):
        P = H * W
    else:
        raise ValueError("compact_bilinear_pooling_layer: bottom2 %s fits neither [%d,%d,%d,d2] nor [%d,1,1,d2]"
                         % (tuple(bottom2.shape), B, H, W, B))
    cbp = autograd.compact_bilinear(bottom1.reshape(B * H * W, d1), bottom2.reshape(-1, d2), *tables, int(output_dim), P=P,
                                    normalize=normalize)
    cbp = cbp.reshape(B, H, W, int(output_dim))
    return cbp.sum((1, 2)) if sum_pool else cbp


def mcb_attention_raw(hpis, gq, tables, filter_conv1, filter_conv2):
    """model_mcb.py:628-672 with explicit variables: hpis [N,M,JI,idim] (the raw photo rows), gq [N,2d] (the question's
    last state), tables = (h1, s1, h2, s2) on the device, filter_conv1 [D,c1], filter_conv2 [c1,1] (the 1x1 convolutions
    are linears without a bias) -> (attended [N,idim], att [N, M*JI]).  The pooled rows are normalised inside the op
    (l2_normalize(sqrt|.|), never stored un-normalised), relu(linear) twice, a softmax over ALL M*JI positions (unmasked,
    as in the reference) and the weighted sum of hpis: every product is a library call, the reshapes are torch.
    Left out: the tf.nn.dropout of :649 and the forward NaN scrubs of :635 / :646 (inputs are taken to be finite; the one
    0/0 the graph can produce, a zero bucket under the square root's gradient, is defined as 0)."""
    hpis, gq = _f32(hpis), _f32(gq)
    N, M, JI, idim = hpis.shape
    T = M * JI
    D = filter_conv1.shape[0]
    rows = hpis.reshape(N * T, idim)
    g_mcb = autograd.compact_bilinear(rows, gq, *tables, D, P=T, normalize=True)                # [N*T, D]  (:641-645)
    c1 = autograd.relu(linear_raw(g_mcb, filter_conv1, None))                                   # [N*T, c1] (:658)
    c2 = autograd.relu(linear_raw(c1, filter_conv2, None))                                      # [N*T, 1]  (:664)
    att = softmax(c2.reshape(N, T))                                                             # (:666)
    return _wsum(hpis.reshape(N, T, idim), att), att                                            # (:672)
