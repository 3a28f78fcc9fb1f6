"""What the album attention's kernels compute, restated by hand ONCE for both forms of the family -- shared context
(fvta_attn_shared_*: album [NQ] over h [A,K,T,w]) and album pool (fvta_attn_pool_*: albums [NQ,M] over pool [P,K,JX,w]) --
unwarped and under the time warp, forward and backward.

Everything here is written over the POOLED description of a case: pool [P,K,JX,w], pm [P,K,JX] or None, albums [NQ,M]
with -1 for an empty slot, question i attending its albums' rows laid end to end, T = M JX.  A shared case is the pooled
one at M = 1 -- the claim fvta_memexqa_amd/csrc/attn_pool.hip makes of every launch ("at M = 1 the same bits as the
shared call") -- and `as_pooled` presents it as such by views, `as_shared` maps the result keys back, `shared(fn)` does
both around fn.  tests/test_album_attn_ref_host.py pins that claim on the two DEFINITIONS.

The definitions (`reference`: fp64 oracle.fvta_fused on h[album] / on expand(c), autograd for the gradients), the shapes,
the input recipes and the pinned seeds stay with their families in tests/_attn_{shared,pooled,pool}*_ref.py; nothing here
reads them, and they do not go through the restatements below -- the host tests hold the two against each other."""
import math

import torch

NEG = -1e30
GAP = 1e-5                                   # the arg-max conditions of the training cases: `conditions`
SAT_X, SAT_FRACTION = 0.99, 0.05
# forward, (rtol, atol): tests/test_gpu_attn_shared.py's
TOL = dict(h_a=(1e-4, 1e-5), a_logits=(1e-4, 2e-5), scale=(1e-4, 1e-5))
# gradients, (rtol, atol x max(1, max|ref|)): tests/test_gpu_attn_shared_bwd.py's for the attention's,
# tests/test_gpu_timewarp.py's for the warp's
GRAD_TOL = dict(dh=(1e-4, 1e-5), dq=(1e-4, 1e-5), dW=(1e-4, 1e-5), db=(1e-4, 1e-5),
                dlq=(2e-4, 2e-5), dWH_W=(2e-4, 2e-5), dWH_b=(2e-4, 2e-5), dWC_W=(2e-4, 2e-5), dWC_b=(2e-4, 2e-5))


# ------------------------------------------------------------------ shared = pooled at M = 1
def as_pooled(c):
    """the shared case c (h, hm, album [NQ], A, T) as a pooled one: the same tensors, viewed"""
    return dict(c, pool=c["h"], pm=c["hm"], albums=c["album"][:, None], P=c["A"], M=1, JX=c["T"])


def as_shared(out):
    """a pooled result dict under the shared family's keys"""
    return {{"dpool": "dh"}.get(k, k): v for k, v in out.items()}


def shared(fn):
    """fn, one of the restatements below, for the shared family: it takes a shared case and answers under its keys"""
    def on_shared(c, *args, **kwargs):
        out = fn(as_pooled(c), *args, **kwargs)
        return as_shared(out) if isinstance(out, dict) else out
    return on_shared


# ------------------------------------------------------------------ small things
def _dd(t):
    return None if t is None else t.double()


def _softmax_last(x):
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def _unit(X):
    return X / torch.sqrt(torch.clamp((X * X).sum(1, keepdim=True), min=1e-12))


def within(got, want, key):
    """|got - want| <= atol + rtol |want| at `key`'s GPU tolerance, atol x max(1, max|want|) for a gradient
    -> (ok, worst ratio)"""
    key = {"dpool": "dh"}.get(key, key)
    rtol, atol = TOL[key] if key in TOL else GRAD_TOL[key]
    got, want = got.detach().cpu().double(), want.double()
    if key in GRAD_TOL:
        atol = atol * max(1.0, float(want.abs().max()))
    ratio = ((got - want).abs() / (atol + rtol * want.abs())).max()
    return bool(ratio <= 1.0), float(ratio)


def seed_candidates(name, offset, n):
    base = sum(map(ord, name)) * 10 + offset
    return [base + i for i in range(n)]


def train_inputs(c, pm, tanh, parity=True):
    """The training recipe on a freshly made case, in place: att_logits/W scaled by sqrt(64 / w) (the logits stay clear of
    tanh's saturation at every width), d_h_a = randn of seed 99 and -- parity, as tests/test_gpu_backward.py -- every
    (album, k) of the mask pm and every question partly valid (the fully masked ones carry fvta_attn_bwd's documented
    deviation).  An empty slot and a question that lists nothing stay what they are."""
    c["W"] = c["W"] * (64.0 / c["w"]) ** 0.5
    c["tanh"] = tanh
    if pm is not None and parity:
        pm[0, 0, :3] = True
        if c["NQ"] > 1:
            c["qm"][c["NQ"] - 1, :2] = True
        pm[:, :, 0] |= ~pm.any(-1)                  # (a short row count can leave further (album, k) without a valid row)
    c["gout"] = torch.randn(c["NQ"], c["w"], generator=torch.Generator().manual_seed(99))
    return c


def bilinear_split(W, w, simi):
    """att_logits/W [F] as (Rh, Cq, U, R2): logit = h . (q U) + h . Rh + h^2 . R2 + q . Cq + q^2 . R2 + b"""
    zero = torch.zeros(w, dtype=W.dtype)
    if simi == 1:            # [h, q, h*q] . W
        return W[:w], W[w:2 * w], W[2 * w:], zero
    if simi == 2:            # [h*q, (h-q)^2] . W
        return zero, zero, W[:w] - 2 * W[w:], W[w:]
    return W[:w], W[w:2 * w], W[3 * w:] - 2 * W[2 * w:3 * w], W[2 * w:3 * w]      # [h, q, (h-q)^2, h*q] . W


# ------------------------------------------------------------------ the time warp's scalars
def count(T, warp_type, window_t, dtype):
    """cnt [T]: how many positions the warp sums at each position"""
    t = torch.arange(T)
    if warp_type == 1:
        n = torch.full((T,), T)
    elif warp_type == 2:
        n = torch.ones(T, dtype=torch.int64)
    elif warp_type == 3:
        n = t + 1
    elif warp_type == 4:
        n = T - t
    else:
        win = int(math.ceil(window_t))
        n = torch.clamp(t + win, max=T - 1) - torch.clamp(t - win, min=0) + 1
    return n.to(dtype)


def count_of(c, dtype=torch.float64):
    """cnt [M JX]: the count of the GLOBAL position -- a band, past or future crosses slot boundaries"""
    return count(c["T"], c["warp_type"], c["window_t"], dtype)


def cmax(T, warp_type, window_t):
    """the largest count of the warp: the factor the rows can grow by"""
    if warp_type == 2:
        return 1
    if warp_type == 5:
        return 2 * int(math.ceil(window_t)) + 1
    return T


def energy(c, dtype=torch.float64):
    """e [P,JX] = sum_k sum_c v[c] pool[p,k,j,c]^2, v = WH[:w] WC: per pooled album"""
    w = c["w"]
    v = c["WH_W"].to(dtype)[:w] @ c["WC_W"].to(dtype).reshape(w)
    h = c["pool"].to(dtype)
    return ((h * h) @ v).sum(1)


def _slots(c):
    """albums [NQ,M] with P in place of -1: an index into a table that ends with an empty slot's row"""
    al = c["albums"]
    return torch.where(al >= 0, al, torch.full_like(al, c["P"]))


def scale_of(c, dtype=torch.float64):
    """scale [NQ, M JX]: the pooled albums' energies gathered per slot (an empty slot: 0), the count of the GLOBAL position"""
    cv = lambda t: t.to(dtype)
    K, w = c["K"], c["w"]
    WC = cv(c["WC_W"]).reshape(w)
    s0 = cv(c["WH_b"]) @ WC + cv(c["WC_b"])[0]
    e = torch.cat([energy(c, dtype), torch.zeros(1, c["JX"], dtype=dtype)])     # row P: an empty slot's
    z = e[_slots(c)].reshape(c["NQ"], c["T"]) + K * (s0 + cv(c["lq"]) @ WC)[:, None]
    return torch.tanh(z) * count_of(c, dtype)[None, :]


# ------------------------------------------------------------------ the forward in kernel order
def _references(c):
    """per pooled album with a reference: (p, questions [nref], slots [nref])"""
    for p in range(c["P"]):
        ref = torch.nonzero(c["albums"] == p)                              # [nref, 2]: (question, slot)
        if ref.shape[0]:
            yield p, ref[:, 0], ref[:, 1]


def _scatter(c, logits, p, qi, mi, x):
    """the block x [nref,K,JX,JQ] of album p's references, masked by select, to its slots' positions"""
    JX = c["JX"]
    if c["pm"] is not None and c["qm"] is not None:
        valid = c["pm"][p][None, :, :, None] & c["qm"][qi][:, None, None, :]
        x = torch.where(valid, x, torch.full_like(x, NEG))
    for r in range(qi.numel()):
        logits[qi[r], :, mi[r] * JX:(mi[r] + 1) * JX] = x[r]


def _attend(c, pool, logits, scale=None):
    """the two softmaxes by hand and the weighted sum slot by slot (an empty slot: zero rows); under the warp the weight
    carries the scale -> h_a [NQ,w]"""
    al, JX = c["albums"], c["JX"]
    assert not torch.isnan(logits).any()                                   # open: every slot was written
    amax = logits.max(-1).values                                           # [NQ,K,T]
    pt = _softmax_last(amax) if scale is None else _softmax_last(amax) * scale[:, None, :]
    u = torch.zeros(c["NQ"], c["K"], c["w"], dtype=pool.dtype)
    for i in range(c["NQ"]):
        for m in range(c["M"]):
            p = int(al[i, m])
            if p >= 0:
                u[i] += torch.einsum("kt,ktc->kc", pt[i, :, m * JX:(m + 1) * JX], pool[p])
    r = _softmax_last(amax.max(-1).values)                                 # [NQ,K]
    return torch.einsum("gk,gkc->gc", r, u)


def _empty_logits(c, dtype):
    masked = c["pm"] is not None and c["qm"] is not None
    return torch.full((c["NQ"], c["K"], c["T"], c["JQ"]), NEG if masked else float("nan"), dtype=dtype)


def grouped(c, tanh):
    """fp64, album by album: ONE [K JX, w] x [w, nref JQ] product for all (question, slot) references to the album, written
    out from att_logits/W per similarity form (not through the oracle's helpers), scattered to their slots
    -> (h_a [NQ,w], a_logits [NQ,K,T,JQ])"""
    pool, q, simi = _dd(c["pool"]), _dd(c["q"]), c["simi"]
    K, JX, JQ, w = c["K"], c["JX"], c["JQ"], c["w"]
    if simi != 4:
        Rh, Cq, U, R2 = bilinear_split(_dd(c["W"]).reshape(-1), w, simi)
        b = float(c["b"])
    logits = _empty_logits(c, torch.float64)
    for p, qi, mi in _references(c):
        nref = qi.numel()
        H = pool[p].reshape(K * JX, w)
        Q = q[qi].reshape(nref * JQ, w)
        if simi == 4:        # cosine
            x = _unit(H) @ _unit(Q).t()
        else:
            x = (H * U) @ Q.t() + (H @ Rh + (H * H) @ R2)[:, None] + (Q @ Cq + (Q * Q) @ R2)[None, :] + b
            if tanh:
                x = torch.tanh(x)
        _scatter(c, logits, p, qi, mi, x.reshape(K, JX, nref, JQ).permute(2, 0, 1, 3))
    return _attend(c, pool, logits), logits


def factored(c, dtype=torch.float64):
    """The warped forward the kernels compute, in `dtype`: the warp as one scalar per (question, global position m JX + j)
    whose only term that reads the rows -- the energy -- is taken per POOLED ALBUM; the scalar passed through the bilinear
    form of the logits and through the weighted sum; no [NQ,K,T,w] tensor -> (h_a, a_logits, scale)"""
    cv = lambda t: None if t is None else t.to(dtype)
    pool, q, simi = cv(c["pool"]), cv(c["q"]), c["simi"]
    K, JX, JQ, w = c["K"], c["JX"], c["JQ"], c["w"]
    scale = scale_of(c, dtype)
    if simi != 4:
        Rh, Cq, U, R2 = bilinear_split(cv(c["W"]).reshape(-1), w, simi)
        b = cv(c["b"])[0]
    logits = _empty_logits(c, dtype)
    for p, qi, mi in _references(c):
        nref = qi.numel()
        H = pool[p].reshape(K * JX, w)
        Q = q[qi].reshape(nref * JQ, w)
        pos = mi[:, None] * JX + torch.arange(JX)[None, :]                # [nref,JX]: the references' global positions
        s = torch.gather(scale[qi], 1, pos)[:, None, :].expand(nref, K, JX)
        if simi == 4:
            dot = (H @ _unit(Q).t()).reshape(K, JX, nref, JQ).permute(2, 0, 1, 3)
            n2 = (H * H).sum(1).reshape(K, JX)[None]
            x = dot * (s / torch.sqrt(torch.clamp(s * s * n2, min=1e-12)))[..., None]
        else:
            dot = (H @ (Q * U).t()).reshape(K, JX, nref, JQ).permute(2, 0, 1, 3)
            ct = ((Q @ Cq + (Q * Q) @ R2) + b).reshape(nref, JQ)
            r1, r2 = (H @ Rh).reshape(K, JX)[None], ((H * H) @ R2).reshape(K, JX)[None]
            x = s[..., None] * (dot + r1[..., None]) + (s * s * r2)[..., None] + ct[:, None, None, :]
            if c["tanh"]:
                x = torch.tanh(x)
        _scatter(c, logits, p, qi, mi, x)
    return _attend(c, pool, logits, scale), logits, scale


# ------------------------------------------------------------------ the warped backward by hand
def factored_backward(c, dtype=torch.float64):
    """The warped forward and backward from the formulas the kernels implement, in `dtype`: no autograd, no [NQ,K,T,w]
    tensor.  Per question on its albums' rows, read from the pool slot by slot: the gradient of the scale s per (question,
    k, position) from lin at the winning column and r2; the row gradient goes back to the pool by reference; dz [NQ,M JX]
    with the count of the GLOBAL position and zero at an empty slot; de [P,JX] per pooled album over its references;
    d_pool += 2 de v h; dv and the parameter gradients from there -> dict(h_a, a_logits, scale, dpool, dq, dlq, dW [F],
    db [1], dWH_W [2w,w], dWH_b, dWC_W [w], dWC_b, dz, de, and db_pooled: db as the kernels take it, -sum damax x^2)"""
    cv = lambda x: x.to(dtype)
    pool, q, lq, g, al = cv(c["pool"]), cv(c["q"]), cv(c["lq"]), cv(c["gout"]), c["albums"]
    simi, tanh = c["simi"], c["tanh"]
    Pn, K, JX, w = pool.shape
    NQ, JQ = q.shape[:2]
    M, T = c["M"], c["T"]
    Rh, Cq, U, R2 = bilinear_split(cv(c["W"]).reshape(-1), w, simi)
    b = cv(c["b"])[0]
    WH, WHb, WC, WCb = cv(c["WH_W"])[:w], cv(c["WH_b"]), cv(c["WC_W"]).reshape(w), cv(c["WC_b"])[0]
    v = WH @ WC
    s0 = WHb @ WC + WCb
    e = torch.cat([((pool * pool) @ v).sum(1), torch.zeros(1, JX, dtype=dtype)])      # [P + 1,JX]; row P: an empty slot's
    cnt = count_of(c, dtype)
    tz = torch.tanh(e[_slots(c)].reshape(NQ, T) + K * (s0 + lq @ WC)[:, None])         # [NQ,T]
    s_all = tz * cnt[None, :]
    live = (al >= 0)[:, :, None].expand(NQ, M, JX).reshape(NQ, T)                      # positions of a non-empty slot
    valid = valid_mask(c) if c["pm"] is not None and c["qm"] is not None else None
    zrows = torch.zeros(K, JX, w, dtype=dtype)
    dpool, dq, dz = torch.zeros_like(pool), torch.zeros_like(q), torch.zeros(NQ, T, dtype=dtype)
    h_a, logits = torch.zeros(NQ, w, dtype=dtype), torch.zeros(NQ, K, T, JQ, dtype=dtype)
    dRh, dR2, dU, dCq, dC2 = (torch.zeros(w, dtype=dtype) for _ in range(5))
    db, db_pooled = torch.zeros(1, dtype=dtype), torch.zeros(1, dtype=dtype)
    for i in range(NQ):
        row = al[i].tolist()
        H = torch.cat([pool[p] if p >= 0 else zrows for p in row], 1)             # [K,T,w]: read, never kept
        Q, gi, s = q[i], g[i], s_all[i][None, :]                                  # [JQ,w], [w], [1,T]
        Qs = Q * U
        lin = H @ Qs.t() + (H @ Rh)[..., None]                                    # [K,T,JQ]
        r2 = (H * H) @ R2                                                         # [K,T]
        ct = Q @ Cq + (Q * Q) @ R2 + b
        x = s[..., None] * lin + (s * s * r2)[..., None] + ct
        if tanh:
            x = torch.tanh(x)
        if valid is not None:
            x = torch.where(valid[i], x, torch.full_like(x, NEG))
        logits[i] = x
        amax, jmax = x.max(-1)                                                    # [K,T]
        Mk = amax.max(-1).values                                                  # [K]
        ex = torch.exp(amax - Mk[:, None])
        p_ = ex / ex.sum(-1, keepdim=True)
        u = torch.einsum("kt,ktc->kc", p_ * s, H)
        r = torch.softmax(Mk, 0)
        h_a[i] = r @ u
        # backward
        gu = u @ gi
        dsk = r * (gu - (r * gu).sum())
        top = amax == Mk[:, None]
        allmasked = Mk == NEG
        dss = torch.where(allmasked, torch.zeros_like(dsk), dsk / top.sum(-1))
        gh = H @ gi                                                               # [K,T]
        pr = p_ * r[:, None]
        damax = pr * (s * gh - gu[:, None]) + top * dss[:, None]
        damax = torch.where((pr != 0) & ~allmasked[:, None], damax, torch.zeros_like(damax))
        dx = damax * (1 - amax * amax) if tanh else damax
        dx = torch.where(damax != 0, dx, torch.zeros_like(dx))
        Qsj = Qs[jmax]                                                            # [K,T,w]
        dH = (s * pr)[..., None] * gi + (dx * s)[..., None] * (Qsj + Rh) + 2 * (dx * s * s)[..., None] * R2 * H
        for m, p in enumerate(row):                                               # by reference; an empty slot: nowhere
            if p >= 0:
                dpool[p] += dH[:, m * JX:(m + 1) * JX]
        ds = pr * gh + dx * (lin.gather(-1, jmax[..., None])[..., 0] + 2 * s * r2)
        dxsH = ((dx * s)[..., None] * H).reshape(K * T, w)
        dQs = torch.zeros(JQ, w, dtype=dtype).index_add_(0, jmax.reshape(-1), dxsH)
        dct = torch.zeros(JQ, dtype=dtype).index_add_(0, jmax.reshape(-1), dx.reshape(-1))
        dRh += dxsH.sum(0)
        dR2 += ((dx * s * s)[..., None] * H * H).sum((0, 1))
        dq[i] = U * dQs + dct[:, None] * (Cq + 2 * R2 * Q)
        dU += (dQs * Q).sum(0)
        dCq += (dct[:, None] * Q).sum(0)
        dC2 += (dct[:, None] * Q * Q).sum(0)
        db += dct.sum()
        if tanh:             # the form the kernels take for db: a question's damax sum to zero over (k, t)
            dbt = torch.where(damax != 0, damax * amax * amax, torch.zeros_like(damax))
            db_pooled -= dbt[:, live[i]].sum()                                    # an empty slot's positions: not read
        # dz with the count of the GLOBAL position; zero at an empty slot WITHOUT reading ds there (the kernels cannot)
        dz[i] = torch.where(live[i], cnt * (1 - tz[i] * tz[i]) * torch.where(live[i][None, :], ds, torch.zeros_like(ds)).sum(0),
                            torch.zeros(T, dtype=dtype))
        assert float(ds[:, ~live[i]].abs().max() if bool((~live[i]).any()) else 0.0) == 0.0    # ... and zero IS its value
    de = torch.zeros(Pn, JX, dtype=dtype)
    for i in range(NQ):                                                               # references in plan order
        for m, p in enumerate(al[i].tolist()):
            if p >= 0:
                de[p] += dz[i, m * JX:(m + 1) * JX]
    D = dz.sum(1)
    ds0 = K * D.sum()
    dpool += 2 * de[:, None, :, None] * v * pool                                      # every k, masked rows too: e sums them
    dv = torch.einsum("at,aktc->c", de, pool * pool)
    dWH_W = torch.zeros(2 * w, w, dtype=dtype)
    dWH_W[:w] = dv[:, None] * WC[None, :]
    dD = dR2 + dC2
    if simi == 1:
        dW = torch.cat([dRh, dCq, dU])
    elif simi == 2:
        dW = torch.cat([dU, dD - 2 * dU])
    else:
        dW = torch.cat([dRh, dCq, dD - 2 * dU, dU])
    return dict(h_a=h_a, a_logits=logits, scale=s_all, dpool=dpool, dq=dq, dlq=K * D[:, None] * WC[None, :], dW=dW, db=db,
                dWH_W=dWH_W, dWH_b=ds0 * WC, dWC_W=WH.t() @ dv + ds0 * WHb + K * (D @ lq), dWC_b=ds0.reshape(1),
                db_pooled=db_pooled, dz=dz, de=de)


# ------------------------------------------------------------------ the conditions every training case meets
def valid_mask(c):
    """[NQ,K,T,JQ] bool: the entries exp_mask leaves alone (an empty slot: none)"""
    NQ, K, T, JQ = c["NQ"], c["K"], c["T"], c["JQ"]
    if c["pm"] is None or c["qm"] is None:
        return torch.ones(NQ, K, T, JQ, dtype=torch.bool)
    pm = torch.cat([c["pm"], torch.zeros_like(c["pm"][:1])])[_slots(c)]        # [NQ,M,K,JX]
    return pm.permute(0, 2, 1, 3).reshape(NQ, K, T)[:, :, :, None] & c["qm"][:, None, None, :]


def first_slots(c):
    """[NQ,T] bool: the positions of slots that do NOT repeat an earlier slot's album in the same list"""
    keep = torch.ones(c["NQ"], c["M"], dtype=torch.bool)
    for i, row in enumerate(c["albums"].tolist()):
        for m, p in enumerate(row):
            if p >= 0 and p in row[:m]:
                keep[i, m] = False
    return keep[:, :, None].expand(-1, -1, c["JX"]).reshape(c["NQ"], c["T"])


def conditions(c, a_logits):
    """(smallest top-2 gap over j in a valid row, smallest top-2 gap of amax over t in a (question, k), fraction of valid
    logits with |x| > SAT_X); a gap that does not exist (one valid entry) counts as inf.  A slot that repeats an earlier
    slot's album in the same list is left out of the gap over t: its rows ARE the earlier slot's rows, so the tie is exact
    by construction, and both ways of resolving it (all to one slot, or split) give the same d_pool and d_hq."""
    v = valid_mask(c)
    x = torch.where(v, a_logits, torch.full_like(a_logits, -float("inf")))
    inf = float("inf")
    jgap = inf
    if c["JQ"] > 1:
        top = torch.topk(x, 2, dim=-1).values                       # [NQ,K,T,2]
        two = v.sum(-1) >= 2
        if bool(two.any()):
            jgap = float((top[..., 0] - top[..., 1])[two].min())
    tgap = inf
    rowv = v.any(-1) & first_slots(c)[:, None, :]                   # [NQ,K,T]
    amax = torch.where(rowv, x.max(-1).values, torch.full_like(x[..., 0], -inf))
    if c["T"] > 1:
        top = torch.topk(amax, 2, dim=-1).values
        two = rowv.sum(-1) >= 2
        if bool(two.any()):
            tgap = float((top[..., 0] - top[..., 1])[two].min())
    sat = float((a_logits[v].abs() > SAT_X).double().mean()) if c["tanh"] and bool(v.any()) else 0.0
    return jgap, tgap, sat


def qualifies(c, a_logits):
    jgap, tgap, sat = conditions(c, a_logits)
    return jgap > GAP and tgap > GAP and sat < SAT_FRACTION
