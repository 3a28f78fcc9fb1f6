"""fp64 references and seeded inputs for the focal attention over per-question album lists from one album pool UNDER THE
TIME WARP (fvta_attn_pool_fwd_tw): pool [P,K,JX,w] holds every encoded album once, question i lists albums[i, :] (-1: an
empty slot), attends those albums' rows laid end to end (T = M * JX) and warped by its own last state lq[i]
(model_v2.py:953-1009, use_time_warp without use_time_warp_att).  A position's count runs over the question's whole T
positions: a band, past or future crosses slot boundaries.

`reference` is the definition: tests/_attn_pooled_ref.expand (the context of every question by concatenation, zeros and
mask 0 for an empty slot), oracle.fvta_fused.time_warp_closed, then oracle.fvta_fused.attention_3d on the warped rows.
`factored` is the restatement the kernels compute, written out independently and parametrised by dtype: the energy per
POOLED ALBUM [P,JX], the scale per (question, global position t = m * JX + j), the scalar passed through the bilinear
form of the logits and through the weighted sum, the blocks of a pooled album's references scattered to their slots'
positions; no [NQ,K,T,w] tensor.  tests/test_attn_pooled_tw_host.py holds the two against each other on every shape the
GPU tests use.

Inputs: tests/_attn_pooled_ref.make_case / lists_from_counts, the warp's parameters by tests/_attn_shared_tw_ref.add_warp.
Tolerances: tests/_attn_shared_tw_ref.TOL."""
import torch

from tests import _attn_pooled_ref as R
from tests import _attn_shared_tw_ref as TW

NEG = R.NEG
WINDOW_T = TW.WINDOW_T
TOL = TW.TOL
within = TW.within


# ------------------------------------------------------------------ the cases
# name -> (P, lists(G, masked) -> [NQ,M], K, JX(R), JQ, w, simi, tanh, masked, warp_type, window_t, zero_rows); G and R:
# fvta_attn_pool_plan's words.  Warp types 1, 3 and 4 multiply the rows by counts up to M JX, so the fp32 rounding of the
# warped rows' logits grows with M JX while the a_logits tolerance stays absolute (tests/_attn_shared_tw_ref.py): they
# come at M JX <= 9 only; types 2 and 5 (counts of at most 2 ceil(window_t) + 1) at every shape.
def _counted(counts, M, name):
    return lambda G, masked: R.lists_from_counts(counts(G), M, sum(map(ord, name)), masked)


def _pooled_spec(name):
    """(P, lists, K, JX, JQ, w) of the case `name` of tests/_attn_pooled_ref.SPECS"""
    _, P, lists, K, JX, JQ, w, _ = next(s for s in R.SPECS if s[0] == name)
    return P, lists, K, JX, JQ, w


def _specs():
    out = {}
    mix = _pooled_spec("mix")                    # P 5, references [G+1, 1, 0, 2G+1, G], M 3, K 2, JX 17, JQ 10, w 64
    for s, t in R.SIMI_TANH:                     # warp 5, window 2.3: the band crosses the slot boundaries at 14..19, 31..36
        for m in (True, False):
            out["mix-simi%d-%s" % (s, "masked" if m else "open")] = mix + (s, t, m, 5, WINDOW_T, False)
    out["mix-warp2"] = mix + (2, True, True, 2, WINDOW_T, False)
    # past / future / all time where M JX <= 9: the cases that catch a count taken with the album's j instead of m JX + j
    for M, JX in ((3, 3), (2, 1), (1, 7)):
        for wt in (1, 3, 4):
            for s, t in R.SIMI_TANH:
                nm = "short-M%d-JX%d-warp%d-simi%d" % (M, JX, wt, s)
                out[nm] = (3, _counted(lambda G: [G - 1, 2, 2], M, "short"), 3, (lambda JX: lambda Rr: JX)(JX), 7, 256, s, t, True,
                           wt, WINDOW_T, False)
    for i in range(6):                           # JX in {1, 7, R-1, R, R+1, 200}, M = 2
        s, t = R.SIMI_TANH[i % 4]
        out["rows%d" % i] = _pooled_spec("rows%d" % i) + (s, t, True, 5, WINDOW_T, False)
    for i, win in enumerate((0.5, 3.0, 7.0)):    # M = 2, JX = 3; 7.0: a band wider than M JX
        s, t = R.SIMI_TANH[(i + 1) % 4]
        out["window%.1f" % win] = (3, _counted(lambda G: [G - 1, 2, 2], 2, "window"), 3, lambda Rr: 3, 7, 256, s, t, True, 5, win,
                                   False)
    for i, (JQ, w) in enumerate([(JQ, w) for JQ in (32, 33, 64) for w in (128, 512)]):
        s, t = R.SIMI_TANH[i % 4]
        out["cols-jq%d-w%d" % (JQ, w)] = _pooled_spec("cols_jq%d_w%d" % (JQ, w)) + (s, t, i % 3 != 2, 5, WINDOW_T, False)
    out["wide1024"] = _pooled_spec("wide1024") + (2, True, True, 5, WINDOW_T, False)
    out["wide2048-simi3"] = _pooled_spec("wide2048") + (3, True, True, 5, WINDOW_T, False)     # the weighted sum's CPT 2
    out["wide2048-simi4"] = _pooled_spec("wide2048") + (4, False, False, 5, WINDOW_T, False)
    out["slots9"] = _pooled_spec("slots9") + (2, True, True, 5, WINDOW_T, False)               # M 9, JX 5
    out["k9"] = (2, _counted(lambda G: [2, 1], 2, "k9"), 9, lambda Rr: 17, 10, 64, 3, True, True, 5, WINDOW_T, False)
    out["single-simi1"] = _pooled_spec("single") + (1, False, True, 5, WINDOW_T, False)
    out["single-simi2"] = _pooled_spec("single") + (2, True, False, 5, WINDOW_T, False)
    # question 1 lists nothing at all; question 2 (the last: fully masked by the recipe) has one empty slot
    out["all-empty-simi1"] = _pooled_spec("all-empty") + (1, False, True, 5, WINDOW_T, False)
    out["all-empty-simi3"] = _pooled_spec("all-empty") + (3, True, True, 5, WINDOW_T, False)
    # as the model's padding: the rows behind the masks are ZERO (LSTM outputs past the length); (album 0, k 0) is fully
    # masked, so all of its rows are zero: the cosine form meets |h'| = 0
    out["zero-rows-simi2"] = mix + (2, True, True, 5, WINDOW_T, True)
    out["zero-rows-simi4"] = mix + (4, False, True, 5, WINDOW_T, True)
    return out


SPECS = _specs()
NAMES = list(SPECS)
LOOP_NAMES = list(R.LOOP_IDS)                    # many, heavy, chunks of tests/_attn_pooled_ref.LOOP_SPECS, under warp 5
ALL = NAMES + LOOP_NAMES


def build_case(name):
    """the case `name` of SPECS or LOOP_NAMES -> dict (tests/_attn_pooled_ref.make_case's keys, the warp's, and `tanh`)"""
    if name in LOOP_NAMES:
        c = R.loop_case(name)
        return TW.add_warp(c, sum(map(ord, name)) * 10, 5)
    P, lists, K, JX, JQ, w, simi, tanh, masked, wt, win, zero_rows = SPECS[name]
    G, Rr = R.host_plan(JQ, w)
    seed = sum(map(ord, name)) * 10 + simi + (5 if masked else 0)
    c = R.make_case(lists(G, masked), P, K, JX(Rr), JQ, w, simi, masked, seed)
    if zero_rows:
        c["pool"] = c["pool"] * c["pm"][..., None]
    c["tanh"] = tanh
    return TW.add_warp(c, seed, wt, win)


# ------------------------------------------------------------------ references (CPU)
def _dd(t):
    return None if t is None else t.double()


def reference(c):
    """the definition, fp64 -> (h_a [NQ,w], a_logits [NQ,K,T,JQ], scale [NQ,T]), T = M JX"""
    from oracle import fvta_fused as F
    h, m = R.expand(c)                                                       # [NQ,K,T,w], [NQ,K,T] or None
    warped, cc = F.time_warp_closed(_dd(h), _dd(c["lq"]), _dd(c["WH_W"]), _dd(c["WH_b"]), _dd(c["WC_W"]), _dd(c["WC_b"]),
                                    warp_type=c["warp_type"], window_t=c["window_t"])
    cnt = F.time_indication_band(c["T"], c["warp_type"], c["window_t"], dtype=torch.float64).sum(-1)
    h_a, a = F.attention_3d(warped, _dd(c["q"]), _dd(c["W"]), _dd(c["b"]), m, c["qm"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    return h_a, a, cc * cnt[None, :]


def _softmax_last(x):
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def energy(c, dtype=torch.float64):
    """e [P,JX] = sum_k sum_c v[c] pool[p,k,j,c]^2, v = WH[:w] WC: per pooled album"""
    w = c["w"]
    v = c["WH_W"].to(dtype)[:w] @ c["WC_W"].to(dtype).reshape(w)
    h = c["pool"].to(dtype)
    return ((h * h) @ v).sum(1)


def scale_of(c, dtype=torch.float64):
    """scale [NQ, M JX]: the pooled albums' energies gathered per slot (an empty slot: 0), the count of the GLOBAL position"""
    cv = lambda t: t.to(dtype)
    al, K, M, JX, w = c["albums"], c["K"], c["M"], c["JX"], c["w"]
    WC = cv(c["WC_W"]).reshape(w)
    s0 = cv(c["WH_b"]) @ WC + cv(c["WC_b"])[0]
    e = torch.cat([energy(c, dtype), torch.zeros(1, JX, dtype=dtype)])       # row P: an empty slot's
    ei = e[torch.where(al >= 0, al, torch.full_like(al, c["P"]))].reshape(c["NQ"], M * JX)
    z = ei + K * (s0 + cv(c["lq"]) @ WC)[:, None]
    return torch.tanh(z) * TW._count(M * JX, c["warp_type"], c["window_t"], dtype)[None, :]


def factored(c, dtype=torch.float64):
    """pooled album by pooled album: one product for all (question, slot) references to it, the scale of the reference's
    positions through the bilinear form and the weighted sum, scattered to the slots -> (h_a, a_logits, scale) in `dtype`"""
    cv = lambda t: None if t is None else t.to(dtype)
    pool, q, al, simi, tanh = cv(c["pool"]), cv(c["q"]), c["albums"], c["simi"], c["tanh"]
    P, K, JX, w = pool.shape
    NQ, JQ = q.shape[:2]
    M = al.shape[1]
    T = M * JX
    scale = scale_of(c, dtype)
    W = None if c["W"] is None else cv(c["W"]).reshape(-1)
    b = None if c["b"] is None else cv(c["b"])[0]
    zero = torch.zeros(w, dtype=dtype)
    if simi == 1:            # [h, q, h*q] . W
        Rh, Cq, U, R2 = W[:w], W[w:2 * w], W[2 * w:], zero
    elif simi == 2:          # [h*q, (h-q)^2] . W
        Rh, Cq, U, R2 = zero, zero, W[:w] - 2 * W[w:], W[w:]
    elif simi == 3:          # [h, q, (h-q)^2, h*q] . W
        Rh, Cq, U, R2 = W[:w], W[w:2 * w], W[3 * w:] - 2 * W[2 * w:3 * w], W[2 * w:3 * w]
    masked = c["pm"] is not None and c["qm"] is not None
    logits = torch.full((NQ, K, T, JQ), NEG if masked else float("nan"), dtype=dtype)
    for p in range(P):
        ref = torch.nonzero(al == p)                                      # [nref, 2]: (question, slot)
        if ref.shape[0] == 0:
            continue
        qi, mi = ref[:, 0], ref[:, 1]
        nref = qi.numel()
        H = pool[p].reshape(K * JX, w)
        Q = q[qi].reshape(nref * JQ, w)
        pos = mi[:, None] * JX + torch.arange(JX)[None, :]                # [nref,JX]: the references' global positions
        s = torch.gather(scale[qi], 1, pos)[:, None, :].expand(nref, K, JX)
        if simi == 4:
            Qn = Q / torch.sqrt(torch.clamp((Q * Q).sum(1, keepdim=True), min=1e-12))
            dot = (H @ Qn.t()).reshape(K, JX, nref, JQ).permute(2, 0, 1, 3)
            n2 = (H * H).sum(1).reshape(K, JX)[None]
            x = dot * (s / torch.sqrt(torch.clamp(s * s * n2, min=1e-12)))[..., None]
        else:
            dot = (H @ (Q * U).t()).reshape(K, JX, nref, JQ).permute(2, 0, 1, 3)
            ct = ((Q @ Cq + (Q * Q) @ R2) + b).reshape(nref, JQ)
            r1, r2 = (H @ Rh).reshape(K, JX)[None], ((H * H) @ R2).reshape(K, JX)[None]
            x = s[..., None] * (dot + r1[..., None]) + (s * s * r2)[..., None] + ct[:, None, None, :]
            if tanh:
                x = torch.tanh(x)
        if masked:
            valid = c["pm"][p][None, :, :, None] & c["qm"][qi][:, None, None, :]
            x = torch.where(valid, x, torch.full_like(x, NEG))
        for r in range(nref):
            logits[qi[r], :, mi[r] * JX:(mi[r] + 1) * JX] = x[r]
    assert not torch.isnan(logits).any()                                   # open: every slot was written
    amax = logits.max(-1).values                                           # [NQ,K,T]
    pt = _softmax_last(amax) * scale[:, None, :]                           # the weight carries the scale
    u = torch.zeros(NQ, K, w, dtype=dtype)
    for i in range(NQ):
        for m in range(M):
            p = int(al[i, m])
            if p >= 0:                                                     # (an empty slot: zero rows)
                u[i] += torch.einsum("kt,ktc->kc", pt[i, :, m * JX:(m + 1) * JX], pool[p])
    r = _softmax_last(amax.max(-1).values)                                 # [NQ,K]
    return torch.einsum("gk,gkc->gc", r, u), logits, scale
