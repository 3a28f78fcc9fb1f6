"""fp64 references and seeded inputs for the focal attention over per-question album lists from one album pool UNDER THE
TIME WARP (fvta_attn_pool_fwd_tw): pool [P,K,JX,w] holds every encoded album once, question i lists albums[i, :] (-1: an
empty slot), attends those albums' rows laid end to end (T = M * JX) and warped by its own last state lq[i]
(model_v2.py:953-1009, use_time_warp without use_time_warp_att).  A position's count runs over the question's whole T
positions: a band, past or future crosses slot boundaries.

`reference` is the definition: tests/_attn_pooled_ref.expand (the context of every question by concatenation, zeros and
mask 0 for an empty slot), oracle.fvta_fused.time_warp_closed, then oracle.fvta_fused.attention_3d on the warped rows.
`factored` (tests/_album_attn_ref.py) is the restatement the kernels compute, written out independently and parametrised
by dtype: the energy per POOLED ALBUM [P,JX], the scale per (question, global position t = m * JX + j), the scalar
passed through the bilinear form of the logits and through the weighted sum, the blocks of a pooled album's references
scattered to their slots' positions; no [NQ,K,T,w] tensor.  tests/test_attn_pooled_tw_host.py holds the two against each
other on every shape the GPU tests use.

Inputs: tests/_attn_pooled_ref.make_case / lists_from_counts, the warp's parameters by tests/_attn_shared_tw_ref.add_warp.
Tolerances: tests/_album_attn_ref.TOL."""
import torch

from tests import _album_attn_ref as AR
from tests import _attn_pooled_ref as R
from tests import _attn_shared_tw_ref as TW

NEG = R.NEG
WINDOW_T = TW.WINDOW_T
TOL, within, _dd = AR.TOL, AR.within, AR._dd
energy, scale_of, factored = AR.energy, AR.scale_of, AR.factored


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
def reference(c):
    """the definition, fp64 -> (h_a [NQ,w], a_logits [NQ,K,T,JQ], scale [NQ,T]), T = M JX"""
    from oracle import fvta_fused as F
    h, m = R.expand(c)                                                       # [NQ,K,T,w], [NQ,K,T] or None
    warped, cc = F.time_warp_closed(_dd(h), _dd(c["lq"]), _dd(c["WH_W"]), _dd(c["WH_b"]), _dd(c["WC_W"]), _dd(c["WC_b"]),
                                    warp_type=c["warp_type"], window_t=c["window_t"])
    cnt = F.time_indication_band(c["T"], c["warp_type"], c["window_t"], dtype=torch.float64).sum(-1)
    h_a, a = F.attention_3d(warped, _dd(c["q"]), _dd(c["W"]), _dd(c["b"]), m, c["qm"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    return h_a, a, cc * cnt[None, :]
