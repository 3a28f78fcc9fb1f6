"""Seeded inputs, pinned seeds and the references for the pooled focal attention BACKWARD UNDER THE TIME WARP
(fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw).

`reference` is the definition: fp64 autograd of tests/_attn_pooled_ref.expand -> oracle.fvta_fused.time_warp_closed ->
oracle.fvta_fused.attention_3d, all nine leaves requiring grad.  expand is stack / cat of the pool's albums, so d_pool is
the sum over every (question, slot) reference to an album of BOTH the attention's row gradient and the energy's.
`factored_backward` (tests/_album_attn_ref.py) is the restatement the kernels implement, by hand and without autograd:
the scale per (question, global position m JX + j), ds per (question, k, position), dz from ds with the count of the
GLOBAL position and zero at an empty slot, de per pooled album over its references, d_pool += 2 de v h, db as
-sum damax x^2.
tests/test_attn_pool_tw_bwd_host.py holds the two against each other.

Inputs: tests/_attn_pool_bwd_ref.py's shapes and recipe (att_logits/W scaled by sqrt(64 / w), the parity masks, a seeded
d_h_a) with the warp's parameters by tests/_attn_shared_tw_ref.add_warp, and att_logits/W FURTHER DIVIDED BY cmax^2 as in
tests/_attn_shared_tw_bwd_ref.py and for its reason: the warped rows are up to cmax times the rows (cmax = 2 ceil(window_t)
+ 1 for type 5, M JX for types 1 / 3 / 4, 1 for type 2) and the tanh cases saturate without it.  Added to those shapes:
`mix` under warp 2, the short shapes (M JX <= 9) under warps 1 / 3 / 4, three windows at M 2, JX 3, and `zero-rows`.

Every case satisfies tests/_attn_pool_bwd_ref.conditions, unchanged in value and in its one adaptation (a slot that
repeats an earlier slot's album in the same list is left out of the gap over t), on the WARPED logits.  The adaptation is
still needed under the warp: two slots that name the same album hold the same rows, and wherever the counts of their
positions agree (type 2 everywhere, type 5 in the band's interior) the same scale, so their logits tie exactly.
SEEDS pins, per case, the first qualifying one of `seed_candidates` (32; no case needed more than its first seven)."""
import torch

from tests import _album_attn_ref as AR
from tests import _attn_pool_bwd_ref as B
from tests import _attn_pooled_ref as P
from tests import _attn_shared_tw_bwd_ref as STB
from tests import _attn_shared_tw_ref as TW

NEG = P.NEG
WINDOW_T = TW.WINDOW_T
GAP, SAT_FRACTION = B.GAP, B.SAT_FRACTION
TOL = STB.TOL
GRAD_KEYS = ("dpool", "dq", "dlq", "dW", "db", "dWH_W", "dWH_b", "dWC_W", "dWC_b")
N_CANDIDATES = 32
conditions, qualifies, valid_mask, first_slots, plans_of = B.conditions, B.qualifies, B.valid_mask, B.first_slots, B.plans_of
cmax, count, within, factored_backward = AR.cmax, AR.count_of, AR.within, AR.factored_backward


# (name, P, lists(G, masked) -> [NQ,M], K, JX(Rb), JQ, w, simi, tanh, masked, warp_type, window_t, zero_rows)
def _specs():
    out = [s + (5, WINDOW_T, False) for s in B.SPECS]              # every shape of the unwarped backward, warp 5 at 2.3
    mix = B.spec_of("mix-simi2-masked")
    out.append(("mix-warp2",) + mix[1:] + (2, WINDOW_T, False))
    # M JX = 400 (rows-JX200) turns over dz's stride loop; JX = 260 at M 2 also starts de's second block of 256 positions
    r200 = B.spec_of("rows-JX200")
    out.append(("rows-JX260",) + r200[1:4] + (lambda Rb: 260,) + r200[5:] + (5, WINDOW_T, False))
    # past / future / all time where M JX <= 9 (tests/_attn_pooled_tw_ref.py says why): a count taken with the album's j
    # instead of m JX + j fails here
    short = lambda M: (lambda G, masked: P.lists_from_counts([G - 1, 2, 2], M, sum(map(ord, "short")), masked))
    for i, (M, JX) in enumerate(((3, 3), (2, 1), (1, 7))):
        for j, wt in enumerate((1, 3, 4)):
            simi, tanh = B.SIMI_TANH[(i + j) % 3]
            out.append(("short-M%d-JX%d-warp%d" % (M, JX, wt), 3, short(M), 3, (lambda Rb, JX=JX: JX), 7, 256, simi, tanh, True,
                        wt, WINDOW_T, False))
    for i, win in enumerate((0.5, 3.0, 7.0)):                      # M = 2, JX = 3; 7.0: a band wider than M JX
        simi, tanh = B.SIMI_TANH[(i + 1) % 3]
        out.append(("window%.1f" % win, 3, short(2), 3, lambda Rb: 3, 7, 256, simi, tanh, True, 5, win, False))
    # as the model's padding: the rows behind the masks are exactly ZERO (and (album 0, k 0), fully masked but for the
    # parity rows, nearly all zero)
    out.append(("zero-rows",) + mix[1:] + (5, WINDOW_T, True))
    return out


SPECS = _specs()
CASE_IDS = [s[0] for s in SPECS]
MIX_MASKED = B.MIX_MASKED
LOOP_IDS = B.LOOP_IDS


def spec_of(name):
    return next(s for s in SPECS if s[0] == name)


def seed_candidates(name):
    base = sum(map(ord, name)) * 10 + 6
    return [base + i for i in range(N_CANDIDATES)]


# the first qualifying candidate per case (tests/test_attn_pool_tw_bwd_host.py re-checks every one of them)
SEEDS = {
    "mix-simi1-masked": 15366,
    "mix-simi1-open": 13422,
    "mix-simi2-masked": 15378,
    "mix-simi2-open": 13429,
    "mix-simi3-masked": 15386,
    "mix-simi3-open": 13439,
    "rows-JX1": 7156,
    "rows-JX7": 7216,
    "rows-JXRb-1": 9406,
    "rows-JXRb": 8467,
    "rows-JXRb+1": 9386,
    "rows-JX65": 7736,
    "rows-JX200": 8127,
    "cols-jq1-w128": 10656,
    "cols-jq1-w512": 10626,
    "cols-jq30-w128": 11156,
    "cols-jq30-w512": 11126,
    "cols-jq32-w128": 11176,
    "cols-jq32-w512": 11146,
    "cols-jq33-w128": 11186,
    "cols-jq33-w512": 11156,
    "cols-jq64-w128": 11226,
    "cols-jq64-w512": 11196,
    "wide1024": 6246,
    "wide2048": 6316,
    "slots9": 6226,
    "k6": 1616,
    "single-simi1": 11706,
    "single-simi2": 11716,
    "all-empty-simi1": 14456,
    "all-empty-simi3": 14476,
    "many": 4379,
    "heavy": 5416,
    "tiles": 5460,
    "mix-warp2": 8716,
    "rows-JX260": 8188,
    "short-M3-JX3-warp1": 15276,
    "short-M3-JX3-warp3": 15296,
    "short-M3-JX3-warp4": 15306,
    "short-M2-JX1-warp1": 15246,
    "short-M2-JX1-warp3": 15266,
    "short-M2-JX1-warp4": 15276,
    "short-M1-JX7-warp1": 15296,
    "short-M1-JX7-warp3": 15316,
    "short-M1-JX7-warp4": 15326,
    "window0.5": 8116,
    "window3.0": 8096,
    "window7.0": 8136,
    "zero-rows": 9527,
}


def build_case(name, seed=None, parity=True):
    """tests/_attn_pool_bwd_ref.build_case's recipe (parity: every (album, k) and every question partly valid; an empty
    slot and a question that lists nothing stay what they are), then the warp and the division by cmax^2"""
    _, Pn, lists, K, JX, JQ, w, simi, tanh, masked, wt, win, zero_rows = spec_of(name)
    seed = SEEDS[name] if seed is None else seed
    G, _ = P.host_plan(JQ, w)
    Rb = B.host_bwd_plan_words(1, 1, 1, K, 64, JQ, w)["rows"]
    c = P.make_case(lists(G, masked), Pn, K, JX(Rb), JQ, w, simi, masked, seed)
    AR.train_inputs(c, c["pm"], tanh, parity)
    if zero_rows:
        c["pool"] = c["pool"] * c["pm"][..., None]
    c = TW.add_warp(c, seed, wt, win)
    c["W"] = c["W"] / float(cmax(c["T"], wt, win)) ** 2
    return c


def loop_regime(name, c, plan, bwd_plan):
    B.loop_regime(name, c, plan, bwd_plan)


# ------------------------------------------------------------------ the definition
def reference(c, grads=True):
    """fp64 (autograd) -> dict(h_a, a_logits, scale, dpool [P,K,JX,w], dq, dlq, dW [F], db [1], dWH_W [2w,w], dWH_b,
    dWC_W [w], dWC_b); grads=False: the forward's three alone"""
    from oracle import fvta_fused as F
    names = ("pool", "q", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b")
    t = {k: c[k].double().requires_grad_(grads) for k in names}
    with torch.set_grad_enabled(grads):
        h, m = P.expand(dict(c, pool=t["pool"]))
        warped, cc = F.time_warp_closed(h, t["lq"], t["WH_W"], t["WH_b"], t["WC_W"], t["WC_b"], warp_type=c["warp_type"],
                                        window_t=c["window_t"])
        ha, a = F.attention_3d(warped, t["q"], t["W"], t["b"], m, c["qm"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    out = dict(h_a=ha.detach(), a_logits=a.detach(), scale=cc.detach() * count(c)[None, :])
    if not grads:
        return out
    (ha * c["gout"].double()).sum().backward()
    g = lambda k: t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])
    out.update(dpool=g("pool"), dq=g("q"), dlq=g("lq"), dW=g("W").reshape(-1), db=g("b").reshape(-1), dWH_W=g("WH_W"),
               dWH_b=g("WH_b"), dWC_W=g("WC_W").reshape(-1), dWC_b=g("WC_b").reshape(-1))
    return out


def forward_logits(c):
    """the fp64 warped a_logits alone: what `conditions` reads"""
    return reference(c, grads=False)["a_logits"]


# ------------------------------------------------------------------ a width no kernel has (channel padding): w = 50
ODD_WIDTH_SEED = 4242


def odd_width_case(seed=None):
    seed = ODD_WIDTH_SEED if seed is None else seed
    c = P.make_case(torch.tensor([[0, 1], [1, -1], [0, 0]]), 2, 2, 20, 5, 50, 2, True, seed)
    c = TW.add_warp(AR.train_inputs(c, c["pm"], True), seed, 5, WINDOW_T)
    c["W"] = c["W"] / float(cmax(c["T"], 5, WINDOW_T)) ** 2
    return c
