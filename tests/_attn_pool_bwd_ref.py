"""Seeded inputs, pinned seeds and the fp64 reference for the pooled focal attention BACKWARD (fvta_attn_pool_fwd_train /
fvta_attn_pool_bwd): fp64 autograd of oracle.fvta_fused.attention_3d through tests/_attn_pooled_ref.expand, applied to a
pool that requires grad.  expand is stack / cat of the pool's albums, so the gather's own gradient is the sum of the row
gradients over every (question, slot) reference to an album.

Inputs are tests/_attn_pooled_ref.make_case's with att_logits/W scaled by sqrt(64 / w), for the reason given in
tests/_attn_shared_bwd_ref.py (the tanh logits saturate from w = 512 on at the unscaled recipe), plus a seeded d_h_a.

Every case must satisfy `conditions` (tests/_album_attn_ref.py, tests/_attn_shared_bwd_ref.py's too): the top-2 gap over j
of every valid row and the top-2 gap of amax over t of every (question, k) above GAP, under tanh fewer than 5 % of the valid
logits with |x| > 0.99 -- with ONE adaptation: a slot that repeats an earlier slot's album in the same list is left out
of the gap over t.  Its rows ARE the earlier slot's rows, so the tie is exact by construction, and both ways of resolving
it (all to one slot, or split) give the same d_pool and d_hq.  SEEDS holds, per case, the first seed of `seed_candidates`
that qualifies (tests/test_attn_pool_bwd_host.py re-checks every one in fp64).

The shapes are tests/_attn_pooled_ref.py's SPECS / LOOP_SPECS with the simiMatrix 4 variants dropped (no pooled backward),
the row counts JX placed around the ROW PASS's tile (fvta_attn_pool_bwd_plan) instead of the logits tile, and `tiles`: two
row tiles per workgroup of the row pass."""
import torch

from tests import _album_attn_ref as AR
from tests import _attn_pooled_ref as P

GAP, SAT_X, SAT_FRACTION = AR.GAP, AR.SAT_X, AR.SAT_FRACTION
conditions, qualifies, valid_mask, first_slots = AR.conditions, AR.qualifies, AR.valid_mask, AR.first_slots
SIMI_TANH = [(1, False), (2, True), (3, True)]
ROW_JX = ["1", "7", "Rb-1", "Rb", "Rb+1", "65", "200"]
N_CANDIDATES = 32


def host_bwd_plan_words(Pn, NQ, M, K, JX, JQ, w):
    """the four words of fvta_attn_pool_bwd_plan, named as ops.PooledFocalAttention.bwd_plan() names them (host only)"""
    import ctypes
    from fvta_memexqa_amd import _lib
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().fvta_attn_pool_bwd_plan(ctypes.byref(_lib.AttnPoolDesc(Pn, NQ, M, K, JX, JQ, w, 1, 0)), out) == 0
    return dict(zip(("rows", "tsplit", "channels", "tiles_per_wg"), (int(v) for v in out)))


def _row_JX(tag, Rb):
    return {"Rb-1": max(Rb - 1, 1), "Rb": Rb, "Rb+1": Rb + 1}.get(tag) or int(tag)


def _pspec(name):
    return next(s for s in P.SPECS if s[0] == name)


# (name, P, lists(G, masked) -> [NQ,M], K, JX(Rb), JQ, w, simi, tanh, masked)
def _specs():
    out = []
    _, Pn, lists, K, JX, JQ, w, _ = _pspec("mix")
    for simi, tanh in SIMI_TANH:
        for masked in (True, False):
            out.append(("mix-simi%d-%s" % (simi, "masked" if masked else "open"), Pn, lists, K, lambda Rb, JX=JX: JX(0), JQ, w,
                        simi, tanh, masked))
    _, Pn, lists, K, _, JQ, w, _ = _pspec("rows0")
    for i, tag in enumerate(ROW_JX):
        simi, tanh = SIMI_TANH[i % 3]
        out.append(("rows-JX%s" % tag, Pn, lists, K, (lambda Rb, tag=tag: _row_JX(tag, Rb)), JQ, w, simi, tanh, True))
    for i, (JQ, w) in enumerate([(JQ, w) for JQ in (1, 30, 32, 33, 64) for w in (128, 512)]):
        simi, tanh = SIMI_TANH[i % 3]
        _, Pn, lists, K, JX, _, _, _ = _pspec("cols_jq%d_w%d" % (JQ, w))
        out.append(("cols-jq%d-w%d" % (JQ, w), Pn, lists, K, lambda Rb, JX=JX: JX(0), JQ, w, simi, tanh, i % 4 != 3))
    for name, variants in (("wide1024", [(2, True, True)]), ("wide2048", [(3, True, True)]), ("slots9", [(2, True, True)]),
                           ("k6", [(3, True, True)]), ("single", [(1, False, True), (2, True, False)]),
                           ("all-empty", [(1, False, True), (3, True, True)])):
        _, Pn, lists, K, JX, JQ, w, _ = _pspec(name)
        for simi, tanh, masked in variants:
            tag = name if len(variants) == 1 else "%s-simi%d" % (name, simi)
            out.append((tag, Pn, lists, K, lambda Rb, JX=JX: JX(0), JQ, w, simi, tanh, masked))
    # past one round of the plan's and the row pass's loops
    for name in ("many", "heavy"):
        _, Pn, counts, M, K, JX, JQ, w, simi, tanh = next(s for s in P.LOOP_SPECS if s[0] == name)
        lists = (lambda G, masked, counts=counts, M=M, name=name:
                 P.lists_from_counts(counts(G), M, sum(map(ord, name)) * 10, True))
        out.append((name, Pn, lists, K, lambda Rb, JX=JX: JX, JQ, w, simi, tanh, True))
    # 180 albums x 3 k x 2 row tiles of 128 rows at w = 64: more tiles than the row pass starts workgroups for
    out.append(("tiles", 180, lambda G, masked: P.lists_from_counts([3, 2] + [0] * 177 + [2], 2, 5300, True), 3,
                lambda Rb: 130, 5, 64, 2, True, True))
    return out


SPECS = _specs()
CASE_IDS = [s[0] for s in SPECS]
MIX_MASKED = "mix-simi2-masked"      # the case of the per-question comparison, there with its masks unmodified
LOOP_IDS = ["many", "heavy", "tiles"]


def seed_candidates(name):
    return AR.seed_candidates(name, 0, N_CANDIDATES)


# the first qualifying candidate per case (tests/test_attn_pool_bwd_host.py re-checks every one of them)
SEEDS = {
    "mix-simi1-masked": 15360,
    "mix-simi1-open": 13410,
    "mix-simi2-masked": 15370,
    "mix-simi2-open": 13420,
    "mix-simi3-masked": 15380,
    "mix-simi3-open": 13430,
    "rows-JX1": 7150,
    "rows-JX7": 7210,
    "rows-JXRb-1": 9400,
    "rows-JXRb": 8460,
    "rows-JXRb+1": 9380,
    "rows-JX65": 7730,
    "rows-JX200": 8120,
    "cols-jq1-w128": 10650,
    "cols-jq1-w512": 10620,
    "cols-jq30-w128": 11150,
    "cols-jq30-w512": 11120,
    "cols-jq32-w128": 11170,
    "cols-jq32-w512": 11140,
    "cols-jq33-w128": 11180,
    "cols-jq33-w512": 11150,
    "cols-jq64-w128": 11220,
    "cols-jq64-w512": 11190,
    "wide1024": 6240,
    "wide2048": 6310,
    "slots9": 6220,
    "k6": 1610,
    "single-simi1": 11700,
    "single-simi2": 11710,
    "all-empty-simi1": 14450,
    "all-empty-simi3": 14470,
    "many": 4370,
    "heavy": 5410,
    "tiles": 5450,
}


def spec_of(name):
    return next(s for s in SPECS if s[0] == name)


def build_case(name, seed=None, parity=True):
    """parity: as tests/_attn_shared_bwd_ref.build_case, every (album, k) and every question partly valid (the fully
    masked ones carry fvta_attn_bwd's documented deviation); an empty slot and a question that lists nothing stay what
    they are.  parity=False leaves make_case's masks as they are."""
    _, Pn, lists, K, JX, JQ, w, simi, tanh, masked = spec_of(name)
    G, _ = P.host_plan(JQ, w)
    Rb = host_bwd_plan_words(1, 1, 1, K, 64, JQ, w)["rows"]
    c = P.make_case(lists(G, masked), Pn, K, JX(Rb), JQ, w, simi, masked, SEEDS[name] if seed is None else seed)
    return AR.train_inputs(c, c["pm"], tanh, parity)


def plans_of(c):
    """the words of both host-only plans for case c's shape"""
    shape = (c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"])
    return P.host_plan_words(*shape), host_bwd_plan_words(*shape)


def loop_regime(name, c, plan, bwd_plan):
    """Asserts that a LOOP_IDS case reaches the code it is there for, from the two plans' words; other names pass."""
    if name in ("many", "heavy"):
        P.loop_regime(name, c, plan)
    elif name == "tiles":
        assert bwd_plan["tiles_per_wg"] >= 2 and c["JX"] > bwd_plan["rows"], bwd_plan      # two tiles, one workgroup


def reference(c):
    """fp64 autograd -> dict(h_a, a_logits, dpool [P,K,JX,w], dq, dW [F], db [1])"""
    from oracle import fvta_fused as F
    pool, q, W, b = (t.double().requires_grad_() for t in (c["pool"], c["q"], c["W"], c["b"]))
    h, m = P.expand(dict(c, pool=pool))
    ha, a = F.attention_3d(h, q, W, b, m, c["qm"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    (ha * c["gout"].double()).sum().backward()
    dpool = pool.grad if pool.grad is not None else torch.zeros_like(pool)
    return dict(h_a=ha.detach(), a_logits=a.detach(), dpool=dpool, dq=q.grad, dW=W.grad.reshape(-1), db=b.grad.reshape(-1))


def forward_logits(c):
    """the fp64 a_logits alone (no autograd): what `conditions` reads"""
    with torch.no_grad():
        return P.reference(c, c["tanh"])[1]


# ------------------------------------------------------------------ a width no kernel has (channel padding): w = 100
def odd_width_case():
    c = P.make_case(torch.tensor([[0, 1], [1, -1], [0, 0]]), 2, 2, 20, 5, 100, 2, True, 4242)
    return AR.train_inputs(c, c["pm"], True)
