"""Seeded inputs, pinned seeds and the fp64 reference for the shared-context focal attention BACKWARD
(fvta_attn_shared_fwd_train / fvta_attn_shared_bwd): fp64 autograd of oracle.fvta_fused.attention_3d on h[album]; the
gather's own gradient sums the row gradients per album.

Inputs are tests/_attn_shared_ref.make_case's with att_logits/W scaled by sqrt(64 / w): at the unscaled recipe the tanh
logits saturate from w = 512 on (all |x| = 1.000 in fp64, top-2 gaps down to 1e-13 at w = 2048), where the logit
gradient vanishes -- a broken question pass would pass -- and the fp32 arg-max is arbitrary.

Every case must satisfy `conditions` (tests/_album_attn_ref.py, the album pool's at one album per question;
tests/test_attn_shared_bwd_host.py asserts them per pinned seed in fp64), so that
the GPU test excludes nothing: the first and second valid logit over j of every valid row, and the two largest amax
over t of every (question, k), lie more than GAP apart, and under tanh fewer than 5 % of the valid logits have
|x| > 0.99.  SEEDS holds, per case, the first seed of `seed_candidates` that qualifies.

Beside the shapes that turn over T, JQ and the widths, SPECS ends with those of tests/_attn_shared_ref.py LOOP_SPECS, which
go past one round of the plan's and the row pass's loops: `many` (A = 1500, NQ = 1284), `heavy` ([150, 0, 50] questions),
`tiles-w64` / `-w512` / `-w2048` (two row tiles per workgroup at each thread layout of the row pass), `k17`, `k64`,
`splits9` (nine T splits of the question pass)."""
import torch

from tests import _album_attn_ref as AR
from tests import _attn_shared_ref as R

GAP, SAT_X, SAT_FRACTION = AR.GAP, AR.SAT_X, AR.SAT_FRACTION
SIMI_TANH = [(1, False), (2, True), (3, True)]
ROW_TS = ["1", "7", "Rb-1", "Rb", "Rb+1", "63", "64", "65", "333"]


def host_bwd_plan(K, T, JQ, w, A=1, NQ=1):
    """(rows per tile of the row pass, T splits of the question pass, channels per slice): host only, no GPU"""
    p = host_bwd_plan_words(A, NQ, K, T, JQ, w)
    return p["rows"], p["tsplit"], p["channels"]


def host_bwd_plan_words(A, NQ, K, T, JQ, w):
    """all four words of fvta_attn_shared_bwd_plan, named as ops.SharedFocalAttention.bwd_plan() names them"""
    import ctypes
    from fvta_memexqa_amd import _lib
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().fvta_attn_shared_bwd_plan(ctypes.byref(_lib.AttnSharedDesc(A, NQ, K, T, JQ, w, 1, 0)), out) == 0
    return dict(zip(("rows", "tsplit", "channels", "tiles_per_wg"), (int(v) for v in out)))


def _row_T(tag, Rb):
    return {"Rb-1": max(Rb - 1, 1), "Rb": Rb, "Rb+1": Rb + 1}.get(tag) or int(tag)


# (name, counts(G), K, T(Rb), JQ, w, simi, tanh, masked)
def _specs():
    out = []
    for simi, tanh in SIMI_TANH:
        for masked in (True, False):
            out.append(("mix-simi%d-%s" % (simi, "masked" if masked else "open"),
                        lambda G: [G + 1, 1, 0, 2 * G + 1, G], 2, lambda Rb: 50, 10, 64, simi, tanh, masked))
    for i, tag in enumerate(ROW_TS):
        simi, tanh = SIMI_TANH[i % 3]
        out.append(("rows-T%s" % tag, lambda G: [G - 1, 2], 3, (lambda Rb, tag=tag: _row_T(tag, Rb)), 7, 256, simi, tanh, True))
    for i, (JQ, w) in enumerate([(JQ, w) for JQ in (1, 30, 32, 33, 64) for w in (128, 512)]):
        simi, tanh = SIMI_TANH[i % 3]
        out.append(("cols-jq%d-w%d" % (JQ, w), lambda G: [G + 1, 1], 2, lambda Rb: 40, JQ, w, simi, tanh, i % 4 != 3))
    out.append(("wide1024", lambda G: [3, 2], 2, lambda Rb: 70, 30, 1024, 2, True, True))
    out.append(("wide2048", lambda G: [3, 2], 2, lambda Rb: 70, 30, 2048, 3, True, True))
    out.append(("single", lambda G: [1], 2, lambda Rb: 50, 10, 64, 2, True, True))
    out.append(("k6", lambda G: [2, 1], 6, lambda Rb: 50, 10, 64, 3, True, True))
    # past one round of the plan and tile loops (tests/_attn_shared_ref.py LOOP_SPECS; `chunks` is the forward's alone)
    out.extend(spec for spec in R.LOOP_SPECS if spec[0] not in R.FORWARD_ONLY)
    return out


SPECS = _specs()
CASE_IDS = [s[0] for s in SPECS]
MIX_MASKED = "mix-simi2-masked"      # the case of the per-question comparison, there with its masks unmodified


def seed_candidates(name):
    return AR.seed_candidates(name, 0, 8)


# the first qualifying candidate per case (tests/test_attn_shared_bwd_host.py re-checks every one of them)
SEEDS = {
    "mix-simi1-masked": 15360,
    "mix-simi1-open": 13410,
    "mix-simi2-masked": 15370,
    "mix-simi2-open": 13420,
    "mix-simi3-masked": 15380,
    "mix-simi3-open": 13431,
    "rows-T1": 6370,
    "rows-T7": 6430,
    "rows-TRb-1": 8620,
    "rows-TRb": 7680,
    "rows-TRb+1": 8600,
    "rows-T63": 6930,
    "rows-T64": 6940,
    "rows-T65": 6950,
    "rows-T333": 7410,
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
    "single": 6420,
    "k6": 1610,
    "many": 4370,
    "heavy": 5410,
    "tiles-w64": 8150,
    "tiles-w512": 8612,
    "tiles-w2048": 9151,
    "k17": 2110,
    "k64": 2130,
    "splits9": 7280,
}


def spec_of(name):
    return next(s for s in SPECS if s[0] == name)


def shape_of(name):
    """(counts, K, T, JQ, w, simi, tanh, masked) with G and the row tile read from the library's host-only plans"""
    _, counts, K, T, JQ, w, simi, tanh, masked = spec_of(name)
    G, _ = R.host_plan(JQ, w)
    Rb, _, _ = host_bwd_plan(K, 64, JQ, w)
    return counts(G), K, T(Rb), JQ, w, simi, tanh, masked


def build_case(name, seed=None, parity=True):
    """parity: as tests/test_gpu_backward.py, every (album, k) and every question partly valid (the fully masked ones
    carry fvta_attn_bwd's documented deviation); parity=False leaves make_case's masks as they are."""
    counts, K, T, JQ, w, simi, tanh, masked = shape_of(name)
    return R.train_recipe(counts, K, T, JQ, w, simi, tanh, masked, SEEDS[name] if seed is None else seed, parity)


def plans_of(c):
    """the words of both host-only plans for case c's shape"""
    shape = (c["A"], c["NQ"], c["K"], c["T"], c["JQ"], c["w"])
    return R.host_plan_words(*shape), host_bwd_plan_words(*shape)


def reference(c):
    """fp64 autograd -> dict(h_a, a_logits, dh [A,K,T,w], dq, dW [F], db [1])"""
    from oracle import fvta_fused as F
    al = c["album"]
    h, q, W, b = (t.double().requires_grad_() for t in (c["h"], c["q"], c["W"], c["b"]))
    hm = None if c["hm"] is None else c["hm"][al]
    ha, a = F.attention_3d(h[al], q, W, b, hm, c["qm"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    (ha * c["gout"].double()).sum().backward()
    dh = h.grad if h.grad is not None else torch.zeros_like(h)
    return dict(h_a=ha.detach(), a_logits=a.detach(), dh=dh, dq=q.grad, dW=W.grad.reshape(-1), db=b.grad.reshape(-1))


valid_mask, conditions, qualifies = AR.shared(AR.valid_mask), AR.shared(AR.conditions), AR.shared(AR.qualifies)


# ------------------------------------------------------------------ a width no kernel has (channel padding): w = 100
def odd_width_case():
    c = R.make_case([2, 1], 2, 20, 5, 100, 2, True, 4242)
    return AR.train_inputs(c, c["hm"], True)         # (every (album, k) has a valid row: the parity's last line changes none)
