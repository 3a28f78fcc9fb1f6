"""fp64 references and seeded inputs for the focal attention over per-question album lists from one album pool
(fvta_attn_pool_fwd): pool [P,K,JX,w] holds every encoded album once, question i lists albums[i, :] (-1: an empty slot)
and attends those albums' rows laid end to end, T = M * JX.

`reference` is the definition: the context of every question assembled by concatenation (zeros and mask 0 for an empty
slot), then oracle.fvta_fused.attention_3d.  `grouped` (tests/_album_attn_ref.py) is an independent restatement in the
order the kernels work in.  tests/test_attn_pooled_host.py holds the two against each other on every shape the GPU tests
use (SPECS and LOOP_SPECS)."""
import torch

from tests import _album_attn_ref as AR

NEG = AR.NEG
SIMI_TANH = [(1, False), (2, True), (3, True), (4, False)]      # the parametrisation of tests/test_gpu_forward.py
PLAN_THREADS = 1024          # threads of the plan's single workgroup
WSUM_CHUNK = 64              # rows the weighted sum stages at a time


# ------------------------------------------------------------------ inputs
def lists_from_counts(counts, M, seed, masked):
    """album lists [NQ,M] with counts[p] references to album p: the multiset of references flattened, shuffled with the
    seed, cut into rows of M, the tail padded with -1.  Open (unmasked) cases may hold no -1: the album with the most
    references is topped up until the total divides by M."""
    counts = list(counts)
    if not masked:
        counts[max(range(len(counts)), key=lambda p: counts[p])] += -sum(counts) % M
    refs = torch.cat([torch.full((c,), p, dtype=torch.int64) for p, c in enumerate(counts)])
    refs = refs[torch.randperm(refs.numel(), generator=torch.Generator().manual_seed(seed))]
    refs = torch.cat([refs, torch.full((-refs.numel() % M,), -1, dtype=torch.int64)])
    return refs.reshape(-1, M)


def make_case(albums, P, K, JX, JQ, w, simi, masked, seed):
    """The recipe of tests/_attn_shared_ref.make_case on a pool: rows and questions randn * 0.5, pool mask p = 0.6 with
    (album 0, k 0) fully masked and (album 0, k 1) down to a single valid row, question mask p = 0.8 with column 0 valid and
    the LAST question fully masked."""
    g = torch.Generator().manual_seed(seed)
    albums = torch.as_tensor(albums, dtype=torch.int64)
    NQ, M = albums.shape
    pool = torch.randn(P, K, JX, w, generator=g) * 0.5
    q = torch.randn(NQ, JQ, w, generator=g) * 0.5
    F_ = {1: 3 * w, 2: 2 * w, 3: 4 * w, 4: 0}[simi]
    W = torch.randn(F_, 1, generator=g) * 0.1 if F_ else None
    b = torch.randn(1, generator=g) * 0.1 if F_ else None
    if masked:
        pm = torch.rand(P, K, JX, generator=g) < 0.6
        qm = torch.rand(NQ, JQ, generator=g) < 0.8
        qm[:, 0] = True
        pm[0, 0] = False
        if NQ > 1:
            qm[NQ - 1] = False
        if K > 1:
            pm[0, 1] = False
            pm[0, 1, JX // 2] = True
    else:
        assert int(albums.min()) >= 0, "an empty slot needs masks"
        pm = qm = None
    return dict(pool=pool, q=q, W=W, b=b, pm=pm, qm=qm, albums=albums, simi=simi, P=P, NQ=NQ, M=M, K=K, JX=JX, T=M * JX,
                JQ=JQ, w=w)


def host_plan_words(P, NQ, M, K, JX, JQ, w):
    """the four words of fvta_attn_pool_plan, named as ops.PooledFocalAttention.plan() names them: a host-only call, it
    needs the built library but no GPU"""
    import ctypes
    from fvta_memexqa_amd import _lib
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().fvta_attn_pool_plan(ctypes.byref(_lib.AttnPoolDesc(P, NQ, M, K, JX, JQ, w, 1, 0)), out) == 0
    return dict(zip(("G", "rows", "tsplit", "rows_per_split"), (int(v) for v in out)))


def host_plan(JQ, w=64):
    """(G, R): references per group and rows per logits tile for this JQ"""
    p = host_plan_words(1, 1, 1, 1, 1, JQ, w)
    return p["G"], p["rows"]


# every fp64-reference shape of tests/test_gpu_attn_pooled.py:
# (name, P, lists(G, masked) -> [NQ,M], K, JX(R), JQ, w, [(simi, tanh, masked), ...])
def _counted(counts, M, name):
    return lambda G, masked: lists_from_counts(counts(G), M, sum(map(ord, name)), masked)


def _specs():
    out = []
    # references per album G+1, 1, 0, 2G+1, G in one call; 4G+3 references in rows of three: an empty slot (masked), and
    # more references to album 3 than there are questions: some question lists it twice
    out.append(("mix", 5, _counted(lambda G: [G + 1, 1, 0, 2 * G + 1, G], 3, "mix"), 2, lambda R: 17, 10, 64,
                [(s, t, m) for s, t in SIMI_TANH for m in (True, False)]))
    for i, JX in enumerate([lambda R: 1, lambda R: 7, lambda R: R - 1, lambda R: R, lambda R: R + 1, lambda R: 200]):
        s, t = SIMI_TANH[i % 4]
        out.append(("rows%d" % i, 3, _counted(lambda G: [G - 1, 2, 2], 2, "rows"), 3, JX, 7, 256, [(s, t, True)]))
    for i, (JQ, w) in enumerate([(JQ, w) for JQ in (1, 30, 32, 33, 64) for w in (128, 512)]):
        s, t = SIMI_TANH[i % 4]
        out.append(("cols_jq%d_w%d" % (JQ, w), 2, _counted(lambda G: [G, 1], 2, "cols"), 2, lambda R: 40, JQ, w,
                    [(s, t, i % 3 != 2)]))
    out.append(("wide1024", 2, _counted(lambda G: [3, 2], 2, "wide"), 2, lambda R: 70, 30, 1024, [(2, True, True)]))
    out.append(("wide2048", 2, _counted(lambda G: [3, 2], 2, "wide"), 2, lambda R: 70, 30, 2048,
                [(3, True, True), (4, False, False)]))
    out.append(("slots9", 4, _counted(lambda G: [10, 1, 9, 4], 9, "slots9"), 2, lambda R: 5, 10, 64, [(2, True, True)]))
    out.append(("k6", 2, _counted(lambda G: [2, 1], 2, "k6"), 6, lambda R: 17, 10, 64, [(3, True, True)]))
    out.append(("single", 1, lambda G, masked: torch.zeros(1, 1, dtype=torch.int64), 2, lambda R: 50, 10, 64,
                [(1, False, True), (2, True, False)]))
    # question 1 lists nothing at all; question 2 (the last: fully masked by the recipe) has one empty slot
    out.append(("all-empty", 2, lambda G, masked: torch.tensor([[0, 1], [-1, -1], [1, -1]]), 2, lambda R: 17, 10, 64,
                [(1, False, True), (3, True, True)]))
    return out


SPECS = _specs()
CASES = [(name, s, t, m) for name, _, _, _, _, _, _, variants in SPECS for s, t, m in variants]
CASE_IDS = ["%s-simi%d-%s" % (name, s, "masked" if m else "open") for name, s, t, m in CASES]


def build_case(name, simi, masked):
    _, P, lists, K, JX, JQ, w, _ = next(s for s in SPECS if s[0] == name)
    G, R = host_plan(JQ, w)
    seed = sum(map(ord, name)) * 10 + simi + (5 if masked else 0)
    return make_case(lists(G, masked), P, K, JX(R), JQ, w, simi, masked, seed)


# ------------------------------------------------------------------ past one round of the plan and weighted-sum loops
#   many     P = 1500, NQ = 400, M = 4: 1600 references -- the strided counting and placing loops, two albums per plan
#            thread, ngmax clamped to NQ M; albums with 0, 1, G and 2G+1 references
#   heavy    [150, 0, 50] references: 19 groups of ONE album (and questions that list it four times)
#   chunks   [2] x 120, JX = 200: a split of the weighted sum holds more than 64 rows and no multiple of 64
def _many_counts(G):
    c = [2 * G + 1 if p % 97 == 0 else G if p % 41 == 0 else 1 if p % 2 == 0 else 0 for p in range(1500)]
    for p in range(1499, 0, -2):                 # odd albums, from the end: one reference each until 1600 are named
        if sum(c) >= 1600:
            break
        if c[p] == 0:
            c[p] = 1
    return c


# (name, P, counts(G), M, K, JX, JQ, w, simi, tanh)  -- all masked
LOOP_SPECS = [
    ("many", 1500, _many_counts, 4, 1, 3, 2, 64, 2, True),
    ("heavy", 3, lambda G: [150, 0, 50], 4, 2, 9, 3, 64, 3, True),
    ("chunks", 120, lambda G: [2] * 120, 2, 3, 200, 5, 64, 1, False),
]
LOOP_IDS = [s[0] for s in LOOP_SPECS]


def loop_case(name):
    _, P, counts, M, K, JX, JQ, w, simi, tanh = next(s for s in LOOP_SPECS if s[0] == name)
    seed = sum(map(ord, name)) * 10
    c = make_case(lists_from_counts(counts(host_plan(JQ, w)[0]), M, seed, True), P, K, JX, JQ, w, simi, True, seed)
    c["tanh"] = tanh
    return c


def loop_regime(name, c, plan):
    """Asserts that case c of LOOP_SPECS reaches the code it is there for; plan: the words of fvta_attn_pool_plan for c's
    shape.  A retuned constant that moves a shape out of its regime fails here: then the SHAPE changes."""
    P, NR, G = c["P"], c["NQ"] * c["M"], plan["G"]
    al = c["albums"].reshape(-1)
    cnt = torch.bincount(al[al >= 0], minlength=P)
    if name == "many":
        assert (c["NQ"], c["M"]) == (400, 4) and P > PLAN_THREADS and NR > PLAN_THREADS       # strided loops, 2 albums a thread
        assert NR // G + min(P, NR) > NR                                                      # ngmax clamped to NQ M
        assert {0, 1, G, 2 * G + 1} == set(cnt.tolist()) and plan["tsplit"] == 1
    elif name == "heavy":
        assert int(cnt.max()) == 150 and -(-150 // G) >= 19 and int(cnt.min()) == 0, G         # groups of ONE album
        assert int((c["albums"] == 0).sum(1).max()) >= 2                                       # an album twice in a list
    elif name == "chunks":
        rps, S = plan["rows_per_split"], plan["tsplit"]
        last = c["JX"] - (S - 1) * rps
        assert rps > WSUM_CHUNK and rps % WSUM_CHUNK != 0, plan
        assert S >= 2 and last > WSUM_CHUNK and last % WSUM_CHUNK != 0, (plan, last)


# ------------------------------------------------------------------ references (fp64, CPU)
_dd, grouped = AR._dd, AR.grouped


def expand(c):
    """(hinfo [NQ,K,T,w], mask [NQ,K,T] or None): every question's context by concatenation of its albums' rows"""
    al, pool, pm = c["albums"], c["pool"], c["pm"]
    P, K, JX, w = pool.shape
    zero, off = torch.zeros(K, JX, w, dtype=pool.dtype), torch.zeros(K, JX, dtype=torch.bool)
    h = torch.stack([torch.cat([pool[p] if p >= 0 else zero for p in row], 1) for row in al.tolist()])
    m = None if pm is None else torch.stack([torch.cat([pm[p] if p >= 0 else off for p in row], 1) for row in al.tolist()])
    return h, m


def reference(c, tanh):
    """the definition -> (h_a [NQ,w], a_logits [NQ,K,T,JQ])"""
    from oracle import fvta_fused as F
    h, m = expand(c)
    return F.attention_3d(_dd(h), _dd(c["q"]), _dd(c["W"]), _dd(c["b"]), m, c["qm"], simiMatrix=c["simi"], add_tanh=tanh)
