"""fp64 references and seeded inputs for the shared-context focal attention (fvta_attn_shared_fwd): NQ questions over A
albums whose context rows [A,K,T,w] are held once, question i attending album[i].

`reference` is the definition: gather the album's rows per question, then oracle.fvta_fused.attention_3d.
`grouped` is an independent restatement in the order the kernels work in: tests/_album_attn_ref.grouped, the album pool's
at one album per question.  tests/test_attn_shared_host.py holds the two against each other on every shape the GPU tests
use (SPECS, and LOOP_SPECS: the shapes with many albums and many questions)."""
import torch

from tests import _album_attn_ref as AR

NEG = AR.NEG
SIMI_TANH = [(1, False), (2, True), (3, True), (4, False)]      # the parametrisation of tests/test_gpu_forward.py


# ------------------------------------------------------------------ inputs
def make_case(counts, K, T, JQ, w, simi, masked, seed):
    """counts[a] = questions about album a (0 allowed); the questions are shuffled.  The recipe of
    tests/test_gpu_forward.py::_att_case: rows and questions randn * 0.5, hmask p = 0.6 with (album 0, k 0) fully masked and
    (album 0, k 1) down to a single valid row, qmask p = 0.8 with column 0 valid and the LAST question fully masked."""
    g = torch.Generator().manual_seed(seed)
    A, NQ = len(counts), sum(counts)
    h = torch.randn(A, K, T, w, generator=g) * 0.5
    q = torch.randn(NQ, JQ, w, generator=g) * 0.5
    F_ = {1: 3 * w, 2: 2 * w, 3: 4 * w, 4: 0}[simi]
    W = torch.randn(F_, 1, generator=g) * 0.1 if F_ else None
    b = torch.randn(1, generator=g) * 0.1 if F_ else None
    album = torch.cat([torch.full((c,), a, dtype=torch.int64) for a, c in enumerate(counts)])
    album = album[torch.randperm(NQ, generator=g)]
    if masked:
        hm = torch.rand(A, K, T, generator=g) < 0.6
        qm = torch.rand(NQ, JQ, generator=g) < 0.8
        qm[:, 0] = True
        hm[0, 0] = False
        if NQ > 1:
            qm[NQ - 1] = False
        if K > 1:
            hm[0, 1] = False
            hm[0, 1, T // 2] = True
    else:
        hm = qm = None
    return dict(h=h, q=q, W=W, b=b, hm=hm, qm=qm, album=album, simi=simi, A=A, NQ=NQ, K=K, T=T, JQ=JQ, w=w)


# every shape of tests/test_gpu_attn_shared.py: (name, counts(G), K, T(R), JQ, w, [(simi, tanh, masked), ...]); G and R are
# what fvta_attn_shared_plan reports for the shape's JQ (questions per group, rows per logits tile)
def _specs():
    out = []
    # questions per album 1, G, G+1, 2G+1 in one call, one album without a question
    out.append(("mix", lambda G: [G + 1, 1, 0, 2 * G + 1, G], 2, lambda R: 50, 10, 64,
                [(s, t, m) for s, t in SIMI_TANH for m in (True, False)]))
    for i, T in enumerate([lambda R: 1, lambda R: 7, lambda R: R - 1, lambda R: R, lambda R: R + 1, lambda R: 333]):
        s, t = SIMI_TANH[i % 4]
        out.append(("rows%d" % i, lambda G: [G - 1, 2], 3, T, 7, 256, [(s, t, True)]))
    for i, (JQ, w) in enumerate([(JQ, w) for JQ in (1, 30, 32, 33, 64) for w in (128, 512)]):
        s, t = SIMI_TANH[i % 4]
        out.append(("cols_jq%d_w%d" % (JQ, w), lambda G: [G, 1], 2, lambda R: 40, JQ, w, [(s, t, i % 3 != 2)]))
    out.append(("wide1024", lambda G: [3, 2], 2, lambda R: 70, 30, 1024, [(2, True, True)]))
    out.append(("wide2048", lambda G: [3, 2], 2, lambda R: 70, 30, 2048, [(3, True, True), (4, False, False)]))
    out.append(("single", lambda G: [1], 2, lambda R: 50, 10, 64, [(1, False, True), (2, True, False)]))
    out.append(("k6", lambda G: [2, 1], 6, lambda R: 50, 10, 64, [(3, True, True)]))
    return out


SPECS = _specs()
CASES = [(name, s, t, m) for name, _, _, _, _, _, variants in SPECS for s, t, m in variants]
CASE_IDS = ["%s-simi%d-%s" % (name, s, "masked" if m else "open") for name, s, t, m in CASES]


def host_plan(JQ, w=64):
    """(G, R) of fvta_attn_shared_plan: a host-only call, it needs the built library but no GPU"""
    p = host_plan_words(1, 1, 1, 1, JQ, w)
    return p["G"], p["rows"]


def host_plan_words(A, NQ, K, T, JQ, w):
    """all four words of fvta_attn_shared_plan for a whole shape, named as ops.SharedFocalAttention.plan() names them"""
    import ctypes
    from fvta_memexqa_amd import _lib
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().fvta_attn_shared_plan(ctypes.byref(_lib.AttnSharedDesc(A, NQ, K, T, JQ, w, 1, 0)), out) == 0
    return dict(zip(("G", "rows", "tsplit", "rows_per_split"), (int(v) for v in out)))


def build_case(name, simi, masked):
    spec = next(s for s in SPECS if s[0] == name)
    _, counts, K, T, JQ, w, _ = spec
    G, R = host_plan(JQ, w)
    seed = sum(map(ord, name)) * 10 + simi + (5 if masked else 0)
    return make_case(counts(G), K, T(R), JQ, w, simi, masked, seed)


# ------------------------------------------------------------------ past one round of the plan and tile loops
# Shapes tiny in T, JQ and w but NOT in what the shared context is for -- many albums, many questions -- each the smallest
# that reaches its loop.  (name, counts(G), K, T, JQ, w, simi, tanh, masked), the tuple of tests/_attn_shared_bwd_ref.py,
# which runs all but `chunks` through the backward as well.  loop_regime() states what each one reaches:
#   many         A = 1500, NQ = 1284: a plan thread owns two albums and carries its running offsets across them; 21
#                ordered batches of 64 questions; the strided counting and placing loops; ngmax clamped to NQ; one T split
#   heavy        [150, 0, 50]: one album's cursor advanced by every ordered batch, 19 groups of one album, a 150-question
#                row pass
#   chunks       [2] x 120, T = 200 (forward only): the weighted sum's splits hold more than SH_CH = 64 rows and no multiple
#                of it: a second, ragged round of its staging loop
#   tiles-w64    A = 260, five albums with questions, T = 260: the backward's row pass walks two tiles per workgroup, the
#                last workgroup of an (album, k) one; albums without a question walk them too
#   tiles-w512   two tiles per workgroup where two waves share a row;  tiles-w2048  where a thread holds two float4 per row
#   k17, k64     the backward's per-k wave loop a second and a fourth time; K at its limit of 64
#   splits9      [2, 1], K = 1, T = 513: the backward's question pass cuts T into nine splits, so its fold sums a question's
#                slots as one full round of eight loads in flight and a remainder of one
PLAN_THREADS = 1024          # SH_PLAN_NT: threads of the plan's single workgroup
PLAN_BATCH = 64              # questions per batch of the ordered (training) plan
WSUM_CHUNK = 64              # SH_CH: rows the weighted sum stages at a time


def _many_counts(G):
    return [2 * G + 1 if a % 97 == 0 else G if a % 41 == 0 else 1 if a % 2 == 0 else 0 for a in range(1500)]


def _sparse_counts(A, at):
    return lambda G: [at.get(a, 0) for a in range(A)]


LOOP_SPECS = [
    ("many", _many_counts, 1, lambda Rb: 5, 3, 64, 2, True, True),
    ("heavy", lambda G: [150, 0, 50], 2, lambda Rb: 40, 3, 64, 3, True, True),
    ("chunks", lambda G: [2] * 120, 3, lambda Rb: 200, 5, 64, 1, False, True),
    ("tiles-w64", _sparse_counts(260, {0: 9, 3: 1, 7: 17, 100: 8, 259: 5}), 2, lambda Rb: 260, 4, 64, 1, False, True),
    ("tiles-w512", _sparse_counts(40, {0: 5, 1: 1, 20: 4, 39: 2}), 2, lambda Rb: 220, 4, 512, 2, True, True),
    ("tiles-w2048", _sparse_counts(6, {0: 3, 2: 1, 5: 3}), 2, lambda Rb: 360, 4, 2048, 3, True, False),
    ("k17", lambda G: [3, 2], 17, lambda Rb: 9, 4, 64, 2, True, True),
    ("k64", lambda G: [3, 2], 64, lambda Rb: 9, 4, 64, 3, True, True),
    ("splits9", lambda G: [2, 1], 1, lambda Rb: 513, 4, 64, 1, False, True),
]
LOOP_IDS = [s[0] for s in LOOP_SPECS]
FORWARD_ONLY = ["chunks"]
CHUNKS_SEED = sum(map(ord, "chunks")) * 10      # no arg-max condition on a forward: the first candidate


def train_recipe(counts, K, T, JQ, w, simi, tanh, masked, seed, parity=True):
    """The recipe of tests/_attn_shared_bwd_ref.build_case: make_case with att_logits/W scaled by sqrt(64 / w) (the logits
    stay clear of tanh's saturation at every width), d_h_a = randn of seed 99 and -- parity, as tests/test_gpu_backward.py --
    every (album, k) and every question partly valid (the fully masked ones carry fvta_attn_bwd's documented deviation)."""
    c = make_case(counts, K, T, JQ, w, simi, masked, seed)
    return AR.train_inputs(c, c["hm"], tanh, parity)


def loop_case(name, seed):
    _, counts, K, T, JQ, w, simi, tanh, masked = next(s for s in LOOP_SPECS if s[0] == name)
    return train_recipe(counts(host_plan(JQ, w)[0]), K, T(0), JQ, w, simi, tanh, masked, seed)


def loop_regime(name, c, plan, bwd_plan=None):
    """Asserts that case c of LOOP_SPECS reaches the code it is there for.  plan / bwd_plan: the words of
    fvta_attn_shared_plan / fvta_attn_shared_bwd_plan for c's shape, as ops.SharedFocalAttention.plan() / bwd_plan() name
    them (bwd_plan None: a forward-only case).  Other names pass.  A retuned constant that moves a shape out of its regime
    fails here: then the SHAPE changes."""
    if name not in LOOP_IDS:
        return
    A, NQ, K, T, G = c["A"], c["NQ"], c["K"], c["T"], plan["G"]
    cnt = torch.bincount(c["album"], minlength=A)
    assert c["album"].tolist() != sorted(c["album"].tolist())                          # shuffled
    if name == "many":
        assert A > PLAN_THREADS and NQ > PLAN_THREADS, (A, NQ)                          # albums per thread 2, strided loops
        assert NQ // G + min(A, NQ) > NQ                                                # ngmax clamped to NQ
        assert {0, 1, G, 2 * G + 1} == set(cnt.tolist()) and plan["tsplit"] == 1
    elif name == "heavy":
        assert NQ > 3 * PLAN_BATCH and int(cnt.max()) > 2 * PLAN_BATCH and int(cnt.min()) == 0
        assert -(-int(cnt.max()) // G) >= 19, G                                         # groups of ONE album
    elif name == "chunks":
        rps, S = plan["rows_per_split"], plan["tsplit"]
        last = T - (S - 1) * rps
        assert rps > WSUM_CHUNK and rps % WSUM_CHUNK != 0, plan
        assert S >= 2 and last > WSUM_CHUNK and last % WSUM_CHUNK != 0, (plan, last)
    elif name.startswith("tiles-"):
        ntb = -(-T // bwd_plan["rows"])
        assert bwd_plan["tiles_per_wg"] >= 2, bwd_plan
        assert int((cnt == 0).sum()) > 0 and int(cnt[0]) > 0
        if name == "tiles-w64":
            assert ntb % bwd_plan["tiles_per_wg"] != 0, (ntb, bwd_plan)                 # a ragged last chunk of tiles
        assert c["w"] == int(name[len("tiles-w"):])
    elif name in ("k17", "k64"):
        assert K == int(name[1:])
    elif name == "splits9":
        assert bwd_plan["tsplit"] >= 9 and bwd_plan["tsplit"] % 8 != 0, bwd_plan       # a full round of eight and a rest


# ------------------------------------------------------------------ references (fp64, CPU)
_dd = AR._dd


def reference(c, tanh, block=None):
    """the definition: rows gathered per question, oracle.fvta_fused.attention_3d -> (h_a [NQ,w], a_logits [NQ,K,T,JQ]);
    block: that many questions at a time (the gathered rows of all of them at once would not fit)"""
    from oracle import fvta_fused as F
    if block is not None and block < c["NQ"]:
        parts = []
        for i in range(0, c["NQ"], block):
            sub = dict(c, q=c["q"][i:i + block], album=c["album"][i:i + block],
                       qm=None if c["qm"] is None else c["qm"][i:i + block])
            parts.append(reference(sub, tanh))
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    al = c["album"]
    hm = None if c["hm"] is None else c["hm"][al]
    return F.attention_3d(_dd(c["h"])[al], _dd(c["q"]), _dd(c["W"]), _dd(c["b"]), hm, c["qm"], simiMatrix=c["simi"],
                          add_tanh=tanh)


grouped = AR.shared(AR.grouped)          # album by album, one product for all of the album's questions -> (h_a, a_logits)


# ------------------------------------------------------------------ the tiny end-to-end graph
E2E = dict(A=2, M=2, J=(5, 3), din=8, hidden=32, JQ=6, C=4, NQ=5, simi=2, tanh=True, seed=3, margin=1e-3)


def e2e_case():
    """Seeded inputs AND parameters (generated here, on the CPU, and copied into the nn modules by the GPU test) of: two
    bi-LSTM streams -> context tensor -> focal attention -> question attention -> scorer."""
    e = E2E
    g = torch.Generator().manual_seed(e["seed"])
    d, w = e["hidden"], 2 * e["hidden"]
    c = dict(e)
    c["x"] = [torch.randn(e["A"] * e["M"], J, e["din"], generator=g) for J in e["J"]]
    c["lens"] = [torch.randint(1, J + 1, (e["A"] * e["M"],), generator=g) for J in e["J"]]
    lim = (6.0 / (e["din"] + 5 * d)) ** 0.5
    c["lstm_k"] = [(torch.rand(e["din"] + d, 4 * d, generator=g) * 2 - 1) * lim * 2 for _ in e["J"]]
    c["lstm_b"] = [torch.randn(4 * d, generator=g) * 0.1 for _ in e["J"]]
    c["hq"] = torch.randn(e["NQ"], e["JQ"], w, generator=g) * 0.5
    c["qlen"] = torch.tensor([6, 3, 5, 1, 4])
    c["album"] = torch.tensor([1, 0, 1, 1, 0])
    c["gch"] = torch.randn(e["NQ"], e["C"], w, generator=g) * 0.5
    c["att_W"], c["att_b"] = torch.randn(2 * w, 1, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1
    c["qatt_W"], c["qatt_b"] = torch.randn(2 * w, 1, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1
    c["out_W"], c["out_b"] = torch.randn(5 * w, 1, generator=g) * 0.3, torch.randn(1, generator=g) * 0.1
    return c


def e2e_reference(c):
    """(logits [NQ,C], yp [NQ,C]) in fp64 through oracle.fvta_fused"""
    from oracle import fvta_fused as F
    A, M = c["A"], c["M"]
    hs, ms = [], []
    for x, ln, k, b in zip(c["x"], c["lens"], c["lstm_k"], c["lstm_b"]):
        mask = torch.arange(x.shape[1])[None, :] < ln[:, None]
        out, _ = F.encode_stream(x.double(), mask, k.double(), b.double())
        hs.append(out.reshape(A, M, x.shape[1], -1))
        ms.append(mask.reshape(A, M, -1))
    hall, hmask = F.context_tensor(hs, ms)
    al = c["album"]
    qmask = torch.arange(c["JQ"])[None, :] < c["qlen"][:, None]
    hq = c["hq"].double()
    g1, _ = F.attention_3d(hall[al], hq, c["att_W"].double(), c["att_b"].double(), hmask[al], qmask, simiMatrix=c["simi"],
                           add_tanh=c["tanh"])
    gq, _ = F.attention(hq, g1[:, None, :], c["qatt_W"].double(), c["qatt_b"].double(), qmask,
                        torch.ones(c["NQ"], 1, dtype=torch.bool), simiMatrix=c["simi"], add_tanh=c["tanh"])
    return F.scorer(gq, g1, c["gch"].double(), c["out_W"].double(), c["out_b"].double())


def top2_margin(yp):
    top = torch.sort(yp, dim=-1, descending=True).values
    return top[:, 0] - top[:, 1]
