"""fp64 references and seeded inputs for the shared-context focal attention (fvta_attn_shared_fwd): NQ questions over A
albums whose context rows [A,K,T,w] are held once, question i attending album[i].

`reference` is the definition: gather the album's rows per question, then oracle.fvta_fused.attention_3d.
`grouped` is an independent restatement in the order the kernels work in: the logits of ALL questions of an album from one
[K*T, w] x [w, nq*JQ] product, written out from att_logits/W per similarity (not through the oracle's helpers), the mask
as a select, the two softmaxes by hand.  tests/test_attn_shared_host.py holds the two against each other on every shape
the GPU tests use (SPECS)."""
import torch

NEG = -1e30
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
    import ctypes
    from fvta_memexqa_amd import _lib
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().fvta_attn_shared_plan(ctypes.byref(_lib.AttnSharedDesc(1, 1, 1, 1, JQ, w, 1, 0)), out) == 0
    return int(out[0]), int(out[1])


def build_case(name, simi, masked):
    spec = next(s for s in SPECS if s[0] == name)
    _, counts, K, T, JQ, w, _ = spec
    G, R = host_plan(JQ, w)
    seed = sum(map(ord, name)) * 10 + simi + (5 if masked else 0)
    return make_case(counts(G), K, T(R), JQ, w, simi, masked, seed)


# ------------------------------------------------------------------ references (fp64, CPU)
def _dd(t):
    return None if t is None else t.double()


def reference(c, tanh):
    """the definition: rows gathered per question, oracle.fvta_fused.attention_3d -> (h_a [NQ,w], a_logits [NQ,K,T,JQ])"""
    from oracle import fvta_fused as F
    al = c["album"]
    hm = None if c["hm"] is None else c["hm"][al]
    return F.attention_3d(_dd(c["h"])[al], _dd(c["q"]), _dd(c["W"]), _dd(c["b"]), hm, c["qm"], simiMatrix=c["simi"],
                          add_tanh=tanh)


def _softmax_last(x):
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def grouped(c, tanh):
    """album by album: one product for all of the album's questions"""
    h, q, al, simi = _dd(c["h"]), _dd(c["q"]), c["album"], c["simi"]
    A, K, T, w = h.shape
    NQ, JQ = q.shape[:2]
    W = None if c["W"] is None else _dd(c["W"]).reshape(-1)
    b = None if c["b"] is None else float(c["b"])
    h_a = torch.zeros(NQ, w, dtype=torch.float64)
    logits = torch.zeros(NQ, K, T, JQ, dtype=torch.float64)
    for a in range(A):
        qi = torch.nonzero(al == a).reshape(-1)
        if qi.numel() == 0:
            continue
        nq = qi.numel()
        H = h[a].reshape(K * T, w)
        Q = q[qi].reshape(nq * JQ, w)
        if simi == 1:        # [h, q, h*q] . W
            x = (H * W[2 * w:]) @ Q.t() + (H @ W[:w])[:, None] + (Q @ W[w:2 * w])[None, :] + b
        elif simi == 2:      # [h*q, (h-q)^2] . W
            Wd = W[w:]
            x = (H * (W[:w] - 2 * Wd)) @ Q.t() + ((H * H) @ Wd)[:, None] + ((Q * Q) @ Wd)[None, :] + b
        elif simi == 3:      # [h, q, (h-q)^2, h*q] . W
            Wd = W[2 * w:3 * w]
            x = (H * (W[3 * w:] - 2 * Wd)) @ Q.t() + (H @ W[:w] + (H * H) @ Wd)[:, None] \
                + (Q @ W[w:2 * w] + (Q * Q) @ Wd)[None, :] + b
        else:                # cosine
            Hn = H / torch.sqrt(torch.clamp((H * H).sum(1, keepdim=True), min=1e-12))
            Qn = Q / torch.sqrt(torch.clamp((Q * Q).sum(1, keepdim=True), min=1e-12))
            x = Hn @ Qn.t()
        if tanh and simi != 4:
            x = torch.tanh(x)
        x = x.reshape(K, T, nq, JQ).permute(2, 0, 1, 3)                 # [nq,K,T,JQ]
        if c["hm"] is not None and c["qm"] is not None:
            valid = c["hm"][a][None, :, :, None] & c["qm"][qi][:, None, None, :]
            x = torch.where(valid, x, torch.full_like(x, NEG))
        amax = x.max(-1).values                                          # [nq,K,T]
        p = _softmax_last(amax)
        u = torch.einsum("gkt,ktc->gkc", p, h[a])
        r = _softmax_last(amax.max(-1).values)                           # [nq,K]
        h_a[qi] = torch.einsum("gk,gkc->gc", r, u)
        logits[qi] = x
    return h_a, logits


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
