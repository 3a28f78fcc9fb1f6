"""fp64 references and seeded inputs for the shared-context focal attention UNDER THE TIME WARP (fvta_attn_shared_fwd_tw):
NQ questions over A albums whose rows [A,K,T,w] are held once; question i attends album[i]'s rows warped by its own last
state lq[i] (model_v2.py:953-1009, use_time_warp without use_time_warp_att).

`reference` is the definition: gather the album's rows per question, oracle.fvta_fused.time_warp_closed, then
oracle.fvta_fused.attention_3d on the warped rows.
`factored` is the restatement the kernels compute, written out independently and parametrised by dtype
(tests/_album_attn_ref.factored, the album pool's at one album per question): the warp as one scalar per (question,
position), whose only term that reads the rows -- the energy e [A,T] -- is taken per ALBUM, the scalar passed through the
bilinear form of the logits and through the weighted sum; no [NQ,K,T,w] tensor.
tests/test_attn_shared_tw_host.py holds the two against each other on every shape the GPU tests use.

Inputs: tests/_attn_shared_ref.make_case, and the warp parameters by the recipe of tests/test_gpu_timewarp.py (WH/W scaled
0.3 / sqrt(w), WC/W 0.5 / sqrt(w), biases 0.1, lq 0.5)."""
import torch

from tests import _album_attn_ref as AR
from tests import _attn_shared_ref as R

NEG = R.NEG
WINDOW_T = 2.3
TOL, within, _count, _dd = AR.TOL, AR.within, AR.count, AR._dd


# ------------------------------------------------------------------ inputs
def add_warp(c, seed, warp_type, window_t=WINDOW_T):
    """the time warp's parameters and the questions' last states, seeded apart from the attention's inputs"""
    g = torch.Generator().manual_seed(seed * 7 + 11)
    w, NQ = c["w"], c["NQ"]
    c = dict(c)
    c["lq"] = torch.randn(NQ, w, generator=g) * 0.5
    c["WH_W"] = torch.randn(2 * w, w, generator=g) * (0.3 / w ** 0.5)
    c["WH_b"] = torch.randn(w, generator=g) * 0.1
    c["WC_W"] = torch.randn(w, 1, generator=g) * (0.5 / w ** 0.5)
    c["WC_b"] = torch.randn(1, generator=g) * 0.1
    c["warp_type"], c["window_t"] = warp_type, window_t
    return c


# (name, counts(G), K, T(R), JQ, w, simi, tanh, masked, warp_type, window_t); G and R: fvta_attn_shared_plan's words.
# Warp types 1, 3 and 4 multiply the rows by counts up to T, so the fp32 rounding of the warped rows' logits grows with T
# while the a_logits tolerance stays absolute: they come at T in {1, 7, 9} only, where the counts stay below 10; types 2
# and 5 (counts of at most 2 ceil(window_t) + 1) at every shape.
def _specs():
    mix = lambda G: [G + 1, 1, 0, 2 * G + 1, G]
    two = lambda G: [G - 1, 2]
    out = []
    for s, t in R.SIMI_TANH:
        for m in (True, False):
            out.append(("mix-simi%d-%s" % (s, "masked" if m else "open"), mix, 2, lambda Rr: 50, 10, 64, s, t, m, 5, WINDOW_T))
    out.append(("mix-warp2", mix, 2, lambda Rr: 50, 10, 64, 2, True, True, 2, WINDOW_T))
    for T in (1, 7, 9):
        for wt in (1, 3, 4):
            for s, t in R.SIMI_TANH:
                out.append(("short-T%d-warp%d-simi%d" % (T, wt, s), two, 3, (lambda T: lambda Rr: T)(T), 7, 256, s, t, True, wt,
                            WINDOW_T))
    for i, (nm, T) in enumerate([("Rm1", lambda Rr: Rr - 1), ("R", lambda Rr: Rr), ("Rp1", lambda Rr: Rr + 1), ("333", lambda Rr: 333)]):
        s, t = R.SIMI_TANH[i % 4]
        out.append(("tile-T%s" % nm, two, 3, T, 7, 256, s, t, True, 5, WINDOW_T))
    out.append(("window0.5-T7", two, 3, lambda Rr: 7, 7, 256, 2, True, True, 5, 0.5))
    out.append(("window3.0-T7", two, 3, lambda Rr: 7, 7, 256, 3, True, True, 5, 3.0))
    out.append(("window7.0-T5", two, 3, lambda Rr: 5, 7, 256, 1, False, True, 5, 7.0))      # the band wider than T
    for i, (JQ, w) in enumerate([(JQ, w) for JQ in (32, 33, 64) for w in (128, 512)]):
        s, t = R.SIMI_TANH[i % 4]
        out.append(("cols-jq%d-w%d" % (JQ, w), lambda G: [G, 1], 2, lambda Rr: 40, JQ, w, s, t, i % 3 != 2, 5, WINDOW_T))
    out.append(("wide1024", lambda G: [3, 2], 2, lambda Rr: 70, 30, 1024, 2, True, True, 5, WINDOW_T))
    out.append(("wide2048", lambda G: [3, 2], 2, lambda Rr: 70, 30, 2048, 4, False, True, 5, WINDOW_T))
    out.append(("k9", lambda G: [2, 1], 9, lambda Rr: 50, 10, 64, 3, True, True, 5, WINDOW_T))
    return out


SPECS = _specs()
NAMES = [s[0] for s in SPECS]
EXTRA = ["chunks", "zero-rows-simi2", "zero-rows-simi4"]


def build_case(name):
    """the case `name` of SPECS or EXTRA -> dict (make_case's keys, the warp's, and `tanh`)"""
    if name == "chunks":            # LOOP_SPECS' (T 200, 120 albums x 2): the weighted sum's second, ragged staging round
        c = R.loop_case("chunks", R.CHUNKS_SEED)
        return add_warp(c, R.CHUNKS_SEED, 5)
    if name.startswith("zero-rows"):
        # as the model's padding: the rows behind one album's mask are ZERO (LSTM outputs past the length), and album 0 has
        # a fully masked k whose rows are all zero: e = 0 there, the cosine form meets |h'| = 0
        simi = int(name[-1])
        G, _ = R.host_plan(10, 64)
        c = R.make_case([G + 1, 2, 1], 2, 50, 10, 64, simi, True, 4242 + simi)
        c["h"][0] = c["h"][0] * c["hm"][0][..., None]
        c["tanh"] = simi in (2, 3)
        return add_warp(c, 4242 + simi, 5)
    _, counts, K, T, JQ, w, simi, tanh, masked, wt, win = next(s for s in SPECS if s[0] == name)
    G, Rr = R.host_plan(JQ, w)
    seed = sum(map(ord, name)) * 10 + simi + (5 if masked else 0)
    c = R.make_case(counts(G), K, T(Rr), JQ, w, simi, masked, seed)
    c["tanh"] = tanh
    return add_warp(c, seed, wt, win)


# ------------------------------------------------------------------ references (CPU)
def reference(c, block=None):
    """the definition, fp64 -> (h_a [NQ,w], a_logits [NQ,K,T,JQ], scale [NQ,T]); block: that many questions at a time"""
    from oracle import fvta_fused as F
    if block is not None and block < c["NQ"]:
        parts = []
        for i in range(0, c["NQ"], block):
            sub = dict(c, q=c["q"][i:i + block], album=c["album"][i:i + block], lq=c["lq"][i:i + block],
                       qm=None if c["qm"] is None else c["qm"][i:i + block], NQ=min(block, c["NQ"] - i))
            parts.append(reference(sub))
        return tuple(torch.cat([p[j] for p in parts]) for j in range(3))
    al = c["album"]
    rows = _dd(c["h"])[al]                                                   # [NQ,K,T,w]
    warped, cc = F.time_warp_closed(rows, _dd(c["lq"]), _dd(c["WH_W"]), _dd(c["WH_b"]), _dd(c["WC_W"]), _dd(c["WC_b"]),
                                    warp_type=c["warp_type"], window_t=c["window_t"])
    cnt = F.time_indication_band(c["T"], c["warp_type"], c["window_t"], dtype=torch.float64).sum(-1)
    hm = None if c["hm"] is None else c["hm"][al]
    h_a, a = F.attention_3d(warped, _dd(c["q"]), _dd(c["W"]), _dd(c["b"]), hm, c["qm"], simiMatrix=c["simi"],
                            add_tanh=c["tanh"])
    return h_a, a, cc * cnt[None, :]


energy = AR.shared(AR.energy)            # e [A,T] = sum_k sum_c v[c] h[a,k,t,c]^2, v = WH[:w] WC
factored = AR.shared(AR.factored)        # (c, dtype=torch.float64) -> (h_a, a_logits, scale) in `dtype`
