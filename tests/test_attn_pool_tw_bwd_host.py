"""CPU-side checks of the pooled focal attention's training calls UNDER THE TIME WARP (fvta_attn_pool_tw_saved_bytes,
fvta_attn_pool_tw_bwd_workspace_bytes, fvta_attn_pool_fwd_tw_train, fvta_attn_pool_bwd_tw): header, binding and library,
the size queries and their refusals, what M = 1 shares with the shared warped calls, the memory bound at the benchmark's
shape, the Python refusals that reach no device, the conditions tests/_attn_pool_tw_bwd_ref.py puts on every pinned seed
(so that the GPU test excludes nothing), and the factored backward the kernels compute against autograd of the
definition.  No GPU."""
import ctypes

import pytest
import torch

from tests import _attn_pool_tw_bwd_ref as TB
from tests._album_attn_host import declared_symbols, err, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_pool_tw_saved_bytes", "fvta_attn_pool_tw_bwd_workspace_bytes", "fvta_attn_pool_fwd_tw_train",
        "fvta_attn_pool_bwd_tw")
D = _lib.AttnPoolDesc          # (P, NQ, M, K, JX, JQ, w, simi, add_tanh)
DS = _lib.AttnSharedDesc       # (A, NQ, K, T, JQ, w, simi, add_tanh)
QUERIES = SYMS[:2]


def TWD(*shape, warp_type=5, window_t=3.0):
    return _lib.AttnPoolTwDesc(D(*shape), warp_type, window_t)


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
    n = lambda s: len(_lib._SIGS[s][1])
    assert n("fvta_attn_pool_fwd_tw_train") == n("fvta_attn_pool_fwd_tw") + 1 == 19      # `saved` in front of `workspace`
    assert n("fvta_attn_pool_bwd_tw") == n("fvta_attn_shared_bwd_tw") == 26              # the shared warped backward's count
    assert n("fvta_attn_pool_fwd_tw_train") == n("fvta_attn_shared_fwd_tw_train")
    assert lib.fvta_abi_struct_bytes(15) == ctypes.sizeof(_lib.AttnPoolTwDesc) == 44     # no new struct


@pytest.mark.parametrize("name", TB.CASE_IDS)
def test_pinned_seed_meets_the_conditions_in_fp64(lib, name):
    c = TB.build_case(name)
    jgap, tgap, sat = TB.conditions(c, TB.forward_logits(c))
    assert jgap > TB.GAP and tgap > TB.GAP and sat < TB.SAT_FRACTION, (name, jgap, tgap, sat)
    assert TB.SEEDS[name] in TB.seed_candidates(name) and len(TB.seed_candidates(name)) == 32
    TB.loop_regime(name, c, *TB.plans_of(c))                            # a past-one-round case reaches its loop


def test_the_case_list_holds_what_it_must():
    ids = set(TB.CASE_IDS)
    assert set(TB.SEEDS) == ids
    for need in ("mix-warp2", "single-simi1", "all-empty-simi1", "zero-rows", "many", "heavy", "tiles", "wide1024", "wide2048",
                 "slots9", "k6", "window0.5", "window3.0", "window7.0"):
        assert need in ids, need
    for M, JX in ((3, 3), (2, 1), (1, 7)):
        for wt in (1, 3, 4):
            c = TB.build_case("short-M%d-JX%d-warp%d" % (M, JX, wt))
            assert (c["M"], c["JX"], c["warp_type"]) == (M, JX, wt) and c["T"] <= 9
    c = TB.build_case("window7.0")
    assert c["window_t"] > c["T"] == 6
    c = TB.build_case("mix-simi2-masked")                               # the band crosses both slot boundaries
    assert (c["P"], c["M"], c["K"], c["JX"], c["JQ"], c["w"]) == (5, 3, 2, 17, 10, 64) and c["warp_type"] == 5
    cnt = torch.bincount(c["albums"][c["albums"] >= 0], minlength=5).tolist()
    assert 0 in cnt and bool((c["albums"] < 0).any())
    assert any(257 <= TB.build_case(n)["T"] <= 600 for n in ("rows-JX200", "rows-JX260"))
    assert TB.build_case("rows-JX260")["JX"] > 256                      # de's second block of 256 positions
    c = TB.build_case("all-empty-simi1")
    assert bool((c["albums"] < 0).all(1).any()) and bool(((c["albums"] < 0).sum(1) == 1).any())
    c = TB.build_case("zero-rows")
    assert float(c["pool"][~c["pm"]].abs().max()) == 0.0


def test_the_adapted_condition_leaves_out_repeated_slots_only():
    c = TB.build_case("heavy")                                          # warp 5
    first = TB.first_slots(c)
    al, JX = c["albums"], c["JX"]
    assert bool((al == 0).sum(1).max() >= 2) and not bool(first.all())  # some list names album 0 more than once ...
    for i, row in enumerate(al.tolist()):
        for m, p in enumerate(row):
            repeated = p >= 0 and p in row[:m]
            assert bool(first[i, m * JX:(m + 1) * JX].all()) != repeated
    # ... and under the warp two slots that name the same album still tie, exactly, wherever their counts agree
    a = TB.forward_logits(c)
    v = TB.valid_mask(c)
    amax = torch.where(v, a, torch.full_like(a, -float("inf"))).max(-1).values           # [NQ,K,T]
    cnt = TB.count(c)
    ties = 0
    for i, row in enumerate(al.tolist()):
        for m, p in enumerate(row):
            if p >= 0 and p in row[:m]:
                m0 = row.index(p)
                same = cnt[m * JX:(m + 1) * JX] == cnt[m0 * JX:(m0 + 1) * JX]
                x, y = amax[i, :, m * JX:(m + 1) * JX][:, same], amax[i, :, m0 * JX:(m0 + 1) * JX][:, same]
                assert torch.equal(x, y)
                ties += int(same.sum())
    assert ties > 0
    top = torch.topk(amax, 2, dim=-1).values                           # so without the adaptation some top-2 gap over t is 0
    assert float((top[..., 0] - top[..., 1]).min()) == 0.0


def test_size_queries_answer_over_the_whole_range(lib):
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for Pn, NQ, M in ((1, 1, 1), (100, 3, 4), (3, 100, 2)):
                for simi, wt in ((1, 5), (2, 1), (3, 3)):
                    d = TWD(Pn, NQ, M, 2, 70, JQ, w, simi, 1, warp_type=wt)
                    du = D(Pn, NQ, M, 2, 70, JQ, w, simi, 1)
                    sb, wb = lib.fvta_attn_pool_tw_saved_bytes(ctypes.byref(d)), lib.fvta_attn_pool_tw_bwd_workspace_bytes(ctypes.byref(d))
                    # the unwarped pair's, and the warp's arrays past them: scale, tanh(z), lin / ds, dx s, dbt, dz
                    assert sb >= lib.fvta_attn_pool_saved_bytes(ctypes.byref(du)) + NQ * M * 70 * 4 * (2 + 2), (w, JQ, Pn, NQ, M)
                    assert wb >= lib.fvta_attn_pool_bwd_workspace_bytes(ctypes.byref(du)) + NQ * M * 70 * 4 * (3 * 2 + 1), (w, JQ, Pn, NQ, M)


def test_one_slot_is_the_shared_layout(lib):
    """M = 1: `saved` and the backward's workspace less dctq [NQ,JP] are the shared warped calls' for (A = P, T = JX)"""
    for Pn, NQ, K, JX, JQ, w in ((8, 64, 6, 300, 30, 512), (1, 1, 1, 1, 1, 64), (1500, 1284, 1, 3, 2, 64), (3, 200, 2, 333, 33, 2048)):
        for simi in (1, 2, 3):
            dp = TWD(Pn, NQ, 1, K, JX, JQ, w, simi, 1)
            ds = _lib.AttnSharedTwDesc(DS(Pn, NQ, K, JX, JQ, w, simi, 1), 5, 3.0)
            assert lib.fvta_attn_pool_tw_saved_bytes(ctypes.byref(dp)) == lib.fvta_attn_shared_tw_saved_bytes(ctypes.byref(ds)) > 0
            extra = lib.fvta_attn_pool_tw_bwd_workspace_bytes(ctypes.byref(dp)) - lib.fvta_attn_shared_tw_bwd_workspace_bytes(ctypes.byref(ds))
            JP = 32 if JQ <= 32 else 64
            assert NQ * JP * 4 <= extra <= NQ * JP * 4 + 512, extra


def test_no_expanded_tensor_at_the_benchmark_shape(lib):
    """8 users x 8 questions, P = 64, M = 4, K = 6, JX = 300, JQ = 30: `saved` plus the backward's workspace stay below an
    eighth of ONE [NQ,K,M JX,w] fp32 tensor (the per-question route holds four: the gathered rows, their warp and both
    gradients)"""
    for w in (512, 1024):
        d = TWD(64, 64, 4, 6, 300, 30, w, 2, 1)
        sb = lib.fvta_attn_pool_tw_saved_bytes(ctypes.byref(d))
        wb = lib.fvta_attn_pool_tw_bwd_workspace_bytes(ctypes.byref(d))
        expanded = 64 * 6 * 4 * 300 * w * 4
        print("w = %d: saved %.1f MB + backward workspace %.1f MB of an expanded %.1f MB" % (w, sb / 1e6, wb / 1e6, expanded / 1e6))
        assert sb > 0 and wb > 0
        assert sb + wb < expanded // 8, (w, sb, wb, expanded)


def test_refusals_carry_a_message(lib):
    queries = [getattr(lib, s) for s in QUERIES]
    cosine = TWD(64, 64, 4, 6, 300, 30, 1024, 4, 0)
    for f in queries:
        assert f(ctypes.byref(cosine)) == 0
        assert b"per-question" in err(lib) and b"simiMatrix 4" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw_train(ctypes.byref(cosine), *(None,) * 18) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_pool_bwd_tw(ctypes.byref(cosine), *(None,) * 25) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(cosine)) > 0      # the inference call keeps the cosine form
    for bad in (TWD(64, 64, 4, 6, 300, 30, 1000, 2, 0), TWD(64, 64, 4, 6, 300, 65, 1024, 2, 0), TWD(64, 64, 4, 65, 300, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(bad)) == 0 and b"unsupported" in err(lib)
            assert b"P=64 NQ=64 M=4" in err(lib)                               # the pooled family's letters
        assert lib.fvta_attn_pool_bwd_tw(ctypes.byref(bad), *(None,) * 25) == -3 and b"unsupported" in err(lib)
    for zero in (TWD(0, 64, 4, 6, 300, 30, 1024, 2, 0), TWD(64, 0, 4, 6, 300, 30, 1024, 2, 0), TWD(64, 64, 0, 6, 300, 30, 1024, 2, 0),
                 TWD(64, 64, 4, 6, -3, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(zero)) == 0 and b"bad P/NQ" in err(lib)
    warp9 = TWD(64, 64, 4, 6, 300, 30, 1024, 2, 0, warp_type=9)
    for f in queries:
        assert f(ctypes.byref(warp9)) == 0 and b"time warping type not implemented" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw_train(ctypes.byref(warp9), *(None,) * 18) == -1
    assert b"time warping type not implemented" in err(lib) and b"attn_pool_fwd_tw_train" in err(lib)
    assert lib.fvta_attn_pool_bwd_tw(ctypes.byref(warp9), *(None,) * 25) == -1
    assert b"time warping type not implemented" in err(lib) and b"attn_pool_bwd_tw" in err(lib)
    for f in queries:
        assert f(None) == 0 and b"null descriptor" in err(lib)


def test_null_pointers_are_refused(lib):
    ok = TWD(2, 3, 2, 2, 10, 5, 64, 2, 0)
    assert lib.fvta_attn_pool_fwd_tw_train(ctypes.byref(ok), *(None,) * 18) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_pool_bwd_tw(ctypes.byref(ok), *(None,) * 25) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw_train(None, *(None,) * 18) == -1 and b"null descriptor" in err(lib)
    assert lib.fvta_attn_pool_bwd_tw(None, *(None,) * 25) == -1 and b"null descriptor" in err(lib)


def test_python_refusals_reach_no_device(monkeypatch):
    """the default stays forward-only; simiMatrix 4 has no pooled backward; forward_pooled(time_warp=, differentiable=True)
    keeps refusing and names the new method.  With the op's constructor made to fail and require_gpu answered with the CPU,
    each refusal is raised before anything reaches the library -- and differentiable=True with valid arguments does reach
    the op."""
    from fvta_memexqa_amd import autograd, functional as Fn, nn, ops

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(ops.PooledWarpedFocalAttention, "__init__", boom)
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    Pn, K, JX, JQ, w, NQ = 3, 2, 5, 4, 64, 2
    pool, hq, lq = torch.randn(Pn, K, JX, w).requires_grad_(), torch.randn(NQ, JQ, w), torch.randn(NQ, w)
    pm, qm = torch.ones(Pn, K, JX, dtype=torch.bool), torch.ones(NQ, JQ, dtype=torch.bool)
    W, b = torch.randn(2 * w, 1), torch.zeros(1)
    WH_W, WH_b, WC_W, WC_b = torch.randn(2 * w, w), torch.randn(w), torch.randn(w, 1), torch.zeros(1)
    good = [[0, 1], [1, 2]]
    warp = (WH_W, WH_b, WC_W, WC_b, pm, qm)
    with pytest.raises(RuntimeError, match="forward-only.*per-question time_warp \\+ attention_3d"):
        Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *warp, simiMatrix=2, warp_type=5)
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *warp, simiMatrix=2, warp_type=5, differentiable=False)
    with pytest.raises(NotImplementedError, match="simiMatrix 4.*per-question"):
        Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, None, None, *warp, simiMatrix=4, warp_type=5, differentiable=True)
    with pytest.raises(NotImplementedError, match="simiMatrix 4.*per-question"):
        autograd.pooled_warped_focal_attention(pool, hq, lq, None, None, None, WH_W, WH_b, WC_W, WC_b, simi=4)
    with pytest.raises(Exception, match="time warping type not implemented"):
        Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *warp, simiMatrix=2, warp_type=9, differentiable=True)
    with pytest.raises(AssertionError, match="the library was reached"):          # differentiable=True does get that far
        Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *warp, simiMatrix=2, warp_type=5, differentiable=True)
    att, tw = nn.FocalAttention3D(w, simiMatrix=2), nn.TimeWarp(w, warp_type=5)
    assert callable(getattr(att, "forward_pooled_warped"))
    with pytest.raises(AssertionError, match="the library was reached"):          # the training call reaches the op too
        att.forward_pooled_warped(pool, hq, good, lq, tw, pm, qm)
    with pytest.raises(ValueError, match="forward_pooled_warped: lq must be"):
        att.forward_pooled_warped(pool, hq, good, lq[:1], tw, pm, qm)
    with pytest.raises(NotImplementedError, match="per-question") as e:
        att.forward_pooled(pool, hq, good, pm, qm, time_warp=tw, lq=lq, differentiable=True)
    assert "forward_pooled_warped" in str(e.value)
    with pytest.raises(NotImplementedError, match="simiMatrix 4"):
        nn.FocalAttention3D(w, simiMatrix=4).forward_pooled_warped(pool, hq, good, lq, tw, pm, qm)
    assert "forward only" not in ops.PooledWarpedFocalAttention.__doc__
    assert ops.PooledWarpedFocalAttention.backward is ops.SharedWarpedFocalAttention.backward   # one copy
    assert "detached" in nn.AlbumPool.__doc__


@pytest.mark.parametrize("name", ["mix-simi1-masked", "mix-simi2-masked", "mix-simi3-open", "mix-warp2", "all-empty-simi1",
                                  "all-empty-simi3", "short-M3-JX3-warp3", "heavy"])
def test_the_factored_backward_is_the_definitions_gradient(name):
    """What the kernels compute, stated in torch fp64 without autograd (tests/_attn_pool_tw_bwd_ref.factored_backward): dz
    from ds with the count of the GLOBAL position and zero at an empty slot without reading ds there, de over an album's
    references, d_pool += 2 de v h, db as -sum damax x^2 -- against fp64 autograd of expand -> time_warp_closed ->
    attention_3d at 1e-9 (x max(1, max|ref|))."""
    c = TB.build_case(name)
    ref, fac = TB.reference(c), TB.factored_backward(c)
    for key in ("scale",) + TB.GRAD_KEYS:
        want = ref[key]
        err = float((fac[key] - want).abs().max())
        assert err <= 1e-9 * max(1.0, float(want.abs().max())), (name, key, err)
    if c["tanh"]:                                                       # db as the kernels sum it
        assert abs(float(fac["db_pooled"] - ref["db"])) <= 1e-9, (float(fac["db_pooled"]), float(ref["db"]))
    al, JX = c["albums"], c["JX"]
    for i, row in enumerate(al.tolist()):                               # zero at empty slots
        for m, p in enumerate(row):
            if p < 0:
                assert float(fac["dz"][i, m * JX:(m + 1) * JX].abs().max()) == 0.0
    listed = torch.bincount(al[al >= 0], minlength=c["P"])
    for p in range(c["P"]):                                             # an album nobody lists: no energy gradient either
        if int(listed[p]) == 0:
            assert float(fac["de"][p].abs().max()) == 0.0 and float(fac["dpool"][p].abs().max()) == 0.0
    nothing = (al < 0).all(1)
    if bool(nothing.any()):                                             # a question that lists nothing: d_hq = d_lq = 0
        assert float(fac["dq"][nothing].abs().max()) == 0.0 and float(fac["dlq"][nothing].abs().max()) == 0.0
        assert float(ref["dq"][nothing].abs().max()) == 0.0 and float(ref["dlq"][nothing].abs().max()) == 0.0


def test_a_count_taken_per_album_is_caught():
    """the bug the short cases exist for: dz with the count of the album's own j instead of m JX + j misses d_lq by far
    more than its tolerance (torch only)"""
    from tests import _attn_shared_tw_ref as TW
    c = TB.build_case("short-M3-JX3-warp3")
    ref = TB.reference(c)
    wrong = dict(c, T=c["JX"])
    local = TW._count(wrong["T"], c["warp_type"], c["window_t"], torch.float64).repeat(c["M"])
    assert not torch.equal(local, TB.count(c))
    fac = TB.factored_backward(c)
    bad_dz = fac["dz"] / TB.count(c)[None, :] * local[None, :]
    WC = c["WC_W"].double().reshape(-1)
    bad_dlq = c["K"] * bad_dz.sum(1)[:, None] * WC[None, :]
    assert not TB.within(bad_dlq, ref["dlq"], "dlq")[0]
    assert TB.within(fac["dlq"], ref["dlq"], "dlq")[0]
