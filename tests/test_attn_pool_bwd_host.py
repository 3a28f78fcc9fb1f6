"""CPU-side checks of the pooled focal attention's training calls (fvta_attn_pool_saved_bytes,
fvta_attn_pool_bwd_workspace_bytes, fvta_attn_pool_bwd_plan, fvta_attn_pool_fwd_train, fvta_attn_pool_bwd): header, binding
and library, the size queries and their refusals, the host-only plan, what M = 1 shares with the shared-context calls,
the memory bound at the benchmark's shape, the Python refusals that reach no device, and the conditions
tests/_attn_pool_bwd_ref.py puts on every pinned seed (so that the GPU test excludes nothing).  No GPU."""
import ctypes

import pytest
import torch

from tests import _attn_pool_bwd_ref as B
from tests._album_attn_host import declared_symbols, err, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_pool_saved_bytes", "fvta_attn_pool_bwd_workspace_bytes", "fvta_attn_pool_bwd_plan",
        "fvta_attn_pool_fwd_train", "fvta_attn_pool_bwd")
D = _lib.AttnPoolDesc          # (P, NQ, M, K, JX, JQ, w, simi, add_tanh)
DS = _lib.AttnSharedDesc       # (A, NQ, K, T, JQ, w, simi, add_tanh)


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert len(_lib._SIGS["fvta_attn_pool_fwd_train"][1]) == 13         # the descriptor, 11 pointers, the stream
    assert len(_lib._SIGS["fvta_attn_pool_bwd"][1]) == 16               # the descriptor, 14 pointers, the stream
    assert len(_lib._SIGS["fvta_attn_pool_fwd"][1]) == 12               # the inference call keeps its arguments
    assert lib.fvta_abi_struct_bytes(14) == ctypes.sizeof(D) == 36      # and the descriptor its 36 bytes: no new struct


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_pinned_seed_meets_the_conditions_in_fp64(lib, name):
    c = B.build_case(name)
    jgap, tgap, sat = B.conditions(c, B.forward_logits(c))
    assert jgap > B.GAP and tgap > B.GAP and sat < B.SAT_FRACTION, (name, jgap, tgap, sat)
    assert B.SEEDS[name] in B.seed_candidates(name)
    B.loop_regime(name, c, *B.plans_of(c))                              # a past-one-round case reaches its loop


def test_the_adapted_condition_leaves_out_repeated_slots_only():
    c = B.build_case("heavy")
    first = B.first_slots(c)
    al = c["albums"]
    assert bool((al == 0).sum(1).max() >= 2) and not bool(first.all())   # some list names album 0 more than once ...
    for i, row in enumerate(al.tolist()):
        for m, p in enumerate(row):
            repeated = p >= 0 and p in row[:m]
            assert bool(first[i, m * c["JX"]:(m + 1) * c["JX"]].all()) != repeated
    # ... and without the adaptation such a question's two largest amax over t tie exactly
    a = B.forward_logits(c)
    v = B.valid_mask(c)
    amax = torch.where(v, a, torch.full_like(a, -float("inf"))).max(-1).values
    top = torch.topk(amax, 2, dim=-1).values
    assert float((top[..., 0] - top[..., 1]).min()) == 0.0


def test_size_queries_answer_over_the_whole_range(lib):
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for Pn, NQ, M in ((1, 1, 1), (100, 3, 4), (3, 100, 2)):
                for simi in (1, 2, 3):
                    d = D(Pn, NQ, M, 2, 70, JQ, w, simi, 1)
                    assert lib.fvta_attn_pool_saved_bytes(ctypes.byref(d)) > NQ * 2 * M * 70 * 5, (w, JQ, Pn, NQ, M)
                    assert lib.fvta_attn_pool_bwd_workspace_bytes(ctypes.byref(d)) > NQ * 2 * M * 70 * 4, (w, JQ, Pn, NQ, M)
                    out = (ctypes.c_int32 * 4)()
                    assert lib.fvta_attn_pool_bwd_plan(ctypes.byref(d), out) == 0
                    rows, tsplit, chan, tpw = (int(x) for x in out)
                    assert rows >= 1 and 1 <= tsplit <= 70 and w % chan == 0 and 1 <= tpw <= -(-70 // rows)


def test_one_slot_is_the_shared_layout(lib):
    """M = 1: the training ShWork and the backward's plan are the shared calls' for (A = P, T = JX)"""
    for Pn, NQ, K, JX, JQ, w in ((8, 64, 6, 300, 30, 512), (1, 1, 1, 1, 1, 64), (1500, 1284, 1, 3, 2, 64), (3, 200, 2, 333, 33, 2048)):
        for simi in (1, 2, 3):
            dp, ds = D(Pn, NQ, 1, K, JX, JQ, w, simi, 1), DS(Pn, NQ, K, JX, JQ, w, simi, 1)
            assert lib.fvta_attn_pool_saved_bytes(ctypes.byref(dp)) == lib.fvta_attn_shared_saved_bytes(ctypes.byref(ds)) > 0
            a, b = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
            assert lib.fvta_attn_pool_bwd_plan(ctypes.byref(dp), a) == 0
            assert lib.fvta_attn_shared_bwd_plan(ctypes.byref(ds), b) == 0
            assert tuple(a) == tuple(b)


def test_no_expanded_tensor_at_the_benchmark_shape(lib):
    """8 users x 8 questions, P = 64, M = 4, K = 6, JX = 300, JQ = 30: `saved` plus the backward's workspace stay below an
    eighth of ONE [NQ,K,M JX,w] fp32 tensor (the per-question route holds two: the gathered rows and their gradient)"""
    for w in (512, 1024):
        d = D(64, 64, 4, 6, 300, 30, w, 2, 1)
        sb = lib.fvta_attn_pool_saved_bytes(ctypes.byref(d))
        wb = lib.fvta_attn_pool_bwd_workspace_bytes(ctypes.byref(d))
        expanded = 64 * 6 * 4 * 300 * w * 4
        print("w = %d: saved %.1f MB + backward workspace %.1f MB of an expanded %.1f MB" % (w, sb / 1e6, wb / 1e6, expanded / 1e6))
        assert sb > 0 and wb > 0
        assert sb + wb < expanded // 8, (w, sb, wb, expanded)


def test_refusals_carry_a_message(lib):
    queries = (lib.fvta_attn_pool_saved_bytes, lib.fvta_attn_pool_bwd_workspace_bytes)
    out = (ctypes.c_int32 * 4)()
    cosine = D(64, 64, 4, 6, 300, 30, 1024, 4, 0)
    for f in queries:
        assert f(ctypes.byref(cosine)) == 0
        assert b"per-question" in err(lib) and b"simiMatrix 4" in err(lib)
    assert lib.fvta_attn_pool_bwd_plan(ctypes.byref(cosine), out) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_pool_fwd_train(ctypes.byref(cosine), *(None,) * 12) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_pool_bwd(ctypes.byref(cosine), *(None,) * 15) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(cosine)) > 0          # the inference call keeps the cosine form
    for bad in (D(64, 64, 4, 6, 300, 30, 1000, 2, 0), D(64, 64, 4, 6, 300, 65, 1024, 2, 0), D(64, 64, 4, 65, 300, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(bad)) == 0 and b"unsupported" in err(lib)
        assert lib.fvta_attn_pool_bwd_plan(ctypes.byref(bad), out) == -3 and b"unsupported" in err(lib)
    for zero in (D(0, 64, 4, 6, 300, 30, 1024, 2, 0), D(64, 0, 4, 6, 300, 30, 1024, 2, 0), D(64, 64, 0, 6, 300, 30, 1024, 2, 0),
                 D(64, 64, 4, 6, -3, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(zero)) == 0 and b"bad P/NQ" in err(lib)
    for f in queries:
        assert f(None) == 0 and b"null descriptor" in err(lib)
    assert lib.fvta_attn_pool_bwd_plan(None, out) == -1 and b"null descriptor" in err(lib)


def test_null_pointers_are_refused(lib):
    ok = D(2, 3, 2, 2, 10, 5, 64, 2, 0)
    assert lib.fvta_attn_pool_fwd_train(ctypes.byref(ok), *(None,) * 12) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_pool_bwd(ctypes.byref(ok), *(None,) * 15) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_pool_fwd_train(None, *(None,) * 12) == -1
    assert lib.fvta_attn_pool_bwd(None, *(None,) * 15) == -1
    assert lib.fvta_attn_pool_bwd_plan(ctypes.byref(ok), None) == -1 and b"null pointer" in err(lib)


def test_python_refusals_reach_no_device(monkeypatch):
    """the default stays forward-only; simiMatrix 4 and the time warp have no pooled backward.  With the op's constructor
    made to fail and require_gpu answered with the CPU, each refusal is raised before anything reaches the library."""
    from fvta_memexqa_amd import functional as Fn, nn, ops

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(ops.PooledFocalAttention, "__init__", boom)
    monkeypatch.setattr(ops.PooledWarpedFocalAttention, "__init__", boom)
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    Pn, K, JX, JQ, w, NQ = 3, 2, 5, 4, 64, 2
    pool, hq, lq = torch.randn(Pn, K, JX, w).requires_grad_(), torch.randn(NQ, JQ, w), torch.randn(NQ, w)
    pm, qm = torch.ones(Pn, K, JX, dtype=torch.bool), torch.ones(NQ, JQ, dtype=torch.bool)
    W, b = torch.randn(2 * w, 1), torch.zeros(1)
    good = [[0, 1], [1, 2]]
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_pooled_raw(pool, hq, good, W, b, pm, qm, simiMatrix=2)
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_pooled_raw(pool, hq, good, W, b, pm, qm, simiMatrix=2, differentiable=False)
    with pytest.raises(NotImplementedError, match="simiMatrix 4.*per-question"):
        Fn.attention_3d_pooled_raw(pool, hq, good, None, None, pm, qm, simiMatrix=4, differentiable=True)
    with pytest.raises(AssertionError, match="the library was reached"):          # differentiable=True does get that far
        Fn.attention_3d_pooled_raw(pool, hq, good, W, b, pm, qm, simiMatrix=2, differentiable=True)
    att, warp = nn.FocalAttention3D(w, simiMatrix=2), nn.TimeWarp(w, warp_type=5)
    with pytest.raises(RuntimeError, match="forward-only"):
        att.forward_pooled(pool, hq, good, pm, qm)
    with pytest.raises(NotImplementedError, match="per-question"):
        att.forward_pooled(pool, hq, good, pm, qm, time_warp=warp, lq=lq, differentiable=True)
    with pytest.raises(NotImplementedError, match="simiMatrix 4"):
        nn.FocalAttention3D(w, simiMatrix=4).forward_pooled(pool, hq, good, pm, qm, differentiable=True)
    assert "detached" in nn.AlbumPool.__doc__
