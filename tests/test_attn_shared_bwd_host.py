"""CPU-side checks of the shared-context focal attention's training calls (fvta_attn_shared_saved_bytes,
fvta_attn_shared_bwd_workspace_bytes, fvta_attn_shared_bwd_plan, fvta_attn_shared_fwd_train, fvta_attn_shared_bwd): header,
binding and library, the size queries and their refusals, the host-only plan, argument errors as status codes, and the
conditions tests/_attn_shared_bwd_ref.py puts on every pinned seed (so that the GPU test excludes nothing).  No GPU."""
import ctypes

import pytest

from tests import _attn_shared_bwd_ref as B
from tests import _attn_shared_ref as R
from tests._album_attn_host import declared_symbols, err, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_shared_saved_bytes", "fvta_attn_shared_bwd_workspace_bytes", "fvta_attn_shared_bwd_plan",
        "fvta_attn_shared_fwd_train", "fvta_attn_shared_bwd")
D = _lib.AttnSharedDesc


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert len(_lib._SIGS["fvta_attn_shared_fwd_train"][1]) == 13       # the descriptor, 11 pointers, the stream
    assert len(_lib._SIGS["fvta_attn_shared_bwd"][1]) == 16             # the descriptor, 14 pointers, the stream
    assert len(_lib._SIGS["fvta_attn_shared_fwd"][1]) == 12             # the inference call keeps its arguments
    assert lib.fvta_abi_struct_bytes(12) == ctypes.sizeof(D) == 32      # and the descriptor its 32 bytes


def test_size_queries_answer_over_the_whole_range(lib):
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for A, NQ in ((1, 1), (100, 3), (3, 100)):
                for simi in (1, 2, 3):
                    d = D(A, NQ, 2, 70, JQ, w, simi, 1)
                    assert lib.fvta_attn_shared_saved_bytes(ctypes.byref(d)) > NQ * 2 * 70 * 5, (w, JQ, A, NQ)
                    assert lib.fvta_attn_shared_bwd_workspace_bytes(ctypes.byref(d)) > NQ * 2 * 70 * 4, (w, JQ, A, NQ)


def test_no_expanded_tensor_at_the_measured_shape(lib):
    """(A, questions per album) = (8, 8), K = 6, T = 1200, JQ = 30, w = 1024: `saved` and the backward's
    workspace together stay below an eighth of one [NQ,K,T,w] tensor; so do the other measured splits of 64 questions"""
    for A, NQ in ((8, 64), (2, 64), (16, 64), (64, 64)):
        d = D(A, NQ, 6, 1200, 30, 1024, 2, 1)
        sb = lib.fvta_attn_shared_saved_bytes(ctypes.byref(d))
        wb = lib.fvta_attn_shared_bwd_workspace_bytes(ctypes.byref(d))
        assert sb > 0 and wb > 0
        assert sb + wb < NQ * 6 * 1200 * 1024 * 4 // 8, (A, NQ, sb, wb)


def test_refusals_carry_a_message(lib):
    queries = (lib.fvta_attn_shared_saved_bytes, lib.fvta_attn_shared_bwd_workspace_bytes)
    cosine = D(8, 64, 6, 1200, 30, 1024, 4, 0)
    for f in queries:
        assert f(ctypes.byref(cosine)) == 0
        assert b"per-question" in err(lib) and b"simiMatrix 4" in err(lib)
    out = (ctypes.c_int32 * 4)()
    assert lib.fvta_attn_shared_bwd_plan(ctypes.byref(cosine), out) == -3 and b"per-question" in err(lib)
    nul12, nul15 = (None,) * 12, (None,) * 15
    assert lib.fvta_attn_shared_fwd_train(ctypes.byref(cosine), *nul12) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_shared_bwd(ctypes.byref(cosine), *nul15) == -3 and b"per-question" in err(lib)
    for bad in (D(8, 64, 6, 1200, 30, 1000, 2, 0), D(8, 64, 6, 1200, 65, 1024, 2, 0), D(8, 64, 65, 1200, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(bad)) == 0 and b"unsupported" in err(lib)
        assert lib.fvta_attn_shared_bwd_plan(ctypes.byref(bad), out) == -3
    for zero in (D(0, 64, 6, 1200, 30, 1024, 2, 0), D(8, 0, 6, 1200, 30, 1024, 2, 0), D(8, 64, 6, -3, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(zero)) == 0 and b"bad A/NQ" in err(lib)
    for f in queries:
        assert f(None) == 0 and b"null descriptor" in err(lib)
    assert lib.fvta_attn_shared_bwd_plan(None, out) == -1 and b"null descriptor" in err(lib)


def test_null_pointers_are_refused(lib):
    ok = D(2, 3, 2, 10, 5, 64, 2, 0)
    assert lib.fvta_attn_shared_fwd_train(ctypes.byref(ok), *(None,) * 12) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_shared_bwd(ctypes.byref(ok), *(None,) * 15) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_shared_fwd_train(None, *(None,) * 12) == -1
    assert lib.fvta_attn_shared_bwd(None, *(None,) * 15) == -1
    assert lib.fvta_attn_shared_bwd_plan(ctypes.byref(ok), None) == -1 and b"null pointer" in err(lib)


def test_backward_plan_is_deterministic_and_host_only(lib):
    """no GPU here: the call answers all the same.  The tile and the slice depend on the width alone, the splits on the
    descriptor alone; never more splits than rows."""
    for w in (64, 128, 256, 512, 1024, 2048):
        first = None
        for T in (1, 7, 64, 65, 333, 1200):
            d = D(8, 64, 6, T, 30, w, 2, 1)
            a, b = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
            assert lib.fvta_attn_shared_bwd_plan(ctypes.byref(d), a) == 0
            assert lib.fvta_attn_shared_bwd_plan(ctypes.byref(d), b) == 0 and tuple(a) == tuple(b)
            rows, tsplit, chan, tpw = (int(v) for v in a)
            assert rows >= 1 and 1 <= tsplit <= T and chan >= 4 and w % chan == 0
            assert 1 <= tpw <= -(-T // rows)                   # tiles per workgroup: at most the tiles of an (album, k)
            first = first or (rows, chan)
            assert (rows, chan) == first
    assert B.host_bwd_plan(1, 1, 1, 64)[1] == 1
    # few tiles in all: one per workgroup; more (album, k, tile) than the row pass wants workgroups: several, and more
    # of them as the albums grow
    small = B.host_bwd_plan_words(5, 35, 2, 333, 10, 64)
    assert set(small) == {"rows", "tsplit", "channels", "tiles_per_wg"} and small["tiles_per_wg"] == 1
    grown = [B.host_bwd_plan_words(A, 35, 2, 1200, 10, 64)["tiles_per_wg"] for A in (8, 256, 1024, 4096)]
    assert grown[0] == 1 and grown[-1] > 1 and grown == sorted(grown)


def test_the_row_cases_stand_on_the_edges(lib):
    """T = Rb - 1, Rb, Rb + 1 around the row pass's tile, and one T that the question pass splits"""
    Ts, splits = {}, {}
    for name in B.CASE_IDS:
        if name.startswith("rows-"):
            counts, K, T, JQ, w, _, _, _ = B.shape_of(name)
            Ts[name] = T
            splits[name] = B.host_bwd_plan(K, T, JQ, w, A=len(counts), NQ=sum(counts))[1]
    Rb = B.host_bwd_plan(3, 64, 7, 256)[0]
    assert {Ts["rows-TRb-1"], Ts["rows-TRb"], Ts["rows-TRb+1"]} == {max(Rb - 1, 1), Rb, Rb + 1}
    assert {1, 7, 63, 64, 65, 333} <= set(Ts.values())
    assert splits["rows-T333"] > 1 and splits["rows-T1"] == 1
    assert set(B.CASE_IDS) == set(B.SEEDS)


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_pinned_seed_meets_the_reference_conditions(lib, name):
    c = B.build_case(name)
    assert B.SEEDS[name] in B.seed_candidates(name)
    ref = B.reference(c)
    jgap, tgap, sat = B.conditions(c, ref["a_logits"])
    assert jgap > B.GAP, "top-2 gap over j %.3g" % jgap
    assert tgap > B.GAP, "top-2 gap of amax over t %.3g" % tgap
    assert sat < B.SAT_FRACTION, "%.3f of the valid logits beyond |x| = %.2f" % (sat, B.SAT_X)
    if c["hm"] is not None:                                     # parity cases: every (album, k) and question partly valid
        assert bool(c["hm"].flatten(2).any(-1).all()) and bool(c["qm"].any(-1).all())
    assert tuple(ref["dh"].shape) == tuple(c["h"].shape) and tuple(ref["dq"].shape) == tuple(c["q"].shape)
    assert float(ref["dq"].abs().max()) > 0 and float(ref["dW"].abs().max()) > 0   # the logit gradient is alive


@pytest.mark.parametrize("name", [n for n in R.LOOP_IDS if n not in R.FORWARD_ONLY])
def test_loop_case_seed_is_the_first_that_qualifies_and_the_shape_its_regime(lib, name):
    """the pinned seed was not picked among the qualifying ones: every candidate before it fails the conditions; and the
    case stands in the regime it is named for, by the words of the two host-only plans"""
    for seed in B.seed_candidates(name)[:B.seed_candidates(name).index(B.SEEDS[name])]:
        c = B.build_case(name, seed=seed)
        assert not B.qualifies(c, B.reference(c)["a_logits"]), seed
    c = B.build_case(name)
    plan, bwd_plan = B.plans_of(c)
    R.loop_regime(name, c, plan, bwd_plan)


def test_the_unmodified_mix_case_keeps_its_edges(lib):
    """the per-question comparison's case: a fully masked (album, k), a single-row (album, k), a fully masked question, an
    album without a question"""
    import torch
    c = B.build_case(B.MIX_MASKED, parity=False)
    cnt = torch.bincount(c["album"], minlength=c["A"]).tolist()
    assert 0 in cnt and cnt[0] > 0
    assert not c["hm"][0, 0].any() and int(c["hm"][0, 1].sum()) == 1 and not c["qm"][-1].any()
