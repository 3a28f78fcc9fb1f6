"""CPU-side checks of the shared-context focal attention's training calls UNDER THE TIME WARP
(fvta_attn_shared_tw_saved_bytes, fvta_attn_shared_tw_bwd_workspace_bytes, fvta_attn_shared_fwd_tw_train,
fvta_attn_shared_bwd_tw): header, binding and library; the size queries and their refusals; argument errors as status
codes (host side, no launch); the conditions every pinned seed of tests/_attn_shared_tw_bwd_ref.py meets in fp64 (so that
the GPU test excludes nothing); and the mathematics itself, independently of any kernel: the hand-written
`factored_backward` against fp64 autograd of the definition at 1e-9 on every case.  No GPU."""
import ctypes

import pytest
import torch

from tests import _attn_shared_bwd_ref as B
from tests import _attn_shared_ref as R
from tests import _attn_shared_tw_bwd_ref as TB
from tests._album_attn_host import declared_symbols, err, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_shared_tw_saved_bytes", "fvta_attn_shared_tw_bwd_workspace_bytes", "fvta_attn_shared_fwd_tw_train",
        "fvta_attn_shared_bwd_tw")
D = _lib.AttnSharedDesc
N_FWD, N_BWD = 18, 25            # arguments after the descriptor


def TD(shape, warp_type=5, window_t=3.0):
    return _lib.AttnSharedTwDesc(shape, warp_type, window_t)


_REF = {}


def _case(name):
    """the case, its fp64 autograd reference and the hand-written backward: computed once, never written to"""
    if name not in _REF:
        c = TB.build_case(name)
        _REF[name] = (c, TB.reference(c), TB.factored_backward(c, torch.float64))
    return _REF[name]


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert len(_lib._SIGS["fvta_attn_shared_fwd_tw_train"][1]) == 1 + N_FWD    # fvta_attn_shared_fwd_tw's and `saved`
    assert len(_lib._SIGS["fvta_attn_shared_fwd_tw_train"][1]) == len(_lib._SIGS["fvta_attn_shared_fwd_tw"][1]) + 1
    assert len(_lib._SIGS["fvta_attn_shared_bwd_tw"][1]) == 1 + N_BWD
    assert lib.fvta_abi_struct_bytes(13) == ctypes.sizeof(_lib.AttnSharedTwDesc) == 40   # no new struct, the same 40 bytes


def test_size_queries_answer_over_the_whole_range(lib):
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for A, NQ in ((1, 1), (100, 3), (3, 100)):
                for wt in (1, 2, 3, 4, 5):
                    d = TD(D(A, NQ, 2, 70, JQ, w, 1 + wt % 3, 1), wt)
                    plain = lib.fvta_attn_shared_saved_bytes(ctypes.byref(d.shape))
                    sb = lib.fvta_attn_shared_tw_saved_bytes(ctypes.byref(d))
                    # what the plain training forward saves, plus scale, tanh(z) [NQ,T], lin [NQ,K,T] and r2 [A,K,T]
                    assert sb >= plain + 4 * (2 * NQ * 70 + NQ * 2 * 70 + A * 2 * 70), (w, JQ, A, NQ)
                    wb = lib.fvta_attn_shared_tw_bwd_workspace_bytes(ctypes.byref(d))
                    assert wb > lib.fvta_attn_shared_bwd_workspace_bytes(ctypes.byref(d.shape)), (w, JQ, A, NQ)


def test_no_expanded_tensor_at_the_measured_shape(lib):
    """(A, questions per album) = (8, 8), K = 6, T = 1200, JQ = 30, w = 1024: `saved` and the backward's workspace
    together stay below an eighth of one [NQ,K,T,w] tensor; so do the other splits of 64 questions, (64, 1) included"""
    for A, NQ in ((8, 64), (2, 64), (16, 64), (64, 64)):
        d = TD(D(A, NQ, 6, 1200, 30, 1024, 2, 1))
        sb = lib.fvta_attn_shared_tw_saved_bytes(ctypes.byref(d))
        wb = lib.fvta_attn_shared_tw_bwd_workspace_bytes(ctypes.byref(d))
        assert sb > 0 and wb > 0
        assert sb + wb < NQ * 6 * 1200 * 1024 * 4 // 8, (A, NQ, sb, wb)


def test_refusals_carry_a_message(lib):
    queries = (lib.fvta_attn_shared_tw_saved_bytes, lib.fvta_attn_shared_tw_bwd_workspace_bytes)
    cosine = TD(D(8, 64, 6, 1200, 30, 1024, 4, 0))
    for f in queries:
        assert f(ctypes.byref(cosine)) == 0
        assert b"per-question" in err(lib) and b"simiMatrix 4" in err(lib)
    assert lib.fvta_attn_shared_fwd_tw_train(ctypes.byref(cosine), *(None,) * N_FWD) == -3 and b"per-question" in err(lib)
    assert lib.fvta_attn_shared_bwd_tw(ctypes.byref(cosine), *(None,) * N_BWD) == -3 and b"per-question" in err(lib)
    for wt in (0, 6):
        bad = TD(D(8, 64, 6, 1200, 30, 1024, 2, 1), wt)
        for f in queries:
            assert f(ctypes.byref(bad)) == 0 and b"time warping type not implemented" in err(lib)
        assert lib.fvta_attn_shared_fwd_tw_train(ctypes.byref(bad), *(None,) * N_FWD) == -1
        assert b"time warping type not implemented" in err(lib)
        assert lib.fvta_attn_shared_bwd_tw(ctypes.byref(bad), *(None,) * N_BWD) == -1
        assert b"time warping type not implemented" in err(lib)
    for shape in (D(8, 64, 6, 1200, 30, 1000, 2, 0), D(8, 64, 6, 1200, 65, 1024, 2, 0), D(8, 64, 65, 1200, 30, 1024, 2, 0)):
        for f in queries:
            assert f(ctypes.byref(TD(shape))) == 0 and b"unsupported" in err(lib)
    for f in queries:
        assert f(ctypes.byref(TD(D(8, 64, 6, 1200, 30, 1024, 2, 0), 5, -1.0))) == 0 and b"window_t" in err(lib)
        assert f(None) == 0 and b"null descriptor" in err(lib)


def test_null_pointers_are_refused(lib):
    ok = TD(D(2, 3, 2, 10, 5, 64, 2, 0))
    assert lib.fvta_attn_shared_fwd_tw_train(ctypes.byref(ok), *(None,) * N_FWD) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_shared_bwd_tw(ctypes.byref(ok), *(None,) * N_BWD) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_shared_fwd_tw_train(None, *(None,) * N_FWD) == -1
    assert lib.fvta_attn_shared_bwd_tw(None, *(None,) * N_BWD) == -1


def test_the_cases_stand_where_they_are_meant_to(lib):
    Ts, splits = {}, {}
    for name in TB.CASE_IDS:
        if name.startswith("rows-"):
            counts, K, T, JQ, w = TB.shape_of(name)[:5]
            Ts[name] = T
            splits[name] = B.host_bwd_plan(K, T, JQ, w, A=len(counts), NQ=sum(counts))[1]
    Rb = B.host_bwd_plan(3, 64, 7, 256)[0]
    assert {Ts["rows-TRb-1"], Ts["rows-TRb"], Ts["rows-TRb+1"]} == {max(Rb - 1, 1), Rb, Rb + 1}
    assert {1, 7, 63, 64, 65, 333} <= set(Ts.values())
    assert splits["rows-T333"] > 1 and splits["rows-T1"] == 1
    assert set(TB.CASE_IDS) == set(TB.SEEDS)
    assert {TB.shape_of(n)[8] for n in TB.CASE_IDS} == {1, 2, 3, 4, 5}                     # every warp type
    assert TB.cmax(7, 5, 0.5) == 3 and TB.cmax(7, 5, 3.0) == 7 and TB.cmax(5, 5, 7.0) == 15 and TB.cmax(9, 3, 2.3) == 9
    c = TB.build_case("window7.0-T5")
    assert float(TB._count(c, torch.float64).min()) == 5.0                                  # the band wider than T: all of T
    z = TB.build_case("zero-rows")
    assert float(z["h"][0][~z["hm"][0]].abs().max()) == 0.0 and float(z["h"][0, 1].abs().max()) == 0.0
    assert int(z["hm"][0, 1].sum()) == 1
    e = TB.TW.energy(z)
    assert bool((e[0] == 0).any()) and bool((e[0] != 0).any())
    assert TB.odd_width_case()["w"] == 100


@pytest.mark.parametrize("name", TB.CASE_IDS)
def test_pinned_seed_meets_the_reference_conditions(lib, name):
    c, ref, _ = _case(name)
    assert TB.SEEDS[name] in TB.seed_candidates(name, 32)
    jgap, tgap, sat = TB.conditions(c, ref["a_logits"])
    assert jgap > B.GAP, "top-2 gap over j %.3g" % jgap
    assert tgap > B.GAP, "top-2 gap of amax over t %.3g" % tgap
    assert sat < B.SAT_FRACTION, "%.3f of the valid logits beyond |x| = %.2f" % (sat, B.SAT_X)
    if c["hm"] is not None:                                     # parity cases: every (album, k) and question partly valid
        assert bool(c["hm"].flatten(2).any(-1).all()) and bool(c["qm"].any(-1).all())
    for key in TB.GRAD_KEYS:                                    # every gradient is alive: a dead one would pass any kernel
        if key == "db" and not c["tanh"]:                       # (without tanh the bias shifts every logit alike: db = 0)
            continue
        assert float(ref[key].abs().max()) > 0, key
    assert float(ref["dWH_W"][c["w"]:].abs().max()) == 0.0      # the rows of WH that see a zero feature


def test_odd_width_seed_meets_the_reference_conditions(lib):
    c = TB.odd_width_case()
    assert TB.qualifies(c, TB.reference(c, grads=False)["a_logits"])


@pytest.mark.parametrize("name", TB.CASE_IDS)
def test_factored_backward_is_the_definition_s_gradient(lib, name):
    """the formulas the kernels implement against fp64 autograd of time_warp_closed -> attention_3d on h[album]: 1e-9
    relative to the largest entry of each output"""
    c, ref, fac = _case(name)
    assert set(TB.GRAD_KEYS) <= set(fac)
    for key in ("h_a", "a_logits", "scale") + TB.GRAD_KEYS:
        want, got = ref[key], fac[key]
        assert tuple(got.shape) == tuple(want.shape), key
        if key == "a_logits":                                   # (the masked entries are -1e30 on both sides)
            v = TB.valid_mask(c)
            want, got = want[v], got[v]
        err = float((got - want).abs().max())
        assert err <= 1e-9 * max(1.0, float(want.abs().max())), (key, err, float(want.abs().max()))
    # db as the kernels sum it -- minus the sum of damax x^2 under tanh, zero without: the damax of a question sum to zero
    assert float((fac["db_pooled"] - ref["db"]).abs().max()) <= 1e-9 * max(1.0, float(ref["db"].abs().max()))


@pytest.mark.parametrize("name", ["tiles-w64", "tiles-w512", "tiles-w2048", "k17", "k64", "splits9", "heavy", "many"])
def test_loop_case_seed_is_the_first_that_qualifies_and_the_shape_its_regime(lib, name):
    for seed in TB.seed_candidates(name, 32)[:TB.seed_candidates(name, 32).index(TB.SEEDS[name])]:
        c = TB.build_case(name, seed=seed)
        assert not TB.qualifies(c, TB.reference(c, grads=False)["a_logits"]), seed
    c = TB.build_case(name)
    plan, bwd_plan = TB.plans_of(c)
    R.loop_regime(name, c, plan, bwd_plan)


def test_the_unmodified_mix_case_keeps_its_edges(lib):
    """the per-question comparison's case: a fully masked (album, k), a single-row (album, k), a fully masked question, an
    album without a question"""
    c = TB.build_case(TB.MIX_MASKED, parity=False)
    cnt = torch.bincount(c["album"], minlength=c["A"]).tolist()
    assert 0 in cnt and cnt[0] > 0
    assert not c["hm"][0, 0].any() and int(c["hm"][0, 1].sum()) == 1 and not c["qm"][-1].any()
