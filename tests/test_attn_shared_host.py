"""CPU-side checks of the shared-context focal attention (fvta_attn_shared_*): header and binding, descriptor size, the
size query and its refusals, the host-only plan, argument errors as status codes, ops.check_album_index, and the two fp64
references of tests/_attn_shared_ref.py against each other on every shape the GPU tests use, and the regime of each
LOOP_SPECS case by the plan's words.  No GPU."""
import ctypes

import pytest
import torch

from tests import _attn_shared_ref as R
from tests._album_attn_host import declared_symbols, err, header_code, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_shared_workspace_bytes", "fvta_attn_shared_plan", "fvta_attn_shared_fwd")


def test_header_and_binding_agree():
    src, declared = header_code(), declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols(), s
    assert "fvta_attn_shared_desc" in src
    res, args = _lib._SIGS["fvta_attn_shared_fwd"]
    assert res is ctypes.c_int and len(args) == 12             # the descriptor, 10 pointers, the stream


def test_descriptor_size(lib):
    assert lib.fvta_abi_struct_bytes(12) == ctypes.sizeof(_lib.AttnSharedDesc) == 32
    for s in SYMS:
        assert hasattr(lib, s)


def test_workspace_query_and_refusals(lib):
    ok = _lib.AttnSharedDesc(8, 64, 6, 1200, 30, 1024, 2, 0)
    nb = lib.fvta_attn_shared_workspace_bytes(ctypes.byref(ok))
    assert nb > 64 * 6 * 1200 * 4                               # at least the max-pooled logits
    assert nb < 8 * 64 * 6 * 1200 * 1024 * 4 // 8               # and nowhere near an expanded [NQ,K,T,w] tensor
    for bad in (_lib.AttnSharedDesc(8, 64, 6, 1200, 30, 1000, 2, 0), _lib.AttnSharedDesc(8, 64, 6, 1200, 65, 1024, 2, 0)):
        assert lib.fvta_attn_shared_workspace_bytes(ctypes.byref(bad)) == 0
        assert b"unsupported" in err(lib)
    bad5 = _lib.AttnSharedDesc(8, 64, 6, 1200, 30, 1024, 5, 0)
    assert lib.fvta_attn_shared_workspace_bytes(ctypes.byref(bad5)) == 0
    assert b"similarity matrix not implemented" in err(lib)
    for zero in (_lib.AttnSharedDesc(0, 64, 6, 1200, 30, 1024, 2, 0), _lib.AttnSharedDesc(8, 0, 6, 1200, 30, 1024, 2, 0),
                 _lib.AttnSharedDesc(8, 64, 6, -3, 30, 1024, 2, 0)):
        assert lib.fvta_attn_shared_workspace_bytes(ctypes.byref(zero)) == 0 and b"bad A/NQ" in err(lib)
    assert lib.fvta_attn_shared_workspace_bytes(None) == 0
    # every supported width and both column regimes answer; A > NQ and NQ > A alike
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for A, NQ in ((1, 1), (100, 3), (3, 100)):
                assert lib.fvta_attn_shared_workspace_bytes(ctypes.byref(_lib.AttnSharedDesc(A, NQ, 2, 70, JQ, w, 1, 0))) > 0


def test_plan_answers_on_the_host(lib):
    out = (ctypes.c_int32 * 4)()
    d30 = _lib.AttnSharedDesc(8, 64, 6, 1200, 30, 1024, 2, 0)
    assert lib.fvta_attn_shared_plan(ctypes.byref(d30), out) == 0
    G, rows, tsplit, rps = (int(v) for v in out)
    assert G >= 8 and rows >= 1 and tsplit >= 1
    assert G * 32 <= 256 or G * 30 <= 256                       # the group's columns fit the product's N side
    assert rps >= 1 and (tsplit - 1) * rps < 1200 <= tsplit * rps   # the splits of rps rows cover T, none of them empty
    d60 = _lib.AttnSharedDesc(8, 64, 6, 1200, 60, 1024, 2, 0)
    assert lib.fvta_attn_shared_plan(ctypes.byref(d60), out) == 0 and out[0] >= 4
    # the T splits depend on the descriptor only: the same answer twice, and never more splits than rows
    again = (ctypes.c_int32 * 4)()
    assert lib.fvta_attn_shared_plan(ctypes.byref(d60), again) == 0 and tuple(again) == tuple(out)
    d1 = _lib.AttnSharedDesc(1, 1, 1, 1, 1, 64, 1, 0)
    assert lib.fvta_attn_shared_plan(ctypes.byref(d1), out) == 0 and out[2] == 1 and out[3] == 1
    # the words by name, and over shapes: every split within T, the rows per split what ceil(T / splits) gives
    for A, NQ, K, T in ((1, 1, 1, 1), (5, 40, 2, 50), (120, 240, 3, 200), (3, 5, 6, 333), (8, 64, 6, 1200)):
        p = R.host_plan_words(A, NQ, K, T, 10, 64)
        assert set(p) == {"G", "rows", "tsplit", "rows_per_split"}
        assert (p["tsplit"] - 1) * p["rows_per_split"] < T <= p["tsplit"] * p["rows_per_split"], (T, p)
        assert p["rows_per_split"] == -(-T // p["tsplit"]), (T, p)
    assert lib.fvta_attn_shared_plan(ctypes.byref(d30), None) == -1 and b"null pointer" in err(lib)
    bad = _lib.AttnSharedDesc(8, 64, 6, 1200, 30, 1000, 2, 0)
    assert lib.fvta_attn_shared_plan(ctypes.byref(bad), out) == -3 and b"unsupported" in err(lib)


def test_forward_refuses_null_pointers(lib):
    ok = _lib.AttnSharedDesc(2, 3, 2, 10, 5, 64, 2, 0)
    st = lib.fvta_attn_shared_fwd(ctypes.byref(ok), None, None, None, None, None, None, None, None, None, None, None)
    assert st == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_shared_fwd(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    bad = _lib.AttnSharedDesc(2, 3, 2, 10, 65, 64, 2, 0)
    st = lib.fvta_attn_shared_fwd(ctypes.byref(bad), None, None, None, None, None, None, None, None, None, None, None)
    assert st == -3 and b"unsupported" in err(lib)


def test_check_album_index():
    from fvta_memexqa_amd import ops
    idx = torch.tensor([3, 0, 3, 1, 2, 2, 0, 3])
    out = ops.check_album_index(idx, 4)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.tolist() == idx.tolist()
    assert ops.check_album_index(torch.tensor([0, 0], dtype=torch.int32), 1).tolist() == [0, 0]
    assert ops.check_album_index([1, 0], 2).tolist() == [1, 0]
    for bad in (torch.tensor([0, -1]), torch.tensor([0, 4]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            ops.check_album_index(bad, 4)


@pytest.mark.parametrize("name,simi,tanh,masked", R.CASES, ids=R.CASE_IDS)
def test_the_two_references_agree(lib, name, simi, tanh, masked):
    c = R.build_case(name, simi, masked)
    ha1, a1 = R.reference(c, tanh)
    ha2, a2 = R.grouped(c, tanh)
    assert tuple(ha1.shape) == (c["NQ"], c["w"]) and tuple(a1.shape) == (c["NQ"], c["K"], c["T"], c["JQ"])
    assert torch.allclose(ha1, ha2, rtol=0, atol=1e-10), float((ha1 - ha2).abs().max())
    live = a1 > -1e29                                            # masked logits are -1e30 in both, exactly
    assert torch.equal(live, a2 > -1e29)
    assert torch.allclose(a1[live], a2[live], rtol=0, atol=1e-10)
    assert torch.equal(a1[~live], a2[~live])


def _loop_case(name):
    from tests import _attn_shared_bwd_ref as B
    return R.loop_case(name, R.CHUNKS_SEED) if name in R.FORWARD_ONLY else B.build_case(name)


@pytest.mark.parametrize("name", R.LOOP_IDS)
def test_the_loop_cases_reach_their_loops_and_the_references_agree(lib, name):
    """every case of LOOP_SPECS stands in the regime it is named for, by the plan's own words; the blocked evaluation of
    the definition is the unblocked one, and the album-by-album restatement agrees with it"""
    from tests import _attn_shared_bwd_ref as B
    c = _loop_case(name)
    plan, bwd_plan = B.plans_of(c)
    R.loop_regime(name, c, plan, None if name in R.FORWARD_ONLY else bwd_plan)
    assert (name in B.CASE_IDS) == (name not in R.FORWARD_ONLY)
    ha1, a1 = R.reference(c, c["tanh"], block=100)
    ha2, a2 = R.grouped(c, c["tanh"])
    assert tuple(ha1.shape) == (c["NQ"], c["w"]) and tuple(a1.shape) == (c["NQ"], c["K"], c["T"], c["JQ"])
    assert torch.allclose(ha1, ha2, rtol=0, atol=1e-10), float((ha1 - ha2).abs().max())
    live = a1 > -1e29
    assert torch.equal(live, a2 > -1e29) and torch.allclose(a1[live], a2[live], rtol=0, atol=1e-10)
    if c["NQ"] <= 300:
        ha0, a0 = R.reference(c, c["tanh"])
        assert torch.allclose(ha0, ha1, rtol=0, atol=1e-12) and torch.allclose(a0, a1, rtol=0, atol=1e-12)


def test_case_recipe_covers_the_edges(lib):
    """the masked `mix` case holds what the GPU tests rely on: a fully masked (album, k), a single-row (album, k), a fully
    masked question, an album without a question, group sizes 1, G, G+1, 2G+1, a shuffled index"""
    c = R.build_case("mix", 1, True)
    G, _ = R.host_plan(c["JQ"], c["w"])
    cnt = torch.bincount(c["album"], minlength=c["A"]).tolist()
    assert sorted(cnt) == sorted([0, 1, G, G + 1, 2 * G + 1]) and cnt[0] > 0
    assert c["album"].tolist() != sorted(c["album"].tolist())
    assert not c["hm"][0, 0].any() and int(c["hm"][0, 1].sum()) == 1 and not c["qm"][-1].any() and c["qm"][:-1, 0].all()


def test_end_to_end_seed_keeps_every_answer_clear():
    """the tiny end-to-end graph's seed: every question's top two probabilities differ by more than the margin in fp64, so
    the GPU test's argmax comparison excludes nothing"""
    c = R.e2e_case()
    logits, yp = R.e2e_reference(c)
    assert tuple(yp.shape) == (c["NQ"], c["C"])
    assert bool((R.top2_margin(yp) > c["margin"]).all()), R.top2_margin(yp)
    assert len(set(c["album"].tolist())) == c["A"]
