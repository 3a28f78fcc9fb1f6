"""CPU-side checks of the focal attention over per-question album lists from one album pool (fvta_attn_pool_*): header,
binding and library, descriptor size, the size query and the plan's words against fvta_attn_shared_plan's, every refusal
with its message, ops.check_album_lists and the order of validation and library calls in functional / nn / AlbumPool, the
workspace's size against an expanded context, and the two fp64 references of tests/_attn_pooled_ref.py against each other
on every shape the GPU tests use.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _attn_pooled_ref as R
from tests import _attn_shared_ref as S
from tests._album_attn_host import declared_symbols, err, header_code, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_pool_workspace_bytes", "fvta_attn_pool_plan", "fvta_attn_pool_fwd")


def _desc(P=8, NQ=64, M=4, K=6, JX=64, JQ=30, w=512, simi=2, tanh=0):
    return _lib.AttnPoolDesc(P, NQ, M, K, JX, JQ, w, simi, tanh)


def test_header_binding_and_library_export_the_symbols(lib):
    src, declared = header_code(), declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "fvta_attn_pool_desc" in src
    res, args = _lib._SIGS["fvta_attn_pool_fwd"]
    assert res is ctypes.c_int and len(args) == 12             # the descriptor, 10 pointers, the stream
    assert lib.fvta_abi_struct_bytes(14) == ctypes.sizeof(_lib.AttnPoolDesc) == 36
    assert [n for n, _ in _lib.AttnPoolDesc._fields_] == ["P", "NQ", "M", "K", "JX", "JQ", "w", "simi", "add_tanh"]


def test_plan_words(lib):
    out, ref = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    for JQ in (1, 10, 32, 33, 64):
        for w in (64, 512, 2048):
            assert lib.fvta_attn_pool_plan(ctypes.byref(_desc(JQ=JQ, w=w)), out) == 0
            assert out[0] == (8 if JQ <= 32 else 4)
            assert (out[0], out[1]) == S.host_plan(JQ, w) == R.host_plan(JQ, w)       # rows per tile: the shared call's
            assert (out[2] - 1) * out[3] < 64 <= out[2] * out[3]                      # the splits cover JX, none empty
    # at M = 1 the pooled call is the shared call on (A = P, T = JX): all four words
    for P, NQ, K, JX, JQ, w in ((1, 1, 1, 1, 1, 64), (5, 40, 2, 50, 10, 64), (120, 240, 3, 200, 5, 64), (3, 5, 6, 333, 40, 256),
                                (8, 64, 6, 1200, 30, 1024), (1500, 1284, 1, 5, 3, 64)):
        assert lib.fvta_attn_pool_plan(ctypes.byref(_desc(P, NQ, 1, K, JX, JQ, w)), out) == 0
        assert lib.fvta_attn_shared_plan(ctypes.byref(_lib.AttnSharedDesc(P, NQ, K, JX, JQ, w, 2, 0)), ref) == 0
        assert tuple(out) == tuple(ref), (P, NQ, K, JX, JQ, w)
    # the splits depend on the descriptor only
    again = (ctypes.c_int32 * 4)()
    d = _desc(120, 120, 2, 3, 200, 5, 64)
    assert lib.fvta_attn_pool_plan(ctypes.byref(d), out) == 0 and lib.fvta_attn_pool_plan(ctypes.byref(d), again) == 0
    assert tuple(out) == tuple(again) and R.host_plan_words(120, 120, 2, 3, 200, 5, 64)["tsplit"] == out[2]


def test_refusals_each_with_its_message(lib):
    out = (ctypes.c_int32 * 4)()
    for zero in (_desc(P=0), _desc(P=-1), _desc(M=0), _desc(M=-2), _desc(JX=0), _desc(JX=-5)):
        assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(zero)) == 0 and b"bad P/NQ/M/K/JX/JQ/w" in err(lib)
        assert lib.fvta_attn_pool_plan(ctypes.byref(zero), out) == -1 and b"bad P/NQ/M/K/JX/JQ/w" in err(lib)
    for bad, why in ((_desc(w=1000), b"w must be one of"), (_desc(JQ=65), b"JQ must be 1..64"), (_desc(K=65), b"K must be 1..64")):
        assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(bad)) == 0
        assert b"unsupported shape (P=" in err(lib) and why in err(lib)
        assert lib.fvta_attn_pool_plan(ctypes.byref(bad), out) == -3 and why in err(lib)
    assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(_desc(simi=5))) == 0
    assert b"similarity matrix not implemented" in err(lib)
    assert lib.fvta_attn_pool_plan(ctypes.byref(_desc(simi=0)), out) == -3 and b"similarity matrix not implemented" in err(lib)
    assert lib.fvta_attn_pool_plan(ctypes.byref(_desc()), None) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_pool_workspace_bytes(None) == 0 and b"null descriptor" in err(lib)
    # NQ M past 2^28, M JX past an int
    assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(_desc(NQ=1 << 20, M=1 << 9))) == 0 and b"NQ*M" in err(lib)
    assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(_desc(NQ=1, M=1 << 16, JX=1 << 16))) == 0 and b"M*JX" in err(lib)
    # the forward: status codes, nothing launched
    nul = [None] * 11
    assert lib.fvta_attn_pool_fwd(ctypes.byref(_desc()), *nul) == -1 and b"null pointer" in err(lib)
    assert lib.fvta_attn_pool_fwd(None, *nul) == -1
    assert lib.fvta_attn_pool_fwd(ctypes.byref(_desc(JQ=65)), *nul) == -3 and b"unsupported" in err(lib)
    # every supported width and both column regimes answer; P > NQ M and NQ M > P alike
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for P, NQ, M in ((1, 1, 1), (100, 3, 2), (3, 100, 9)):
                assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(_desc(P, NQ, M, 2, 70, JQ, w))) > 0


def test_no_expansion_sized_buffer(lib):
    """P = 8, NQ = 64, M = 4, K = 6, JX = 64, JQ = 30, w = 512: the expanded rows [NQ,K,M*JX,w] are 201 MB; the workspace
    holds Qs (4.2 MB), the partial sums (about 3.9 MB), amax (0.4 MB) and small change: about 9 MB"""
    nb = lib.fvta_attn_pool_workspace_bytes(ctypes.byref(_desc()))
    expanded = 64 * 6 * 4 * 64 * 512 * 4
    assert expanded == 201326592 and 0 < nb < expanded // 10, nb
    assert nb > 64 * 32 * 512 * 4 + 64 * 6 * 256 * 4            # at least Qs and amax
    assert nb < 12 << 20, nb


def test_check_album_lists():
    from fvta_memexqa_amd import ops
    t = torch.tensor([[3, 0, -1], [1, 1, 2]])
    out = ops.check_album_lists(t, 4, True)
    assert out.dtype == torch.int32 and out.is_contiguous() and not out.is_cuda and out.tolist() == t.tolist()
    assert ops.check_album_lists(np.array([[0, 1], [1, 0]], dtype=np.int16), 2, False).tolist() == [[0, 1], [1, 0]]
    assert ops.check_album_lists([[2, 0, 1], [1], [], (0, 3)], 4, True).tolist() == [[2, 0, 1], [1, -1, -1], [-1, -1, -1],
                                                                                   [0, 3, -1]]
    assert tuple(ops.check_album_lists(torch.zeros(5, 1, dtype=torch.int32), 1, False).shape) == (5, 1)
    for bad in (torch.tensor([[0, 4]]), torch.tensor([[0, -2]]), [[0, 1], [7]]):
        with pytest.raises(ValueError, match=r"must lie in \[-1, 4\)"):
            ops.check_album_lists(bad, 4, True)
    for unmasked in (torch.tensor([[0, -1]]), [[0, 1], [2]]):
        assert ops.check_album_lists(unmasked, 4, True).shape[1] == 2
        with pytest.raises(ValueError, match="needs both masks"):
            ops.check_album_lists(unmasked, 4, False)
    for empty in ([], [[]], [[], []], torch.zeros(0, 3, dtype=torch.int64), torch.zeros(3, 0, dtype=torch.int64),
                  np.zeros((2, 0), np.int32)):
        with pytest.raises(ValueError, match="empty|no question"):
            ops.check_album_lists(empty, 4, True)
    for shape in (torch.tensor([0, 1]), torch.tensor([[[0]]]), torch.tensor([[0.0, 1.0]])):
        with pytest.raises(ValueError):
            ops.check_album_lists(shape, 4, True)


def test_list_errors_are_raised_before_any_library_call(monkeypatch):
    """functional.attention_3d_pooled_raw, nn.FocalAttention3D.forward_pooled and nn.AlbumPool.attend validate the lists
    on the host first: with the op's constructor and forward made to fail, every error below is still the ValueError.  No
    device: require_gpu is answered with the CPU here, and nothing past the validation is reached."""
    from fvta_memexqa_amd import functional as Fn, nn, ops

    def boom(*a, **k):
        raise AssertionError("the library was reached with invalid album lists")
    monkeypatch.setattr(ops.PooledFocalAttention, "forward", boom)
    monkeypatch.setattr(ops.PooledFocalAttention, "__init__", boom)
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    P, K, JX, JQ, w, NQ = 3, 2, 5, 4, 64, 2
    pool, hq = torch.randn(P, K, JX, w), torch.randn(NQ, JQ, w)
    pm, qm = torch.ones(P, K, JX, dtype=torch.bool), torch.ones(NQ, JQ, dtype=torch.bool)
    W, b = torch.randn(2 * w, 1), torch.zeros(1)
    att = nn.FocalAttention3D(w, simiMatrix=2)
    mem = nn.AlbumPool(pool, pm)
    assert len(mem) == P and mem.pool.dtype == torch.float32 and mem.pool_mask.dtype == torch.uint8
    assert not isinstance(mem, torch.nn.Module)
    with torch.no_grad():
        for bad in ([[0, P], [1, 2]], [[0, -2], [1, 2]], [], [[], []], [[0, 1]], torch.tensor([0, 1]), [[0.5, 1.0], [1.0, 2.0]]):
            with pytest.raises(ValueError):
                Fn.attention_3d_pooled_raw(pool, hq, bad, W, b, pm, qm, simiMatrix=2)
            with pytest.raises(ValueError):
                att.forward_pooled(pool, hq, bad, pm, qm)
            with pytest.raises(ValueError):
                mem.attend(att, hq, qm, bad)
        ragged = [[0, 1], [2]]                                               # an empty slot: fine with masks, refused without
        with pytest.raises(ValueError, match="needs both masks"):
            Fn.attention_3d_pooled_raw(pool, hq, ragged, W, b, None, None, simiMatrix=2)
        with pytest.raises(ValueError, match="needs both masks"):
            att.forward_pooled(pool, hq, ragged, pm, None)
        with pytest.raises(ValueError, match="needs both masks"):
            nn.AlbumPool(pool).attend(att, hq, qm, ragged)
        with pytest.raises(ValueError, match="needs both masks"):
            mem.attend(att, hq, None, ragged)
        with pytest.raises(AssertionError, match="the library was reached"):  # valid lists do get that far
            mem.attend(att, hq, qm, ragged)
        with pytest.raises(ValueError, match="similarity matrix not implemented"):
            Fn.attention_3d_pooled_raw(pool, hq, [[0, 1], [1, 2]], W, b, pm, qm, simiMatrix=5)
    with pytest.raises(RuntimeError, match="forward-only"):                  # gradient mode on, parameters require grad
        att.forward_pooled(pool, hq, [[0, 1], [1, 2]], pm, qm)
    with pytest.raises(RuntimeError, match="forward-only"):
        Fn.attention_3d_pooled_raw(pool, hq.clone().requires_grad_(), [[0, 1], [1, 2]], W, b, pm, qm, simiMatrix=2)


def test_from_context_cuts_the_context_into_its_albums(monkeypatch):
    from fvta_memexqa_amd import nn, ops
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    N, K, M, JX, w = 3, 2, 4, 5, 8
    hall = torch.randn(N, K, M, JX, w)
    mask = torch.rand(N, K, M, JX) < 0.5
    mem, albums = nn.AlbumPool.from_context(hall, mask)
    assert len(mem) == N * M and albums.dtype == torch.int32 and albums.tolist() == torch.arange(N * M).reshape(N, M).tolist()
    c = dict(pool=mem.pool, pm=mem.pool_mask.bool(), albums=albums.long())
    h, m = R.expand(c)                                                       # laid end to end again: the context itself
    assert torch.equal(h, hall.reshape(N, K, M * JX, w)) and torch.equal(m, mask.reshape(N, K, M * JX))
    mem2, _ = nn.AlbumPool.from_context(hall)
    assert mem2.pool_mask is None and mem2.pool.is_contiguous()
    with pytest.raises(ValueError):
        nn.AlbumPool.from_context(hall[0])


def _agree(c, tanh):
    ha1, a1 = R.reference(c, tanh)
    ha2, a2 = R.grouped(c, tanh)
    assert tuple(ha1.shape) == (c["NQ"], c["w"]) and tuple(a1.shape) == (c["NQ"], c["K"], c["T"], c["JQ"])
    assert torch.allclose(ha1, ha2, rtol=0, atol=1e-9), float((ha1 - ha2).abs().max())
    live = a1 > -1e29                                            # masked logits are -1e30 in both, exactly
    assert torch.equal(live, a2 > -1e29)
    assert torch.allclose(a1[live], a2[live], rtol=0, atol=1e-9)
    assert torch.equal(a1[~live], a2[~live])
    return ha1, a1


@pytest.mark.parametrize("name,simi,tanh,masked", R.CASES, ids=R.CASE_IDS)
def test_the_two_references_agree(lib, name, simi, tanh, masked):
    _agree(R.build_case(name, simi, masked), tanh)


@pytest.mark.parametrize("name", R.LOOP_IDS)
def test_the_loop_cases_reach_their_loops_and_the_references_agree(lib, name):
    c = R.loop_case(name)
    R.loop_regime(name, c, R.host_plan_words(c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"]))
    _agree(c, c["tanh"])


def test_case_recipe_covers_the_edges(lib):
    """the masked `mix` case holds what the GPU tests rely on: references per album 0, 1, G, G+1, 2G+1, an empty slot, a
    question that lists one album twice, a fully masked (album, k), a single-row (album, k), a fully masked question; the
    open one holds no empty slot; `all-empty` a question without any album, whose h_a is exactly 0"""
    c = R.build_case("mix", 1, True)
    G, _ = R.host_plan(c["JQ"], c["w"])
    al = c["albums"]
    cnt = torch.bincount(al[al >= 0], minlength=c["P"]).tolist()
    assert sorted(cnt) == sorted([0, 1, G, G + 1, 2 * G + 1]) and cnt[0] > 0 and (c["M"], c["JX"]) == (3, 17)
    assert int((al < 0).sum()) == 1 and al.reshape(-1).tolist() != sorted(al.reshape(-1).tolist())
    assert any(len(set(r)) < len(r) for r in al.tolist() if min(r) >= 0)
    assert not c["pm"][0, 0].any() and int(c["pm"][0, 1].sum()) == 1 and not c["qm"][-1].any() and c["qm"][:-1, 0].all()
    o = R.build_case("mix", 1, False)
    assert int(o["albums"].min()) >= 0 and o["pm"] is None and o["NQ"] == c["NQ"]
    e = R.build_case("all-empty", 1, True)
    assert e["albums"][1].tolist() == [-1, -1] and bool(e["qm"][1].any())
    ha, a = R.reference(e, False)
    assert torch.equal(ha[1], torch.zeros(e["w"], dtype=torch.float64)) and bool((a[1] == R.NEG).all())
    assert float(ha[0].abs().max()) > 0 and float(ha[2].abs().max()) > 0
    s9 = R.build_case("slots9", 2, True)
    assert (s9["P"], s9["NQ"], s9["M"], s9["JX"]) == (4, 3, 9, 5)
