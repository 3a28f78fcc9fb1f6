"""CPU-side checks of the pooled focal attention under the time warp (fvta_attn_pool_tw_workspace_bytes /
fvta_attn_pool_energy / fvta_attn_pool_fwd_tw), on every shape tests/test_gpu_attn_pooled_tw.py runs: header, binding and
library, the descriptor, the size query, every refusal with its message; the factorisation the kernels compute
(tests/_attn_pooled_tw_ref.factored: the energy per pooled album, the scale per (question, global position)) IS the
definition (expand, time_warp_closed, attention_3d) in fp64, and evaluated in fp32 it stays inside the GPU tolerances (a
shape that does not is ill conditioned: then the shape changes, never the tolerance); the scales come in both signs; the
count runs over the question's whole M JX positions; and the Python surface's host-side errors come before any library
call.  No GPU."""
import ctypes

import pytest
import torch

from tests import _attn_pooled_ref as R
from tests import _attn_pooled_tw_ref as PT
from tests._album_attn_host import declared_symbols, err, header_code, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_pool_tw_workspace_bytes", "fvta_attn_pool_energy", "fvta_attn_pool_fwd_tw")
_REF = {}


def _case(name):
    if name not in _REF:
        c = PT.build_case(name)
        _REF[name] = (c, PT.reference(c))
    return _REF[name]


def _desc(P=8, NQ=64, M=4, K=6, JX=64, JQ=30, w=512, simi=2, tanh=0, warp_type=5, window_t=3.0):
    return _lib.AttnPoolTwDesc(_lib.AttnPoolDesc(P, NQ, M, K, JX, JQ, w, simi, tanh), warp_type, window_t)


# ------------------------------------------------------------------ the C ABI, host side
def test_header_binding_and_library_export_the_symbols(lib):
    src, declared = header_code(), declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "fvta_attn_pool_tw_desc" in src                      # the fourth new symbol: the descriptor
    res, args = _lib._SIGS["fvta_attn_pool_fwd_tw"]
    assert res is ctypes.c_int and len(args) == 18              # the descriptor, 16 pointers, the stream
    res, args = _lib._SIGS["fvta_attn_pool_energy"]
    assert res is ctypes.c_int and len(args) == 7
    assert lib.fvta_abi_struct_bytes(15) == ctypes.sizeof(_lib.AttnPoolTwDesc) == 44
    assert [n for n, _ in _lib.AttnPoolTwDesc._fields_] == ["shape", "warp_type", "window_t"]
    assert lib.fvta_abi_struct_bytes(16) == -1 and lib.fvta_abi_struct_bytes(8) == -1


def test_workspace_query_answers_over_the_range(lib):
    d = _desc()
    nb = lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(d))
    base = lib.fvta_attn_pool_workspace_bytes(ctypes.byref(d.shape))
    # the pooled call's, scale [NQ, M JX], v [w]
    assert base > 0 and nb >= base + 4 * (d.shape.NQ * d.shape.M * d.shape.JX + d.shape.w)
    assert nb < base + 4 * (d.shape.NQ * d.shape.M * d.shape.JX + d.shape.w) + 1024
    for w in (64, 128, 256, 512, 1024, 2048):
        for JQ in (1, 32, 33, 64):
            for P, NQ, M in ((1, 1, 1), (100, 3, 2), (3, 100, 9)):
                for wt in (1, 2, 3, 4, 5):
                    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(P, NQ, M, 2, 70, JQ, w, warp_type=wt))) > 0
    for K in (9, 64):                                           # the attention's K limit, not the per-question warp's 8
        assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(K=K))) > 0
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(window_t=0.0))) > 0
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(M=65535, JX=256, NQ=1, P=1))) > 0     # the limit itself


def test_no_expansion_sized_buffer(lib):
    """P = 8, NQ = 64, M = 4, K = 6, JX = 300, w = 512: the expanded rows [NQ,K,M*JX,w] are 944 MB and the per-question
    route holds them twice (gathered and warped); the workspace holds Qs (4.2 MB), the partial sums (40 groups x K x 5
    splits x G 8 x w: 19.7 MB), amax (1.8 MB), the scale (0.3 MB) and small change: about 26 MB"""
    nb = lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(JX=300)))
    expanded = 64 * 6 * 4 * 300 * 512 * 4
    assert expanded == 943718400 and 0 < nb < expanded // 10, nb
    assert nb > 64 * 32 * 512 * 4 + 64 * 6 * 1200 * 4 + 64 * 1200 * 4          # at least Qs, amax and the scale
    assert nb < 32 << 20, nb


@pytest.mark.parametrize("warp_type", [0, 6, -1])
def test_bad_warp_type_fails_like_the_reference(lib, warp_type):
    d = _desc(warp_type=warp_type)
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(d)) == 0
    assert b"time warping type not implemented" in err(lib)
    assert lib.fvta_attn_pool_energy(ctypes.byref(d), *([None] * 6)) == -1
    assert b"time warping type not implemented" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw(ctypes.byref(d), *([None] * 17)) == -1
    assert b"time warping type not implemented" in err(lib) and b"attn_pool_fwd_tw" in err(lib)


def test_refusals_each_with_its_message(lib):
    nul = [None] * 17
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(window_t=-1.0))) == 0 and b"bad window_t" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw(ctypes.byref(_desc(window_t=-0.5)), *nul) == -1 and b"bad window_t" in err(lib)
    # M JX past the scale kernel's grid (still within an int: the pooled call itself takes it)
    big = _desc(P=1, NQ=1, M=65535, JX=257)
    assert lib.fvta_attn_pool_workspace_bytes(ctypes.byref(big.shape)) > 0
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(big)) == 0
    assert b"M*JX must not exceed 65535 * 256" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw(ctypes.byref(big), *nul) == -3 and b"65535 * 256" in err(lib)
    assert lib.fvta_attn_pool_energy(ctypes.byref(big), *([None] * 6)) == -3
    for bad, why in ((_desc(w=100), b"w must be one of"), (_desc(w=1000), b"w must be one of"), (_desc(JQ=65), b"JQ must be 1..64"),
                     (_desc(K=65), b"K must be 1..64")):
        assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(bad)) == 0
        assert b"unsupported shape (P=" in err(lib) and why in err(lib)
        assert lib.fvta_attn_pool_fwd_tw(ctypes.byref(bad), *nul) == -3 and why in err(lib)
        assert lib.fvta_attn_pool_energy(ctypes.byref(bad), *([None] * 6)) == -3 and why in err(lib)
    for zero in (_desc(P=0), _desc(M=0), _desc(JX=-5)):
        assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(zero)) == 0 and b"bad P/NQ/M/K/JX/JQ/w" in err(lib)
    assert lib.fvta_attn_pool_tw_workspace_bytes(ctypes.byref(_desc(simi=5))) == 0
    assert b"similarity matrix not implemented" in err(lib)
    assert lib.fvta_attn_pool_tw_workspace_bytes(None) == 0 and b"null descriptor" in err(lib)
    # null required pointers come back as status, nothing launched
    assert lib.fvta_attn_pool_energy(ctypes.byref(_desc()), *([None] * 6)) == -1 and b"attn_pool_energy: null pointer" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw(ctypes.byref(_desc()), *nul) == -1 and b"attn_pool_fwd_tw: null pointer" in err(lib)
    assert lib.fvta_attn_pool_fwd_tw(None, *nul) == -1 and b"null descriptor" in err(lib)
    assert lib.fvta_attn_pool_energy(None, *([None] * 6)) == -1


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", PT.ALL)
def test_factored_is_the_definition_in_fp64(lib, name):
    c, (ref_ha, ref_a, ref_s) = _case(name)
    assert tuple(ref_ha.shape) == (c["NQ"], c["w"]) and tuple(ref_a.shape) == (c["NQ"], c["K"], c["T"], c["JQ"])
    assert tuple(ref_s.shape) == (c["NQ"], c["T"])
    ha, a, s = PT.factored(c, torch.float64)
    for got, want, what in ((ha, ref_ha, "h_a"), (a, ref_a, "a_logits"), (s, ref_s, "scale")):
        assert torch.isfinite(got).all(), what
        err = float((got - want).abs().max())
        assert err <= 1e-9 * max(1.0, float(want[want > -1e29].abs().max()) if bool((want > -1e29).any()) else 1.0), (what, err)
    assert torch.equal(a <= -1e29, ref_a <= -1e29)                              # the same entries are masked


@pytest.mark.parametrize("name", PT.ALL)
def test_factored_in_fp32_stays_inside_the_gpu_tolerances(lib, name):
    c, (ref_ha, ref_a, ref_s) = _case(name)
    ha, a, s = PT.factored(c, torch.float32)
    for got, want, what in ((ha, ref_ha, "h_a"), (a, ref_a, "a_logits"), (s, ref_s, "scale")):
        ok, ratio = PT.within(got, want, what)
        print("%s %s: worst |err| / (atol + rtol |ref|) = %.3f" % (name, what, ratio))
        assert ok, (what, ratio)


@pytest.mark.parametrize("name", PT.LOOP_NAMES)
def test_the_loop_cases_reach_their_loops(lib, name):
    c, _ = _case(name)
    assert c["warp_type"] == 5
    R.loop_regime(name, c, R.host_plan_words(c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"]))


def test_case_recipe_covers_the_edges(lib):
    c, (ha, a, s) = _case("mix-simi1-masked")
    G, _ = R.host_plan(c["JQ"], c["w"])
    al = c["albums"]
    cnt = torch.bincount(al[al >= 0], minlength=c["P"]).tolist()
    assert sorted(cnt) == sorted([0, 1, G, G + 1, 2 * G + 1]) and (c["M"], c["JX"], c["K"], c["JQ"], c["w"]) == (3, 17, 2, 10, 64)
    assert int((al < 0).sum()) == 1
    # warp 5, window 2.3 -> half-width 3: full bands of 7 across the slot boundaries at 17 and 34, shorter at the ends only
    band = PT.TW._count(51, 5, 2.3, torch.float64)
    assert band[14:20].tolist() == [7.0] * 6 and band[0] == 4 and band[50] == 4 and int((band < 7).sum()) == 6
    o, _ = _case("mix-simi1-open")
    assert int(o["albums"].min()) >= 0 and o["pm"] is None
    assert _case("mix-warp2")[0]["warp_type"] == 2
    for nm, MJX in (("short-M3-JX3-warp3-simi1", 9), ("short-M2-JX1-warp4-simi2", 2), ("short-M1-JX7-warp1-simi4", 7)):
        cc = _case(nm)[0]
        assert cc["M"] * cc["JX"] == MJX <= 9 and cc["pm"] is not None
    for nm in PT.NAMES:
        if PT.SPECS[nm][9] in (1, 3, 4):
            assert nm.startswith("short-"), nm
    assert [_case("rows%d" % i)[0]["JX"] for i in range(6)] == [1, 7, 63, 64, 65, 200] and _case("rows0")[0]["M"] == 2
    assert [(_case(n)[0]["M"], _case(n)[0]["JX"], _case(n)[0]["window_t"]) for n in ("window0.5", "window3.0", "window7.0")] == \
        [(2, 3, 0.5), (2, 3, 3.0), (2, 3, 7.0)]
    assert (_case("slots9")[0]["M"], _case("slots9")[0]["JX"]) == (9, 5) and _case("k9")[0]["K"] == 9
    assert _case("wide2048-simi3")[0]["w"] == 2048 and _case("wide1024")[0]["w"] == 1024
    # all-empty: question 1 lists nothing: h_a exactly 0, every logit masked, its scale tanh(K (s0 + WC.lq)) cnt(t)
    e, (eha, ea, es) = _case("all-empty-simi1")
    assert e["albums"][1].tolist() == [-1, -1] and e["albums"][2].tolist() == [1, -1] and not e["qm"][2].any()
    assert torch.equal(eha[1], torch.zeros(e["w"], dtype=torch.float64)) and bool((ea[1] == PT.NEG).all())
    assert float(eha[0].abs().max()) > 0 and float(eha[2].abs().max()) > 0       # the last: uniform over its non-empty rows
    per_cnt = es[1] / PT.TW._count(e["T"], 5, e["window_t"], torch.float64)
    assert float((per_cnt - per_cnt[0]).abs().max()) < 1e-12 and float(per_cnt[0].abs()) > 0
    for nm in ("zero-rows-simi2", "zero-rows-simi4"):
        z, (zha, za, zs) = _case(nm)
        assert not bool(z["pm"][0, 0].any()) and float(z["pool"][0, 0].abs().max()) == 0.0
        assert float(z["pool"][~z["pm"]].abs().max()) == 0.0 and int((z["albums"] < 0).sum()) == 1
        assert torch.isfinite(zha).all() and torch.isfinite(zs).all()


def test_scales_come_in_both_signs(lib):
    """the sign flip of the cosine form, and of s against s^2 in the bilinear form, is exercised"""
    neg = tot = 0
    for name in [n for n in PT.NAMES if n.startswith("mix-")]:
        s = _case(name)[1][2]
        print("%s: share of negative scales %.3f" % (name, float((s < 0).double().mean())))
        assert bool((s != 0).all()) and bool((s < 0).any()) and bool((s > 0).any()), name    # every mix case: both signs
        neg += int((s < 0).sum())
        tot += s.numel()
    # (the sign is mostly the question's, K (s0 + WC.lq): a dozen questions a case, so the share is held over all of them)
    assert 0.2 <= neg / tot <= 0.8, neg / tot


def test_energy_is_per_pooled_album(lib):
    """what the factorisation rests on: the energy of an expanded question is its albums' energies end to end"""
    c, _ = _case("mix-simi2-masked")
    e = PT.energy(c)
    assert e.shape == (c["P"], c["JX"])
    h, _ = R.expand(c)
    v = c["WH_W"].double()[:c["w"]] @ c["WC_W"].double().reshape(-1)
    full = ((h.double() ** 2) @ v).sum(1)                                       # [NQ, M JX]
    for i, row in enumerate(c["albums"].tolist()):
        want = torch.cat([e[p] if p >= 0 else torch.zeros(c["JX"], dtype=torch.float64) for p in row])
        assert torch.allclose(full[i], want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("warp_type,moves", [(2, False), (3, True), (4, True)])
def test_permuting_a_list_moves_the_scale_through_the_count(lib, warp_type, moves):
    """the count belongs to the global position m JX + j: with a list's slots permuted, a block of the scale moves with its
    album and -- past, future -- is counted anew; under the diagonal (count 1) it only moves"""
    c = PT.TW.add_warp(R.make_case(torch.tensor([[0, 1, 2], [2, 2, 1]]), 3, 2, 3, 4, 64, 2, True, 77), 77, warp_type)
    c["tanh"] = True
    s = PT.scale_of(c)
    perm = [2, 0, 1]
    cp = dict(c, albums=c["albums"][:, perm])
    sp = PT.scale_of(cp)
    assert torch.allclose(sp, PT.reference(cp)[2], rtol=0, atol=1e-12)
    JX = c["JX"]
    moved = torch.cat([s[:, m * JX:(m + 1) * JX] for m in perm], 1)             # the blocks carried along with their albums
    if moves:
        assert float((sp - moved).abs().max()) > 1e-3
        cnt = PT.TW._count(3 * JX, warp_type, c["window_t"], torch.float64)
        back = torch.cat([(s / cnt)[:, m * JX:(m + 1) * JX] for m in perm], 1) * cnt
        assert torch.allclose(sp, back, rtol=0, atol=1e-12)                     # tanh(z) moves, the count stays with t
    else:
        assert torch.allclose(sp, moved, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ the Python surface, host side
def test_host_errors_are_raised_before_any_library_call(monkeypatch):
    """functional.attention_3d_pooled_warped_raw, nn.FocalAttention3D.forward_pooled(time_warp=) and nn.AlbumPool.attend
    (time_warp=) validate on the host first: with the ops' constructors and calls made to fail, every error below is still
    the ValueError.  No device: require_gpu is answered with the CPU here."""
    from fvta_memexqa_amd import functional as Fn, nn, ops

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    for cls in (ops.PooledWarpedFocalAttention, ops.PooledFocalAttention, ops.SharedWarpedFocalAttention):
        monkeypatch.setattr(cls, "__init__", boom)
        monkeypatch.setattr(cls, "forward", boom)
    monkeypatch.setattr(ops.PooledWarpedFocalAttention, "album_energy", boom)
    monkeypatch.setattr(ops.SharedWarpedFocalAttention, "album_energy", boom)
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    P, K, JX, JQ, w, NQ = 3, 2, 5, 4, 64, 2
    pool, hq, lq = torch.randn(P, K, JX, w), torch.randn(NQ, JQ, w), torch.randn(NQ, w)
    pm, qm = torch.ones(P, K, JX, dtype=torch.bool), torch.ones(NQ, JQ, dtype=torch.bool)
    W, b = torch.randn(2 * w, 1), torch.zeros(1)
    tw = (torch.zeros(2 * w, w), torch.zeros(w), torch.zeros(w, 1), torch.zeros(1))
    att, warp = nn.FocalAttention3D(w, simiMatrix=2), nn.TimeWarp(w, warp_type=5)
    mem = nn.AlbumPool(pool, pm)
    good = [[0, 1], [1, 2]]
    with torch.no_grad():
        for bad in ([[0, P], [1, 2]], [[0, -2], [1, 2]], [], [[], []], [[0, 1]], torch.tensor([0, 1]), [[0.5, 1.0], [1.0, 2.0]]):
            with pytest.raises(ValueError):
                Fn.attention_3d_pooled_warped_raw(pool, hq, bad, lq, W, b, *tw, pool_mask=pm, hq_mask=qm, simiMatrix=2, warp_type=5)
            with pytest.raises(ValueError):
                att.forward_pooled(pool, hq, bad, pm, qm, time_warp=warp, lq=lq)
            with pytest.raises(ValueError):
                mem.attend(att, hq, qm, bad, time_warp=warp, lq=lq)
        ragged = [[0, 1], [2]]                                               # an empty slot: refused without both masks
        with pytest.raises(ValueError, match="needs both masks"):
            Fn.attention_3d_pooled_warped_raw(pool, hq, ragged, lq, W, b, *tw, simiMatrix=2, warp_type=5)
        with pytest.raises(ValueError, match="needs both masks"):
            att.forward_pooled(pool, hq, ragged, pm, None, time_warp=warp, lq=lq)
        with pytest.raises(ValueError, match="needs both masks"):
            mem.attend(att, hq, None, ragged, time_warp=warp, lq=lq)
        # lq: its shape, and lq / energy without a time warp, a time warp without lq
        with pytest.raises(ValueError, match="lq"):
            Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq[:1], W, b, *tw, pool_mask=pm, hq_mask=qm, simiMatrix=2, warp_type=5)
        with pytest.raises(ValueError, match="lq"):
            Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq[:, :32], W, b, *tw, simiMatrix=2, warp_type=5)
        with pytest.raises(ValueError, match="lq must be"):
            att.forward_pooled(pool, hq, good, pm, qm, time_warp=warp, lq=lq[:1])
        with pytest.raises(ValueError, match="lq must be"):
            mem.attend(att, hq, qm, good, time_warp=warp, lq=lq[:1])
        with pytest.raises(ValueError, match="belong to the time warp"):
            att.forward_pooled(pool, hq, good, pm, qm, lq=lq)
        with pytest.raises(ValueError, match="belong to the time warp"):
            att.forward_pooled(pool, hq, good, pm, qm, energy=torch.zeros(P, JX))
        with pytest.raises(ValueError, match="needs lq"):
            att.forward_pooled(pool, hq, good, pm, qm, time_warp=warp)
        with pytest.raises(ValueError, match="belongs to the time warp"):
            mem.attend(att, hq, qm, good, lq=lq)
        with pytest.raises(ValueError, match="needs lq"):
            mem.attend(att, hq, qm, good, time_warp=warp)
        with pytest.raises(ValueError, match="energy"):
            Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *tw, simiMatrix=2, warp_type=5, energy=torch.zeros(P, JX + 1))
        with pytest.raises(Exception, match="time warping type not implemented"):
            Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *tw, simiMatrix=2, warp_type=7)
        with pytest.raises(ValueError, match="similarity matrix not implemented"):
            Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq, W, b, *tw, simiMatrix=5, warp_type=5)
        with pytest.raises(AssertionError, match="the library was reached"):  # valid arguments do get that far
            Fn.attention_3d_pooled_warped_raw(pool, hq, ragged, lq, W, b, *tw, pool_mask=pm, hq_mask=qm, simiMatrix=2, warp_type=5)
        with pytest.raises(AssertionError, match="the library was reached"):  # (the energy first)
            mem.attend(att, hq, qm, ragged, time_warp=warp, lq=lq)
    # forward-only: gradient mode on and an argument that requires grad; the message names the per-question route
    with pytest.raises(RuntimeError, match="forward-only.*per-question time_warp \\+ attention_3d"):
        Fn.attention_3d_pooled_warped_raw(pool, hq, good, lq.clone().requires_grad_(), W, b, *tw, simiMatrix=2, warp_type=5)
    with pytest.raises(RuntimeError, match="forward-only"):
        att.forward_pooled(pool, hq, good, pm, qm, time_warp=warp, lq=lq)


def test_the_energy_key_is_shared_by_both_holders():
    """AlbumMemory.energy's key -- (id, data_ptr, version) of WH/W and WC/W -- in ONE place, used by AlbumPool too"""
    from fvta_memexqa_amd import nn
    src = open(nn.__file__).read()
    assert src.count("t._version) for t in (WH, WC)") == 1
    assert hasattr(nn.AlbumPool, "energy") and hasattr(nn.AlbumMemory, "energy")
    doc = __import__("fvta_memexqa_amd.functional", fromlist=["album_energy"]).album_energy.__doc__
    assert "[P,K,JX,w]" in doc and "[P,JX]" in doc
