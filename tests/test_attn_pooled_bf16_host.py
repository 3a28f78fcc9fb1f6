"""CPU-side checks of the album pool held in bf16 (fvta_attn_pool_fwd_bf16 / fvta_attn_pool_energy_bf16 /
fvta_attn_pool_fwd_tw_bf16): header, binding and library agree on the three names and add no descriptor; every refusal
through the new entries is a status code under the entry's own name, before anything is launched; nn.AlbumPool's dtype
argument and nbytes; and functional.attention_3d_pooled_raw raises what it raises for an fp32 pool, in the same order.
No GPU."""
import ctypes
import re

import pytest
import torch

from tests._album_attn_host import HEADER, declared_symbols, err, header_code, lib  # noqa: F401
from fvta_memexqa_amd import _lib

SYMS = ("fvta_attn_pool_fwd_bf16", "fvta_attn_pool_energy_bf16", "fvta_attn_pool_fwd_tw_bf16")


def _desc(P=8, NQ=64, M=4, K=6, JX=64, JQ=30, w=512, simi=2, tanh=0):
    return _lib.AttnPoolDesc(P, NQ, M, K, JX, JQ, w, simi, tanh)


def _tw(warp_type=5, window_t=3.0, **kw):
    return _lib.AttnPoolTwDesc(_desc(**kw), warp_type, window_t)


def test_header_binding_and_library_agree_on_the_three_names(lib):
    code, declared = header_code(), declared_symbols()
    for s in SYMS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(lib, s), s
        fp32 = s[:-len("_bf16")]
        assert _lib._SIGS[s] == _lib._SIGS[fp32], s                # the descriptor and argument order of the namesake
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % s, code, re.S).group(1)
        assert "const uint16_t* pool" in proto and "const float* pool" not in proto
    # no new descriptor: the two pooled ones, at their sizes, and nothing after them
    assert lib.fvta_abi_struct_bytes(14) == ctypes.sizeof(_lib.AttnPoolDesc) == 36
    assert lib.fvta_abi_struct_bytes(15) == ctypes.sizeof(_lib.AttnPoolTwDesc) == 44
    assert lib.fvta_abi_struct_bytes(16) == -1
    # the header states the contract, the alignment and what is not there
    doc = " ".join(open(HEADER).read().split())
    for words in ("BIT FOR BIT", "8-byte aligned", "Not here: training"):
        assert words in doc, words


def test_refusals_carry_the_entry_s_own_name_and_launch_nothing(lib):
    nul11, nul17 = [None] * 11, [None] * 17
    fwd, energy, fwd_tw = lib.fvta_attn_pool_fwd_bf16, lib.fvta_attn_pool_energy_bf16, lib.fvta_attn_pool_fwd_tw_bf16
    # a null pool (everything null): FVTA_ERR_INVALID_ARG
    assert fwd(ctypes.byref(_desc()), *nul11) == -1 and err(lib) == b"attn_pool_fwd_bf16: null pointer"
    assert fwd_tw(ctypes.byref(_tw()), *nul17) == -1 and err(lib) == b"attn_pool_fwd_tw_bf16: null pointer"
    assert energy(ctypes.byref(_tw()), *([None] * 6)) == -1 and err(lib) == b"attn_pool_energy_bf16: null pointer"
    assert fwd(None, *nul11) == -1 and b"attn_pool_fwd_bf16: null descriptor" in err(lib)
    # simiMatrix 5, w = 1000: FVTA_ERR_UNSUPPORTED, the fp32 entries' words under the new names
    for call, d, nul, who in ((fwd, _desc, nul11, b"attn_pool_fwd_bf16"), (fwd_tw, _tw, nul17, b"attn_pool_fwd_tw_bf16"),
                              (energy, _tw, [None] * 6, b"attn_pool_energy_bf16")):
        assert call(ctypes.byref(d(simi=5)), *nul) == -3
        assert err(lib) == who + b": similarity matrix not implemented (simiMatrix=5)"
        assert call(ctypes.byref(d(w=1000)), *nul) == -3
        assert err(lib).startswith(who + b": unsupported shape (P=8 NQ=64 M=4 K=6 JX=64 JQ=30 w=1000)")
        assert b"w must be one of 64,128,256,512,1024,2048" in err(lib)
    # the fp32 namesake refuses in the same words
    assert lib.fvta_attn_pool_fwd(ctypes.byref(_desc(w=1000)), *nul11) == -3
    fp32_words = err(lib)
    assert fwd(ctypes.byref(_desc(w=1000)), *nul11) == -3
    assert err(lib) == fp32_words.replace(b"attn_pool_fwd", b"attn_pool_fwd_bf16")
    # warp type 6: FVTA_ERR_INVALID_ARG from both warped entries
    for call, nul, who in ((fwd_tw, nul17, b"attn_pool_fwd_tw_bf16"), (energy, [None] * 6, b"attn_pool_energy_bf16")):
        assert call(ctypes.byref(_tw(warp_type=6)), *nul) == -1
        assert err(lib) == who + b": time warping type not implemented (warp_type=6)"
    # a pool that is not 8-byte aligned is refused before the launch (the other pointers are never followed)
    some = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1000 + 2)
    assert fwd(ctypes.byref(_desc()), odd, None, some, None, some, some, None, some, None, some, None) == -1
    assert err(lib) == b"attn_pool_fwd_bf16: the bf16 pool must be 8-byte aligned"
    assert energy(ctypes.byref(_tw()), odd, some, some, some, some, None) == -1
    assert err(lib) == b"attn_pool_energy_bf16: the bf16 pool must be 8-byte aligned"
    assert fwd_tw(ctypes.byref(_tw()), odd, None, some, some, None, some, some, some, None, some, some, some, some, None, None, some,
                  None) == -1
    assert err(lib) == b"attn_pool_fwd_tw_bf16: the bf16 pool must be 8-byte aligned"


def test_album_pool_dtype(monkeypatch):
    from tests import _attn_pooled_ref as R
    from fvta_memexqa_amd import nn, ops
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    g = torch.Generator().manual_seed(3)
    N, K, M, JX, w = 3, 2, 4, 5, 8
    hall = torch.randn(N, K, M, JX, w, generator=g)
    mask = torch.rand(N, K, M, JX, generator=g) < 0.5
    pool = hall[:, :, 0].contiguous()
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="dtype must be torch.float32 or torch.bfloat16"):
            nn.AlbumPool(pool, dtype=bad)
        with pytest.raises(ValueError, match="dtype must be torch.float32 or torch.bfloat16"):
            nn.AlbumPool.from_context(hall, mask, dtype=bad)
    f32, b16 = nn.AlbumPool(pool), nn.AlbumPool(pool, dtype=torch.bfloat16)
    assert f32.pool.dtype == torch.float32 and b16.pool.dtype == torch.bfloat16 and b16.pool.is_contiguous()
    assert f32.nbytes == pool.numel() * 4 and b16.nbytes * 2 == f32.nbytes
    assert torch.equal(b16.pool, pool.to(torch.bfloat16))                     # rounded to nearest even, once
    assert torch.equal(nn.AlbumPool(b16.pool, dtype=torch.bfloat16).pool, b16.pool)
    assert torch.equal(nn.AlbumPool(b16.pool).pool, b16.pool.float())         # the default stays fp32, whatever comes in
    # from_context cuts the same albums
    mem32, al32 = nn.AlbumPool.from_context(hall, mask)
    mem16, al16 = nn.AlbumPool.from_context(hall, mask, dtype=torch.bfloat16)
    assert torch.equal(al16, al32) and len(mem16) == len(mem32) == N * M and mem16.nbytes * 2 == mem32.nbytes
    assert mem16.pool.dtype == torch.bfloat16 and torch.equal(mem16.pool, mem32.pool.to(torch.bfloat16))
    assert torch.equal(mem16.pool_mask, mem32.pool_mask)
    c = dict(pool=mem16.pool, pm=mem16.pool_mask.bool(), albums=al16.long())
    h, m = R.expand(c)                                                         # laid end to end again: the rounded context
    assert torch.equal(h, hall.to(torch.bfloat16).reshape(N, K, M * JX, w)) and torch.equal(m, mask.reshape(N, K, M * JX))


def test_functional_refuses_a_bf16_pool_as_it_refuses_an_fp32_one(monkeypatch):
    """every host-side refusal of functional.attention_3d_pooled_raw, alone and in pairs (which of two comes first), with
    the op made to fail if it is reached: the same exception and words for both dtypes"""
    from fvta_memexqa_amd import functional as Fn, ops

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops.PooledFocalAttention, "forward", boom)
    monkeypatch.setattr(ops.PooledFocalAttention, "__init__", boom)
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    P, K, JX, JQ, w, NQ = 3, 2, 5, 4, 64, 2
    g = torch.Generator().manual_seed(5)
    pool32, hq = torch.randn(P, K, JX, w, generator=g), torch.randn(NQ, JQ, w, generator=g)
    pm, qm = torch.ones(P, K, JX, dtype=torch.bool), torch.ones(NQ, JQ, dtype=torch.bool)
    W, b = torch.randn(2 * w, 1, generator=g), torch.zeros(1)
    good, bad, ragged = [[0, 1], [1, 2]], [[0, P], [1, 2]], [[0, 1], [2]]
    grad_q = hq.clone().requires_grad_()
    # (albums, masks, hq, simi, grad mode) -> the exception and a word of its message, in the order the checks come
    calls = [
        (bad, True, hq, 2, False, ValueError, r"must lie in \[-1, 3\)"),
        (ragged, False, hq, 2, False, ValueError, "needs both masks"),
        (good, True, grad_q, 2, True, RuntimeError, "forward-only"),
        (bad, True, hq, 5, False, ValueError, "similarity matrix not implemented"),        # the similarity before the list
        (bad, True, grad_q, 2, True, RuntimeError, "forward-only"),                         # gradient mode before the list
        (bad, False, hq, 2, False, ValueError, r"must lie in"),                             # the range before the masks
        (good, True, hq, 2, False, AssertionError, "the library was reached"),              # valid: gets that far
    ]
    said = {}
    for dtype in (torch.float32, torch.bfloat16):
        pool = pool32.to(dtype)
        for i, (al, masked, q, simi, grad, exc, words) in enumerate(calls):
            with torch.set_grad_enabled(grad), pytest.raises(exc, match=words) as e:
                Fn.attention_3d_pooled_raw(pool, q, al, W, b, pm if masked else None, qm if masked else None, simiMatrix=simi)
            said.setdefault(i, []).append((type(e.value), str(e.value)))
        with pytest.raises(ValueError, match=r"expected \[P,K,JX,w\]"):
            with torch.no_grad():
                Fn.attention_3d_pooled_raw(pool[0], hq, good, W, b, pm, qm, simiMatrix=2)
    for i, (a, b16) in said.items():
        assert a == b16, (i, a, b16)
