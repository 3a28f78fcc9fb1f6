"""The album pool held in bf16 on the GPU (fvta_attn_pool_fwd_bf16 / fvta_attn_pool_energy_bf16 /
fvta_attn_pool_fwd_tw_bf16; ops.PooledFocalAttention, ops.PooledWarpedFocalAttention, functional, nn.AlbumPool).

The contract is bitwise: a call on a bf16 pool returns what the same call returns on the WIDENED pool (pool.float(), every
bf16 value as the fp32 it stands for) -- the kernels load four bf16 where they loaded four floats, widen in registers,
which is exact, and keep every lane on its channels.  So the oracle is the fp32 pooled call itself, which
tests/test_gpu_attn_pooled.py and tests/test_gpu_attn_pooled_tw.py hold against fp64; a subset is held against fp64 here
as well (the reference on the widened pool, at those files' tolerances: the rows are exact in fp64, nothing new to allow).
The cases are those files' (tests/_attn_pooled_ref.py, tests/_attn_pooled_tw_ref.py): w = 64 (16 live lanes in the row
terms) to 2048 (the weighted sum's second 1024-channel block), JX = 1, R-1, R, R+1, JQ = 1 .. 64, empty slots, an album
listed twice, an album nobody lists.  The bf16 pool of a case is c["pool"].to(torch.bfloat16).  Every index given to a GPU
call is valid."""
import ctypes

import pytest
import torch

from tests import _attn_pooled_ref as R
from tests import _attn_pooled_tw_ref as PT
from tests._album_attn_gpu import album_energy, close, cu, infer, modules, once

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _same(got, want, what=""):
    for g, w_, name in zip(got, want, ("h_a", "a_logits", "scale")):
        assert (g is None) == (w_ is None), (what, name)
        if g is not None:
            assert g.dtype == torch.float32 and torch.equal(g, w_), "%s %s: max |diff| %.3g" % (what, name, float((g - w_).abs().max()))


def _case(key):
    """a case with its bf16 pool and the widened pool, built once and never written to.  key: (name, simi, tanh, masked) of
    R.CASES, a name of R.LOOP_IDS, or ("tw", name) of the warped reference"""
    def make():
        if isinstance(key, tuple) and key[0] == "tw":
            c = PT.build_case(key[1])
        elif isinstance(key, tuple):
            c = dict(R.build_case(key[0], key[1], key[3]), tanh=key[2])
        else:
            c = R.loop_case(key)
        bf = c["pool"].to(BF16)
        return dict(c, bf=bf, wide=bf.float())
    return once(("bf16", key), make)


def _fwd(c, pool, want_logits=True):
    """ops.PooledFocalAttention.forward on case c with `pool` (on the device) in place of the case's"""
    return infer(c, "pooled", pool=pool, want_logits=want_logits)


def _fwd_tw(c, pool, energy=None):
    """ops.PooledWarpedFocalAttention on case c with `pool` -> (energy, (h_a, a_logits, scale))"""
    if energy is None:
        energy = album_energy(c, "pooled", rows=pool)
    return energy, infer(c, "pooled", True, pool=pool, energy=energy)


# ------------------------------------------------------------------ 1. the same bits
def _same_bits_unwarped(c, what):
    bf, wide = cu(c["bf"]), cu(c["wide"])
    assert bf.dtype == BF16 and wide.dtype == torch.float32
    want = _fwd(c, wide)
    got = _fwd(c, bf)
    _same(got, want, what)
    _same(_fwd(c, bf), got, what + " (the second call)")
    assert bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("name,simi,tanh,masked", R.CASES, ids=R.CASE_IDS)
def test_bf16_pool_gives_the_bits_of_the_widened_pool(name, simi, tanh, masked):
    _same_bits_unwarped(_case((name, simi, tanh, masked)), name)


@pytest.mark.parametrize("name", R.LOOP_IDS)
def test_loop_cases_give_the_bits_of_the_widened_pool(name):
    _same_bits_unwarped(_case(name), name)


# ------------------------------------------------------------------ 2. the same bits under the warp
@pytest.mark.parametrize("name", PT.NAMES)
def test_warped_bf16_pool_gives_the_bits_of_the_widened_pool(name):
    c = _case(("tw", name))
    bf, wide = cu(c["bf"]), cu(c["wide"])
    e_want, want = _fwd_tw(c, wide)
    e_got, got = _fwd_tw(c, bf)
    assert tuple(e_got.shape) == (c["P"], c["JX"]) and torch.equal(e_got, e_want), name
    _same(got, want, name)
    _same(_fwd_tw(c, bf, e_got)[1], got, name + " (the second call, the kept energy)")


def test_the_warped_cases_cover_every_warp_type():
    assert {PT.SPECS[n][9] for n in PT.NAMES} == {1, 2, 3, 4, 5}


# ------------------------------------------------------------------ 3. against fp64, on the widened pool
FP64_CASES = [(k, i) for k, i in zip(R.CASES, R.CASE_IDS) if k[0] == "mix" or k[0].startswith("rows") or k[0] == "wide2048"]


@pytest.mark.parametrize("key", [k for k, _ in FP64_CASES], ids=[i for _, i in FP64_CASES])
def test_matches_the_fp64_reference_on_the_widened_pool(key):
    name, simi, tanh, masked = key
    c = _case(key)
    ref_ha, ref_a = once(("bf16 fp64", key), lambda: R.reference(dict(c, pool=c["wide"]), tanh))
    ha, a = _fwd(c, cu(c["bf"]))
    live = ref_a > -1e29
    print("%s h_a: max |got - ref| %.3g, max |ref| %.3g; a_logits: max |got - ref| over valid entries %.3g"
          % (name, float((ha.cpu().double() - ref_ha).abs().max()), float(ref_ha.abs().max()),
             float((a.cpu().double() - ref_a)[live].abs().max()) if bool(live.any()) else 0.0))
    close(ha, ref_ha, rtol=1e-4, atol=1e-5, msg="h_a")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")


def test_the_fp64_subset_is_what_it_says():
    names = {k[0] for k, _ in FP64_CASES}
    assert names == {"mix", "wide2048"} | {"rows%d" % i for i in range(6)}
    assert sum(1 for k, _ in FP64_CASES if k[0] == "mix") == 8 and sum(1 for k, _ in FP64_CASES if k[0] == "wide2048") == 2


# ------------------------------------------------------------------ 4. no fp32 copy
def _no_copy_case():
    """P = 8, K = 2, JX = 64, w = 1024, NQ = 2, M = 2: the bf16 pool is 2 MiB, an fp32 copy of it 4 MiB"""
    g = torch.Generator().manual_seed(41)
    P, K, JX, w, NQ, M, JQ = 8, 2, 64, 1024, 2, 2, 5
    return dict(P=P, K=K, JX=JX, w=w, NQ=NQ, M=M, JQ=JQ, simi=2, tanh=True, pm=None, qm=None,
                pool=(torch.randn(P, K, JX, w, generator=g) * 0.5).to(BF16).cuda(), q=(torch.randn(NQ, JQ, w, generator=g) * 0.5).cuda(),
                W=(torch.randn(2 * w, 1, generator=g) * 0.1).cuda(), b=torch.zeros(1).cuda(), albums=torch.tensor([[0, 3], [3, 7]]))


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, out


def test_no_fp32_copy_of_the_pool_is_made():
    from fvta_memexqa_amd import _lib, nn, ops
    c = _no_copy_case()
    pool_bytes = c["pool"].numel() * c["pool"].element_size()
    assert pool_bytes == 2 << 20 and c["pool"].dtype == BF16
    # a condition on the shape, from the host-only size query: everything the call allocates is smaller than the pool
    desc = _lib.AttnPoolDesc(c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"], c["simi"], 1)
    work = _lib.load().fvta_attn_pool_workspace_bytes(ctypes.byref(desc))
    outputs = c["NQ"] * c["w"] * 4
    assert 0 < work and work + outputs < pool_bytes, (work, outputs)
    op = ops.PooledFocalAttention(c["P"], c["NQ"], c["M"], c["K"], c["JX"], c["JQ"], c["w"], c["simi"], c["tanh"])
    idx = ops.check_album_lists(c["albums"], c["P"], False).cuda()
    W = c["W"].reshape(-1).contiguous()
    rise, (ha, none) = _peak_rise(lambda: op.forward(c["pool"], None, c["q"], None, idx, W, c["b"], want_logits=False))
    print("ops.PooledFocalAttention.forward on a 2 MiB bf16 pool: workspace %d B, peak rose by %d B" % (work, rise))
    assert none is None and rise < pool_bytes, rise                            # an fp32 copy alone is twice the pool
    # the holder: the rows stay where they are through functional / nn (op, workspace, index and outputs are allocated)
    att = nn.FocalAttention3D(c["w"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    with torch.no_grad():
        att.p("att_logits/W").copy_(c["W"])
        att.p("att_logits/b").copy_(c["b"])
        mem = nn.AlbumPool(c["pool"], dtype=BF16)
        assert mem.pool.data_ptr() == c["pool"].data_ptr() and mem.nbytes == pool_bytes     # held as it came
        a_bytes = c["NQ"] * c["K"] * c["M"] * c["JX"] * c["JQ"] * 4                          # attend() asks for the logits
        assert work + outputs + a_bytes + c["q"].numel() * 4 < pool_bytes
        rise2, (ha2, a2) = _peak_rise(lambda: mem.attend(att, c["q"], None, c["albums"]))
    print("nn.AlbumPool(dtype=bfloat16).attend: peak rose by %d B" % rise2)
    assert rise2 < pool_bytes, rise2
    assert torch.equal(ha2, ha)


# ------------------------------------------------------------------ 5. nothing outside the listed albums is read
def _poison_case(w, JX):
    """P = 4, album 1 listed by nobody; M = 2, K = 2, JQ = 7, masked (the recipe's masks: (album 0, k 0) fully masked)"""
    G, _ = R.host_plan(7, w)
    seed = 1000 + w + JX
    c = R.make_case(R.lists_from_counts([G + 1, 0, 2, 1], 2, seed, True), 4, 2, JX, 7, w, 2, True, seed)
    c = PT.TW.add_warp(dict(c, tanh=True), seed, 5)
    assert not bool((c["albums"] == 1).any()) and bool((c["albums"] == 0).any())
    return c


@pytest.mark.parametrize("w", [64, 2048])
@pytest.mark.parametrize("jx", ["1", "R+1"])
def test_nothing_outside_the_listed_albums_is_read(w, jx):
    JX = 1 if jx == "1" else R.host_plan(7, w)[1] + 1
    c = _poison_case(w, JX)
    clean = cu(c["pool"].to(BF16))
    n, pad = clean.numel(), 4 * w                                             # the pool stays 8-byte aligned in the buffer
    nan = torch.full((n + 2 * pad,), float("nan"), dtype=BF16, device="cuda")
    assert int(nan.view(torch.int16)[0]) == 0x7FC0                            # the bf16 NaN pattern
    inside = nan[pad:pad + n].view(c["P"], c["K"], JX, w)
    inside.copy_(clean)
    inside[1] = float("nan")                                                  # the album nobody lists
    assert inside.is_contiguous() and inside.data_ptr() % 8 == 0 and bool(torch.isnan(nan[:pad]).all())
    assert bool(torch.isnan(nan[pad + n:]).all()) and bool(torch.isnan(inside[1]).all())
    want = _fwd(c, clean)
    got = _fwd(c, inside)
    _same(got, want, "poisoned surroundings")
    assert all(bool(torch.isfinite(t).all()) for t in got)
    # under the warp: the energy is the pool's, every album's -- the unlisted album's is NaN and is never read either
    e_clean, want_tw = _fwd_tw(c, clean)
    e_in, got_tw = _fwd_tw(c, inside)
    keep = [0, 2, 3]
    assert torch.equal(e_in[keep], e_clean[keep]) and bool(torch.isnan(e_in[1]).all())
    _same(got_tw, want_tw, "poisoned surroundings, warped")
    assert all(bool(torch.isfinite(t).all()) for t in got_tw)
    assert bool(torch.isnan(nan[:pad]).all()) and bool(torch.isnan(nan[pad + n:]).all())    # and nothing was written there


# ------------------------------------------------------------------ 6. nn.AlbumPool(dtype=torch.bfloat16)
def test_album_pool_in_bf16_is_the_fp32_pool_of_the_widened_rows():
    from fvta_memexqa_amd import functional as Fn, nn
    c = _case(("tw", "mix-simi2-masked"))
    att, tw = modules(c)
    q, lq, pm, qm = cu(c["q"]), cu(c["lq"]), cu(c["pm"]), cu(c["qm"])
    with torch.no_grad():
        mem = nn.AlbumPool(cu(c["pool"]), pm, dtype=BF16)                     # fp32 rows in: rounded once, here
        ref = nn.AlbumPool(cu(c["wide"]), pm)
        assert mem.pool.dtype == BF16 and ref.pool.dtype == torch.float32 and torch.equal(mem.pool.float(), ref.pool)
        assert mem.nbytes * 2 == ref.nbytes and len(mem) == len(ref) == c["P"]
        _same(mem.attend(att, q, qm, c["albums"]), ref.attend(att, q, qm, c["albums"]), "attend")
        got = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)
        _same(got, ref.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq), "attend under the warp")
        _same(got, _fwd_tw(c, cu(c["bf"]))[1][:2], "attend against the op")
        # the energy: computed once, kept, recomputed after an in-place change of WH/W
        e0 = mem.energy(tw)
        assert mem.energy(tw) is e0 and torch.equal(e0, ref.energy(tw)) and tuple(e0.shape) == (c["P"], c["JX"])
        assert torch.equal(e0, Fn.album_energy(mem.pool, tw.p("WH/W"), tw.p("WC/W")))
        tw.p("WH/W").mul_(0.5)
        e1 = mem.energy(tw)
        assert e1 is not e0 and not torch.equal(e1, e0) and torch.equal(e1, ref.energy(tw))
        got2 = mem.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq)
        _same(got2, ref.attend(att, q, qm, c["albums"], time_warp=tw, lq=lq), "attend after the update")
        assert mem.energy(tw) is e1 and not torch.equal(got2[0], got[0])
        # the functional surface on the same tensor
        ha, a = Fn.attention_3d_pooled_raw(mem.pool, q, c["albums"], cu(c["W"]), cu(c["b"]), pm, qm, simiMatrix=c["simi"],
                                           add_tanh=c["tanh"])
        _same((ha, a), mem.attend(att, q, qm, c["albums"]), "functional")


def test_a_padded_width_stays_bf16_and_exact():
    """w = 100 runs at the kernels' 128: the bf16 pool is zero padded in bf16, which is exact"""
    from fvta_memexqa_amd import functional as Fn
    c = R.make_case(R.lists_from_counts([3, 1, 2], 2, 7, True), 3, 2, 9, 5, 100, 3, True, 71)
    bf = cu(c["pool"].to(BF16))
    args = (cu(c["q"]), c["albums"], cu(c["W"]), cu(c["b"]), cu(c["pm"]), cu(c["qm"]))
    with torch.no_grad():
        got = Fn.attention_3d_pooled_raw(bf, *args, simiMatrix=3, add_tanh=True)
        want = Fn.attention_3d_pooled_raw(bf.float(), *args, simiMatrix=3, add_tanh=True)
    assert tuple(got[0].shape) == (c["NQ"], 100)
    _same(got, want, "w = 100")


# ------------------------------------------------------------------ 7. training still widens
def test_training_over_a_bf16_leaf_still_widens():
    from fvta_memexqa_amd import functional as Fn
    c = _case(("mix", 2, True, True))
    leaf = cu(c["bf"]).requires_grad_()
    ha, a = Fn.attention_3d_pooled_raw(leaf, cu(c["q"]), c["albums"], cu(c["W"]), cu(c["b"]), cu(c["pm"]), cu(c["qm"]),
                                       simiMatrix=2, add_tanh=True, differentiable=True)
    ha.sum().backward()
    assert leaf.grad is not None and leaf.grad.dtype == BF16 and tuple(leaf.grad.shape) == tuple(leaf.shape)
    assert bool(torch.isfinite(leaf.grad.float()).all()) and float(leaf.grad.float().abs().max()) > 0
    with torch.no_grad():                                                      # the forward it took: the widened rows'
        _same((ha.detach(),), (Fn.attention_3d_pooled_raw(leaf.detach().float(), cu(c["q"]), c["albums"], cu(c["W"]), cu(c["b"]),
                                                          cu(c["pm"]), cu(c["qm"]), simiMatrix=2, add_tanh=True)[0],), "forward")
