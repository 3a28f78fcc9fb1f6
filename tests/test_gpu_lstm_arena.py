"""The bi-LSTM engine's ADDRESSING and SCHEDULING (model_v2.py:652-661, 694-823), which the value tests never vary: they
all run dense layouts (x_off = b*J*in, out_off = b*J*2d, seq_J = J, out_ld = 2d).  The model runs it on a shared arena.

  * arena layouts: several segments with their own seq_J, scattered x_off / out_off in two different orders with gaps,
    out_ld > 2d, a separate input per direction, dx_overwrite -- every element of every arena is either compared with the
    fp64 oracle (F.encode_stream per segment and its autograd), required to be an exact zero, or required to still hold
    the prefill's bits; x and d_out carry a large finite poison wherever the contract says "ignored";
  * out_skip on a shuffled arena (bf16 engine) and the shadow rows behind it;
  * the length sort (plan_sort_kernel) past J + 1 = 64, at J = 1024 and past 16384 ragged sequences;
  * last_state / last_state_bwd over sub-ranges, bit for bit;
  * a second plan / forward / backward on one op: nothing of the first batch survives in the op's buffers.

Tolerances are the ones the engines' value tests hold (tests/test_gpu_bf16.py, tests/test_gpu_backward.py): fp32 rtol 1e-4 /
atol 1e-5 on outputs and rtol 2e-4 / atol 2e-5 x max|ref| on gradients; bf16x3 rtol 1e-4 / atol 3e-5 x max|ref|; bf16 atol
3e-2 on outputs and 4e-2 relative L2 per gradient tensor."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, BF16, BF16X3 = 0, 1, 2
ENGINES = [F32, BF16, BF16X3]
ENGINE_IDS = ["f32", "bf16", "bf16x3"]
POISON = 1.0e3              # finite: "ignored" is the contract, not "never loaded"
SENT_BITS = 0x7FC12345      # a quiet NaN with a payload: no kernel writes these bits
GAP = 7.0                   # the dx arena's prefill between sequences
SEGMENTS = ((5, 3), (60, 7), (75, 12))      # B = 140: two 128-row tiles (fp32 engine), a partial last 32-row tile (wreg)
SHAPES = [(8, 32), (12, 128)]               # (din, d): the tiled kernels / in_internal = 32, lstm_fwd_wreg_bf16 <2, 8, ...>


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _sentinel(*shape, device="cuda"):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=device).view(torch.float32)


def _weights(g, din, d):
    lim = (6.0 / (din + 5 * d)) ** 0.5
    mk = lambda: ((torch.rand(din + d, 4 * d, generator=g) * 2 - 1) * lim, torch.randn(4 * d, generator=g) * 0.1)
    return mk() + mk()


def _check(precision, got, ref, name, grad, used=None):
    """got vs the fp64 reference at the engine's tolerance (module docstring); `used` collects the fraction taken"""
    a, b = got.detach().cpu().double().numpy().ravel(), ref.detach().cpu().double().numpy().ravel()
    assert np.isfinite(a).all(), "%s: not finite (an element nobody wrote?)" % name
    peak = float(np.abs(b).max()) if b.size else 0.0
    if precision == BF16 and grad:
        err = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
        if used is not None:
            used[name] = err / 4e-2
        assert err < 4e-2, "%s: relative L2 error %.4f" % (name, err)
        return
    if precision == BF16:
        rtol, atol = 0.0, 3e-2
    elif precision == BF16X3:
        rtol, atol = 1e-4, 3e-5 * peak
    else:
        rtol, atol = (2e-4, 2e-5 * peak) if grad else (1e-4, 1e-5)
    if used is not None and b.size:
        used[name] = float((np.abs(a - b) / (atol + rtol * np.abs(b) + 1e-300)).max())
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=name)


# ------------------------------------------------------------------------------------------------ 1. the arena helper
@functools.lru_cache(maxsize=None)
def _arena_case(segments, din, d, out_pad, seed, xdir):
    """segments ((count, seq_J), ...) -> one call's arenas (CPU, fp32; read-only: shared between tests).

    x arena: the sequences in a shuffled order, seq_J * din elements each, 4..16 elements (a multiple of 4) between
    neighbours; with xdir a second copy x_bw_delta = n_x elements behind.  out arena: rows of out_ld = 2d + out_pad, the
    sequences on seq_J consecutive rows each in ANOTHER shuffled order, 0..2 whole rows between neighbours.  x holds POISON
    at t >= len and in the gaps, d_out holds POISON at padded rows, in the pad columns and in the gap rows.  x_kind /
    out_kind classify every element: 1 valid (t < len), 2 padding (len <= t < seq_J), 0 nobody's."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    c = types.SimpleNamespace(segments=segments, din=din, d=d, out_pad=out_pad, xdir=xdir)
    seq_J = torch.cat([torch.full((n,), j, dtype=torch.int64) for n, j in segments])
    B, J = int(seq_J.numel()), int(seq_J.max())
    lens = torch.minimum((torch.rand(B, generator=g) * (seq_J + 1).double()).floor().long(), seq_J)
    s = 0
    for n, j in segments:           # every segment has an empty and a full sequence
        lens[s], lens[s + 1] = 0, j
        s += n
    x_off = torch.zeros(B, dtype=torch.int64)
    perm_x = torch.randperm(B, generator=g)
    pos = 4 * ri(1, 5)
    for b in perm_x.tolist():
        x_off[b] = pos
        pos += int(seq_J[b]) * din + 4 * ri(1, 5)
    n_x = pos
    out_ld = 2 * d + out_pad
    out_row = torch.zeros(B, dtype=torch.int64)
    perm_o = torch.randperm(B, generator=g)
    assert not torch.equal(perm_x, perm_o) and not torch.equal(perm_o, torch.arange(B))
    r = ri(1, 3)
    for b in perm_o.tolist():
        out_row[b] = r
        r += int(seq_J[b]) + ri(0, 3)
    nrows = r + 1
    x_kind = torch.zeros(n_x, dtype=torch.int8)
    out_kind = torch.zeros(nrows, out_ld, dtype=torch.int8)
    for b in range(B):
        o, L, Jb, r0 = int(x_off[b]), int(lens[b]), int(seq_J[b]), int(out_row[b])
        assert int(x_kind[o:o + Jb * din].sum()) == 0 and int(out_kind[r0:r0 + Jb].sum()) == 0     # no overlap
        x_kind[o:o + L * din] = 1
        x_kind[o + L * din:o + Jb * din] = 2
        out_kind[r0:r0 + L, :2 * d] = 1
        out_kind[r0 + L:r0 + Jb, :2 * d] = 2
    ncopy = 2 if xdir else 1
    x = torch.full((ncopy * n_x,), POISON)
    for k in range(ncopy):
        x[k * n_x:(k + 1) * n_x][x_kind == 1] = torch.randn(int((x_kind == 1).sum()), generator=g)
    d_out = torch.full((nrows, out_ld), POISON)
    d_out[out_kind == 1] = torch.randn(int((out_kind == 1).sum()), generator=g)
    c.B, c.J, c.seq_J, c.lens, c.x_off, c.out_row, c.out_off = B, J, seq_J, lens, x_off, out_row, out_row * out_ld
    c.n_x, c.ncopy, c.out_ld, c.nrows, c.x_kind, c.out_kind = n_x, ncopy, out_ld, nrows, x_kind, out_kind
    c.x, c.d_out, c.g_last = x, d_out, torch.randn(B, 2 * d, generator=g)
    c.weights = _weights(g, din, d)
    # the three classes partition each arena: no element escapes both the value check and the sentinel check
    for kind, numel in ((x_kind, n_x), (out_kind, nrows * out_ld)):
        parts = [(kind == v) for v in (0, 1, 2)]
        assert int(sum(p.sum() for p in parts)) == numel and bool((parts[0] ^ parts[1] ^ parts[2]).all())
        assert all(int(p.sum()) > 0 for p in parts)
    assert bool((out_kind[:, 2 * d:] == 0).all()) and int((out_kind.sum(1) == 0).sum()) >= 3      # pad columns, gap rows

    @functools.lru_cache(maxsize=None)
    def expected(share):
        """fp64: out arena (NaN where out_kind == 0), last [B, 2d], dx arena (NaN in the gaps), dkernel / dbias"""
        from oracle import fvta_fused as F
        w = [t.double().requires_grad_() for t in (c.weights[:2] if share else c.weights)]
        e = types.SimpleNamespace(out=torch.full((nrows, out_ld), float("nan"), dtype=torch.float64),
                                  last=torch.zeros(B, 2 * d, dtype=torch.float64),
                                  dx=torch.full((ncopy * n_x,), float("nan"), dtype=torch.float64))
        loss, keep, s0 = 0.0, [], 0
        for n, Js in segments:
            sl = slice(s0, s0 + n)
            xi = x_off[sl, None] + torch.arange(Js * din)[None, :]
            rows = out_row[sl, None] + torch.arange(Js)[None, :]
            mask = torch.arange(Js)[None, :] < lens[sl, None]
            xv = [(x[k * n_x + xi].view(n, Js, din).double() * mask[:, :, None]).requires_grad_() for k in range(ncopy)]
            gv = d_out[rows][:, :, :2 * d].double() * mask[:, :, None]           # the valid part of d_out only
            o, l = F.encode_stream(xv[0], mask, *w)
            if xdir:            # the backward direction reads its own copy
                o2, l2 = F.encode_stream(xv[1], mask, *w)
                o, l = torch.cat([o[:, :, :d], o2[:, :, d:]], 2), torch.cat([l[:, :d], l2[:, d:]], 1)
            loss = loss + (o * gv).sum() + (l * c.g_last[sl].double()).sum()
            keep.append((sl, xi, rows, xv, o, l))
            s0 += n
        loss.backward()
        for sl, xi, rows, xv, o, l in keep:
            e.out[rows, :2 * d] = o.detach()
            e.last[sl] = l.detach()
            for k in range(ncopy):
                e.dx[k * n_x + xi] = xv[k].grad.reshape(xi.shape)
        e.dw = [t.grad for t in w]
        assert bool((torch.isnan(e.out) == (out_kind == 0)).all()) and bool((torch.isnan(e.dx[:n_x]) == (x_kind == 0)).all())
        assert float(e.out[out_kind == 2].abs().max()) == 0.0 and float(e.dx[:n_x][x_kind == 2].abs().max()) == 0.0
        return e

    c.expected = expected
    return c


def _arena_op(c, precision, share, **kw):
    from fvta_memexqa_amd import ops
    return ops.BiLstm(c.B, c.J, c.din, c.d, c.x_off, c.out_off, c.seq_J.to(torch.int32), c.out_ld, share_fw_bw=share,
                      precision=precision, training=True, x_bw_delta=c.n_x if c.xdir else 0, **kw)


def _arena_weights(c, share):
    kf, bf, kb, bb = [t.cuda() for t in c.weights]
    return (kf, bf, None, None) if share else (kf, bf, kb, bb)


def _arena_forward_backward(c, precision, share):
    """plan, forward, last_state, last_state_bwd, backward (dx_overwrite) -> everything on the CPU"""
    op = _arena_op(c, precision, share, dx_overwrite=True)
    op.make_plan(c.lens)
    kf, bf, kb, bb = _arena_weights(c, share)
    x = c.x.cuda()
    out = _sentinel(c.nrows, c.out_ld)
    op.forward(x, out, kf, bf, kb, bb)
    last = _sentinel(c.B, 2 * c.d)
    op.last_state(out, 0, c.B, last)
    d_out = c.d_out.cuda()
    op.last_state_bwd(c.g_last.cuda(), 0, c.B, d_out)
    seq = (c.x_kind != 0).repeat(c.ncopy)
    dx0 = torch.where(seq, torch.tensor(float("nan")), torch.tensor(GAP))
    dx = dx0.cuda()
    dw = [torch.zeros_like(t) for t in ((kf, bf) if share else (kf, bf, kb, bb))]
    op.backward(x, out, d_out, kf, kb, dx, dw[0], dw[1], *(dw[2:] if not share else (None, None)))
    torch.cuda.synchronize()
    return types.SimpleNamespace(out=out.cpu(), last=last.cpu(), dx=dx.cpu(), dx0=dx0, dw=[t.cpu() for t in dw])


def _assert_arena(c, precision, share, got, tag):
    e = c.expected(share)
    used = {}
    valid, pad, other = (c.out_kind == 1), (c.out_kind == 2), (c.out_kind == 0)
    assert bool((valid ^ pad ^ other).all()) and int(valid.sum() + pad.sum() + other.sum()) == got.out.numel()
    # everything nobody owns keeps the prefill's bits: pad columns, gap rows, the rows past a short segment's seq_J
    stray = (_bits(got.out) != SENT_BITS) & other
    assert not bool(stray.any()), "%s: %d stray writes into the out arena, first (row, col) %r" % (
        tag, int(stray.sum()), stray.nonzero()[0].tolist())
    assert bool((_bits(got.out)[pad] == 0).all()), "%s: rows len <= t < seq_J are not exact zeros" % tag
    _check(precision, got.out[valid], e.out[valid], tag + " out", False, used)
    _check(precision, got.last, e.last, tag + " last", False, used)
    for k in range(c.ncopy):
        dx, dx_ref, dx0 = [t[k * c.n_x:(k + 1) * c.n_x] for t in (got.dx, e.dx, got.dx0)]
        xv, xp, xg = (c.x_kind == 1), (c.x_kind == 2), (c.x_kind == 0)
        assert bool((xv ^ xp ^ xg).all()) and int(xv.sum() + xp.sum() + xg.sum()) == dx.numel()
        assert torch.equal(_bits(dx)[xg], _bits(dx0)[xg]), "%s: dx copy %d: the gaps between sequences were written" % (tag, k)
        assert bool((dx[xp] == 0).all()), "%s: dx copy %d is not exactly 0 at len <= t < seq_J" % (tag, k)
        _check(precision, dx[xv], dx_ref[xv], "%s dx[%d]" % (tag, k), True, used)
    # the weight gradients sum over every row the kernels touched: poison read from x or d_out would land here
    for name, a, b in zip(("dkernel_fw", "dbias_fw", "dkernel_bw", "dbias_bw"), got.dw, e.dw):
        _check(precision, a, b, tag + " " + name, True, used)
    print("%s: fraction of the tolerance taken: %s" % (tag, " ".join("%s %.3f" % (k.split(" ")[-1], v) for k, v in used.items())))


# ------------------------------------------------------------------------------------ 2. arena layout against the oracle
@pytest.mark.parametrize("out_pad", [0, 8])
@pytest.mark.parametrize("share", [True, False], ids=["share", "fw_bw"])
@pytest.mark.parametrize("din,d", SHAPES)
@pytest.mark.parametrize("precision", ENGINES, ids=ENGINE_IDS)
def test_bilstm_on_a_shuffled_arena_matches_the_oracle(precision, din, d, share, out_pad):
    c = _arena_case(SEGMENTS, din, d, out_pad, 1000 + din + d + out_pad, False)
    assert c.B == 140 and c.B > 128 and c.B % 32 != 0 and c.J == 12 and len(set(c.seq_J.tolist())) == 3
    got = _arena_forward_backward(c, precision, share)
    _assert_arena(c, precision, share, got, "%s din=%d d=%d pad=%d" % (ENGINE_IDS[precision], din, d, out_pad))


@pytest.mark.parametrize("din,d", SHAPES)
@pytest.mark.parametrize("precision", [F32, BF16], ids=["f32", "bf16"])
def test_bilstm_on_a_shuffled_arena_with_an_input_per_direction(precision, din, d):
    """fvta_lstm_plan_xdir: the backward direction reads (and writes dx) x_bw_delta elements behind -- both copies checked"""
    c = _arena_case(SEGMENTS, din, d, 8, 2000 + din + d, True)
    assert c.ncopy == 2 and c.x.numel() == 2 * c.n_x and c.n_x % 4 == 0
    got = _arena_forward_backward(c, precision, True)
    _assert_arena(c, precision, True, got, "%s xdir din=%d d=%d" % (ENGINE_IDS[precision], din, d))


# --------------------------------------------------------------------------------------- 3. out_skip on a shuffled arena
@pytest.mark.parametrize("din,d", SHAPES)
def test_out_skip_on_a_shuffled_arena_and_its_shadow_rows(din, d):
    """out_skip (bf16 engine) at the first row of the sequence in the middle of the arena (a sequence is below it or above it
    as a whole, as in the model): sequences below leave their fp32 rows alone, the others are bitwise the plain call's, and
    the shadow rows of the ones below are bf16(out) of the plain call -- the caller's zero row where nobody wrote."""
    from fvta_memexqa_amd import ops
    c = _arena_case(SEGMENTS, din, d, 8, 1000 + din + d + 8, False)
    kf, bf, _, _ = _arena_weights(c, True)
    x = c.x.cuda()
    skip_row = int(c.out_row.sort().values[c.B // 2])
    below = c.out_row < skip_row
    assert 0 < int(below.sum()) < c.B and bool(((c.out_row + c.seq_J)[below] <= skip_row).all())
    outs = []
    for skip in (0, skip_row * c.out_ld):
        op = _arena_op(c, BF16, True, out_skip=skip)
        op.make_plan(c.lens)
        out = _sentinel(c.nrows, c.out_ld)
        op.forward(x, out, kf, bf)
        outs.append(out)
    zero_half = torch.zeros(d, dtype=torch.bfloat16, device="cuda")
    table = torch.full((2, skip_row), zero_half.data_ptr(), dtype=torch.int64, device="cuda")
    op.shadow_rows(table, skip_row)
    got = torch.full((skip_row, c.out_ld), 3.0, device="cuda")
    ops.rows_from_shadow(table, skip_row, d, c.out_ld, got)
    torch.cuda.synchronize()
    plain, skipped, got = outs[0].cpu(), outs[1].cpu(), got.cpu()
    assert bool((_bits(skipped)[:skip_row] == SENT_BITS).all()), "fp32 rows below out_skip were written"
    assert torch.equal(_bits(skipped)[skip_row:], _bits(plain)[skip_row:]), "rows above out_skip differ from the plain call"
    valid = (c.out_kind == 1)[:skip_row]
    want = torch.zeros(skip_row, c.out_ld)
    want[:, 2 * d:] = 3.0                                       # rows_from_shadow writes the 2d columns of a row only
    want[valid] = plain[:skip_row][valid].bfloat16().float()
    assert int(valid.sum()) > 0 and torch.equal(_bits(got), _bits(want)), "shadow rows != bf16(out) below out_skip"
    _check(BF16, plain[c.out_kind == 1], c.expected(True).out[c.out_kind == 1], "out", False)


# ------------------------------------------------------------------------------- 4./5. the length sort: long, big, ragged
@functools.lru_cache(maxsize=None)
def _dense_case(B, J, din, d, seed, fixed_lens=None, backward=True):
    """dense layout, ragged lengths with lens[0] = J and lens[1] = 0; d_out is random at EVERY position (the padded ones
    are ignored by contract).  -> inputs and the fp64 oracle's outputs / gradients (read-only)"""
    from oracle import fvta_fused as F
    g = torch.Generator().manual_seed(seed)
    c = types.SimpleNamespace(B=B, J=J, din=din, d=d)
    c.x = torch.randn(B, J, din, generator=g)
    if fixed_lens is None:
        c.lens = torch.randint(0, J + 1, (B,), generator=g)
        c.lens[0], c.lens[1] = J, 0
    else:
        c.lens = torch.tensor(fixed_lens)
    c.k, c.b = _weights(g, din, d)[:2]
    c.g_out = torch.randn(B, J, 2 * d, generator=g)
    c.g_last = torch.randn(B, 2 * d, generator=g)
    mask = torch.arange(J)[None, :] < c.lens[:, None]
    leaves = [t.double().requires_grad_(backward) for t in (c.x, c.k, c.b)]
    with torch.set_grad_enabled(backward):
        out, last = F.encode_stream(leaves[0], mask, leaves[1], leaves[2])
    if backward:
        ((out * (c.g_out * mask[:, :, None]).double()).sum() + (last * c.g_last.double()).sum()).backward()
        c.grads = [t.grad for t in leaves]
    c.out, c.last = out.detach(), last.detach()
    return c


def _dense_run_and_check(c, precision, tag, backward=True):
    """BiLstm built directly; `out` starts as NaN, so a sequence the sort lost or duplicated shows as an unwritten row"""
    from fvta_memexqa_amd import ops
    B, J, din, d = c.B, c.J, c.din, c.d
    ar = torch.arange(B, dtype=torch.int64)
    op = ops.BiLstm(B, J, din, d, ar * J * din, ar * J * 2 * d, torch.full((B,), J, dtype=torch.int32), 2 * d,
                    share_fw_bw=True, precision=precision, training=backward)
    op.make_plan(c.lens)
    x, k, b = c.x.cuda(), c.k.cuda(), c.b.cuda()
    out = _sentinel(B, J, 2 * d)
    op.forward(x, out, k, b)
    last = _sentinel(B, 2 * d)
    op.last_state(out, 0, B, last)
    used = {}
    _check(precision, out, c.out, tag + " out", False, used)
    _check(precision, last, c.last, tag + " last", False, used)
    pad = (torch.arange(J)[None, :] >= c.lens[:, None])
    assert bool((_bits(out)[pad] == 0).all()), tag + ": padded rows are not exact zeros"
    if backward:
        d_out = c.g_out.cuda()
        op.last_state_bwd(c.g_last.cuda(), 0, B, d_out)
        dx, dk, db = torch.zeros_like(x), torch.zeros_like(k), torch.zeros_like(b)
        op.backward(x, out, d_out, k, None, dx, dk, db)
        for name, a, r in zip(("dx", "dkernel", "dbias"), (dx, dk, db), c.grads):
            _check(precision, a, r, tag + " " + name, True, used)
        assert bool((dx.cpu()[pad] == 0).all()), tag + ": dx at padded positions"
    print("%s: fraction of the tolerance taken: %s" % (tag, " ".join("%s %.3f" % (k_.split(" ")[-1], v) for k_, v in used.items())))


LONG = [(300, 63, 8, 32),       # the last shape of the lane-per-length sort (H = 64)
        (300, 64, 8, 32),       # the first shape of the leader-by-leader sort
        (1100, 64, 4, 32),      # a wave's chunk > 64 sequences: several rounds of the leader loop per wave
        (37, 130, 4, 32)]       # most waves own 2-3 sequences, some none


@pytest.mark.parametrize("precision,B,J,din,d", [(F32,) + s for s in LONG] + [(BF16, 300, 64, 8, 32), (BF16X3, 300, 64, 8, 32)],
                         ids=lambda v: str(v))
def test_long_sequences_forward_backward(precision, B, J, din, d):
    """the bf16 engines at J = 64 as well: their saved state is indexed [2][J][B] and the weight gradient's step groups
    depend on J"""
    c = _dense_case(B, J, din, d, 3000 + B + J)
    assert J + 1 == 64 if (B, J) == LONG[0][:2] else J + 1 > 64           # lanes hold the histogram / the leaders do
    assert int(c.lens[0]) == J and int(c.lens[1]) == 0 and len(set(c.lens.tolist())) >= 13
    chunk = (B + 15) // 16                                                  # sequences per wave of the sort
    if B == 1100:
        assert chunk > 64
    if B == 37:
        assert chunk == 3 and 15 * chunk >= B                               # the last wave (at least) owns nothing
    _dense_run_and_check(c, precision, "%s B=%d J=%d" % (ENGINE_IDS[precision], B, J))


def test_sequences_of_1024_steps_forward_and_last_state():
    """J = 1024, the largest the descriptor admits: the sort's [16][J + 1] histogram is 65,600 bytes of dynamic LDS, above
    64 KiB (gfx950 gives one workgroup up to 160 KiB and the launch is accepted without opting in: a refused launch would
    fail make_plan here).  Forward and last_state at the fp32 tolerance (the oracle run in fp32 is within 2e-7 of fp64 at
    this shape: 1024 steps do not call for a wider one)."""
    B, J, din, d = 3, 1024, 4, 32
    c = _dense_case(B, J, din, d, 4024, fixed_lens=(1024, 1, 517), backward=False)
    assert J + 1 > 64 and 16 * (J + 1) * 4 > 64 * 1024
    _dense_run_and_check(c, F32, "f32 B=3 J=1024", backward=False)


def test_autograd_bilstm_takes_long_sequences():
    """the public differentiable entry (autograd.bilstm) at J = 70: the same plan path, through torch.autograd.grad"""
    from fvta_memexqa_amd import autograd as A
    B, J, din, d = 50, 70, 8, 32
    c = _dense_case(B, J, din, d, 5070)
    assert J + 1 > 64 and len(set(c.lens.tolist())) >= 13
    leaves = [t.cuda().requires_grad_() for t in (c.x, c.k, c.b)]
    out, last = A.bilstm(leaves[0], c.lens.cuda(), leaves[1], leaves[2], precision="f32")
    grads = torch.autograd.grad((out * c.g_out.cuda()).sum() + (last * c.g_last.cuda()).sum(), leaves)
    _check(F32, out, c.out, "out", False)
    _check(F32, last, c.last, "last", False)
    # (autograd multiplies nothing by the mask here: d_out at padded positions is c.g_out's random values)
    for name, a, r in zip(("dx", "dkernel", "dbias"), grads, c.grads):
        _check(F32, a, r, name, True)


def test_big_ragged_batch_forward_backward():
    """B = 16448 ragged: a wave's chunk is 1028 > 1024 sequences, so the sort reads its lengths back from the plan and moves
    the running bases by shuffle (every other ragged test is at most 16384; the one above it is dense: a trivial sort)"""
    B, J, din, d = 16448, 3, 4, 32
    c = _dense_case(B, J, din, d, 6000)
    assert (B + 15) // 16 > 1024 and J + 1 <= 64 and sorted(set(c.lens.tolist())) == [0, 1, 2, 3]
    _dense_run_and_check(c, F32, "f32 B=16448 J=3")


# --------------------------------------------------------------------------- 6. last_state / last_state_bwd sub-ranges
@pytest.mark.parametrize("which", [0, 1, 2])
def test_last_state_sub_ranges_bitwise(which):
    din, d = SHAPES[0]
    c = _arena_case(SEGMENTS, din, d, 8, 1000 + din + d + 8, False)
    s0, count = [(0, c.B), (5, 60), (c.B - 1, 1)][which]
    op = _arena_op(c, F32, True)
    op.make_plan(c.lens)
    kf, bf, _, _ = _arena_weights(c, True)
    out = _sentinel(c.nrows, c.out_ld)
    op.forward(c.x.cuda(), out, kf, bf)
    dst = _sentinel(count + 1, 2 * d)
    op.last_state(out, s0, count, dst)
    g = torch.Generator().manual_seed(60 + which)
    d_out0 = torch.randn(c.nrows, c.out_ld, generator=g)
    d_dst = torch.randn(count, 2 * d, generator=g)
    d_out = d_out0.cuda()
    op.last_state_bwd(d_dst.cuda(), s0, count, d_out)
    torch.cuda.synchronize()
    out_h = out.cpu()
    want = _sentinel(count + 1, 2 * d, device="cpu").clone()
    want_d = d_out0.clone()
    lens_in_range = c.lens[s0:s0 + count].tolist()
    assert which != 0 or (0 in lens_in_range and max(lens_in_range) == c.J)
    for s in range(count):
        b = s0 + s
        L, r0 = int(c.lens[b]), int(c.out_row[b])
        if L == 0:          # no final state: zeros, and no gradient anywhere
            want[s] = 0.0
            continue
        want[s, :d] = out_h[r0 + L - 1, :d]             # the forward direction ends at t = len - 1 ...
        want[s, d:] = out_h[r0, d:2 * d]                # ... the reversed one at t = 0
        want_d[r0 + L - 1, :d] += d_dst[s, :d]
        want_d[r0, d:2 * d] += d_dst[s, d:]
    assert torch.equal(_bits(dst), _bits(want)), "last_state(s0=%d, count=%d)" % (s0, count)
    assert torch.equal(_bits(d_out), _bits(want_d)), "last_state_bwd(s0=%d, count=%d)" % (s0, count)
    assert int((_bits(d_out) != _bits(d_out0)).sum()) <= 2 * d * sum(1 for L in lens_in_range if L > 0)


# --------------------------------------------------------------------------------------------- 7. re-planning one op
@pytest.mark.parametrize("overwrite", [True, False], ids=["dx_overwrite", "dx_accumulate"])
@pytest.mark.parametrize("precision", ENGINES, ids=ENGINE_IDS)
def test_second_plan_on_one_op_is_bitwise_a_fresh_op(precision, overwrite):
    """saved, dzb and cstate are reused by the second round; the bf16 backward reads dc of rows that were not active at
    step t + 1 as zero by the PLAN, not by a memset -- so nothing of the first batch may show: out, dx, dkernel and dbias
    of the second round are bitwise those of a fresh op with the same inputs and prefills."""
    from fvta_memexqa_amd import ops
    B, J, din, d = 140, 12, 12, 128
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, J, din, generator=g).cuda()
    k, b = [t.cuda() for t in _weights(g, din, d)[:2]]
    g_out = torch.randn(B, J, 2 * d, generator=g).cuda()        # random at padded positions too
    lens1 = torch.randint(0, J + 1, (B,), generator=g)
    lens1[0], lens1[1] = J, 0
    lens2 = (lens1.double() * torch.rand(B, generator=g)).floor().long()          # mostly shorter ...
    lens2[::9] = torch.minimum(lens1[::9] + 3, torch.tensor(J))                    # ... a few longer
    lens2[1] = 5
    assert int((lens2 < lens1).sum()) > B // 2 and int((lens2 > lens1).sum()) >= 10
    ar = torch.arange(B, dtype=torch.int64)
    mk = lambda: ops.BiLstm(B, J, din, d, ar * J * din, ar * J * 2 * d, torch.full((B,), J, dtype=torch.int32), 2 * d,
                            share_fw_bw=True, precision=precision, training=True, dx_overwrite=overwrite)

    def round_(op, lens):
        op.make_plan(lens)
        out = torch.full((B, J, 2 * d), 7.0, device="cuda")
        op.forward(x, out, k, b)
        dx = torch.full_like(x, float("nan")) if overwrite else torch.zeros_like(x)
        dk, db = torch.zeros_like(k), torch.zeros_like(b)
        op.backward(x, out, g_out, k, None, dx, dk, db)
        torch.cuda.synchronize()
        return out, dx, dk, db

    op = mk()
    first = round_(op, lens1)
    second = round_(op, lens2)
    fresh = round_(mk(), lens2)
    assert not torch.equal(first[2], second[2])
    assert bool(torch.isfinite(second[1]).all())
    for name, a, e in zip(("out", "dx", "dkernel", "dbias"), second, fresh):
        assert torch.equal(_bits(a), _bits(e)), "%s: the second round on one op differs from a fresh op" % name
