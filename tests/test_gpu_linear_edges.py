"""fvta_linear_fwd[_blk] / fvta_linear_bwd[_blk] (csrc/elementwise.hip: linear_kernel, linear_bwd_dx_kernel,
linear_bwd_dw_kernel) at the edges of their 64 x 64 tiles and 16-deep k slices, dense and on one stream of an arena,
against fp64 on the CPU computed from the fp32 inputs.

The error bound is derived, not measured.  An output that is a sum of K products (+ a bias), the products rounded or fused,
summed in any order, gets, per element and in fp64,

    bound = (K + 16) * 2^-24 * (sum_k |a_k| |b_k| + |bias|)

-- the first-order forward error bound of fp32 round-to-nearest summation in any order; the 16 covers the bias add and the
three roundings of dyt = dy (1 - y^2).  Added onto a non-zero start (dW, db always; dx under accumulate_dx) the one more
addition adds 2^-23 |start + sum|.  Behind a tanh the pre-activation's bound holds for the output (|tanh'| <= 1) and 1e-5 is
added for tanhf itself (the forward atol of tests/test_gpu_v1_ops.py::test_linear_bwd_against_autograd).  Backward
references take the kernel's own fp32 y as given and form dyt in fp64 from it, so no forward error enters.  Every test
prints its worst |got - ref| / bound; above 1 the kernel does not do the arithmetic its comment says."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENT = -7777.25          # guard-band / overwrite sentinel (exact in fp32)
PAD = 96                 # floats of guard band on each side of y and of W

# (blocks, rows_per_blk, gap rows between blocks, in, out); dense shapes (M, in, out) are one block without a gap
DENSE = [(1, 1, 1), (63, 15, 63), (64, 16, 64), (65, 17, 65), (129, 130, 70), (1000, 33, 130), (200, 300, 5)]
BLOCKED = [(7, 29, 11, 48, 20), (3, 64, 5, 17, 65), (70, 1, 2, 16, 64)]
CASES = [(1, M, 0, din, dout) for M, din, dout in DENSE] + BLOCKED
IDS = ["dense-%dx%dx%d" % s for s in DENSE] + ["blocked-%dx%d+%d-%dx%d" % s for s in BLOCKED]


def _bound(K, absprod, bias=None):
    return (K + 16) * EPS * (absprod + (0 if bias is None else bias.abs()))


def _check(got, ref, bound, what):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), what + ": not finite"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    print("%s: worst |got - ref| / bound = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst |got - ref| / bound = %.4f" % (what, worst)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(blocks, rpb, gap, din, dout):
    """fp32 inputs and starts on the CPU, seeded; the stream's rows are rows [off, off + rpb) of every block"""
    g = torch.Generator().manual_seed(7 + 1009 * blocks + 101 * rpb + 13 * din + dout)
    M, rows, off = blocks * rpb, rpb + gap, gap // 2
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(M=M, rows=rows, off=off, din=din, dout=dout, blk=(rpb, rows * din) if gap else None,
             arena=rn(blocks, rows, din), W=rn(din, dout) * 0.2, b=rn(dout), dy=rn(M, dout), dx0=rn(blocks, rows, din),
             dW0=rn(din, dout), db0=rn(dout))
    c["mine"] = torch.zeros(blocks, rows, dtype=torch.bool)
    c["mine"][:, off:off + rpb] = True
    c["x"] = c["arena"][:, off:off + rpb].reshape(M, din)
    x64, W64 = c["x"].double(), c["W"].double()
    c["pre"] = x64 @ W64                                     # without the bias
    c["pre_abs"] = x64.abs() @ W64.abs()
    return c


class _Dev:
    """the case on the device: the arena's other rows and a band around W hold NaN"""

    def __init__(self, c):
        from fvta_memexqa_amd import ops
        self.dev = ops.require_gpu()
        arena = c["arena"].clone()
        arena[~c["mine"]] = float("nan")
        self.arena = arena.to(self.dev)
        self.x = self.arena.view(-1)[c["off"] * c["din"]:]
        wbuf = torch.full((2 * PAD + c["din"] * c["dout"],), float("nan"))
        wbuf[PAD:PAD + c["din"] * c["dout"]] = c["W"].reshape(-1)
        self.wbuf = wbuf.to(self.dev)
        self.W = self.wbuf[PAD:PAD + c["din"] * c["dout"]]
        self.b, self.dy = c["b"].to(self.dev), c["dy"].to(self.dev)

    def forward(self, c, tanh, bias=True):
        """(y, its buffer with the guard bands)"""
        from fvta_memexqa_amd import ops
        n = c["M"] * c["dout"]
        ybuf = torch.full((2 * PAD + n,), SENT, device=self.dev)
        y = ybuf[PAD:PAD + n]
        ops.linear_fwd(self.x, self.W, self.b if bias else None, y, c["M"], c["din"], c["dout"], tanh, blk=c["blk"])
        return y, ybuf


@pytest.mark.parametrize("tanh", [False, True], ids=["linear", "tanh"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward(case, tanh):
    from fvta_memexqa_amd import ops
    c = _case(*case)
    d = _Dev(c)
    M, din, dout = c["M"], c["din"], c["dout"]
    act = torch.tanh if tanh else (lambda t: t)
    extra = 1e-5 if tanh else 0.0
    y, ybuf = d.forward(c, tanh)
    _check(y.view(M, dout), act(c["pre"] + c["b"].double()), _bound(din, c["pre_abs"], c["b"].double()) + extra,
           "linear_kernel y %s" % (case,))
    band = torch.full((PAD,), SENT, device=d.dev)
    assert torch.equal(_bits(ybuf[:PAD]), _bits(band)) and torch.equal(_bits(ybuf[-PAD:]), _bits(band)), "y's guard band"
    first = y.clone()                                        # the same call on the same buffers: the same bits
    ops.linear_fwd(d.x, d.W, d.b, y, M, din, dout, tanh, blk=c["blk"])
    assert torch.equal(_bits(first), _bits(y)), "two forward calls differ"
    y0, ybuf0 = d.forward(c, tanh, bias=False)               # b == NULL
    _check(y0.view(M, dout), act(c["pre"]), _bound(din, c["pre_abs"]) + extra, "linear_kernel y without b %s" % (case,))
    assert torch.equal(_bits(ybuf0[:PAD]), _bits(band)) and torch.equal(_bits(ybuf0[-PAD:]), _bits(band)), "y's guard band"


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("tanh", [False, True], ids=["linear", "tanh"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward(case, tanh, accumulate):
    from fvta_memexqa_amd import ops
    c = _case(*case)
    d = _Dev(c)
    M, din, dout, mine = c["M"], c["din"], c["dout"], c["mine"]
    y = d.forward(c, tanh)[0] if tanh else None
    dy64 = c["dy"].double()
    dyt = dy64 * (1 - y.view(M, dout).cpu().double() ** 2) if tanh else dy64
    x64, W64 = c["x"].double(), c["W"].double()
    dx_start = c["dx0"] if accumulate else torch.full_like(c["dx0"], SENT)

    def run(dx=True, dW=True, db=True):
        """one call from the same starts: (dx arena, dW, db), None where the pointer was NULL"""
        o_dx = dx_start.to(d.dev) if dx else None
        o_dW = c["dW0"].to(d.dev) if dW else None
        o_db = c["db0"].to(d.dev) if db else None
        ops.linear_bwd(d.x if dW else None, d.W, y, d.dy, o_dx.view(-1)[c["off"] * din:] if dx else None, o_dW, o_db, M, din,
                       dout, tanh, accumulate_dx=accumulate, blk=c["blk"])
        return o_dx, o_dW, o_db

    dx, dW, db = run()
    tag = "%s tanh=%d accumulate=%d" % (case, tanh, accumulate)
    # dx: K = out
    ref = dyt @ W64.t()
    bound = _bound(dout, dyt.abs() @ W64.abs().t())
    if accumulate:
        ref = ref + c["dx0"][mine].reshape(M, din).double()
        bound = bound + 2 * EPS * ref.abs()
    _check(dx.cpu()[mine].reshape(M, din), ref, bound, "linear_bwd_dx_kernel dx " + tag)
    assert torch.equal(_bits(dx.cpu()[~mine]), _bits(dx_start[~mine])), "the other streams' rows of dx changed"
    # dW, db: K = M, always onto a non-zero start
    ref = c["dW0"].double() + x64.t() @ dyt
    _check(dW, ref, _bound(M, x64.abs().t() @ dyt.abs()) + 2 * EPS * ref.abs(), "linear_bwd_dw_kernel dW " + tag)
    ref = c["db0"].double() + dyt.sum(0)
    _check(db, ref, _bound(M, dyt.abs().sum(0)) + 2 * EPS * ref.abs(), "linear_bwd_dw_kernel db " + tag)
    # the same call from equal starts: the same bits
    for name, u, v in zip(("dx", "dW", "db"), (dx, dW, db), run()):
        assert torch.equal(_bits(u), _bits(v)), "two backward calls differ in " + name
    # NULL outputs leave the others what the full call makes them
    _, dW1, db1 = run(dx=False)
    assert torch.equal(_bits(dW1), _bits(dW)) and torch.equal(_bits(db1), _bits(db)), "dx == NULL"
    dx2, _, _ = run(dW=False, db=False)                      # (and x == NULL: nothing reads it)
    assert torch.equal(_bits(dx2), _bits(dx)), "dW == NULL, x == NULL"
    dx3, dW3, _ = run(db=False)
    assert torch.equal(_bits(dx3), _bits(dx)) and torch.equal(_bits(dW3), _bits(dW)), "db == NULL"
