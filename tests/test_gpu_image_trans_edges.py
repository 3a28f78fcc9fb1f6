"""fvta_image_trans_fwd / _bwd (csrc/image_trans.hip) through ops.ImageTrans at the edges of its kernels: the matrix-pipe
pair img_fwd_mfma / img_dw_mfma (16-row tiles, chunks of 16 k dealt to 8 waves, the second column group from tdim 64 on,
more than one round of the step loop for only some waves), the generic 32 x 32 pair img_fwd_kernel / img_dw_kernel, the
launcher's fallback to the generic pair when W or the workspace is off the 16-byte grid, and the plain gather.

Every case scatters its rows to a shuffled, unevenly spaced row_off inside a sentinel-filled x, reads the photos from a
view inside a larger buffer whose guard rows and unlisted photos are NaN, and accumulates dW / db onto random starts.

Bound (derived, see tests/test_gpu_linear_edges.py): (K + 16) 2^-24 (sum_k |a_k| |b_k| + |bias|) per element in fp64, K = idim
forward and K = M for dW and db, + 1e-5 behind the tanh, + 2^-23 |start + sum| for the addition onto the start.  The backward
reference takes the kernel's own fp32 rows as given: dpre = dx (1 - y^2) is formed from them in fp64.  The forward reference
is oracle.fvta_fused.image_features in fp64."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENT = -7777.25

# (VI, idim, tdim, M)
MFMA = [(40, 1, 4, 1), (40, 3, 60, 15), (40, 16, 64, 16), (40, 17, 68, 17), (40, 127, 100, 129), (40, 128, 124, 131),
        (40, 129, 128, 259)]
GENERIC = [(40, 61, 1, 33), (40, 33, 30, 65), (40, 64, 33, 32), (40, 70, 130, 40), (40, 50, 132, 20)]
FALLBACK = (40, 129, 100, 131)
# (shape, variant): "" as listed; "W+4" W one float past a 16-byte boundary; "work+4" the workspace so; "same" one photo only
CASES = [(s, "") for s in MFMA + GENERIC] + [(FALLBACK, "W+4"), (FALLBACK, "work+4"), ((40, 17, 68, 17), "same")]
IDS = ["%dx%dx%dx%d%s" % (s + (("-" + v) if v else "",)) for s, v in CASES]
GATHER = [(40, 33, 33, 65), (40, 1, 1, 3)]


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


def _off_grid(t):
    """a copy of t on the device that starts one float past a 16-byte boundary of a larger buffer"""
    buf = torch.zeros(t.numel() + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _case(VI, idim, tdim, M, same=False, trans=True):
    """CPU inputs: the photo list holds 0, VI - 1 and one photo five times (as far as M entries hold them), shuffled;
    row r goes to [off[r], off[r] + tdim) of x, the slots shuffled and 0..8 floats apart, behind a lead of 3 floats"""
    g = torch.Generator().manual_seed(31 * idim + 7 * tdim + M + (1000 if same else 0))
    ri = lambda hi, n: torch.randint(0, hi, (n,), generator=g)
    five = 1 + int(ri(VI - 2, 1))
    lst = ([0, VI - 1] + [five] * 5 + ri(VI, max(M - 7, 0)).tolist())[:M]
    pidx = torch.tensor(lst, dtype=torch.int32)[torch.randperm(M, generator=g)]
    if same:
        pidx = torch.full((M,), five, dtype=torch.int32)
    nd = tdim if trans else idim
    size = nd + ri(9, M)
    start = 3 + torch.cumsum(size, 0) - size
    row_off = start[torch.randperm(M, generator=g)].to(torch.int64)
    nx = int(3 + size.sum()) + 5
    inside = torch.zeros(nx, dtype=torch.bool)
    cols = (row_off[:, None] + torch.arange(nd)[None, :]).reshape(-1)
    inside[cols] = True
    assert int(inside.sum()) == M * nd                       # the rows do not overlap
    feat = torch.randn(VI, idim, generator=g)
    listed = torch.zeros(VI, dtype=torch.bool)
    listed[pidx.long()] = True
    feat[~listed] = float("nan")
    c = dict(VI=VI, idim=idim, tdim=tdim, M=M, pidx=pidx, row_off=row_off, nx=nx, inside=inside, cols=cols, feat=feat)
    if trans:
        c.update(W=torch.randn(idim, tdim, generator=g) * 0.1, b=torch.randn(tdim, generator=g) * 0.1,
                 gout=torch.randn(M, tdim, generator=g), dW0=torch.randn(idim, tdim, generator=g),
                 db0=torch.randn(tdim, generator=g))
    return c


def _device_feat(c):
    """the photo table as a view inside a larger buffer with two NaN guard rows on each side"""
    buf = torch.full((c["VI"] + 4, c["idim"]), float("nan"))
    buf[2:2 + c["VI"]] = c["feat"]
    return buf.cuda()[2:2 + c["VI"]]


@pytest.mark.parametrize("tanh", [False, True], ids=["linear", "tanh"])
@pytest.mark.parametrize("shape,variant", CASES, ids=IDS)
def test_transform_forward_backward(shape, variant, tanh):
    from fvta_memexqa_amd import ops
    from oracle import fvta_fused as F
    VI, idim, tdim, M = shape
    c = _case(*shape, same=variant == "same")
    on_pipe = tdim % 4 == 0 and tdim <= 128 and not variant.endswith("+4")
    kf, kw = ("img_fwd_mfma", "img_dw_mfma") if on_pipe else ("img_fwd_kernel", "img_dw_kernel")
    tag = " %s%s tanh=%d" % (shape, variant, tanh)
    feat, pidx, row_off = _device_feat(c), c["pidx"].cuda(), c["row_off"].cuda()
    W = _off_grid(c["W"]) if variant == "W+4" else c["W"].cuda()
    b = c["b"].cuda()
    op = ops.ImageTrans(M, idim, tdim, tanh)
    if variant == "work+4":
        op.work = _off_grid(op.work)
    # forward into a sentinel-filled x
    x = torch.full((c["nx"],), SENT, device="cuda")
    op.forward(pidx, row_off, feat, W, b, x)
    rows64 = c["feat"][c["pidx"].long()].double()
    W64, b64 = c["W"].double(), c["b"].double()
    ref = F.image_features(c["pidx"], c["feat"].double(), W64, b64, tanh)
    bound = (idim + 16) * EPS * (rows64.abs() @ W64.abs() + b64.abs()) + (1e-5 if tanh else 0.0)
    xc = x.cpu()
    _check(xc[c["cols"]].view(M, tdim), ref, bound, kf + " x" + tag)
    assert torch.equal(_bits(xc[~c["inside"]]), _bits(torch.full_like(xc[~c["inside"]], SENT))), "x outside the rows changed"
    # backward: x and dx are NaN outside the rows, dW and db start from random buffers
    xn = torch.full((c["nx"],), float("nan"), device="cuda")
    op.forward(pidx, row_off, feat, W, b, xn)
    assert torch.equal(_bits(xn.cpu()[c["cols"]]), _bits(xc[c["cols"]])), "two forward calls differ"
    dx = torch.full((c["nx"],), float("nan"))
    dx[c["cols"]] = c["gout"].reshape(-1)
    dx = dx.cuda()

    def run():
        dW, db = c["dW0"].cuda(), c["db0"].cuda()
        op.backward(pidx, row_off, feat, xn, dx, dW, db)
        return dW, db

    dW, db = run()
    y64 = xc[c["cols"]].view(M, tdim).double()
    dpre = c["gout"].double() * (1 - y64 * y64) if tanh else c["gout"].double()
    ref = c["dW0"].double() + rows64.t() @ dpre
    _check(dW, ref, (M + 16) * EPS * (rows64.abs().t() @ dpre.abs()) + 2 * EPS * ref.abs(), kw + " dW" + tag)
    ref = c["db0"].double() + dpre.sum(0)
    _check(db, ref, (M + 16) * EPS * dpre.abs().sum(0) + 2 * EPS * ref.abs(), kw + " db" + tag)
    dW2, db2 = run()                                          # the waves combine in wave order: the same bits
    assert torch.equal(_bits(dW), _bits(dW2)) and torch.equal(_bits(db), _bits(db2)), "two backward calls differ"


@pytest.mark.parametrize("shape", GATHER, ids=["%dx%dx%dx%d" % s for s in GATHER])
def test_plain_gather(shape):
    """no transform (W == NULL): the rows are the listed photos' rows, bit for bit, and nothing else is written"""
    from fvta_memexqa_amd import ops
    VI, idim, tdim, M = shape
    c = _case(*shape, trans=False)
    x = torch.full((c["nx"],), SENT, device="cuda")
    ops.ImageTrans(M, idim, tdim, False).forward(c["pidx"].cuda(), c["row_off"].cuda(), _device_feat(c), None, None, x)
    xc = x.cpu()
    assert torch.equal(xc[c["cols"]].view(M, idim), c["feat"][c["pidx"].long()])
    assert torch.equal(_bits(xc[~c["inside"]]), _bits(torch.full_like(xc[~c["inside"]], SENT))), "x outside the rows changed"
