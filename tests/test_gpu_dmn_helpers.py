"""autograd.dmn_features (fvta_dmn_features / _bwd) and autograd.relu (fvta_relu_fwd / _bwd) past one round of their
256-thread loops: d (n) on both sides of 256, a third round (d = 600), a second grid row, more than 256 workgroups.

dmn_features' forward is one rounded product or one rounded difference per output: it equals the same formula in fp32 on
the CPU bit for bit.  Its backward is checked against fp64 autograd with the derived bound of
tests/test_gpu_linear_edges.py, (K + 16) 2^-24 sum_k |a_k| |b_k| per element: K = 4 for d_facts (four products), K = 2 F for
d_q and d_m (two products per fact), accumulated onto the fresh zero buffers _DmnFeatures makes.  A few facts are set
exactly equal to q or m: |x| has derivative 0 at 0 (the kernel's comment; torch.abs agrees)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _check(got, ref, bound, what):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), what + ": not finite"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    print("%s: worst |got - ref| / bound = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst |got - ref| / bound = %.4f" % (what, worst)


def _features(facts, q, m):
    qq, mm = q[:, None, :], m[:, None, :]
    return torch.cat([facts * qq, facts * mm, (facts - qq).abs(), (facts - mm).abs()], -1)


@pytest.mark.parametrize("F", [1, 11])
@pytest.mark.parametrize("d", [255, 256, 257, 600])
def test_dmn_features_forward_backward(d, F):
    from fvta_memexqa_amd import autograd
    N = 3
    g = torch.Generator().manual_seed(100 * d + F)
    facts, q, m = torch.randn(N, F, d, generator=g), torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    gout = torch.randn(N, F, 4 * d, generator=g)
    facts[0, 0, 0] = q[0, 0]                                  # ties: |fact - q| or |fact - m| is exactly 0
    facts[1, 0, d // 2] = q[1, d // 2]
    facts[2, F - 1, d - 1] = m[2, d - 1]
    facts[1, F - 1, 255 % d] = m[1, 255 % d]
    q[2, 3] = m[2, 3]
    facts[2, 0, 3] = q[2, 3]                                  # both at once
    leaves = [t.cuda().requires_grad_() for t in (facts, q, m)]
    out = autograd.dmn_features(*leaves)
    assert tuple(out.shape) == (N, F, 4 * d)
    assert torch.equal(out.detach().cpu(), _features(facts, q, m)), "forward"
    out.backward(gout.cuda())
    l64 = [t.double().requires_grad_() for t in (facts, q, m)]
    _features(*l64).backward(gout.double())
    f64, q64, m64 = (t.detach() for t in l64)
    qq, mm = q64[:, None, :], m64[:, None, :]
    g1, g2, g3, g4 = (t.abs() for t in gout.double().split(d, -1))
    tq, tm = (f64 != qq).double(), (f64 != mm).double()       # |sgn|
    tag = " d=%d F=%d" % (d, F)
    _check(leaves[0].grad, l64[0].grad, (4 + 16) * EPS * (g1 * qq.abs() + g2 * mm.abs() + g3 * tq + g4 * tm),
           "dmn_features_bwd_kernel d_facts" + tag)
    _check(leaves[1].grad, l64[1].grad, (2 * F + 16) * EPS * (g1 * f64.abs() + g3 * tq).sum(1), "dmn_features_bwd_kernel d_q" + tag)
    _check(leaves[2].grad, l64[2].grad, (2 * F + 16) * EPS * (g2 * f64.abs() + g4 * tm).sum(1), "dmn_features_bwd_kernel d_m" + tag)


@pytest.mark.parametrize("n", [255, 256, 257, 65537])
def test_relu_forward_backward(n):
    from fvta_memexqa_amd import autograd
    g = torch.Generator().manual_seed(n)
    x, gout = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x[0], x[n - 1], x[n // 2], x[n // 3] = 0.0, -0.0, 0.0, 1e-30
    xd = x.cuda().requires_grad_()
    y = autograd.relu(xd)
    assert torch.equal(y.detach().cpu(), torch.relu(x))
    y.backward(gout.cuda())
    assert torch.equal(xd.grad.cpu(), gout * (x > 0))
