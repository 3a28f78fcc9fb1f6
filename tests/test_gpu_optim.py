"""GPU parity of the l2 terms (fvta_weight_decay) and of the Adadelta / Adam updates (csrc/optim.hip) against float64:
the sizes where the one-workgroup stride of weight_decay_kernel and the 256-thread grid of the update kernels turn over,
25 consecutive steps on one state from a zero and from a warm start, exactly zero gradients, and grad_scale != 1.

Tolerance of the optimizer steps, measured against the reference and never against the kernel: E32 is the max abs
difference, per tensor, between oracle.fvta_literal's step function run on float32 arrays and run in float64; a kernel
element may be off by 1e-4 * |ref| + max(8 * E32, 2^-23 * max|ref|).  It is relative to each tensor's own scale so that
the about-1e-7 accum_update of a zero start is actually checked.  The hyper-parameters reach the kernels as C floats, so
the oracle is given their float32 values (1 - 0.999f is 4.7e-5 away from 0.001).

Every test prints `max err / allowed` per tensor (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4
f32 = lambda x: float(np.float32(x))


# ---------------------------------------------------------------------------------------------------- weight decay
# one workgroup of 1024 threads striding by 1024; the last size is the order of the largest real slice
WD_SIZES = [1, 1023, 1024, 1025, 5000, 3 * 2 ** 20 + 1]
COEF = f32(0.002 * 7)                                        # wd * the char-CNN multiplier


@functools.lru_cache(maxsize=None)
def _wd_reference(n):
    g = torch.Generator().manual_seed(4000 + n % 9973)
    var = (torch.randn(n, generator=g) * 0.1).numpy()
    pre_grad = torch.randn(n, generator=g).numpy()
    inc = 0.5 * COEF * float(np.sum(var.astype(np.float64) ** 2))
    # grad and loss start from non-zero values because the kernel adds; the loss starts at about half of what is added,
    # so that the float32 `+=` keeps the increment visible to within an ulp of it
    pre_loss = np.float32(0.5 * 0.5 * COEF * n * 0.01)
    ref_grad = pre_grad.astype(np.float64) + COEF * var.astype(np.float64)
    ref_loss = float(pre_loss) + inc
    # float32 emulation of the kernel's order: 1024 strided partial sums, then a halving tree, then 0.5f * coef * sum
    pad = np.zeros((n + 1023) // 1024 * 1024, np.float32)
    pad[:n] = var
    acc = np.zeros(1024, np.float32)
    for row in pad.reshape(-1, 1024):
        acc = acc + row * row
    st = 512
    while st > 0:
        acc[:st] = acc[:st] + acc[st:2 * st]
        st >>= 1
    inc32 = np.float32(0.5) * np.float32(COEF) * acc[0]
    e32 = abs(float(inc32) - inc)
    for a in (var, pre_grad):
        a.setflags(write=False)
    return dict(var=var, pre_grad=pre_grad, pre_loss=pre_loss, ref_grad=ref_grad, ref_loss=ref_loss, inc=inc, e32=e32)


@pytest.mark.parametrize("mode", ["grad", "loss", "both"])
@pytest.mark.parametrize("n", WD_SIZES)
def test_weight_decay_matches_float64(n, mode):
    from fvta_memexqa_amd import ops
    R = _wd_reference(n)
    var = torch.from_numpy(R["var"].copy()).cuda()
    var0 = var.clone()
    outs = []
    for _ in range(2):
        grad = torch.from_numpy(R["pre_grad"].copy()).cuda()
        loss = torch.full((1,), float(R["pre_loss"]), device="cuda")
        ops.weight_decay(var, grad if mode != "loss" else None, COEF, loss if mode != "grad" else None)
        outs.append((grad, loss))
    assert torch.equal(var, var0)                                  # var is read only
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # one fixed order
    grad, loss = outs[0]
    report = []
    if mode == "loss":                                             # grad=None leaves the gradient buffer alone
        assert np.array_equal(grad.cpu().numpy(), R["pre_grad"])
    else:
        # rtol 1e-6 plus one ulp of the tensor's scale: the compiler may or may not fuse the multiply-add, both are right
        allowed = 1e-6 * np.abs(R["ref_grad"]) + 2.0 ** -23 * np.abs(R["ref_grad"]).max()
        err = np.abs(grad.cpu().numpy().astype(np.float64) - R["ref_grad"])
        report.append(("grad", float((err / allowed).max())))
    if mode == "grad":                                             # loss=None leaves the loss alone
        assert loss.item() == float(R["pre_loss"])
    else:
        # the increment within 8 * E32 of its float64 value, E32 from the emulation of the kernel's order; and, because
        # the kernel adds it to the running loss in float32 (fused with the last multiply or not), one ulp of that sum
        assert 8 * R["e32"] <= 0.1 * RTOL * R["inc"], (R["e32"], R["inc"])   # about 1e-7 relative: hides nothing
        allowed = 8 * R["e32"] + 2.0 ** -23 * abs(R["ref_loss"])
        err = abs(float(loss.cpu().double()) - R["ref_loss"])
        report.append(("loss", err / allowed))
        assert abs(float(loss.cpu().double()) - float(R["pre_loss"])) > 0.5 * R["inc"]     # added to what was there
    print("\n[weight_decay n=%d %s] max err / allowed: %s" % (n, mode, "  ".join("%s %.3g" % r for r in report)))
    for k, r in report:
        assert r <= 1.0, "%s: max err / allowed = %.3g" % (k, r)


# ------------------------------------------------------------------------------------------------ optimizer steps
OPT_SIZES = [1, 255, 256, 257, 4099]                # 256 threads per block: one thread, a block less / plus one, many
STEPS = 25
ADADELTA = dict(lr=f32(0.5), rho=f32(0.95), eps=f32(1e-8))
ADAM = dict(lr=f32(0.001), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))


def _grads(rng, n, steps):
    """Fresh gradients every step, mixed magnitudes 1e-4 .. 1 per element; fifty elements are exactly zero in step 2
    (every element when n < 50), and where n > 5 the last five also in step 1, when a zero start has nothing but eps
    under the square roots."""
    out = []
    for s in range(steps):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 1, n)).astype(np.float32)
        if s == 1:
            g[rng.permutation(n)[:50]] = 0.0
        if s == 0 and n > 5:
            g[-5:] = 0.0
        out.append(g)
    return out


def _state(rng, n, kind, warm):
    var = rng.standard_normal(n).astype(np.float32)
    if not warm:
        return [var, np.zeros(n, np.float32), np.zeros(n, np.float32)]
    a, b = rng.standard_normal(n).astype(np.float32), np.abs(rng.standard_normal(n)).astype(np.float32)
    if kind == "adadelta":
        return [var, np.abs(a), b * np.float32(0.01)]
    return [var, a * np.float32(0.1), b * np.float32(0.1)]


def _oracle_step(kind, state, grad, t):
    from oracle import fvta_literal as L
    if kind == "adadelta":
        return L.adadelta_step(state[0], grad, state[1], state[2], ADADELTA["lr"], ADADELTA["rho"], ADADELTA["eps"])
    return L.adam_step(state[0], grad, state[1], state[2], t, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"])


def _run_oracle(kind, state, grads, grad_scale, ts, dtype):
    """The oracle on `dtype` arrays, fed grad * grad_scale; the state after the first and after the last step."""
    st = [a.astype(dtype) for a in state]
    first = None
    for g, t in zip(grads, ts):
        st = list(_oracle_step(kind, st, g.astype(dtype) * dtype(grad_scale), t))
        assert all(a.dtype == dtype for a in st)
        if first is None:
            first = [a.copy() for a in st]
    return first, st


def _kernel_step(kind, dev, grad, grad_scale, t):
    from fvta_memexqa_amd import ops
    if kind == "adadelta":
        ops.adadelta_step(dev[0], grad, dev[1], dev[2], grad_scale=grad_scale, **ADADELTA)
    else:
        ops.adam_step(dev[0], grad, dev[1], dev[2], t, grad_scale=grad_scale, **ADAM)


def _compare(tag, kind, got, ref64, ref32):
    names = ("var", "accum", "accum_update") if kind == "adadelta" else ("var", "m", "v")
    report = []
    for k, a, r, r32 in zip(names, got, ref64, ref32):
        e32 = float(np.abs(r32.astype(np.float64) - r).max())
        top = float(np.abs(r).max())
        assert 8 * e32 <= RTOL * top or top == 0.0, (tag, k, e32, top)      # the measured part hides nothing
        allowed = RTOL * np.abs(r) + max(8 * e32, 2.0 ** -23 * top)
        err = np.abs(a.cpu().numpy().astype(np.float64) - r)
        assert np.isfinite(err).all(), (tag, k)
        ratio = np.where(err == 0, 0.0, err / np.where(allowed == 0, 1e-300, allowed))
        report.append((k, float(ratio.max())))
    print("\n[%s] max err / allowed: %s" % (tag, "  ".join("%s %.3g" % r for r in report)))
    for k, r in report:
        assert r <= 1.0, "%s %s: max err / allowed = %.3g" % (tag, k, r)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("warm", [False, True], ids=["zero", "warm"])
@pytest.mark.parametrize("n", OPT_SIZES)
@pytest.mark.parametrize("kind", ["adadelta", "adam"])
def test_optimizer_25_steps_match_oracle(kind, n, warm, grad_scale):
    rng = np.random.default_rng(100 + n + 7 * warm + (0 if kind == "adam" else 50))
    state = _state(rng, n, kind, warm)
    grads = _grads(rng, n, STEPS)
    ts = list(range(1, STEPS + 1))
    first64, last64 = _run_oracle(kind, state, grads, grad_scale, ts, np.float64)
    first32, last32 = _run_oracle(kind, state, grads, grad_scale, ts, np.float32)
    dev = [torch.from_numpy(a.copy()).cuda() for a in state]
    tag = "%s n=%d %s gs=%g" % (kind, n, "warm" if warm else "zero", grad_scale)
    for g, t in zip(grads, ts):
        _kernel_step(kind, dev, torch.from_numpy(g).cuda(), grad_scale, t)
        if t == 1:
            _compare(tag + " step 1", kind, dev, first64, first32)
    _compare(tag + " step %d" % STEPS, kind, dev, last64, last32)


@pytest.mark.parametrize("n", OPT_SIZES)
def test_adam_single_step_at_t_10000(n):
    """The bias correction lr * sqrt(1 - b2^t) / (1 - b1^t), computed in double on the host, far from t = 1."""
    rng = np.random.default_rng(900 + n)
    state = _state(rng, n, "adam", True)
    grads = _grads(rng, n, 1)
    _, last64 = _run_oracle("adam", state, grads, 1.0, [10000], np.float64)
    _, last32 = _run_oracle("adam", state, grads, 1.0, [10000], np.float32)
    dev = [torch.from_numpy(a.copy()).cuda() for a in state]
    _kernel_step("adam", dev, torch.from_numpy(grads[0]).cuda(), 1.0, 10000)
    _compare("adam n=%d t=10000" % n, "adam", dev, last64, last32)
