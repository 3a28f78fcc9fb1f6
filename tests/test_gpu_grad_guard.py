"""Gradient guard on the device: the statistics kernel against float64 on the CPU (odd sizes, an unaligned start, more
than two sweeps of the grid), exact non-finite counts, bitwise reproducibility, the guarded Adadelta / Adam steps against
the unguarded ones, and the Trainer with the guard on (clipping, a skipped step, checkpoint / resume).

Bounds.  A lane of the statistics kernel adds at most ceil(n / (2048 * 256 * 4)) * 4 + 2 squares in fp32 (12 + 2 at the
largest n here), everything after that is double: the worst case is 14 * 2^-24 = 8.4e-7 relative on the sum of squares,
half of it on the norm -- inside the rtol 1e-5 the norm is held to.  Adam's lr_t is a device double pow against the host's
double pow, both rounded to float: the parameter DELTA is held to 2^-22 relative (of the largest delta)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWEEP = 2048 * 256 * 4                      # elements one sweep of the capped grid covers
BIG = 2 * SWEEP + 3 * 1024 + 777            # two sweeps, a ragged third one, a 16-byte body that is not whole, < 8M
SIZES = (1, 3, 255, 256, 257, 4099, BIG)
ADAM_BOUND = 2.0 ** -22


@pytest.fixture(scope="module")
def dev():
    from fvta_memexqa_amd import ops
    return ops.require_gpu()


@pytest.fixture(scope="module")
def base():
    """one random buffer every statistics test slices (host copy in float32); [1:] is 4 bytes past a 16-byte boundary"""
    rng = np.random.RandomState(7)
    return (rng.standard_normal(BIG + 1) * np.exp(rng.uniform(-6, 2, BIG + 1))).astype(np.float32)


def _expect(x, scale=1.0, clip=0.0):
    """float64 statistics of the float32 values the kernel forms"""
    g = x * np.float32(scale)
    if clip > 0:
        g = np.clip(g, np.float32(-clip), np.float32(clip))
    fin = np.isfinite(g)
    return (float(np.sqrt(np.sum(g[fin].astype(np.float64) ** 2))), float(np.abs(g[fin]).max()) if fin.any() else 0.0,
            int((~np.isfinite(x)).sum()))


def _guard(flat, ctl=None, **kw):
    from fvta_memexqa_amd import ops
    ctl = ctl if ctl is not None else ops.guard_ctl_new(flat.device)
    ops.grad_guard(flat, ctl, **kw)
    return ctl, ops.guard_ctl_read(ctl)


@pytest.mark.parametrize("n", SIZES)
def test_statistics_match_float64(dev, base, n):
    full = torch.from_numpy(base).to(dev)
    assert full.data_ptr() % 16 == 0
    for off in (0, 1):                                          # aligned, and 4 bytes past the boundary (head peel)
        flat, x = full[off:off + n], base[off:off + n]
        assert flat.data_ptr() % 16 == 4 * off
        _, c = _guard(flat, grad_scale=0.5, skip_nonfinite=True)
        norm, maxabs, _ = _expect(x, 0.5)
        print("n %d off %d: norm rel err %.3g" % (n, off, abs(c["norm"] - norm) / norm))
        np.testing.assert_allclose(c["norm"], norm, rtol=1e-5)
        assert np.float32(c["maxabs"]) == np.float32(maxabs)
        assert c["nonfinite"] == 0 and c["apply"] == 1 and c["factor"] == 1.0 and c["applied"] == 1 and c["skipped"] == 0
        assert c["grad_scale"] == 0.5
        # value clipping: the norm of the CLAMPED vector, and the global-norm factor on top of it
        clip = float(np.float32(0.25 * maxabs))
        normc, maxc, _ = _expect(x, 0.5, clip)
        _, c = _guard(flat, grad_scale=0.5, clip_value=clip, clip_norm=0.5 * normc)
        np.testing.assert_allclose(c["norm"], normc, rtol=1e-5)
        assert np.float32(c["maxabs"]) == np.float32(maxc) == np.float32(clip)
        cn = np.float32(0.5 * normc)
        assert np.float32(c["factor"]) == cn / max(np.float32(c["norm"]), cn)
        np.testing.assert_allclose(c["factor"], 0.5, rtol=1e-5)


@pytest.mark.parametrize("n", (4101, BIG))
def test_nonfinite_elements_are_counted_exactly(dev, base, n):
    from fvta_memexqa_amd import ops
    x = base[1:1 + n].copy()
    tail0 = 3 + (n - 3) // 4 * 4                                # flat[1:]: 3 head elements, then whole 16-byte loads
    assert tail0 < n - 1                                        # at least two tail elements: one inside, one last
    where = {0: np.nan, n - 1: np.inf, tail0: -np.inf, 2: np.inf, n // 2: np.nan, n // 3: -np.inf, n - 1025: np.nan}
    for i, v in where.items():
        x[i] = v
    full = torch.zeros(n + 1, device=dev)
    full[1:] = torch.from_numpy(x).to(dev)
    flat = full[1:]
    norm, maxabs, count = _expect(x)
    assert count == len(where)
    ctl, c = _guard(flat, skip_nonfinite=True)
    assert c["nonfinite"] == count and c["apply"] == 0 and (c["applied"], c["skipped"]) == (0, 1)
    assert np.float32(c["maxabs"]) == np.float32(maxabs)        # ignores them
    assert not np.isfinite(c["norm"])                           # not hidden
    _, c = _guard(flat, ctl, skip_nonfinite=False)              # off: counted, reported, applied
    assert c["nonfinite"] == count and c["apply"] == 1 and (c["applied"], c["skipped"]) == (1, 1)
    # only infinities, value clipping on: they clamp to +-c (finite), the count is still of the RAW buffer
    y = base[1:1 + n].copy()
    y[0], y[n - 1], y[tail0] = np.inf, -np.inf, np.inf
    full[1:] = torch.from_numpy(y).to(dev)
    normc, maxc, count = _expect(y, 1.0, 0.5)
    _, c = _guard(flat, clip_value=0.5, skip_nonfinite=True)
    assert count == 3 and c["nonfinite"] == 3 and c["apply"] == 0
    np.testing.assert_allclose(c["norm"], normc, rtol=1e-5)             # _expect clamps them the same way
    assert np.float32(c["maxabs"]) == np.float32(maxc) == np.float32(0.5)
    # a NaN survives the clamp
    y[5] = np.nan
    full[1:] = torch.from_numpy(y).to(dev)
    _, c = _guard(flat, clip_value=0.5, skip_nonfinite=True)
    assert c["nonfinite"] == 4 and np.isnan(c["norm"]) and c["apply"] == 0
    # a clean buffer whose squares overflow float32: nothing to count, the norm is not finite, the step is skipped
    z = torch.full((n,), 3e19, device=dev)
    _, c = _guard(z, skip_nonfinite=True)
    assert c["nonfinite"] == 0 and np.isinf(c["norm"]) and c["apply"] == 0 and c["maxabs"] == np.float32(3e19)


def test_two_calls_give_the_same_control_block_bit_for_bit(dev, base):
    from fvta_memexqa_amd import ops
    flat = torch.from_numpy(base).to(dev)[1:]
    ctl = ops.guard_ctl_new(dev, applied=41, skipped=2)
    kw = dict(grad_scale=0.25, clip_value=3.0, clip_norm=1.0, skip_nonfinite=True, adam=(1e-3, 0.9, 0.999))
    ops.grad_guard(flat, ctl, **kw)
    a = ctl.cpu().numpy().copy()
    ctl2 = ops.guard_ctl_new(dev, applied=41, skipped=2)
    ops.grad_guard(flat, ctl2, **kw)
    assert np.array_equal(a, ctl2.cpu().numpy())                                    # all 56 bytes
    ops.grad_guard(flat, ctl, **kw)
    b = ctl.cpu().numpy()
    assert np.array_equal(a[:12], b[:12]) and np.array_equal(a[16:40], b[16:40])    # all but lr_t and the counters
    ca, cb = ops.guard_ctl_read(ctl2), ops.guard_ctl_read(ctl)
    assert (ca["applied"], ca["skipped"]) == (42, 2) and (cb["applied"], cb["skipped"]) == (43, 2)
    lr, b1, b2 = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999))                # the ABI carries them as float
    want = lr * np.sqrt(1.0 - b2 ** 42) / (1.0 - b1 ** 42)
    assert abs(ca["lr_t"] - want) <= 2.0 ** -23 * want


def _state(dev, n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    var = torch.randn(n, generator=g).to(dev)
    grad = (torch.randn(n, generator=g) * 0.3).to(dev)
    s0 = (torch.rand(n, generator=g) * 0.01).to(dev)
    s1 = (torch.rand(n, generator=g) * 0.01).to(dev)
    return var, grad, s0, s1


def test_guarded_adadelta_is_the_unguarded_step_bit_for_bit(dev):
    from fvta_memexqa_amd import ops
    n = 4099
    var, grad, a, u = _state(dev, n, 1)
    rv, ra, ru = var.clone(), a.clone(), u.clone()
    ops.adadelta_step(rv, grad, ra, ru, 0.5, grad_scale=0.5)
    ctl, c = _guard(grad, grad_scale=0.5, clip_norm=1e30, skip_nonfinite=True)
    assert c["factor"] == 1.0 and c["apply"] == 1
    ops.adadelta_step_guarded(var, grad, a, u, ctl, 0.5)
    assert torch.equal(var, rv) and torch.equal(a, ra) and torch.equal(u, ru)
    # apply == 0: nothing is written
    grad[7] = float("nan")
    ctl, c = _guard(grad, ctl, grad_scale=0.5, skip_nonfinite=True)
    assert c["apply"] == 0
    ops.adadelta_step_guarded(var, grad, a, u, ctl, 0.5)
    assert torch.equal(var, rv) and torch.equal(a, ra) and torch.equal(u, ru)
    # the guard off: the NaN goes where it goes today, into that element alone
    ctl, c = _guard(grad, ctl, grad_scale=0.5)
    ops.adadelta_step_guarded(var, grad, a, u, ctl, 0.5)
    ops.adadelta_step(rv, grad, ra, ru, 0.5, grad_scale=0.5)
    assert torch.isnan(var[7]) and int(torch.isnan(var).sum()) == 1
    assert torch.equal(torch.nan_to_num(var), torch.nan_to_num(rv))


def test_guarded_adam_matches_the_unguarded_step(dev):
    from fvta_memexqa_amd import ops
    n, t = 4099, 5
    var, grad, m, v = _state(dev, n, 2)
    var0 = var.clone()
    rv, rm, rvv = var.clone(), m.clone(), v.clone()
    ops.adam_step(rv, grad, rm, rvv, t, 1e-3, grad_scale=0.5)
    ctl = ops.guard_ctl_new(dev, applied=t - 1)
    ctl, c = _guard(grad, ctl, grad_scale=0.5, clip_norm=1e30, skip_nonfinite=True, adam=(1e-3, 0.9, 0.999))
    assert c["factor"] == 1.0 and c["apply"] == 1 and c["applied"] == t
    ops.adam_step_guarded(var, grad, m, v, ctl)
    assert torch.equal(m, rm) and torch.equal(v, rvv)
    d, rd = (var - var0).double(), (rv - var0).double()
    err = float((d - rd).abs().max() / rd.abs().max())
    print("adam delta rel err %.3g" % err)
    assert err <= ADAM_BOUND
    keep = (var.clone(), m.clone(), v.clone())
    grad[n - 1] = float("inf")
    ctl, c = _guard(grad, ctl, grad_scale=0.5, skip_nonfinite=True, adam=(1e-3, 0.9, 0.999))
    assert c["apply"] == 0 and c["applied"] == t and c["skipped"] == 1
    ops.adam_step_guarded(var, grad, m, v, ctl)
    assert torch.equal(var, keep[0]) and torch.equal(m, keep[1]) and torch.equal(v, keep[2])


# ---------------------------------------------------------------------------------------------------------- Trainer
@pytest.fixture(scope="module")
def setup():
    from fvta_memexqa_amd.synth import SynthSpec, make_inputs, make_params
    spec = SynthSpec(N=4, A=1, P=3, S=2, L=5, d=20, dense=False, text_in=12, img_in=8)
    return spec, make_params(spec), make_inputs(spec)


def _fresh(setup, optimizer, **guard):
    from fvta_memexqa_amd.model_v2 import Model
    from fvta_memexqa_amd.trainer import Trainer
    spec, params, inputs = setup
    cfg = dict(spec.cfg(), batch_size=spec.N, init_lr=0.5 if optimizer == "adadelta" else 1e-3, optimizer=optimizer, **guard)
    m = Model(cfg, text_in=spec.text_in, img_in=spec.img_in)
    m.set_oracle_params(params)
    t = Trainer(m, cfg)
    return m, t, m.load_inputs(inputs, training=True)


def _fwd_bwd(m, t, L):
    m.zero_grad()
    m.forward(L)
    m.backward(L, loss_scale=1.0, need_dx=t.need_dx)


@pytest.mark.parametrize("optimizer", ["adadelta", "adam"])
def test_trainer_guard_below_every_threshold_changes_nothing(setup, optimizer):
    m1, t1, L1 = _fresh(setup, optimizer)
    m2, t2, L2 = _fresh(setup, optimizer, clip_global_norm=1e30, skip_nonfinite=True)
    assert not t1.guard_on and t2.guard_on
    start = m1.params.flat.clone()
    for _ in range(3):
        l1, l2 = t1.step_device(L1), t2.step_device(L2)
    st = t2.guard_stats()
    assert st["applied"] == 3 and st["skipped"] == 0 and st["factor"] == 1.0 and st["nonfinite"] == 0
    assert m1.global_step == m2.global_step == 3 and t1.guard_ctl is None and t2.guard_ctl is not None
    if optimizer == "adadelta":
        assert torch.equal(m1.params.flat, m2.params.flat) and torch.equal(l1, l2)
        for a, b in zip(t1.opt.state, t2.opt.state):
            assert torch.equal(a, b)
    else:
        assert t2.opt.t == 3
        d1, d2 = (m1.params.flat - start).double(), (m2.params.flat - start).double()
        err = float((d1 - d2).abs().max() / d1.abs().max())
        print("adam 3-step delta rel err %.3g" % err)
        assert err <= ADAM_BOUND


def test_trainer_clips_to_the_global_norm(setup):
    from fvta_memexqa_amd import ops
    m1, t1, L1 = _fresh(setup, "adadelta")
    _fwd_bwd(m1, t1, L1)                                           # the unguarded twin: the first step's gradient
    grad = m1.params.grad.clone()
    norm = float(np.sqrt(np.sum(grad.cpu().numpy().astype(np.float64) ** 2)))
    m2, t2, L2 = _fresh(setup, "adadelta", clip_global_norm=0.5 * norm)
    start = m2.params.flat.clone()
    t2.step_device(L2)
    st = t2.guard_stats()
    np.testing.assert_allclose(st["norm"], norm, rtol=1e-5)
    np.testing.assert_allclose(st["factor"], 0.5, rtol=1e-5)
    want, a, u = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
    ops.adadelta_step(want, grad, a, u, 0.5, grad_scale=0.5)
    d, wd = (m2.params.flat - start).double(), (want - start).double()
    err = float((d - wd).abs().max() / wd.abs().max())
    print("clipped step delta err %.3g of max |delta|" % err)
    assert err <= 1e-4
    # value clipping: the reference's commented-out tf.clip_by_value
    c = 0.25 * float(grad.abs().max())
    m3, t3, L3 = _fresh(setup, "adadelta", clip_gradient_value=c)
    t3.step_device(L3)
    st = t3.guard_stats()
    assert np.float32(st["maxabs"]) == np.float32(c) and st["factor"] == 1.0
    np.testing.assert_allclose(st["norm"], float(grad.clamp(-c, c).double().norm()), rtol=1e-5)


@pytest.mark.parametrize("optimizer", ["adadelta", "adam"])
def test_trainer_skips_a_nonfinite_step(setup, optimizer):
    m, t, L = _fresh(setup, optimizer, skip_nonfinite=True)
    start = m.params.flat.clone()
    _fwd_bwd(m, t, L)
    m.params.grad[7] = float("nan")                                # poison the gradient itself: no kernel is fed a NaN
    t.apply_update()
    st = t.guard_stats()
    assert (st["skipped"], st["applied"], st["nonfinite"]) == (1, 0, 1) and m.global_step == 1
    assert torch.equal(m.params.flat, start)
    for s in t.opt.state:
        assert int(torch.count_nonzero(s)) == 0                    # the slots: still the zeros they were created as
    t.step_device(L)                                               # a clean step applies
    st = t.guard_stats()
    assert (st["skipped"], st["applied"], st["nonfinite"]) == (1, 1, 0) and m.global_step == 2
    mr, tr, Lr = _fresh(setup, optimizer)                          # ... as an unguarded trainer's FIRST step
    tr.step_device(Lr)
    if optimizer == "adadelta":
        assert torch.equal(m.params.flat, mr.params.flat)
    else:
        assert t.opt.t == 1
        d, rd = (m.params.flat - start).double(), (mr.params.flat - start).double()
        assert float((d - rd).abs().max() / rd.abs().max()) <= ADAM_BOUND


@pytest.mark.parametrize("optimizer", ["adadelta", "adam"])
def test_trainer_checkpoint_carries_the_counters(setup, tmp_path, optimizer):
    guard = dict(clip_global_norm=1e30, skip_nonfinite=True)

    def applied_then_skipped(t, m, L):
        t.step_device(L)
        _fwd_bwd(m, t, L)
        m.params.grad[7] = float("nan")
        t.apply_update()
    m1, t1, L1 = _fresh(setup, optimizer, **guard)
    applied_then_skipped(t1, m1, L1)
    ref = [float(t1.step_device(L1)) for _ in range(2)]
    m2, t2, L2 = _fresh(setup, optimizer, **guard)
    applied_then_skipped(t2, m2, L2)
    t2.save(str(tmp_path))
    with np.load(str(tmp_path / "optimizer.npz")) as z:
        assert int(z["applied_steps"]) == 1 and int(z["skipped_steps"]) == 1
        assert optimizer == "adadelta" or int(z["step_count"]) == 1
    m3, t3, L3 = _fresh(setup, optimizer, **guard)
    assert t3.restore(str(tmp_path)) and m3.global_step == 2
    st = t3.guard_stats()
    assert (st["applied"], st["skipped"]) == (1, 1)
    got = [float(t3.step_device(L3)) for _ in range(2)]
    assert got == ref and torch.equal(m3.params.flat, m1.params.flat)
    st = t3.guard_stats()
    assert (st["applied"], st["skipped"]) == (3, 1) and m3.global_step == 4
    # a checkpoint of an unguarded run (no counters in the file) restores as before, into either kind of trainer
    m4, t4, L4 = _fresh(setup, optimizer)
    t4.step_device(L4)
    t4.save(str(tmp_path / "plain"))
    with np.load(str(tmp_path / "plain" / "optimizer.npz")) as z:
        assert "applied_steps" not in z.files
    m5, t5, L5 = _fresh(setup, optimizer, **guard)
    assert t5.restore(str(tmp_path / "plain"))
    st = t5.guard_stats()
    assert st["skipped"] == 0 and st["applied"] == (1 if optimizer == "adam" else 0)
