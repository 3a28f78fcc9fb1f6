"""GPU parity of the answer scorer and its softmax cross-entropy (csrc/scorer.hip) where their loops turn over: the
four-rows-per-round loop of scorer_bwd_params_kernel, its generic-C loop, the inline dlogit_of path past SCORER_DL_MAX,
the `ch += 256` / `n += 256` strides, a partly filled 64-channel block, loss_scale != 1 and multi-hot labels.

Reference: oracle.fvta_fused.scorer + softmax_cross_entropy_mean in float64, gradients by autograd.

Tolerance, measured against the reference and never against the kernel: E32 is the max abs difference, per tensor,
between the oracle run on float32 copies of the inputs and the oracle run in float64; a kernel element may be off by
    1e-4 * |ref| + max(8 * E32, 2^-23 * max|ref|)
(1e-4 is the project's rtol; 8 because the kernels sum sequentially per thread where torch sums pairwise, and the
device expf / tanhf are allowed a couple of ulp).  So that this cannot hide anything, every tensor except db must have
8 * E32 <= 1e-4 * max|ref|.  db is about 0 with one-hot labels in TF mode, so its own scale is useless: it is bound by
2^-19 * sum|d logits_ref| (loss_scale included; d logits = the gradient at the linear output, the terms the kernel
sums): each thread adds at most 17 terms and the tree has 8 levels = at most 25 roundings of 2^-24 on the absolute sum,
and a few ulp per d logit come on top.

Every test prints `max err / allowed` per tensor (pytest -s)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4
NAMES = ("logits", "yp", "loss", "dgq", "dg1", "dgch", "dW", "db")

# (N, C, w, use_eu_output, add_tanh, weight scale, the tf_xent_grad values to run)
CASES = {
    # group 0 takes one unrolled round, groups 1-3 none (n+12 < N holds for n=0 only); w=100: a partly filled second
    # 64-channel block (the ch < w guard) and idle lanes in the forward
    "13x4x100": (13, 4, 100, False, False, 0.1, (True, False)),
    # every group takes two unrolled rounds, the remainder loop runs for groups 0-2 and is empty for group 3; w=320: two
    # trips of ch += 256, the second partial; loss_scale 0.25
    "35x4x320": (35, 4, 320, True, True, 0.1, (True, False)),
    # the headline's own scorer shape: three unrolled rounds plus the remainder loop, four full trips of ch += 256
    "64x4x1024": (64, 4, 1024, False, False, 0.1, (True, False)),
    # C != 4: the generic loop, N past the point where the unrolled loop would have been taken
    "20x5x70": (20, 5, 70, True, False, 0.1, (True, False)),
    "18x3x64": (18, 3, 64, False, False, 0.1, (True, False)),
    # C = 64: the limit of s_logit[64] / s_dl[64]
    "3x64x40": (3, 64, 40, True, False, 0.1, (True, False)),
    # C = 1: yp is exactly 1
    "9x1x33": (9, 1, 33, False, False, 0.1, (True, False)),
    # the n += 256 turn-over of ce_loss_kernel, with a partial second trip
    "300x4x64": (300, 4, 64, False, False, 0.1, (False,)),
    # N*C = 4096 is the last shape whose d logits are cached in LDS, 4100 the first uncached one: the inline dlogit_of
    # then carries its tanh factor in both the dW and the db path
    "1024x4x64": (1024, 4, 64, True, True, 0.1, (True, False)),
    "1025x4x64": (1025, 4, 64, True, True, 0.1, (True, False)),
    # uncached and generic C together
    "820x5x64": (820, 5, 64, False, False, 0.1, (True, False)),
    # saturated softmax: max|logit| about 100, some yp exactly 1; the max-subtraction in the forward and in
    # ce_loss_kernel is what keeps this finite
    "33x4x192_sat": (33, 4, 192, False, False, 3.0, (True, False)),
}
PARAMS = [(k, tf) for k, c in CASES.items() for tf in c[6]]
IDS = ["%s-%s" % (k, "tf" if tf else "math") for k, tf in PARAMS]


def _loss_scale(name):
    N = CASES[name][0]
    # N >= 300: the oracle backpropagates loss * N, which keeps the gradients O(0.1) so that the tolerance means something
    return float(N) if N >= 300 else (0.25 if name == "35x4x320" else 1.0)


def _npad(N):
    # the padded rows of a short last batch (labels all False): three where N >= 13, else one as in the older tests
    return 3 if N >= 13 else 1


def _oracle(inp, y, eu, tanh, tf_grad, loss_scale, dtype):
    from oracle import fvta_fused as F
    leaves = [t.to(dtype).clone().requires_grad_() for t in inp]
    logits, yp = F.scorer(*leaves, eu, tanh)
    logits.retain_grad()
    loss = F.softmax_cross_entropy_mean(logits, y, tf_grad=tf_grad)
    (loss * loss_scale).backward()
    dl = logits.grad
    if eu and tanh:                                   # back through the tanh: the gradient at the linear output
        dl = dl * (1 - logits.detach() ** 2)
    out = dict(logits=logits.detach(), yp=yp.detach(), loss=loss.detach().reshape(1), dgq=leaves[0].grad,
               dg1=leaves[1].grad, dgch=leaves[2].grad, dW=leaves[3].grad.reshape(-1), db=leaves[4].grad)
    return out, dl


@functools.lru_cache(maxsize=None)
def _reference(name, tf_grad):
    """Inputs, labels, the float64 oracle and the allowed error per tensor; computed once, shared and left unchanged."""
    N, C, w, eu, tanh, wscale, _ = CASES[name]
    g = torch.Generator().manual_seed(7 + 131 * N + 17 * C + w)
    gq = torch.randn(N, w, generator=g) * 0.5
    g1 = torch.randn(N, w, generator=g) * 0.5
    gch = torch.randn(N, C, w, generator=g) * 0.5
    W = torch.randn((7 if eu else 5) * w, 1, generator=g) * wscale
    b = torch.randn(1, generator=g) * 0.1
    live = N - _npad(N)
    y = torch.zeros(N, C, dtype=torch.bool)
    lab = torch.randint(0, C, (live,), generator=g)
    y[torch.arange(live), lab] = True
    if C > 1:                                         # one multi-hot row (two labels): makes ysum observable when
        y[1, (int(lab[1]) + 1) % C] = True            # tf_grad is False; a C = 1 row cannot have two
    inp = (gq, g1, gch, W, b)
    ls = _loss_scale(name)
    ref, dl = _oracle(inp, y, eu, tanh, tf_grad, ls, torch.float64)
    r32, _ = _oracle(inp, y, eu, tanh, tf_grad, ls, torch.float32)
    allowed, e32 = {}, {}
    for k in NAMES:
        e32[k] = float((r32[k].double() - ref[k]).abs().max())
        top = float(ref[k].abs().max())
        if k == "db":
            allowed[k] = torch.full_like(ref[k], 2.0 ** -19 * float(dl.abs().sum()))
            continue
        # the tolerance may not hide anything: the measured part stays below the rtol of the tensor's own scale
        assert 8 * e32[k] <= RTOL * top, (name, k, e32[k], top)
        allowed[k] = RTOL * ref[k].abs() + max(8 * e32[k], 2.0 ** -23 * top)
    return dict(inp=inp, y=y, ref=ref, allowed=allowed, e32=e32, loss_scale=ls)


def _check(tag, got, R, names):
    worst = {}
    for k in names:
        err = (got[k].detach().cpu().double().reshape(R["ref"][k].shape) - R["ref"][k]).abs()
        assert torch.isfinite(err).all(), (tag, k)
        ratio = err / R["allowed"][k]
        ratio[err == 0] = 0.0                         # 0 / 0: an exact zero where zero is expected
        worst[k] = float(ratio.max())
    print("\n[%s] max err / allowed: %s" % (tag, "  ".join("%s %.3g" % (k, worst[k]) for k in names)))
    for k in names:
        assert worst[k] <= 1.0, "%s %s: max err / allowed = %.3g (E32 %.3g)" % (tag, k, worst[k], R["e32"][k])


def _dev(R):
    f = lambda t: t.float().cuda().contiguous()
    gq, g1, gch, W, b = R["inp"]
    return f(gq), f(g1), f(gch), f(W).reshape(-1), f(b)


def _forward(name, R):
    from fvta_memexqa_amd import ops
    _, _, _, eu, tanh, _, _ = CASES[name]
    yd = ops.as_mask_u8(R["y"]).cuda()
    d = _dev(R)
    logits, yp, loss = ops.scorer_ce_fwd(*d, yd, eu, tanh)
    return d, yd, logits, yp, loss


@pytest.mark.parametrize("name,tf_grad", PARAMS, ids=IDS)
def test_scorer_ce_matches_oracle(name, tf_grad):
    from fvta_memexqa_amd import ops
    N, C, w, eu, tanh, _, _ = CASES[name]
    R = _reference(name, tf_grad)
    d, yd, logits, yp, loss = _forward(name, R)
    dW = torch.zeros(d[3].numel(), device="cuda")
    db = torch.zeros(1, device="cuda")
    dgq, dg1, dgch = ops.scorer_ce_bwd(*d, yd, logits, yp, R["loss_scale"], dW, db, eu, tanh, tf_xent_grad=tf_grad)
    got = dict(logits=logits, yp=yp, loss=loss, dgq=dgq, dg1=dg1, dgch=dgch, dW=dW, db=db)
    _check("%s %s" % (name, "tf" if tf_grad else "math"), got, R, NAMES)
    assert (yp.argmax(1).cpu() == R["ref"]["yp"].argmax(1)).all()
    rows = (yp.cpu().double().sum(1) - 1.0).abs()      # each row of yp sums to 1 within its elements' tolerance
    assert (rows <= R["allowed"]["yp"].sum(1)).all(), float(rows.max())
    if C == 1:
        assert (yp == 1.0).all()
    if name == "33x4x192_sat":
        assert float(R["ref"]["logits"].abs().max()) > 50 and (yp == 1.0).any()
    # the padded rows: softmax/N through the scorer with TF's gradient, nothing with the mathematical one
    for n in range(N - _npad(N), N):
        assert (dgch[n].abs().max().item() > 0) == tf_grad, n


@pytest.mark.parametrize("name", ["35x4x320", "1025x4x64"])
def test_scorer_bwd_is_repeatable_and_adds_once(name):
    """The kernel's claim of a fixed summation order and a single add into dW / db: two runs from zero are bitwise equal,
    and a run into pre-filled dW / db is prefill + (the run from zero), formed in float32 on the device, bitwise."""
    from fvta_memexqa_amd import ops
    _, _, _, eu, tanh, _, _ = CASES[name]
    R = _reference(name, True)
    d, yd, logits, yp, _ = _forward(name, R)
    F = d[3].numel()
    g = torch.Generator().manual_seed(99)
    pre_W, pre_b = torch.randn(F, generator=g).cuda(), torch.randn(1, generator=g).cuda()
    runs = []
    for fill in (None, None, (pre_W, pre_b)):
        dW = torch.zeros(F, device="cuda") if fill is None else fill[0].clone()
        db = torch.zeros(1, device="cuda") if fill is None else fill[1].clone()
        out = ops.scorer_ce_bwd(*d, yd, logits, yp, R["loss_scale"], dW, db, eu, tanh, tf_xent_grad=True)
        runs.append(tuple(out) + (dW, db))
    for a, b2 in zip(runs[0], runs[1]):
        assert torch.equal(a, b2)
    assert runs[0][3].abs().max().item() > 0 and runs[0][4].abs().max().item() > 0
    assert torch.equal(runs[2][3], pre_W + runs[0][3])
    assert torch.equal(runs[2][4], pre_b + runs[0][4])
    for a, b2 in zip(runs[0][:3], runs[2][:3]):       # the input gradients do not depend on what dW / db held
        assert torch.equal(a, b2)


@pytest.mark.parametrize("tf_grad", [True, False], ids=["tf", "math"])
def test_scorer_ce_autograd_wrapper(tf_grad):
    """fvta_memexqa_amd.autograd.scorer_ce at 35x4x320 (unrolled rounds, two trips of ch += 256, a multi-hot row)."""
    from fvta_memexqa_amd import autograd as A
    name = "35x4x320"
    _, _, _, eu, tanh, _, _ = CASES[name]
    R = _reference(name, tf_grad)
    gq, g1, gch, W, b = R["inp"]
    cl = [t.float().cuda().requires_grad_() for t in (gq, g1, gch, W, b)]
    loss, logits, yp = A.scorer_ce(*cl, R["y"].cuda(), use_eu_output=eu, add_tanh=tanh, tf_xent_grad=tf_grad)
    assert loss.grad_fn is not None and not logits.requires_grad and not yp.requires_grad
    (loss * R["loss_scale"]).backward()
    got = dict(logits=logits, yp=yp, loss=loss, dgq=cl[0].grad, dg1=cl[1].grad, dgch=cl[2].grad, dW=cl[3].grad,
               db=cl[4].grad)
    _check("autograd %s %s" % (name, "tf" if tf_grad else "math"), got, R, NAMES)
