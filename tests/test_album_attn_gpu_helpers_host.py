"""The comparers of tests/_album_attn_gpu.py, which every album attention GPU test trusts, on synthetic CPU tensors: the
scaled comparison against the absolute one, `check_grads` holding each output to its own entry of the real TOL
(tests/_attn_shared_tw_bwd_ref.py) and skipping none, and the dWH_W rule.  No reference computation, no GPU."""
import pytest
import torch

from tests import _attn_shared_tw_bwd_ref as TB
from tests._album_attn_gpu import check_grads, close, close_scaled, output_names, ref_key, tol_of

W = 4
SHAPES = dict(dh=(2, 3, W), dpool=(2, 3, W), dq=(3, 2, W), dlq=(3, W), dW=(3 * W,), db=(1,), dWH_W=(2 * W, W), dWH_b=(W,),
              dWC_W=(W,), dWC_b=(1,))
VARIANTS = [(family, warped) for family in ("shared", "pooled") for warped in (True, False)]


def test_scaled_against_absolute():
    ref = torch.tensor([100.0, 0.0, 1.0])
    got = ref + torch.tensor([0.0, 5e-4, 0.0])
    close_scaled(got, ref)                                       # 5e-4 <= 1e-5 * 100
    with pytest.raises(AssertionError):
        close(got, ref)                                          # 5e-4 > 1e-5
    close(got.numpy(), ref.tolist(), atol=1e-3)                  # arrays and lists, as well as tensors


def _reference(names, seed=0):
    """a reference dict under the reference modules' keys: magnitudes from 1e-3 to 30, mixed signs, no zero"""
    g = torch.Generator().manual_seed(seed)
    ref = {}
    for i, n in enumerate(names):
        mag = 10.0 ** (torch.rand(SHAPES[ref_key(n)], generator=g, dtype=torch.float64) * 4.5 - 3.0)
        ref[ref_key(n)] = mag * torch.where(torch.rand(mag.shape, generator=g) < 0.5, -1.0, 1.0) * (1 + i % 3)
    return ref


def _outputs(names, ref, off=None, factor=0.5):
    """every output off by `factor` (one output `off`: by twice) of its own bound atol max(1, max|ref|) + rtol |ref|; dWH_W
    comes as the op gives it, [w,w]"""
    got = []
    for n in names:
        want = ref[ref_key(n)][:W] if n == "dWH_W" else ref[ref_key(n)]
        rtol, atol = tol_of(TB.TOL, n)
        bound = atol * max(1.0, float(want.abs().max())) + rtol * want.abs()
        got.append(want + (2.0 if n == off else factor) * bound)
    return got


@pytest.mark.parametrize("family,warped", VARIANTS)
def test_check_grads_holds_every_output_to_its_own_tolerance(family, warped, capsys):
    names = output_names(family, warped)
    assert len(names) == (9 if warped else 4) and len(set(names)) == len(names)
    assert {tol_of(TB.TOL, n) for n in names} == ({(1e-4, 1e-5), (2e-4, 2e-5)} if warped else {(1e-4, 1e-5)})
    ref = _reference(names)
    check_grads("synthetic", _outputs(names, ref), ref, names, TB.TOL, TB.within)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("synthetic ")]
    assert len(lines) == len(names) and all("= 0.500" in ln for ln in lines), lines     # one line per output, at half its bound
    for off in names:                                                                    # exactly one output past its bound
        with pytest.raises(AssertionError, match=off):
            check_grads("synthetic", _outputs(names, ref, off), ref, names, TB.TOL, TB.within)
    with pytest.raises(AssertionError):                                                  # an output missing is not a pass
        check_grads("synthetic", _outputs(names, ref)[:-1], ref, names, TB.TOL, TB.within)


def test_the_tolerances_are_told_apart():
    """an error inside d_lq's 2e-4 / 2e-5 but outside d_hq's 1e-4 / 1e-5 passes as the one and fails as the other"""
    names = output_names("shared", True)
    ref = _reference(names)
    got = _outputs(names, ref, factor=0.25)
    i, j = names.index("d_lq"), names.index("d_hq")
    for k, n in ((i, "d_lq"), (j, "d_hq")):
        want = ref[ref_key(n)]
        got[k] = want + 1.5 * (1e-5 * max(1.0, float(want.abs().max())) + 1e-4 * want.abs())
    with pytest.raises(AssertionError, match="d_hq"):
        check_grads("synthetic", got, ref, names, TB.TOL, TB.within)
    got[j] = ref["dq"]
    check_grads("synthetic", got, ref, names, TB.TOL, TB.within)                         # d_lq at 0.75 of its own bound


def test_dWH_W_is_compared_on_the_rows_the_output_has():
    names = output_names("pooled", True)
    ref = _reference(names)
    assert tuple(ref["dWH_W"].shape) == (2 * W, W) and float(ref["dWH_W"][W:].abs().min()) > 0
    got = _outputs(names, ref)
    assert tuple(got[names.index("dWH_W")].shape) == (W, W)
    check_grads("synthetic", got, ref, names, TB.TOL, TB.within)                         # [w,w] against [2w,w]: the first w rows
    ref["dWH_W"] = torch.cat([ref["dWH_W"][W:], ref["dWH_W"][:W]])                       # ... and not the last
    with pytest.raises(AssertionError, match="dWH_W"):
        check_grads("synthetic", got, ref, names, TB.TOL, TB.within)
