"""Host side of the GRU sequence op (no GPU: the library loads without one): the identities the torch reference of
tests/_gru_ref.py must satisfy, and the host queries of the C ABI -- fvta_gru_seq_plan, _saved_bytes, _workspace_bytes and the
argument checks of _fwd / _bwd."""
import ctypes
import math

import pytest
import torch

from tests import _gru_ref as R


def _inputs(N=5, T=6, din=3, d=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    s = 0.5 / math.sqrt(din + d)
    return dict(x=rnd(N, T, din) * 0.5, h0=rnd(N, d) * 0.5, Wg=rnd(din + d, 2 * d) * s, bg=1 + 0.1 * rnd(2 * d),
                Wc=rnd(din + d, d) * s, bc=0.1 * rnd(d))


def test_reference_reverse_is_flip_forward_flip():
    c = _inputs()
    lens = [6, 0, 1, 4, 3]
    P = (c["Wg"], c["bg"], c["Wc"], c["bc"])
    out_r, last_r = R.gru_seq(c["x"], lens, c["h0"], *P, reverse=True)
    out_f, last_f = R.gru_seq(R.flip_prefix(c["x"], lens), lens, c["h0"], *P)
    assert (out_r - R.flip_prefix(out_f, lens)).abs().max().item() == 0
    assert (last_r - last_f).abs().max().item() == 0


@pytest.mark.parametrize("reverse", [False, True])
def test_reference_padding_and_empty_rows(reverse):
    c = _inputs()
    lens = [6, 0, 1, 4, 3]
    P = (c["Wg"], c["bg"], c["Wc"], c["bc"])
    out, last = R.gru_seq(c["x"], lens, c["h0"], *P, reverse=reverse)
    for n, L in enumerate(lens):
        assert out[n, L:].abs().sum().item() == 0
        if L:
            assert torch.equal(last[n], out[n, 0 if reverse else L - 1])
    assert torch.equal(last[1], c["h0"][1])
    assert torch.equal(R.gru_seq(c["x"], lens, None, *P, reverse=reverse)[1][1], torch.zeros(4, dtype=torch.float64))
    full = R.gru_seq(c["x"], None, c["h0"], *P, reverse=reverse)
    same = R.gru_seq(c["x"], [6] * 5, c["h0"], *P, reverse=reverse)
    assert torch.equal(full[0], same[0]) and torch.equal(full[1], same[1])


def test_reference_closed_form_with_zero_kernels():
    """zero kernels, bg = 1, bc = b: every step is h' = s h + (1 - s) tanh(b) with s = sigmoid(1), so from h0 = 0
    h_T = tanh(b) (1 - s^T)"""
    N, T, din, d = 2, 7, 3, 4
    b = torch.tensor([0.3, -1.2, 0.0, 2.0], dtype=torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    x = torch.randn(N, T, din, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out, last = R.gru_seq(x, None, None, z(din + d, 2 * d), torch.ones(2 * d, dtype=torch.float64), z(din + d, d), b)
    s = 1 / (1 + math.exp(-1.0))
    want = torch.tanh(b) * (1 - s ** T)
    assert (last - want[None, :]).abs().max().item() < 1e-14
    assert (out[:, 2] - (torch.tanh(b) * (1 - s ** 3))[None, :]).abs().max().item() < 1e-14


# ------------------------------------------------------------------ the C ABI's host queries
@pytest.fixture(scope="module")
def lib():
    from fvta_memexqa_amd import _lib
    return _lib.load()


def _desc(N=4, T=3, in_dim=8, d=16, reverse=0, training=1):
    from fvta_memexqa_amd import _lib
    return _lib.GruSeqDesc(N, T, in_dim, d, reverse, training)


def test_descriptor_layout(lib):
    from fvta_memexqa_amd import _lib
    assert lib.fvta_abi_struct_bytes(10) == ctypes.sizeof(_lib.GruSeqDesc) == 24
    for name in ("saved_bytes", "workspace_bytes", "plan", "fwd", "bwd"):
        assert "fvta_gru_seq_" + name in _lib.exported_symbols()


def test_plan_regimes_and_edge():
    from fvta_memexqa_amd import ops
    for d in (16, 100):
        p = ops.gru_seq_plan(64, 192, 100, d)
        assert p["regime"] == "A" and p["fwd_launches"] == 3 and p["row_tile"] >= 1, (d, p)
    assert ops.gru_seq_plan(64, 2, 100, 100) == ops.gru_seq_plan(64, 192, 100, 100)      # one launch, whatever T
    b1, b48 = ops.gru_seq_plan(64, 1, 512, 512), ops.gru_seq_plan(64, 48, 512, 512)
    assert b1["regime"] == b48["regime"] == "B"
    assert b48["fwd_launches"] - b1["fwd_launches"] == 2 * 47                            # one launch per product per step
    assert b48["bwd_launches"] - b1["bwd_launches"] == 2 * 47
    regimes = [ops.gru_seq_plan(17, 3, 24, d)["regime"] for d in range(1, 514)]
    edge = regimes.index("B") + 1
    assert edge > 100, "the single-launch regime must cover d = 100"
    assert all(r == "A" for r in regimes[:edge - 1]) and all(r == "B" for r in regimes[edge - 1:])
    assert ops.gru_seq_plan(17, 3, 999, edge - 1)["regime"] == "A"                       # the edge does not depend on in_dim


def test_size_queries(lib):
    for d in (16, 100, 512):
        for training in (0, 1):
            desc = _desc(N=5, T=7, in_dim=9, d=d, training=training)
            assert lib.fvta_gru_seq_workspace_bytes(ctypes.byref(desc), 0) >= 4 * 5 * 7 * 3 * d
            assert lib.fvta_gru_seq_workspace_bytes(ctypes.byref(desc), 1) >= 4 * 5 * 7 * 4 * d
            saved = lib.fvta_gru_seq_saved_bytes(ctypes.byref(desc))
            assert (saved >= 4 * 5 * 7 * 3 * d) if training else (saved == 0)


@pytest.mark.parametrize("field", ["N", "T", "in_dim", "d"])
@pytest.mark.parametrize("bad", [0, -3])
def test_non_positive_sizes_are_refused(lib, field, bad):
    desc = _desc(**{field: bad})
    out = (ctypes.c_int32 * 4)()
    assert lib.fvta_gru_seq_plan(ctypes.byref(desc), out) == -1
    assert b"gru_seq_plan" in lib.fvta_last_error()
    assert lib.fvta_gru_seq_saved_bytes(ctypes.byref(desc)) == 0
    assert lib.fvta_gru_seq_workspace_bytes(ctypes.byref(desc), 0) == 0
    assert b"gru_seq_workspace_bytes" in lib.fvta_last_error()
    one = ctypes.c_void_p(256)          # never dereferenced: the argument check comes first
    assert lib.fvta_gru_seq_fwd(ctypes.byref(desc), one, None, None, one, one, one, one, one, one, one, one, None) == -1
    assert b"gru_seq_fwd" in lib.fvta_last_error()


def test_null_arguments_are_refused(lib):
    one = ctypes.c_void_p(256)
    desc, out = _desc(), (ctypes.c_int32 * 4)()
    assert lib.fvta_gru_seq_plan(None, out) == -1
    assert lib.fvta_gru_seq_plan(ctypes.byref(desc), None) == -1
    assert b"null" in lib.fvta_last_error()
    assert lib.fvta_gru_seq_saved_bytes(None) == 0 and lib.fvta_gru_seq_workspace_bytes(None, 1) == 0
    assert lib.fvta_gru_seq_plan(ctypes.byref(_desc(reverse=2)), out) == -1
    # forward: x, a weight, h_last, the workspace, `saved` under training
    fwd = [one, None, None, one, one, one, one, one, one, one, one, None]
    for i in (0, 3, 4, 5, 6, 8, 9, 10):
        args = list(fwd)
        args[i] = None
        assert lib.fvta_gru_seq_fwd(ctypes.byref(desc), *args) == -1, i
        assert b"gru_seq_fwd" in lib.fvta_last_error()
    # backward: both output gradients NULL; a NULL target; a descriptor that saved nothing
    bwd = [one, None, one, one, one, one, one, one, None, one, one, one, one, 0, one, None]
    args = list(bwd)
    args[5] = args[6] = None
    assert lib.fvta_gru_seq_bwd(ctypes.byref(desc), *args) == -1
    assert b"both NULL" in lib.fvta_last_error()
    for i in (0, 2, 3, 4, 7, 9, 10, 11, 12, 14):
        args = list(bwd)
        args[i] = None
        assert lib.fvta_gru_seq_bwd(ctypes.byref(desc), *args) == -1, i
    assert lib.fvta_gru_seq_bwd(ctypes.byref(_desc(training=0)), *bwd) == -1
    assert b"nothing was saved" in lib.fvta_last_error()


def test_nn_modules_exist():
    """the three modules are part of the public surface (constructing one needs a GPU, naming it does not)"""
    from fvta_memexqa_amd import autograd, nn, ops
    assert callable(autograd.gru_seq) and callable(ops.GRUSeq)
    for name in ("GRUEncoder", "BiGRUFusion", "DMNPlusHead"):
        assert issubclass(getattr(nn, name), torch.nn.Module)
