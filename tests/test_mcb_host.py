"""Host-side checks of the MCB pieces, no GPU: the count sketch tables are the ones the reference's layer draws, the
fp64 reference's two routes (the definition and the FFT route) agree, the C ABI of compact bilinear pooling answers its
size queries and reports bad arguments as status codes, and user-supplied tables are validated before any upload."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from fvta_memexqa_amd import _lib, ops
from tests import _mcb_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
# the cases of tests/test_gpu_mcb.py: (N, P, d1, d2, D)
CASES = [(1, 1, 8, 4, 64), (2, 3, 37, 10, 100), (3, 64, 300, 40, 250), (2, 5, 257, 128, 1000), (5, 1, 64, 64, 4096),
         (1, 2, 2537, 100, 16000), (2, 2, 100, 20, 16384)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _numpy_recipe(d1, d2, D, seeds=(1, 3, 5, 7)):
    """the layer's own draws, through the global legacy generator it uses"""
    state = np.random.get_state()
    try:
        np.random.seed(seeds[0])
        h1 = np.random.randint(D, size=d1)
        np.random.seed(seeds[1])
        s1 = 2 * np.random.randint(2, size=d1) - 1
        np.random.seed(seeds[2])
        h2 = np.random.randint(D, size=d2)
        np.random.seed(seeds[3])
        s2 = 2 * np.random.randint(2, size=d2) - 1
    finally:
        np.random.set_state(state)
    return h1, s1, h2, s2


@pytest.mark.parametrize("shape", [(2537, 100, 16000), (8, 4, 64)])
def test_count_sketch_tables_are_the_layers_draws(shape):
    got = ops.count_sketch_tables(*shape)
    want = _numpy_recipe(*shape)
    golden = json.load(open(os.path.join(HERE, "golden", "count_sketch_tables.json")))["%d_%d_%d" % shape]
    for name, g, w in zip(("h1", "s1", "h2", "s2"), got, want):
        assert g.shape == w.shape and (g == w).all(), name
        assert list(map(int, g[:16])) == golden[name], name + ": the generator's stream changed"
    assert got[0].min() >= 0 and got[0].max() < shape[2] and set(np.unique(got[1])) <= {-1, 1}


def test_count_sketch_tables_follow_their_seeds():
    a = ops.count_sketch_tables(37, 10, 100)
    b = ops.count_sketch_tables(37, 10, 100, seeds=(2, 3, 5, 8))
    assert (a[0] != b[0]).any() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] != b[3]).any()


@pytest.mark.parametrize("case", CASES)
def test_reference_routes_agree(case):
    N, P, d1, d2, D = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.relu(torch.randn(N * P, d1, generator=g, dtype=torch.float64))
    q = 0.5 * torch.randn(N, d2, generator=g, dtype=torch.float64)
    tabs = ops.count_sketch_tables(d1, d2, D)
    a, b = R.cbp_direct(x, q, *tabs, D, P), R.cbp_fft(x, q, *tabs, D, P)
    assert float((a - b).abs().max()) <= 1e-10
    y = R.normalize(a)
    live = a.abs().sum(1) > 0
    assert torch.allclose((y * y).sum(1)[live], torch.ones(int(live.sum()), dtype=torch.float64), atol=1e-12)


def test_reference_normalize_zero_conventions():
    z = torch.tensor([[0.0, 4.0, -9.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    y = R.normalize(z)
    assert torch.allclose(y[0], torch.tensor([0.0, 2.0, 3.0, 0.0], dtype=torch.float64) / 13 ** 0.5) and (y[1] == 0).all()
    (y * torch.arange(8, dtype=torch.float64).reshape(2, 4)).sum().backward()
    assert torch.isfinite(z.grad).all() and (z.grad[0, [0, 3]] == 0).all() and (z.grad[1] == 0).all()


def test_abi_descriptor_and_size_queries(lib):
    assert lib.fvta_abi_struct_bytes(11) == ctypes.sizeof(_lib.CbpDesc) == 28
    assert lib.fvta_abi_struct_bytes(8) == -1
    infer = _lib.CbpDesc(16, 64, 2537, 100, 16000, 1, 0)
    train = _lib.CbpDesc(16, 64, 2537, 100, 16000, 1, 1)
    assert lib.fvta_cbp_saved_bytes(ctypes.byref(infer)) == 0
    assert lib.fvta_cbp_saved_bytes(ctypes.byref(train)) >= 16 * 64 * 4
    # `saved` is words per row, never a copy of the [N P, D] output
    assert lib.fvta_cbp_saved_bytes(ctypes.byref(train)) < 16 * 64 * 16000
    fwd = lib.fvta_cbp_workspace_bytes(ctypes.byref(train), 0)
    bwd = lib.fvta_cbp_workspace_bytes(ctypes.byref(train), 1)
    assert 0 < fwd < bwd and bwd - fwd >= 16 * 64 * 100 * 4          # the per-row partials of dq
    for D in (16000, 16384):
        assert lib.fvta_cbp_workspace_bytes(ctypes.byref(_lib.CbpDesc(1, 1, 8, 4, D, 0, 1)), 1) > 0
    big = _lib.CbpDesc(1, 1, 20000, 17000, 64, 0, 1)                  # d1 > D, d2 > D are legal
    assert lib.fvta_cbp_workspace_bytes(ctypes.byref(big), 1) > 0


def test_abi_reports_bad_arguments(lib):
    P = ctypes.c_void_p
    one = ctypes.create_string_buffer(256)
    ptrs = lambda n: [ctypes.cast(one, P)] * n
    for bad in (_lib.CbpDesc(2, 3, 8, 4, 0, 0, 1), _lib.CbpDesc(2, 3, 8, 4, -5, 0, 1), _lib.CbpDesc(2, 0, 8, 4, 64, 0, 1),
                _lib.CbpDesc(2, -1, 8, 4, 64, 0, 1), _lib.CbpDesc(2, 3, 8, 4, 64, 2, 1)):
        assert lib.fvta_cbp_saved_bytes(ctypes.byref(bad)) == 0 and b"bad N/P/d1/d2/D" in lib.fvta_last_error()
        assert lib.fvta_cbp_workspace_bytes(ctypes.byref(bad), 0) == 0
        assert lib.fvta_cbp_fwd(ctypes.byref(bad), *ptrs(9), None) == -1 and b"cbp_fwd" in lib.fvta_last_error()
        assert lib.fvta_cbp_bwd(ctypes.byref(bad), *ptrs(10), 0, ctypes.cast(one, P), None) == -1
    over = _lib.CbpDesc(2, 3, 8, 4, 16385, 1, 1)
    assert lib.fvta_cbp_saved_bytes(ctypes.byref(over)) == 0
    assert b"unsupported" in lib.fvta_last_error() and b"16384" in lib.fvta_last_error()
    assert lib.fvta_cbp_workspace_bytes(ctypes.byref(over), 1) == 0
    assert lib.fvta_cbp_fwd(ctypes.byref(over), *ptrs(9), None) == -3 and b"16384" in lib.fvta_last_error()
    assert lib.fvta_cbp_bwd(ctypes.byref(over), *ptrs(10), 0, ctypes.cast(one, P), None) == -3
    ok = _lib.CbpDesc(2, 3, 8, 4, 64, 1, 1)
    assert lib.fvta_cbp_fwd(ctypes.byref(ok), None, *ptrs(8), None) == -1 and b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_cbp_fwd(None, *ptrs(9), None) == -1
    # normalize = 1 in training keeps a word per row: a NULL `saved` is an error, not a crash
    a = ptrs(9)
    a[7] = None
    assert lib.fvta_cbp_fwd(ctypes.byref(ok), *a, None) == -1 and b"saved" in lib.fvta_last_error()
    b = ptrs(10)
    b[8] = b[9] = None                                                 # dx and dq both NULL
    assert lib.fvta_cbp_bwd(ctypes.byref(ok), *b, 0, ctypes.cast(one, P), None) == -1 and b"both NULL" in lib.fvta_last_error()
    notrain = _lib.CbpDesc(2, 3, 8, 4, 64, 1, 0)
    assert lib.fvta_cbp_bwd(ctypes.byref(notrain), *ptrs(10), 0, ctypes.cast(one, P), None) == -1
    assert b"training = 0" in lib.fvta_last_error()


def test_host_side_table_validation():
    h1, s1, h2, s2 = ops.count_sketch_tables(8, 4, 64)
    got = ops.check_sketch_tables(h1, s1, h2, s2, 8, 4, 64)
    assert [a.dtype for a in got] == [np.int32, np.float32, np.int32, np.float32]
    assert (got[0] == h1).all() and (got[1] == s1).all()
    assert (ops.check_sketch_tables(torch.as_tensor(h1), torch.as_tensor(s1), h2, s2, 8, 4, 64)[0] == h1).all()
    bad = h1.copy()
    bad[3] = 64
    with pytest.raises(ValueError, match=r"rand_h_1.*\[0, 64\)"):
        ops.check_sketch_tables(bad, s1, h2, s2, 8, 4, 64)
    bad[3] = -1
    with pytest.raises(ValueError, match="rand_h_1"):
        ops.check_sketch_tables(bad, s1, h2, s2, 8, 4, 64)
    bad = s2.copy()
    bad[0] = 0
    with pytest.raises(ValueError, match="rand_s_2.*signs"):
        ops.check_sketch_tables(h1, s1, h2, bad, 8, 4, 64)
    with pytest.raises(ValueError, match="rand_h_2.*4 entries"):
        ops.check_sketch_tables(h1, s1, h2[:3], s2, 8, 4, 64)
    with pytest.raises(ValueError, match="rand_h_1.*integers"):
        ops.check_sketch_tables(h1 + 0.5, s1, h2, s2, 8, 4, 64)
