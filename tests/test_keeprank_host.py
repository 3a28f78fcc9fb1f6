"""Host-side checks behind tests/test_gpu_keeprank_autograd.py: what must hold without a GPU."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from fvta_memexqa_amd import _lib
    return _lib.load()


def test_oracle_has_no_exact_tie_in_the_keeprank_cases():
    """The GPU tests compare the gradient of attention_keeprank1 with the oracle's (TensorFlow's tie splitting); the
    kernels send a tie to the first arg-max, and a fully masked list passes nothing into its logits.  The two agree only
    where every (n,m) keeps a valid row, every question a valid position, and every valid row has a unique maximum over
    the question."""
    from oracle import fvta_fused as F
    from tests.test_gpu_keeprank_autograd import ORACLE_CASES, kr_case
    for name, (N, M, V, JQ, w, simi, masked, seed, bidirect) in ORACLE_CASES.items():
        h, q, W, b, hm, qm = kr_case(N, M, V, JQ, w, simi, masked, seed)
        a = F.simi_logits(h.double(), q.double()[:, None], W.double(), b.double(), simi, False, "v1")
        valid = torch.ones(N, M, V, dtype=torch.bool)
        if masked:
            assert bool(hm.reshape(N * M, V).any(1).all()), "%s: an (n,m) without a valid row" % name
            assert bool(qm.any(1).all()), "%s: a question without a valid position" % name
            a = F.exp_mask(a, hm[..., None] & qm[:, None, None, :])
            valid = hm
        amax = a.amax(-1, keepdim=True)
        assert int(((a == amax).sum(-1) > 1)[valid].sum()) == 0, "%s: a tie in the max over the question" % name


def test_plan_puts_the_split_and_grouped_shapes_in_their_regimes(lib):
    """fvta_attn_plan (host only): the (b) shapes run several backward workgroups per (n,m), the (c) shape lies where the
    ordinary backward groups several k into one workgroup"""
    from fvta_memexqa_amd._lib import AttnDesc
    from tests.test_gpu_keeprank_autograd import ORACLE_CASES, PLAN
    plan = (ctypes.c_int32 * 4)()
    for name, (key, want) in PLAN.items():
        N, M, V, JQ, w, simi, masked, seed, bidirect = ORACLE_CASES[name]
        assert lib.fvta_attn_plan(ctypes.byref(AttnDesc(N, M, V, JQ, w, simi, 1, 0, 0)), int(masked), plan) == 0
        got = dict(zip(("nsplit", "bsplit", "gk", "ng"), plan))
        assert got[key] == want and want > 1, "%s: %r" % (name, got)
        if key == "gk":
            assert got["bsplit"] == 1 and N * M >= 1024


def test_attn_bwd_u_is_bound_and_rejects_bad_descriptors_on_the_host(lib):
    """the entry's argument checks run before anything touches the GPU: simiMatrix 4, a non-zero hinfo_stride and
    accumulate = 2 come back as a negative status with a message; the workspace query answers for a supported shape and
    grows past the ordinary backward's where that one groups k"""
    from fvta_memexqa_amd._lib import AttnDesc
    null = (None,) * 7

    def call(desc, acc):
        return lib.fvta_attn_bwd_u(ctypes.byref(desc), *null, None, None, None, None, None, acc, None, None)

    assert call(AttnDesc(2, 1, 8, 3, 64, 4, 0, 0, 0), 0) < 0 and b"simiMatrix 4" in lib.fvta_last_error()
    assert call(AttnDesc(2, 1, 8, 3, 64, 1, 0, 0, 1024), 0) < 0 and b"hinfo_stride" in lib.fvta_last_error()
    assert call(AttnDesc(2, 1, 8, 3, 64, 1, 0, 0, 0), 2) < 0 and b"accumulate" in lib.fvta_last_error()
    assert call(AttnDesc(2, 1, 8, 3, 64, 1, 0, 0, 0), 0) < 0 and b"null pointer" in lib.fvta_last_error()
    assert lib.fvta_attn_bwd_u_workspace_bytes(ctypes.byref(AttnDesc(2, 1, 8, 3, 64, 4, 0, 0, 0))) == 0
    assert lib.fvta_attn_bwd_u_workspace_bytes(ctypes.byref(AttnDesc(16384, 4, 1, 2, 64, 1, 1, 0, 0))) == 0
    assert b"65535" in lib.fvta_last_error()
    d = AttnDesc(260, 4, 6, 3, 64, 2, 1, 0, 0)
    # one slab set per (n,k) instead of one per group of gk = 2: 16 row groups x 32 padded question positions x w floats each
    assert lib.fvta_attn_bwd_u_workspace_bytes(ctypes.byref(d)) >= 260 * 4 * 16 * 32 * 64 * 4
