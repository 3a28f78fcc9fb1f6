"""The context tensor (model_v2.py:863-914) as one library call each way: fvta_context_fwd / _bwd and
functional.context_tensor against the oracle's pad + stack.  The op is a copy, so every comparison is bitwise."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, M, J list, w)
SHAPES = [(2, 2, [1, 5, 12], 100), (1, 3, [7], 64),          # K = 1: no padding at all
          (2, 1, [4, 4, 4], 8),                                # all equal
          (1, 2, [3, 1, 2, 5, 1, 4, 2, 6], 4),                 # K = 8
          (2, 2, [5, 9], 6),                                   # w % 4 != 0: the 4-byte path
          (3, 1, [2, 11], 1024)]


def _case(N, M, Js, w, seed=0):
    g = torch.Generator().manual_seed(seed + N * 100 + M * 10 + len(Js) + w)
    streams = [torch.randn(N, M, J, w, generator=g) for J in Js]
    masks = [torch.rand(N, M, J, generator=g) < 0.6 for J in Js]
    K, jmax = len(Js), max(Js)
    if K > 1:
        k_short = min(range(K), key=lambda k: (Js[k], k))
        k_long = max(range(K), key=lambda k: (Js[k], k))
        masks[k_short][:] = False                              # an all-False stream
        masks[k_long][:, :, jmax - 1] = True                   # a set bit where the shorter streams have only padding
    return streams, masks


def _ref(streams, masks):
    from oracle import fvta_fused as F
    return F.context_tensor(streams, masks)


@pytest.mark.parametrize("N,M,Js,w", SHAPES)
def test_forward_writes_every_element_once(N, M, Js, w):
    """through ops.context_fwd into outputs pre-filled with NaN / 0xFF; with and without masks; twice"""
    from fvta_memexqa_amd import ops
    streams, masks = _case(N, M, Js, w)
    ref_h, ref_m = _ref(streams, masks)
    cs = [s.cuda() for s in streams]
    cm = [m.cuda().to(torch.uint8) for m in masks]
    K, jmax = len(Js), max(Js)
    for with_masks in (True, False):
        runs = []
        for _ in range(2):
            hall = torch.full((N, K, M, jmax, w), float("nan"), device="cuda")
            hm = torch.full((N, K, M, jmax), 0xFF, dtype=torch.uint8, device="cuda") if with_masks else None
            ops.context_fwd(cs, cm if with_masks else None, hall, hm)
            assert torch.equal(hall.cpu(), ref_h)
            if with_masks:
                assert torch.equal(hm.cpu(), ref_m.to(torch.uint8))
            runs.append((hall, hm))
        assert torch.equal(runs[0][0], runs[1][0])


@pytest.mark.parametrize("N,M,Js,w", SHAPES)
def test_backward_overwrites_the_gradient_buffers(N, M, Js, w):
    from fvta_memexqa_amd import ops
    K, jmax = len(Js), max(Js)
    g = torch.Generator().manual_seed(7 + w)
    d_hall = torch.randn(N, K, M, jmax, w, generator=g)
    dh = d_hall.cuda()
    ds = [torch.full((N, M, J, w), float("nan"), device="cuda") for J in Js]
    ops.context_bwd(dh, ds, N, M, Js, w)
    for k, J in enumerate(Js):
        assert torch.equal(ds[k].cpu(), d_hall[:, k, :, :J]), k
    if K > 1:                                                  # a skipped entry: the others are still written, it is untouched
        ds2 = [torch.full((N, M, J, w), float("nan"), device="cuda") for J in Js]
        keep = ds2[0].clone()
        ops.context_bwd(dh, [None] + ds2[1:], N, M, Js, w)
        assert torch.equal(ds2[0].isnan(), keep.isnan()) and bool(ds2[0].isnan().all())
        for k in range(1, K):
            assert torch.equal(ds2[k].cpu(), d_hall[:, k, :, :Js[k]]), k


def test_a_stream_off_the_16_byte_grid_takes_the_scalar_path_and_is_exact():
    """w % 4 == 0, but stream 1 starts one float past a 16-byte boundary (a slice of a larger buffer)"""
    from fvta_memexqa_amd import functional as Fn
    N, M, Js, w = 2, 2, [3, 6], 8
    streams, masks = _case(N, M, Js, w, seed=3)
    ref_h, ref_m = _ref(streams, masks)
    buf = torch.empty(streams[1].numel() + 4, device="cuda")
    off = buf[1:1 + streams[1].numel()].view(streams[1].shape)
    off.copy_(streams[1])
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    hall, hm = Fn.context_tensor([streams[0].cuda(), off], [m.cuda() for m in masks])
    assert torch.equal(hall.cpu(), ref_h) and torch.equal(hm.cpu(), ref_m)
    # ... and a gradient buffer off the grid
    from fvta_memexqa_amd import ops
    d_hall = torch.randn(N, 2, M, 6, w, generator=torch.Generator().manual_seed(1))
    gbuf = torch.full((streams[0].numel() + 4,), float("nan"), device="cuda")
    d0 = gbuf[1:1 + streams[0].numel()].view(streams[0].shape)
    d1 = torch.full(streams[1].shape, float("nan"), device="cuda")
    ops.context_bwd(d_hall.cuda(), [d0, d1], N, M, Js, w)
    assert torch.equal(d0.cpu(), d_hall[:, 0, :, :3]) and torch.equal(d1.cpu(), d_hall[:, 1])
    assert bool(gbuf[0].isnan()) and bool(gbuf[-3:].isnan().all())          # nothing outside the slice


@pytest.mark.parametrize("N,M,Js,w", [SHAPES[0], SHAPES[4]])
def test_functional_context_tensor_under_autograd(N, M, Js, w):
    from fvta_memexqa_amd import functional as Fn
    streams, masks = _case(N, M, Js, w, seed=5)
    ref_h, ref_m = _ref(streams, masks)
    K = len(Js)
    d_hall = torch.randn(ref_h.shape, generator=torch.Generator().manual_seed(2))
    # bool masks in, bool mask out; the mask is not differentiable
    cs = [s.cuda().requires_grad_() for s in streams]
    hall, hm = Fn.context_tensor(cs, [m.cuda() for m in masks])
    assert hm.dtype == torch.bool and not hm.requires_grad and hall.grad_fn is not None
    assert torch.equal(hall.detach().cpu(), ref_h) and torch.equal(hm.cpu(), ref_m)
    torch.autograd.backward([hall], [d_hall.cuda()])
    for k, J in enumerate(Js):
        assert torch.equal(cs[k].grad.cpu(), d_hall[:, k, :, :J]), k
    # u8 masks give the same; no masks give no mask
    hall_u, hm_u = Fn.context_tensor([s.detach() for s in cs], [m.cuda().to(torch.uint8) for m in masks])
    assert hm_u.dtype == torch.bool and torch.equal(hm_u, hm)
    hall_n, none = Fn.context_tensor([s.detach() for s in cs])
    assert none is None
    # nothing requires grad: no graph, the same bits
    assert hall_u.grad_fn is None and hall_n.grad_fn is None
    assert torch.equal(hall_u, hall.detach()) and torch.equal(hall_n, hall.detach())
    # only some streams require grad: the others' .grad stay None
    part = [s.cuda().requires_grad_(k == K - 1) for k, s in enumerate(streams)]
    hall_p, _ = Fn.context_tensor(part, [m.cuda() for m in masks])
    torch.autograd.backward([hall_p], [d_hall.cuda()])
    assert all(p.grad is None for p in part[:-1])
    assert torch.equal(part[-1].grad.cpu(), d_hall[:, K - 1, :, :Js[-1]])


def test_functional_context_tensor_refuses_what_the_kernel_cannot_take():
    from fvta_memexqa_amd import functional as Fn
    s = lambda J, w=8: torch.zeros(2, 1, J, w, device="cuda")
    with pytest.raises(ValueError):
        Fn.context_tensor([s(2)] * 9)
    with pytest.raises(ValueError):
        Fn.context_tensor([s(2), s(3, w=4)])
    with pytest.raises(ValueError):
        Fn.context_tensor([s(2), s(3)], [torch.ones(2, 1, 2, dtype=torch.bool, device="cuda")])


def test_past_two_to_the_31_elements():
    """N = 1, M = 1, J = [1_100_000, 8], w = 1024: hall has 2.25 G elements (9 GB), stream 0 4.5 GB.  Sampled rows only --
    the torch reference is not built at this size."""
    from fvta_memexqa_amd import ops
    J0, J1, w = 1_100_000, 8, 1024
    if torch.cuda.mem_get_info()[0] < 20 * 2 ** 30:
        pytest.fail("this test needs 20 GB of free device memory")
    s0 = torch.empty(1, 1, J0, w, device="cuda")
    s0.view(-1, w)[:] = torch.arange(w, device="cuda", dtype=torch.float32)[None, :]
    s0[0, 0, :, 0] = torch.arange(J0, device="cuda", dtype=torch.float32)           # row j carries j in channel 0 (exact < 2^24)
    s1 = torch.randn(1, 1, J1, w, device="cuda")
    m0 = torch.zeros(1, 1, J0, dtype=torch.uint8, device="cuda")
    m0[0, 0, -3:] = torch.tensor([1, 0, 1], dtype=torch.uint8)
    m1 = torch.ones(1, 1, J1, dtype=torch.uint8, device="cuda")
    hall = torch.empty(1, 2, 1, J0, w, device="cuda")
    hm = torch.full((1, 2, 1, J0), 0xFF, dtype=torch.uint8, device="cuda")
    assert hall.numel() > 2 ** 31
    # NaN in the regions the checks below read, so a kernel that skipped them would show
    hall[0, 0, 0, -2:] = float("nan")
    hall[0, 1, 0, :16] = float("nan")
    hall[0, 1, 0, -2:] = float("nan")
    ops.context_fwd([s0, s1], [m0, m1], hall, hm)
    assert torch.equal(hall[0, 0, 0, -1], s0[0, 0, -1]) and float(hall[0, 0, 0, -1, 0]) == J0 - 1
    assert torch.equal(hall[0, 0, 0, J0 // 2 + 1], s0[0, 0, J0 // 2 + 1])
    assert torch.equal(hall[0, 1, 0, :8], s1[0, 0])
    assert bool((hall[0, 1, 0, 8:16] == 0).all()) and bool((hall[0, 1, 0, -2:] == 0).all())
    assert hm[0, 0, 0, -3:].tolist() == [1, 0, 1]
    assert hm[0, 1, 0, :8].tolist() == [1] * 8 and hm[0, 1, 0, -3:].tolist() == [0, 0, 0] and int(hm[0, 1, 0, 8]) == 0
    del s0, m0
    # backward: hall as d_hall, the same sampled rows
    d0 = torch.empty(1, 1, J0, w, device="cuda")
    d0[0, 0, -2:] = float("nan")
    d0[0, 0, :2] = float("nan")
    d1 = torch.full((1, 1, J1, w), float("nan"), device="cuda")
    ops.context_bwd(hall, [d0, d1], 1, 1, [J0, J1], w)
    assert torch.equal(d0[0, 0, -1], hall[0, 0, 0, -1]) and float(d0[0, 0, -1, 0]) == J0 - 1
    assert torch.equal(d0[0, 0, 0], hall[0, 0, 0, 0]) and torch.equal(d0[0, 0, J0 // 2 + 1], hall[0, 0, 0, J0 // 2 + 1])
    assert torch.equal(d1[0, 0], s1[0, 0])
