"""The context tensor (model_v2.py:863-914) at the metric shape: functional.context_tensor (fvta_context_fwd / _bwd, one
launch each way) against the eager alternative an nn user had before it (torch.nn.functional.pad x 6 + torch.stack,
masks included), forward and forward + backward, in ONE process, alternating, HIP events around blocks of calls.

Default shape: N = 64, M = 1, w = 1024, five streams of J = 1200 and one of J = 40 -- hall is 1.89 GB, the streams
1.58 GB.  Bytes of the kernel from its shape formula (each input element read once, each output element written once):

    forward   4 w (sum_k N M J_k  +  N K M JMAX)  +  (sum_k N M J_k + N K M JMAX)   mask bytes
    backward  4 w (sum_k N M J_k) x 2                                               (the slice: read, write)

`*_share_of_hbm_peak` is those bytes over the median time over the MI355X's HBM3E peak (8.0 TB/s spec; a plain
float4 copy reaches 6.29 TB/s): the kernel's MODEL bytes over its wall time between events, not a counter.
Prints one JSON line.

    python tools/bench_context.py [--N 64] [--M 1] [--w 1024] [--J 1200,1200,1200,1200,1200,40] [--rounds 24] [--block 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_SPEC = 8.0e12        # bytes / s, HBM3E spec peak of the MI355X
HBM_COPY_MEASURED = 6.29e12   # ... and what a plain float4 copy reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--M", type=int, default=1)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--J", default="1200,1200,1200,1200,1200,40")
    ap.add_argument("--rounds", type=int, default=24, help="timed blocks per variant (>= 20)")
    ap.add_argument("--block", type=int, default=5, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from fvta_memexqa_amd import functional as Fn
    from fvta_memexqa_amd import ops
    dev = ops.require_gpu()
    N, M, w = args.N, args.M, args.w
    Js = [int(j) for j in args.J.split(",")]
    K, JMAX = len(Js), max(Js)
    g = torch.Generator(device=dev).manual_seed(1)
    streams = [torch.randn(N, M, J, w, device=dev, generator=g).requires_grad_() for J in Js]
    masks = [torch.rand(N, M, J, device=dev, generator=g) < 0.7 for J in Js]
    d_hall = torch.randn(N, K, M, JMAX, w, device=dev, generator=g)

    def lib_fwd():
        return Fn.context_tensor(streams, masks)

    def eager_fwd():
        pad = torch.nn.functional.pad
        hs = [pad(s, (0, 0, 0, JMAX - s.shape[2])) for s in streams]
        ms = [pad(m, (0, JMAX - m.shape[2])) for m in masks]
        return torch.stack(hs, 1), torch.stack(ms, 1)

    def with_bwd(fwd):
        def run():
            for s in streams:
                s.grad = None
            hall, _ = fwd()
            hall.backward(d_hall)
        return run

    variants = dict(lib_fwd=lib_fwd, eager_fwd=eager_fwd, lib_fwd_bwd=with_bwd(lib_fwd), eager_fwd_bwd=with_bwd(eager_fwd))
    # the two paths agree bit for bit at the size that is timed
    a, b = lib_fwd(), eager_fwd()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    variants["lib_fwd_bwd"]()
    glib = [s.grad.clone() for s in streams]
    variants["eager_fwd_bwd"]()
    assert all(torch.equal(x, s.grad) for x, s in zip(glib, streams))
    del a, b, glib
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    names = list(variants)
    for r in range(args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.block):
                variants[name]()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.block)
    rows_in, rows_out = sum(N * M * J for J in Js), N * K * M * JMAX
    fwd_bytes = 4 * w * (rows_in + rows_out) + rows_in + rows_out
    bwd_bytes = 4 * w * rows_in * 2
    st = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4),
                        iqr=round(statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0], 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lib_bwd_ms = med["lib_fwd_bwd"] - med["lib_fwd"]
    print(json.dumps(dict(
        shape=dict(N=N, M=M, w=w, J=Js), hall_gb=round(4e-9 * w * rows_out, 3), streams_gb=round(4e-9 * w * rows_in, 3),
        rounds=args.rounds, block=args.block, ms={k: st(v) for k, v in ms.items()},
        speedup_fwd=round(med["eager_fwd"] / med["lib_fwd"], 3),
        speedup_fwd_bwd=round(med["eager_fwd_bwd"] / med["lib_fwd_bwd"], 3),
        lib_fwd_model_bytes=fwd_bytes, lib_fwd_model_tbs=round(fwd_bytes / (med["lib_fwd"] * 1e-3) / 1e12, 3),
        lib_fwd_share_of_hbm_peak=round(fwd_bytes / (med["lib_fwd"] * 1e-3) / HBM_PEAK_SPEC, 3),
        lib_fwd_share_of_measured_copy=round(fwd_bytes / (med["lib_fwd"] * 1e-3) / HBM_COPY_MEASURED, 3),
        lib_bwd_model_bytes=bwd_bytes, lib_bwd_ms_by_difference=round(lib_bwd_ms, 4),
        lib_bwd_share_of_hbm_peak=round(bwd_bytes / (lib_bwd_ms * 1e-3) / HBM_PEAK_SPEC, 3) if lib_bwd_ms > 0 else None)))


if __name__ == "__main__":
    main()
