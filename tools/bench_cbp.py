"""Times compact bilinear pooling with the normalisation fused (autograd.compact_bilinear, normalize=True, the question
row shared by the M*JI photo positions of its batch row) and nn.MCBAttention built on it, forward and backward, beside the
same math composed in torch on the same device: index_add_ count sketches, torch.fft.rfft / irfft of length D, sqrt|.|
and the l2 normalisation (the route the reference's layer takes).  If this torch build has no device FFT the baseline is
the direct formulation in torch (one roll of the sketch per tap) and the record says so ("baseline": "direct").
HIP events around the forward and around the backward of each iteration; one JSON line per measurement: median / min /
max ms of each, a checksum.  The torch route's gradient at a bucket that is exactly zero is NaN (sqrt at 0): its checksum
may be NaN, its time is what is compared.

Every measurement runs in a fresh child process under a time limit (--limit seconds); this process never touches the GPU.
A child that fails or runs out of time ends the whole run: nothing more is started on the GPU after it.

Usage: python tools/bench_cbp.py [--shape N M JI idim qdim D]... [--what op attention torch_op torch_attention]
                                 [--iters 10] [--warmup 3] [--limit 240]
       (default shapes: 16 8 8 2537 100 16000, the reference's own batch (model_mcb.py:637-638), and 64 8 8 2537 100 16000)
Under a kernel trace run one child directly, one forward + backward:
       <tracer> -- python tools/bench_cbp.py --child op --shape 16 8 8 2537 100 16000 --iters 1 --warmup 0"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHAT = ["op", "attention", "torch_op", "torch_attention"]
ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=6, action="append", metavar=("N", "M", "JI", "idim", "qdim", "D"))
ap.add_argument("--what", nargs="+", default=WHAT, choices=WHAT)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limit", type=float, default=240.0)
ap.add_argument("--child", default=None, choices=WHAT)
args = ap.parse_args()
shapes = args.shape or [[16, 8, 8, 2537, 100, 16000], [64, 8, 8, 2537, 100, 16000]]

if args.child is None:
    for shape in shapes:
        for what in args.what:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--shape"] + [str(v) for v in shape] + \
                  ["--iters", str(args.iters), "--warmup", str(args.warmup)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps(dict(what=what, shape=shape, failed=rc)), flush=True)
                sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import autograd, nn, ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
N, M, JI, idim, qdim, D = shapes[0]
T, c1 = M * JI, 512
g = torch.Generator().manual_seed(N + M + JI + idim + qdim + D)
hpis = torch.relu(torch.randn(N, M, JI, idim, generator=g)).cuda().requires_grad_()
gq = (0.5 * torch.randn(N, qdim, generator=g)).cuda().requires_grad_()
tabs = ops.upload_sketch_tables(*ops.count_sketch_tables(idim, qdim, D), idim, qdim, D)
rec = dict(what=args.child, shape=[N, M, JI, idim, qdim, D], iters=args.iters)


def torch_pool(rows, q):
    """l2_normalize(sqrt|count sketch of the outer product|) composed in torch: rows [N*T, idim], q [N, qdim] -> [N*T, D]"""
    h1, s1, h2, s2 = (t.long() if t.dtype == torch.int32 else t for t in tabs)
    sk1 = torch.zeros(rows.shape[0], D, device=rows.device).index_add_(1, h1, rows * s1)
    if rec["baseline"] == "fft":
        sk2 = torch.zeros(N, D, device=rows.device).index_add_(1, h2, q * s2)
        z = torch.fft.irfft(torch.fft.rfft(sk1).reshape(N, T, -1) * torch.fft.rfft(sk2)[:, None, :], n=D).reshape(N * T, D)
    else:
        z = torch.zeros_like(sk1).reshape(N, T, D)
        for j in range(qdim):
            z = z + (q[:, j] * s2[j])[:, None, None] * torch.roll(sk1.reshape(N, T, D), int(h2[j]), 2)
        z = z.reshape(N * T, D)
    w = z.abs().sqrt()
    return w * torch.rsqrt(torch.clamp((w * w).sum(1, keepdim=True), min=1e-12))


if args.child.startswith("torch"):
    try:
        torch.fft.irfft(torch.fft.rfft(torch.ones(2, D, device="cuda")), n=D).sum().item()
        rec["baseline"] = "fft"
    except RuntimeError as e:
        rec["baseline"], rec["no_device_fft"] = "direct", str(e).splitlines()[0][:120]

if args.child in ("op", "torch_op"):
    g_out = torch.randn(N * T, D, generator=g).cuda()
    params = []
    if args.child == "op":
        fwd = lambda: autograd.compact_bilinear(hpis.reshape(N * T, idim), gq, *tabs, D, P=T, normalize=True)
    else:
        fwd = lambda: torch_pool(hpis.reshape(N * T, idim), gq)
    bwd = lambda out: out.backward(g_out)
else:
    att_mod = nn.MCBAttention(idim, qdim, mcb_outdim=D, conv1_out=c1, seed=1)
    params = list(att_mod.parameters())
    g_att, g_w = torch.randn(N, idim, generator=g).cuda(), torch.randn(N, T, generator=g).cuda()
    if args.child == "attention":
        fwd = lambda: att_mod(hpis, gq)
    else:
        def fwd():
            pooled = torch_pool(hpis.reshape(N * T, idim), gq)
            c2 = torch.relu(torch.relu(pooled @ att_mod.p("filter_conv1")) @ att_mod.p("filter_conv2"))
            att = torch.softmax(c2.reshape(N, T), 1)
            return (hpis.reshape(N, T, idim) * att[:, :, None]).sum(1), att
    bwd = lambda out: torch.autograd.backward(out, (g_att, g_w))

for _ in range(args.warmup):
    bwd(fwd())
t_fwd, t_bwd = [], []
for _ in range(args.iters):
    for p in params + [hpis, gq]:
        p.grad = None
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    res = fwd()
    e1.record()
    bwd(res)
    e2.record()
    torch.cuda.synchronize()
    t_fwd.append(e0.elapsed_time(e1))
    t_bwd.append(e1.elapsed_time(e2))
first = res[0] if isinstance(res, tuple) else res
for name, ts in (("fwd", t_fwd), ("bwd", t_bwd)):
    rec.update({name + "_ms_median": round(statistics.median(ts), 3), name + "_ms_min": round(min(ts), 3),
                name + "_ms_max": round(max(ts), 3)})
rec.update(out_sum=float(first.detach().double().sum()), dgq_sum=float(gq.grad.double().sum()))
print(json.dumps(rec), flush=True)
