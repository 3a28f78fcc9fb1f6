"""Times forward + backward of the GRU sequence op (autograd.gru_seq: out and h_last both in the loss, random lengths), of
nn.DMNPlusHead (fusion of the facts -> episodic memory, 3 hops -> choice logits) and, for orientation, of torch.nn.GRU on
the same device at the same sizes (another candidate form -- r applied after the state-side product -- with the same
products; whatever backend torch picks).  HIP events around each iteration; one JSON line per measurement: median / min /
max ms, the regime and launch counts the library's plan reports, a checksum.

Every measurement runs in a fresh child process under a time limit (--limit seconds); this process never touches the GPU.
A child that fails or runs out of time ends the whole run: nothing more is started on the GPU after it.

Usage: python tools/bench_gru_seq.py [--shape N T in d]... [--what op head torch] [--iters 10] [--warmup 3] [--limit 240]
       (default shapes: 64 192 100 100 and 64 192 512 512, the reference's DMN+ batch at its default and at the README
       hidden size; the head takes F = T facts of width d)
Under a kernel trace run one child directly, one forward + backward:
       <tracer> -- python tools/bench_gru_seq.py --child op --shape 64 192 100 100 --iters 1 --warmup 0"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("N", "T", "in", "d"))
ap.add_argument("--what", nargs="+", default=["op", "head", "torch"], choices=["op", "head", "torch"])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limit", type=float, default=240.0)
ap.add_argument("--child", default=None, choices=["op", "head", "torch"])
args = ap.parse_args()
shapes = args.shape or [[64, 192, 100, 100], [64, 192, 512, 512]]

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
N, T, din, d = shapes[0]
g = torch.Generator().manual_seed(N + T + din + d)
x = (torch.randn(N, T, din, generator=g) * 0.5).cuda().requires_grad_()
lens = torch.randint(1, T + 1, (N,), generator=g)
rec = dict(what=args.child, shape=[N, T, din, d], iters=args.iters)

if args.child == "op":
    enc = nn.GRUEncoder(din, d, seed=1)
    g_out, g_last = torch.randn(N, T, d, generator=g).cuda(), torch.randn(N, d, generator=g).cuda()
    lens_dev = lens.to(torch.int32).cuda()
    params = list(enc.parameters())

    def step():
        out, last = autograd.gru_seq(x, lens_dev, None, *(enc.p(n) for n in nn._GRU_VARS))
        torch.autograd.backward((out, last), (g_out, g_last))
        return last

    rec["plan"] = ops.gru_seq_plan(N, T, din, d)
elif args.child == "head":
    head = nn.DMNPlusHead(d, 3, seed=1)
    lq = (torch.randn(N, d, generator=g) * 0.5).cuda().requires_grad_()
    lch = (torch.randn(N, 4, d, generator=g) * 0.5).cuda().requires_grad_()
    x = (torch.randn(N, T, d, generator=g) * 0.5).cuda().requires_grad_()
    g_logits = torch.randn(N, 4, generator=g).cuda()
    params = list(head.parameters()) + [lq, lch]

    def step():
        logits = head(lq, lch, x, lens)
        logits.backward(g_logits)
        return logits

    rec["plan"] = ops.gru_seq_plan(N, T, d, d)
    rec["memory_plan"] = ops.attgru_seq_plan(N, T, d)
else:
    gru = torch.nn.GRU(din, d, batch_first=True).cuda()
    g_out = torch.randn(N, T, d, generator=g).cuda()
    params = list(gru.parameters())

    def step():
        out, last = gru(x)
        out.backward(g_out)
        return last

for _ in range(args.warmup):
    step()
times = []
for _ in range(args.iters):
    for p in params + [x]:
        p.grad = None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = step()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
rec.update(ms_median=round(statistics.median(times), 3), ms_min=round(min(times), 3), ms_max=round(max(times), 3),
           out_sum=float(res.detach().double().sum()))
print(json.dumps(rec), flush=True)
