"""Times forward + backward of the whole DMN+ episodic memory (dmn.EpisodicMemory: per hop the attention MLP, the softmax
over the facts, the AttentionGRU over all F facts, the hop's dense + relu) with HIP events around each iteration, and
prints one JSON line per shape: median / min / max ms over the iterations, the regime and launch counts the library's
plan reports for the recurrence, and a checksum of the output.  dmn.EpisodicMemory keeps its interface across revisions,
so `--root <another checkout>` times that revision's package with the same script (fresh process per revision, alternated
by the caller); `--dump` writes the output and the fact gradient for a comparison between revisions.  Fails without a GPU.

Usage: python tools/bench_attgru_seq.py [--shape N F d hops]... [--iters 10] [--warmup 3] [--root DIR] [--dump FILE]
       (default shapes: 64 192 80 3 and 64 192 512 3, the reference's DMN+ batch at the test and the README hidden size)
Under a kernel trace run it with --iters 1 --warmup 0: one forward + backward per shape."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("N", "F", "d", "hops"))
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--root", default=os.getcwd())
ap.add_argument("--dump", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from fvta_memexqa_amd import dmn, ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
dumps = {}
for N, F, d, hops in (args.shape or [[64, 192, 80, 3], [64, 192, 512, 3]]):
    g = torch.Generator().manual_seed(N + F + d)
    facts = (torch.randn(N, F, d, generator=g) * 0.5).cuda()
    gq = (torch.randn(N, d, generator=g) * 0.5).cuda()
    lens = torch.randint(1, F + 1, (N,), generator=g)
    d_out = torch.randn(N, d, generator=g).cuda()
    mem = dmn.EpisodicMemory(d, hops, seed=1)

    def step():
        out = mem(gq, facts, lens)
        d_gq, d_facts = mem.backward(d_out)
        return out, d_facts

    for _ in range(args.warmup):
        step()
    times = []
    for _ in range(args.iters):
        mem.zero_grad()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, d_facts = step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    rec = dict(shape=[N, F, d, hops], iters=args.iters, ms_median=round(statistics.median(times), 3),
               ms_min=round(min(times), 3), ms_max=round(max(times), 3), out_sum=float(out.double().sum()),
               root=os.path.abspath(args.root))
    if hasattr(ops, "attgru_seq_plan"):
        rec["plan"] = ops.attgru_seq_plan(N, F, d)
    print(json.dumps(rec), flush=True)
    dumps["%d_%d_%d_%d" % (N, F, d, hops)] = dict(out=out.cpu(), d_facts=d_facts.cpu(),
                                                 dWg=mem.grads[dmn.CELL + "gates/weights"].cpu())
if args.dump:
    torch.save(dumps, args.dump)
