"""Times the focal attention of NQ questions over A albums three ways, on the same inputs:
  (a) shared    ops.SharedFocalAttention.forward: the albums' rows [A,K,T,w] held once (fvta_attn_shared_fwd)
  (b) expand    today's route: index_select of the rows and their mask to [NQ,K,T,w], then ops.FocalAttention.forward with
                the default kernel selection
  (c) per_q     that forward alone, on a tensor expanded beforehand
HIP events around each call, --warmup calls first, then --iters timed ones; every case runs in a fresh child process under
a time limit, this process never touches the GPU, and a child that fails or runs out of time ends the run.  One JSON line
per case (median / min / max ms of each route, the largest |h_a| difference between (a) and (c)) goes to stdout and is
appended to --out (default profiles/attn_shared_bench.jsonl).  Both masks are given and all ones: every row is read.

Usage: python tools/bench_attn_shared.py [--case A QPA w]... [--iters 10] [--warmup 3] [--limit 240] [--out FILE]
       (default cases: (8, 8), (64, 1), (2, 32) albums x questions per album at w = 1024 and at w = 512;
        K = 6, T = 1200, JQ = 30, simiMatrix 2 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_shared.py --child --case 8 8 1024 --iters 1 --warmup 0"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, T, JQ, SIMI = 6, 1200, 30, 2
ap = argparse.ArgumentParser()
ap.add_argument("--case", type=int, nargs=3, action="append", metavar=("A", "QPA", "w"))
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limit", type=float, default=240.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_shared_bench.jsonl"))
ap.add_argument("--child", action="store_true")
args = ap.parse_args()
cases = args.case or [[A, qpa, w] for w in (1024, 512) for A, qpa in ((8, 8), (64, 1), (2, 32))]

if not args.child:
    for case in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case"] + [str(v) for v in case] + \
              ["--iters", str(args.iters), "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
            rc, line = p.returncode, p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
        except subprocess.TimeoutExpired:
            rc, line = 124, ""
        if rc != 0:
            print(json.dumps(dict(case=case, failed=rc)), flush=True)
            sys.exit(rc)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0)

sys.path.insert(0, ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
A, QPA, w = cases[0]
NQ = A * QPA
g = torch.Generator().manual_seed(A * 1000 + QPA + w)
hall = (torch.randn(A, K, T, w, generator=g) * 0.5).cuda()
hq = (torch.randn(NQ, JQ, w, generator=g) * 0.5).cuda()
W = (torch.randn(2 * w, generator=g) * 0.1).cuda()
b = (torch.randn(1, generator=g) * 0.1).cuda()
hmask = torch.ones(A, K, T, dtype=torch.uint8, device="cuda")
qmask = torch.ones(NQ, JQ, dtype=torch.uint8, device="cuda")
album_host = torch.arange(A).repeat_interleave(QPA)[torch.randperm(NQ, generator=g)]
album = ops.check_album_index(album_host, A).cuda()
album64 = album.long()

shared = ops.SharedFocalAttention(A, NQ, K, T, JQ, w, SIMI, False)
per_q = ops.FocalAttention(NQ, K, T, JQ, w, SIMI, False)
expanded, expanded_mask = hall.index_select(0, album64), hmask.index_select(0, album64)
routes = {
    "shared": lambda: shared.forward(hall, hmask, hq, qmask, album, W, b)[0],
    "expand": lambda: per_q.forward(hall.index_select(0, album64), hq, hmask.index_select(0, album64), qmask, W, b)[0],
    "per_q": lambda: per_q.forward(expanded, hq, expanded_mask, qmask, W, b)[0],
}
rec = dict(A=A, questions_per_album=QPA, NQ=NQ, K=K, T=T, JQ=JQ, w=w, simi=SIMI, iters=args.iters, plan=shared.plan())
out = {}
for name, fn in routes.items():
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out[name] = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    rec.update({name + "_ms_median": round(statistics.median(ts), 3), name + "_ms_min": round(min(ts), 3),
                name + "_ms_max": round(max(ts), 3)})
rec["max_abs_diff_shared_vs_per_q"] = float((out["shared"] - out["per_q"]).abs().max())
rec["h_a_sum"] = float(out["shared"].double().sum())
print(json.dumps(rec), flush=True)
