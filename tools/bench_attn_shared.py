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
import json
import sys

import _album_bench as ab

K, T, JQ, SIMI = 6, 1200, 30, 2
args = ab.parse(("A", "QPA", "w"), [[A, qpa, w] for w in (1024, 512) for A, qpa in ((8, 8), (64, 1), (2, 32))], 240.0,
                "attn_shared_bench.jsonl")
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
A, QPA, w = args.cases[0]
NQ = A * QPA
(hall, hq, W, b), hmask, qmask, album_host = ab.shared_inputs(("hall", "hq", "W_flat", "b"), (A, QPA, w), K, T, JQ)
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
    out[name], ts = ab.time_route(fn, args.iters, args.warmup)
    ab.record_ms(rec, name, ts)
rec["max_abs_diff_shared_vs_per_q"] = float((out["shared"] - out["per_q"]).abs().max())
rec["h_a_sum"] = float(out["shared"].double().sum())
print(json.dumps(rec), flush=True)
