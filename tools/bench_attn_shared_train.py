"""Times the focal attention's forward + backward for NQ questions over A albums two ways, on the same inputs and the same
incoming gradient d_h_a:
  (a) shared    ops.SharedFocalAttention.forward_train + backward: rows and row gradient stay [A,K,T,w]
                (fvta_attn_shared_fwd_train / fvta_attn_shared_bwd)
  (b) expand    the per-question route: index_select of the rows and their mask to [NQ,K,T,w], ops.FocalAttention forward
                + backward (accumulate 0), index_add_ of the [NQ,K,T,w] row gradient into [A,K,T,w]
The two routes ALTERNATE inside one process (a, b, a, b, ...): HIP events around each whole route, --warmup rounds first,
then --iters timed ones.  Every case runs in a fresh child process under a time limit, this process never touches the
GPU, and a child that fails or runs out of time ends the run.  One JSON line per case goes to stdout and is appended to
--out (default profiles/attn_shared_train_bench.jsonl): median / min / max ms per route, the largest differences of the
four gradients between the routes, and the peak allocated bytes of each route (torch.cuda.max_memory_allocated over one
call, the inputs included).  Both masks are given and all ones: every row is read and written.

Usage: python tools/bench_attn_shared_train.py [--case A QPA w]... [--iters 10] [--warmup 3] [--limit 300] [--out FILE]
       (default cases: (8, 8), (2, 32), (16, 4), (64, 1) albums x questions per album at w = 1024, (8, 8) and (2, 32) at
        w = 512; K = 6, T = 1200, JQ = 30, simiMatrix 2 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_shared_train.py --child --case 8 8 1024 --iters 1 --warmup 0 --only shared"""
import json
import sys

import _album_bench as ab

K, T, JQ, SIMI = 6, 1200, 30, 2
args = ab.parse(("A", "QPA", "w"), [[8, 8, 1024], [2, 32, 1024], [16, 4, 1024], [64, 1, 1024], [8, 8, 512], [2, 32, 512]], 300.0,
                "attn_shared_train_bench.jsonl", only=("shared", "expand"))
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
A, QPA, w = args.cases[0]
NQ = A * QPA
(hall, hq, W, b, gout), hmask, qmask, album_host = ab.shared_inputs(("hall", "hq", "W", "b", "gout"), (A, QPA, w), K, T, JQ)
album = ops.check_album_index(album_host, A).cuda()
album64 = album.long()

shared = ops.SharedFocalAttention(A, NQ, K, T, JQ, w, SIMI, False)
per_q = ops.FocalAttention(NQ, K, T, JQ, w, SIMI, False)


def route_shared():
    shared.forward_train(hall, hmask, hq, qmask, album, W, b)
    dh, dq = torch.empty_like(hall), torch.empty_like(hq)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    shared.backward(hall, hmask, hq, qmask, album, W, b, gout, dh, dq, dW, db)
    return dh, dq, dW, db


def route_expand():
    he, hme = hall.index_select(0, album64), hmask.index_select(0, album64)
    per_q.forward(he, hq, hme, qmask, W, b)
    dhe, dq = torch.empty_like(he), torch.empty_like(hq)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    per_q.backward(he, hq, hme, qmask, W, b, gout, dhe, dq, dW, db, 0)
    dh = torch.zeros_like(hall).index_add_(0, album64, dhe)
    return dh, dq, dW, db


routes = {"shared": route_shared, "expand": route_expand}
if args.only:
    routes = {args.only: routes[args.only]}
rec = dict(A=A, questions_per_album=QPA, NQ=NQ, K=K, T=T, JQ=JQ, w=w, simi=SIMI, iters=args.iters, plan=shared.plan(),
           bwd_plan=shared.bwd_plan())
out = ab.peak_bytes(routes, rec)
ab.time_alternating(routes, rec, args.iters, args.warmup)       # a, b, a, b, ...
if len(out) == 2:
    ab.grad_diffs(rec, ("d_hinfo", "d_hq", "dW", "db"), out["shared"], out["expand"])
print(json.dumps(rec), flush=True)
