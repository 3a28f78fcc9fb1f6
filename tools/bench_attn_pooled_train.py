"""Times the focal attention's forward + backward for NQ questions that each list M albums of their user's pooled albums two
ways, on the same inputs and the same incoming gradient d_h_a:
  (a) pooled    ops.PooledFocalAttention.forward_train + backward: rows and row gradient stay [P,K,JX,w]
                (fvta_attn_pool_fwd_train / fvta_attn_pool_bwd)
  (b) expand    the per-question route: gather the listed albums' rows and mask to [NQ,K,M*JX,w], ops.FocalAttention
                forward + backward (accumulate 0), index_add_ of the [NQ,K,M*JX,w] row gradient by reference into [P,K,JX,w]
Users own --owned albums each (8) and every question lists M = 4 of its user's, drawn with the seed; P = users * owned.
The two routes ALTERNATE inside one process (a, b, a, b, ...): HIP events around each whole route, --warmup rounds first,
then --iters timed ones.  Every case runs in a fresh child process under a time limit, this process never touches the
GPU, and a child that fails or runs out of time ends the run.  One JSON line per case goes to stdout and is appended to
--out (default profiles/attn_pooled_train_bench.jsonl): median / min / max ms per route, the largest differences of the
four gradients between the routes, and the peak allocated bytes of each route (torch.cuda.max_memory_allocated over one
call, the inputs included).  Both masks are given and all ones: every row is read and written.

Usage: python tools/bench_attn_pooled_train.py [--case USERS QPU w]... [--iters 10] [--warmup 3] [--limit 300] [--out FILE]
       (default cases: (8, 8), (8, 32), (64, 1) users x questions per user at w = 512 and at w = 1024;
        K = 6, JX = 300, M = 4, JQ = 30, simiMatrix 2 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_pooled_train.py --child --case 8 8 512 --iters 1 --warmup 0 --only pooled"""
import json
import sys

import _album_bench as ab

K, JX, M, JQ, SIMI, OWNED = 6, 300, 4, 30, 2, 8
args = ab.parse(("USERS", "QPU", "w"), [[U, qpu, w] for w in (512, 1024) for U, qpu in ((8, 8), (8, 32), (64, 1))], 300.0,
                "attn_pooled_train_bench.jsonl", only=("pooled", "expand"))
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
U, QPU, w = args.cases[0]
P, NQ, T = U * OWNED, U * QPU, M * JX
(pool, hq, W, b, gout), pmask, qmask, lists_host = ab.pooled_inputs(("pool", "hq", "W", "b", "gout"), (U, QPU, w), K, JX, M, JQ,
                                                                    OWNED)
lists = ops.check_album_lists(lists_host, P, True).cuda()
lists64 = lists.long()
refs64 = lists64.reshape(-1)

pooled = ops.PooledFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False)
per_q = ops.FocalAttention(NQ, K, T, JQ, w, SIMI, False)


def route_pooled():
    pooled.forward_train(pool, pmask, hq, qmask, lists, W, b)
    dp, dq = torch.empty_like(pool), torch.empty_like(hq)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    pooled.backward(pool, pmask, hq, qmask, lists, W, b, gout, dp, dq, dW, db)
    return dp, dq, dW, db


def route_expand():
    rows, mask = ab.gather_lists(pool, pmask, lists64)
    per_q.forward(rows, hq, mask, qmask, W, b)
    drows, dq = torch.empty_like(rows), torch.empty_like(hq)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    per_q.backward(rows, hq, mask, qmask, W, b, gout, drows, dq, dW, db, 0)
    per_ref = drows.reshape(NQ, K, M, JX, w).permute(0, 2, 1, 3, 4).reshape(NQ * M, K, JX, w)
    dp = torch.zeros_like(pool).index_add_(0, refs64, per_ref)
    return dp, dq, dW, db


routes = {"pooled": route_pooled, "expand": route_expand}
if args.only:
    routes = {args.only: routes[args.only]}
row_bytes = K * JX * w * 4
rec = dict(users=U, questions_per_user=QPU, owned=OWNED, P=P, NQ=NQ, M=M, K=K, JX=JX, T=T, JQ=JQ, w=w, simi=SIMI,
           iters=args.iters, plan=pooled.plan(), bwd_plan=pooled.bwd_plan(), pool_bytes=P * row_bytes,
           expanded_bytes=NQ * M * row_bytes)
out = ab.peak_bytes(routes, rec)
ab.time_alternating(routes, rec, args.iters, args.warmup)       # a, b, a, b, ...
if len(out) == 2:
    ab.grad_diffs(rec, ("d_pool", "d_hq", "dW", "db"), out["pooled"], out["expand"])
print(json.dumps(rec), flush=True)
