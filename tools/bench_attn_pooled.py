"""Times the focal attention of NQ questions that each list M albums of their user's pooled albums, three ways on the same
inputs:
  (a) pooled    ops.PooledFocalAttention.forward: every encoded album held once, pool [P,K,JX,w] (fvta_attn_pool_fwd)
  (b) expand    the per-question route: gather the listed albums' rows and mask to [NQ,K,M*JX,w], then
                ops.FocalAttention.forward with the default kernel selection
  (c) shared    ops.SharedFocalAttention.forward over one context [K,M*JX,w] per DISTINCT list, built beforehand (not
                timed): the best there is without the pool and without an expansion per call
Users own --owned albums each (8) and every question lists M = 4 of its user's, drawn with the seed; P = users * owned.
HIP events around each call, --warmup calls first, then --iters timed ones; every case runs in a fresh child process under
a time limit, this process never touches the GPU, and a child that fails or runs out of time ends the run.  One JSON line
per case (median / min / max ms of each route, the bytes each route holds in rows -- the pool, the expanded rows, the
distinct contexts --, the largest |h_a| difference between (a) and (b)) goes to stdout and is appended to --out (default
profiles/attn_pooled_bench.jsonl).  Both masks are given and all ones: every row is read.

Usage: python tools/bench_attn_pooled.py [--case USERS QPU w]... [--iters 10] [--warmup 3] [--limit 240] [--out FILE]
       (default cases: (8, 8), (8, 32), (64, 1) users x questions per user at w = 512 and at w = 1024;
        K = 6, JX = 300, M = 4, JQ = 30, simiMatrix 2 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_pooled.py --child --case 8 8 512 --iters 1 --warmup 0"""
import json
import sys

import _album_bench as ab

K, JX, M, JQ, SIMI, OWNED = 6, 300, 4, 30, 2, 8
args = ab.parse(("USERS", "QPU", "w"), [[U, qpu, w] for w in (512, 1024) for U, qpu in ((8, 8), (8, 32), (64, 1))], 240.0,
                "attn_pooled_bench.jsonl")
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
U, QPU, w = args.cases[0]
P, NQ, T = U * OWNED, U * QPU, M * JX
(pool, hq, W, b), pmask, qmask, lists_host = ab.pooled_inputs(("pool", "hq", "W_flat", "b"), (U, QPU, w), K, JX, M, JQ, OWNED)
lists = ops.check_album_lists(lists_host, P, True).cuda()
lists64 = lists.long()

# (c): one context per distinct list, built beforehand
distinct, which = torch.unique(lists_host, dim=0, return_inverse=True)
D = distinct.shape[0]
d64 = distinct.cuda().reshape(-1)
contexts = pool.index_select(0, d64).reshape(D, M, K, JX, w).permute(0, 2, 1, 3, 4).reshape(D, K, T, w).contiguous()
contexts_mask = torch.ones(D, K, T, dtype=torch.uint8, device="cuda")
which_dev = ops.check_album_index(which, D).cuda()

pooled = ops.PooledFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False)
per_q = ops.FocalAttention(NQ, K, T, JQ, w, SIMI, False)
shared = ops.SharedFocalAttention(D, NQ, K, T, JQ, w, SIMI, False)


def expand():
    rows, mask = ab.gather_lists(pool, pmask, lists64)
    return per_q.forward(rows, hq, mask, qmask, W, b)[0]


routes = {
    "pooled": lambda: pooled.forward(pool, pmask, hq, qmask, lists, W, b)[0],
    "expand": expand,
    "shared": lambda: shared.forward(contexts, contexts_mask, hq, qmask, which_dev, W, b)[0],
}
row_bytes = K * JX * w * 4
rec = dict(users=U, questions_per_user=QPU, owned=OWNED, P=P, NQ=NQ, M=M, K=K, JX=JX, T=T, JQ=JQ, w=w, simi=SIMI,
           iters=args.iters, distinct_lists=D, plan=pooled.plan(), pool_bytes=P * row_bytes, expanded_bytes=NQ * M * row_bytes,
           distinct_context_bytes=D * M * row_bytes)
out = {}
for name, fn in routes.items():
    out[name], ts = ab.time_route(fn, args.iters, args.warmup)
    ab.record_ms(rec, name, ts)
rec["max_abs_diff_pooled_vs_expand"] = float((out["pooled"] - out["expand"]).abs().max())
rec["max_abs_diff_pooled_vs_shared"] = float((out["pooled"] - out["shared"]).abs().max())
rec["h_a_sum"] = float(out["pooled"].double().sum())
print(json.dumps(rec), flush=True)
