"""Times the focal attention of NQ questions that each list M albums of their user's pooled albums UNDER THE TIME WARP
(use_time_warp, warp type 5), four ways on the same inputs:
  (a) pooled_held    ops.PooledWarpedFocalAttention.forward with the pool's energy [P,JX] computed beforehand and kept
                     (fvta_attn_pool_fwd_tw): every encoded album held once, pool [P,K,JX,w], no expanded or warped tensor
  (b) pooled_energy  album_energy + forward in every call: the energy recomputed (one more pass over the pool)
  (c) expand         the existing route: gather the listed albums' rows and mask to [NQ,K,M*JX,w], ops.TimeWarp.forward
                     into a warped tensor of that size, then ops.FocalAttention.forward with the default kernel selection
  (d) unwarped       ops.PooledFocalAttention.forward (fvta_attn_pool_fwd) in the same process: (a) - (d) is what the warp
                     costs over the pool
Users own --owned albums each (8) and every question lists M = 4 of its user's, drawn with the seed; P = users * owned:
tools/bench_attn_pooled.py's lists.  HIP events around each call, --warmup calls first, then --iters timed ones; every case
runs in a fresh child process under a time limit, this process never touches the GPU, and a child that fails or runs out
of time ends the run.  One JSON line per case (median / min / max ms of each route, the bytes each route holds in rows --
the pool, the expanded rows and their warp --, the largest |h_a| difference between (a) and (c), absolute and relative to
the largest |h_a|) goes to stdout and is appended to --out (default profiles/attn_pooled_tw_bench.jsonl).  Both masks are
given and all ones: every row is read.

Usage: python tools/bench_attn_pooled_tw.py [--case USERS QPU w]... [--iters 10] [--warmup 3] [--limit 240] [--out FILE]
       (default cases: (8, 8), (8, 32), (64, 1) users x questions per user at w = 512 and at w = 1024;
        K = 6, JX = 300, M = 4, JQ = 30, simiMatrix 2, warp type 5, window 3.0 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_pooled_tw.py --child --case 8 8 512 --iters 1 --warmup 0"""
import json
import sys

import _album_bench as ab

K, JX, M, JQ, SIMI, OWNED, WARP, WINDOW = 6, 300, 4, 30, 2, 8, 5, 3.0
args = ab.parse(("USERS", "QPU", "w"), [[U, qpu, w] for w in (512, 1024) for U, qpu in ((8, 8), (8, 32), (64, 1))], 240.0,
                "attn_pooled_tw_bench.jsonl")
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
U, QPU, w = args.cases[0]
P, NQ, T = U * OWNED, U * QPU, M * JX
(pool, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b), pmask, qmask, lists_host = ab.pooled_inputs(
    ("pool", "hq", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b"), (U, QPU, w), K, JX, M, JQ, OWNED)
lists = ops.check_album_lists(lists_host, P, True).cuda()
lists64 = lists.long()

pooled_tw = ops.PooledWarpedFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False, WARP, WINDOW)
pooled = ops.PooledFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False)
warp = ops.TimeWarp(NQ, K, T, w, WARP, WINDOW)
per_q = ops.FocalAttention(NQ, K, T, JQ, w, SIMI, False)
warped = torch.empty(NQ, K, T, w, device="cuda", dtype=torch.float32)
energy = pooled_tw.album_energy(pool, WH_W, WC_W)


def fwd(e):
    return pooled_tw.forward(pool, pmask, e, hq, qmask, lq, lists, W, b, WH_b, WC_W, WC_b)[0]


def expand():
    """gather to [NQ,K,M*JX,w] (and the mask), warp into a second tensor of that size, attend per question"""
    rows, mask = ab.gather_lists(pool, pmask, lists64)
    warp.forward(rows, lq, WH_W, WH_b, WC_W, WC_b, warped)
    return per_q.forward(warped, hq, mask, qmask, W, b)[0]


routes = {
    "pooled_held": lambda: fwd(energy),
    "pooled_energy": lambda: fwd(pooled_tw.album_energy(pool, WH_W, WC_W)),
    "expand": expand,
    "unwarped": lambda: pooled.forward(pool, pmask, hq, qmask, lists, W, b)[0],
}
row_bytes = K * JX * w * 4
rec = dict(users=U, questions_per_user=QPU, owned=OWNED, P=P, NQ=NQ, M=M, K=K, JX=JX, T=T, JQ=JQ, w=w, simi=SIMI, warp_type=WARP,
           window_t=WINDOW, iters=args.iters, warmup=args.warmup, plan=pooled_tw.plan(), pool_bytes=P * row_bytes,
           energy_bytes=P * JX * 4, expanded_bytes=NQ * M * row_bytes, expand_route_rows_bytes=2 * NQ * M * row_bytes)
out = {}
for name, fn in routes.items():
    out[name], ts = ab.time_route(fn, args.iters, args.warmup)
    ab.record_ms(rec, name, ts)
top = float(out["expand"].abs().max())
rec["max_abs_diff_pooled_vs_expand"] = float((out["pooled_held"] - out["expand"]).abs().max())
rec["max_abs_diff_pooled_vs_expand_over_max_abs"] = rec["max_abs_diff_pooled_vs_expand"] / top
rec["held_equals_recomputed"] = bool(torch.equal(out["pooled_held"], out["pooled_energy"]))
rec["h_a_sum"] = float(out["pooled_held"].double().sum())
print(json.dumps(rec), flush=True)
