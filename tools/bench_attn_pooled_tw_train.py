"""Times the focal attention's forward + backward UNDER THE TIME WARP for NQ questions that each list M albums of their
user's pooled albums three ways, on the same inputs and the same incoming gradient d_h_a:
  (a) pooled_energy  ops.PooledWarpedFocalAttention.album_energy + forward_train + backward: rows and row gradient stay
                [P,K,JX,w] (fvta_attn_pool_energy / fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw).  This is the
                training step's figure: the pool's rows change with every step, and the energy e [P,JX] with them
  (a') pooled   the same with the energy held from outside the timed region (rows that do not change between calls:
                several batches of questions over one encoded pool)
  (b) expand    the per-question route: gather the listed albums' rows and mask to [NQ,K,M*JX,w], autograd.time_warp
                (nn.TimeWarp's op), autograd.focal_attention (nn.FocalAttention3D.forward's op), backward() -- the gathered
                rows, their warp and both gradients are [NQ,K,M*JX,w] each, and the gather's own backward index_add_s the
                last into [P,K,JX,w]
Users own --owned albums each (8) and every question lists M = 4 of its user's, drawn with the seed; P = users * owned.
The routes ALTERNATE inside one process (a, a', b, a, a', b, ...): HIP events around each whole route, --warmup rounds
first, then --iters timed ones.  Every case runs in a fresh child process under a time limit, this process never touches the
GPU, and a child that fails or runs out of time ends the run.  One JSON line per case goes to stdout and is appended to
--out (default profiles/attn_pooled_tw_train_bench.jsonl): median / min / max ms per route, the largest differences of the
nine gradients between the routes, and the peak allocated bytes of each route (torch.cuda.max_memory_allocated over one
call, the inputs included).  Both masks are given and all ones: every row is read and written.  Run the tool twice in a
row on one box and compare the ranges of both runs before calling a winner.

Usage: python tools/bench_attn_pooled_tw_train.py [--case USERS QPU w]... [--iters 10] [--warmup 3] [--limit 300] [--out FILE]
       (default cases: (8, 8), (8, 32), (64, 1) users x questions per user at w = 512 and at w = 1024;
        K = 6, JX = 300, M = 4, JQ = 30, simiMatrix 2, warp type 5, window 3 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_pooled_tw_train.py --child --case 8 8 512 --iters 1 --warmup 0 --only pooled"""
import json
import sys

import _album_bench as ab

K, JX, M, JQ, SIMI, OWNED, WARP, WINDOW = 6, 300, 4, 30, 2, 8, 5, 3.0
args = ab.parse(("USERS", "QPU", "w"), [[U, qpu, w] for w in (512, 1024) for U, qpu in ((8, 8), (8, 32), (64, 1))], 300.0,
                "attn_pooled_tw_train_bench.jsonl", only=("pooled_energy", "pooled", "expand"))
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import autograd, ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
U, QPU, w = args.cases[0]
P, NQ, T = U * OWNED, U * QPU, M * JX
# W_band: logits of order 1 at every width under the warp's band (tests/_attn_pool_tw_bwd_ref.py's recipe)
(pool, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b, gout), pmask, qmask, lists_host = ab.pooled_inputs(
    ("pool", "hq", "lq", "W_band", "b", "WH_W", "WH_b", "WC_W", "WC_b", "gout"), (U, QPU, w), K, JX, M, JQ, OWNED)
lists = ops.check_album_lists(lists_host, P, True).cuda()
lists64 = lists.long()

pooled = ops.PooledWarpedFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False, WARP, WINDOW)
energy = pooled.album_energy(pool, WH_W, WC_W)      # held: it belongs to the pool and the warp's weights


def route_pooled(e=None):
    e = energy if e is None else e
    pooled.forward_train(pool, pmask, e, hq, qmask, lq, lists, W, b, WH_b, WC_W, WC_b)
    dp, dq, dlq = torch.empty_like(pool), torch.empty_like(hq), torch.empty_like(lq)
    acc = tuple(torch.zeros_like(t) for t in (W, b, WH_W, WH_b, WC_W, WC_b))
    pooled.backward(pool, pmask, hq, qmask, lq, lists, W, b, WH_W, WH_b, WC_W, WC_b, gout, dp, dq, dlq, *acc)
    return (dp, dq, dlq) + acc


def route_pooled_energy():
    return route_pooled(pooled.album_energy(pool, WH_W, WC_W))


def route_expand():
    leaves = [t.detach().requires_grad_() for t in (pool, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b)]
    p_, q, l, W_, b_, WH_, WHb_, WC_, WCb_ = leaves
    rows, mask = ab.gather_lists(p_, pmask, lists64)
    warped, _ = autograd.time_warp(rows, l, WH_, WHb_, WC_, WCb_, WARP, WINDOW)
    h_a, _ = autograd.focal_attention(warped, q, W_, b_, mask, qmask, SIMI, False)
    h_a.backward(gout)
    return tuple(t.grad for t in leaves)


routes = {"pooled_energy": route_pooled_energy, "pooled": route_pooled, "expand": route_expand}
if args.only:
    routes = {args.only: routes[args.only]}
row_bytes = K * JX * w * 4
rec = dict(users=U, questions_per_user=QPU, owned=OWNED, P=P, NQ=NQ, M=M, K=K, JX=JX, T=T, JQ=JQ, w=w, simi=SIMI,
           warp_type=WARP, window_t=WINDOW, iters=args.iters, plan=pooled.plan(), bwd_plan=pooled.bwd_plan(),
           pool_bytes=P * row_bytes, expanded_bytes=NQ * M * row_bytes)
out = ab.peak_bytes(routes, rec)
ab.time_alternating(routes, rec, args.iters, args.warmup)       # a, a', b, a, a', b, ...
if "pooled" in out and "expand" in out:
    ab.grad_diffs(rec, ("d_pool", "d_hq", "d_lq", "dW", "db", "dWH_W", "dWH_b", "dWC_W", "dWC_b"), out["pooled"], out["expand"])
print(json.dumps(rec), flush=True)
