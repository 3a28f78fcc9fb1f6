"""Times the pooled focal attention with the album pool held in fp32 and held in bf16, on the SAME bf16-valued rows (the
fp32 pool is the bf16 pool widened, so both calls compute the same bits), unwarped and under the time warp:
  fp32 / bf16        ops.PooledFocalAttention.forward        (fvta_attn_pool_fwd / fvta_attn_pool_fwd_bf16)
  fp32_tw / bf16_tw  ops.PooledWarpedFocalAttention.forward  (fvta_attn_pool_fwd_tw / fvta_attn_pool_fwd_tw_bf16), warp type 5,
                     window 3.0, the pool's energy [P,JX] computed beforehand and kept, as nn.AlbumPool keeps it
  fp32_energy / bf16_energy   album_energy alone: the one pass over the whole pool (fvta_attn_pool_energy[_bf16])
The shapes are tools/bench_attn_pooled.py's: users own --owned albums each (8), every question lists M = 4 of its user's,
drawn with the seed; P = users * owned.  HIP events around each call, --warmup calls first, then --iters timed ones; every
case runs in a fresh child process under a time limit, this process never touches the GPU, and a child that fails or runs
out of time ends the run.  One JSON line per case (median / min / max ms of each route, the bytes each pool holds, whether
the two dtypes gave the same bits) goes to stdout and is appended to --out (default
profiles/attn_pooled_bf16_bench.jsonl).  Both masks are given and all ones: every row is read.

Usage: python tools/bench_attn_pooled_bf16.py [--case USERS QPU w]... [--iters 10] [--warmup 3] [--limit 240] [--out FILE]
       (default cases: (8, 8), (8, 32), (64, 1) users x questions per user at w = 512 and at w = 1024;
        K = 6, JX = 300, M = 4, JQ = 30, simiMatrix 2 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_pooled_bf16.py --child --case 8 8 512 --iters 1 --warmup 0"""
import json
import sys

import _album_bench as ab

K, JX, M, JQ, SIMI, OWNED, WARP, WINDOW = 6, 300, 4, 30, 2, 8, 5, 3.0
args = ab.parse(("USERS", "QPU", "w"), [[U, qpu, w] for w in (512, 1024) for U, qpu in ((8, 8), (8, 32), (64, 1))], 240.0,
                "attn_pooled_bf16_bench.jsonl")
if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
U, QPU, w = args.cases[0]
P, NQ, T = U * OWNED, U * QPU, M * JX
(pool16, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b), pmask, qmask, lists_host = ab.pooled_inputs(
    ("pool_bf16", "hq", "lq", "W_flat", "b", "WH_W", "WH_b", "WC_W", "WC_b"), (U, QPU, w), K, JX, M, JQ, OWNED)
pool32 = pool16.float()                 # the same values: what a holder that insists on fp32 keeps
lists = ops.check_album_lists(lists_host, P, True).cuda()

pooled = ops.PooledFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False)
pooled_tw = ops.PooledWarpedFocalAttention(P, NQ, M, K, JX, JQ, w, SIMI, False, WARP, WINDOW)
energy = {id(p): pooled_tw.album_energy(p, WH_W, WC_W) for p in (pool32, pool16)}     # kept, as nn.AlbumPool keeps it


def fwd(pool):
    return pooled.forward(pool, pmask, hq, qmask, lists, W, b)[0]


def fwd_tw(pool):
    return pooled_tw.forward(pool, pmask, energy[id(pool)], hq, qmask, lq, lists, W, b, WH_b, WC_W, WC_b)[0]


routes = {
    "fp32": lambda: fwd(pool32), "bf16": lambda: fwd(pool16),
    "fp32_tw": lambda: fwd_tw(pool32), "bf16_tw": lambda: fwd_tw(pool16),
    "fp32_energy": lambda: pooled_tw.album_energy(pool32, WH_W, WC_W), "bf16_energy": lambda: pooled_tw.album_energy(pool16, WH_W, WC_W),
}
rec = dict(users=U, questions_per_user=QPU, owned=OWNED, P=P, NQ=NQ, M=M, K=K, JX=JX, T=T, JQ=JQ, w=w, simi=SIMI, warp_type=WARP,
           window_t=WINDOW, iters=args.iters, warmup=args.warmup, plan=pooled.plan(),
           pool_bytes_fp32=pool32.numel() * pool32.element_size(), pool_bytes_bf16=pool16.numel() * pool16.element_size())
out = {}
for name, fn in routes.items():
    out[name], ts = ab.time_route(fn, args.iters, args.warmup)
    ab.record_ms(rec, name, ts)
rec["same_bits"] = bool(torch.equal(out["fp32"], out["bf16"]) and torch.equal(out["fp32_tw"], out["bf16_tw"])
                        and torch.equal(out["fp32_energy"], out["bf16_energy"]))
rec["h_a_sum"] = float(out["bf16"].double().sum())
print(json.dumps(rec), flush=True)
