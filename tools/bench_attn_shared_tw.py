"""Times the focal attention of NQ questions over A albums UNDER THE TIME WARP (use_time_warp, warp type 5) three ways, on
the same inputs:
  (a) shared_held    ops.SharedWarpedFocalAttention.forward with the albums' energy [A,T] computed beforehand and kept
                     (fvta_attn_shared_fwd_tw): the rows [A,K,T,w] held once, no warped tensor
  (b) shared_energy  album_energy + forward in every call: the energy recomputed (one more pass over the rows)
  (c) expand         the existing route: index_select of the rows and their mask to [NQ,K,T,w], ops.TimeWarp.forward into a
                     warped [NQ,K,T,w], then ops.FocalAttention.forward with the default kernel selection
HIP events around each call, --warmup calls first, then --iters timed ones; every case runs in a fresh child process under
a time limit, this process never touches the GPU, and a child that fails or runs out of time ends the run.  One JSON line
per case (median / min / max ms and the algorithmic bytes of each route, the largest |h_a| difference between (a) and (c)
relative to the largest |h_a|) goes to stdout and is appended to --out (default profiles/attn_shared_tw_bench.jsonl).  Both
masks are given and all ones: every row is read.

Algorithmic bytes (what the route must move, from the shapes; caches may save some of it, a kernel may move more):
  shared_held    rows 2 x groups x K T w x 4 (logits and weighted sum, once per group of <= G questions of an album) + the
                 questions + energy, scale, the max-pooled logits written and read + h_a
  shared_energy  that + the rows once more (A K T w x 4) + WH/W's first w rows
  expand         the gather reads and writes NQ K T w x 4, the warp reads and writes it, the attention reads it at least
                 once: 5 x NQ K T w x 4, + the questions + h_a

Usage: python tools/bench_attn_shared_tw.py [--case A QPA w]... [--iters 10] [--warmup 3] [--limit 240] [--out FILE]
       (default cases: (8, 8) and (64, 1) albums x questions per album at w = 512; K = 6, T = 1200, JQ = 30, simiMatrix 2,
        warp type 5, window 3.0 throughout: tools/bench_attn_shared.py's shape)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_shared_tw.py --child --case 8 8 512 --iters 1 --warmup 0"""
import json
import sys

import _album_bench as ab

K, T, JQ, SIMI, WARP, WINDOW = 6, 1200, 30, 2, 5, 3.0
args = ab.parse(("A", "QPA", "w"), [[8, 8, 512], [64, 1, 512]], 240.0, "attn_shared_tw_bench.jsonl")


def algorithmic_bytes(A, QPA, w, G):
    """{route: bytes} from the shapes alone (see the module docstring)"""
    NQ = A * QPA
    groups = A * -(-QPA // G)
    row = K * T * w * 4
    small = NQ * JQ * w * 4 + NQ * w * 4 * 2                       # hq, lq, h_a
    held = 2 * groups * row + small + A * T * 4 + NQ * T * 4 * 3 + NQ * K * T * 4 * 3
    return dict(shared_held=held, shared_energy=held + A * row + w * w * 4, expand=5 * NQ * row + small)


if not args.child:
    sys.exit(ab.run_parent(__file__, args))

sys.path.insert(0, ab.ROOT)
import torch  # noqa: E402
from fvta_memexqa_amd import ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
A, QPA, w = args.cases[0]
NQ = A * QPA
(hall, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b), hmask, qmask, album_host = ab.shared_inputs(
    ("hall", "hq", "lq", "W", "b", "WH_W", "WH_b", "WC_W", "WC_b"), (A, QPA, w), K, T, JQ)
album = ops.check_album_index(album_host, A).cuda()
album64 = album.long()

shared = ops.SharedWarpedFocalAttention(A, NQ, K, T, JQ, w, SIMI, False, WARP, WINDOW)
warp = ops.TimeWarp(NQ, K, T, w, WARP, WINDOW)
per_q = ops.FocalAttention(NQ, K, T, JQ, w, SIMI, False)
warped = torch.empty(NQ, K, T, w, device="cuda", dtype=torch.float32)
energy = shared.album_energy(hall, WH_W, WC_W)


def fwd(e):
    return shared.forward(hall, hmask, e, hq, qmask, lq, album, W, b, WH_b, WC_W, WC_b)[0]


def expand():
    warp.forward(hall.index_select(0, album64), lq, WH_W, WH_b, WC_W, WC_b, warped)
    return per_q.forward(warped, hq, hmask.index_select(0, album64), qmask, W, b)[0]


routes = {"shared_held": lambda: fwd(energy), "shared_energy": lambda: fwd(shared.album_energy(hall, WH_W, WC_W)),
          "expand": expand}
plan = ops.SharedFocalAttention(A, NQ, K, T, JQ, w, SIMI, False).plan()
rec = dict(A=A, questions_per_album=QPA, NQ=NQ, K=K, T=T, JQ=JQ, w=w, simi=SIMI, warp_type=WARP, window_t=WINDOW,
           iters=args.iters, warmup=args.warmup, plan=plan, energy_bytes=A * T * 4, rows_bytes=A * K * T * w * 4,
           expanded_rows_bytes=NQ * K * T * w * 4)
nbytes = algorithmic_bytes(A, QPA, w, plan["G"])
out = {}
for name, fn in routes.items():
    out[name], ts = ab.time_route(fn, args.iters, args.warmup)
    med = ab.record_ms(rec, name, ts)
    rec.update({name + "_algorithmic_bytes": nbytes[name], name + "_algorithmic_GBps": round(nbytes[name] / med / 1e6, 1)})
top = float(out["expand"].abs().max())
rec["max_abs_diff_shared_vs_expand_over_max_abs"] = float((out["shared_held"] - out["expand"]).abs().max()) / top
rec["held_equals_recomputed"] = bool(torch.equal(out["shared_held"], out["shared_energy"]))
rec["h_a_sum"] = float(out["shared_held"].double().sum())
print(json.dumps(rec), flush=True)
