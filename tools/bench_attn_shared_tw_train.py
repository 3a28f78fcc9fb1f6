"""Times the focal attention's forward + backward UNDER THE TIME WARP for NQ questions over A albums two ways, on the same
inputs and the same incoming gradient d_h_a:
  (a) shared    ops.SharedWarpedFocalAttention.forward_train + backward with the albums' energy e [A,T] held: rows and row
                gradient stay [A,K,T,w] (fvta_attn_shared_fwd_tw_train / fvta_attn_shared_bwd_tw)
  (b) expand    what a user had before: index_select of the rows and their mask to [NQ,K,T,w], autograd.time_warp,
                autograd.focal_attention, backward() -- the warped rows, their gradient and the gathered rows' gradient are
                [NQ,K,T,w] each, the index_select's own backward adds the last into [A,K,T,w]
The two routes ALTERNATE inside one process (a, b, a, b, ...): HIP events around each whole route, --warmup rounds first,
then --iters timed ones.  Every case runs in a fresh child process under a time limit, this process never touches the
GPU, and a child that fails or runs out of time ends the run.  One JSON line per case goes to stdout and is appended to
--out (default profiles/attn_shared_tw_train_bench.jsonl): median / min / max ms per route, the largest differences of the
nine gradients between the routes, and the peak allocated bytes of each route (torch.cuda.max_memory_allocated over one
call, the inputs included).  Both masks are given and all ones: every row is read and written.  Run the tool twice in a
row on one box and compare the ranges of both runs before calling a winner.

Usage: python tools/bench_attn_shared_tw_train.py [--case A QPA w]... [--iters 10] [--warmup 3] [--limit 300] [--out FILE]
       (default cases: (8, 8) and (64, 1) albums x questions per album at w = 512 and w = 1024; K = 6, T = 1200, JQ = 30,
        simiMatrix 2, warp type 5, window 3 throughout)
Under a kernel trace run one child directly:
       <tracer> -- python tools/bench_attn_shared_tw_train.py --child --case 8 8 1024 --iters 1 --warmup 0 --only shared"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, T, JQ, SIMI, WARP, WINDOW = 6, 1200, 30, 2, 5, 3.0
ap = argparse.ArgumentParser()
ap.add_argument("--case", type=int, nargs=3, action="append", metavar=("A", "QPA", "w"))
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limit", type=float, default=300.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_shared_tw_train_bench.jsonl"))
ap.add_argument("--only", choices=("shared", "expand"), help="child: run one route only (kernel traces)")
ap.add_argument("--child", action="store_true")
args = ap.parse_args()
cases = args.case or [[8, 8, 512], [64, 1, 512], [8, 8, 1024], [64, 1, 1024]]

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
from fvta_memexqa_amd import autograd, ops  # noqa: E402

ops.require_gpu()                       # raises without a GPU: there is nothing to time on a CPU
A, QPA, w = cases[0]
NQ = A * QPA
g = torch.Generator().manual_seed(A * 1000 + QPA + w)
hall = (torch.randn(A, K, T, w, generator=g) * 0.5).cuda()
hq = (torch.randn(NQ, JQ, w, generator=g) * 0.5).cuda()
lq = (torch.randn(NQ, w, generator=g) * 0.5).cuda()
# logits of order 1 at every width under a band of 2 * 3 + 1 = 7 positions (tests/_attn_shared_tw_bwd_ref.py's recipe)
W = (torch.randn(2 * w, generator=g) * 0.1 * (64.0 / w) ** 0.5 / 49.0).cuda()
b = (torch.randn(1, generator=g) * 0.1).cuda()
WH_W = (torch.randn(2 * w, w, generator=g) * (0.3 / w ** 0.5)).cuda()
WH_b = (torch.randn(w, generator=g) * 0.1).cuda()
WC_W = (torch.randn(w, generator=g) * (0.5 / w ** 0.5)).cuda()
WC_b = (torch.randn(1, generator=g) * 0.1).cuda()
gout = torch.randn(NQ, w, generator=g).cuda()
hmask = torch.ones(A, K, T, dtype=torch.uint8, device="cuda")
qmask = torch.ones(NQ, JQ, dtype=torch.uint8, device="cuda")
album_host = torch.arange(A).repeat_interleave(QPA)[torch.randperm(NQ, generator=g)]
album = ops.check_album_index(album_host, A).cuda()
album64 = album.long()

shared = ops.SharedWarpedFocalAttention(A, NQ, K, T, JQ, w, SIMI, False, WARP, WINDOW)
energy = shared.album_energy(hall, WH_W, WC_W)      # held: it belongs to the albums and the warp's weights


def route_shared():
    shared.forward_train(hall, hmask, energy, hq, qmask, lq, album, W, b, WH_b, WC_W, WC_b)
    dh, dq, dlq = torch.empty_like(hall), torch.empty_like(hq), torch.empty_like(lq)
    acc = tuple(torch.zeros_like(t) for t in (W, b, WH_W, WH_b, WC_W, WC_b))
    shared.backward(hall, hmask, hq, qmask, lq, album, W, b, WH_W, WH_b, WC_W, WC_b, gout, dh, dq, dlq, *acc)
    return (dh, dq, dlq) + acc


def route_expand():
    leaves = [t.detach().requires_grad_() for t in (hall, hq, lq, W, b, WH_W, WH_b, WC_W, WC_b)]
    h, q, l, W_, b_, WH_, WHb_, WC_, WCb_ = leaves
    he, hme = h.index_select(0, album64), hmask.index_select(0, album64)
    warped, _ = autograd.time_warp(he, l, WH_, WHb_, WC_, WCb_, WARP, WINDOW)
    h_a, _ = autograd.focal_attention(warped, q, W_, b_, hme, qmask, SIMI, False)
    h_a.backward(gout)
    return tuple(t.grad for t in leaves)


routes = {"shared": route_shared, "expand": route_expand}
if args.only:
    routes = {args.only: routes[args.only]}
rec = dict(A=A, questions_per_album=QPA, NQ=NQ, K=K, T=T, JQ=JQ, w=w, simi=SIMI, warp_type=WARP, window_t=WINDOW, iters=args.iters,
           bwd_plan=shared.bwd_plan(), expanded_tensor_bytes=NQ * K * T * w * 4)
out, ts = {}, {name: [] for name in routes}
for name, fn in routes.items():         # peak memory of one call of each route, on a warm allocator
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out[name] = fn()
    torch.cuda.synchronize()
    rec[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    out[name] = tuple(t.clone() for t in out[name])
for it in range(args.warmup + args.iters):
    for name, fn in routes.items():     # alternating: a, b, a, b, ...
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        del res
        if it >= args.warmup:
            ts[name].append(e0.elapsed_time(e1))
for name, t in ts.items():
    rec.update({name + "_ms_median": round(statistics.median(t), 3), name + "_ms_min": round(min(t), 3),
                name + "_ms_max": round(max(t), 3)})
if len(out) == 2:
    for i, key in enumerate(("d_hinfo", "d_hq", "d_lq", "dW", "db", "dWH_W", "dWH_b", "dWC_W", "dWC_b")):
        x, y = out["shared"][i], out["expand"][i]
        rec["max_abs_diff_" + key] = float((x.reshape(-1) - y.reshape(-1)).abs().max())
        rec["max_abs_" + key] = float(y.abs().max())
print(json.dumps(rec), flush=True)
