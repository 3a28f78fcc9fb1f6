"""What the nine album attention benchmark tools (tools/bench_attn_shared*.py, tools/bench_attn_pooled*.py) have in common:
the argument parser, the parent loop that runs every case in a fresh child process under a time limit, the seeded inputs,
the pooled gather, the two HIP-event timing loops, the peak-memory bracket and the record fields they all write.  Each tool
keeps its docstring (the documented method), its constants and cases, its route functions and its record's own fields.
The parent side (parse, run_parent) imports neither torch nor the package and never touches the GPU; every other function
is the child's and imports torch when it is called."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(metavar, cases, limit, out, only=None, argv=None):
    """the tools' command line; `metavar` names --case's three ints, `cases` are the default cases, `out` the default file
    under profiles/, `only` the routes a child may be restricted to (tools that time alternating routes).  The cases to
    run are in .cases"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, nargs=3, action="append", metavar=metavar)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=limit)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    if only:
        ap.add_argument("--only", choices=only, help="child: run one route only (kernel traces)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args(argv)
    args.cases = args.case or cases
    return args


def run_parent(script, args):
    """every case of args.cases in a fresh child of `script` under args.limit seconds; a child's last stdout line is echoed
    and appended to args.out.  A child that fails (running out of time is status 124) ends the run: returns its status"""
    for case in args.cases:
        cmd = [sys.executable, os.path.abspath(script), "--child", "--case"] + [str(v) for v in case] + \
              ["--iters", str(args.iters), "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
            rc, line = p.returncode, p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
        except subprocess.TimeoutExpired:
            rc, line = 124, ""
        if rc != 0:
            print(json.dumps(dict(case=case, failed=rc)), flush=True)
            return rc
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


# name in a tool's draw order -> (shape, how the standard normal draw is scaled).  A shape names its sizes ("rows": the
# album rows' own shape).  The scalings stand as the tools published them: each `*` and `/` on the tensor rounds to fp32,
# so regrouping one would change h_a_sum and the difference fields.
_DRAWS = {
    "hall": ("rows", lambda t, w: t * 0.5),
    "pool": ("rows", lambda t, w: t * 0.5),
    "pool_bf16": ("rows", lambda t, w: (t * 0.5).bfloat16()),
    "hq": ("NQ JQ w", lambda t, w: t * 0.5),
    "lq": ("NQ w", lambda t, w: t * 0.5),
    "W_flat": ("2w", lambda t, w: t * 0.1),                                  # the unwarped forward tools' W
    "W": ("2w", lambda t, w: t * 0.1 * (64.0 / w) ** 0.5),                   # logits of order 1 at every width
    "W_band": ("2w", lambda t, w: t * 0.1 * (64.0 / w) ** 0.5 / 49.0),       # the same under a band of 2 * 3 + 1 = 7 positions
    "b": ("1", lambda t, w: t * 0.1),
    "WH_W": ("2w w", lambda t, w: t * (0.3 / w ** 0.5)),
    "WH_b": ("w", lambda t, w: t * 0.1),
    "WC_W": ("w", lambda t, w: t * (0.5 / w ** 0.5)),
    "WC_b": ("1", lambda t, w: t * 0.1),
    "gout": ("NQ w", lambda t, w: t),
}


def _draw(g, order, rows, NQ, JQ, w, device):
    """the tensors named in `order`, drawn from g in that order and moved to `device` one by one"""
    import torch
    size = {"NQ": NQ, "JQ": JQ, "w": w, "2w": 2 * w, "1": 1}
    out = []
    for name in order:
        shape, scale = _DRAWS[name]
        shape = rows if shape == "rows" else tuple(size[s] for s in shape.split())
        out.append(scale(torch.randn(*shape, generator=g), w).to(device))
    return out


def shared_inputs(order, case, K=6, T=1200, JQ=30, device="cuda"):
    """(tensors in `order`, hmask [A,K,T], qmask [NQ,JQ], album_host [NQ]) of case (A, QPA, w): both masks all ones, the
    questions' albums drawn after the tensors"""
    import torch
    A, QPA, w = case
    NQ = A * QPA
    g = torch.Generator().manual_seed(A * 1000 + QPA + w)
    tensors = _draw(g, order, (A, K, T, w), NQ, JQ, w, device)
    hmask = torch.ones(A, K, T, dtype=torch.uint8, device=device)
    qmask = torch.ones(NQ, JQ, dtype=torch.uint8, device=device)
    album_host = torch.arange(A).repeat_interleave(QPA)[torch.randperm(NQ, generator=g)]
    return tensors, hmask, qmask, album_host


def pooled_inputs(order, case, K=6, JX=300, M=4, JQ=30, OWNED=8, device="cuda"):
    """(tensors in `order`, pmask [P,K,JX], qmask [NQ,JQ], lists_host [NQ,M]) of case (USERS, QPU, w): both masks all ones;
    users own OWNED albums each (P = USERS * OWNED) and every question lists M of its user's, drawn after the tensors"""
    import torch
    U, QPU, w = case
    P, NQ = U * OWNED, U * QPU
    g = torch.Generator().manual_seed(U * 1000 + QPU + w)
    tensors = _draw(g, order, (P, K, JX, w), NQ, JQ, w, device)
    pmask = torch.ones(P, K, JX, dtype=torch.uint8, device=device)
    qmask = torch.ones(NQ, JQ, dtype=torch.uint8, device=device)
    user = torch.arange(U).repeat_interleave(QPU)[torch.randperm(NQ, generator=g)]
    lists_host = torch.stack([int(u) * OWNED + torch.randperm(OWNED, generator=g)[:M] for u in user])
    return tensors, pmask, qmask, lists_host


def gather_lists(pool, pmask, lists64):
    """[NQ,K,M*JX,w] rows and [NQ,K,M*JX] mask of the albums that lists64 [NQ,M] (int64) lists: the per-question route's
    context.  Differentiable in pool: its backward is the index_add_ into [P,K,JX,w]"""
    (P, K, JX, w), (NQ, M), refs = pool.shape, lists64.shape, lists64.reshape(-1)
    rows = pool.index_select(0, refs).reshape(NQ, M, K, JX, w).permute(0, 2, 1, 3, 4).reshape(NQ, K, M * JX, w)
    mask = pmask.index_select(0, refs).reshape(NQ, M, K, JX).permute(0, 2, 1, 3).reshape(NQ, K, M * JX)
    return rows.contiguous(), mask.contiguous()


def record_ms(rec, name, ts):
    """name_ms_median / _min / _max of the times ts into rec; returns the unrounded median"""
    med = statistics.median(ts)
    rec.update({name + "_ms_median": round(med, 3), name + "_ms_min": round(min(ts), 3), name + "_ms_max": round(max(ts), 3)})
    return med


def _timed(fn):
    """(fn's result, ms between HIP events around the call), synchronised"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return res, e0.elapsed_time(e1)


def time_route(fn, iters, warmup):
    """route after route (the forward tools): `warmup` calls, then `iters` timed ones.  Returns (last result, the times)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    res, ts = None, []
    for _ in range(iters):
        res, t = _timed(fn)
        ts.append(t)
    return res, ts


def peak_bytes(routes, rec):
    """name_peak_bytes into rec: the peak allocated bytes of one call of each route, on a warm allocator.  Returns
    {name: clones of that call's outputs}"""
    import torch
    out = {}
    for name, fn in routes.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        out[name] = fn()
        torch.cuda.synchronize()
        rec[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        out[name] = tuple(t.clone() for t in out[name])
    return out


def time_alternating(routes, rec, iters, warmup):
    """alternating (the train tools): warmup + iters rounds of a, b, a, b, ..., each route's result dropped before the next
    starts; the times of the last `iters` rounds into rec"""
    ts = {name: [] for name in routes}
    for it in range(warmup + iters):
        for name, fn in routes.items():
            res, t = _timed(fn)
            del res
            if it >= warmup:
                ts[name].append(t)
    for name, t in ts.items():
        record_ms(rec, name, t)


def grad_diffs(rec, keys, got, want):
    """max_abs_diff_<key> and max_abs_<key> into rec for each gradient of the two routes' outputs"""
    for key, x, y in zip(keys, got, want):
        rec["max_abs_diff_" + key] = float((x.reshape(-1) - y.reshape(-1)).abs().max())
        rec["max_abs_" + key] = float(y.abs().max())
