"""What the gradient guard costs per train step: the guarded step against the unguarded one in ONE process, at
BASELINE.json's metric shape (bench.py's default headline: dense, bf16, Adam), HIP events around alternating blocks of
steps.  Both trainers drive the same model and batch; the guarded one runs with thresholds nothing reaches
(clip_global_norm 1e30, skip_nonfinite on), so both do the same arithmetic and the difference is the guard's two
launches plus the guarded update's reads of the control block.  Also times the guard's launches alone on the model's
flat gradient.  Prints one JSON line.

    python tools/guard_overhead.py [--config metric] [--precision bf16] [--optimizer adam] [--rounds 10] [--block 10]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="metric", choices=["metric", "plumbing", "long_album"])
    ap.add_argument("--precision", default="bf16", choices=["f32", "bf16", "bf16x3"])
    ap.add_argument("--optimizer", default="adam", choices=["adam", "adadelta"])
    ap.add_argument("--rounds", type=int, default=10, help="alternations: each times one block of either kind")
    ap.add_argument("--block", type=int, default=10, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from fvta_memexqa_amd import ops
    from fvta_memexqa_amd.model_v2 import Model
    from fvta_memexqa_amd.synth import CONFIGS, SynthSpec, make_inputs
    from fvta_memexqa_amd.trainer import Trainer
    dev = ops.require_gpu()
    spec = SynthSpec(**dict(CONFIGS[args.config], dense=True))
    cfg = dict(spec.cfg(), batch_size=spec.N, precision=args.precision, optimizer=args.optimizer,
               init_lr=0.001 if args.optimizer == "adam" else 0.5)
    model = Model(cfg, text_in=spec.text_in, img_in=spec.img_in, device=dev)
    trainers = dict(plain=Trainer(model, cfg), guarded=Trainer(model, dict(cfg, clip_global_norm=1e30, skip_nonfinite=True)))
    for t in trainers.values():
        t.need_dx = True
    L = model.load_inputs(make_inputs(spec), training=True)
    for _ in range(args.warmup):
        for t in trainers.values():
            t.step_device(L)
    torch.cuda.synchronize()
    ms = dict(plain=[], guarded=[])
    for r in range(args.rounds):
        for name in (("plain", "guarded") if r % 2 == 0 else ("guarded", "plain")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.block):
                trainers[name].step_device(L)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.block)
    st = trainers["guarded"].guard_stats()
    assert st["factor"] == 1.0 and st["skipped"] == 0, st
    # the guard's two launches alone, back to back on the gradient the last step left
    grad, ctl = model.params.grad, ops.guard_ctl_new(dev)
    ws = ops.grad_guard_workspace(grad.numel(), dev)
    alone = []
    for r in range(args.rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(100):
            ops.grad_guard(grad, ctl, ws, 1.0, 0.0, 1e30, True)
        b.record()
        b.synchronize()
        if r:
            alone.append(a.elapsed_time(b) * 10.0)          # us per call
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(
        config=args.config, precision=args.precision, optimizer=args.optimizer, params=int(grad.numel()),
        rounds=args.rounds, block=args.block,
        plain_ms_per_step=dict(median=round(med["plain"], 4), min=round(min(ms["plain"]), 4), max=round(max(ms["plain"]), 4)),
        guarded_ms_per_step=dict(median=round(med["guarded"], 4), min=round(min(ms["guarded"]), 4),
                                 max=round(max(ms["guarded"]), 4)),
        overhead_pct_of_step=round(100.0 * (med["guarded"] - med["plain"]) / med["plain"], 3),
        guard_launches_alone_us=dict(median=round(statistics.median(alone), 2), min=round(min(alone), 2)),
        guard_read_gbs=round(grad.numel() * 4 / (statistics.median(alone) * 1e-6) / 1e9, 1))))


if __name__ == "__main__":
    main()
