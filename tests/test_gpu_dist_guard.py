"""The gradient guard under data parallelism: two ranks (gloo, as tests/test_gpu_dist.py) and one whole-batch process,
f32, with clip_global_norm below the first step's norm so that the clip factor really bites.  Every rank sees the same
reduced gradient and the statistics kernel has one fixed summation order: the ranks take the same decision with no extra
collective -- bitwise-identical parameters AND control blocks -- and match the single process at the unguarded test's
f32 tolerance."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

STEPS = 2
CLIP = 0.05          # far below the first step's global norm of this spec (asserted below through the clip factor)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spec(n):
    from fvta_memexqa_amd.synth import SynthSpec
    return SynthSpec(N=n, A=2, P=3, S=2, L=5, d=32, SA=1, dense=False, text_in=12, img_in=8)


def _shard(inputs, lo, hi):
    cut = lambda st: {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in st.items()}
    return dict(ctx=[cut(s) for s in inputs["ctx"]], q=cut(inputs["q"]), choices=cut(inputs["choices"]), y=inputs["y"][lo:hi])


def _run(rank, ws, q):
    from fvta_memexqa_amd import dist
    from fvta_memexqa_amd.model_v2 import Model
    from fvta_memexqa_amd.synth import make_inputs, make_params
    from fvta_memexqa_amd.trainer import Trainer
    spec = _spec(8)
    lo, hi = dist.shard_range(spec.N, ws, max(rank, 0))
    cfg = dict(spec.cfg(), batch_size=hi - lo, init_lr=0.5, precision="f32", clip_global_norm=CLIP, skip_nonfinite=True)
    model = Model(cfg, text_in=spec.text_in, img_in=spec.img_in)
    model.set_oracle_params(make_params(spec))
    tr = Trainer(model, cfg)
    tr.need_dx = True
    L = model.load_inputs(_shard(make_inputs(spec), lo, hi), training=True)
    losses, factors = [], []
    for _ in range(STEPS):
        loss = tr.step_device(L)
        losses.append(float(dist.mean_over_ranks(loss.clone()).item()))
        factors.append(tr.guard_stats()["factor"])
    torch.cuda.synchronize()
    q.put((rank, model.params.flat.cpu().numpy(), losses, tr.guard_ctl.cpu().numpy(), factors, tr.guard_stats()))


def _worker(rank, ws, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from fvta_memexqa_amd import dist
    dist.init(backend="gloo")
    _run(rank, ws, q)
    dist.barrier()
    dist.shutdown()


def _reference_worker(q):
    """one process, the whole batch"""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    _run(-1, 1, q)


def test_two_guarded_ranks_equal_one_guarded_process():
    # every GPU user of this test is a CHILD process; the pytest process must not have initialised the GPU before it
    # starts them (conftest.py runs the test_gpu_dist* files first)
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: child processes may not be exec'd from it here; "
                    "run the tests/test_gpu_dist*.py files first or alone")
    ws, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, ws, port, q)) for r in range(ws)]
    ps.append(ctx.Process(target=_reference_worker, args=(q,)))
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=300) for _ in ps], key=lambda x: x[0])
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    ref, r0, r1 = res
    assert all(f < 1.0 for f in r0[4]) and all(f < 1.0 for f in ref[4]), "the clip must bite at every step"
    assert np.array_equal(r0[1], r1[1]), "ranks must hold identical parameters"
    assert np.array_equal(r0[3], r1[3]), "ranks must hold identical control blocks"
    assert r0[5]["applied"] == r1[5]["applied"] == ref[5]["applied"] == STEPS and r0[5]["skipped"] == 0
    np.testing.assert_allclose(r0[1], ref[1], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r0[2], ref[2], rtol=1e-4)
    np.testing.assert_allclose(r0[5]["norm"], ref[5]["norm"], rtol=1e-4)
    assert abs(r0[5]["norm"] * r0[5]["factor"] - CLIP) <= 1e-5 * CLIP       # the clipped gradient has the norm asked for
