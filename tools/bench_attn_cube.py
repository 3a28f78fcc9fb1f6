"""Times fvta_attn_cube_bwd (the dense gradient of the focal logits cube: main kernel + its three folds) at the metric
shape with HIP events around the call, and prints the fraction of the 8 TB/s HBM roof on the bytes of hinfo read and
d_hinfo written (plus d_hinfo read when accumulating).  Usage: python tools/bench_attn_cube.py [iterations]"""
import ctypes, os, sys, torch
sys.path.insert(0, os.getcwd())
from fvta_memexqa_amd import _lib
from fvta_memexqa_amd._lib import AttnDesc, check, ptr, stream_ptr
N, K, T, JQ, w = 64, 6, 1200, 30, 1024  # the metric shape
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
lib = _lib.load()
g = torch.Generator(device="cuda").manual_seed(0)
h = torch.randn(N, K, T, w, device="cuda", generator=g) * 0.5
q = torch.randn(N, JQ, w, device="cuda", generator=g) * 0.5
W = torch.randn(2 * w, device="cuda", generator=g) * 0.1
b = torch.zeros(1, device="cuda")
dA = torch.randn(N, K, T, JQ, device="cuda", generator=g)
dh, dq, dW, db = torch.zeros_like(h), torch.zeros_like(q), torch.zeros_like(W), torch.zeros(1, device="cuda")
for tanh in (0, 1):
    desc = AttnDesc(N, K, T, JQ, w, 2, 0, tanh, 0)
    nb = lib.fvta_attn_cube_bwd_workspace_bytes(ctypes.byref(desc))
    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for acc in (0, 1):
        run = lambda: check(lib.fvta_attn_cube_bwd(ctypes.byref(desc), ptr(h), ptr(q), ptr(W), ptr(b), ptr(dA), ptr(dh), ptr(dq),
                                                   ptr(dW), ptr(db), acc, ptr(work), stream_ptr()), "fvta_attn_cube_bwd")
        run(); run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        gb = h.numel() * 4 * (2 + acc) / 1e9
        print("add_tanh=%d accumulate=%d: %.3f ms per call, %.2f GB of rows -> %.2f TB/s = %.2f of the 8 TB/s roof (workspace %.0f MB)"
              % (tanh, acc, ms, gb, gb / ms, gb / ms / 8.0, nb / 2 ** 20))
