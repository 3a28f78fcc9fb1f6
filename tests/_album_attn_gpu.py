"""What the album attention's GPU tests share -- tests/test_gpu_attn_{shared,pooled,pool}*.py: the two compare functions,
the memo of cases and references, the upload of a case and the ops handle on it (`TrainRun`, `infer`), and the comparison
of a backward's outputs with a reference (`check_grads`).  The fp64 references, shapes, tolerances (`TOL`, `within`) and
seeds stay in tests/_attn_*_ref.py and tests/_album_attn_ref.py; nothing here computes one.

A `family` is "shared" (h [A,K,T,w], hm, album [NQ]) or "pooled" (pool [P,K,JX,w], pm, albums [NQ,M]); `warped` says
whether the call is the one under the time warp.  fvta_memexqa_amd is imported inside the functions, so that this module
and the tests collect without the built library."""
import numpy as np
import torch

# family -> the case's keys of (rows, their mask, the index, the number of albums held)
_KEYS = {"shared": ("h", "hm", "album", "A"), "pooled": ("pool", "pm", "albums", "P")}
# a backward output -> its key in a reference dict; the others are their own
_REF_KEY = {"d_hinfo": "dh", "d_pool": "dpool", "d_hq": "dq", "d_lq": "dlq"}


# ------------------------------------------------------------------ compare
def _np(x):
    return x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    """|a - b| <= atol + rtol |b|: the forward tests' comparison"""
    np.testing.assert_allclose(_np(a), _np(b), rtol=rtol, atol=atol, err_msg=msg)


def close_scaled(a, b, rtol=1e-4, atol=1e-5, msg=""):
    """|a - b| <= atol max(1, max|b|) + rtol |b|: the gradient tests' comparison (tests/test_gpu_backward.py's)"""
    a, b = _np(a), _np(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * max(1.0, float(np.abs(b).max())), err_msg=msg)


def ref_key(name):
    return _REF_KEY.get(name, name)


def want_of(ref, name, got):
    """the reference of output `name`; dWH_W [2w,w] cut to the rows the output has ([w,w]: the rest is zero)"""
    want = ref[ref_key(name)]
    return want[:got.shape[0]] if name == "dWH_W" else want


def tol_of(tol, name):
    """(rtol, atol) of output `name` in a TOL dict; d_pool is held to d_hinfo's"""
    key = ref_key(name)
    return tol[{"dpool": "dh"}.get(key, key)]


def check_forward(name, got, ref, within):
    """(h_a, a_logits, scale) of a warped forward against the fp64 definition, at tests/test_gpu_attn_shared.py's tolerances:
    all finite (no sentinel left, nothing unwritten), one printed line per output, then the three comparisons"""
    (ha, a, s), (ref_ha, ref_a, ref_s) = got, ref
    for g, r, what in ((ha, ref_ha, "h_a"), (a, ref_a, "a_logits"), (s, ref_s, "scale")):
        assert bool(torch.isfinite(g).all()), what
        print("%s %s: worst |err| / (atol + rtol |ref|) = %.3f" % (name, what, within(g.cpu(), r, what)[1]))
    close(s, ref_s, rtol=1e-4, atol=1e-5, msg="scale")
    close(a, ref_a, rtol=1e-4, atol=2e-5, msg="a_logits")
    close(ha, ref_ha, rtol=1e-4, atol=1e-5, msg="h_a")


def check_grads(name, got, ref, names, tol, within, what=""):
    """The outputs `got` of a backward, in the order `names` (a tuple, or a TrainRun for its own), against the dict `ref`:
    one printed line per output, then each held to its own entry of `tol` by close_scaled.  within: the reference
    module's, for the printed ratio."""
    names = getattr(names, "names", names)
    assert len(got) == len(names), (len(got), names)
    for n, g in zip(names, got):
        want = want_of(ref, n, g)
        print("%s %s%s: worst |err| / (atol max(1, max|ref|) + rtol |ref|) = %.3f, max |ref| %.3g"
              % (name, what, n, within(g, want, ref_key(n))[1], float(want.abs().max())))
    for n, g in zip(names, got):
        rtol, atol = tol_of(tol, n)
        close_scaled(g, want_of(ref, n, g), rtol=rtol, atol=atol, msg=what + n)


# ------------------------------------------------------------------ cases
_MEMO = {}


def once(key, make):
    """make() under `key`: computed once per session; what it returns is never written to"""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def case(R, name, build=None, reference=None):
    """(case, fp64 reference) of `name` in the reference module R: build(name) and reference(case), by default R's
    build_case and reference, run once per session and (R, name)"""
    def make():
        c = (build or R.build_case)(name)
        return c, (reference or R.reference)(c)
    return once((R.__name__, name), make)


def cu(t):
    return None if t is None else t.cuda().contiguous()


def listed(c):
    """[P]: how many (question, slot) list each pooled album"""
    al = c["albums"].reshape(-1)
    return torch.bincount(al[al >= 0], minlength=c["P"])


def gather(pool, pm, al):
    """on the device, differentiable in pool: (hinfo [NQ,K,M JX,w], mask [NQ,K,M JX] of pm's dtype) of lists al [NQ,M]; an
    empty slot: zero rows, mask 0"""
    NQ, M = al.shape
    Pn, K, JX, w = pool.shape
    live = (al >= 0)
    idx = al.clamp(min=0).long()
    h = pool[idx] * live[:, :, None, None, None]                                 # [NQ,M,K,JX,w]
    m = torch.where(live[:, :, None, None], pm[idx], torch.zeros_like(pm[idx]))
    return (h.permute(0, 2, 1, 3, 4).reshape(NQ, K, M * JX, w).contiguous(),
            m.permute(0, 2, 1, 3).reshape(NQ, K, M * JX).contiguous())


def nan_fill(buf):
    """every aligned four bytes of a byte buffer: the quiet NaN 0x7FC00000"""
    flat = buf.reshape(-1)
    flat[:flat.numel() // 4 * 4].view(torch.int32).fill_(0x7FC00000)


def modules(c):
    """(nn.FocalAttention3D, nn.TimeWarp) holding the parameters of the warped case c"""
    from fvta_memexqa_amd import nn
    att = nn.FocalAttention3D(c["w"], simiMatrix=c["simi"], add_tanh=c["tanh"])
    tw = nn.TimeWarp(c["w"], warp_type=c["warp_type"], window_t=c["window_t"])
    with torch.no_grad():
        att.p("att_logits/W").copy_(c["W"])
        att.p("att_logits/b").copy_(c["b"])
        for name, key in (("WH/W", "WH_W"), ("WH/b", "WH_b"), ("WC/W", "WC_W"), ("WC/b", "WC_b")):
            tw.p(name).copy_(c[key])
    return att, tw


# ------------------------------------------------------------------ the ops handle on a case
def handle(c, family, warped=False, tanh=None, NQ=None, M=None):
    """a fresh ops.{Shared,Pooled}[Warped]FocalAttention of case c's shape; tanh: where the case does not carry it"""
    from fvta_memexqa_amd import ops
    NQ, tanh = c["NQ"] if NQ is None else NQ, c["tanh"] if tanh is None else tanh
    if family == "shared":
        cls = ops.SharedWarpedFocalAttention if warped else ops.SharedFocalAttention
        shape = (c["A"], NQ, c["K"], c["T"])
    else:
        cls = ops.PooledWarpedFocalAttention if warped else ops.PooledFocalAttention
        shape = (c["P"], NQ, c["M"] if M is None else M, c["K"], c["JX"])
    warp = (c["warp_type"], c["window_t"]) if warped else ()
    return cls(*shape, c["JQ"], c["w"], c["simi"], tanh, *warp)


def output_names(family, warped):
    """backward()'s outputs, in the op's order: the overwritten ones (2, under the warp 3), then the accumulated ones"""
    rows = "d_hinfo" if family == "shared" else "d_pool"
    return (rows, "d_hq", "d_lq", "dW", "db", "dWH_W", "dWH_b", "dWC_W", "dWC_b") if warped else (rows, "d_hq", "dW", "db")


def warp_args(c):
    return cu(c["WH_b"]), cu(c["WC_W"].reshape(-1)), cu(c["WC_b"])


def album_energy(c, family, op=None, rows=None):
    """op.album_energy of case c's rows (or `rows` in their place), by `op` or a fresh handle"""
    op = op or handle(c, family, True)
    return op.album_energy(cu(c[_KEYS[family][0]] if rows is None else rows), cu(c["WH_W"]), cu(c["WC_W"].reshape(-1)))


class TrainRun:
    """The ops handle of `family` / `warped` on case c, its index validated on the host and its tensors uploaded and kept.
    rows: a subset of the questions (an index list); albums / pool / pm: in place of the case's own index, rows and rows'
    mask; tanh: where the case does not carry it; energy: a held one (warped; else computed here).

    op, al (the device index), g (d_h_a, where the case has one), rows, mask, q, qm, W, b and under the warp lq, WH, WHb,
    WC, WCb, energy; args: the unwarped calls' seven arguments; names: backward()'s outputs, in order."""

    def __init__(self, c, family, warped=False, tanh=None, rows=None, albums=None, pool=None, pm=None, energy=None):
        from fvta_memexqa_amd import ops
        k_rows, k_mask, k_index, k_n = _KEYS[family]
        q, qm, lq, g = c["q"], c["qm"], c.get("lq"), c.get("gout")
        al = c[k_index] if albums is None else albums
        pool = c[k_rows] if pool is None else pool
        pm = c[k_mask] if pm is None else pm
        if rows is not None:
            q, al = q[rows], al[rows]
            qm, lq, g = (None if t is None else t[rows] for t in (qm, lq, g))
        self.c, self.family, self.warped, self.NQ = c, family, warped, q.shape[0]
        if family == "shared":
            index = ops.check_album_index(al, c[k_n])
            self.op = handle(c, family, warped, tanh, self.NQ)
        else:
            index = ops.check_album_lists(al, c[k_n], pm is not None and qm is not None)
            self.op = handle(c, family, warped, tanh, self.NQ, al.shape[1])
        self.rows, self.mask, self.q, self.qm = cu(pool), cu(ops.as_mask_u8(pm)), cu(q), cu(ops.as_mask_u8(qm))
        self.al, self.g = index.cuda(), cu(g)
        self.W, self.b = None if c["W"] is None else cu(c["W"].reshape(-1)), cu(c["b"])
        self.args = (self.rows, self.mask, self.q, self.qm, self.al, self.W, self.b)
        self.names = output_names(family, warped)
        if warped:
            self.lq, self.WH = cu(lq), cu(c["WH_W"])
            self.WHb, self.WC, self.WCb = warp_args(c)
            self.energy = self.op.album_energy(self.rows, self.WH, self.WC) if energy is None else energy

    def fwd_args(self):
        """the forward calls' arguments: under the warp the energy, lq and the warp's parameters among the seven"""
        if not self.warped:
            return self.args
        return (self.rows, self.mask, self.energy, self.q, self.qm, self.lq, self.al, self.W, self.b, self.WHb, self.WC, self.WCb)

    def _forward(self, call, want_logits):
        return call(*self.fwd_args(), want_logits=want_logits, **(dict(want_scale=True) if self.warped else {}))

    def forward_train(self, want_logits=True):
        return self._forward(self.op.forward_train, want_logits)

    def forward(self, want_logits=True):
        return self._forward(self.op.forward, want_logits)

    def backward(self, acc=None, fill=7.0):
        """-> the outputs in the op's order (`names`: 4, under the warp 9).  The overwritten ones (the rows', d_hq, d_lq)
        are prefilled with `fill`; the accumulated ones (dW, db, the warp's four) are fresh zeros, or `acc`: those of an
        earlier call"""
        w = self.c["w"]
        full = lambda like: torch.full(like.shape, fill, device="cuda")
        zeros = lambda *shape: torch.zeros(*shape, device="cuda")
        if not self.warped:
            over = (full(self.rows), full(self.q))
            acc = (torch.zeros_like(self.W), zeros(1)) if acc is None else tuple(acc)
            self.op.backward(*self.args, self.g, *over, *acc)
        else:
            over = (full(self.rows), full(self.q), full(self.lq))
            acc = (torch.zeros_like(self.W), zeros(1), zeros(w, w), zeros(w), zeros(w), zeros(1)) if acc is None else tuple(acc)
            self.op.backward(self.rows, self.mask, self.q, self.qm, self.lq, self.al, self.W, self.b, self.WH, self.WHb, self.WC,
                             self.WCb, self.g, *over, *acc)
        return over + acc


def infer(c, family, warped=False, want_logits=True, sentinels=False, **kw):
    """The inference call on case c -> (h_a, a_logits), under the warp (h_a, a_logits, scale).  kw: TrainRun's tanh, rows,
    albums, pool, pm and energy.  sentinels (pooled, warped): the C call itself on outputs that hold NaN -- whatever it
    leaves unwritten stays NaN"""
    run = TrainRun(c, family, warped, **kw)
    if not sentinels:
        return run.forward(want_logits)
    import ctypes
    from fvta_memexqa_amd import _lib
    assert family == "pooled" and warped
    op, T = run.op, run.al.shape[1] * c["JX"]
    shapes = ((run.NQ, c["w"]), (run.NQ, c["K"], T, c["JQ"]), (run.NQ, T))
    outs = tuple(torch.full(shape, float("nan"), device="cuda") for shape in shapes)
    _lib.check(op.lib.fvta_attn_pool_fwd_tw(ctypes.byref(op.desc), *[_lib.ptr(t) for t in run.fwd_args() + outs],
                                            _lib.ptr(op.work), _lib.stream_ptr()), "fvta_attn_pool_fwd_tw")
    torch.cuda.synchronize()
    return outs
