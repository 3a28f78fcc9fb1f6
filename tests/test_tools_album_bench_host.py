"""tools/_album_bench.py, the plumbing the nine album attention benchmark tools share, without a GPU: each tool's inputs
against that tool's draw sequence written out (the order of the draws is what makes h_a_sum and the difference fields
of the published records reproducible), the pooled gather against its expression, the parent loop on stub children, and
every tool's --help without torch."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
_spec = importlib.util.spec_from_file_location("_album_bench", os.path.join(TOOLS, "_album_bench.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

CASE = (2, 2, 8)
K, T, JQ = 2, 5, 3                      # the shared-context tools' constants, tiny
JX, M, OWNED = 5, 2, 3                  # the album-pool tools'


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _album(g, A, QPA):
    return torch.arange(A).repeat_interleave(QPA)[torch.randperm(A * QPA, generator=g)]


def _lists(g, U, QPU):
    user = torch.arange(U).repeat_interleave(QPU)[torch.randperm(U * QPU, generator=g)]
    return torch.stack([int(u) * OWNED + torch.randperm(OWNED, generator=g)[:M] for u in user])


def _warp_weights(g, w):
    """WH_W, WH_b, WC_W, WC_b as every warped tool draws them"""
    return [_randn(g, 2 * w, w) * (0.3 / w ** 0.5), _randn(g, w) * 0.1, _randn(g, w) * (0.5 / w ** 0.5), _randn(g, 1) * 0.1]


def _rows(g, family, first, second, w):
    """(rows, NQ): hall [A,K,T,w] of the shared tools, pool [P,K,JX,w] of the pooled ones"""
    rows = _randn(g, first, K, T, w) if family == "shared" else _randn(g, first * OWNED, K, JX, w)
    return rows * 0.5, first * second


# each tool's draws after the rows, as the tool wrote them before the shared module (g: the generator, n: NQ, w: the width)
def _fwd(g, n, w):                      # bench_attn_shared.py, bench_attn_pooled.py
    return [_randn(g, n, JQ, w) * 0.5, _randn(g, 2 * w) * 0.1, _randn(g, 1) * 0.1]


def _fwd_tw(g, n, w):                   # bench_attn_shared_tw.py, bench_attn_pooled_tw.py
    return [_randn(g, n, JQ, w) * 0.5, _randn(g, n, w) * 0.5, _randn(g, 2 * w) * 0.1 * (64.0 / w) ** 0.5,
            _randn(g, 1) * 0.1] + _warp_weights(g, w)


def _train(g, n, w):                    # bench_attn_shared_train.py, bench_attn_pooled_train.py
    return [_randn(g, n, JQ, w) * 0.5, _randn(g, 2 * w) * 0.1 * (64.0 / w) ** 0.5, _randn(g, 1) * 0.1, _randn(g, n, w)]


def _tw_train(g, n, w):                 # bench_attn_shared_tw_train.py, bench_attn_pooled_tw_train.py
    return [_randn(g, n, JQ, w) * 0.5, _randn(g, n, w) * 0.5, _randn(g, 2 * w) * 0.1 * (64.0 / w) ** 0.5 / 49.0,
            _randn(g, 1) * 0.1] + _warp_weights(g, w) + [_randn(g, n, w)]


def _bf16(g, n, w):                     # bench_attn_pooled_bf16.py (its pool goes to bf16 on the host: below)
    return [_randn(g, n, JQ, w) * 0.5, _randn(g, n, w) * 0.5, _randn(g, 2 * w) * 0.1, _randn(g, 1) * 0.1] + _warp_weights(g, w)


WARP_NAMES = ("WH_W", "WH_b", "WC_W", "WC_b")
TOOLS_SPECS = {  # tool: (family, the order it passes to the module, its literal draws after the rows)
    "bench_attn_shared.py": ("shared", ("hall", "hq", "W_flat", "b"), _fwd),
    "bench_attn_shared_tw.py": ("shared", ("hall", "hq", "lq", "W", "b") + WARP_NAMES, _fwd_tw),
    "bench_attn_shared_train.py": ("shared", ("hall", "hq", "W", "b", "gout"), _train),
    "bench_attn_shared_tw_train.py": ("shared", ("hall", "hq", "lq", "W_band", "b") + WARP_NAMES + ("gout",), _tw_train),
    "bench_attn_pooled.py": ("pooled", ("pool", "hq", "W_flat", "b"), _fwd),
    "bench_attn_pooled_tw.py": ("pooled", ("pool", "hq", "lq", "W", "b") + WARP_NAMES, _fwd_tw),
    "bench_attn_pooled_train.py": ("pooled", ("pool", "hq", "W", "b", "gout"), _train),
    "bench_attn_pooled_tw_train.py": ("pooled", ("pool", "hq", "lq", "W_band", "b") + WARP_NAMES + ("gout",), _tw_train),
    "bench_attn_pooled_bf16.py": ("pooled", ("pool_bf16", "hq", "lq", "W_flat", "b") + WARP_NAMES, _bf16),
}


@pytest.mark.parametrize("tool", sorted(TOOLS_SPECS))
def test_inputs_are_the_tools_own_draws(tool):
    family, order, rest = TOOLS_SPECS[tool]
    with open(os.path.join(TOOLS, tool)) as f:          # the order under test is the one the tool passes
        assert ", ".join('"%s"' % n for n in order) in f.read()
    first, second, w = CASE
    g = torch.Generator().manual_seed(first * 1000 + second + w)
    rows, NQ = _rows(g, family, first, second, w)
    want = [rows.to(torch.bfloat16) if order[0] == "pool_bf16" else rows] + rest(g, NQ, w)
    if family == "shared":
        want_index, want_mask = _album(g, first, second), torch.ones(first, K, T, dtype=torch.uint8)
        got, mask, qmask, index = ab.shared_inputs(order, CASE, K, T, JQ, device="cpu")
    else:
        want_index, want_mask = _lists(g, first, second), torch.ones(first * OWNED, K, JX, dtype=torch.uint8)
        got, mask, qmask, index = ab.pooled_inputs(order, CASE, K, JX, M, JQ, OWNED, device="cpu")
    assert len(got) == len(want) == len(order)
    for name, x, y in zip(order, got, want):
        assert x.dtype == y.dtype and torch.equal(x, y), name
    assert torch.equal(index, want_index) and index.dtype == torch.int64
    assert torch.equal(mask, want_mask) and mask.dtype == torch.uint8
    assert torch.equal(qmask, torch.ones(NQ, JQ, dtype=torch.uint8)) and qmask.dtype == torch.uint8


def test_input_defaults_are_the_published_shapes():
    """the tools' constants are the functions' defaults (checked on the signatures: the tensors are 100 MB and more)"""
    import inspect

    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not p.empty}

    assert defaults(ab.shared_inputs) == dict(K=6, T=1200, JQ=30, device="cuda")
    assert defaults(ab.pooled_inputs) == dict(K=6, JX=300, M=4, JQ=30, OWNED=8, device="cuda")


def test_pooled_gather():
    P, NQ, w = 6, 4, 8
    g = torch.Generator().manual_seed(7)
    pool = torch.randn(P, K, JX, w, generator=g)
    pmask = (torch.rand(P, K, JX, generator=g) < 0.7).to(torch.uint8)
    lists64 = torch.stack([torch.randperm(P, generator=g)[:M] for _ in range(NQ)])
    refs = lists64.reshape(-1)
    want_rows = pool.index_select(0, refs).reshape(NQ, M, K, JX, w).permute(0, 2, 1, 3, 4).reshape(NQ, K, M * JX, w)
    want_mask = pmask.index_select(0, refs).reshape(NQ, M, K, JX).permute(0, 2, 1, 3).reshape(NQ, K, M * JX)
    rows, mask = ab.gather_lists(pool, pmask, lists64)
    assert rows.is_contiguous() and mask.is_contiguous()
    assert torch.equal(rows, want_rows) and torch.equal(mask, want_mask)
    assert torch.equal(rows[1, :, JX:], pool[lists64[1, 1]])           # question 1's second album follows its first


def test_record_fields():
    rec = {}
    assert ab.record_ms(rec, "a", [3.00049, 1.0, 2.0004]) == 2.0004
    assert list(rec.items()) == [("a_ms_median", 2.0), ("a_ms_min", 1.0), ("a_ms_max", 3.0)]
    x, y = (torch.tensor([[1.0, -2.0]]), torch.tensor([5.0])), (torch.tensor([1.5, -2.0]), torch.tensor([-7.0]))
    ab.grad_diffs(rec, ("dW", "db"), x, y)
    assert list(rec.items())[3:] == [("max_abs_diff_dW", 0.5), ("max_abs_dW", 2.0), ("max_abs_diff_db", 12.0), ("max_abs_db", 7.0)]


def _parent(tmp_path, child_source, cases, limit=30.0):
    """run_parent over a stub child (plain Python, no torch); returns (status, --out path)"""
    child = tmp_path / "child.py"
    child.write_text(child_source)
    out = tmp_path / "fresh" / "dir" / "out.jsonl"
    argv = ["--iters", "2", "--warmup", "1", "--limit", str(limit), "--out", str(out)]
    for case in cases:
        argv += ["--case"] + [str(v) for v in case]
    args = ab.parse(("A", "QPA", "w"), [[9, 9, 9]], 240.0, "unused.jsonl", argv=argv)
    return ab.run_parent(str(child), args), out


def test_parent_echoes_and_appends_the_last_line(tmp_path, capfd):
    rc, out = _parent(tmp_path, "import json, sys\nprint('noise')\nprint(json.dumps(sys.argv[1:]))\n", [(1, 2, 3), (4, 5, 6)])
    assert rc == 0
    lines = [["--child", "--case"] + case + ["--iters", "2", "--warmup", "1"] for case in (["1", "2", "3"], ["4", "5", "6"])]
    assert [json.loads(line) for line in capfd.readouterr().out.splitlines()] == lines
    assert [json.loads(line) for line in out.read_text().splitlines()] == lines


def test_parent_stops_at_a_failed_child(tmp_path, capfd):
    marker = tmp_path / "started"
    source = "import sys\nopen(%r, 'a').write('x')\nprint('partial')\nsys.exit(3)\n" % str(marker)
    rc, out = _parent(tmp_path, source, [(1, 2, 3), (4, 5, 6)])
    assert rc == 3
    assert [json.loads(line) for line in capfd.readouterr().out.splitlines()] == [dict(case=[1, 2, 3], failed=3)]
    assert not out.exists() and marker.read_text() == "x"                # nothing appended, the second case never started


def test_parent_counts_a_timeout_as_124(tmp_path, capfd):
    rc, out = _parent(tmp_path, "import time\ntime.sleep(60)\n", [(1, 2, 3)], limit=1.0)
    assert rc == 124
    assert json.loads(capfd.readouterr().out) == dict(case=[1, 2, 3], failed=124)
    assert not out.exists()


def test_parser_defaults(tmp_path):
    args = ab.parse(("USERS", "QPU", "w"), [[8, 8, 512]], 300.0, "x.jsonl", only=("a", "b"), argv=[])
    assert (args.cases, args.iters, args.warmup, args.limit, args.child, args.only) == ([[8, 8, 512]], 10, 3, 300.0, False, None)
    assert args.out == os.path.join(os.path.dirname(TOOLS), "profiles", "x.jsonl")
    with pytest.raises(SystemExit):
        ab.parse(("A", "QPA", "w"), [[8, 8, 512]], 240.0, "x.jsonl", argv=["--only", "a"])      # only where a tool has it


@pytest.mark.parametrize("tool", sorted(TOOLS_SPECS))
def test_help_needs_neither_gpu_nor_torch(tool):
    code = ("import runpy, sys\n"
            "sys.argv = [%r, '--help']\n"
            "sys.path.insert(0, %r)\n"
            "try:\n"
            "    runpy.run_path(sys.argv[0], run_name='__main__')\n"
            "except SystemExit as e:\n"
            "    assert e.code == 0, e.code\n"
            "else:\n"
            "    raise AssertionError('--help did not exit')\n"
            "assert 'torch' not in sys.modules and 'fvta_memexqa_amd' not in sys.modules\n"
            "print('parent side clean')\n") % (os.path.join(TOOLS, tool), TOOLS)
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert "--case" in p.stdout and "--limit" in p.stdout and p.stdout.rstrip().endswith("parent side clean")
