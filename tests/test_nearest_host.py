"""CPU-only: the nearest-neighbour entry of include/facegen_hip.h (fg_nearest_workspace_bytes, fg_nearest_update) in a planning-only
context (FG_DEVICE_NONE): declarations and exports, the scratch size, every refusal with its message, the launch list of one call
beside that of fg_parzen_min_dist (which shares the two kernel templates), and the `--neighbours` surface of sample.py as far as
planning goes.  What the kernels compute is checked on the device (tests/test_gpu_nearest.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_ERR_INVALID, FG_ERR_UNSUPPORTED, FG_ERR_WORKSPACE = -1, -4, -5
LAUNCH_RE = re.compile(r"^fg-launch \(?\s*([A-Za-z_]\w*)[^)]*\)? grid=(\d+),(\d+),(\d+) block=(\d+) lds=(\d+)$")


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def _err(ctx):
    return ctx.lib.fg_last_error(ctx.h).decode()


def test_header_declares_and_library_exports_the_entries(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    for name in ("fg_nearest_workspace_bytes", "fg_nearest_update"):
        assert name in decls, name
        assert hasattr(plan_ctx.lib, name), name
    assert decls["fg_nearest_workspace_bytes"][2] == ["q", "n"]
    assert decls["fg_nearest_update"][2] == ["ctx", "queries", "q", "rows", "n", "elems", "first_index", "first", "best_d2", "best_index",
                                             "best_dist", "scratch", "scratch_bytes"]
    hdr = open(_lib.HEADER).read()
    assert "PARITY UNPINNED" in hdr[hdr.index("findClosestNeighboursOf (sample.lua:133-151)"):hdr.index("size_t fg_nearest_workspace_bytes")]


def test_workspace_grows_with_q_and_n(plan_ctx):
    ws = plan_ctx.lib.fg_nearest_workspace_bytes
    for q in (1, 2, 15, 16):
        for n in (1, 63, 8192, 1 << 20):
            assert ws(q, n) >= 8 * q * n, (q, n)
    assert ws(1, 100) < ws(2, 100) < ws(16, 100) < ws(17, 100) < ws(33, 100)
    assert ws(16, 1) < ws(16, 2) < ws(16, 8192) < ws(16, 1 << 20)
    assert ws(0, 100) == 0 and ws(16, 0) == 0 and ws(0, 0) == 0 and ws(-1, 5) == 0


def test_refusals(plan_ctx):
    lib, h = plan_ctx.lib, plan_ctx.h
    q, n, elems = 3, 10, 12
    Q, R = torch.zeros(q, elems), torch.zeros(n, elems)
    d2, idx, dist = torch.zeros(q, dtype=torch.float64), torch.zeros(q, dtype=torch.int32), torch.zeros(q)
    scratch = torch.zeros(q * n, dtype=torch.float64)
    P = lambda t: t.data_ptr()
    good = dict(queries=P(Q), q=q, rows=P(R), n=n, elems=elems, first_index=0, first=1, best_d2=P(d2), best_index=P(idx), best_dist=P(dist),
                scratch=P(scratch), scratch_bytes=lib.fg_nearest_workspace_bytes(q, n))
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fg_nearest_update(h, *[a[k] for k in order])

    assert call() == 0
    assert call(first_index=(1 << 31) - 1 - n, first=0) == 0
    # more rows than one call takes: refused by name (the scratch size is not what stops it)
    big = (1 << 20) + 1
    assert call(n=big, scratch_bytes=lib.fg_nearest_workspace_bytes(q, big)) == FG_ERR_UNSUPPORTED
    assert "n = %d" % big in _err(plan_ctx)
    assert call(n=1 << 20, scratch_bytes=lib.fg_nearest_workspace_bytes(q, 1 << 20)) == 0
    # indices beyond 2^31 - 1
    for fi in ((1 << 31) - n, 1 << 31, 1 << 40, -1):
        assert call(first_index=fi) == FG_ERR_INVALID, fi
        assert "index" in _err(plan_ctx)
    # scratch one byte short
    assert call(scratch_bytes=good["scratch_bytes"] - 1) == FG_ERR_WORKSPACE
    assert "%d" % good["scratch_bytes"] in _err(plan_ctx) and "scratch" in _err(plan_ctx)
    assert call(scratch_bytes=0) == FG_ERR_WORKSPACE
    # NULL arguments
    for k in ("queries", "rows", "best_d2", "best_index", "best_dist", "scratch"):
        assert call(**{k: None}) == FG_ERR_INVALID, k
        assert "NULL" in _err(plan_ctx), k
    assert lib.fg_nearest_update(None, *[good[k] for k in order]) == FG_ERR_INVALID
    # non-positive counts
    for k in ("q", "n", "elems"):
        for v in (0, -1):
            assert call(**{k: v}) == FG_ERR_INVALID, (k, v)
            assert "%s = %d" % (k, v) in _err(plan_ctx), (k, v)


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: t.data_ptr())
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
E = lambda *s: torch.zeros(*s)
mark("parzen"); ctx.check(lib.fg_parzen_min_dist(ctx.h, P(E(5, 300)), P(E(300)), P(E(300)), 5, 300, P(E(5)), P(E(1))))
for q, n, elems, off in %r:
    mark("nearest-%%d-%%d-%%d-%%d" %% (q, n, elems, off))
    rows = E(n * elems + 4)[off:]
    scratch = torch.zeros(q * n, dtype=torch.float64)
    ctx.check(lib.fg_nearest_update(ctx.h, P(E(q, elems)), q, P(rows), n, elems, 0, 1, P(torch.zeros(q, dtype=torch.float64)),
                                    P(torch.zeros(q, dtype=torch.int32)), P(E(q)), P(scratch), q * n * 8))
mark("end")
"""
LOGGED = [(16, 1000, 3072, 0), (33, 1000, 3072, 0), (1, 17, 5, 0), (3, 16, 8, 0), (16, 4096, 3072, 1), (7, 1 << 20, 4, 0)]


@pytest.fixture(scope="module")
def launch_sections():
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, LOGGED)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = l.split()[1]
            sections[cur] = []
        elif cur is not None and l.startswith("fg-launch"):
            m = LAUNCH_RE.match(l)
            assert m, l
            sections[cur].append((m.group(1),) + tuple(int(v) for v in m.groups()[1:]) + (l,))
    return sections


def test_parzen_launches_are_what_they_were(launch_sections):
    """fg_parzen_min_dist(n = 5, elems = 300) logged, before its kernels became templates,
        fg-launch parzen_dist_kernel grid=5,1,1 block=256 lds=0
        fg-launch min_kernel grid=1,1,1 block=64 lds=0
    -- the same kernels, grid, block and dynamic LDS now."""
    assert [s[:-1] for s in launch_sections["parzen"]] == [("parzen_dist_kernel", 5, 1, 1, 256, 0), ("min_kernel", 1, 1, 1, 64, 0)]


@pytest.mark.parametrize("q,n,elems,off", LOGGED)
def test_nearest_launch_list(launch_sections, q, n, elems, off):
    """One call = one pass over the rows per group of up to 16 queries (16 rows per block of 512, grid sized from n with no cap)
    and one fold launch of one block per query: instances of the two parzen kernels and nothing else."""
    lines = launch_sections["nearest-%d-%d-%d-%d" % (q, n, elems, off)]
    assert {s[0] for s in lines} == {"parzen_dist_kernel", "min_kernel"}
    groups = -(-q // 16)
    assert len(lines) == groups + 1
    for s in lines[:-1]:
        assert s[:-1] == ("parzen_dist_kernel", -(-n // 16), 1, 1, 512, 0), s
    assert lines[-1][:-1] == ("min_kernel", q, 1, 1, 256, 0)
    # 16-byte loads need elems % 4 == 0 and aligned bases; the instance is named in the log
    vec = elems % 4 == 0 and off % 4 == 0
    assert all(("true>" if vec else "false>") in s[-1] for s in lines[:-1]), lines
    left = q - 16 * (groups - 1)
    assert "<%d," % (16 if left > 4 else 4 if left > 1 else 1) in lines[-2][-1]


def test_output_files_with_and_without_the_flag():
    from face_generator_amd import sample
    opt = dict(sample.DEFAULTS, writeto="w", runs=2)
    assert opt["neighbours"] is False
    plain = sample.output_files(opt)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in plain]
    assert stems == ["random256_0001_base", "random1024_0001_base", "best_0001_base", "worst_0001_base", "random_0001_base",
                     "random256_0002_base", "random1024_0002_base", "best_0002_base", "worst_0002_base", "random_0002_base"]
    assert sample.output_files({k: v for k, v in opt.items() if k not in ("neighbours", "trainingSet")}) == plain
    six = sample.output_files(dict(opt, neighbours=True, trainingSet="set.npy"))
    assert len(six) == 12
    for run in (0, 1):
        assert six[6 * run:6 * run + 5] == plain[5 * run:5 * run + 5]
        assert os.path.splitext(os.path.basename(six[6 * run + 5]))[0] == "best_%04d_neighbours_base" % (run + 1)


def test_neighbours_without_a_training_set_is_an_error(plan_ctx, tmp_path):
    from face_generator_amd import sample
    opt = sample.parse_args(["--neighbours"])
    assert opt["neighbours"] is True and opt["trainingSet"] == ""
    assert sample.parse_args([])["neighbours"] is False
    assert sample.parse_args(["--neighbours", "--trainingSet", "x.npy"])["trainingSet"] == "x.npy"
    with pytest.raises(ValueError, match="--trainingSet"):
        sample.main(dict(opt, writeto=str(tmp_path / "samples"), gpu=-1), plan_ctx)
    assert not os.path.exists(str(tmp_path / "samples"))


def test_sample_main_plans_the_sixth_picture(plan_ctx, tmp_path):
    """sample.main --neighbours on the fixture checkpoint (16-px nets) with a small .npy set, in the planning-only context: loads the
    set, walks the search in chunks and the pairs grid, and names six pictures per run."""
    from face_generator_amd import sample
    from face_generator_amd.state import S
    S.reset()
    path = str(tmp_path / "set.npy")
    np.save(path, np.random.default_rng(5).random((37, 3, 16, 16), dtype=np.float32))
    opt = dict(save_base=os.path.join(ROOT, "tests", "golden"), G_base="adversarial_small.net", D_base="adversarial_small.net",
               scale=16, writeto=str(tmp_path / "samples"), gpu=-1, batchSize=16, runs=2, neighbours=True, trainingSet=path)
    files = sample.main(opt, plan_ctx)
    assert files == sample.output_files(dict(sample.DEFAULTS, **opt)) and len(files) == 12
    assert [os.path.basename(f).split(".")[0] for f in files[5::6]] == ["best_0001_neighbours_base", "best_0002_neighbours_base"]
    for f in files:
        assert os.path.isfile(f) and os.path.getsize(f) > 0, f
    # a set of another size than the nets' is refused by name
    np.save(path, np.zeros((4, 3, 32, 32), np.float32))
    with pytest.raises(ValueError, match="--trainingSet"):
        sample.main(opt, plan_ctx)
    S.reset()


def test_training_set_from_a_directory_of_pictures(plan_ctx, tmp_path):
    """--trainingSet DIR: the sorted *.jpg / *.ppm / *.pgm files, scaled to the sampled size (through PIL where it is installed;
    without it the message asks for a .npy)."""
    from face_generator_amd import sample
    d = tmp_path / "set"
    for i, side in enumerate((16, 20, 8)):
        sample.save_picture(str(d / ("img%d.ppm" % i)), torch.rand(3, side, side))
    (d / "notes.txt").write_text("not a picture")
    if sample.picture_extension() is None:
        with pytest.raises(ValueError, match="PIL"):
            sample.loadTrainingSet(str(d), (3, 16, 16), plan_ctx)
        return
    data = sample.loadTrainingSet(str(d), (3, 16, 16), plan_ctx)
    assert data.dtype == torch.float32 and tuple(data.shape) == (3, 3, 16, 16)
    gray = sample.loadTrainingSet(str(d), (1, 16, 16), plan_ctx)
    assert tuple(gray.shape) == (3, 1, 16, 16)
    with pytest.raises(ValueError, match="no \\*.jpg"):
        sample.loadTrainingSet(str(tmp_path), (3, 16, 16), plan_ctx)
