"""CPU-only: the sampler level of include/facegen_hip.h (fg_rank_scores, fg_image_grid, fg_sampler_*, fg_sample*) in a planning-only
context (FG_DEVICE_NONE): declarations and exports, the workspace size, every refusal with its message, the launch list of one
fg_sample call, and sample.main as far as planning goes.  What the kernels compute is checked on the device
(tests/test_gpu_sampler.py).  (Like tests/test_branched_host.py this module creates the process-wide planning-only context and runs
after tests/test_abi_host.py in the suite's default order.)"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fg_rank_scores_workspace_bytes", "fg_rank_scores", "fg_image_grid", "fg_sampler_workspace_bytes", "fg_sampler_create",
           "fg_sampler_destroy", "fg_sampler_bind_workspaces", "fg_sampler_set_seed", "fg_sampler_buffer", "fg_sample_generate",
           "fg_sample_score", "fg_sample")
FG_ERR_INVALID, FG_ERR_UNSUPPORTED, FG_ERR_WORKSPACE = -1, -4, -5


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def _nets(ctx, dims=(3, 32, 32), noise=100, max_batch=8):
    from face_generator_amd import models
    G = models.create_G(dims, noise).cuda(ctx, max_batch=max_batch)
    D = models.create_D(dims).cuda(ctx, max_batch=max_batch)
    return G._inner().device_net, D._inner().device_net


def _err(ctx):
    return ctx.lib.fg_last_error(ctx.h).decode()


def test_header_declares_and_library_exports_the_sampler_level(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    for name in ENTRIES:
        assert name in decls, name
        assert hasattr(plan_ctx.lib, name), name
    assert len(decls["fg_image_grid"][1]) == 12 and len(decls["fg_rank_scores"][1]) == 7 and len(decls["fg_sampler_create"][1]) == 8
    hdr = open(_lib.HEADER).read()
    for enum in ("FG_SAMPLER_NOISE = 0", "FG_SAMPLER_IMAGES = 1", "FG_SAMPLER_PREDS = 2", "FG_SAMPLER_ORDER_DESC = 3", "FG_SAMPLER_ORDER_ASC = 4"):
        assert enum in hdr
    assert "PARITY UNPINNED" in hdr[hdr.index("fg_image_grid = image.toDisplayTensor"):hdr.index("fg_sampler: G and D")]


def test_workspace_covers_every_buffer_and_grows(plan_ctx):
    dnG, dnD = _nets(plan_ctx)
    lib = plan_ctx.lib
    sizes = [lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, n) for n in (1, 22, 1024, 65536)]
    assert sizes == sorted(set(sizes))
    for n, b in zip((1, 22, 1024, 65536), sizes):
        assert b >= 4 * (n * (100 + 32 * 32 * 3 + 1) + 2 * n), (n, b)
    assert lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, 0) == 0
    # the buffers lie inside it, in order, without overlap
    from face_generator_amd.runtime import Sampler
    sm = Sampler(plan_ctx, dnG, dnD, 22, 8)
    prev_end = 0
    for what, per in (("NOISE", 100), ("IMAGES", 3072), ("PREDS", 1), ("ORDER_DESC", 1), ("ORDER_ASC", 1)):
        off, cnt = ctypes.c_longlong(), ctypes.c_longlong()
        assert lib.fg_sampler_buffer(sm.h, Sampler.BUF[what], ctypes.byref(off), ctypes.byref(cnt)) == 0
        assert cnt.value == 22 * per and off.value >= prev_end and off.value % 4 == 0, (what, off.value, cnt.value)
        prev_end = off.value + cnt.value
    assert prev_end * 4 <= lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, 22)
    assert lib.fg_sampler_buffer(sm.h, 9, None, None) == FG_ERR_INVALID and "unknown buffer 9" in _err(plan_ctx)
    assert sm.view("ORDER_ASC", 22).dtype == torch.int32 and tuple(sm.view("IMAGES", 5).shape) == (5, 32, 32, 3)


def test_refusals_carry_a_message(plan_ctx):
    from face_generator_amd import models_c2f, models
    from face_generator_amd.runtime import Sampler
    from face_generator_amd import FgError
    lib = plan_ctx.lib
    dnG, dnD = _nets(plan_ctx, max_batch=4)
    nbytes = lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, 64)
    ws = torch.zeros(nbytes // 4 + 128)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    h = ctypes.c_void_p()

    # a table-input pair (the c2f nets)
    Gc = models_c2f.create_G((3, 16, 16)).cuda(plan_ctx, max_batch=4)
    Dc = models_c2f.create_D((3, 16, 16)).cuda(plan_ctx, max_batch=4)
    rc = lib.fg_sampler_create(plan_ctx.h, Gc._inner().device_net.h, Dc._inner().device_net.h, 64, 4, base, nbytes, ctypes.byref(h))
    assert rc == FG_ERR_UNSUPPORTED and not h.value and "table-input" in _err(plan_ctx), _err(plan_ctx)
    with pytest.raises(FgError, match="table-input"):
        Sampler(plan_ctx, Gc._inner().device_net, Dc._inner().device_net, 64, 4)

    # a too-small workspace
    rc = lib.fg_sampler_create(plan_ctx.h, dnG.h, dnD.h, 64, 4, base, nbytes - 4096, ctypes.byref(h))
    assert rc == FG_ERR_WORKSPACE and not h.value and "workspace" in _err(plan_ctx) and str(nbytes - 4096) in _err(plan_ctx)
    rc = lib.fg_sampler_create(plan_ctx.h, dnG.h, dnD.h, 64, 4, base + 16, nbytes, ctypes.byref(h))
    assert rc == FG_ERR_INVALID and "256-byte" in _err(plan_ctx)
    rc = lib.fg_sampler_create(plan_ctx.h, dnG.h, dnD.h, 64, 0, base, nbytes, ctypes.byref(h))
    assert rc == FG_ERR_INVALID and not h.value

    # a chunk whose slices would not start on 16 bytes (noiseDim 10: chunk 2 is fine, chunk 1 and 3 are not)
    G10 = models.create_G((3, 32, 32), 10).cuda(plan_ctx, max_batch=4)._inner().device_net
    for chunk, ok in ((1, False), (2, True), (3, False), (4, True)):
        hh = ctypes.c_void_p()
        rc = lib.fg_sampler_create(plan_ctx.h, G10.h, dnD.h, 64, chunk, base, nbytes, ctypes.byref(hh))
        assert (rc == 0) == ok, (chunk, rc, _err(plan_ctx))
        if ok:
            lib.fg_sampler_destroy(hh)
        else:
            assert rc == FG_ERR_UNSUPPORTED and "chunk %d" % chunk in _err(plan_ctx)

    # a chunk larger than what the bound net workspaces hold (the nets above were sized for 4 samples)
    rc = lib.fg_sampler_create(plan_ctx.h, dnG.h, dnD.h, 64, 16, base, nbytes, ctypes.byref(h))
    assert rc == 0 and h.value
    rc = lib.fg_sample(h, 8, None)
    assert rc == FG_ERR_INVALID and "fg_sampler_bind_workspaces first" in _err(plan_ctx)
    rc = lib.fg_sampler_bind_workspaces(h, dnG.ws.data_ptr(), dnG.ws.numel() * 4, dnD.ws.data_ptr(), dnD.ws.numel() * 4)
    assert rc == FG_ERR_WORKSPACE and "chunk 16" in _err(plan_ctx), _err(plan_ctx)
    rc = lib.fg_sample(h, 8, None)
    assert rc == FG_ERR_INVALID                                   # the refused binding did not stick
    lib.fg_sampler_destroy(h)

    # more images than the sampler was built for
    sm = Sampler(plan_ctx, dnG, dnD, 64, 4)
    sm.sample(64)
    for call in (lambda: sm.sample(65), lambda: sm.generate(65), lambda: sm.score(65), lambda: sm.sample(0)):
        with pytest.raises(FgError, match=r"images \(1\.\.64"):
            call()

    # ranking: n beyond what one call takes is refused by name, n < 1 is invalid
    out = torch.zeros(4, dtype=torch.int32)
    sc = torch.zeros(4)
    assert lib.fg_rank_scores(plan_ctx.h, sc.data_ptr(), (1 << 20) + 1, 0, out.data_ptr(), None, 0) == FG_ERR_UNSUPPORTED
    assert "n = %d" % ((1 << 20) + 1) in _err(plan_ctx)
    assert lib.fg_rank_scores(plan_ctx.h, sc.data_ptr(), 0, 0, out.data_ptr(), None, 0) == FG_ERR_INVALID
    assert lib.fg_rank_scores(plan_ctx.h, sc.data_ptr(), 65536, 1, out.data_ptr(), None, lib.fg_rank_scores_workspace_bytes(65536)) == 0
    assert lib.fg_image_grid(plan_ctx.h, sc.data_ptr(), None, 0, 3, 4, 4, 8, 0, 1, sc.data_ptr(), None) == FG_ERR_INVALID


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd import models
from face_generator_amd.runtime import get_context, Sampler
ctx = get_context(-1)
N, chunk = %d, %d
G = models.create_G((3, 32, 32), 100).cuda(ctx, max_batch=chunk)
D = models.create_D((3, 32, 32)).cuda(ctx, max_batch=chunk)
G.evaluate(); D.evaluate()
dnG, dnD = G._inner().device_net, D._inner().device_net
sm = Sampler(ctx, dnG, dnD, N, chunk)
sm.sample(N)                                   # the first forward of a net packs its weights: not part of the steady state
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
tail = N %% chunk
mark("G-chunk"); dnG.forward(torch.zeros(chunk, 100), train=False)
mark("D-chunk"); dnD.forward(torch.zeros(chunk, 32, 32, 3), train=False)
if tail:
    mark("G-tail"); dnG.forward(torch.zeros(tail, 100), train=False)
    mark("D-tail"); dnD.forward(torch.zeros(tail, 32, 32, 3), train=False)
mark("sample"); sm.sample(N)
mark("grids"); sm.grid("ORDER_DESC", min(N, 64), 8); sm.grid("ORDER_ASC", min(N, 64), 8)
mark("end")
"""


def sample_launch_sections(N, chunk):
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, N, chunk)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = l.split()[1]
            sections[cur] = []
        elif cur is not None and l.startswith("fg-launch"):
            sections[cur].append(l)
    return sections


@pytest.mark.parametrize("N,chunk", [(1024, 128), (22, 8)])
def test_fg_sample_launch_list(N, chunk):
    """One fg_sample = one RNG launch, ceil(N / chunk) G forwards, as many D forwards -- never a second D pass -- and one ranking
    launch covering both directions: the logged lines ARE that concatenation, line for line (a chunk's forward inside the sampler
    lists exactly what a stand-alone evaluate-mode forward of that batch size lists).  Counts recorded in profiles/r08_sample.md."""
    sec = sample_launch_sections(N, chunk)
    full, tail = N // chunk, N % chunk
    lines = sec["sample"]
    rng = [l for l in lines if "rng" in l]
    rank = [l for l in lines if "rank_count_kernel" in l]
    assert len(rng) == 1 and lines[0] == rng[0], rng
    assert len(rank) == 1 and lines[-1] == rank[0] and "grid=%d,2,1" % -(-N // 256) in rank[0], rank
    want = [rng[0]] + sec["G-chunk"] * full + (sec["G-tail"] if tail else []) + sec["D-chunk"] * full + (sec["D-tail"] if tail else []) + rank
    assert lines == want
    n_fwd = full + (1 if tail else 0)
    assert n_fwd == -(-N // chunk)
    first_D, first_G = sec["D-chunk"][0], sec["G-chunk"][0]
    assert first_D not in sec["G-chunk"] and first_G not in sec["D-chunk"]
    g_starts = sum(1 for i in range(len(lines)) if lines[i:i + len(sec["G-chunk"])] == sec["G-chunk"])
    d_starts = sum(1 for i in range(len(lines)) if lines[i:i + len(sec["D-chunk"])] == sec["D-chunk"])
    assert (g_starts, d_starts) == (full, full)
    assert not any("pack" in l for l in lines)
    assert [l.split()[1] for l in sec["grids"]] == ["grid_minmax_kernel", "grid_fill_kernel"] * 2
    print("fg_sample N = %d, chunk %d: %d launch lines (1 rng + %d G forwards + %d D forwards + 1 ranking)" % (N, chunk, len(lines), n_fwd, n_fwd))
    prof = open(os.path.join(ROOT, "profiles", "r08_sample.md")).read()
    assert "N = %d, chunk %d: %d launch lines" % (N, chunk, len(lines)) in prof


def test_sample_main_plans_and_names_its_files(plan_ctx, tmp_path):
    """sample.main on the era-format fixture checkpoint (16-px nets, a ConcatTable discriminator) in the planning-only context: loads,
    compiles, builds the sampler with chunk = batchSize, walks one run and names the five pictures of sample.lua:80-89."""
    from face_generator_amd import sample
    from face_generator_amd.state import S
    S.reset()
    opt = dict(save_base=os.path.join(ROOT, "tests", "golden"), G_base="adversarial_small.net", D_base="adversarial_small.net",
               scale=16, writeto=str(tmp_path / "samples"), gpu=-1, batchSize=16, runs=2)
    files = sample.main(opt, plan_ctx)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    assert stems == ["random256_0001_base", "random1024_0001_base", "best_0001_base", "worst_0001_base", "random_0001_base",
                     "random256_0002_base", "random1024_0002_base", "best_0002_base", "worst_0002_base", "random_0002_base"]
    assert files == sample.output_files(dict(sample.DEFAULTS, **opt))
    for f in files:
        assert os.path.isfile(f) and os.path.getsize(f) > 0, f
    # the dependency-free writer: binary PPM / PGM with the right header and payload
    g = torch.linspace(0, 1, 3 * 4 * 5).view(3, 4, 5)
    sample.save_picture(str(tmp_path / "a.ppm"), g)
    raw = open(str(tmp_path / "a.ppm"), "rb").read()
    assert raw.startswith(b"P6\n5 4\n255\n") and len(raw) == len(b"P6\n5 4\n255\n") + 60 and raw[-1] == 255
    sample.save_picture(str(tmp_path / "a.pgm"), g[:1])
    assert open(str(tmp_path / "a.pgm"), "rb").read().startswith(b"P5\n5 4\n255\n")
    idx = sample.selectRandomImagesFrom(10, 64, torch.Generator().manual_seed(1))
    assert idx.dtype == torch.int32 and sorted(idx.tolist()) == list(range(10))
    S.reset()
