"""Which kernel does the library launch for which geometry?  Answered on the CPU: a planning-only context (get_context(-1)) with
FG_LAUNCH_LOG=1 prints one line per launch, produced by the very host code that decides the launches on a device.  This module
holds the child programs (replay of the GPU parity lists, the seeded sweep of the public conv / linear entries, one training
iteration of the baseline nets; the strided sweep and replay of one-layer stride-2 nets; the replay of the module-level pointwise,
BatchNorm, optimizer and RNG lists; the sweep and replay of whole layer lists from tests/net_cases.py and of whole G / D pairs at the
step level from tests/gan_cases.py), the parser of their logs,
the census of the launch sites in csrc/*.hip and the census of the launches with a capped grid.
tests/test_dispatch_coverage_host.py, tests/test_net_fusions_host.py and tests/test_gan_steps_host.py assert on what they return; tests/DISPATCH_COVERAGE.md is
the ledger.

A launch's SIGNATURE is (launch-site text, block size, dynamic LDS bytes); the grid is left out.

`python tests/dispatch_audit.py report` prints the uncovered signatures with the smallest sweep geometry (in FLOPs of the pass)
that reaches each; `... census` prints every launch site's kernel name with the status the logs give it."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face_generator_amd", "csrc")
LEDGER = os.path.join(ROOT, "tests", "DISPATCH_COVERAGE.md")

FG_FUSE_DEFAULT = 503
THIN_SLAB = 2                      # FG_FUSE_THIN_SLAB
WINO_FWD = 32 | 64 | 128           # FG_FUSE_WINOGRAD | _UP | _5X5
WINO_ALL = WINO_FWD | 256          # ... | FG_FUSE_WINOGRAD_WGRAD
PASSES = ("fwd", "dgrad", "wgrad")
SWEEP_SEED, SWEEP_CONV, SWEEP_LINEAR = 20261018, 1600, 320
CHANNELS = [1, 2, 3, 4, 5, 6, 8, 12, 16, 20, 32, 48, 64, 96, 128, 192, 256, 320, 512]
CAP = 1 << 25                      # floats per operand

LAUNCH_RE = re.compile(r"^fg-launch (.*) grid=(\d+),(\d+),(\d+) block=(\d+) lds=(\d+)$")

_MEMO = {}


def memo(f):
    """one run per process: tests/test_dispatch_coverage_host.py and tests/test_net_fusions_host.py ask for the same logs"""
    def g():
        if f.__name__ not in _MEMO:
            _MEMO[f.__name__] = f()
        return _MEMO[f.__name__]
    g.__name__, g.__doc__ = f.__name__, f.__doc__
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# the job engine shared by the replay and the sweep children: a job = one geometry under one setting, run through the three passes
# ---------------------------------------------------------------------------------------------------------------------------------
ENGINE = r"""
import json, sys, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from face_generator_amd import ops
from face_generator_amd._lib import FgError
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib = ctx.lib

def say(s):
    sys.stderr.write(s + "\n"); sys.stderr.flush()

def settings(job):
    ctx.set_math(job["math"]); ctx.set_fusion(job["fusion"])
    ctx.check(lib.fg_test_set_wino_wgrad_thresholds(ctx.h, 1 if job.get("hook") else 0, 1 if job.get("hook") else 0))

def run_ops(job):
    # through face_generator_amd.ops with host tensors, as the GPU tests call it
    settings(job)
    say("fg-job " + json.dumps(job))
    E = torch.empty
    if job["kind"] == "conv":
        B, H, W, Cin, Cout, k, up = job["shape"]
        f = 2 if up else 1
        x, w, b, gy = E(B, H, W, Cin), E(Cout, Cin, k, k), E(Cout), E(B, H * f, W * f, Cout)
        calls = dict(fwd=lambda: ops.conv2d_forward(x, w, b, upsample2x=bool(up), ctx=ctx),
                     dgrad=lambda: ops.conv2d_backward_data(gy, w, (H, W), upsample2x=bool(up), ctx=ctx),
                     wgrad=lambda: ops.conv2d_backward_weight(x, gy, k, upsample2x=bool(up), ctx=ctx),
                     wgrad_acc=lambda: ops.conv2d_backward_weight(x, gy, k, upsample2x=bool(up), gw=E(Cout, Cin, k, k), gb=E(Cout), beta=1.0, ctx=ctx))
    else:
        B, K, N = job["shape"]
        x, w, b, gy = E(B, K), E(N, K), E(N), E(B, N)
        calls = dict(fwd=lambda: ops.linear_forward(x, w, b, ctx=ctx), dgrad=lambda: ops.linear_backward_data(gy, w, ctx=ctx),
                     wgrad=lambda: ops.linear_backward_weight(x, gy, ctx=ctx))
    for p in job["passes"]:
        say("fg-pass " + p)
        try:
            calls[p]()
            say("fg-rc 0")
        except FgError as e:
            say("fg-rc -1 " + str(e).replace("\n", " "))

BUF = None
def run_abi(job):
    # straight through the C entries: the return codes, and a workspace of exactly fg_*_workspace_bytes
    global BUF
    settings(job)
    say("fg-job " + json.dumps(job))
    if BUF is None:
        BUF = torch.empty((1 << 25) + 64)
    p = BUF.data_ptr()
    if job["kind"] == "conv":
        B, H, W, Cin, Cout, k, up = job["shape"]
        nb = lib.fg_conv2d_workspace_bytes(B, H, W, Cin, Cout, k, up)
        ws = torch.empty((nb + 3) // 4 + 1)
        pad = (k - 1) // 2
        calls = dict(fwd=lambda: lib.fg_conv2d_forward(ctx.h, p, p, p, p, B, H, W, Cin, Cout, k, pad, up, ws.data_ptr(), nb),
                     dgrad=lambda: lib.fg_conv2d_backward_data(ctx.h, p, p, p, B, H, W, Cin, Cout, k, pad, up, ws.data_ptr(), nb),
                     wgrad=lambda: lib.fg_conv2d_backward_weight(ctx.h, p, p, p, p, 0.0, B, H, W, Cin, Cout, k, pad, up, ws.data_ptr(), nb))
    else:
        B, K, N = job["shape"]
        nb = lib.fg_linear_workspace_bytes(B, K, N)
        ws = torch.empty((nb + 3) // 4 + 1)
        calls = dict(fwd=lambda: lib.fg_linear_forward(ctx.h, p, p, p, p, B, K, N, ws.data_ptr(), nb),
                     dgrad=lambda: lib.fg_linear_backward_data(ctx.h, p, p, p, B, K, N, ws.data_ptr(), nb),
                     wgrad=lambda: lib.fg_linear_backward_weight(ctx.h, p, p, p, p, 0.0, B, K, N, ws.data_ptr(), nb))
    for q in job["passes"]:
        say("fg-pass " + q)
        rc = calls[q]()
        say("fg-rc %%d %%s" %% (rc, lib.fg_last_error(ctx.h).decode() if rc else ""))
"""

# one-layer nets [FG_CONV p=2]: the only public way to a strided convolution.  Passes: create, fwd (train), bwd (both flags); the
# workspace is exactly fg_net_workspace_bytes long
STRIDED_ENGINE = ENGINE + r"""
import ctypes
from face_generator_amd.runtime import make_specs
def run_strided(job):
    settings(job)                       # the fusion bits are read when a net is created
    say("fg-job " + json.dumps(job))
    B, H, W, cin, cout, k = job["shape"]
    h, off = ctypes.c_void_p(), ctypes.c_longlong()
    def done(rc):
        say("fg-rc %%d %%s" %% (rc, lib.fg_last_error(ctx.h).decode() if rc else ""))
        return rc
    say("fg-pass create")
    if done(lib.fg_net_create(ctx.h, make_specs([("CONV", cin, cout, k, (k - 1) // 2, 2)]), 1, cin, H, W, ctypes.byref(h))):
        return
    n = lib.fg_net_num_params(h)
    params, grads, buffers = torch.zeros(n), torch.zeros(n), torch.zeros(1)
    ctx.check(lib.fg_net_bind(h, params.data_ptr(), grads.data_ptr(), buffers.data_ptr()))
    nb = lib.fg_net_workspace_bytes(h, B)
    ws, x, gy = torch.empty((nb + 3) // 4 + 1), torch.empty(B * H * W * cin), torch.empty(B * (H // 2) * (W // 2) * cout)
    gx = torch.empty(x.numel())
    say("fg-pass fwd")
    done(lib.fg_net_forward(h, B, x.data_ptr(), ws.data_ptr(), nb, 1, None, 0, ctypes.byref(off)))
    say("fg-pass bwd")
    done(lib.fg_net_backward_range(h, B, x.data_ptr(), gy.data_ptr(), ws.data_ptr(), nb, 3, gx.data_ptr(), lib.fg_net_num_stages(h) - 1, 0))
    lib.fg_net_destroy(h)
"""

STRIDED = STRIDED_ENGINE + r"""
for j in json.load(open(sys.argv[1])): run_strided(j)
"""

STRIDED_REPLAY = STRIDED_ENGINE + r"""
import test_gpu_strided_conv as TS
for c in TS.STRIDED_CASES:
    for m in ((0, 6) if c != TS.CAP_CASE else (0,)):
        run_strided(dict(list="STRIDED_CASES", kind="sconv", shape=[int(v) for v in c], math=m, fusion=%(default)d))
"""

# the module-level lists of tests/test_gpu_pointwise_paths.py: the same calls on host tensors, no reference computed
POINTWISE_REPLAY = ENGINE + r"""
import test_gpu_pointwise_paths as TQ
def run(lst, name, f):
    say("fg-job " + json.dumps(dict(list=lst, kind="pointwise", case=name, shape=[], math=0, fusion=%(default)d)))
    say("fg-pass run")
    f()
    say("fg-rc 0")
for c in TQ.CAP_CASES: run("CAP_CASES", c[0], lambda: TQ.run_cap(ctx, c, dry=True))
for c in TQ.BN_CASES + [TQ.OFFSET_CASE]: run("BN_CASES", "%%dx%%d" %% c, lambda: TQ.run_bn(ctx, c, dry=True))
for c in TQ.OPT_CASES: run("OPT_CASES", c[0], lambda: TQ.run_opt(ctx, c, dry=True))
for c in TQ.RNG_CASES: run("RNG_CASES", "seed%%x-off%%x-n%%d" %% c, lambda: TQ.run_rng(ctx, c, dry=True))
# the remaining single-process entries, called as their GPU tests call them (tests/test_gpu_sampler.py, test_gpu_memory_contract.py
# test_parzen_min_dist, test_gpu_bench.py): which kernels stand behind fg_rank_scores, fg_image_grid, fg_parzen_min_dist, fg_prof_clock_start
def other_entries():
    E, P = torch.empty, (lambda t: t.data_ptr())
    n = 37
    order, nb = torch.empty(n, dtype=torch.int32), lib.fg_rank_scores_workspace_bytes(37)
    scr = E(nb // 4 + 1)
    ctx.check(lib.fg_rank_scores(ctx.h, P(E(n)), n, 0, P(order), P(scr), nb))
    grid, mm = E(3 * 64 * 64), E(2)
    ctx.check(lib.fg_image_grid(ctx.h, P(E(n, 8, 8, 3)), P(order), 6, 3, 8, 8, 3, 2, 1, P(grid), P(mm)))
    ctx.check(lib.fg_parzen_min_dist(ctx.h, P(E(5, 300)), P(E(300)), P(E(300)), 5, 300, P(E(5)), P(E(1))))
    ctx.check(lib.fg_prof_clock_start(ctx.h, 1.0))
run("OTHER_ENTRIES", "rank-grid-parzen-clock", other_entries)
# the device data path (csrc/image.hip, and the gather of pointwise.hip), one job per case: planning-only calls of the public entries
# at the smallest shapes that select each instance.  The GPU tests that compare them with a reference: test_gpu_dataset.py,
# test_gpu_augment.py, test_gpu_augment_c2f.py, test_gpu_photo_faces.py, test_gpu_augment_draw.py
def data_entries():
    import ctypes
    from face_generator_amd.runtime import DeviceAugmenter
    E, P, PAIRS = torch.empty, (lambda t: t.data_ptr()), [(sl, ol) for sl in (1, 0) for ol in (1, 0)]
    idx, mats, gains = torch.empty(4, dtype=torch.int32), E(4 * 6), E(4)
    def gather():
        for ol in (0, 1): ctx.check(lib.fg_gather_images(ctx.h, P(E(7, 3, 6, 8)), 7, 3, 6, 8, 1, P(idx), 4, P(E(4 * 3 * 6 * 8)), ol))
    def gather_above_cap():     # the row copy at a shape of test_gpu_dataset.py::test_gather_above_the_grid_cap: one unit per image
        n = 4096 + 259
        ctx.check(lib.fg_gather_images(ctx.h, P(E(37, 3, 5, 7)), 37, 3, 5, 7, 1, P(torch.empty(n, dtype=torch.int32)), n, P(E(n * 3 * 5 * 7)), 1))
    def warp_images():
        for sl, ol in PAIRS:
            ctx.check(lib.fg_warp_images(ctx.h, P(E(7 * 3 * 6 * 8)), 7, 3, 6, 8, sl, P(idx), P(mats), P(gains), 4, P(E(4 * 3 * 5 * 7)), 5, 7, ol, 0))
    def warp_c2f(c, hs, s, cs, pairs):
        o = [E(4 * c * s * s) for _ in range(3)]
        for sl, ol in pairs:
            ctx.check(lib.fg_warp_c2f(ctx.h, P(E(7 * c * hs * hs)), 7, c, hs, hs, sl, P(idx), P(mats), P(gains), 4, s, cs, P(o[0]), P(o[1]), P(o[2]), ol, 0))
    def warp_faces(hs, ws, hw, ww, s, cs, pairs):
        o = [E(4 * 3 * s * s) for _ in range(3)]
        for sl, ol in pairs:
            ctx.check(lib.fg_warp_faces(ctx.h, P(E(7 * 3 * hs * ws)), 7, 3, hs, ws, sl, P(idx), P(mats), P(gains), 4, hw, ww, s, cs, P(o[0]),
                                        P(o[1]) if cs else None, P(o[2]) if cs else None, ol, 0))
    def draw(n):
        both = E(7 * n)
        ctx.check(lib.fg_draw_transforms(ctx.h, ctypes.byref(DeviceAugmenter((32, 32)).spec()), 43, 0, n, 40, 40, 32, 32, P(both), P(both) + 24 * n))
    return [("gather", gather), ("gather-above-cap", gather_above_cap), ("warp-images", warp_images), ("warp-c2f", lambda: warp_c2f(3, 6, 4, 2, PAIRS)),
            ("warp-c2f-big", lambda: warp_c2f(3, 64, 64, 32, PAIRS[:1])),
            ("warp-faces", lambda: (warp_faces(9, 11, 5, 6, 4, 2, PAIRS), warp_faces(9, 11, 5, 6, 4, 0, PAIRS[:1]))),
            ("warp-faces-big", lambda: warp_faces(100, 100, 84, 84, 64, 32, PAIRS[:1])),
            ("draw", lambda: draw(4)), ("draw-above-cap", lambda: draw(4096 * 256 + 259))]
DATA_ENTRIES = data_entries()
for name, f in DATA_ENTRIES: run("DATA_ENTRIES", name, f)
"""

REPLAY = ENGINE + r"""
import test_gpu_ops as T, test_gpu_wino as TW, test_gpu_math_modes as TM, test_gpu_fusion as TF, test_gpu_dispatch_paths as TP
D, ALL3 = %(default)d, ["fwd", "dgrad", "wgrad"]
def job(lst, kind, shape, math=0, fusion=D, passes=ALL3, hook=False, **kw):
    return dict(list=lst, kind=kind, shape=[int(v) for v in shape], math=math, fusion=fusion, passes=passes, hook=hook, **kw)
jobs = []
for c in T.CONV_CASES: jobs.append(job("CONV_CASES", "conv", c, passes=ALL3 + ["wgrad_acc"]))
for c in T._fuzz_cases():
    for m in (0, 6): jobs.append(job("_fuzz_cases", "conv", c, math=m))
for c in T.LINEAR_CASES: jobs.append(job("LINEAR_CASES", "lin", c))
for c in TW.CASES:
    for fl in (D, D & ~TW.FG_FUSE_WINOGRAD): jobs.append(job("wino.CASES", "conv", tuple(c) + (3, 0), fusion=fl, passes=["fwd", "dgrad"]))
for lst, cases in (("wino.UP_CASES", TW.UP_CASES), ("wino.ERR_CASES", TW.ERR_CASES)):
    for c in cases:
        for fl in (D, D & ~TW.WINO_ALL): jobs.append(job(lst, "conv", c, fusion=fl, passes=["fwd", "dgrad"]))
for c in TW.WGRAD_CASES:
    for fl in (D, D & ~TW.FG_FUSE_WINOGRAD_WGRAD): jobs.append(job("wino.WGRAD_CASES", "conv", c, fusion=fl, passes=["wgrad"], hook=True))
for c in TM.BF16X6_SHAPES:
    for m in (0, 6): jobs.append(job("math_modes.BF16X6_SHAPES", "conv", c, math=m, fusion=D & ~(32 | 64 | 128)))
for (B, H, W, Cw, Cs, flip) in TF.SLAB_CASES:
    for fl in (TF.FG_FUSE_ALL, TF.FG_FUSE_ALL & ~TF.FG_FUSE_THIN_SLAB):
        jobs.append(job("fusion.SLAB_CASES", "conv", (B, H, W, Cs, Cw, 3, 0) if flip else (B, H, W, Cw, Cs, 3, 0), fusion=fl, passes=["dgrad" if flip else "fwd"]))
for c in TP.PATH_CASES: jobs.append(job("PATH_CASES", c.kind, c.shape, math=c.math, fusion=c.fusion, case=c.name))
for j in jobs: run_ops(j)
"""

SWEEP = ENGINE + r"""
for j in json.load(open(sys.argv[1])): run_abi(j)
"""

NETS = r"""
import sys, torch
sys.path.insert(0, %(root)r)
from face_generator_amd import models, models_c2f, adversarial, adversarial_c2f
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
def say(s):
    sys.stderr.write(s + "\n"); sys.stderr.flush()
def gan(tag, S, B):
    G = models.create_G((3, S, S), 100).cuda(ctx, max_batch=B)
    D = models.create_D((3, S, S)).cuda(ctx, max_batch=B)
    tr = adversarial.Trainer(ctx, G, D, dict(batchSize=B, noiseDim=100))
    assert tr.gan is not None
    for it in range(2):
        say("fg-net %%s %%d" %% (tag, it))
        tr.step_D(torch.zeros(B // 2, S, S, 3), None)
        tr.step_G(B)
    say("fg-net end 0")
gan("32px-B128", 32, 128)
gan("16px-B8", 16, 8)
def c2f(tag, S, B):
    G = models_c2f.create_G((3, S, S), cuda=True, max_batch=B)
    D = models_c2f.create_D((3, S, S), cuda=True, max_batch=B)
    tr = adversarial_c2f.TrainerC2F(ctx, G, D, dict(batchSize=B))
    Z = torch.zeros
    for it in range(2):
        say("fg-net %%s %%d" %% (tag, it))
        tr.step_D(Z(B // 2, S, S, 3), Z(B // 2, S, S, 3), Z(B // 2, S, S, 1), Z(B // 2, S, S, 3))
        tr.step_G(Z(B, S, S, 1), Z(B, S, S, 3))
    say("fg-net end 0")
c2f("c2f64-B8", 64, 8)
# the same nets with the Winograd bits cleared (read when a net is created): the implicit-GEMM kernels with the PReLU in their epilogue
ctx.set_fusion(%(default)d & ~(32 | 64 | 128 | 256))
gan("32px-B128-nowino", 32, 128)
c2f("c2f64-B8-nowino", 64, 8)
say("fg-net end 0")
"""


# nets whose first / last layers have few channels on one side WITHOUT a full set of thin instances (fg_thin_layer false): the gray
# coarse-to-fine generator (2 -> 64 at 3x3: noise + one gray plane), a 4 -> 64 5x5 layer, a 192 -> 1 layer
RECLASSIFIED = r"""
import sys, torch
sys.path.insert(0, %(root)r)
from face_generator_amd import models_c2f
from face_generator_amd.runtime import get_context, DeviceNet
ctx = get_context(-1)
def say(s):
    sys.stderr.write(s + "\n"); sys.stderr.flush()
S, B = 16, 4
G = models_c2f.create_G((1, S, S), cuda=True, max_batch=B)
dn = G.inner.device_net
say("fg-net gray-c2f-G 1")
y = dn.forward(G.combine_device(ctx, torch.zeros(B, S, S, 1), torch.zeros(B, S, S, 1)))
assert tuple(y.shape) == (B, S, S, 1), y.shape
dn.backward(torch.zeros(B, S, S, 1), param_grads=True)
specs = [("CONV", 4, 64, 5, 2), ("PRELU",), ("CONV", 64, 192, 3, 1), ("PRELU",), ("CONV", 192, 1, 3, 1), ("SIGMOID",)]
dn = DeviceNet(ctx, specs, (4, S, S), B)
say("fg-net few-channel-chain 1")
y = dn.forward(torch.zeros(B, S, S, 4))
assert tuple(y.shape) == (B, S, S, 1), y.shape
assert tuple(dn.backward(torch.zeros(B, S, S, 1), True, True).shape) == (B, S, S, 4)
say("fg-net end 0")
"""


# whole layer lists (tests/net_cases.py) as compiled nets: create, forward (train), forward (evaluate), forward (train), backward with
# flags 3, 1 and 2, then fg_net_backward_range split at every stage boundary, in a workspace of exactly fg_net_workspace_bytes.  The
# launch log of thousands of nets is too long to hand to the parent: the child sends its own stderr to a file and prints one JSON
# line per job with the return codes and the launch signatures (and grids) of every pass.
NET_PASSES = ("fwd", "eval", "fwd2", "bwd3", "bwd1", "bwd2", "range")
NET_ENGINE = ENGINE + r"""
import ctypes, fcntl, os, tempfile
from face_generator_amd.runtime import make_specs
import net_cases as NC
LOG = tempfile.NamedTemporaryFile("w+", suffix=".log", delete=False)
# O_APPEND on the descriptor itself (mkstemp does not set it, whatever the mode string): the file is truncated after every job, and
# without it the next write would land at the old offset behind a run of NUL bytes -- the job's first launch line would be lost
fcntl.fcntl(LOG.fileno(), fcntl.F_SETFL, fcntl.fcntl(LOG.fileno(), fcntl.F_GETFL) | os.O_APPEND)
ERR = os.dup(2)
os.dup2(LOG.fileno(), 2)
RD = open(LOG.name)
os.unlink(LOG.name)
def guarded(f):
    try:
        f()
    except BaseException:
        import traceback
        os.write(ERR, traceback.format_exc().encode())
        raise
lib.fg_net_mask_elems.restype = ctypes.c_longlong
def launches():
    out = []
    for l in RD.read().splitlines():
        assert "\0" not in l, "a hole in the launch log"
        if l.startswith("fg-launch "): out.append(l)
    return out
def run_net(job, grids=False):
    settings(job)                       # the fusion bits are read when a net is created
    layers, (c, hh, w), B = [NC.pad(l) for l in job["layers"]], job["dims"], job["batch"]
    res = dict(job, rc={}, log={})
    h, off = ctypes.c_void_p(), ctypes.c_longlong()
    launches()
    def done(p, rc):
        res["rc"][p] = [rc, lib.fg_last_error(ctx.h).decode() if rc else ""]
        res["log"].setdefault(p, []).extend(launches())
        return rc
    def finish():
        os.ftruncate(LOG.fileno(), 0); RD.seek(0)
        if not grids:
            res["log"] = {p: sorted(set(" ".join(l.split(" grid=")[0:1] + l.split(" ")[-2:]) for l in v)) for p, v in res["log"].items()}
        print(json.dumps(res), flush=True)
    if done("create", lib.fg_net_create(ctx.h, make_specs(layers), len(layers), c, hh, w, ctypes.byref(h))):
        return finish()
    n, nbuf, ns = lib.fg_net_num_params(h), lib.fg_net_num_buffers(h), lib.fg_net_num_stages(h)
    res["stages"] = ns
    P, G, Bf = torch.empty(max(n, 1)), torch.empty(max(n, 1)), torch.empty(max(nbuf, 1))
    ctx.check(lib.fg_net_bind(h, P.data_ptr(), G.data_ptr(), Bf.data_ptr()))
    nb = lib.fg_net_workspace_bytes(h, B)
    ws, x = torch.empty((nb + 3) // 4), torch.empty(B * c * hh * w)
    gx = torch.empty(x.numel())
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.fg_net_out_dims(h, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow))
    gy = torch.empty(B * oc.value * oh.value * ow.value)
    nm = lib.fg_net_num_masks(h)
    ms = [torch.ones(max(1, lib.fg_net_mask_elems(h, i, B))) for i in range(nm)]
    mp = (ctypes.c_void_p * max(nm, 1))(*[m.data_ptr() for m in ms])
    F = lambda train: lib.fg_net_forward(h, B, x.data_ptr(), ws.data_ptr(), nb, train, mp if nm else None, nm, ctypes.byref(off))
    R = lambda fl, a, b: lib.fg_net_backward_range(h, B, x.data_ptr(), gy.data_ptr(), ws.data_ptr(), nb, fl, gx.data_ptr(), a, b)
    ok = not done("fwd", F(1)) and not done("eval", F(0)) and not done("fwd2", F(1))
    if ok:
        for fl in (3, 1, 2):
            done("bwd%%d" %% fl, R(fl, ns - 1, 0))
        rc = 0
        for s in range(1, ns):
            rc = rc or R(3, ns - 1, s) or R(3, s - 1, 0)
        done("range", rc)
    lib.fg_net_destroy(h)
    finish()
"""

NET_SWEEP = NET_ENGINE + r"""
guarded(lambda: [run_net(j) for j in json.load(open(sys.argv[1]))])
"""

NET_REPLAY = NET_ENGINE + r"""
def replay_all():
  for c in NC.NET_CASES:
    run_net(dict(list="NET_CASES", kind="net", case=c.name, dims=list(c.dims), layers=[list(l) for l in c.layers], batch=c.batch, math=c.math,
                 fusion=c.fusion, shape=[]), grids=True)
  for (name, row, dims, layers, msg) in NC.REFUSED_CASES:
    run_net(dict(list="REFUSED_CASES", kind="net", case=name, dims=list(dims), layers=[list(l) for l in layers], batch=2, math=0,
                 fusion=%(default)d, shape=[]))
guarded(replay_all)
"""

# SYNC_CASES of tests/sync_cases.py with sync-BN on: one net per shard, each driven through its own pauses (no reduce: nothing reads
# the buffer in a planning-only context).  Per pass the fg_net_sync_count of every pause, per shard; then the capacity refusal:
# a buffer of 2 C doubles for the widest BatchNorm in the forward pass and, behind a forward that ran, in the backward pass.
# Kept out of net_replay: the ledger holds the four sync kernels as `other-entry`, launched by no replay of the coverage audit.
SYNC_PASSES = ("fwd", "eval", "fwd2", "bwd3", "bwd1", "bwd2", "range")
SYNC_REPLAY = NET_ENGINE + r"""
import sync_cases as SC
def run_sync(c):
    job = dict(list="SYNC_CASES", kind="net", case=c.name, dims=list(c.dims), layers=[list(l) for l in c.layers], batch=c.batch,
               shards=list(c.shards), math=c.math, fusion=c.fusion, shape=[])
    settings(job)
    layers, (ci, hh, w) = [NC.pad(l) for l in c.layers], c.dims
    res = dict(job, rc={}, log={}, pauses={}, cap={})
    launches()
    def done(p, rc):
        if p not in res["rc"] or not res["rc"][p][0]:
            res["rc"][p] = [rc, lib.fg_last_error(ctx.h).decode() if rc else ""]
        res["log"].setdefault(p, []).extend(launches())
        return rc
    cap = SC.capacity(c)
    sync = torch.empty(cap, dtype=torch.float64)
    for B in c.shards:
        h, off = ctypes.c_void_p(), ctypes.c_longlong()
        ctx.check(lib.fg_net_create(ctx.h, make_specs(layers), len(layers), ci, hh, w, ctypes.byref(h)))
        n, nbuf, ns = lib.fg_net_num_params(h), lib.fg_net_num_buffers(h), lib.fg_net_num_stages(h)
        res["stages"] = ns
        P, G, Bf = torch.empty(max(n, 1)), torch.empty(max(n, 1)), torch.empty(max(nbuf, 1))
        ctx.check(lib.fg_net_bind(h, P.data_ptr(), G.data_ptr(), Bf.data_ptr()))
        nb = lib.fg_net_workspace_bytes(h, B)
        ws, x = torch.empty((nb + 3) // 4), torch.empty(B * ci * hh * w)
        gx = torch.empty(x.numel())
        oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib.fg_net_out_dims(h, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow))
        gy = torch.empty(B * oc.value * oh.value * ow.value)
        nm = lib.fg_net_num_masks(h)
        ms = [torch.ones(max(1, lib.fg_net_mask_elems(h, i, B))) for i in range(nm)]
        mp = (ctypes.c_void_p * max(nm, 1))(*[m.data_ptr() for m in ms])
        F = lambda train: lib.fg_net_forward(h, B, x.data_ptr(), ws.data_ptr(), nb, train, mp if nm else None, nm, ctypes.byref(off))
        FR = lambda: lib.fg_net_forward_resume(h, ctypes.byref(off))
        R = lambda fl, a, b: lib.fg_net_backward_range(h, B, x.data_ptr(), gy.data_ptr(), ws.data_ptr(), nb, fl, gx.data_ptr(), a, b)
        BR = lambda: lib.fg_net_backward_resume(h)
        def drive(rc, resume, counts):
            while rc == 1:
                counts.append(lib.fg_net_sync_count(h)); rc = resume()
            return rc
        def run(p, start, resume):
            counts = []
            rc = done(p, drive(start(), resume, counts))
            res["pauses"].setdefault(p, []).append(counts)
            return rc
        done("plain", F(1))              # sync off, at the shard's batch: does the producer's epilogue carry the statistics?
        ctx.check(lib.fg_net_set_sync_bn(h, 1, sync.data_ptr(), cap))
        ok = not run("fwd", lambda: F(1), FR) and not run("eval", lambda: F(0), FR) and not run("fwd2", lambda: F(1), FR)
        if ok:
            for fl in (3, 1, 2):
                run("bwd%%d" %% fl, lambda: R(fl, ns - 1, 0), BR)
            rc, per = 0, []
            for s in range(1, ns):
                counts = []
                rc = rc or drive(R(3, ns - 1, s), BR, counts) or drive(R(3, s - 1, 0), BR, counts)
                per.append(counts)
            done("range", rc)
            res["pauses"].setdefault("range", []).append(per)
            # the capacity refusal, backward: the forward above ran to its end
            ctx.check(lib.fg_net_set_sync_bn(h, 1, sync.data_ptr(), cap - 1))
            counts = []
            rc = drive(R(3, ns - 1, 0), BR, counts)
            res["cap"].setdefault("bwd", []).append([rc, lib.fg_last_error(ctx.h).decode() if rc else "", counts, BR()])
            # ... forward, then what follows it
            counts = []
            rc = drive(F(1), FR, counts)
            row = [rc, lib.fg_last_error(ctx.h).decode() if rc else "", counts, FR(), R(3, ns - 1, 0)]
            ctx.check(lib.fg_net_set_sync_bn(h, 1, sync.data_ptr(), cap))
            row.append(drive(F(1), FR, []))
            res["cap"].setdefault("fwd", []).append(row)
            res["log"].setdefault("cap", []).extend(launches())
        lib.fg_net_destroy(h)
    os.ftruncate(LOG.fileno(), 0); RD.seek(0)
    print(json.dumps(res), flush=True)
guarded(lambda: [run_sync(c) for c in SC.SYNC_CASES])
"""


# whole G / D pairs (tests/gan_cases.py) at the step level: both nets and the step object created with workspaces of exactly
# fg_net_workspace_bytes / fg_gan_workspace_bytes, then per batch and per way of giving noise and masks (NULL: drawn by the library;
# explicit) fg_step_D, fg_step_G, fg_step_D | FG_STEP_NO_UPDATE + fg_gan_update(0), fg_step_G | FG_STEP_NO_UPDATE + fg_gan_update(1).
# A pass is named "<closure>@<batch><n|x>"; a replayed case also runs the scenarios of tests/test_gan_steps_host.py (c), (d) and the
# bucketed backward of its generator on transport-less communicators.
GAN_CLOSURES = ("D", "G", "Dn", "uD", "Gn", "uG")
GAN_ENGINE = NET_ENGINE + r"""
import re
import gan_cases as GC
from face_generator_amd.runtime import DeviceNet, FusedGan
lib.fg_net_mask_elems.restype = ctypes.c_longlong

class Pair:
    def __init__(self, job):
        self.job, self.table, self.maxB = job, job["table"], job["max_batch"]
        self.dnG = DeviceNet(ctx, [NC.pad(l) for l in job["glayers"]], tuple(job["gdims"]), self.maxB)
        self.dnD = DeviceNet(ctx, [NC.pad(l) for l in job["dlayers"]], tuple(job["ddims"]), self.maxB)
        for dn in (self.dnG, self.dnD):
            assert dn.ws.numel() * 4 - lib.fg_net_workspace_bytes(dn.h, self.maxB) in (0, 1, 2, 3)
        self.gan = FusedGan(ctx, self.dnG, self.dnD, self.table, self.maxB)
        self.gan.set_seeds(3, 0, 777, 0)
        cfg = job.get("cfg")
        if cfg:
            p = cfg["pen"]
            self.gan.set_penalty(0, p["D_L1"], p["D_L2"], p["D_clamp"]); self.gan.set_penalty(1, p["G_L1"], p["G_L2"], p["G_clamp"])
            self.gan.set_optimizer(0, *cfg["optD"]); self.gan.set_optimizer(1, *cfg["optG"])
            if cfg["bucket"]:
                ctx.check(lib.fg_test_set_gan_bucket_target(self.gan.h, cfg["bucket"]))
        self.gan._bind()
        c, h, w = job["ddims"]
        self.img, self.nz = c * h * w, (h * w if self.table else job["gdims"][0])
        E = torch.zeros
        self.real, self.cond, self.noise = E(self.maxB * self.img), E(self.maxB * self.img), E(self.maxB * self.nz)
        self.masks = [torch.ones(max(1, lib.fg_net_mask_elems(self.dnD.h, i, self.maxB))) for i in range(self.dnD.n_masks)]
        self.mp = (ctypes.c_void_p * max(1, len(self.masks)))(*[m.data_ptr() for m in self.masks])
    def call(self, which, B, explicit, flags=0, real=True):
        P = lambda t, on=True: t.data_ptr() if on else None
        nz, mp = P(self.noise, explicit), (self.mp if explicit and self.masks else None)
        if which == "D":
            return lib.fg_step_D(self.gan.h, B, P(self.real, real), P(self.cond, self.table), P(self.cond, self.table), nz, mp, flags)
        return lib.fg_step_G(self.gan.h, B, P(self.cond, self.table), nz, mp, flags)
    def offsets(self):
        a, b = ctypes.c_longlong(), ctypes.c_longlong()
        ctx.check(lib.fg_gan_get_offsets(self.gan.h, ctypes.byref(a), ctypes.byref(b)))
        return [a.value, b.value]
    def d_output_count(self):
        o, c = ctypes.c_longlong(), ctypes.c_longlong()
        ctx.check(lib.fg_gan_buffer(self.gan.h, 7, ctypes.byref(o), ctypes.byref(c)))
        return c.value

def run_pair(job, grids=False):
    settings(dict(math=0, fusion=%(default)d))
    res = dict(job, rc={}, log={})
    launches()
    def done(p, rc, msg=None):
        res["rc"][p] = [rc, (lib.fg_last_error(ctx.h).decode() if msg is None else msg) if rc else ""]
        res["log"].setdefault(p, []).extend(launches())
        return rc
    def finish():
        os.ftruncate(LOG.fileno(), 0); RD.seek(0)
        if not grids:
            res["log"] = {p: sorted(set(" ".join(l.split(" grid=")[0:1] + l.split(" ")[-2:]) for l in v)) for p, v in res["log"].items()}
        print(json.dumps(res), flush=True)
    try:
        pr = Pair(job)
    except FgError as e:
        m = re.match(r"libfacegen_hip error (-?\d+): (.*)", str(e), re.S)
        done("create", int(m.group(1)) if m else -99, m.group(2) if m else str(e))
        return finish()
    done("create", 0)
    for B in job["batches"]:
        for explicit in (False, True):
            tag = "@%%d%%s" %% (B, "x" if explicit else "n")
            done("D" + tag, pr.call("D", B, explicit))
            done("G" + tag, pr.call("G", B, explicit))
            if not done("Dn" + tag, pr.call("D", B, explicit, 1)):
                done("uD" + tag, lib.fg_gan_update(pr.gan.h, 0))
            if not done("Gn" + tag, pr.call("G", B, explicit, 1)):
                done("uG" + tag, lib.fg_gan_update(pr.gan.h, 1))
    if job.get("scenarios"):
        scenarios(job, res, done)
    finish()

def scenarios(job, res, done):
    M = job["max_batch"]
    extra = res.setdefault("extra", {})
    # (c) a refused step leaves the offsets of the random streams alone: the same calls on a pair that is refused in between and on a
    # fresh twin with the same seeds
    def drawn(refusals):
        pr = Pair(job)
        out = [pr.offsets()]
        assert pr.call("D", M, False) == 0 and pr.call("G", M, False) == 0
        out.append(pr.offsets())
        codes = refusals(pr) if refusals else {}
        out.append(pr.offsets())
        assert pr.call("D", M, False) == 0
        out.append(pr.offsets())
        assert pr.call("G", 2, False) == 0
        out.append(pr.offsets())
        return out, codes
    def refusals(pr):
        g, codes = pr.gan, {}
        codes["fg_step_D at an odd batch"] = pr.call("D", M - 1, False)
        codes["fg_step_G at an odd batch"] = pr.call("G", M - 1, False)
        codes["fg_step_D above max_batch"] = pr.call("D", M + 2, False)
        codes["fg_step_G above max_batch"] = pr.call("G", M + 2, False)
        codes["fg_step_D with a null real"] = pr.call("D", M, False, real=False)
        key = pr.gan._bound
        ctx.check(lib.fg_gan_bind_workspaces(g.h, key[0], key[1] * 4, key[2], 16))
        codes["FG_ERR_WORKSPACE: fg_step_D with D's workspace bound too small"] = pr.call("D", M, False)
        codes["FG_ERR_WORKSPACE: fg_step_G with D's workspace bound too small"] = pr.call("G", M, False)
        ctx.check(lib.fg_gan_bind_workspaces(g.h, key[0], 16, key[2], key[3] * 4))
        codes["FG_ERR_WORKSPACE: fg_step_D with G's workspace bound too small"] = pr.call("D", M, False)
        codes["FG_ERR_WORKSPACE: fg_step_G with G's workspace bound too small"] = pr.call("G", M, False)
        ctx.check(lib.fg_gan_bind_workspaces(g.h, key[0], key[1] * 4, key[2], key[3] * 4))
        return codes
    used, codes = drawn(refusals)
    twin, _ = drawn(None)
    extra["offsets"] = dict(used=used, twin=twin, codes=codes)
    # (d) FG_GAN_D_OUTPUT reports the batch of the last closure
    if M >= 4:
        pr = Pair(job)
        assert pr.call("D", M, True) == 0 and pr.call("G", M - 2, True) == 0
        a = pr.d_output_count()
        assert pr.call("D", M, True) == 0
        extra["d_output"] = dict(M=M, after_D_then_G=a, after_G_then_D=pr.d_output_count())
    launches()
    # item 4: the bucketed generator backward on a transport-less communicator
    pr0 = Pair(job)
    ns = lib.fg_net_num_stages(pr0.dnG.h)
    if ns >= 3:
        from face_generator_amd.distributed import DryCollective
        nP = lib.fg_net_num_params(pr0.dnG.h)
        stages = []
        for s in range(ns):
            lo, hi = ctypes.c_longlong(), ctypes.c_longlong()
            ctx.check(lib.fg_net_stage_params(pr0.dnG.h, s, ctypes.byref(lo), ctypes.byref(hi)))
            stages.append([lo.value, hi.value])
        runs = []
        for world in (2, 4):
            for target in (1, max(2, nP // 3), nP):
                pr = Pair(job)
                coll = DryCollective(ctx, 0, world)
                pr.gan.set_comm(coll, sync_bn=False, overlap=1)
                ctx.check(lib.fg_test_set_gan_bucket_target(pr.gan.h, target))
                assert pr.call("D", M, True) == 0
                ctx.check(lib.fg_gan_finish_pending(pr.gan.h))
                coll.schedule(reset=True)
                launches()
                assert pr.call("G", M, True) == 0
                runs.append(dict(world=world, target=target, schedule=coll.schedule(reset=True), log=launches()))
                pr.gan.set_comm(None)
        extra["buckets"] = dict(nP=nP, stages=stages, runs=runs)
"""

GAN_SWEEP = GAN_ENGINE + r"""
guarded(lambda: [run_pair(j) for j in json.load(open(sys.argv[1]))])
"""

GAN_REPLAY = GAN_ENGINE + r"""
def replay_all():
    for c in GC.GAN_CASES:
        run_pair(dict(list="GAN_CASES", kind="gan", case=c.name, gdims=list(c.gdims), glayers=[list(l) for l in c.glayers], ddims=list(c.ddims),
                      dlayers=[list(l) for l in c.dlayers], table=c.table, max_batch=c.max_batch, batches=GC.SWEEP_BATCHES(c.max_batch), shape=[], math=0,
                      fusion=%(default)d, cfg=dict(optD=list(c.optD), optG=list(c.optG), pen=c.pen, bucket=c.bucket), scenarios=True), grids=True)
    for (name, row, gd, gl, dd, dl, table, mb, msg) in GC.REFUSED_GAN_CASES:
        run_pair(dict(list="REFUSED_GAN_CASES", kind="gan", case=name, gdims=list(gd), glayers=[list(l) for l in gl], ddims=list(dd),
                      dlayers=[list(l) for l in dl], table=table, max_batch=mb, batches=[2], shape=[], math=0, fusion=%(default)d))
guarded(replay_all)
"""


# SYNC_STEP_CASES of tests/sync_cases.py: the BN-bearing GAN_CASES on a transport-less communicator, rank 0 of 2, with sync-BN on --
# every iteration's D-step and G-step with explicit noise and masks, fg_gan_finish_pending behind each when the exchange overlaps.
# One JSON line per (case, overlap, bucket target): the text of fg_comm_schedule over the whole run and the launch log.
SYNC_GAN_REPLAY = GAN_ENGINE + r"""
import sync_cases as SC
from face_generator_amd.distributed import DryCollective
def run_sync_pair(c, overlap, bucket):
    settings(dict(math=0, fusion=%(default)d))
    job = dict(list="SYNC_STEP_CASES", kind="gan", case=c.name, gdims=list(c.gdims), glayers=[list(l) for l in c.glayers], ddims=list(c.ddims),
               dlayers=[list(l) for l in c.dlayers], table=c.table, max_batch=c.max_batch, batches=list(c.iters), shape=[], math=0, fusion=%(default)d,
               cfg=dict(optD=list(c.optD), optG=list(c.optG), pen=c.pen, bucket=0), overlap=overlap, bucket=bucket)
    res = dict(job, rc={}, log={})
    launches()
    pr = Pair(job)
    coll = DryCollective(ctx, 0, 2)
    ctx.check(lib.fg_gan_set_comm(pr.gan.h, coll.h, 1, overlap))
    target = SC.bucket_target(bucket, lib.fg_net_num_params(pr.dnG.h))
    if target:
        ctx.check(lib.fg_test_set_gan_bucket_target(pr.gan.h, target))
    rc = 0
    for B in c.iters:
        for which in "DG":
            rc = rc or pr.call(which, B, True)
            if overlap:
                rc = rc or lib.fg_gan_finish_pending(pr.gan.h)
    res["rc"]["run"] = [rc, lib.fg_last_error(ctx.h).decode() if rc else ""]
    res["schedule"] = coll.schedule(reset=True)
    res["log"]["run"] = launches()
    ctx.check(lib.fg_gan_set_comm(pr.gan.h, None, 0, 1))
    coll.close()
    os.ftruncate(LOG.fileno(), 0); RD.seek(0)
    print(json.dumps(res), flush=True)
guarded(lambda: [run_sync_pair(GC.BY_NAME[n], ov, bk) for n in SC.SYNC_STEP_CASES for ov, bk in SC.step_settings(n)])
"""


@memo
def sync_gan_replay():
    """SYNC_STEP_CASES x SC.step_settings on a dry two-rank communicator with sync-BN on -> parsed jobs with `schedule` (the lines of
    fg_comm_schedule over the whole run)"""
    p = _run_stdout(SYNC_GAN_REPLAY)
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0, err[-3000:]
    return _parse_net_jobs(out.splitlines())


@memo
def gan_replay():
    """GAN_CASES and REFUSED_GAN_CASES of tests/gan_cases.py under each case's own optimizers and penalties -> parsed jobs (full launch
    lines per pass; "extra": the scenarios of tests/test_gan_steps_host.py)"""
    p = _run_stdout(GAN_REPLAY)
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0, err[-3000:]
    return _parse_net_jobs(out.splitlines())


@memo
def gan_sweep():
    """every generated pair at every even batch of {2, 4, 6, max_batch - 2, max_batch} -> parsed jobs (unique signatures per pass)"""
    import tempfile
    import gan_cases as GC
    jobs = [dict(list="gan-sweep", kind="gan", idx=i, gdims=list(gd), glayers=[list(l) for l in gl], ddims=list(dd), dlayers=[list(l) for l in dl], table=t,
                 max_batch=mb, batches=GC.SWEEP_BATCHES(mb), shape=[], math=0, fusion=FG_FUSE_DEFAULT)
            for i, (gd, gl, dd, dl, t, mb) in enumerate(GC.random_pairs(GC.SWEEP_SEED, GC.SWEEP_N))]
    workers = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
    files, procs = [], []
    try:
        for k in range(workers):
            f = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
            json.dump(jobs[k::workers], f); f.close()
            o = tempfile.NamedTemporaryFile("w+", suffix=".out", delete=False)
            files += [f.name, o.name]
            procs.append((_run_stdout(GAN_SWEEP, [f.name], out=o), o))
        res = []
        for p, o in procs:
            _, err = p.communicate(timeout=900)
            assert p.returncode == 0, err[-3000:]
            o.seek(0)
            res += _parse_net_jobs(o.read().splitlines())
            o.close()
    finally:
        for f in files:
            os.unlink(f)
    return sorted(res, key=lambda j: j["idx"])


def _parse_net_jobs(lines):
    """JSON lines of the net children -> jobs in the shape parse_jobs gives: rc {pass: (code, message)}, sigs, grids"""
    jobs = []
    for l in lines:
        if not l.startswith("{"):
            continue
        j = json.loads(l)
        j["rc"] = {p: tuple(v) for p, v in j["rc"].items()}
        j["sigs"], j["grids"] = {}, {}
        for p, v in j.pop("log").items():
            j["sigs"][p], j["grids"][p] = [], []
            for line in v:
                m = LAUNCH_RE.match(line)
                if m:
                    j["sigs"][p].append(sig_of(line))
                    j["grids"][p].append((kernel_of(m.group(1)),) + tuple(int(g) for g in m.group(2, 3, 4)))
                else:           # the sweep's compact form: "fg-launch <site> block=N lds=N"
                    m = re.match(r"^fg-launch (.*) block=(\d+) lds=(\d+)$", line)
                    assert m, line
                    j["sigs"][p].append((m.group(1), int(m.group(2)), int(m.group(3))))
        jobs.append(j)
    return jobs


def _run_stdout(code, args=(), out=subprocess.PIPE):
    env = dict(os.environ, FG_LAUNCH_LOG="1", OMP_NUM_THREADS="1")     # (several children side by side: one thread each)
    fmt = dict(root=ROOT, tests=os.path.join(ROOT, "tests"), default=FG_FUSE_DEFAULT)
    return subprocess.Popen([sys.executable, "-c", code % fmt] + list(args), env=env, stdout=out, stderr=subprocess.PIPE, text=True)


@memo
def net_replay():
    """NET_CASES and REFUSED_CASES of tests/net_cases.py under each case's own settings -> parsed jobs (full launch lines)"""
    p = _run_stdout(NET_REPLAY)
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0, err[-3000:]
    return _parse_net_jobs(out.splitlines())


@memo
def sync_replay():
    """SYNC_CASES of tests/sync_cases.py with sync-BN on -> parsed jobs (full launch lines) with `pauses` {pass: [[sync_count per
    pause] per shard]} and `cap` {"fwd" / "bwd": [row per shard]} (the rows: SYNC_REPLAY above)"""
    p = _run_stdout(SYNC_REPLAY)
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0, err[-3000:]
    return _parse_net_jobs(out.splitlines())


def net_sweep(n=None, workers=None):
    """every generated layer list x {fusion 503, 23, 502} x {math 0, 6} -> parsed jobs (unique signatures per pass, no grids)"""
    import tempfile
    import net_cases as NC
    lists = NC.random_layer_lists(NC.SWEEP_SEED, NC.SWEEP_N if n is None else n)
    jobs = [dict(list="net-sweep", kind="net", idx=i, dims=list(d), layers=[list(l) for l in L], batch=B, math=m, fusion=f, shape=[])
            for i, (d, L, B) in enumerate(lists) for f in NC.FUSIONS for m in NC.MATHS]
    workers = workers or max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
    files, procs = [], []
    try:
        for k in range(workers):
            f = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
            json.dump(jobs[k::workers], f); f.close()
            o = tempfile.NamedTemporaryFile("w+", suffix=".out", delete=False)     # (a file, not a pipe: nobody reads until the end)
            files += [f.name, o.name]
            procs.append((_run_stdout(NET_SWEEP, [f.name], out=o), o))
        res = []
        for p, o in procs:
            _, err = p.communicate(timeout=900)
            assert p.returncode == 0, err[-3000:]
            o.seek(0)
            res += _parse_net_jobs(o.read().splitlines())
            o.close()
    finally:
        for f in files:
            os.unlink(f)
    return sorted(res, key=lambda j: (j["idx"], j["fusion"], j["math"]))


def reclassified_net_launches():
    """{tag: [launch line, ...]} of forward + backward of the nets above, planning-only"""
    return _split_nets(_run(RECLASSIFIED), "1")


def _run(code, args=(), timeout=900):
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    fmt = dict(root=ROOT, tests=os.path.join(ROOT, "tests"), default=FG_FUSE_DEFAULT)
    r = subprocess.run([sys.executable, "-c", code % fmt] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr.splitlines()


def sig_of(line):
    m = LAUNCH_RE.match(line)
    return (m.group(1), int(m.group(5)), int(m.group(6))) if m else None


def parse_jobs(lines):
    """-> [job dict + "rc": {pass: (code, message)}, "sigs": {pass: [signature, ...] in launch order}]"""
    jobs, cur, p = [], None, None
    for l in lines:
        if l.startswith("fg-job "):
            cur = json.loads(l[7:]); cur["rc"] = {}; cur["sigs"] = {}; cur["grids"] = {}
            jobs.append(cur)
        elif l.startswith("fg-pass "):
            p = l[8:]; cur["sigs"][p] = []; cur["grids"][p] = []
        elif l.startswith("fg-rc "):
            parts = l[6:].split(" ", 1)
            cur["rc"][p] = (int(parts[0]), parts[1] if len(parts) > 1 else "")
            p = None
        elif l.startswith("fg-launch ") and p is not None:
            s = sig_of(l)
            assert s, l
            cur["sigs"][p].append(s)
            cur["grids"][p].append((kernel_of(s[0]),) + tuple(int(v) for v in LAUNCH_RE.match(l).group(2, 3, 4)))
    return jobs


def all_sigs(jobs):
    return {s for j in jobs for v in j["sigs"].values() for s in v}


@memo
def replay():
    """the GPU parity lists under the tests' own settings -> parsed jobs"""
    return parse_jobs(_run(REPLAY))


def flops(job, p=None):
    if job["kind"] == "sconv":
        B, H, W, Cin, Cout, k = job["shape"]
        return 2.0 * B * (H // 2) * (W // 2) * k * k * Cin * Cout
    if job["kind"] == "lin":
        B, K, N = job["shape"]
        return 2.0 * B * K * N
    B, H, W, Cin, Cout, k, up = job["shape"]
    return 2.0 * B * H * W * (4 if up else 1) * k * k * Cin * Cout


def sweep_geometries():
    import numpy as np
    rng = np.random.default_rng(SWEEP_SEED)
    conv, lin = [], []
    for i in range(SWEEP_CONV):
        k = int(rng.choice([3, 5, 7]))
        if rng.random() < 0.4:          # few channels on one side, a wide other side: the thin kernels and their neighbours
            a, b = int(rng.choice([1, 2, 3, 4])), int(rng.choice([64, 96, 128, 192, 256, 320, 512]))
            cin, cout = (a, b) if rng.random() < 0.5 else (b, a)
        else:
            cin, cout = int(rng.choice(CHANNELS)), int(rng.choice(CHANNELS))
        up = int(rng.random() < 0.3)
        if rng.random() < 0.5:
            h, w = int(rng.choice([2, 4, 8, 16, 32, 64])), int(rng.choice([2, 4, 8, 16, 32, 64]))
        else:
            h, w = int(rng.integers(3, 41)), int(rng.integers(3, 41))
        b = int(round(2 ** rng.uniform(0, 7)))
        per = h * w * (4 if up else 1) * max(cin, cout)
        b = max(1, min(b, CAP // per))
        conv.append((b, h, w, cin, cout, k, up))
    # Linear: 256-row tiles at tiny K, long reductions at a tiny batch (the 128 x 128 split-K branch of choose_igemm starts at
    # 32768 input features), then random ones
    lin += [(65536, 16, 64), (16384, 32, 512), (8192, 32, 512), (4, 16384, 128), (4, 16384, 192), (65536, 16, 192), (8, 16384, 512),
            (4, 32768, 128), (4, 33000, 128)]
    NS = [1, 2, 7, 10, 64, 100, 128, 192, 256, 320, 512, 1024, 2048, 8192]
    while len(lin) < SWEEP_LINEAR:
        B, K, N = int(round(2 ** rng.uniform(0, 16))), int(round(2 ** rng.uniform(4, 14))), int(rng.choice(NS))
        if B * K > CAP or B * N > CAP or K * N > CAP:
            continue
        lin.append((B, K, N))
    return conv, lin


def sweep():
    """every sweep geometry in math 0 / 6, Winograd bits on / cleared, through the C entries -> parsed jobs"""
    import tempfile
    conv, lin = sweep_geometries()
    jobs = []
    for kind, shapes in (("conv", conv), ("lin", lin)):
        for s in shapes:
            for m in (0, 6):
                for fl in ((FG_FUSE_DEFAULT, FG_FUSE_DEFAULT & ~WINO_ALL, FG_FUSE_DEFAULT & ~THIN_SLAB) if kind == "conv" else (FG_FUSE_DEFAULT,)):
                    if fl == FG_FUSE_DEFAULT & ~THIN_SLAB and (m == 6 or min(s[3], s[4]) > 4):
                        continue        # FG_FUSE_THIN_SLAB picks between two fp32 kernels of the thin 3x3 layers only
                    jobs.append(dict(list="sweep", kind=kind, shape=list(s), math=m, fusion=fl, passes=list(PASSES)))
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(jobs, f)
    try:
        return parse_jobs(_run(SWEEP, [f.name]))
    finally:
        os.unlink(f.name)


STRIDED_SEED, STRIDED_N = 20261019, 200
STRIDED_PASSES = ("create", "fwd", "bwd")


def strided_geometries():
    """(B, H, W, cin, cout, k): k in {3, 5, 7}, even H, W in 2..32, channels from CHANNELS, B in 1..64"""
    import numpy as np
    rng = np.random.default_rng(STRIDED_SEED)
    out = []
    for i in range(STRIDED_N):
        k = int(rng.choice([3, 5, 7]))
        h, w = 2 * int(rng.integers(1, 17)), 2 * int(rng.integers(1, 17))
        cin, cout = int(rng.choice(CHANNELS)), int(rng.choice(CHANNELS))
        out.append((int(round(2 ** rng.uniform(0, 6))), h, w, cin, cout, k))
    return out


def _run_jobs(code, jobs):
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(jobs, f)
    try:
        return parse_jobs(_run(code, [f.name]))
    finally:
        os.unlink(f.name)


def strided_sweep(extra=()):
    """every strided geometry (+ extra ones) in math 0 / 6 with the fusion default and the Winograd bits cleared, as one-layer nets"""
    jobs = [dict(list="strided-sweep", kind="sconv", shape=list(s), math=m, fusion=fl)
            for s in list(strided_geometries()) + list(extra) for m in (0, 6) for fl in (FG_FUSE_DEFAULT, FG_FUSE_DEFAULT & ~WINO_ALL)]
    return _run_jobs(STRIDED, jobs)


@memo
def pointwise_replay():
    """CAP_CASES, BN_CASES, OPT_CASES and RNG_CASES of tests/test_gpu_pointwise_paths.py, then OTHER_ENTRIES and DATA_ENTRIES (the
    single-process entries and the device data path, called as their GPU tests call them) -> parsed jobs (one pass, "run")"""
    return parse_jobs(_run(POINTWISE_REPLAY))


@memo
def strided_replay():
    """STRIDED_CASES of tests/test_gpu_strided_conv.py under that module's settings"""
    return parse_jobs(_run(STRIDED_REPLAY))


def net_launches():
    """{tag: [launch line, ...]} of the second (steady-state) iteration of each baseline pair, plus the set of all kernel texts"""
    return _split_nets(_run(NETS), "1")


def _split_nets(lines, take):
    out, cur = {}, None
    for l in lines:
        if l.startswith("fg-net "):
            _, tag, it = l.split()
            cur = out.setdefault(tag, []) if (tag != "end" and it == take) else None
        elif l.startswith("fg-launch ") and cur is not None:
            cur.append(l)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# launch-site census
# ---------------------------------------------------------------------------------------------------------------------------------
def kernel_of(text):
    """launch-site text (or the first macro argument in the source) -> the kernel's plain name"""
    return re.match(r"\(?\s*([A-Za-z_]\w*)", text).group(1)


def launch_sites():
    """{kernel name: [file:line, ...]} for every hipLaunchKernelGGL( in csrc/*.hip"""
    sites = {}
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith(".hip"):
            continue
        for n, line in enumerate(open(os.path.join(CSRC, fn)), 1):
            for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", line):
                sites.setdefault(m.group(1), []).append("%s:%d" % (fn, n))
    return sites


# ---------------------------------------------------------------------------------------------------------------------------------
# capped-grid census: a launch whose grid is capped below its work count needs a kernel that walks the rest
# ---------------------------------------------------------------------------------------------------------------------------------
def _strip_comments(t):
    t = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), t, flags=re.S)
    return re.sub(r"//[^\n]*", "", t)


def _matching(t, i, op="(", cl=")"):
    """index just behind the bracket that closes the one at t[i]"""
    d = 0
    for j in range(i, len(t)):
        if t[j] == op:
            d += 1
        elif t[j] == cl:
            d -= 1
            if d == 0:
                return j + 1
    raise ValueError("unbalanced %s at %d" % (op, i))


def _split_args(t):
    out, d, cur = [], 0, ""
    for ch in t:
        if ch in "([{":
            d += 1
        elif ch in ")]}":
            d -= 1
        if ch == "," and d == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return out


_NUM = r"(\d+|[A-Z][A-Z0-9_]{2,})"
# `e < N ? e : N`, `min(e, N)` / `std::min`, `if (v > N) v = N`
_CAPS = [re.compile(r"<\s*" + _NUM + r"\s*\?[^:;]*:\s*\1\b"), re.compile(r"\bmin\s*(?:<[^>]*>)?\s*\([^;]*,\s*" + _NUM + r"\s*\)"),
         re.compile(r"\bmin\s*(?:<[^>]*>)?\s*\(\s*(?:\([\w ]+\)\s*)?" + _NUM + r"\s*,"), re.compile(r"if\s*\(\s*[\w.]+\s*>\s*" + _NUM + r"\s*\)\s*[\w.]+\s*=\s*\1\s*;")]


def _cap_in(expr, helpers):
    """-> the cap an expression carries (text of N), or None"""
    for r in _CAPS:                     # an explicit cap first: `if (grid.x > 1024) ..` behind an FG_GRID( is the tighter one
        m = r.search(expr)
        if m:
            return m.group(1)
    for name, n in helpers.items():
        if re.search(r"\b%s\s*\(" % re.escape(name), expr):
            return n
    return None


def capped_launches():
    """-> [dict(kernel, site, cap, dim, strides)] for every hipLaunchKernelGGL( in csrc/*.hip whose grid expression is capped in
    some dimension: through FG_GRID( or another helper whose own definition holds a cap, an explicit min(.., N) / `< N ? .. : N`, or
    a following `if (grid.x > N) grid.x = N`.  `strides` says whether the kernel's body, or a __device__ function it names, reads
    gridDim in that dimension -- a grid-stride loop, or a partition of the work by the number of blocks."""
    texts = {fn: _strip_comments(open(os.path.join(CSRC, fn)).read()) for fn in sorted(os.listdir(CSRC)) if fn.endswith((".hip", ".h"))}
    # helpers: macros and small functions whose definition carries a cap
    helpers = {}
    for fn, t in texts.items():
        for m in re.finditer(r"#define\s+(\w+)\(([^)]*)\)((?:[^\n\\]|\\\n)*)", t):
            c = _cap_in(m.group(3), {})
            if c:
                helpers[m.group(1)] = c
        for m in re.finditer(r"\bstatic\s+inline\s+(?:int|long long|unsigned)\s+(\w+)\s*\([^)]*\)\s*\{", t):
            body = t[m.end() - 1:_matching(t, m.end() - 1, "{", "}")]
            c = _cap_in(body, {})
            if c:
                helpers[m.group(1)] = c
    # bodies of kernels and __device__ functions
    bodies, kernels = {}, set()
    for fn, t in texts.items():
        for m in re.finditer(r"__(global|device)__\s*(?:__launch_bounds__\s*\([^)]*\)\s*)?[^;{}()]*?\b(\w+)\s*\(", t):
            e = _matching(t, m.end() - 1)
            k = re.match(r"\s*(?:const\s*)?\{", t[e:])
            if not k:
                continue
            b0 = e + k.end() - 1
            bodies[m.group(2)] = bodies.get(m.group(2), "") + t[b0:_matching(t, b0, "{", "}")]
            if m.group(1) == "global":
                kernels.add(m.group(2))

    def closure(name):
        seen, todo, out = set(), [name], ""
        while todo:
            n = todo.pop()
            if n in seen or n not in bodies:
                continue
            seen.add(n)
            out += bodies[n]
            todo += [w for w in set(re.findall(r"\b[A-Za-z_]\w*\b", bodies[n])) if w in bodies and w not in kernels]
        return out

    macros = {m.group(1): int(m.group(2)) for t in texts.values() for m in re.finditer(r"#define\s+([A-Z][A-Z0-9_]+)\s+(\d+)\s*$", t, flags=re.M)}
    for t in texts.values():            # one macro named after another (TW_BLOCKS)
        for m in re.finditer(r"#define\s+([A-Z][A-Z0-9_]+)\s+([A-Z][A-Z0-9_]+)\s*$", t, flags=re.M):
            if m.group(2) in macros:
                macros[m.group(1)] = macros[m.group(2)]
    out = []
    for fn, t in texts.items():
        if not fn.endswith(".hip"):
            continue
        for m in re.finditer(r"hipLaunchKernelGGL\s*\(", t):
            if t[max(0, m.start() - 8):m.start()].endswith("#define "):
                continue
            args = _split_args(t[m.end():_matching(t, m.end() - 1) - 1])
            kernel, grid = kernel_of(args[0]), args[1]
            line = t.count("\n", 0, m.start()) + 1
            # the enclosing function's text in front of the launch: definitions of the names the grid expression uses
            start = max(t.rfind("\n}\n", 0, m.start()), 0)
            before = t[start:m.start()]

            def resolve(expr, depth=0):
                comps = [expr]
                mm = re.match(r"^(?:dim3\s*)?\((.*)\)$", expr, flags=re.S) if expr.startswith(("dim3", "(")) else None
                if mm and _matching(expr, expr.index("(")) == len(expr):
                    comps = _split_args(mm.group(1))
                res = []
                for c in comps:
                    extra = ""
                    if depth < 3:
                        for ident in set(re.findall(r"\b[a-z_]\w*\b", c)):
                            # (the definition and the clamp nearest to the launch)
                            for d in list(re.finditer(r"\b(?:dim3|int|long long|unsigned|auto)\s+%s\s*(?:=\s*([^;]*);|\(([^;]*)\)\s*;)" % re.escape(ident), before))[-1:]:
                                sub = d.group(1) if d.group(1) is not None else "dim3(" + d.group(2) + ")"
                                if re.fullmatch(r"\w+", c) and (sub.startswith("dim3") or d.group(2) is not None):
                                    return resolve(sub, depth + 1) if not res else res + resolve(sub, depth + 1)
                                extra += " " + " ".join(resolve(sub, depth + 1))
                            for d in list(re.finditer(r"if\s*\(\s*%s(?:\.x)?\s*>\s*%s\s*\)\s*%s(?:\.x)?\s*=\s*\1\s*;" % (re.escape(ident), _NUM, re.escape(ident)), before))[-1:]:
                                extra += " " + d.group(0)
                    res.append(c + extra)
                return res
            comps = resolve(grid)
            # `if (grid.x > N) grid.x = N` behind a dim3 variable
            if re.fullmatch(r"\w+", grid):
                for d in re.finditer(r"if\s*\(\s*%s\.([xy])\s*>\s*%s\s*\)\s*%s\.\1\s*=\s*\2\s*;" % (grid, _NUM, grid), before):
                    i = "xy".index(d.group(1))
                    while len(comps) <= i:
                        comps.append("")
                    comps[i] = d.group(0) + " " + comps[i]
            for dim, c in zip("xyz", comps):
                cap = _cap_in(c, helpers)
                if cap is None:
                    continue
                body = closure(kernel)
                assert body, "no body found for kernel %s (%s:%d)" % (kernel, fn, line)
                out.append(dict(kernel=kernel, site="%s:%d" % (fn, line), cap=int(cap) if cap.isdigit() else macros[cap], dim=dim, strides=bool(re.search(r"\bgridDim\.%s\b" % dim, body))))
    return out


def at_cap(jobs, kernel, dim, cap):
    """the jobs (parsed logs) with a launch of `kernel` whose grid has `cap` blocks in `dim` (bn_apply_blocks rounds the clamped
    count up to its unit: or a few more): the launcher clamped it"""
    i = 1 + "xyz".index(dim)
    return [j for j in jobs if any(g[0] == kernel and g[i] >= cap for v in j["grids"].values() for g in v)]


def job_id(j):
    return (j["list"], j.get("case") or "x".join(str(v) for v in j["shape"]) + ("-math%d" % j["math"] if j.get("math") else ""))


def all_logs(replay_jobs, strided_jobs, pointwise_jobs, nets):
    """every parsed log as one job list; a net iteration becomes the job ("net", tag)"""
    jobs = list(pointwise_jobs) + list(strided_jobs) + list(replay_jobs)
    for tag, lines in nets.items():
        g = [(kernel_of(sig_of(l)[0]),) + tuple(int(v) for v in LAUNCH_RE.match(l).group(2, 3, 4)) for l in lines]
        jobs.append(dict(list="net", case=tag, shape=[], grids=dict(run=g), sigs=dict(run=[sig_of(l) for l in lines]), rc={}))
    return jobs


def capped_rows(path=LEDGER):
    """the "Capped launchers" table of DISPATCH_COVERAGE.md: {(kernel, dim): (cap, unit of work, covering case)}"""
    rows, inside = {}, False
    for l in open(path):
        if l.startswith("## "):
            inside = l.startswith("## Capped launchers")
        m = re.match(r"^\| `(\w+)` \| ([xyz]) \| (\S+) \| (.*?) \| (.*) \|\s*$", l)
        if inside and m:
            assert (m.group(1), m.group(2)) not in rows
            rows[(m.group(1), m.group(2))] = (m.group(3), m.group(4).strip(), m.group(5).strip())
    return rows


def ledger_rows(path=LEDGER):
    """the ledger table of DISPATCH_COVERAGE.md: {kernel name: (status, note)}; a duplicated name is an error"""
    rows, inside = {}, False
    for l in open(path):
        if l.startswith("## "):
            inside = l.startswith("## Ledger")
        m = re.match(r"^\| `(\w+)` \| (\S+) \| (.*) \|\s*$", l)
        if m and inside:
            assert m.group(1) not in rows, "ledger lists %s twice" % m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3).strip())
    return rows


def smallest_per_signature(jobs):
    best = {}
    for j in jobs:
        for p, sigs in j["sigs"].items():
            if j["rc"].get(p, (0,))[0] != 0:
                continue
            for s in set(sigs):
                f = flops(j)
                if s not in best or f < best[s][0]:
                    best[s] = (f, j["kind"], tuple(j["shape"]), j["math"], j["fusion"], p)
    return best


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "report"
    t0 = time.time()
    rep = replay(); t1 = time.time()
    sw = sweep(); t2 = time.time()
    covered, reach = all_sigs(rep), all_sigs(sw)
    print("replay: %d jobs, %d signatures (%.1f s); sweep: %d jobs, %d signatures (%.1f s)" % (len(rep), len(covered), t1 - t0, len(sw), len(reach), t2 - t1))
    if what == "report":
        best = smallest_per_signature(sw)
        for s in sorted(reach - covered):
            print("UNCOVERED %-48s block %4d lds %6d   smallest: %s" % (s + (best.get(s),)))
    else:
        nets = net_launches()
        netk = {kernel_of(sig_of(l)[0]) for v in nets.values() for l in v}
        # "the replay" as tests/test_dispatch_coverage_host.py takes it: every replayed list, not the conv / linear ones alone
        covered = covered | all_sigs(strided_replay()) | all_sigs(pointwise_replay()) | all_sigs(net_replay()) | all_sigs(gan_replay())
        repk, swk = {kernel_of(s[0]) for s in covered}, {kernel_of(s[0]) for s in reach}
        for k, where in sorted(launch_sites().items()):
            st = "operator" if k in repk else "net-only" if k in netk else "SWEEP-ONLY" if k in swk else "?"
            print("| `%s` | %s | %s |" % (k, st, ", ".join(sorted({w.split(":")[0] for w in where}))))
