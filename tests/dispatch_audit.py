"""Which kernel does the library launch for which geometry?  Answered on the CPU: a planning-only context (get_context(-1)) with
FG_LAUNCH_LOG=1 prints one line per launch, produced by the very host code that decides the launches on a device.  This module
holds the three child programs (replay of the GPU parity lists, the seeded sweep of the public conv / linear entries, one training
iteration of the baseline nets), the parser of their logs and the census of the launch sites in csrc/*.hip.
tests/test_dispatch_coverage_host.py asserts on what they return; tests/DISPATCH_COVERAGE.md is the ledger.

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
            cur = json.loads(l[7:]); cur["rc"] = {}; cur["sigs"] = {}
            jobs.append(cur)
        elif l.startswith("fg-pass "):
            p = l[8:]; cur["sigs"][p] = []
        elif l.startswith("fg-rc "):
            parts = l[6:].split(" ", 1)
            cur["rc"][p] = (int(parts[0]), parts[1] if len(parts) > 1 else "")
            p = None
        elif l.startswith("fg-launch ") and p is not None:
            s = sig_of(l)
            assert s, l
            cur["sigs"][p].append(s)
    return jobs


def all_sigs(jobs):
    return {s for j in jobs for v in j["sigs"].values() for s in v}


def replay():
    """the GPU parity lists under the tests' own settings -> parsed jobs"""
    return parse_jobs(_run(REPLAY))


def flops(job, p=None):
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


def ledger_rows(path=LEDGER):
    """the ledger table of DISPATCH_COVERAGE.md: {kernel name: (status, note)}; a duplicated name is an error"""
    rows = {}
    for l in open(path):
        m = re.match(r"^\| `(\w+)` \| (\S+) \| (.*) \|\s*$", l)
        if m:
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
        repk, swk = {kernel_of(s[0]) for s in covered}, {kernel_of(s[0]) for s in reach}
        for k, where in sorted(launch_sites().items()):
            st = "operator" if k in repk else "net-only" if k in netk else "SWEEP-ONLY" if k in swk else "?"
            print("| `%s` | %s | %s |" % (k, st, ", ".join(sorted({w.split(":")[0] for w in where}))))
