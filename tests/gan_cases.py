"""Small generator / discriminator pairs off the models' shapes, one on each side of every decision of the step level (fg_gan_create,
fg_step_D, fg_step_G, fg_gan_update and gan_optimize of csrc/step.hip): the fixed GAN_CASES, the refused REFUSED_GAN_CASES, the grammar
random_pairs, and the two builders that make the oracle.torch7_nn.GanState and the runtime.FusedGan of one case.  Built on the helpers
of tests/net_cases.py.  Module-level data, no GPU use at import: tests/dispatch_audit.py runs the pairs in the planning-only context
(gan_sweep, gan_replay), tests/test_gan_steps_host.py asserts on the logs, tests/test_gpu_gan_steps.py compares every case with the
float64 oracle.  tests/GAN_STEPS.md is the table of decisions with the case names.

An iteration of a case is a D-step and a G-step at one batch; `iters` lists the batches.  Every case gives D another optimizer than G."""
import collections
import zlib

import numpy as np

import net_cases as NC
from net_cases import PR, BN, SIG, UP, _conv, _sd, _do

SWEEP_SEED, SWEEP_N = 20261020, 300
SWEEP_BATCHES = lambda max_batch: sorted({b for b in (2, 4, 6, max_batch - 2, max_batch) if 2 <= b <= max_batch})
METHODS = dict(adam=0, sgd=1, adagrad=2)
OPT_KERNELS = ("adam_kernel", "pack_jobs_kernel<true>", "sgd_kernel", "adagrad_kernel")

GanCase = collections.namedtuple("GanCase", "name row gdims glayers ddims dlayers table max_batch iters optD optG pen masks gate overlap bucket seed expect absent")

GAN_CASES = []
REFUSED_GAN_CASES = []       # (name, row, gdims, glayers, ddims, dlayers, table, max_batch, part of the message)

# penalties the reference's train.lua starts from, and what a case changes of them
PEN0 = dict(D_L1=0.0, D_L2=1e-4, G_L1=0.0, G_L2=0.0, D_clamp=1.0, G_clamp=5.0)
ADAM_D = ("adam", dict(learningRate=2e-3, beta1=0.5, beta2=0.99, epsilon=1e-6))
SGD_G = ("sgd", dict(learningRate=0.05))


def _gan(name, row, G, D, max_batch, iters, table=0, optD=ADAM_D, optG=SGD_G, pen=None, masks="explicit", gate=None, overlap=None, bucket=0, seed=0,
         expect=None, absent=None):
    (gd, gl), (dd, dl) = G, D
    GAN_CASES.append(GanCase(name, row, tuple(gd), [tuple(l) for l in gl], tuple(dd), [tuple(l) for l in dl], table, max_batch, list(iters), optD, optG,
                             dict(PEN0, **(pen or {})), masks, gate, overlap, bucket, seed, expect or {}, absent or {}))


def g_lin(nz, c, h, w, tail=(SIG,)):
    """G = Linear + View(C, H, W) [+ tail]"""
    return (nz, 1, 1), [("LINEAR", nz, c * h * w), ("VIEW", c, h, w)] + list(tail)


def d_mlp(c, h, w, ndrop=0, hidden=6, p=0.5):
    """D = flatten, Linear -> hidden, PReLU, ndrop Dropout(p) layers, Linear -> 1, Sigmoid"""
    return (c, h, w), [("VIEW", c * h * w), ("LINEAR", c * h * w, hidden), PR] + [_do(p)] * ndrop + [("LINEAR", hidden, 1), SIG]


# ---- row 1: G's output into the second half of D's batch, (B/2) * C*H*W % 4 in {0, 1, 2, 3} -----------------------------------------
_gan("r1-3x3x3-b2-6-8", 1, g_lin(6, 3, 3, 3), d_mlp(3, 3, 3), 8, [2, 6, 8], expect=dict(D=["bce_kernel", "copy_kernel"], G=["bce_kernel"]),
     absent=dict(D=["add_halves_kernel"], G=["copy_kernel", "add_halves_kernel", "rng_multi_kernel"]))       # 27 -> 3, 81 -> 1, 108 -> 0
_gan("r1-1x5x5-b2-4", 1, g_lin(5, 1, 5, 5), d_mlp(1, 5, 5), 4, [2, 4], optD=("sgd", dict(learningRate=0.05)), optG=ADAM_D)      # 25 -> 1, 50 -> 2
_gan("r1-1x4x4-aligned", 1, g_lin(5, 1, 4, 4), d_mlp(1, 4, 4), 4, [2, 4])                                                       # 16, 32 -> 0
_gan("r1-2x3x5-nonsquare", 1, g_lin(7, 2, 3, 5), d_mlp(2, 3, 5), 6, [2, 4, 6], optD=("adagrad", dict(learningRate=0.02)), optG=ADAM_D)     # 30 -> 2, 60 -> 0, 90 -> 2
# ---- row 2: G's last stage, the one that is redirected ------------------------------------------------------------------------------
_gan("r2-linear-view-alone", 2, g_lin(6, 3, 3, 3, tail=()), d_mlp(3, 3, 3), 6, [6, 4])
_gan("r2-linear-view-sigmoid", 2, g_lin(6, 2, 3, 3), d_mlp(2, 3, 3), 6, [6, 2])
_gan("r2-thinout-conv-sigmoid-3ch", 2, ((6, 1, 1), [("LINEAR", 6, 64 * 9), ("VIEW", 64, 3, 3), PR, _conv(64, 3), SIG]), d_mlp(3, 3, 3), 6, [6, 2])
_gan("r2-general-conv-5ch", 2, ((6, 1, 1), [("LINEAR", 6, 8 * 9), ("VIEW", 8, 3, 3), PR, _conv(8, 5)]), d_mlp(5, 3, 3), 6, [6, 2])     # 45 x 3 -> 3
_gan("r2-folded-upconv", 2, ((6, 1, 1), [("LINEAR", 6, 8 * 4), ("VIEW", 8, 2, 2), UP, _conv(8, 8)]), d_mlp(8, 4, 4), 4, [4, 2],
     absent=dict(D=["upsample_fwd_kernel"], G=["upsample_fwd_kernel"]))
_gan("r2-bn-prelu-last", 2, ((6, 1, 1), [("LINEAR", 6, 4 * 9), ("VIEW", 4, 3, 3), BN(4), PR]), d_mlp(4, 3, 3), 6, [6, 4])
# ---- row 3: BatchNorm inside G: batch statistics over B/2 in a D-step and over B in a G-step -----------------------------------------
_gan("r3-bn-inner-3ch", 3, ((6, 1, 1), [("LINEAR", 6, 4 * 9), ("VIEW", 4, 3, 3), BN(4), PR, _conv(4, 3), SIG]), d_mlp(3, 3, 3), 6, [6, 2, 6])
_gan("r3-bn-both-nets", 3, ((6, 1, 1), [("LINEAR", 6, 4 * 9), ("VIEW", 4, 3, 3), BN(4), PR, _conv(4, 4), BN(4)]),
     ((4, 3, 3), [BN(4), PR, ("VIEW", 36), ("LINEAR", 36, 6), PR, ("LINEAR", 6, 1), SIG]), 6, [6, 4])
# ---- row 4: plain / table mode --------------------------------------------------------------------------------------------------------
_TD1 = ((1, 3, 3), [("VIEW", 9), ("LINEAR", 9, 6), PR, ("LINEAR", 6, 1), SIG])
_TD3 = ((3, 3, 3), [_conv(3, 8), PR, ("VIEW", 72), ("LINEAR", 72, 6), PR, _do(), ("LINEAR", 6, 1), SIG])
_ADAM_G = ("adam", dict(learningRate=5e-4, beta1=0.8, beta2=0.95, epsilon=1e-7))
_gan("r4-table-1ch", 4, ((2, 3, 3), [_conv(2, 8), PR, _conv(8, 1)]), _TD1, 6, [2, 6], table=1, optG=_ADAM_G,
     expect=dict(D=["add_halves_kernel", "concat_kernel"], G=["add_kernel", "concat_kernel"]), absent=dict(G=["copy_kernel", "add_halves_kernel"]))      # 9, 27: odd
_gan("r4-table-3ch", 4, ((4, 3, 3), [_conv(4, 8), PR, _conv(8, 3)]), _TD3, 8, [6, 2, 8], table=1, optG=_ADAM_G, pen=dict(D_L1=1e-7, D_L2=0.0))       # 81 -> 1, 27 -> 3, 108 -> 0
# (a dozen Dropout layers in a row keep a unit with probability 0.95 each: at 0.5 nothing would be left to compare)
# ---- row 5: D's dropout masks ---------------------------------------------------------------------------------------------------------
_gan("r5-one-dropout-explicit", 5, g_lin(5, 1, 4, 4), d_mlp(1, 4, 4, 1), 4, [4, 2], absent=dict(D=["rng_multi_kernel"], G=["rng_multi_kernel"]))
_gan("r5-one-dropout-library", 5, g_lin(5, 1, 4, 4), d_mlp(1, 4, 4, 1), 4, [4, 2], masks="library", expect=dict(D=["rng_multi_kernel"], G=["rng_multi_kernel"]))
_gan("r5-spatial-and-dropout-library", 5, g_lin(5, 1, 4, 4), ((1, 4, 4), [_conv(1, 8), PR, _sd(), ("VIEW", 128), ("LINEAR", 128, 6), PR, _do(), ("LINEAR", 6, 1), SIG]), 4,
     [4, 2], masks="library")
_gan("r5-11-dropouts-library", 5, g_lin(5, 1, 4, 4), d_mlp(1, 4, 4, 11, p=0.05), 4, [4, 2], masks="library")       # 12 segments: one launch
_gan("r5-12-dropouts-library", 5, g_lin(5, 1, 4, 4), d_mlp(1, 4, 4, 12, p=0.05), 4, [4, 2], masks="library")       # 13 segments: two launches
_gan("r5-12-dropouts-explicit", 5, g_lin(5, 1, 4, 4), d_mlp(1, 4, 4, 12, p=0.05), 4, [4], masks="explicit")
_gan("r5-no-dropout-library-noise", 5, g_lin(5, 1, 5, 5), d_mlp(1, 5, 5), 4, [2, 4], masks="library", expect=dict(D=["rng_multi_kernel"]))
# ---- row 6: D's shape -----------------------------------------------------------------------------------------------------------------
_gan("r6-concat-table-D", 6, g_lin(6, 3, 3, 3),
     ((3, 3, 3), [("CONCAT_TABLE", 2), ("BRANCH",), ("VIEW", 27), ("LINEAR", 27, 5), ("BRANCH",), _conv(3, 8), PR, ("VIEW", 72), ("LINEAR", 72, 7), PR,
                  ("JOIN_TABLE",), ("LINEAR", 12, 1), SIG]), 6, [6, 2])
_gan("r6-conv-first-D", 6, g_lin(6, 3, 3, 3), ((3, 3, 3), [_conv(3, 8), PR, ("VIEW", 72), ("LINEAR", 72, 6), PR, ("LINEAR", 6, 1), SIG]), 6, [6, 2])
_gan("r6-bn-first-D", 6, ((6, 1, 1), [("LINEAR", 6, 36), ("VIEW", 4, 3, 3), SIG]), ((4, 3, 3), [BN(4), PR, ("VIEW", 36), ("LINEAR", 36, 6), PR, ("LINEAR", 6, 1), SIG]), 6, [6, 2])
# ---- row 7: batches against max_batch -------------------------------------------------------------------------------------------------
_gan("r7-tail-then-max", 7, g_lin(6, 3, 3, 3), d_mlp(3, 3, 3, 1), 8, [2, 8, 4, 8, 6], masks="library")
# ---- row 8: the gate --------------------------------------------------------------------------------------------------------------------
_gan("r8-gate", 8, g_lin(6, 3, 3, 3), d_mlp(3, 3, 3, 1), 6, [6, 6, 6], gate=dict(D=[True, False, True], G=[True, "held", True]))
# ---- row 9: the optimizer wiring, three consecutive steps per net ------------------------------------------------------------------------
_G9, _D9 = g_lin(6, 3, 3, 3), d_mlp(3, 3, 3)
for _n, _oD, _oG in (
        ("adam-nondefault-vs-sgd-plain", ("adam", dict(learningRate=3e-3, beta1=0.6, beta2=0.9, epsilon=1e-4)), ("sgd", dict(learningRate=0.05))),
        ("sgd-momentum-vs-adam", ("sgd", dict(learningRate=0.05, momentum=0.9)), ("adam", {})),
        ("sgd-dampening0-vs-adagrad", ("sgd", dict(learningRate=0.05, momentum=0.9, dampening=0.0)), ("adagrad", dict(learningRate=0.05, learningRateDecay=0.3))),
        ("sgd-nesterov-vs-sgd-decay", ("sgd", dict(learningRate=0.05, momentum=0.8, dampening=0.0, nesterov=True)), ("sgd", dict(learningRate=0.1, learningRateDecay=0.5))),
        ("sgd-weight-decay-vs-sgd-momentum-decay", ("sgd", dict(learningRate=0.05, weightDecay=0.01)), ("sgd", dict(learningRate=0.05, momentum=0.5, learningRateDecay=0.25))),
        ("adagrad-decay-vs-adam", ("adagrad", dict(learningRate=0.05, learningRateDecay=0.5)), ("adam", dict(learningRate=1e-3, beta1=0.7, beta2=0.8, epsilon=1e-5)))):
    _gan("r9-" + _n, 9, _G9, _D9, 6, [6, 6, 6], optD=_oD, optG=_oG, seed=1 if _n.startswith("adagrad") else 0)
# ---- row 10: penalty and clamp ----------------------------------------------------------------------------------------------------------
for _n, _p in (("D-L1-alone", dict(D_L1=1e-2, D_L2=0.0)), ("D-L2-alone", dict(D_L1=0.0, D_L2=5e-2)), ("D-L1-and-L2", dict(D_L1=1e-2, D_L2=5e-2)),
               ("G-L2-drives-the-sign-term", dict(G_L2=2e-2)), ("G-L1-alone-both-zero", dict(G_L1=3e-2)), ("clamp-off", dict(D_clamp=0.0, G_clamp=0.0, G_L2=1e-2)),
               ("clamp-binds", dict(D_clamp=2e-3, G_clamp=2e-4, D_L2=0.0))):
    _gan("r10-" + _n, 10, _G9, _D9, 6, [6, 6], optD=("sgd", dict(learningRate=0.05)), optG=("adagrad", dict(learningRate=0.05)), pen=_p,
         seed={"G-L1-alone-both-zero": 1, "clamp-binds": 2}.get(_n, 0))       # (seeds: tests/test_gan_steps_host.py (e))
# ---- row 11: overlap on a one-rank communicator -----------------------------------------------------------------------------------------
_G11 = ((6, 1, 1), [("LINEAR", 6, 4 * 9), ("VIEW", 4, 3, 3), BN(4), PR, _conv(4, 8), PR, _conv(8, 3), SIG])
for _n, _ov, _bk in (("blocking", 0, 0), ("overlapped", 2, 0), ("overlapped-3-buckets", 2, 1)):
    _gan("r11-" + _n, 11, _G11, d_mlp(3, 3, 3, 1), 6, [6, 2], overlap=_ov, bucket=_bk, optD=("sgd", dict(learningRate=0.05, momentum=0.5)), optG=ADAM_D)

# ---- refused pairs: refused by fg_gan_create / fg_net_create, with a message that names the reason -------------------------------------
REFUSED_GAN_CASES += [
    ("x-dropout-in-G", 5, (5, 1, 1), [("LINEAR", 5, 16), ("VIEW", 1, 4, 4), _sd(), SIG], (1, 4, 4), d_mlp(1, 4, 4)[1], 0, 4, "dropout inside G is not built"),
    ("x-G-D-size-mismatch", 1, (5, 1, 1), [("LINEAR", 5, 16), ("VIEW", 1, 4, 4)], (1, 5, 5), d_mlp(1, 5, 5)[1], 0, 4, "G produces 1x4x4, D takes 1x5x5"),
    ("x-table-G-without-noise-plane", 4, (3, 3, 3), [_conv(3, 3)], (3, 3, 3), _TD3[1], 1, 4, "table mode expects G{noise[1], cond[C]} at D's resolution"),
    ("x-D-two-outputs", 6, (5, 1, 1), [("LINEAR", 5, 16), ("VIEW", 1, 4, 4)], (1, 4, 4), [("VIEW", 16), ("LINEAR", 16, 2), SIG], 0, 4, "D must end in one probability"),
    ("x-D-gemv-behind-flatten", 6, (5, 1, 1), [("LINEAR", 5, 16), ("VIEW", 1, 4, 4)], (1, 4, 4), [("VIEW", 16), ("LINEAR", 16, 1), SIG], 0, 4, "Linear(->1) after a spatial flatten"),
]

BY_NAME = {c.name: c for c in GAN_CASES}
assert len(BY_NAME) == len(GAN_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# the grammar
# ---------------------------------------------------------------------------------------------------------------------------------
def random_pairs(seed, n):
    """-> [(gdims, glayers, ddims, dlayers, table, max_batch)].  G: a vector in front of Linear + View(C, H, W), optionally a short
    spatial run of net_cases' pieces, ending in a Sigmoid or in nothing; in table mode (about one pair in five) a short spatial run on
    C + 1 channels at D's resolution and a convolution back to C.  D: a short spatial run and a linear tail ending Linear(-> 1) +
    Sigmoid with a Linear between any flatten and the -> 1; about one in ten a ConcatTable.  What remains for the library to refuse:
    a dropout layer inside G (the spatial run may draw one)."""
    r = np.random.default_rng(seed)
    pick = lambda xs: xs[int(r.integers(len(xs)))]
    out = []
    while len(out) < n:
        table = 1 if r.random() < 0.2 else 0
        C, H, W = int(pick([1, 2, 3, 4, 8])), int(r.integers(2, 9)), int(r.integers(2, 9))
        max_batch = int(pick([2, 4, 6, 8, 10, 16]))
        if table:
            S, c, h, w = NC._spatial_run(r, C + 1, H, W, int(r.integers(0, 3)))
            if (h, w) != (H, W):
                continue
            gdims, gl = (C + 1, H, W), S + [_conv(c, C, int(pick([3, 5])))]
        else:
            nz = int(pick([4, 10, 100]))
            if r.random() < 0.5:
                gl = [("LINEAR", nz, C * H * W), ("VIEW", C, H, W)]
            else:
                c0 = int(pick([4, 8, 12, 16]))
                h0, w0 = H, W
                S, C, H, W = NC._spatial_run(r, c0, h0, w0, int(r.integers(1, 4)))
                gl = [("LINEAR", nz, c0 * h0 * w0), ("VIEW", c0, h0, w0)] + S
            if r.random() < 0.5 and gl[-1][0] != "SIGMOID":
                gl.append(SIG)
            gdims = (nz, 1, 1)
        if r.random() < 0.1:
            nb = int(r.integers(2, 4))
            dl, tot = [("CONCAT_TABLE", nb)], 0
            for _ in range(nb):
                S, cc, hh, ww = NC._spatial_run(r, C, H, W, int(r.integers(0, 3)), in_branch=True)
                o = int(pick(NC.LINEAR_OUT[1:6]))
                dl += [("BRANCH",)] + S + [("VIEW", cc * hh * ww), ("LINEAR", cc * hh * ww, o)] + ([PR] if r.random() < 0.5 else [])
                tot += o
            dl += [("JOIN_TABLE",)] + ([PR] if r.random() < 0.5 else []) + ([_do()] if r.random() < 0.5 else []) + [("LINEAR", tot, 1), SIG]
        else:
            S, cc, hh, ww = NC._spatial_run(r, C, H, W, int(r.integers(0, 4)))
            o = int(pick(NC.LINEAR_OUT[1:6]))
            dl = S + [("VIEW", cc * hh * ww), ("LINEAR", cc * hh * ww, o)] + ([PR] if r.random() < 0.7 else []) + [_do()] * int(pick([0, 0, 1, 1, 2, 13])) + [("LINEAR", o, 1), SIG]
        ddims = (C, H, W)
        clean = lambda L: [tuple(int(v) if not isinstance(v, (str, float)) else v for v in l) for l in L]
        gl, dl = clean(gl), clean(dl)
        try:
            _, go = NC.walk(gl, gdims)
            _, do = NC.walk(dl, ddims)
        except ValueError:
            continue
        if go[-1].chw != ddims or max(int(np.prod(o.shape)) for o in go + do) * max_batch > 1 << 18:
            continue
        out.append((gdims, gl, ddims, dl, table, max_batch))
    return out


def stated_refusal(glayers):
    """what include/facegen_hip.h rules out among the pairs the grammar emits -> part of the message, or None"""
    return "dropout inside G is not built" if any(l[0] in ("DROPOUT", "SPATIAL_DROPOUT") for l in glayers) else None


# ---------------------------------------------------------------------------------------------------------------------------------
# the two builders
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_opt(case):
    return dict(case.pen, D_optmethod=case.optD[0], G_optmethod=case.optG[0])


def oracle_gan(case, dtype=np.float64):
    """-> oracle.torch7_nn.GanState of the case in `dtype`: seeded parameters (the float32 values are what the device gets), `opt`
    filled from the case, the optimizer tables holding each net's configuration.  st.mods = (G's modules, D's modules) in list order."""
    from oracle import torch7_nn as O
    rng = np.random.default_rng(zlib.crc32(case.name.encode()) + case.seed)
    G, gm = NC.oracle_net(case.glayers, case.gdims, rng)
    D, dm = NC.oracle_net(case.dlayers, case.ddims, rng)
    G.astype(dtype); D.astype(dtype)
    G.training(); D.training()
    if case.table:
        G, D = O.TableNet(O.JoinTable(), G), O.TableNet(O.CAddTable(), D)
        G.astype(dtype); D.astype(dtype)
    st = O.GanState(G, D, oracle_opt(case))
    st.mods = (gm, dm)
    reset_optimizer(st, case)
    return st


def reset_optimizer(st, case, which=None, state=None):
    """the optimizer table of `which` (default: both) <- the case's configuration plus `state` (the keys interruptable_* keep)"""
    for w, (method, cfg) in (("D", case.optD), ("G", case.optG)):
        if which in (None, w):
            tab = dict(cfg, **(state or {}))
            if method == "adam":
                setattr(st, "adam" + w, tab)
            else:
                if not hasattr(st, "optstate"):
                    st.optstate = {}
                st.optstate[(method, w)] = tab
    return st


def optimizer_table(st, case, which):
    from oracle import torch7_nn as O
    return O.optstate_for(st, which)


def penalised(opt, which, p, g):
    """the gradient the optimizer sees: feval_D / feval_G_on_D of the oracle behind the backward pass (penalty, then clamp), on any
    gradient.  G's sign term is multiplied by G_L2 (quirk C4).  tests/test_gan_steps_host.py holds this to the oracle's own lines."""
    dt = p.dtype.type
    l1, l2, clamp = opt[which + "_L1"], opt[which + "_L2"], opt[which + "_clamp"]
    g = g.copy()
    if l1 != 0 or l2 != 0:
        g += np.sign(p) * dt(l1 if which == "D" else l2) + p * dt(l2)
    if clamp != 0:
        np.clip(g, -clamp, clamp, out=g)
    return g


def apply_rule(case, which, p, g, state0, steps):
    """the case's interruptable_* rule of oracle/torch7_nn.py in float64 on the penalised gradient `g`, from the state the device holds
    (state0: its FG_GAN_OPT_STATE_* vector, steps: its step count) -> (parameters, state vector as the device lays it out)"""
    from oracle import torch7_nn as O
    method, cfg = case.optD if which == "D" else case.optG
    n = p.size
    x = p.astype(np.float64).copy()
    s0 = state0.astype(np.float64)
    if method == "adam":
        tab = dict(cfg, t=steps, m=s0[:n].copy(), v=s0[n:2 * n].copy(), denom=np.zeros(n))
        O.interruptable_adam(lambda _: (0.0, g), x, tab)
        return x, np.concatenate([tab["m"], tab["v"]])
    if method == "sgd":
        tab = dict(cfg, evalCounter=steps)
        if cfg.get("momentum", 0) != 0 and steps > 0:
            tab["dfdx"] = s0[:n].copy()
        O.interruptable_sgd(lambda _: (0.0, g), x, tab)
        return x, np.concatenate([tab["dfdx"], s0[n:]]) if "dfdx" in tab else s0
    tab = dict(cfg, evalCounter=steps, paramVariance=s0[:n].copy())
    O.interruptable_adagrad(lambda _: (0.0, g), x, tab)
    return x, np.concatenate([tab["paramVariance"], s0[n:]])


def configure(gan, case):
    """penalties, optimizers and seeds of the case on a runtime.FusedGan"""
    p = case.pen
    gan.set_penalty(0, p["D_L1"], p["D_L2"], p["D_clamp"])
    gan.set_penalty(1, p["G_L1"], p["G_L2"], p["G_clamp"])
    gan.set_optimizer(0, *case.optD)
    gan.set_optimizer(1, *case.optG)
    gan.set_seeds(3 + case.seed, 0, 777 + case.seed, 0)
    if case.bucket:
        gan.ctx.check(gan.lib.fg_test_set_gan_bucket_target(gan.h, case.bucket))
    return gan


def device_gan(ctx, case, arena=None):
    """-> runtime.FusedGan over two DeviceNets, configured from the case.  With an arena (tests/mem_contract.py) every vector of both
    nets and all three workspaces are views of it, each exactly as long as its size function states."""
    from face_generator_amd.runtime import FusedGan
    dnG = NC.device_net(ctx, case.glayers, case.gdims, case.max_batch)
    dnD = NC.device_net(ctx, case.dlayers, case.ddims, case.max_batch)
    if arena is None:
        return configure(FusedGan(ctx, dnG, dnD, case.table, case.max_batch), case)
    from test_gpu_memory_contract_nets import rehouse

    class ArenaGan(FusedGan):
        def __init__(self):
            import ctypes
            self.ctx, self.lib, self.dnG, self.dnD, self.table, self.max_batch = ctx, ctx.lib, dnG, dnD, case.table, case.max_batch
            rehouse(ctx, arena, dnG, "G"); rehouse(ctx, arena, dnD, "D")
            nbytes = ctx.lib.fg_gan_workspace_bytes(dnG.h, dnD.h, case.table, case.max_batch)
            self.ws, self._skip = arena.take((nbytes + 3) // 4, name="step workspace"), 0
            self.ws.fill_(float("nan"))
            h = ctypes.c_void_p()
            ctx.check(ctx.lib.fg_gan_create(ctx.h, dnG.h, dnD.h, case.table, case.max_batch, self.ws.data_ptr(), nbytes, ctypes.byref(h)))
            self.h, self._bound, self.n_masks = h, None, dnD.n_masks
    return configure(ArenaGan(), case)


def arena_sizes(ctx, case):
    """float counts of everything device_gan(ctx, case, arena) and the test's operands take from the arena"""
    dnG = NC.device_net(ctx, case.glayers, case.gdims, case.max_batch)
    dnD = NC.device_net(ctx, case.dlayers, case.ddims, case.max_batch)
    nstep = (ctx.lib.fg_gan_workspace_bytes(dnG.h, dnD.h, case.table, case.max_batch) + 3) // 4
    return [dnG.n_params] * 2 + [max(dnG.n_buffers, 1), dnG.ws.numel()] + [dnD.n_params] * 2 + [max(dnD.n_buffers, 1), dnD.ws.numel(), nstep]


# ---------------------------------------------------------------------------------------------------------------------------------
# a case's inputs, iteration by iteration
# ---------------------------------------------------------------------------------------------------------------------------------
def noise_shape(case, rows):
    return (rows, 1) + case.ddims[1:] if case.table else (rows, case.gdims[0])


def inputs(case, it):
    """float32, oracle-shaped (NCHW): real, cond_real, cond_fake (B/2 rows), cond (B rows), the noise of the D-step (B/2 rows) and of
    the G-step (B rows), 0/1 masks of D for each of the two closures (B rows each).  cond_real != cond_fake."""
    B = case.iters[it]
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), case.seed, it])
    u = lambda shape, lo=0.0, hi=1.0: rng.uniform(lo, hi, shape).astype(np.float32)
    h = B // 2
    res = dict(B=B, real=u((h,) + case.ddims, -0.5 if case.table else 0.0, 0.5 if case.table else 1.0), noiseD=u(noise_shape(case, h), -1, 1), noiseG=u(noise_shape(case, B), -1, 1))
    if case.table:
        res.update(cond_real=u((h,) + case.ddims), cond_fake=u((h,) + case.ddims), cond=u((B,) + case.ddims))
    res["masksD"] = NC.draw_masks(case.dlayers, case.ddims, B, rng)
    res["masksG"] = NC.draw_masks(case.dlayers, case.ddims, B, rng)
    return res


def oracle_step(st, case, which, inp, masks, noise=None):
    """one closure of the oracle on the case's inputs -> its result dict (f_bce, out, grad, conf / samples); the oracle applies its own
    update.  `noise`: what the device drew, where the library drew it."""
    from oracle import torch7_nn as O
    dt = st.pD.dtype
    a = lambda k: inp[k].astype(dt)
    if which == "D":
        nz = (inp["noiseD"] if noise is None else noise).astype(dt)
        if case.table:
            return O.step_D_c2f(st, a("real"), a("cond_real"), nz, a("cond_fake"), masks)
        return O.step_D(st, a("real"), nz, masks)
    nz = (inp["noiseG"] if noise is None else noise).astype(dt)
    if case.table:
        return O.step_G_c2f(st, nz, a("cond"), masks)
    return O.step_G(st, nz, masks)
