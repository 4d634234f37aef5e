"""Small nets for the sync-BN walk of fg_net (csrc/net.hip: FG_PAUSED_SYNC in forward_run and backward_run_stages, the four
*_sync_* kernels of csrc/pointwise.hip): SYNC_CASES, each a layer list of tests/net_cases.py with the batch cut into per-replica
shards.  Module-level data and helpers, no GPU use at import: tests/dispatch_audit.py walks the cases in the planning-only context
(sync_replay), tests/test_sync_cases_host.py asserts on what it returns, tests/test_gpu_sync_cases.py runs R DeviceNets in
lock-step in one process -- the "all-reduce" is a float64 sum on the device -- and compares with the float64 oracle on the global
batch.  tests/SYNC_BN.md is the table of cases with the branch each one exists for.

A case is: name, group, dims, layers, shards (per-replica batches; the global batch is their sum), fusion word, math."""
import collections

import numpy as np

import net_cases as NC
from net_cases import walk, operands, device_net, to_device, from_device, device_masks, adopt, flips     # noqa: F401  (the shared helpers)

FG_OK, FG_PAUSED_SYNC, FG_ERR_INVALID, FG_ERR_WORKSPACE = 0, 1, -1, -5

# (name, seed, gain: what NC.operands reads beside the lists; batch = sum(shards))
SyncCase = collections.namedtuple("SyncCase", "name group dims layers shards batch math fusion seed gain")

SYNC_CASES = []
PR, BN, AVG = NC.PR, NC.BN, NC.AVG
_conv, _sd, _do = NC._conv, NC._sd, NC._do


def _case(name, group, dims, layers, shards, math=0, fusion=503, seed=0, gain=1.0):
    shards = tuple(int(s) for s in shards)
    SYNC_CASES.append(SyncCase(name, group, tuple(dims), [tuple(l) for l in layers], shards, sum(shards), math, fusion, seed, gain))


# ---- row 6: every BN-bearing row-6 list of NET_CASES, batch and fusion word as there, two halves ------------------------------------
ROW6 = ["r6-bn-behind-winograd", "r6-bn-behind-igemm", "r6-bn-behind-igemm-splitk", "r6-bn-behind-igemm-math6-splitk", "r6-bn-behind-bf16x6",
        "r6-bn-behind-splitk-linear", "r6-bn-behind-thinin", "r6-bn-behind-stride2", "r6-bn-behind-avgpool", "r6-bn-first"]
_NET = {c.name: c for c in NC.NET_CASES}
for _n in ROW6:
    _c = _NET[_n]
    _case("sync-" + _n, "row6", _c.dims, _c.layers, (_c.batch // 2, _c.batch - _c.batch // 2), _c.math, _c.fusion, _c.seed, _c.gain)
# ---- channel edges: 12, 68 and 260 fail cr4_ok (scalar partial kernels); 68: a second 64-channel block with 4 live lanes; 260: a
# second block of the 256-thread global kernels -------------------------------------------------------------------------------------
CHANNEL_EDGES = (4, 12, 68, 128, 260)
for _C in CHANNEL_EDGES:
    _case("sync-c%d" % _C, "channels", (_C, 2, 2), [BN(_C), PR, _conv(_C, 8)], (1, 1))
# ---- row edges at C = 4: 19 row blocks (the second turn of `b += 16`), the cap of cr_rowblocks, M = 4 -------------------------------
_R4 = [BN(4), PR, _conv(4, 8)]
_case("sync-rows-19-blocks", "rows", (4, 34, 34), _R4, (1, 1))
_case("sync-rows-at-cap", "rows", (4, 64, 64), _R4, (5, 5))
_case("sync-rows-4", "rows", (4, 2, 2), _R4, (1, 1))
# ---- shards at C = 8: unequal (sync[2C] carries the row count), three replicas, one replica ------------------------------------------
_S8 = [_conv(8, 8), BN(8), PR, _conv(8, 8)]
_case("sync-shards-1-3", "shards", (8, 4, 4), _S8, (1, 3))
_case("sync-shards-5-2-1", "shards", (8, 4, 4), _S8, (5, 2, 1))
_case("sync-shards-4", "shards", (8, 4, 4), _S8, (4,))
# ---- two widths in one net: sync_count 129 -> 17 forward, 17 -> 129 backward; the last stage is a BatchNorm without PReLU -----------
TWO_WIDTHS = [_conv(8, 64), BN(64), PR, _conv(64, 8), BN(8)]
_case("sync-two-widths", "widths", (8, 4, 4), TWO_WIDTHS, (1, 1))
# ---- masks across pauses: a dropout layer on either side of the BatchNorm, so that the forward reads a mask pointer behind its
# pause and the backward reads one behind its own -----------------------------------------------------------------------------------
_case("sync-masks-spatial-dropout", "masks", (8, 4, 4), [_conv(8, 8), PR, _sd(), AVG, _conv(8, 8), BN(8), PR, _sd(), _conv(8, 8)], (2, 1))
_case("sync-masks-dropout", "masks", (8, 4, 4), [_conv(8, 8), PR, _do(), _conv(8, 8), BN(8), PR, _do(), _conv(8, 8)], (2, 1))
# ---- fusion words and math modes: the two-width net and the Winograd row-6 list ---------------------------------------------------------
for _f in NC.FUSIONS:
    for _m in NC.MATHS:
        if (_f, _m) == (503, 0):
            continue                                  # (sync-two-widths and sync-r6-bn-behind-winograd themselves)
        _case("sync-two-widths-f%d-m%d" % (_f, _m), "settings", (8, 4, 4), TWO_WIDTHS, (1, 1), _m, _f)
        _case("sync-r6-bn-behind-winograd-f%d-m%d" % (_f, _m), "settings", (8, 4, 4), _NET["r6-bn-behind-winograd"].layers, (1, 1), _m, _f)


# ---- the two producers a half batch of row 6 no longer reaches: the un-split implicit GEMM (the one whose epilogue carries the
# statistics with sync off) needs 384 tiles and the bf16x6 kernel 256 blocks of 256 rows PER REPLICA -- the row-6 batch per shard ------
_case("sync-igemm-unsplit-b96-per-shard", "producers", _NET["r6-bn-behind-igemm"].dims, _NET["r6-bn-behind-igemm"].layers, (96, 96), 0, 23)
_case("sync-bf16x6-b64-per-shard", "producers", _NET["r6-bn-behind-bf16x6"].dims, _NET["r6-bn-behind-bf16x6"].layers, (64, 64), 6, 23)

# Cases in which, with sync OFF and at the shard's batch, a producing convolution carries the batch statistics in its epilogue (fewer
# statistics kernels than BatchNorms in the planning-only log; tests/test_sync_cases_host.py holds this list to that log).  With
# sync ON the epilogue must leave its slice of the workspace alone (`!n->sync_bn` in ST_CONV): tests/test_gpu_sync_cases.py looks.
EPILOGUE_CASES = ["sync-r6-bn-behind-winograd", "sync-r6-bn-behind-bf16x6", "sync-shards-1-3", "sync-shards-5-2-1", "sync-shards-4", "sync-two-widths",
                  "sync-masks-spatial-dropout", "sync-masks-dropout", "sync-two-widths-f503-m6", "sync-r6-bn-behind-winograd-f503-m6",
                  "sync-two-widths-f502-m0", "sync-r6-bn-behind-winograd-f502-m0", "sync-two-widths-f502-m6", "sync-r6-bn-behind-winograd-f502-m6",
                  "sync-igemm-unsplit-b96-per-shard"]

# ---------------------------------------------------------------------------------------------------------------------------------
# the step level: the BN-bearing GAN_CASES of tests/gan_cases.py on a dry communicator (fg_comm_create_dry), rank 0 of 2, where
# fg_gan_set_comm(..., sync_bn = 1, ...) sticks.  Every collective is recorded and skipped: BatchNorm sees the local batch, the
# gradient stays local and gan_optimize scales it by 1 / world.
# ---------------------------------------------------------------------------------------------------------------------------------
SYNC_STEP_CASES = ["r2-bn-prelu-last", "r3-bn-inner-3ch", "r3-bn-both-nets", "r6-bn-first-D", "r11-overlapped-3-buckets"]
STEP_WORLD = 2


def step_settings(name):
    """[(overlap, bucket)]: overlap 0 and 1 at the default bucket target; the r11 pair also with G's backward cut at every stage
    ("one": a target of one parameter) and at a third of G's parameters ("third")"""
    return [(0, None), (1, None)] + ([(1, "one"), (1, "third")] if name.startswith("r11-") else [])


def bucket_target(bucket, n_params_G):
    """what fg_test_set_gan_bucket_target gets; 0: the target is left as fg_gan_create set it"""
    return {None: 0, "one": 1, "third": max(2, n_params_G // 3)}[bucket]


def step_f64_counts(case):
    """the counts of the f64 all-reduces a run of the case issues, in order: per iteration a D-step (G forward on B / 2 rows, D
    forward, D backward) and a G-step (G forward, D forward, D backward for the input gradient, G backward)"""
    g = [2 * l[1] + 1 for l in case.glayers if l[0] == "BATCHNORM"]
    d = [2 * l[1] + 1 for l in case.dlayers if l[0] == "BATCHNORM"]
    one = g + d + d[::-1] + g + d + d[::-1] + g[::-1]
    return one * len(case.iters)


# ---------------------------------------------------------------------------------------------------------------------------------
# what the protocol must show, from the layer list alone
# ---------------------------------------------------------------------------------------------------------------------------------
def batchnorms(case):
    """[(layer index, C, rows per sample)] of the BatchNorm layers in list order"""
    first, outs = walk(case.layers, case.dims)
    return [(i, l[1], outs[i].chw[1] * outs[i].chw[2]) for i, l in enumerate(case.layers) if l[0] == "BATCHNORM"]


def sync_counts(case):
    """fg_net_sync_count at the pauses of a forward pass; a backward pass shows the reverse"""
    return [2 * c + 1 for _, c, _ in batchnorms(case)]


def capacity(case):
    """doubles of the exchange buffer: 2 C + 1 of the widest BatchNorm"""
    return max(sync_counts(case))


def bounds(case):
    """[(lo, hi)] rows of the global batch per replica, shard order"""
    e = np.cumsum((0,) + case.shards)
    return [(int(a), int(b)) for a, b in zip(e[:-1], e[1:])]


def shard_masks(case, masks, lo, hi):
    """the oracle-shaped masks of rows lo..hi -> device order (NC.device_masks)"""
    return device_masks(case.layers, case.dims, [m[lo:hi] for m in masks])


def adopt_shards(ctx, nets, case, mods, x, P):
    """NC.adopt per replica on its own rows, the PReLU and pool decisions concatenated in shard order.  A layer whose pre-activation
    one replica exposes is exposed by all (the stages are cut by fg_net_create, whatever the batch)."""
    from oracle import torch7_nn as O
    per = []
    for dn, (lo, hi) in zip(nets, bounds(case)):
        adopt(ctx, dn, case.layers, case.dims, mods, x[lo:hi], P)
        per.append([getattr(m, "pos_override", None) if isinstance(m, O.PReLU) else getattr(m, "indices_override", None) if isinstance(m, O.SpatialMaxPooling) else None
                    for m in mods])
    for i, m in enumerate(mods):
        got = [p[i] for p in per]
        if not isinstance(m, (O.PReLU, O.SpatialMaxPooling)):
            continue
        assert all(g is None for g in got) or all(g is not None for g in got), "%s: layer %d is exposed by some replicas only" % (case.name, i)
        v = None if got[0] is None else np.concatenate(got, 0)
        if isinstance(m, O.PReLU):
            m.pos_override = v
        else:
            m.indices_override = v


def clear_adopted(mods):
    from oracle import torch7_nn as O
    for m in mods:
        if isinstance(m, O.PReLU):
            m.pos_override = None
        elif isinstance(m, O.SpatialMaxPooling):
            m.indices_override = None
