"""CPU-only: the sync-BN walk of fg_net (FG_PAUSED_SYNC in forward_run and backward_run_stages of csrc/net.hip) on SYNC_CASES of
tests/sync_cases.py, from a planning-only child process with FG_LAUNCH_LOG=1 (tests/dispatch_audit.py sync_replay).  (a) the pauses
of every pass and their fg_net_sync_count, (b) the capacity refusal and what follows it, (c) what a pass launches with sync on: the
separate statistics kernel behind every producer, the four sync kernels, no bn_stats_final_kernel, (d) the document and the ledger
name the cases.  tests/test_gpu_sync_cases.py holds the same cases to the float64 oracle; tests/SYNC_BN.md is the document."""
import os
import re

import numpy as np
import pytest

import dispatch_audit as A
import net_cases as NC
import sync_cases as SC

DOC = os.path.join(A.ROOT, "tests", "SYNC_BN.md")
SYNC_KERNELS = ["bn_sync_local_kernel", "bn_sync_global_kernel", "bn_bwd_sync_local_kernel", "bn_bwd_sync_global_kernel"]
STATS = {"bn_stats4_partial_kernel", "bn_stats_partial_kernel"}


@pytest.fixture(scope="module")
def jobs():
    from face_generator_amd import build
    build.build(verbose=False)
    res = A.sync_replay()
    assert [j["case"] for j in res] == [c.name for c in SC.SYNC_CASES]
    return {j["case"]: j for j in res}


def kernels(j, p):
    return [g[0] for g in j["grids"][p]]


def test_the_cases_are_the_ones_the_document_lists():
    names = [c.name for c in SC.SYNC_CASES]
    assert len(set(names)) == len(names)
    by = {}
    for c in SC.SYNC_CASES:
        by.setdefault(c.group, []).append(c)
        assert c.batch == sum(c.shards) and all(s >= 1 for s in c.shards)
        NC.walk(c.layers, c.dims)                 # valid Torch7
        assert SC.batchnorms(c), c.name
    # every BN-bearing row-6 list of NET_CASES, batch and fusion word as there, two halves
    row6 = [c for c in NC.NET_CASES if c.row == 6 and any(l[0] == "BATCHNORM" for l in c.layers)]
    assert [c.name for c in by["row6"]] == ["sync-" + c.name for c in row6] == ["sync-" + n for n in SC.ROW6]
    for s, c in zip(by["row6"], row6):
        assert (s.dims, s.layers, s.batch, s.math, s.fusion) == (c.dims, c.layers, c.batch, c.math, c.fusion)
        assert s.shards == (c.batch // 2, c.batch - c.batch // 2)
    assert [c.dims[0] for c in by["channels"]] == [4, 12, 68, 128, 260] and all(c.shards == (1, 1) and c.dims[1:] == (2, 2) for c in by["channels"])
    assert [(c.dims, c.shards) for c in by["rows"]] == [((4, 34, 34), (1, 1)), ((4, 64, 64), (5, 5)), ((4, 2, 2), (1, 1))]
    assert [c.shards for c in by["shards"]] == [(1, 3), (5, 2, 1), (4,)]
    assert [SC.sync_counts(c) for c in by["widths"]] == [[129, 17]] and by["widths"][0].layers[-1][0] == "BATCHNORM"
    assert {l[0] for c in by["masks"] for l in c.layers} >= {"SPATIAL_DROPOUT", "DROPOUT"}
    for c in by["masks"]:                          # a dropout layer on either side of the BatchNorm
        at = [i for i, l in enumerate(c.layers) if l[0] == "BATCHNORM"][0]
        kinds = [i for i, l in enumerate(c.layers) if l[0] in ("SPATIAL_DROPOUT", "DROPOUT")]
        assert min(kinds) < at < max(kinds), c.name
    assert {(c.fusion, c.math) for c in by["settings"]} == {(f, m) for f in NC.FUSIONS for m in NC.MATHS} - {(503, 0)}
    assert len(by["settings"]) == 10
    assert [(c.shards, c.math, c.fusion) for c in by["producers"]] == [((96, 96), 0, 23), ((64, 64), 6, 23)]
    for c in SC.SYNC_CASES:                        # (as tests/test_net_fusions_host.py (e): a case stays small)
        first, outs = NC.walk(c.layers, c.dims)
        assert sum(int(np.prod(o.shape)) for o in outs) * c.batch <= 1 << 22, "%s: more than 4 M activations" % c.name
    text = open(DOC).read()
    for n in names:
        assert "`%s`" % n in text, "%s is not in tests/SYNC_BN.md" % n


def test_every_pass_pauses_once_per_batchnorm_with_its_count(jobs):
    """(a) forward (train): 2 C + 1 of every BatchNorm in list order; backward with flags 3, 1 and 2: the reverse; a ranged backward
    split at any stage boundary: the same pauses, spread over its two calls; evaluate: none.  Every shard of a case pauses alike."""
    for c in SC.SYNC_CASES:
        j, want = jobs[c.name], SC.sync_counts(c)
        assert all(j["rc"].get(p) == (0, "") for p in A.SYNC_PASSES), (c.name, j["rc"])
        R = len(c.shards)
        assert j["pauses"]["fwd"] == [want] * R and j["pauses"]["fwd2"] == [want] * R, (c.name, j["pauses"]["fwd"])
        assert j["pauses"]["eval"] == [[]] * R, c.name
        for p in ("bwd3", "bwd1", "bwd2"):
            assert j["pauses"][p] == [want[::-1]] * R, (c.name, p, j["pauses"][p])
        assert j["pauses"]["range"] == [[want[::-1]] * (j["stages"] - 1)] * R, (c.name, j["pauses"]["range"])
        assert max(want) == SC.capacity(c)


def test_a_buffer_one_double_short_is_refused_at_the_widest_batchnorm(jobs):
    """(b) capacity 2 C for the widest BatchNorm: the pass pauses at the BatchNorms in front of it, returns FG_ERR_WORKSPACE there and
    is not paused -- its _resume is FG_ERR_INVALID, and so is a backward behind the refused forward; 2 C + 1 passes"""
    for c in SC.SYNC_CASES:
        j, want = jobs[c.name], SC.sync_counts(c)
        k = want.index(max(want))
        for rc, msg, counts, resume, backward, again in j["cap"]["fwd"]:
            assert rc == SC.FG_ERR_WORKSPACE and "sync-BN buffer too small" in msg and counts == want[:k], (c.name, rc, msg, counts)
            assert resume == SC.FG_ERR_INVALID and backward == SC.FG_ERR_INVALID and again == SC.FG_OK, (c.name, resume, backward, again)
        rev = want[::-1]
        k = rev.index(max(rev))
        for rc, msg, counts, resume in j["cap"]["bwd"]:
            assert rc == SC.FG_ERR_WORKSPACE and "sync-BN buffer too small" in msg and counts == rev[:k], (c.name, rc, msg, counts)
            assert resume == SC.FG_ERR_INVALID, (c.name, resume)
        assert len(j["cap"]["fwd"]) == len(j["cap"]["bwd"]) == len(c.shards)


def test_what_a_pass_launches_with_sync_on(jobs):
    """(c) under sync the producing convolution writes no epilogue statistics (`!n->sync_bn` in ST_CONV): the separate statistics
    kernel runs behind every producer, also where the NET_CASES entry of the same list must NOT launch it; the local / global sync
    kernels run once per BatchNorm and shard, and the un-synced final never"""
    absent_there = {"sync-" + c.name for c in NC.NET_CASES if STATS & set(c.absent.get("fwd", ()))}
    assert {"sync-r6-bn-behind-winograd", "sync-r6-bn-behind-igemm"} <= absent_there
    for c in SC.SYNC_CASES:
        j, nbn, R = jobs[c.name], len(SC.batchnorms(c)), len(c.shards)
        fwd, bwd = kernels(j, "fwd"), kernels(j, "bwd3")
        assert STATS & set(fwd), "%s: no statistics kernel: %s" % (c.name, sorted(set(fwd)))
        assert sum(fwd.count(k) for k in STATS) == nbn * R, (c.name, fwd)
        assert fwd.count("bn_sync_local_kernel") == fwd.count("bn_sync_global_kernel") == nbn * R, (c.name, fwd)
        for p in ("bwd3", "bwd1", "bwd2", "range"):
            ks = kernels(j, p)
            times = (j["stages"] - 1) if p == "range" else 1
            assert ks.count("bn_bwd_sync_local_kernel") == ks.count("bn_bwd_sync_global_kernel") == nbn * R * times, (c.name, p)
        assert "bn_stats_final_kernel" not in set(fwd) | set(kernels(j, "fwd2")), c.name
        assert not any("bn_bwd_final_kernel" in kernels(j, p) for p in ("bwd3", "bwd1", "bwd2", "range")), c.name
        assert not set(SYNC_KERNELS) & set(kernels(j, "eval")), c.name
    # where the producer's epilogue carries the statistics with sync off, at the shard's batch: the cases of SC.EPILOGUE_CASES
    plain = [c.name for c in SC.SYNC_CASES if jobs[c.name]["rc"]["plain"] == (0, "") and
             sum(kernels(jobs[c.name], "plain").count(k) for k in STATS) < len(SC.batchnorms(c)) * len(c.shards)]
    assert plain == SC.EPILOGUE_CASES
    # the two producers that the halves of row 6 do not reach
    assert "sum_splits_kernel" in kernels(jobs["sync-r6-bn-behind-igemm"], "fwd") and "igemm_ws6_kernel" not in kernels(jobs["sync-r6-bn-behind-bf16x6"], "fwd")
    assert "igemm_kernel" in kernels(jobs["sync-igemm-unsplit-b96-per-shard"], "fwd") and "sum_splits_kernel" not in kernels(jobs["sync-igemm-unsplit-b96-per-shard"], "fwd")
    assert "igemm_ws6_kernel" in kernels(jobs["sync-bf16x6-b64-per-shard"], "fwd") and "igemm_ws6_kernel" in kernels(jobs["sync-bf16x6-b64-per-shard"], "bwd3")
    # the branches the channel and row edges exist for, from the grids: the scalar partial kernels where cr4_ok fails, the second
    # column block of the local kernels at C = 68, of the global ones at C = 260, more than 16 row blocks, the cap of cr_rowblocks
    grid = lambda name, p, k: [g[1:] for g in jobs[name]["grids"][p] if g[0] == k]
    for C in SC.CHANNEL_EDGES:
        name = "sync-c%d" % C
        scalar = C in (12, 68, 260)
        assert ("bn_stats_partial_kernel" in kernels(jobs[name], "fwd")) == scalar and ("bn_bwd_partial_kernel" in kernels(jobs[name], "bwd3")) == scalar, name
        assert grid(name, "fwd", "bn_sync_local_kernel")[0][0] == -(-C // 64) == grid(name, "bwd3", "bn_bwd_sync_local_kernel")[0][0]
        assert grid(name, "fwd", "bn_sync_global_kernel")[0][0] == -(-C // 256) == grid(name, "bwd3", "bn_bwd_sync_global_kernel")[0][0]
    assert grid("sync-rows-19-blocks", "fwd", "bn_stats4_partial_kernel")[0][0] == 19 and grid("sync-rows-19-blocks", "bwd3", "bn_bwd4_partial_kernel")[0][0] == 19
    assert grid("sync-rows-at-cap", "fwd", "bn_stats4_partial_kernel")[0][0] == 256 and grid("sync-rows-4", "fwd", "bn_stats4_partial_kernel")[0][0] == 1


def test_the_collective_schedule_of_a_step_with_sync_bn():
    """the step level on a dry communicator, rank 0 of 2 (tests/test_gpu_gan_steps.py compares the text recorded on the device with
    this one): one f64 all-reduce of 2 C + 1 doubles per BatchNorm and pass on the compute stream, in the order gan_drain meets them;
    D's gradient blocking (overlap 0) or on the side stream with a wait behind it (overlap 1); G's gradient in one all-reduce or one
    per bucket that owns parameters, the sync-BN exchanges of the ranged backward between them"""
    import gan_cases as GC
    from face_generator_amd import build
    build.build(verbose=False)
    jobs = {(j["case"], j["overlap"], j["bucket"]): j for j in A.sync_gan_replay()}
    assert sorted(jobs, key=str) == sorted(((n, ov, bk) for n in SC.SYNC_STEP_CASES for ov, bk in SC.step_settings(n)), key=str)
    for (name, ov, bk), j in jobs.items():
        c = GC.BY_NAME[name]
        assert any(l[0] == "BATCHNORM" for l in c.glayers + c.dlayers) and j["rc"]["run"] == (0, ""), (name, j["rc"])
        ops = [l.split() for l in j["schedule"]]
        assert [int(o[0]) for o in ops] == list(range(len(ops)))
        f64 = [o for o in ops if o[2] == "f64"]
        assert [int(o[3]) for o in f64] == SC.step_f64_counts(c) and all(o[1] == "allreduce" and o[4] == "compute" for o in f64), (name, ov, bk, j["schedule"])
        f32 = [o for o in ops if o[2] == "f32"]
        nD, nG = GC.oracle_gan(c).pD.size, GC.oracle_gan(c).pG.size
        per = len(f32) // len(c.iters)
        for k in range(len(c.iters)):
            it = f32[k * per:(k + 1) * per]
            assert int(it[0][3]) == nD and it[0][4] == ("side" if ov else "compute"), (name, ov, it)
            assert sum(int(o[3]) for o in it[1:]) == nG and all(o[4] == ("side" if ov else "compute") for o in it[1:]), (name, ov, bk, it)
            # (a target of one parameter: every stage that owns parameters is a bucket; BatchNorm + PReLU is one stage)
            owners = sum(1 for i, l in enumerate(c.glayers) if l[0] in ("LINEAR", "CONV", "BATCHNORM") or (l[0] == "PRELU" and c.glayers[i - 1][0] != "BATCHNORM"))
            assert len(it) - 1 == (1 if bk is None else owners if bk == "one" else 2), (name, bk, it)
        assert len([o for o in ops if o[1] == "wait"]) == (2 * len(c.iters) if ov else 0)
        ks = [g[0] for g in j["grids"]["run"]]
        assert all(k in ks for k in SYNC_KERNELS), name
    # the bucketed backward pauses inside its ranges: the same f64 exchanges, in the same order, as the unsplit one
    a, b = jobs["r11-overlapped-3-buckets", 1, None], jobs["r11-overlapped-3-buckets", 1, "one"]
    f = lambda j: [l.split()[2:] for l in j["schedule"] if " f64 " in l]
    assert f(a) == f(b) and len(b["schedule"]) > len(a["schedule"])


def test_the_float32_oracle_stays_inside_the_flip_cap_on_every_case():
    """the reference alone, as (e) of tests/test_net_fusions_host.py: on the cases' inputs (the global batch) the float32 oracle decides
    no PReLU unit otherwise than the float64 oracle beyond max(1, 1e-5 of the units); its errors are what a fallback bar of
    SYNC_BN.md would be made of"""
    worst = 0.0
    for c in SC.SYNC_CASES:
        e = NC.reference_errors(c)
        assert e["flips"] <= max(1, 1e-5 * e["units"]), "%s: %d of %d units: re-seed the case" % (c.name, e["flips"], e["units"])
        assert e["outputs"] <= 1e-5 and np.isfinite(list(e["tensors"].values())).all(), (c.name, e["outputs"])
        worst = max(worst, e["outputs"])
    print("float32 oracle against float64 oracle over %d cases: worst output error %.3e" % (len(SC.SYNC_CASES), worst))


def test_the_ledger_names_the_sync_cases_for_the_four_sync_kernels():
    """(d) the four kernels stay `other-entry` (no replay of the coverage audit launches them: net_replay runs with sync off); their
    rows name the GPU module that runs SYNC_CASES"""
    rows = A.ledger_rows()
    for k in SYNC_KERNELS:
        st, note = rows[k]
        assert st == "other-entry" and "test_gpu_sync_cases.py" in note and "`SYNC_CASES`" in note, (k, st, note)
    assert re.search(r"\| `sync-two-widths` \|", open(DOC).read())
