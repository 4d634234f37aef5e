"""CPU-only: the step level (fg_gan_create, fg_step_D, fg_step_G, fg_gan_update and gan_optimize of csrc/step.hip) on small G / D pairs
off the models' shapes, from planning-only child processes with FG_LAUNCH_LOG=1 (tests/dispatch_audit.py gan_sweep / gan_replay).
(a) a pair that fg_gan_create accepts steps at every even batch, (b) each closure launches the kernels it should, (c) a refused step
leaves the random streams alone, (d) FG_GAN_D_OUTPUT reports the batch of the last closure, (e) the float32 oracle against the float64
oracle of every case, (f) the ledger rows of the four step kernels; the bucket ranges of the overlapped generator backward.
tests/GAN_STEPS.md is the document."""
import os
import re
import time

import numpy as np
import pytest

import dispatch_audit as A
import gan_cases as GC
import net_cases as NC

DOC = os.path.join(A.ROOT, "tests", "GAN_STEPS.md")
STEP_KERNELS = ["bce_kernel", "rng_multi_kernel", "add_halves_kernel", "copy_kernel"]


@pytest.fixture(scope="module")
def audit():
    from face_generator_amd import build
    build.build(verbose=False)
    t0 = time.time()
    out = dict(sweep=A.gan_sweep(), replay=A.gan_replay())
    out["seconds"] = time.time() - t0
    return out


def passes(batches):
    return ["%s@%d%s" % (c, B, e) for B in batches for e in "nx" for c in A.GAN_CLOSURES]


def test_the_sweep_is_the_one_the_document_describes(audit):
    pairs = GC.random_pairs(GC.SWEEP_SEED, GC.SWEEP_N)
    assert len(pairs) == 300 and pairs == GC.random_pairs(GC.SWEEP_SEED, GC.SWEEP_N)
    tables = [p for p in pairs if p[4]]
    concat = [p for p in pairs if p[3][0][0] == "CONCAT_TABLE"]
    assert 0.12 * len(pairs) < len(tables) < 0.28 * len(pairs) and 0.05 * len(pairs) < len(concat) < 0.16 * len(pairs)
    assert all(p[0][1:] == (1, 1) and p[1][0][0] == "LINEAR" and p[1][1][0] == "VIEW" for p in pairs if not p[4])
    assert all(p[0] == (p[2][0] + 1,) + p[2][1:] for p in tables)
    assert all(p[3][-1] == ("SIGMOID",) and p[3][-2][0] == "LINEAR" and p[3][-2][2] == 1 for p in pairs)
    types = {l[0] for p in pairs for l in p[1] + p[3]}
    assert types >= {"LINEAR", "VIEW", "PRELU", "UPSAMPLE2X", "CONV", "BATCHNORM", "SPATIAL_DROPOUT", "AVGPOOL2", "DROPOUT", "SIGMOID", "CONCAT_TABLE"}
    img = {(B // 2) * int(np.prod(p[2])) % 4 for p in pairs for B in GC.SWEEP_BATCHES(p[5])}
    assert img == {0, 1, 2, 3}
    assert max(sum(1 for l in p[3] if l[0] in ("DROPOUT", "SPATIAL_DROPOUT")) for p in pairs) >= 13
    text = open(DOC).read()
    assert "seed %d" % GC.SWEEP_SEED in text and "%d pairs" % len(pairs) in text
    print("gan sweep + replay: %.1f s" % audit["seconds"])
    assert audit["seconds"] < 120


def test_a_pair_that_is_accepted_steps_at_every_batch(audit):
    """(a) fg_step_D, fg_step_G, fg_step_D | FG_STEP_NO_UPDATE + fg_gan_update(0) and fg_step_G | FG_STEP_NO_UPDATE + fg_gan_update(1)
    return FG_OK at every even batch of {2, 4, 6, max_batch - 2, max_batch}, with noise and masks NULL and explicit, in workspaces of
    exactly fg_gan_workspace_bytes and fg_net_workspace_bytes; every refusal comes from fg_gan_create or fg_net_create, names its reason,
    launches nothing, and exactly the pairs the header rules out are refused.  (Before this module: fg_step_D was refused, "fg_net_forward_to:
    16-byte alignment", wherever (B/2) * C*H*W is no multiple of 4 -- 3x3x3 at B = 6, 1x5x5 at B = 2 --, and both closures were refused
    with library-drawn masks, "more than 12 random segments per step", for a D with 13 Dropout layers.)"""
    bad, counts, accepted = [], {}, 0
    for j in audit["sweep"] + [j for j in audit["replay"] if j["list"] == "GAN_CASES"]:
        rc = j["rc"]
        want = GC.stated_refusal([tuple(l) for l in j["glayers"]])
        if rc["create"][0]:
            ok = rc["create"][0] in (-1, -4) and want is not None and want in rc["create"][1] and set(rc) == {"create"} and not any(j["sigs"].values())
            counts[rc["create"][1]] = counts.get(rc["create"][1], 0) + 1
        else:
            accepted += 1
            ok = want is None and set(rc) == {"create"} | set(passes(j["batches"])) and all(v == (0, "") for v in rc.values())
        if not ok:
            bad.append((j.get("case", j.get("idx")), j["gdims"], j["glayers"], j["ddims"], j["dlayers"], j["table"], j["max_batch"], {p: v for p, v in rc.items() if v[0]}))
    print("accepted: %d; refused: %s" % (accepted, counts))
    assert not bad, "%d pairs; first: %s" % (len(bad), bad[:2])
    assert set(counts) == {"fg_gan_create: dropout inside G is not built"}
    text = open(DOC).read()
    n = len(audit["sweep"])
    assert "%d are accepted" % (n - sum(counts.values())) in text and "%d are refused" % sum(counts.values()) in text


def test_every_refused_pair_is_refused_at_create_time_with_its_reason(audit):
    jobs = {j["case"]: j for j in audit["replay"]}
    for (name, row, gd, gl, dd, dl, table, mb, msg) in GC.REFUSED_GAN_CASES:
        rc = jobs[name]["rc"]
        assert set(rc) == {"create"} and rc["create"][0] in (-1, -4) and msg in rc["create"][1], (name, rc)
        assert rc["create"][1].startswith(("fg_gan_create: ", "fg_net_create: ")), (name, rc)
        assert not any(jobs[name]["sigs"].values()), name


def count(job, p, name):
    return sum(1 for s in job["sigs"][p] if name in s[0])


def test_every_closure_launches_the_kernels_it_should(audit):
    """(b) bce_kernel once per closure; rng_multi_kernel if and only if something is drawn, one launch per 12 segments; copy_kernel for
    the real half in plain mode, for the fakes where the second half is off 16 bytes and for the global confusion counts of a gated
    D-step, never in a G-step; add_halves_kernel in table mode only; no optimizer kernel in a FG_STEP_NO_UPDATE step and exactly one,
    and nothing else, in fg_gan_update"""
    jobs = {j["case"]: j for j in audit["replay"]}
    assert [j["case"] for j in audit["replay"] if j["list"] == "GAN_CASES"] == [c.name for c in GC.GAN_CASES]
    seen = dict(copies=set(), rng=set())
    for c in GC.GAN_CASES:
        j = jobs[c.name]
        nm = sum(1 for l in c.dlayers if l[0] in ("DROPOUT", "SPATIAL_DROPOUT"))
        img = int(np.prod(c.ddims))
        for B in j["batches"]:
            for e in "nx":
                for cl in A.GAN_CLOSURES:
                    p, what = "%s@%d%s" % (cl, B, e), "%s %s@%d%s" % (c.name, cl, B, e)
                    opt = sum(count(j, p, k) for k in GC.OPT_KERNELS)
                    if cl in ("uD", "uG"):
                        assert opt == 1 and len(j["sigs"][p]) == 1, "%s: %s" % (what, j["sigs"][p])
                        method = (c.optD if cl == "uD" else c.optG)[0]
                        assert count(j, p, method + "_kernel") + (count(j, p, "pack_jobs_kernel<true>") if method == "adam" else 0) == 1, what
                        continue
                    assert count(j, p, "bce_kernel") == 1, what
                    assert opt == (0 if cl in ("Dn", "Gn") else 1), "%s: %d optimizer launches" % (what, opt)
                    rng = 0 if e == "x" else -(-(1 + nm) // 12)
                    assert count(j, p, "rng_multi_kernel") == rng, "%s: %d Philox launches, %d segments" % (what, count(j, p, "rng_multi_kernel"), 1 + nm)
                    seen["rng"].add(rng)
                    isD = cl in ("D", "Dn")
                    copies = ((0 if c.table else 1) + (1 if (B // 2) * img % 4 else 0) + (1 if cl == "Dn" else 0)) if isD else 0
                    assert count(j, p, "copy_kernel") == copies, "%s: %d copy_kernel launches, expected %d" % (what, count(j, p, "copy_kernel"), copies)
                    seen["copies"].add((cl, copies))
                    assert count(j, p, "add_halves_kernel") == (1 if c.table and isD else 0), what
                    assert count(j, p, "concat_kernel") == (1 if c.table else 0), what
        e = "x" if c.masks == "explicit" else "n"
        for cl, ks in c.expect.items():
            have = {g[0] for g in j["grids"]["%s@%d%s" % (cl, c.iters[0], e)]}
            assert set(ks) <= have, "%s %s: expected %s, launched %s" % (c.name, cl, sorted(set(ks) - have), sorted(have))
        for cl, ks in c.absent.items():
            have = {g[0] for g in j["grids"]["%s@%d%s" % (cl, c.iters[0], e)]}
            assert not set(ks) & have, "%s %s: launched %s" % (c.name, cl, sorted(set(ks) & have))
    assert seen["rng"] == {0, 1, 2} and seen["copies"] >= {("D", 0), ("D", 1), ("D", 2), ("Dn", 3), ("G", 0)}
    # the table: every row has cases on both sides, every case is in the document
    text = open(DOC).read()
    for row in range(1, 12):
        assert len([c for c in GC.GAN_CASES if c.row == row]) + len([r for r in GC.REFUSED_GAN_CASES if r[1] == row]) >= (1 if row in (7, 8) else 2), row
    for name in [c.name for c in GC.GAN_CASES] + [r[0] for r in GC.REFUSED_GAN_CASES]:
        assert "`%s`" % name in text, "%s is not in tests/GAN_STEPS.md" % name


def test_every_case_uses_another_optimizer_for_D_than_for_G():
    for c in GC.GAN_CASES:
        assert c.optD != c.optG, c.name
    rules = {(c.optD[0], c.optG[0]) for c in GC.GAN_CASES}
    assert {r[0] for r in rules} == {r[1] for r in rules} == {"adam", "sgd", "adagrad"}


def test_a_refused_step_leaves_the_random_streams_alone(audit):
    """(c) nine refusals -- odd batches, batches above max_batch, a null `real`, each net's workspace bound too small (refused by
    fg_net_forward behind the draw, the second also behind G's forward) -- between two steps: the offsets of the noise and mask streams
    (fg_gan_get_offsets) behind every later step equal those of a fresh twin that was never refused.  The launch log carries no
    arguments; the bits are compared on the device (tests/test_gpu_gan_steps.py)."""
    moved = 0
    for j in audit["replay"]:
        if j["list"] != "GAN_CASES":
            continue
        o = j["extra"]["offsets"]
        assert o["used"] == o["twin"], "%s: offsets %s, a twin that was never refused %s" % (j["case"], o["used"], o["twin"])
        assert o["used"][0] == [0, 0] and o["used"][1] == o["used"][2] and o["used"][1][0] > 0, (j["case"], o["used"])
        moved += o["used"][1][1] > 0
        for name, rc in o["codes"].items():
            assert rc == (-5 if name.startswith("FG_ERR_WORKSPACE:") else -1), (j["case"], name, rc)
        assert len(o["codes"]) == 9
    assert moved >= 5


def test_d_output_reports_the_batch_of_the_last_closure(audit):
    """(d) a D-step at max_batch then a G-step at max_batch - 2 gives max_batch - 2; the other order gives max_batch (it used to be
    the larger of the two)"""
    n = 0
    for j in audit["replay"]:
        d = (j.get("extra") or {}).get("d_output")
        if d:
            assert d["after_D_then_G"] == d["M"] - 2 and d["after_G_then_D"] == d["M"], (j["case"], d)
            n += 1
    assert n >= 30


def test_the_bucketed_generator_backward_tiles_the_stages(audit):
    """item 4 of the issue: on transport-less communicators of 2 and 4 ranks, overlap = 1, with bucket targets of 1, a third of the
    vector and the whole vector (fg_test_set_gan_bucket_target): the side-stream all-reduces of one G-step sum to fg_net_num_params(G),
    each is the parameter range of a run of consecutive stages, the runs tile the stages from last to first, one wait follows them, and
    the closure's one optimizer launch is its last launch"""
    n, multi = 0, 0
    for j in audit["replay"]:
        b = (j.get("extra") or {}).get("buckets")
        if not b:
            continue
        n += 1
        stages = [tuple(s) for s in b["stages"]]
        assert len(stages) >= 3
        for r in b["runs"]:
            what = "%s world %d target %d: %s" % (j["case"], r["world"], r["target"], r["schedule"])
            ops = [l.split() for l in r["schedule"]]
            red = [int(o[3]) for o in ops if o[1] == "allreduce"]
            assert all(o[1:3] == ["allreduce", "f32"] and o[4] == "side" for o in ops[:-1]) and ops[-1][1] == "wait" and int(ops[-1][3]) == len(red), what
            assert sum(red) == b["nP"], what
            s = len(stages) - 1
            for cnt in red:                       # each count: the parameters of stages s, s - 1, ... down to where the run ends
                lo, hi, acc = None, None, 0
                while acc < cnt and s >= 0:
                    a, e = stages[s]
                    acc += e - a
                    if e > a:
                        lo, hi = (a if lo is None else min(lo, a)), (e if hi is None else max(hi, e))
                    s -= 1
                assert acc == cnt and hi - lo == cnt, what       # consecutive stages, one contiguous range
                if r["target"] < b["nP"]:
                    assert cnt >= r["target"] or s < 0 or all(e == a for a, e in stages[:s + 1]), what
            assert all(e == a for a, e in stages[:s + 1]), what  # nothing with parameters is left over
            multi += len(red) > 1
            if r["target"] == 1:
                assert len(red) == sum(1 for a, e in stages if e > a) or stages[0][1] == stages[0][0], what
            names = [A.kernel_of(A.LAUNCH_RE.match(l).group(1)) for l in r["log"]]
            opt = [i for i, k in enumerate(names) if k in ("adam_kernel", "sgd_kernel", "adagrad_kernel") or "pack_jobs_kernel<true>" in r["log"][i]]
            assert opt == [len(names) - 1], what
    assert n >= 5 and multi >= 10


def inner(net):
    return getattr(net, "inner", net)


def test_the_penalty_of_the_update_check_is_the_oracles():
    """GC.penalised -- what tests/test_gpu_gan_steps.py puts in front of the interruptable_* rule -- equals the gradient feval_D /
    feval_G_on_D / step_G_c2f of the oracle hand to the optimizer, bit for bit in float64, on every case; G's sign term follows G_L2"""
    from oracle import torch7_nn as O
    for c in GC.GAN_CASES:
        st = GC.oracle_gan(c)
        real = st.opt
        raw = dict(real, D_L1=0.0, D_L2=0.0, G_L1=0.0, G_L2=0.0, D_clamp=0.0, G_clamp=0.0)
        inp = GC.inputs(c, 0)
        for which in "DG":
            p0, bn, grads = (st.pD if which == "D" else st.pG).copy(), save_bn(st), []
            for opt in (raw, real):
                st.opt = opt
                grads.append(GC.oracle_step(st, c, which, inp, inp["masks" + which])["grad"])
                (st.pD if which == "D" else st.pG)[...] = p0
                restore_bn(st, bn)
            assert np.array_equal(GC.penalised(real, which, p0, grads[0]), grads[1]), "%s %s" % (c.name, which)
            assert (c.pen[which + "_L2"] == 0 and (which == "G" or c.pen["D_L1"] == 0)) or not np.array_equal(grads[0], grads[1]), c.name
    p, g = np.array([-2.0, 0.0, 3.0]), np.zeros(3)
    assert np.array_equal(GC.penalised(dict(G_L1=7.0, G_L2=0.5, G_clamp=0.0), "G", p, g), 0.5 * np.sign(p) + 0.5 * p)
    assert np.array_equal(GC.penalised(dict(G_L1=7.0, G_L2=0.0, G_clamp=0.0), "G", p, g), g)
    assert np.array_equal(GC.penalised(dict(D_L1=0.25, D_L2=0.5, D_clamp=1.0), "D", p, g), np.clip(0.25 * np.sign(p) + 0.5 * p, -1, 1))


def bns(st):
    from oracle import torch7_nn as O
    return [m for net in (st.G, st.D) for m in O.walk_modules(inner(net)) if isinstance(m, O.SpatialBatchNormalization)]


def save_bn(st):
    return [(m.running_mean.copy(), m.running_var.copy()) for m in bns(st)]


def restore_bn(st, saved):
    for m, (rm, rv) in zip(bns(st), saved):
        m.running_mean[...] = rm; m.running_var[...] = rv


def adopt_from(src, dst):
    """the PReLU decisions of the oracle `src` after its forward -> pos_override of the same modules of `dst`"""
    from oracle import torch7_nn as O
    for s, d in zip(NC.sequentials(inner(src)), NC.sequentials(inner(dst))):
        for i, (a, b) in enumerate(zip(s.modules, d.modules)):
            if isinstance(a, O.PReLU):
                b.pos_override = None if src is None else s._inputs[i] > 0


def check_reference(c, shares):
    s32, s64 = GC.oracle_gan(c, np.float32), GC.oracle_gan(c, np.float64)
    s64.opt = dict(s64.opt, D_clamp=0.0, G_clamp=0.0)
    assert np.array_equal(s32.pD.astype(np.float64), s64.pD) and s32.pD.size + s32.pG.size <= 8000, c.name
    assert max(c.iters) <= min(16, c.max_batch) and max(c.ddims[1:]) <= 8, c.name
    for it in range(len(c.iters)):
        inp = GC.inputs(c, it)
        for which in "DG":
            s64.pD[...] = s32.pD; s64.pG[...] = s32.pG
            restore_bn(s64, save_bn(s32))
            r32 = GC.oracle_step(s32, c, which, inp, inp["masks" + which])
            for a, b in ((s32.D, s64.D), (s32.G, s64.G)):
                adopt_from(a, b)
            r64 = GC.oracle_step(s64, c, which, inp, inp["masks" + which])
            what = "%s iteration %d %s-step" % (c.name, it, which)
            f = sum(NC.flips(inner(n))[0] for n in (s64.D,) + ((s64.G,) if which == "G" else ()))
            assert f == 0, "%s: %d PReLU decisions differ: re-seed the case" % (what, f)
            assert np.abs(r64["out"] - 0.5).min() > 1e-4, "%s: an output of D within 1e-4 of 0.5: re-seed the case" % what
            assert np.abs(r32["out"] - r64["out"]).max() <= 1e-5, what
            clamp = c.pen[which + "_clamp"]
            g = r64["grad"]
            if clamp and np.abs(g).max() > clamp:
                assert np.abs(np.abs(g) - clamp).min() > 1e-4 * np.abs(g).max(), "%s: a gradient entry at the clamp value: re-seed the case" % what
                shares.setdefault(c.name, []).append(float((np.abs(g) > clamp).mean()))


def test_the_float32_oracle_decides_like_the_float64_oracle_on_every_case():
    """(e) the reference alone, closure by closure over every iteration of every case, the float64 oracle on the float32 oracle's
    parameters and running statistics: no PReLU decision differs, no output of D lies within 1e-4 of 0.5 (the confusion counts are
    decided), and where a clamp binds no entry of the float64 gradient lies within 1e-4 max|g| of the clamp value; the clamp of
    `r10-clamp-binds` binds on at least a tenth of the entries of both gradients.  A condition on the inputs: the seeds are chosen so."""
    t0 = time.time()
    shares = {}
    for c in GC.GAN_CASES:
        check_reference(c, shares)
    print("clamps that bind: %s" % {k: ["%.2f" % s for s in v] for k, v in shares.items()})
    assert set(shares) == {"r10-clamp-binds"} and min(shares["r10-clamp-binds"]) >= 0.1 and len(shares["r10-clamp-binds"]) == 4
    assert time.time() - t0 < 30


def test_the_ledger_rows_of_the_step_kernels(audit):
    """(f) each of the four kernels that only fg_step_* / fg_gan_* launch is `operator` in tests/DISPATCH_COVERAGE.md and is launched
    by the GAN_CASES entries its row names"""
    rows = A.ledger_rows()
    by_kernel = {}
    for j in audit["replay"]:
        for v in j["grids"].values():
            for g in v:
                by_kernel.setdefault(g[0], set()).add(j["case"])
    for k in STEP_KERNELS:
        st, note = rows[k]
        named = set(re.findall(r"`(r\d+-[\w-]+)`", note))
        assert st == "operator" and named and named <= by_kernel.get(k, set()), "%s: %s %s" % (k, st, sorted(named))
