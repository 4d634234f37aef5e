"""CPU-only: the net planner (fg_net_create, forward_run and the backward walk of csrc/net.hip) on layer lists off the models'
shapes, from planning-only child processes with FG_LAUNCH_LOG=1 (tests/dispatch_audit.py net_sweep / net_replay).
(a) a net that fg_net_create accepts runs every pass, (b) every launch signature the sweep reaches is run by a case that is
compared with a reference, (c) each case of tests/net_cases.py launches the kernels it names, (d) the ledger rows of the kernels
that only nets reached, (e) the float32 oracle against the float64 oracle of every case.  tests/NET_FUSIONS.md is the document."""
import os
import re
import time

import numpy as np
import pytest

import dispatch_audit as A
import net_cases as NC
from test_dispatch_coverage_host import norm

DOC = os.path.join(A.ROOT, "tests", "NET_FUSIONS.md")
# the kernels the ledger had as `net-only`, by what became of them
NOW_OPERATOR = ["actmaxpool_fwd_kernel", "colsum_final_thin_kernel", "colsum_perm_kernel", "gemv_bwd_act_kernel", "igemm_act_kernel",
                "maxpool_prelu_bwd_kernel", "sum_splits_actbwd_kernel", "thin_in_mfma_pad_kernel", "thin_out_rows_gather_kernel",
                "thin_out_rows_mfma_kernel"]
STEP_LEVEL = ["bce_kernel", "rng_multi_kernel", "add_halves_kernel", "copy_kernel"]     # fg_step_* / fg_gan_*: out of a net's reach (tests/gan_cases.py)
TOO_LARGE = ["igemm_ws_act_kernel"]     # smallest net that reaches it: 8.4 M output activations (NET_FUSIONS.md, "Known limits")


@pytest.fixture(scope="module")
def audit():
    from face_generator_amd import build
    build.build(verbose=False)
    t0 = time.time()
    out = dict(sweep=A.net_sweep(), replay=A.net_replay())
    out["known"] = A.replay() + A.strided_replay() + A.pointwise_replay()
    out["seconds"] = time.time() - t0
    return out


def stated_refusal(layers, dims):
    """what include/facegen_hip.h rules out among the lists the grammar emits: Linear(-> 1) straight behind a spatial flatten.
    -> index of the refused layer, or None"""
    first, outs = NC.walk(layers, dims)
    for i, l in enumerate(layers):
        if l[0] == "LINEAR" and l[2] == 1 and (outs[i - 1] if i else first).perm is not None:
            return i
    return None


def test_the_sweep_is_the_one_the_document_describes(audit):
    lists = NC.random_layer_lists(NC.SWEEP_SEED, NC.SWEEP_N)
    assert len(lists) >= 2000 and lists == NC.random_layer_lists(NC.SWEEP_SEED, NC.SWEEP_N)
    types = {l[0] for d, L, B in lists for l in L}
    assert types == {"LINEAR", "VIEW", "PRELU", "UPSAMPLE2X", "CONV", "BATCHNORM", "SPATIAL_DROPOUT", "AVGPOOL2", "DROPOUT", "SIGMOID",
                     "LEAKYRELU", "MAXPOOL2", "CONCAT_TABLE", "BRANCH", "JOIN_TABLE"}
    convs = [NC.pad(l) for d, L, B in lists for l in L if l[0] == "CONV"]
    assert {c[3] for c in convs} == {3, 5, 7} and {c[5] for c in convs} == {0, 2} and {c[6] for c in convs} == {0, 2}
    assert {c[1] for c in convs} >= set(NC.CHANNELS) and {d[0] for d, L, B in lists if d[1] * d[2] > 1} == set(NC.IN_C)
    assert {d[1] for d, L, B in lists} >= set(range(2, 17)) and {B for d, L, B in lists} == {1, 2, 3, 4, 5, 8}
    tables = [L for d, L, B in lists if L[0][0] == "CONCAT_TABLE"]
    assert 0.07 * len(lists) < len(tables) < 0.14 * len(lists) and {L[0][1] for L in tables} == {2, 3, 4}
    assert any(l[0] == "VIEW" and NC.pad(l)[2] > 0 for d, L, B in lists for l in L)           # Linear + View(C, H, W) heads
    assert any(l[0] == "LINEAR" and l[2] == 1 for d, L, B in lists for l in L) and any(l[0] == "LINEAR" and l[2] % 4 for d, L, B in lists for l in L)
    jobs = audit["sweep"]
    assert len(jobs) == 6 * len(lists) and {(j["fusion"], j["math"]) for j in jobs} == {(f, m) for f in NC.FUSIONS for m in NC.MATHS}
    text = open(DOC).read()
    assert "seed %d" % NC.SWEEP_SEED in text and "%d layer lists" % len(lists) in text
    print("net sweep + replays: %.1f s" % audit["seconds"])
    assert audit["seconds"] < 120


def test_a_net_that_is_accepted_runs_every_pass(audit):
    """(a) forward (train), forward (evaluate), backward with flags 3, 1 and 2, and fg_net_backward_range split at every stage
    boundary all return FG_OK in a workspace of exactly fg_net_workspace_bytes; every refusal comes from fg_net_create with
    FG_ERR_UNSUPPORTED or FG_ERR_INVALID and names the layer, nothing is launched for it, and exactly the lists the header rules out
    are refused.  (Before this module: Linear + View(C, H, W) -> PReLU -> SpatialDropout -> AvgPool was created and then refused by
    its forward pass, "actpool: bad split partials", where the Linear split K.)"""
    bad, counts = [], {}
    for j in audit["sweep"] + audit["replay"]:
        rc = j["rc"]
        want = stated_refusal([tuple(l) for l in j["layers"]], j["dims"])
        if rc["create"][0]:
            ok = rc["create"][0] in (-1, -4) and want is not None and ("layer %d:" % want) in rc["create"][1] and set(rc) == {"create"} and not any(j["sigs"].values())
            counts[rc["create"][1].split(": ", 2)[-1]] = counts.get(rc["create"][1].split(": ", 2)[-1], 0) + 1
        else:
            ok = want is None and all(rc.get(p) == (0, "") for p in A.NET_PASSES)
        if not ok:
            bad.append((j["dims"], j["layers"], j["batch"], j["math"], j["fusion"], rc))
    print("refused: %s" % counts)
    assert not bad, "%d jobs; first: %s" % (len(bad), bad[:3])
    assert set(counts) == {"Linear(->1) after a spatial flatten"}


def test_every_signature_the_sweep_reaches_is_run_by_a_compared_case(audit):
    """(b) with the ledger's definition of a signature and its two shape-sized exceptions"""
    cases = {norm(s) for j in audit["replay"] if j["list"] == "NET_CASES" for v in j["sigs"].values() for s in v}
    covered = cases | {norm(s) for s in A.all_sigs(audit["known"])}
    reach = {norm(s) for s in A.all_sigs(audit["sweep"])}
    print("%d signatures reached by the sweep, %d of them launched by NET_CASES, %d only by the operator-level lists" % (len(reach), len(reach & cases), len(reach - cases)))
    missing = sorted(reach - covered, key=str)
    assert not missing, "reached by a generated net but never compared with a reference:\n" + "\n".join(map(str, missing))
    text = open(DOC).read()
    assert "%d signatures" % len(reach) in text


def test_every_case_launches_the_kernels_it_names(audit):
    """(c) and the un-fused twin launches the un-fused kernels; the refused lists are refused by fg_net_create, naming the layer"""
    jobs = {j["case"]: j for j in audit["replay"]}
    assert [j["case"] for j in audit["replay"] if j["list"] == "NET_CASES"] == [c.name for c in NC.NET_CASES] and len(jobs) == len(audit["replay"])
    for c in NC.NET_CASES:
        j = jobs[c.name]
        for p, ks in c.expect.items():
            have = {g[0] for g in j["grids"][p]}
            assert set(ks) <= have, "%s %s: expected %s, launched %s" % (c.name, p, sorted(set(ks) - have), sorted(have))
        for p, ks in c.absent.items():
            have = {g[0] for g in j["grids"][p]}
            assert not set(ks) & have, "%s %s: launched %s" % (c.name, p, sorted(set(ks) & have))
    for name, row, dims, layers, msg in NC.REFUSED_CASES:
        rc = jobs[name]["rc"]
        assert set(rc) == {"create"} and rc["create"][0] in (-1, -4) and msg in rc["create"][1] and "layer %d:" % stated_refusal(layers, dims) in rc["create"][1], (name, rc)
    # the table: every row has cases, every case is in the document under its row
    text = open(DOC).read()
    for row in range(1, 13):
        assert len([c for c in NC.NET_CASES if c.row == row]) + len([r for r in NC.REFUSED_CASES if r[1] == row]) >= 2, row
    for name in [c.name for c in NC.NET_CASES] + [r[0] for r in NC.REFUSED_CASES]:
        assert "`%s`" % name in text, "%s is not in tests/NET_FUSIONS.md" % name


def test_the_ledger_rows_of_the_kernels_only_nets_reached(audit):
    """(d) each of them is launched by a NET_CASES entry the ledger names; the step-level ones are out of a net's reach: no NET_CASES
    entry launches them, their rows are `operator` through GAN_CASES (tests/test_gan_steps_host.py holds those rows)"""
    rows = A.ledger_rows()
    by_kernel = {}
    for j in audit["replay"]:
        for v in j["grids"].values():
            for g in v:
                by_kernel.setdefault(g[0], set()).add(j["case"])
    for k in NOW_OPERATOR:
        st, note = rows[k]
        named = set(re.findall(r"`((?:r\d+|s)-[\w-]+)`", note))
        assert st == "operator" and named and named <= by_kernel.get(k, set()), "%s: %s %s; launched by %s" % (k, st, sorted(named), sorted(by_kernel.get(k, ()))[:4])
    for k in STEP_LEVEL:
        assert rows[k][0] == "operator" and "`GAN_CASES`" in rows[k][1] and k not in by_kernel, k
    for k in TOO_LARGE:
        assert rows[k][0] == "net-only" and k not in by_kernel, k
    # the 4096-block cap of actmaxpool_fwd_kernel: one quad per thread, so more than 4096 x 256 quads of the POOLED tensor, that is
    # an input of more than 16 777 216 floats (64 MiB) -- above the 64 MB the GPU module allows a case: the row stays "none"
    assert A.capped_rows()["actmaxpool_fwd_kernel", "x"][0] == "4096" and A.capped_rows()["actmaxpool_fwd_kernel", "x"][2].startswith("none")


def test_the_float32_oracle_stays_inside_the_flip_cap_on_every_case():
    """(e) the reference alone: on the cases' inputs no PReLU unit of the float32 oracle decides otherwise than the float64 oracle
    beyond max(1, 1e-5 of the units); its errors against the float64 oracle are what the fallback bar of NET_FUSIONS.md is made of"""
    t0 = time.time()
    for c in NC.NET_CASES:
        e = NC.reference_errors(c)
        assert e["flips"] <= max(1, 1e-5 * e["units"]), "%s: %d of %d units: re-seed the case" % (c.name, e["flips"], e["units"])
        assert e["outputs"] <= 1e-5 and np.isfinite(list(e["tensors"].values())).all(), (c.name, e["outputs"])
        first, outs = NC.walk(c.layers, c.dims)
        assert sum(int(np.prod(o.shape)) for o in outs) * c.batch <= 1 << 22, "%s: more than 4 M activations" % c.name
    assert time.time() - t0 < 30
