"""CPU-only: every kernel plan that a caller of the conv / linear C entries can reach is compared with a reference by some
operator-level GPU parity case; the three conv passes accept the same geometries; every launch site in csrc/*.hip is entered in
tests/DISPATCH_COVERAGE.md.  All of it from planning-only child processes with FG_LAUNCH_LOG=1 (tests/dispatch_audit.py), like
tests/test_branched_host.py and tests/test_sampler_host.py."""
import os
import re
import time

import pytest

import dispatch_audit as A

LDS_MAX = 160 * 1024            # CDNA4: LDS of one workgroup
LDS_PLAIN = 64 * 1024           # dynamic LDS a launch may ask for without hipFuncAttributeMaxDynamicSharedMemorySize
# Kernels whose dynamic LDS is an arithmetic function of the geometry (rows x width of the map, the batch), not one of a few tile
# configurations: their signature is (launch site, block) alone -- DISPATCH_COVERAGE.md, "Known limits".
SHAPE_SIZED_LDS = {"thin_out_slab_mfma_kernel", "gemv_bwd_kernel"}
STATUSES = {"operator", "net-only", "measure-only", "unreachable", "other-entry"}
# `other-entry` is for kernels that no single planning-only process can launch: the sync-BN exchange needs the pause / all-reduce
# protocol of a second rank, the clock probe a device clock (fg_prof_clock_start launches nothing in a planning-only context)
OTHER_ENTRY = {"bn_sync_local_kernel", "bn_sync_global_kernel", "bn_bwd_sync_local_kernel", "bn_bwd_sync_global_kernel", "clock_probe_kernel"}


# capped launchers that STRIDED_CASES launch as part of a contraction plan, below their caps (their work count follows from the
# plan: split-K partials of a ragged layer, padded copies of thin operands)
CONTRACTION_SIDE = {"sum_splits_scalar_kernel", "thin_pad_kernel"}


def norm(sig):
    return (sig[0], sig[1], None) if A.kernel_of(sig[0]) in SHAPE_SIZED_LDS else sig


def matches(expect, sig):
    return expect[0] == sig[0] and expect[1] == sig[1] and (expect[2] is None or expect[2] == sig[2])


@pytest.fixture(scope="module")
def audit():
    from face_generator_amd import build
    build.build(verbose=False)
    t0 = time.time()
    out = dict(replay=A.replay(), sweep=A.sweep(), nets=A.net_launches(),
               strided_replay=A.strided_replay(), strided_sweep=A.strided_sweep(extra=STRIDED_REFUSED), pointwise=A.pointwise_replay(),
               net_replay=A.net_replay(), gan_replay=A.gan_replay())
    out["seconds"] = time.time() - t0
    return out


# stride-2 layers that include/facegen_hip.h rules out (odd H, odd W, k = 9), appended to the strided sweep: fg_net_create must refuse them
STRIDED_REFUSED = [(2, 5, 8, 8, 16, 3), (2, 8, 7, 6, 10, 5), (1, 8, 8, 8, 8, 9)]


def thin_layer(cs, cw, k):
    """csrc/fg_internal.h fg_thin_layer, restated from include/facegen_hip.h"""
    return (cw in (64, 128) or cw % 256 == 0) and ((k == 3 and cs in (1, 3, 4)) or (k in (5, 7) and cs in (1, 3)))


def test_the_sweep_is_the_one_the_ledger_describes(audit):
    conv, lin = A.sweep_geometries()
    assert len(conv) >= 1500 and len(lin) >= 300
    assert {c[5] for c in conv} == {3, 5, 7} and {c[6] for c in conv} == {0, 1}
    assert {c[3] for c in conv} == set(A.CHANNELS) == {c[4] for c in conv}
    assert max(c[0] for c in conv) == 128 and min(c[0] for c in conv) == 1
    pow2 = sum(1 for c in conv if c[1] & (c[1] - 1) == 0 and c[2] & (c[2] - 1) == 0)
    assert 0.4 * len(conv) < pow2 < 0.65 * len(conv)
    assert all(max(c[3], c[4]) * c[0] * c[1] * c[2] * (4 if c[6] else 1) <= A.CAP for c in conv)
    assert any(b >= 65536 and k <= 16 for b, k, n in lin) and any(b <= 4 and k >= 16384 for b, k, n in lin)
    assert {(j["math"], j["fusion"]) for j in audit["sweep"] if j["kind"] == "conv"} == \
        {(0, 503), (6, 503), (0, 503 & ~A.WINO_ALL), (6, 503 & ~A.WINO_ALL), (0, 503 & ~A.THIN_SLAB)}
    text = open(A.LEDGER).read()
    assert "seed %d" % A.SWEEP_SEED in text and "%d conv geometries" % len(conv) in text and "%d Linear shapes" % len(lin) in text
    print("replay + sweep + net logs: %.1f s" % audit["seconds"])
    assert audit["seconds"] < 120


def test_every_reachable_signature_is_covered_by_an_operator_level_case(audit):
    """(a) no exception list: whatever signature the sweep reaches through fg_conv2d_* / fg_linear_*, some parity list runs it"""
    covered = {norm(s) for s in A.all_sigs(audit["replay"])}
    best = A.smallest_per_signature(audit["sweep"])
    missing = sorted((s for s in A.all_sigs(audit["sweep"]) if norm(s) not in covered), key=str)
    assert not missing, "reachable but never compared with a reference:\n" + "\n".join("%s  smallest: %s" % (s, best.get(s)) for s in missing)


def test_the_strided_sweep_is_the_one_the_ledger_describes(audit):
    geo = A.strided_geometries()
    assert len(geo) == A.STRIDED_N == 200
    assert {g[5] for g in geo} == {3, 5, 7} and all(g[1] % 2 == 0 and g[2] % 2 == 0 and 2 <= g[1] <= 32 and 2 <= g[2] <= 32 for g in geo)
    assert {g[3] for g in geo} | {g[4] for g in geo} == set(A.CHANNELS) and min(g[0] for g in geo) == 1 and 32 < max(g[0] for g in geo) <= 64
    assert any(g[4] % 4 for g in geo) and any(g[3] % 4 for g in geo)
    jobs = audit["strided_sweep"]
    assert len(jobs) == 4 * (len(geo) + len(STRIDED_REFUSED))
    assert {(j["math"], j["fusion"]) for j in jobs} == {(0, 503), (6, 503), (0, 503 & ~A.WINO_ALL), (6, 503 & ~A.WINO_ALL)}
    text = open(A.LEDGER).read()
    assert "seed %d" % A.STRIDED_SEED in text and "%d strided geometries" % len(geo) in text


def test_every_signature_of_the_strided_sweep_is_run_by_a_strided_case(audit):
    """(a) for stride 2: whatever a one-layer net [FG_CONV p=2] launches in forward and backward at any swept geometry, some case of
    tests/test_gpu_strided_conv.py launches too, under the settings that module runs it with"""
    import test_gpu_strided_conv as TS
    rep = audit["strided_replay"]
    assert [tuple(j["shape"]) for j in rep if j["math"] == 0] == list(TS.STRIDED_CASES)
    assert [(tuple(j["shape"]), j["math"]) for j in rep if tuple(j["shape"]) != TS.CAP_CASE] == TS.RUNS
    assert all(j["rc"][p] == (0, "") for j in rep for p in A.STRIDED_PASSES), [(j["shape"], j["rc"]) for j in rep if any(v[0] for v in j["rc"].values())]
    covered = {norm(s) for s in A.all_sigs(rep)}
    best = A.smallest_per_signature(audit["strided_sweep"])
    missing = sorted((s for s in A.all_sigs(audit["strided_sweep"]) if norm(s) not in covered), key=str)
    assert not missing, "reachable at stride 2 but never compared with a reference:\n" + "\n".join("%s  smallest: %s" % (s, best.get(s)) for s in missing)
    # what the cases are there for: both zero-insert kernels, the capped one above its cap
    cap = [j for j in rep if tuple(j["shape"]) == TS.CAP_CASE][0]
    B, H, W, cin, cout, k = TS.CAP_CASE
    assert ("zero_insert2_kernel", 256, 0) in cap["sigs"]["bwd"] and B * H * W * cout // 4 > 4096 * 256
    assert any(("zero_insert2_scalar_kernel", 256, 0) in j["sigs"]["bwd"] for j in rep if j["shape"][4] % 4)


def test_a_strided_layer_is_refused_at_create_time_or_runs_every_pass(audit):
    """(b) for stride 2: a layer that fg_net_create accepts returns FG_OK from the forward pass and from the backward pass with
    FG_BWD_PARAM_GRADS | FG_BWD_INPUT_GRAD, in a workspace of exactly fg_net_workspace_bytes; a refused one is refused by
    fg_net_create with FG_ERR_UNSUPPORTED naming the layer, and exactly the layers the header rules out are refused (before the
    scalar zero insert, Cout % 4 != 0 was created, ran forward and failed in backward: "zero_insert2: C % 4")"""
    bad, refused = [], set()
    for j in audit["strided_sweep"]:
        B, H, W, cin, cout, k = j["shape"]
        stated = bool(H % 2 or W % 2 or k > 7)
        rc = j["rc"]
        if stated:
            refused.add(tuple(j["shape"]))
            ok = rc["create"][0] == -4 and "layer 0" in rc["create"][1] and set(rc) == {"create"} and not any(j["sigs"].values())
        else:
            ok = all(rc.get(p) == (0, "") for p in A.STRIDED_PASSES)
        if not ok:
            bad.append((j["shape"], j["math"], j["fusion"], rc))
    assert not bad, "%d jobs; first: %s" % (len(bad), bad[:5])
    assert refused == set(STRIDED_REFUSED)


def test_the_new_cases_take_the_signatures_written_next_to_them(audit):
    import test_gpu_dispatch_paths as TP
    jobs = {j["case"]: j for j in audit["replay"] if j["list"] == "PATH_CASES"}
    assert sorted(jobs) == sorted(c.name for c in TP.PATH_CASES) and len(jobs) == len(TP.PATH_CASES)
    for c in TP.PATH_CASES:
        j = jobs[c.name]
        assert all(j["rc"][p][0] == 0 for p in A.PASSES), (c.name, j["rc"])
        for p, want in c.expect.items():
            for e in want:
                assert any(matches(e, s) for s in j["sigs"][p]), "%s %s: expected %s, launched %s" % (c.name, p, e, j["sigs"][p])
    # the ledger names every case: removing one from the GPU module shows here even where another case shares its signature
    listed = re.findall(r"^\| `([\w.-]+)` \| (?:conv|lin) ", open(A.LEDGER).read(), flags=re.M)
    assert sorted(listed) == sorted(jobs), set(listed) ^ set(jobs)


def test_the_three_conv_passes_accept_the_same_geometries(audit):
    """(b) forward, data gradient and weight gradient all run or all return the same code; fg_conv2d_workspace_bytes is enough for
    the ones that run (the entries got exactly that many bytes); odd k <= 7 with 'same' padding is refused only for the three
    reasons include/facegen_hip.h states: the folded upsample on a thin layer, the folded upsample at 7x7, and a thin layer whose
    wide operand has 2^31 floats or more (beyond the sweep's cap of 2^25: test_thin_layers_of_2_31_floats_are_refused_by_all_three_passes)."""
    bad = []
    for j in audit["sweep"]:
        codes = {p: j["rc"][p][0] for p in A.PASSES}
        if j["kind"] == "lin":
            if any(codes.values()):
                bad.append((j["shape"], j["rc"]))
            continue
        B, H, W, cin, cout, k, up = j["shape"]
        stated = bool(up) and (k == 7 or thin_layer(cin, cout, k) or thin_layer(cout, cin, k))
        want = -4 if stated else 0          # FG_ERR_UNSUPPORTED
        if any(c != want for c in codes.values()):
            bad.append((j["shape"], j["math"], j["fusion"], {p: j["rc"][p] for p in A.PASSES}))
    assert not bad, "%d geometries; first: %s" % (len(bad), bad[:5])


SIZE_RULE = A.ENGINE + r"""
import ctypes
from face_generator_amd.runtime import make_specs
for j in json.load(open(sys.argv[1])): run_abi(j)
# a net knows its batch when it runs, not when it is created: one thin layer, bound to a small buffer nobody dereferences
h, off, buf = ctypes.c_void_p(), ctypes.c_longlong(), torch.empty(4096)
ctx.check(lib.fg_net_create(ctx.h, make_specs([("CONV", 3, 64, 3, 1)]), 1, 3, 512, 512, ctypes.byref(h)))
ctx.check(lib.fg_net_bind(h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr()))
nb = lib.fg_net_workspace_bytes(h, 127)
for B in (128, 127):
    say("fg-job " + json.dumps(dict(kind="net", shape=[B])))
    say("fg-pass fwd")
    rc = lib.fg_net_forward(h, B, buf.data_ptr(), buf.data_ptr(), nb, 0, None, 0, ctypes.byref(off))
    say("fg-rc %%d %%s" %% (rc, lib.fg_last_error(ctx.h).decode() if rc else ""))
"""
AT_2_31 = [(128, 512, 512, 3, 64, 3), (128, 512, 512, 64, 1, 5), (128, 512, 512, 1, 64, 7), (32, 512, 512, 256, 3, 3)]


def test_thin_layers_of_2_31_floats_are_refused_by_all_three_passes(tmp_path):
    """The size rule (csrc/fg_internal.h fg_thin_fits), planning-only through the C entries: a thin layer whose wide operand has
    exactly 2^31 floats gets FG_ERR_UNSUPPORTED with one message from forward, data gradient and weight gradient and launches
    nothing (before the rule, 64 -> 1 at 5x5 ran forward and data gradient and was refused in the weight gradient alone); one
    sample fewer and all three run, the weight gradient on the matrix pipe.  A net with such a first layer is refused by
    fg_net_forward at batch 128, naming layer 0, and runs at batch 127."""
    import json
    t0 = time.time()
    shapes = AT_2_31 + [(s[0] - 1,) + s[1:] for s in AT_2_31]
    assert all(b * h * w * max(ci, co) == 2 ** 31 for b, h, w, ci, co, k in AT_2_31)
    jobs = [dict(list="size-rule", kind="conv", shape=list(s) + [0], math=0, fusion=A.FG_FUSE_DEFAULT, passes=list(A.PASSES)) for s in shapes]
    f = tmp_path / "jobs.json"
    f.write_text(json.dumps(jobs))
    got = A.parse_jobs(A._run(SIZE_RULE, [str(f)]))
    assert len(got) == len(shapes) + 2
    for j in got[:4]:
        assert {j["rc"][p][0] for p in A.PASSES} == {-4}, (j["shape"], j["rc"])          # FG_ERR_UNSUPPORTED
        assert len({j["rc"][p][1] for p in A.PASSES}) == 1 and "2^31" in j["rc"]["fwd"][1], (j["shape"], j["rc"])
        assert not any(j["sigs"].values()), (j["shape"], j["sigs"])
    for j in got[4:8]:
        assert all(j["rc"][p] == (0, "") for p in A.PASSES), (j["shape"], j["rc"])
        assert any(s[0].startswith("(thin_wgrad_mfma_kernel<") for s in j["sigs"]["wgrad"]), (j["shape"], j["sigs"]["wgrad"])
    at128, at127 = got[8:]
    assert at128["rc"]["fwd"][0] == -4 and "layer 0" in at128["rc"]["fwd"][1] and not at128["sigs"]["fwd"], at128
    assert at127["rc"]["fwd"] == (0, "") and any(s[0].startswith("(thin_in_mfma_kernel<3,") for s in at127["sigs"]["fwd"]), at127
    assert time.time() - t0 < 30


def test_nets_with_reclassified_layers_plan_and_run_forward_and_backward():
    """fg_net_create asks the same predicate as the module-level entries: the gray coarse-to-fine generator (first layer 2 -> 64 at
    3x3) and a chain 4 -> 64 (5x5) -> 192 -> 1 are created, run forward and run backward with parameter gradients (before
    fg_thin_layer the first one planned, ran forward and was refused in its backward: "thin_wgrad: k=3 Cs=2 not built"), their
    few-channel layers as implicit GEMMs with a weight-gradient launch each, the 256 -> 1 7x7 head still on the thin kernels."""
    nets = A.reclassified_net_launches()
    names = {t: [A.sig_of(l)[0] for l in v] for t, v in nets.items()}
    g = names["gray-c2f-G"]
    assert g.count("(igemm_kernel<BM, BN, BK>)") == 1 and g.count("(wgrad_kernel<BT, BK, OCC>)") == 4, g     # 2 -> 64 + three wide layers
    assert not any("thin_in_generic" in n for n in g) and any(n.startswith("(thin_wgrad_mfma_kernel<7, 1") for n in g), g
    c = names["few-channel-chain"]
    assert c.count("(wgrad_kernel<BT, BK, OCC>)") == 3 and not any("thin" in n for n in c), c


def test_no_launch_asks_for_more_lds_than_the_launcher_arranged(audit):
    """a launch above 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize set on that kernel, and nothing above
    160 KB exists -- a planning-only run returns FG_OK for such a launch, a device refuses it.  (The check is by kernel NAME: a
    template one of whose instances raises the limit passes for all its instances.)  The pointwise replay is walked too: its
    DATA_ENTRIES hold the two launches of the data path above 64 KB, warp-c2f-big and warp-faces-big."""
    src = "".join(open(os.path.join(A.CSRC, f)).read() for f in sorted(os.listdir(A.CSRC)) if f.endswith(".hip"))
    raised = set(re.findall(r"hipFuncSetAttribute\(\(const void\*\)\s*([A-Za-z_]\w*)", src))
    bad = {}
    for j in audit["sweep"] + audit["replay"] + audit["pointwise"]:
        for v in j["sigs"].values():
            for s in v:
                if s[2] > LDS_MAX or (s[2] > LDS_PLAIN and A.kernel_of(s[0]) not in raised):
                    bad.setdefault(s, j["shape"])
    assert not bad, bad
    big = {j["case"]: max(s[2] for s in j["sigs"]["run"]) for j in audit["pointwise"] if j["list"] == "DATA_ENTRIES"}
    assert big["warp-c2f-big"] > LDS_PLAIN and big["warp-faces-big"] == 140096, big


def measure_only_sites():
    """kernel names all of whose launch sites sit inside #ifdef FG_MEASURE"""
    inside, outside = set(), set()
    for fn in sorted(os.listdir(A.CSRC)):
        if not fn.endswith(".hip"):
            continue
        stack = []
        for line in open(os.path.join(A.CSRC, fn)):
            t = line.strip()
            if re.match(r"#\s*if", t):
                stack.append("M" if re.match(r"#\s*ifdef\s+FG_MEASURE\b", t) else "-")
            elif re.match(r"#\s*else", t) and stack:
                stack[-1] = {"M": "-", "-": "-"}[stack[-1]]
            elif re.match(r"#\s*endif", t) and stack:
                stack.pop()
            for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", line):
                (inside if "M" in stack else outside).add(m.group(1))
    return inside - outside


def test_every_launch_site_is_entered_in_the_ledger_with_one_status(audit):
    """(c) the census"""
    sites = A.launch_sites()
    rows = A.ledger_rows()
    assert sorted(rows) == sorted(sites), "ledger and csrc/*.hip disagree: %s" % sorted(set(rows) ^ set(sites))
    assert all(st in STATUSES for st, _ in rows.values()), {k: v for k, v in rows.items() if v[0] not in STATUSES}
    # replay: the conv / linear lists, STRIDED_CASES, and the module-level lists of tests/test_gpu_pointwise_paths.py
    # ... and NET_CASES of tests/net_cases.py (whole nets, each compared with the float64 oracle by tests/test_gpu_net_fusions.py)
    # ... and GAN_CASES of tests/gan_cases.py (G / D pairs at the step level, each compared with it by tests/test_gpu_gan_steps.py)
    repk = {A.kernel_of(s[0]) for k in ("replay", "strided_replay", "pointwise", "net_replay", "gan_replay") for s in A.all_sigs(audit[k])}
    swk = {A.kernel_of(s[0]) for k in ("sweep", "strided_sweep") for s in A.all_sigs(audit[k])}
    netk = {A.kernel_of(A.sig_of(l)[0]) for v in audit["nets"].values() for l in v}
    meas = measure_only_sites()
    tests = set(os.listdir(os.path.join(A.ROOT, "tests")))
    for k, (st, note) in sorted(rows.items()):
        if st == "operator":
            assert k in repk, "%s: not seen in the replay" % k
        elif st == "net-only":
            assert k in netk and k not in repk, "%s: net-only means seen in the net logs and not in the replay" % k
            assert any(t in tests for t in re.findall(r"test_gpu_\w+\.py", note)), "%s: name the GPU test that runs it" % k
        elif st == "measure-only":
            assert k in meas, "%s: has a launch site outside #ifdef FG_MEASURE" % k
        elif st == "unreachable":
            assert k not in repk | swk | netk and k not in meas, "%s is reached" % k
            assert len(note) > 20, "%s: say which earlier branch shadows it" % k
        else:       # other-entry: the explicit allow-list above, nothing else
            assert k in OTHER_ENTRY, "%s: other-entry is for %s only; replay its entry in tests/dispatch_audit.py" % (k, sorted(OTHER_ENTRY))
            assert k not in repk | swk | netk and k not in meas, k
            assert any(t in tests for t in re.findall(r"test_gpu_\w+\.py", note)), "%s: name the GPU test of its entry" % k
    assert meas <= {k for k, v in rows.items() if v[0] == "measure-only"}
    assert OTHER_ENTRY == {k for k, v in rows.items() if v[0] == "other-entry"}
    # the two rows that were false: the scalar BatchNorm reductions are launched by BN_CASES with C = 12 / 96 / 2048, by nothing before
    bn = {j["case"]: {A.kernel_of(s[0]) for s in j["sigs"]["run"]} for j in audit["pointwise"] if j["list"] == "BN_CASES"}
    for case in ("3x12", "16421x96", "70x2048", "349600x12"):
        assert {"bn_stats_partial_kernel", "bn_bwd_partial_kernel"} <= bn[case] and not {"bn_stats4_partial_kernel", "bn_bwd4_partial_kernel"} & bn[case], case
    for case in ("5000x4", "130x1024", "2x8", "16421x8", "4096x64"):
        assert {"bn_stats4_partial_kernel", "bn_bwd4_partial_kernel"} <= bn[case], case
    assert not {"bn_stats_partial_kernel", "bn_bwd_partial_kernel"} & {A.kernel_of(s[0]) for s in A.all_sigs(audit["replay"])}


def test_no_capped_grid_without_a_loop():
    """Every launch whose grid expression is capped (FG_GRID(, cr_rowblocks(, bn_apply_blocks(, an explicit min(.., N) or
    `< N ? .. : N`, a following `if (grid.x > N) grid.x = N`, the `rows < 32768` of launch_rows) names a kernel whose body, or a
    __device__ function it calls, reads gridDim in the capped dimension: a grid-stride loop, or a division of the work by the number
    of blocks.  A kernel that handles one unit per thread and returns drops everything above the cap, silently."""
    caps = A.capped_launches()
    names = {c["kernel"] for c in caps}
    assert len(caps) >= 70 and {"zero_insert2_kernel", "zero_insert2_scalar_kernel", "adam_kernel", "rng_kernel", "bn_apply_kernel", "bn_stats_partial_kernel",
                                "sum_splits_kernel", "split_planes_kernel", "thin_in_mfma_pad_kernel", "thin_out_kernel", "thin_out_win_kernel",
                                "thin_wgrad_mfma_kernel"} <= names
    cap = {(c["kernel"], c["dim"]): c["cap"] for c in caps}
    assert cap["prelu_bwd_kernel", "x"] == cap["actpool_bwd_kernel", "x"] == cap["maxpool_prelu_bwd_kernel", "x"] == 1024
    assert cap["norms_partial_kernel", "x"] == 512 and cap["rows_join_split_kernel", "y"] == 32768 and cap["fill_kernel", "x"] == 4096
    assert cap["bn_stats4_partial_kernel", "x"] == 256 and cap["thin_in_mfma_pad_kernel", "x"] == 1024 and cap["thin_in_mfma_kernel", "x"] == 2048
    bad = ["%s (%s): gridDim.%s capped at %d" % (c["kernel"], c["site"], c["dim"], c["cap"]) for c in caps if not c["strides"]]
    assert not bad, "launched with a capped grid by a kernel that never reads gridDim in that dimension:\n" + "\n".join(bad)


def test_the_capped_launchers_table_is_the_census_and_its_cases_reach_the_cap(audit):
    """tests/DISPATCH_COVERAGE.md, "Capped launchers": one row per (kernel, dimension) of the census with its cap; the case named in
    the last column launches the kernel with the clamped grid (planning-only log), and "none" is true: no list and no net
    iteration does.  Every capped launcher that the module-level lists of tests/test_gpu_pointwise_paths.py or STRIDED_CASES reach
    has such a case."""
    census = {(c["kernel"], c["dim"]): c["cap"] for c in A.capped_launches()}
    rows = A.capped_rows()
    assert sorted(rows) == sorted(census), set(rows) ^ set(census)
    jobs = A.all_logs(audit["replay"], audit["strided_replay"], audit["pointwise"], audit["nets"])
    by_id = {A.job_id(j): j for j in jobs}
    module_level = {A.kernel_of(s[0]) for k in ("strided_replay", "pointwise") for s in A.all_sigs(audit[k])}
    for (k, d), (cap, unit, cover) in sorted(rows.items()):
        assert int(cap) == census[k, d] and unit, (k, d, cap)
        hits = A.at_cap(jobs, k, d, census[k, d])
        m = re.match(r"`([^`]+)` `([^`]+)`", cover)
        if m:
            assert (m.group(1), m.group(2)) in by_id, "%s: no job %s" % (k, m.groups())
            assert by_id[m.group(1), m.group(2)] in hits, "%s: %s %s does not launch it with %d blocks in %s" % ((k,) + m.groups() + (census[k, d], d))
            # above the cap, not at it: the pointwise and strided cases are sized 259 units (x 4) past 4096 x 256 and asserted there
        else:
            assert cover.startswith("none") and not hits, "%s: %s" % (k, [A.job_id(j) for j in hits][:3])
            assert k not in module_level or k in CONTRACTION_SIDE, "%s is reached by a module-level list: give it a case above its cap" % k
