"""CPU-only checks of tests/pointwise_domain.py (tests/POINTWISE_DOMAIN.md): every case still launches the kernels it names
(planning-only context with FG_LAUNCH_LOG=1 through tests/dispatch_audit.py, as tests/test_value_domain_host.py does), the probe
layouts hold what the document says they hold, every numpy restatement agrees with oracle/torch7_nn.py where the oracle defines the
case, and the stored Philox offsets produce the extreme words."""
import fnmatch

import numpy as np
import pytest

import dispatch_audit as A
import pointwise_domain as PD
from pointwise_domain import F32, U32, bits
from oracle import torch7_nn as O

PLAN = A.ENGINE + r"""
import pointwise_domain as PD
for c in PD.CASES:
    say("fg-job " + json.dumps(dict(list="POINTWISE_DOMAIN", kind="pointwise", case=c.name, shape=[], math=0, fusion=%(default)d)))
    say("fg-pass run")
    assert PD.run_case(ctx, c, dry=True) == []
    say("fg-rc 0")
"""


@pytest.fixture(scope="module")
def plans():
    from face_generator_amd import build
    build.build(verbose=False)
    return {j["case"]: j for j in A.parse_jobs(A._run(PLAN))}


def test_every_case_launches_the_kernels_it_names(plans):
    assert sorted(plans) == sorted(c.name for c in PD.CASES) and len(plans) == len(PD.CASES)
    for c in PD.CASES:
        j = plans[c.name]
        assert j["rc"]["run"] == (0, ""), (c.name, j["rc"])
        names = [A.kernel_of(s[0]) for s in j["sigs"]["run"]]
        texts = [s[0].strip("()") for s in j["sigs"]["run"]]
        for kernel in c.expect:                     # with "<": a pattern over the whole launch text (the template instance matters)
            assert any(fnmatch.fnmatchcase(t, kernel) for t in texts) if "<" in kernel else kernel in names, \
                "%s: expected %s, launched %s" % (c.name, kernel, sorted(set(texts)))
    # the fused optimizer + re-pack instance, not the plain pack
    assert any("pack_jobs_kernel<true>" in s[0] for s in plans["gan-adam-pack"]["sigs"]["run"]) and "adam_kernel" not in [A.kernel_of(s[0]) for s in plans["gan-adam-pack"]["sigs"]["run"]]
    # the sigmoid of the Linear(K -> 1) head is gemv_fwd_kernel's own; the fused max-pool stages launch neither un-fused kernel
    assert "sigmoid_fwd_kernel" not in [A.kernel_of(s[0]) for s in plans["gemv-sigmoid-net"]["sigs"]["run"]]
    for name in ("actmaxpool-net", "actmaxpool-dropout-net"):
        names = [A.kernel_of(s[0]) for s in plans[name]["sigs"]["run"]]
        assert not {"prelu_fwd_kernel", "maxpool_fwd_kernel", "maxpool_bwd_kernel", "prelu_bwd_kernel", "mul_mask_kernel"} & set(names), (name, sorted(set(names)))


def test_every_part_of_the_document_has_its_kernels(plans):
    seen = {A.kernel_of(s[0]) for j in plans.values() for s in j["sigs"]["run"]}
    for k in ("maxpool_fwd_kernel", "maxpool_bwd_kernel", "actmaxpool_fwd_kernel", "maxpool_prelu_bwd_kernel", "actpool_fwd_kernel", "actpool_bwd_kernel",
              "avgpool_fwd_kernel", "avgpool_bwd_kernel", "upsample_fwd_kernel", "upsample_bwd_kernel", "prelu_fwd_kernel", "prelu_bwd_kernel",
              "leakyrelu_fwd_kernel", "leakyrelu_bwd_kernel", "sigmoid_fwd_kernel", "sigmoid_bwd_kernel", "gemv_fwd_kernel", "mul_mask_kernel",
              "scale_mask_nc_kernel", "add_kernel", "axpby_kernel", "sum_parts_kernel", "sum_splits_actbwd_kernel", "gemv_bwd_act_kernel",
              "thin_in_mfma_kernel", "thin_in_mfma_lds_kernel", "thin_in_mfma_pad_kernel", "igemm_act_kernel",
              "adam_kernel", "sgd_kernel", "adagrad_kernel", "norms_partial_kernel", "bce_kernel", "parzen_dist_kernel", "min_kernel",
              "grid_minmax_kernel", "grid_fill_kernel", "rng_kernel", "rng_multi_kernel", "pack_jobs_kernel"):
        assert k in seen, k


# ---------------------------------------------------------------------------------------------------------------------------------
# probe layouts
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_window_tensor_holds_every_4_tuple_once_and_every_lane_sees_every_value():
    x = PD.window_tensor()
    assert x.shape == PD.WIN_SHAPE and x.size < 2 ** 16
    w = bits(PD.windows(x)).reshape(-1, 4)
    code = {int(b): i for i, b in enumerate(PD.PALETTE)}
    keys = sorted(tuple(code[int(v)] for v in row) for row in w)
    assert keys == sorted(tuple(int(v) for v in np.unravel_index(i, (8, 8, 8, 8))) for i in range(8 ** 4))
    assert not np.array_equal(PD.window_tuples(), np.stack(np.unravel_index(np.arange(8 ** 4), (8, 8, 8, 8)), 1)), "the order is permuted"
    lanes = bits(PD.windows(x)).reshape(-1, 4, 4, 4)                 # [pixel][quad][lane][slot]
    for lane in range(4):
        for slot in range(4):
            assert set(lanes[:, :, lane, slot].reshape(-1).tolist()) == set(PD.PALETTE.tolist())
    assert PD.PALETTE.view(F32)[7] == F32(-2.0 ** -140) and np.isnan(PD.PALETTE.view(F32)[:2]).all()
    # the one-channel form holds the same windows in the same order
    assert np.array_equal(bits(PD.windows(PD.window_tensor_1ch())).reshape(-1, 4), bits(PD.windows(x)).reshape(-1, 4))
    g = PD.actmax_gy()
    assert ((g != 0).sum(-1) == 1).all() and np.isfinite(g).all()


def test_the_probe_vectors():
    p = PD.probes()
    assert 560 <= p.size <= 600 and p.size < 2 ** 16
    b = bits(p)
    p = p[np.isfinite(p)].astype(np.float64)
    for e in range(-149, 128):
        lo, hi = np.ldexp(1.0, e), np.ldexp(1.0, e + 1)
        assert ((p >= lo) & (p < hi)).any() and ((-p >= lo) & (-p < hi)).any(), e
    for v in (0x00000000, 0x80000000, 0x7f7fffff, 0x7f800000, 0xff800000) + tuple(PD.VD.NAN_PROBES):
        assert v in b, hex(v)
    assert np.isnan(PD.probes()).sum() == 6
    # the optimizer probes: all 91 pairs, each in a quad and at another lane (n = 211), a tail of three
    pp, gg = PD.opt_probes(PD.OPT_N)
    assert PD.OPT_N == 211 and PD.OPT_N % 4 == 3
    pairs = {}
    for i, (a, c) in enumerate(zip(bits(pp), bits(gg))):
        pairs.setdefault((int(a), int(c)), []).append(i % 4)
    assert len(pairs) == PD.G_PROBES.size * PD.P_PROBES.size == 91 and all(len(set(v)) >= 2 for v in pairs.values())
    p3, g3 = PD.opt_probes(3)
    assert np.isnan(g3[0]) and np.isinf(g3[1]) and np.isnan(p3[2])
    assert len(PD.OPT_SETTINGS) == 8


def test_axpby_classes_do_not_depend_on_the_order_of_evaluation():
    plain, f1, f2 = PD.axpby_orders(PD.probes(), PD.axpby_y())
    assert np.array_equal(PD.classes(plain), PD.classes(f1)) and np.array_equal(PD.classes(plain), PD.classes(f2))
    assert len(set(PD.classes(plain).tolist())) == 7, "every class occurs"


def test_every_operand_stays_under_2_16_floats():
    assert PD.ACTMAX_B * 32 * 32 * 16 > 2 ** 16      # the nets keep their own shapes (the issue exempts them); everything else:
    for n in (PD.probes().size, PD.OPT_N, PD.NORMS_N, max(PD.BCE_NS), PD.PARZEN[0] * PD.PARZEN[1], int(np.prod(PD.WIN_SHAPE)) // 1):
        assert n <= 2 ** 16, n


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def test_the_max_rule_is_the_oracles_argmax():
    """oracle.SpatialMaxPooling uses argmax: the first NaN of a window wins, else the first maximum; forward and backward share it"""
    x, gy = PD.window_tensor(), PD.pooled_noise()
    m = O.SpatialMaxPooling()
    y = m.updateOutput(nchw(x))
    gx = m.updateGradInput(nchw(x), nchw(gy))
    w = PD.windows(x)
    slot = PD.max_slot(w)
    assert np.array_equal(bits(nhwc(y)), bits(PD.take_slot(w, slot)))
    assert np.array_equal(bits(nhwc(gx)), bits(PD.unwindows(PD.scatter_slot(gy, slot))))
    assert np.array_equal(nhwc(m.indices), slot)
    # the statement itself, without argmax: windows with a NaN choose the first one; the -0 / +0 windows choose slot 0
    nan = np.isnan(w)
    assert (slot[nan.any(-1)] == nan.argmax(-1)[nan.any(-1)]).all() and nan.any(-1).sum() == 8 ** 4 - 6 ** 4
    z = (bits(w) & 0x7fffffff == 0).all(-1)
    assert z.sum() == 16 and (slot[z] == 0).all() and len(set(bits(PD.take_slot(w, slot))[z].tolist())) == 2


@pytest.mark.parametrize("a", PD.SLOPES)
def test_the_fused_stage_reference_is_prelu_then_maxpool_of_the_oracle(a):
    x1, gy, mask = PD.window_tensor_1ch(), PD.actmax_gy(), PD.actmax_mask()
    xpre = np.ascontiguousarray(np.broadcast_to(x1, (PD.ACTMAX_B, 32, 32, 16)))
    for mk in (None, mask):
        y, gx = PD.actmax_reference(xpre, a, gy, mk, 2.0)
        pr, mp = O.PReLU(), O.SpatialMaxPooling()
        pr.weight[0] = a
        with PD.quiet():
            act = pr.updateOutput(nchw(xpre))
            yo = mp.updateOutput(act)
            g = nchw(gy) if mk is None else (nchw(gy) * (nchw(mk) * F32(2))).astype(F32)
            gpre = pr.updateGradInput(nchw(xpre), mp.updateGradInput(act, g))
            if mk is not None:
                yo = (yo * (nchw(mk) * F32(2))).astype(F32)
        assert PD.mismatches(y, nhwc(yo), "nanbits").size == 0
        assert PD.mismatches(gx, nhwc(gpre).astype(np.float64).sum(-1, keepdims=True).astype(F32), "value").size == 0
    with PD.quiet():
        assert np.array_equal(bits(PD.prelu_ref(xpre, a)), bits(nhwc(act)))


def finite_probes():
    p = PD.probes()
    return p[np.isfinite(p)]


def test_pointwise_restatements_against_the_oracle():
    x = finite_probes()
    gy = np.roll(x, 7)
    for a in (0.25, 0.0, -1.0):
        pr = O.PReLU()
        pr.weight[0] = a
        with PD.quiet():
            assert np.array_equal(bits(PD.prelu_ref(x, a)), bits(pr.updateOutput(x)))
            assert np.array_equal(bits(PD.prelu_bwd_ref(x, gy, a)), bits(pr.updateGradInput(x, gy)))
    lk = O.LeakyReLU(0.2)
    with PD.quiet():
        # the oracle's float32 formula is the same expression: the same bits, the +inf of x > FLT_MAX / 2 included
        assert np.array_equal(bits(PD.leakyrelu_ref(x, 0.2)), bits(lk.updateOutput(x)))
        assert np.array_equal(bits(PD.leakyrelu_bwd_ref(x, gy, 0.2)), bits(lk.updateGradInput(x, gy)))
        assert np.isnan(PD.leakyrelu_ref(PD.f32([np.inf]), 0.2))[0] and np.isnan(lk.updateOutput(PD.f32([np.inf])))[0], "LeakyReLU.lua's formula: inf - inf"
        assert PD.leakyrelu_ref(PD.f32([-np.inf]), 0.2)[0] != PD.leakyrelu_ref(PD.f32([-np.inf]), 0.2)[0]
        big = x[x > F32(1.8e38)]
        assert big.size and np.isinf(PD.leakyrelu_ref(big, 0.2)).all()
    # sigmoid: the oracle's float64 module on in-range values
    s = O.Sigmoid()
    xs = x[np.abs(x) < 80].astype(np.float64)
    np.testing.assert_allclose(PD.sigmoid_formula(xs, np.float64), s.updateOutput(xs), rtol=1e-15, atol=0)
    ys = PD.sigmoid_formula(x[np.abs(x) < 80], np.float32)
    gref = s.updateGradInput(xs, np.ones_like(xs))
    np.testing.assert_allclose(PD.sigmoid_bwd_ref(s.output.astype(F32), np.ones(xs.size, F32)), gref, rtol=0, atol=1e-7)      # (1 - y in fp32)
    assert ys.dtype == F32
    bar = PD.sigmoid_bar(PD.probes())
    print("sigmoid bar over the probes: %.3e" % bar)
    assert 0 < bar < 1e-6
    e = PD.sigmoid_formula(PD.f32([-np.inf, np.inf, np.nan]), np.float32)
    assert e[0] == 0 and e[1] == 1 and np.isnan(e[2])
    assert not np.isnan(PD.sigmoid_formula(x, np.float32)).any()
    # pooling: the oracle's modules on finite data
    r = np.random.default_rng(2)
    a4 = r.standard_normal((2, 6, 4, 8)).astype(F32)
    ap = O.SpatialAveragePooling()
    np.testing.assert_allclose(nhwc(ap.updateOutput(nchw(a4))), F32(0.25) * PD.pool4(PD.windows(a4)), rtol=1e-6, atol=1e-7)
    up = O.SpatialUpSamplingNearest(2)
    assert np.array_equal(nhwc(up.updateOutput(nchw(a4))), PD.up2(a4))
    np.testing.assert_allclose(nhwc(up.updateGradInput(nchw(a4[:, :3, :2]), nchw(a4))), PD.pool4(PD.windows(a4)), rtol=1e-6, atol=1e-6)
    m = (r.random((2, 8)) < 0.5).astype(F32)
    pr = O.PReLU()
    pr.weight[0] = -0.5
    act = pr.updateOutput(nchw(a4)) * m[:, :, None, None] * F32(1.25)
    np.testing.assert_allclose(nhwc(ap.updateOutput(act)), PD.actpool_ref(a4, -0.5, m, 1.25), rtol=1e-6, atol=1e-7)
    gy = r.standard_normal((2, 3, 2, 8)).astype(F32)
    gact = ap.updateGradInput(act, nchw(gy)) * m[:, :, None, None] * F32(1.25)
    np.testing.assert_allclose(nhwc(pr.updateGradInput(nchw(a4), gact)), PD.actpool_bwd_ref(a4, gy, -0.5, m, 1.25), rtol=1e-6, atol=1e-7)


def penalty64(p, g, o):
    gg = np.float64(F32(o["gscale"])) * g + np.float64(F32(o["l1"])) * np.sign(p) + np.float64(F32(o["l2"])) * p
    return np.clip(gg, -o["clamp"], o["clamp"]) if o["clamp"] else gg


@pytest.mark.parametrize("o", PD.OPT_SETTINGS, ids=[PD.setting_tag(o) for o in PD.OPT_SETTINGS])
def test_optimizer_restatements_against_the_oracle_on_finite_data(o):
    """the float32 restatements against oracle.interruptable_adam / _sgd / _adagrad in float64, three steps, at the bars of
    tests/test_gpu_pointwise_paths.py (run_opt)"""
    r = np.random.default_rng(12)
    n = 257
    p0 = r.standard_normal(n).astype(F32)
    p0[:3] = [0.0, -0.0, 1e-42]
    pa, ma, va = p0.copy(), np.zeros(n, F32), np.zeros(n, F32)
    p64, st = p0.astype(np.float64), {}
    ps, ms, p64s, sts = p0.copy(), np.zeros(n, F32), p0.astype(np.float64), {}
    pg, vg, p64g, stg = p0.copy(), np.zeros(n, F32), p0.astype(np.float64), {}
    def close(a, b, atol, rtol):
        err = np.abs(a.astype(np.float64) - b)
        assert (err <= atol + rtol * np.abs(b)).all(), (float(err.max()), int(np.argmax(err)))
    for s, t in enumerate(PD.ADAM["ts"]):
        g = (r.standard_normal(n) * 3).astype(F32)
        gp = penalty64(p64, g.astype(np.float64), o)
        st["t"] = t - 1
        O.interruptable_adam(lambda x: (0.0, gp), p64, dict(learningRate=PD.ADAM["lr"], beta1=PD.ADAM["b1"], beta2=PD.ADAM["b2"], epsilon=PD.ADAM["eps"]), st)
        pa, ma, va, go = PD.adam_ref(pa, g, ma, va, o, t)
        close(pa, p64, 2e-7, 2e-7); close(ma, st["m"], 1e-7, 1e-5); close(va, st["v"], 1e-12, 1e-5)
        close(go, gp, 4 * 2.0 ** -24 * (np.abs(g) + 1e-4 + 1e-4 * np.abs(p64)), 0)
        gps = penalty64(p64s, g.astype(np.float64), o)
        O.interruptable_sgd(lambda x: (0.0, gps), p64s, dict(learningRate=PD.SGD["lr"], momentum=PD.SGD["mom"], dampening=PD.SGD["damp"], nesterov=True), sts)
        ps, ms = PD.sgd_ref(ps, g, ms, o, s == 0)
        close(ps, p64s, 1e-5, 0); close(ms, sts["dfdx"], 1e-5, 0)
        gpg = penalty64(p64g, g.astype(np.float64), o)
        O.interruptable_adagrad(lambda x: (0.0, gpg), p64g, dict(learningRate=1e-3), stg)
        pg, vg = PD.adagrad_ref(pg, g, vg, o)
        close(pg, p64g, 1e-6, 0); close(vg, stg["paramVariance"], 0, 1e-5)


def test_the_clamp_of_the_restatement_is_np_clip():
    g = PD.f32([np.nan, np.inf, -np.inf, 7.0, -7.0, 0.5, -0.0])
    o = dict(gscale=1.0, l1=0.0, l2=0.0, clamp=1.0)
    r = PD.prep_grad_ref(g, np.zeros(7, F32), o)
    assert np.isnan(r[0]) and np.array_equal(bits(r[1:]), bits(PD.f32([1, -1, 1, -1, 0.5, -0.0])))
    # what the parent commit's expression did, for the record: fminf(fmaxf(NaN, -c), c) = -c
    assert np.fmin(np.fmax(F32(np.nan), F32(-1)), F32(1)) == -1
    # a NaN parameter reaches the gradient only through the penalty
    assert not np.isnan(PD.prep_grad_ref(PD.f32([0.3]), PD.f32([np.nan]), o))[0]
    assert np.isnan(PD.prep_grad_ref(PD.f32([0.3]), PD.f32([np.nan]), dict(o, l2=1e-4)))[0]


def test_bce_and_norms_and_parzen_restatements():
    crit = O.BCECriterion()
    r = np.random.default_rng(3)
    x = r.uniform(0.01, 0.99, 257).astype(F32)
    t = (r.random(257) < 0.5).astype(F32)
    loss, grad, conf = PD.bce_ref(x, t)
    assert abs(loss[0] - crit.forward(x, t)) <= 1e-6 * abs(crit.forward(x, t))
    np.testing.assert_allclose(grad, crit.backward(x, t), rtol=1e-6, atol=0)
    assert conf.sum() == 257 and conf[3] == ((x > 0.5) & (t > 0.5)).sum()
    # the pinned confusion counts: NaN and 0.5 are both "predicted 0"
    assert PD.bce_ref(PD.f32([np.nan, 0.5]), PD.f32([1, 0]))[2].tolist() == [1, 1, 0, 0]
    for what, v in PD.norms_cases():
        ref = PD.norms_ref(v)
        n2 = np.sqrt((v.astype(np.float64) ** 2).sum())
        if "2e19" in what or "1.5e19" in what:
            assert np.isinf(ref[1]) and np.isfinite(n2) and n2 < 3.4e38 and np.isfinite(ref[0]), what
        if "1e-30" in what:
            assert ref[1] == 0 and n2 > 0
    for what, gen, cond, fine in PD.parzen_cases():
        dist, mn = PD.parzen_ref(gen, cond, fine)
        ok = ~np.isnan(dist)
        assert mn[0] == (dist[ok].min() if ok.any() and dist[ok].min() < 1e10 else F32(1e10)), what
        assert not (dist < 0).any()
    g, mm = PD.grid_ref(PD.grid_cases()[1][1])
    assert np.isnan(g).sum() == 1 and np.isfinite(mm).all(), "a NaN pixel poisons nobody else"
    g, mm = PD.grid_ref(PD.grid_cases()[2][1])
    assert mm[1] == np.inf and np.isnan(g).sum() > 1 and (g[~np.isnan(g)] == 0).all(), "+inf: every finite pixel 0, the pixel and the padding NaN"


# ---------------------------------------------------------------------------------------------------------------------------------
# Philox at its extreme words
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_stored_philox_offsets_are_the_first_extreme_words():
    import test_gpu_pointwise_paths as TQ
    hi, lo = PD.philox_search()
    assert hi == PD.RNG_MAX and lo == PD.RNG_ZERO, (hi, lo)
    wmax = TQ.philox_words(PD.RNG_SEED, PD.RNG_MAX[0], 1).reshape(-1)
    wzero = TQ.philox_words(PD.RNG_SEED, PD.RNG_ZERO[0], 1).reshape(-1)
    assert wmax[PD.RNG_MAX[1]] >> 8 == 0xFFFFFF and wzero[PD.RNG_ZERO[1]] >> 8 == 0
    k = PD.RNG_MAX[1]
    assert PD.uniform_ref(wmax, -1.0, 1.0)[k] == F32(1 - 2.0 ** -23) < 1, "nn_utils.lua:9's noise range never yields 1"
    assert PD.uniform_ref(wmax, 0.0, 1.0)[k] == F32(1 - 2.0 ** -24)
    assert PD.uniform_ref(wmax, 0.5, 1.5)[k] == F32(1.5), "0.5 + (1 - 2^-24) rounds to hi itself"
    assert (PD.uniform_ref(wzero, -1.0, 1.0)[PD.RNG_ZERO[1]], PD.uniform_ref(wzero, 0.5, 1.5)[PD.RNG_ZERO[1]]) == (-1.0, 0.5)
    for w in (wmax, wzero):
        assert np.isfinite(TQ.box_muller(w, np.float64)).all() and np.isfinite(TQ.box_muller(w, np.float32)).all()


@pytest.mark.parametrize("name", PD.E2E_CASES)
def test_the_oracle_ends_the_nan_step_with_nan_parameters(name):
    """what the device test takes from the oracle: with np.clip as the clamp, a closure that saw one NaN leaves the loss and every
    parameter the NaN reaches NaN, under each of the three optimizers at train.lua's default clamps"""
    for rule in PD.E2E_RULES:
        c = PD.gan_case(name, optD=rule, optG=rule)
        for which in "DG":
            st, ref, reached = PD.e2e_oracle(c, which)
            assert np.isnan(ref["f_bce"]) and reached.any(), (name, rule[0], which)
            assert not np.isnan(st.pG if which == "D" else st.pD).any(), "the other net is untouched"
