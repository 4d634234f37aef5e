"""CPU-only checks of tests/value_domain.py: every case still launches the kernel it names (planning-only context with
FG_LAUNCH_LOG=1 through tests/dispatch_audit.py, as tests/test_dispatch_coverage_host.py does -- a case that silently falls to another
kernel tests nothing), the range precondition of the homogeneity test, the split specification, the validity of the Winograd bound
for a float32 evaluation of the same algorithm, the one-hot expectation, and the BatchNorm bars against a float32 emulation of the
shifted single pass."""
import numpy as np
import pytest

import dispatch_audit as A
import value_domain as VD
from value_domain import F32, U32

PLAN = A.ENGINE + r"""
for j in json.load(open(sys.argv[1])): run_ops(j)
"""


@pytest.fixture(scope="module")
def plans():
    from face_generator_amd import build
    build.build(verbose=False)
    jobs = [dict(list="VCASES", kind=c.kind, case=c.name, shape=list(c.shape), math=c.math, fusion=c.fusion, hook=c.hook, passes=VD.passes(c)) for c in VD.VCASES]
    return {j["case"]: j for j in A._run_jobs(PLAN, jobs)}


def test_every_case_launches_the_kernel_it_names(plans):
    assert sorted(plans) == sorted(c.name for c in VD.VCASES) and len(plans) == len(VD.VCASES)
    for c in VD.VCASES:
        j = plans[c.name]
        for p, kernel in c.expect.items():
            assert j["rc"][p] == (0, ""), (c.name, p, j["rc"][p])
            names = [A.kernel_of(s[0]) for s in j["sigs"][p]]
            assert kernel in names, "%s %s: expected %s, launched %s" % (c.name, p, kernel, j["sigs"][p])
            if p in c.wino:
                assert names.count(kernel) == 1 and not any(n.startswith(("igemm", "wgrad_kernel", "wgrad_ws")) for n in names), (c.name, p, names)


def test_the_families_of_the_issue_are_all_there(plans):
    """igemm / igemm_ws / igemm_ws64x3; igemm_ws6 <64> and <128>, forward and data gradient, with and without split-K; the three direct
    weight gradients; Winograd forward / data gradient at 3x3, 5x5 and folded, Winograd weight gradient; thin_in, thin_out slab and
    tiled, thin_wgrad_mfma; the gemv pair"""
    seen = {}
    for c in VD.VCASES:
        for p in c.expect:
            for s in plans[c.name]["sigs"][p]:
                seen.setdefault(A.kernel_of(s[0]), []).append((c.name, p, s[2], [A.kernel_of(t[0]) for t in plans[c.name]["sigs"][p]]))
    for k in ("igemm_kernel", "igemm_ws_kernel", "igemm_ws64x3_kernel", "igemm_ws6_kernel", "wgrad_kernel", "wgrad_ws_kernel", "wgrad_ws6_kernel", "wino_kernel",
              "wino_wgrad_kernel", "thin_in_mfma_kernel", "thin_out_slab_mfma_kernel", "thin_out_tiled_kernel", "thin_wgrad_mfma_kernel", "gemv_fwd_kernel",
              "gemv_bwd_kernel", "split_planes_kernel"):
        assert k in seen, k
    ws6 = {(p, lds, any(n.startswith("sum_splits") for n in names)) for (_, p, lds, names) in seen["igemm_ws6_kernel"]}
    # (pass, LDS bytes: 108544 = <64>, 130048 = <128>, split-K)
    assert {("fwd", 130048, False), ("fwd", 108544, False), ("dgrad", 108544, False), ("dgrad", 108544, True), ("fwd", 130048, True), ("dgrad", 130048, True)} <= ws6, ws6
    wino = {(c.shape[5], c.shape[6], p) for c in VD.VCASES for p in c.wino}
    assert {(3, 0, "fwd"), (3, 0, "dgrad"), (5, 0, "fwd"), (5, 0, "dgrad"), (5, 1, "fwd"), (5, 1, "dgrad"), (3, 0, "wgrad")} <= wino


def test_operands_stay_under_2_23_floats():
    for c in VD.VCASES:
        s = VD.shapes(c)
        used = [s["w"]] * bool({"fwd", "dgrad"} & set(c.expect)) + [s["x"]] * bool({"fwd", "wgrad"} & set(c.expect)) + [s["gy"]] * bool({"dgrad", "wgrad"} & set(c.expect))
        assert all(int(np.prod(u)) < 2 ** 23 for u in used), (c.name, used)


@pytest.mark.parametrize("name", [c.name for c in VD.VCASES])
def test_scaled_runs_stay_between_2_m100_and_2_100(name):
    """the precondition of the homogeneity test, from the float64 reference of the unscaled operands (scaling by 2^(a + b) is exact in
    float64): no nonzero reference output of a scaled run below 2^-100 or above 2^100, and the scaled operands themselves (and the
    lowest plane of the three-way split: 2^-24 of the operand) normal"""
    c = VD.BY_NAME[name]
    op = VD.unit_operands(c)
    ref = VD.reference(c, op)
    for a, b in VD.SCALES:
        for p, r in ref.items():
            nz = np.abs(r[r != 0]) * 2.0 ** (a + b)
            assert nz.size and nz.min() >= 2.0 ** -100 and nz.max() <= 2.0 ** 100, (name, p, a, b, nz.min(), nz.max())
        sc = VD.scaled_operands(op, a, b)
        for k, v in sc.items():
            nz = np.abs(v[v != 0]).astype(np.float64)
            assert nz.min() * 2.0 ** -24 > 2.0 ** -126 and nz.max() < 2.0 ** 100, (name, k, a, b)
            assert np.array_equal(np.ldexp(v.astype(np.float64), -(b if k in ("w", "gy_wgrad") else a)), op[k.split("_")[0]].astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# the split specification
# ---------------------------------------------------------------------------------------------------------------------------------
def probe_values():
    rng = np.random.default_rng(5)
    v = np.concatenate([VD.finite_probes(), rng.integers(0, 0x7f7f0001, 200000, dtype=np.int64).astype(U32), (rng.integers(0, 0x7f7f0001, 200000, dtype=np.int64) | 0x80000000).astype(U32)])
    return v[(v & 0x7fffffff) <= VD.SPLIT_MAX]


def test_split3_is_exact_wherever_its_planes_are_normal_or_zero():
    v = probe_values()
    h, m, l = VD.split3(v.view(F32))
    sub = VD.plane_is_subnormal(h) | VD.plane_is_subnormal(m) | VD.plane_is_subnormal(l)
    tot = VD.bf16_value(h).astype(np.float64) + VD.bf16_value(m).astype(np.float64) + VD.bf16_value(l).astype(np.float64)
    assert np.isfinite(tot).all()
    x = v.view(F32).astype(np.float64)
    # an fp32-subnormal operand is outside the statement: bf16 subnormals resolve 2^-133, so its bits below that are lost by the
    # specification itself (0x00000001 splits to three zero planes)
    # (the statement "exact wherever the planes are normal or zero" needs one more clause at the very bottom: a residual below 2^-134
    # rounds to a ZERO plane, e.g. 0x00000001 -> (0, 0, 0); from 2^-103 up no plane is subnormal and no residual is lost)
    ok = np.abs(x) >= 2.0 ** -103
    assert not sub[ok].any() and np.array_equal(tot[ok], x[ok]) and np.array_equal(tot[x == 0], x[x == 0])
    # with subnormal planes honoured (the matrix pipe does, tests/VALUE_DOMAIN.md) the sum is x rounded to a multiple of 2^-133, the
    # resolution of a bf16 subnormal: exact for every |x| >= 2^-110 (ulp 2^-133), within 2^-134 below, zero below 2^-134
    big = np.abs(x) >= 2.0 ** VD.MODE6_EXACT_MIN_EXP
    assert np.array_equal(tot[big], x[big]) and (np.abs(tot - x) <= VD.MODE6_ABS_ERR).all()
    assert (tot[np.abs(x) < 2.0 ** -134] == 0).all()
    assert (tot != x)[~big & (np.abs(x) >= 2.0 ** -111)].any(), "2^-110 is the first exponent that is always exact"
    assert np.array_equal(VD.split3_sum(v.view(F32)).astype(np.float64), tot)
    assert ok.sum() > 300000


def test_where_the_planes_go_subnormal():
    """For operands in [2^e, 2^(e+1)): the h plane is a bf16 subnormal exactly for the fp32-subnormal operands (e <= -127).  A residual
    can be as small as the operand's last bit, 2^(e-23), so the m and l planes CAN be subnormal from e = -104 down; with a random
    mantissa they typically are from about 2^-118 (m) and 2^-110 (l) down, and from those exponents on most operands have one."""
    rng = np.random.default_rng(6)
    first, most = {}, {}
    for e in range(-149, -90):
        lo = 1 << max(e + 149, 0) if e < -126 else ((e + 127) << 23)
        n = lo if e < -126 else (1 << 23)
        v = (lo + rng.integers(0, n, 20000)).astype(U32)
        v[0] = lo + 1 if n > 1 else lo                      # only the last bit set below the leading one
        for name, pl in zip("hml", VD.split3(v.view(F32))):
            if VD.plane_is_subnormal(pl).any():
                first[name] = e
            if VD.plane_is_subnormal(pl).mean() > 0.5:
                most[name] = e
    print("largest operand exponent with a subnormal plane:", first, "; with most operands having one:", most)
    assert first == dict(h=-127, m=-104, l=-104)
    assert most["h"] == -127 and -120 <= most["m"] <= -116 and -112 <= most["l"] <= -108


def test_three_plane_operand_gives_each_of_the_six_products_a_bit_of_its_own():
    x = F32(VD.THREE_PLANE)
    assert np.float64(x) == VD.THREE_PLANE
    h, m, l = (float(VD.bf16_value(p)[0]) for p in VD.split3(np.array([x, -x], F32)[:1]))
    assert (h, m, l) == (1.0, 2.0 ** -10, 2.0 ** -19)
    six = [h * h, h * m, m * h, h * l, l * h, m * m]
    assert sum(six) == VD.THREE_PLANE_PRODUCT == float(F32(VD.THREE_PLANE_PRODUCT)) == float(F32(np.float64(x) * np.float64(x)))
    # leaving any one out, or counting one twice, changes the fp32 result; every partial sum is exact in fp32 (21 bits)
    for i in range(6):
        assert float(F32(sum(six) - six[i])) != VD.THREE_PLANE_PRODUCT and float(F32(sum(six) + six[i])) != VD.THREE_PLANE_PRODUCT
    import itertools
    for r in range(1, 7):
        for sub in itertools.combinations(six, r):
            assert float(F32(sum(sub))) == sum(sub)
    for s in (-60, 60):       # the probes' scales keep every plane product normal
        assert 2.0 ** -126 < l * l * 2.0 ** s < 2.0 ** 100


def test_nan_in_gives_nan_out_and_the_unguarded_rounding_did_not():
    nans = np.array(VD.NAN_PROBES, dtype=U32)
    for pl in VD.split3(nans.view(F32)):
        assert np.isnan(VD.bf16_value(pl)).all()
    wrapped = VD.bf16_rn_unguarded(nans.view(F32))
    assert [int(x) for x in wrapped[3:]] == [0x0000, 0x0000, 0x0000] or [int(x) & 0x7fff for x in wrapped[3:]] == [0, 0, 0]
    assert np.isnan(VD.bf16_value(wrapped[:2])).all()
    # 0x7f800001: the high plane rounds to +inf
    assert int(wrapped[2]) == 0x7f80
    # the top of the range: 0x7f7f0000 splits exactly, 0x7f7f8000 rounds its high plane to infinity
    top = np.array([VD.SPLIT_MAX, 0x7f7f8000, 0x7f7fffff], dtype=U32)
    h, m, l = VD.split3(top.view(F32))
    assert [int(x) for x in h] == [0x7f7f, 0x7f80, 0x7f80] and np.isnan(VD.bf16_value(l)[1:]).all() and int(m[0]) == 0 and int(l[0]) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# probes and the one-hot expectation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in VD.VCASES])
def test_one_hot_expectation_is_the_float64_contraction_and_probes_keep_their_distance(name):
    c = VD.BY_NAME[name]
    for p in [q for q in VD.passes(c) if q != "wgrad"]:
        opn, S = VD.probe_operand(c, p)
        shape = VD.shapes(c)[opn]
        slots = VD.probe_slots(shape, S, VD.observed_channels(c))
        assert len(slots) and len(set(slots.tolist())) == len(slots)
        sparse = VD.sparse_slots(shape, S, VD.observed_channels(c))
        assert len(sparse) and len(set(sparse.tolist())) == len(sparse)
        if len(shape) == 4:
            B, H, W, C = shape
            b, y, x, ch = np.unravel_index(slots, shape)
            res = {(int(yy) % 2, int(xx) % 2) for yy, xx in zip(y, x)}
            assert res == {(0, 0), (0, 1), (1, 0), (1, 1)}, "a tile row / column residue without a probe"
            assert y.max() >= H - 2 and x.max() >= W - 2 and y.min() == 0 and x.min() == 0, "no probe in the first / last tile"
            for key in set(zip(b.tolist(), ch.tolist())):
                sel = (b == key[0]) & (ch == key[1])
                ys, xs = y[sel], x[sel]
                d = np.maximum(np.abs(ys[:, None] - ys[None]), np.abs(xs[:, None] - xs[None])) + S * np.eye(len(ys), dtype=int)
                assert d.min() >= S
        vals = VD.finite_probes()
        vals = vals[(vals & 0x7f800000) != 0][:len(slots)]       # normal probes: float64 holds the copy exactly
        a, used, v = VD.probe_rounds(shape, slots, vals)[0]
        s = VD.shapes(c)
        op = dict(x=a if opn == "x" else np.zeros(s["x"], F32), gy=a if opn == "gy" else np.zeros(s["gy"], F32), w=VD.onehot_weights(c, p))
        want = VD.onehot_expected(c, p, a)
        assert np.array_equal(VD.reference(c, op, [p])[p], want.astype(np.float64)), (name, p)
        assert len(v) == len(used) and (want != 0).sum() >= len(v), "every probe placed reaches an output"
        if c.kind == "conv" and c.shape[6]:
            # the folded form is the same operation on finite operands ...
            un = VD.unit_operands(c)
            r0, r1 = VD.reference(c, un, [p])[p], VD.reference_folded(c, un, [p])[p]
            assert np.abs(r0 - r1).max() <= 1e-12 * np.abs(r0).max()
            # ... and on a non-finite source pixel it keeps the pixel's own class where the unfolded form has 0 * inf
            a2 = np.zeros(shape, F32)
            a2[0, 2, 2, 0] = np.inf
            op2 = dict(op, **{opn: a2})
            with np.errstate(invalid="ignore"):
                f = VD.reference_folded(c, op2, [p])[p]
                u = VD.reference(c, op2, [p])[p]
            assert (f == np.inf).any() and not (u == np.inf).any() and np.array_equal(np.isfinite(f), np.isfinite(u))


@pytest.mark.parametrize("name", [c.name for c in VD.VCASES if "wgrad" in c.expect and "wgrad" not in c.wino])
def test_weight_gradient_copy_reaches_every_probe(name):
    """x = 1 at one pixel: the float64 weight gradient is a float32 in every element, and every probe placed in gy comes out in it"""
    c = VD.BY_NAME[name]
    vals = VD.finite_probes()
    vals = vals[vals << 1 != 0]
    rounds = VD.wgrad_copy_operands(c, vals)
    assert 1 <= len(rounds) <= 3
    out = []
    for x, gy in rounds:
        ref = VD.reference(c, dict(x=x, gy=gy, w=np.zeros(VD.shapes(c)["w"], F32)), ["wgrad"])["wgrad"]
        assert np.array_equal(ref.astype(F32).astype(np.float64), ref)
        out.append(np.unique(VD.bits(ref.astype(F32))))
    assert set(vals.tolist()) <= set(np.concatenate(out).tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# the Winograd evaluation and its bound
# ---------------------------------------------------------------------------------------------------------------------------------
WINO = [(c.name, p) for c in VD.VCASES for p in c.wino]


@pytest.mark.parametrize("name,p", WINO)
def test_winograd_float32_evaluation_stays_inside_the_bound(name, p):
    """the algorithm of wino.hip / wino_wgrad.hip in numpy: in float64 it IS the convolution (the decomposition into groups, parities
    and folded taps is right); in float32, on the very operands of the GPU test, it stays inside (K_c + 16) 2^-24 times its own
    evaluation on absolute values -- so the bound is valid for a correct fp32 implementation, whatever the device measures"""
    c = VD.BY_NAME[name]
    op = VD.wide_operands(c)
    ref = VD.reference(c, op, [p])[p]
    ev = (lambda t: VD.wino_wgrad_eval(c, op["x"], op["gy"], t)) if p == "wgrad" else (lambda t: VD.wino_eval(c, p, op["x"] if p == "fwd" else op["gy"], op["w"], t))
    e64 = ev(np.float64)
    assert np.abs(e64 - ref).max() <= 1e-12 * np.abs(ref).max(), "the numpy Winograd is not the convolution"
    bnd = VD.bound(c, op, p)
    direct = VD.direct_bound(c, op, [p])[p]
    assert (bnd >= direct * (VD.wino_channel_reduction(c, p) + VD.WINO_C) / (VD.reduction_length(c, p) + 16) * (1 - 1e-12)).all(), "absolute-value matrices bound the direct sum"
    err = np.abs(ev(F32).astype(np.float64) - ref)
    r = float((err / bnd).max())
    print("%s %s: float32 numpy evaluation: max |err| / bound = %.4f" % (name, p, r))
    assert r <= 1.0
    assert r >= 1e-4, "a bound four orders above a float32 evaluation says nothing"


def test_direct_bound_holds_for_a_float32_matmul():
    c = VD.BY_NAME["gemv"]
    op = VD.wide_operands(c)
    ref, bnd = VD.reference(c, op), VD.direct_bound(c, op)
    got = dict(fwd=op["x"] @ op["w"].T, dgrad=op["gy"] @ op["w"], wgrad=op["gy"].T @ op["x"])
    for p in ref:
        assert (np.abs(got[p].astype(np.float64) - ref[p]) <= bnd[p]).all(), p


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm: the partition of the statistics launch, the derived bars, the float32 emulation of the shifted single pass
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_partition_is_the_one_in_the_source():
    import os
    import re
    src = open(os.path.join(A.CSRC, "pointwise.hip")).read()
    assert re.search(r"#define CR_ROWBLOCKS 256\b", src) and re.search(r"#define CR4_NT 1024\b", src)
    assert "(M + 63) / 64 < CR_ROWBLOCKS ? (M + 63) / 64 : CR_ROWBLOCKS" in src
    assert "C % 4 == 0 && C >= 4 && C <= 1024 && 256 % (C / 4) == 0" in src
    assert "const float d = x[r * C + c] - x[c];" in src and "const float4 piv = *((const float4*)x + threadIdx.x % (C >> 2));" in src
    assert VD.bn_partition(4096, 96) == (64, 64, 4, False) and VD.bn_partition(4096, 8) == (64, 64, 512, True)
    assert VD.bn_partial_adds(4096, 96) == 18 and VD.bn_partial_adds(4096, 8) == 64
    assert VD.bn_partition(64 * 256 + 37, 96)[:2] == (256, 65) and VD.bn_partition(1, 8)[:2] == (1, 1)


@pytest.mark.parametrize("C", VD.BN_LADDERS)
@pytest.mark.parametrize("k", VD.BN_PIVOTS)
def test_shifted_pass_in_float32_stays_inside_the_pivot_terms(C, k):
    op = VD.bn_outlier_operands(4096, C, k)
    x = op["x"].astype(np.float64)
    t, dm, r = VD.bn_pivot_terms(op)
    infl = t / VD.U / r
    # the pivot is k standard deviations of the other rows out; its own row adds k^2 / M to the variance
    assert (infl > 0.4 * (1 + k * k) / (1 + k * k / 4096.0)).all() and (infl < 1.1 * (1 + k * k)).all(), (infl.min(), infl.max())
    mean, var = VD.bn_shifted_pass_f32(op["x"])
    ev, em = np.abs(var / x.var(0) - 1), np.abs(mean - x.mean(0))
    print("bn pivot C=%d k=%d: float32 emulation: variance error / term %.4f, mean error / term %.4f" % (C, k, float((ev / t).max()), float((em / dm).max())))
    assert (ev <= t).all() and (em <= dm).all()
    assert (ev / t).max() > 1e-4, "a term four orders above the emulation says nothing"


def test_pivot_zero_at_a_large_offset_breaks_the_bars():
    """the sensitivity of the large-offset cases: the same emulation with the pivot replaced by 0 puts mean^2 / var = 4e8 times the
    mass into the fp32 sums and misses bn_invstd_rtol by orders of magnitude; with the pivot it is inside"""
    import test_gpu_pointwise_paths as TQ
    from gpu_util import BAR
    op = TQ.bn_operands(4096, 64, TQ.Src(4160), offset=1000.0)
    x = op["x"].astype(np.float64)
    inv = lambda var: 1 / np.sqrt(var + TQ.BN_EPS)
    good, bad = VD.bn_shifted_pass_f32(op["x"])[1], VD.bn_shifted_pass_f32(op["x"], pivot=0.0)[1]
    assert (np.abs(inv(good) / inv(x.var(0)) - 1) <= BAR["bn_invstd_rtol"]).all()
    assert (np.abs(inv(bad) / inv(x.var(0)) - 1) > 100 * BAR["bn_invstd_rtol"]).any()


def test_constant_channel_is_exactly_zero_variance_without_the_clamp():
    op, const = VD.bn_constant_operands(4096, 96)
    mean, var = VD.bn_shifted_pass_f32(op["x"])
    cc = sorted(const)
    assert np.array_equal(var[cc], np.zeros(len(cc))) and np.array_equal(mean[cc], [const[c] for c in cc])
    assert set(const.values()) == {float(F32(v)) for v in VD.BN_CONSTANTS} >= {0.0, 1000.0, -3.25} and op["x"][0, 4] == 1000.0
    # un-shifted fp32 sums (pivot 0) keep 0, 1000 and -3.25 at variance 0 by luck -- their squares add exactly -- but not 1000.1
    bad = VD.bn_shifted_pass_f32(op["x"], pivot=0.0)[1]
    nice = [c for c in cc if const[c] in (0.0, 1000.0, -3.25)]
    assert not bad[nice].any() and all(bad[c] > 1e-4 for c in cc if c not in nice)

