"""The value domain of the contraction kernels and of BatchNorm on the device (tests/VALUE_DOMAIN.md; cases, references and bounds in
tests/value_domain.py; tests/test_value_domain_host.py shows on the CPU that every case launches the kernel it names and that the
bounds hold for a float32 evaluation).

  1. power-of-two homogeneity, bit for bit: a hidden absolute constant, clamp, flush or narrower intermediate breaks it;
  2. operands over 24 octaves of dynamic range against float64, inside an a-priori bound of the reference alone;
  3. the edges of the documented domain (include/facegen_hip.h, fg_set_math) through a one-hot contraction whose output is a copy of
     its input: every binade, the top of the range, infinities and NaNs;
  4. BatchNorm statistics with an outlying pivot, constant channels, one and two rows, the sync path at a large offset."""
import functools

import numpy as np
import pytest
import torch

import value_domain as VD
from value_domain import F32, U32

pytestmark = pytest.mark.gpu

IDS = [c.name for c in VD.VCASES]


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math, fusion = c.get_math(), c.get_fusion()
    yield c
    c.set_math(math); c.set_fusion(fusion)
    c.check(c.lib.fg_test_set_wino_wgrad_thresholds(c.h, 0, 0))


def device_passes(ctx, c, op, which=None):
    """the case's passes on the device under its own math mode, fusion bits and hook -> {pass: float32 numpy}; no bias (zeros)"""
    from face_generator_amd import ops
    which = VD.passes(c) if which is None else which
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(ctx.device)
    math, fusion = ctx.get_math(), ctx.get_fusion()
    ctx.set_math(c.math); ctx.set_fusion(c.fusion)
    ctx.check(ctx.lib.fg_test_set_wino_wgrad_thresholds(ctx.h, int(c.hook), int(c.hook)))
    out = {}
    try:
        w = put(op["w"]) if ("fwd" in which or "dgrad" in which) else None
        x = put(op["x"]) if ("fwd" in which or "wgrad" in which) else None
        gy = put(op["gy"]) if "dgrad" in which else None
        gyw = put(op.get("gy_wgrad", op["gy"])) if "wgrad" in which else None
        if c.kind == "lin":
            B, K, N = c.shape
            zb = torch.zeros(N, device=ctx.device)
            if "fwd" in which: out["fwd"] = ops.linear_forward(x, w, zb)
            if "dgrad" in which: out["dgrad"] = ops.linear_backward_data(gy, w)
            if "wgrad" in which: out["wgrad"] = ops.linear_backward_weight(x, gyw)[0]
        else:
            B, H, W, Cin, Cout, k, up = c.shape
            zb = torch.zeros(Cout, device=ctx.device)
            if "fwd" in which: out["fwd"] = ops.conv2d_forward(x, w, zb, upsample2x=bool(up))
            if "dgrad" in which: out["dgrad"] = ops.conv2d_backward_data(gy, w, (H, W), upsample2x=bool(up))
            if "wgrad" in which: out["wgrad"] = ops.conv2d_backward_weight(x, gyw, k, upsample2x=bool(up))[0]
        return {p: v.cpu().numpy() for p, v in out.items()}
    finally:
        ctx.set_math(math); ctx.set_fusion(fusion)
        ctx.check(ctx.lib.fg_test_set_wino_wgrad_thresholds(ctx.h, 0, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. homogeneity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_power_of_two_scaling_commutes_bit_for_bit(ctx, name):
    """y(2^a x, 2^b w) == ldexp(y(x, w), a + b) in every bit of every output of every pass, for (a, b) in VD.SCALES: scaling by a power
    of two commutes with every fp32 rounding as long as nothing under- or overflows (the host test shows nothing does)."""
    c = VD.BY_NAME[name]
    op = VD.unit_operands(c)
    base = device_passes(ctx, c, op)
    for p, y in base.items():
        assert np.isfinite(y).all() and np.abs(y).max() > 0, (name, p)
    for a, b in VD.SCALES:
        got = device_passes(ctx, c, VD.scaled_operands(op, a, b))
        for p in VD.passes(c):
            want = np.ldexp(base[p], a + b).astype(F32)
            diff = VD.bits(got[p]) != VD.bits(want)
            print("%s %s scaled by 2^(%d, %d): %d of %d outputs differ" % (name, p, a, b, int(diff.sum()), diff.size))
            if diff.any():
                i = np.unravel_index(int(np.argmax(diff)), diff.shape)
                raise AssertionError("%s %s: scaling by (2^%d, 2^%d) changed %d of %d outputs; first at %s: got %r, want %r (unscaled %r)"
                                     % (name, p, a, b, int(diff.sum()), diff.size, i, got[p][i], want[i], base[p][i]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. wide dynamic range against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def wide_reference(name):
    c = VD.BY_NAME[name]
    op = VD.wide_operands(c)
    return op, VD.reference(c, op), {p: VD.bound(c, op, p) for p in VD.passes(c)}


def wide_ratios(ctx, name):
    c = VD.BY_NAME[name]
    op, ref, bnd = wide_reference(name)
    got = device_passes(ctx, c, op)
    out = {}
    for p in VD.passes(c):
        err = np.abs(got[p].astype(np.float64) - ref[p])
        assert np.isfinite(got[p]).all(), (name, p)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bnd[p] > 0, err / bnd[p], np.where(err > 0, np.inf, 0.0))
        out[p] = (float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape), float(err.max()))
    return out, got, ref, bnd


@pytest.mark.parametrize("name", IDS)
def test_wide_dynamic_range_within_the_a_priori_bound(ctx, name):
    """operands N(0, 1) 2^e with e drawn per element: |got - float64| <= (K + 16) 2^-24 A, A the same contraction of the absolute
    values (Winograd: the algorithm on absolute values with absolute-value matrices, K_c + 16) -- the unit-scale bars of gpu_util.BAR
    mean nothing here, and the bound comes from the reference alone"""
    ratios, got, ref, bnd = wide_ratios(ctx, name)
    for p, (r, i, e) in ratios.items():
        print("value-domain wide %s %s: max |err| / bound = %.4f (at %s; max |err| %.3e, max |ref| %.3e)" % (name, p, r, i, e, float(np.abs(ref[p]).max())))
    for p, (r, i, e) in ratios.items():
        assert r <= 1.0, "%s %s: |err| / bound = %.3f at %s: got %r, float64 %r, bound %.3e" % (name, p, r, i, got[p][i], ref[p][i], bnd[p][i])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. edges of the documented domain
# ---------------------------------------------------------------------------------------------------------------------------------
def copy_passes(c):
    return [p for p in VD.passes(c) if p != "wgrad"]        # the one-hot contraction is defined by its weights


COPY_IDS = ["%s-%s" % (c.name, p) for c in VD.VCASES for p in copy_passes(c)]


def run_probe_rounds(ctx, c, p, rounds):
    """-> [(expected copy float32, device output float32)] per round"""
    name, _ = VD.probe_operand(c, p)
    w = VD.onehot_weights(c, p)
    s = VD.shapes(c)
    res = []
    for a, slots, vals in rounds:
        op = dict(x=a if name == "x" else np.zeros(s["x"], F32), gy=a if name == "gy" else np.zeros(s["gy"], F32), w=w)
        res.append((VD.onehot_expected(c, p, a), device_passes(ctx, c, op, [p])[p]))
    return res


def finite_probe_table(ctx, c, p):
    """every finite probe through the one-hot pass -> (input bits, output bits) of every output that copies a probe, and the number of
    outputs elsewhere that are not zero"""
    name, S = VD.probe_operand(c, p)
    shape = VD.shapes(c)[name]
    values = VD.finite_probes()
    if not VD.mode6(c, p):                                  # finite in fp32: 0x7f7f8000 and 0x7f7fffff are copied like any other value
        values = np.concatenate([values, np.array(VD.TOP_PROBES, dtype=U32), np.array(VD.TOP_PROBES, dtype=U32) | U32(0x80000000)])
    rounds = VD.probe_rounds(shape, VD.probe_slots(shape, S, VD.observed_channels(c)), values)
    xin, yout, stray = [], [], 0.0
    for want, got in run_probe_rounds(ctx, c, p, rounds):
        assert want.shape == got.shape, (want.shape, got.shape)
        at = VD.bits(want) << 1 != 0                        # where the copy holds a nonzero probe
        xin.append(VD.bits(want)[at]); yout.append(VD.bits(got)[at])
        with np.errstate(invalid="ignore"):
            stray = max(stray, float(np.nan_to_num(np.abs(got[~at].astype(np.float64)), nan=np.inf).max()))
    return np.concatenate(xin), np.concatenate(yout), stray


def exponent(b):
    """floor(log2 |x|) of float32 bit patterns (subnormals included)"""
    v = np.abs(b.view(F32).astype(np.float64))
    return np.floor(np.log2(v)).astype(int)


@pytest.mark.parametrize("cp", COPY_IDS)
def test_one_hot_contraction_copies_every_finite_binade(ctx, cp):
    """Weight 1 at the centre tap, zero elsewhere: the output is the input.  Every finite probe with 2^-100 <= |x| (mode 6: and
    |x| <= 0x7f7f0000, the largest value whose high plane is finite) must come out bit for bit.  Below 2^-100 the comment of
    fg_set_math in include/facegen_hip.h states what holds, and exactly that is asserted (VD.subnormal_rule):
      fp32 kernels (MFMA, thin, gemv): every subnormal operand is copied exactly, nothing is flushed;
      mode 6: the output is the sum of the three planes of the numpy specification, bit for bit -- exact from 2^-110 up, within 2^-134
        below (bf16 subnormal planes resolve 2^-133 and are honoured by the matrix pipe), zero below 2^-134;
      Winograd: exact from 2^-124 up, within 9 x 2^-150 below (the transformed taps are 1, 1/2, 1/4; the products round to the fp32
        subnormal grid), and an output that copies a zero may hold such a residue.
    Elsewhere every output that copies a zero is zero."""
    name, p = cp.rsplit("-", 1)
    c = VD.BY_NAME[name]
    xin, yout, stray = finite_probe_table(ctx, c, p)
    exact_to, abs_err = VD.subnormal_rule(c, p)
    assert exact_to <= VD.EXACT_MIN_EXP
    e = exponent(xin)
    assert set(range(-149, 128)) <= set(e.tolist()), "a binade got no probe"
    x, y = xin.view(F32).astype(np.float64), yout.view(F32).astype(np.float64)
    neq = xin != yout
    err = np.abs(y - x)
    print("value-domain probes %s: %d probes; exact from 2^%d up (stated: 2^%d); max |err| below: %.3e = 2^%.1f (stated %.3e); max relative error %.3e; "
          "%d outputs flushed to zero, the largest input among them 2^%d; residue where a zero is copied %.3e"
          % (cp, len(xin), int(max([-150] + e[neq].tolist())) + 1, exact_to, float(err.max()), np.log2(max(float(err.max()), 2.0 ** -200)), abs_err,
             float((err / np.abs(x)).max()), int((y == 0).sum()), int(max([-150] + e[y == 0].tolist())), stray))
    assert np.isfinite(y).all()
    bad = neq & (e >= exact_to)
    assert not bad.any(), "%s: %d probes at or above 2^%d differ; largest: in %08x out %08x" % (cp, int(bad.sum()), exact_to, xin[bad][np.argmax(e[bad])], yout[bad][np.argmax(e[bad])])
    assert (err <= abs_err).all(), "%s: |err| %.3e above the stated %.3e below 2^%d" % (cp, float(err.max()), abs_err, exact_to)
    assert stray <= (abs_err if p in c.wino else 0.0), "%s: an output that copies a zero holds %.3e" % (cp, stray)
    if VD.mode6(c, p):
        want = VD.bits(VD.split3_sum(xin.view(F32)))
        assert np.array_equal(want << 1 == 0, yout << 1 == 0) and np.array_equal(want[want << 1 != 0], yout[want << 1 != 0]), "%s: not the sum of the specification's planes" % cp


WGRAD_COPY_IDS = [c.name for c in VD.VCASES if "wgrad" in c.expect and "wgrad" not in c.wino]


@pytest.mark.parametrize("name", WGRAD_COPY_IDS)
def test_weight_gradient_copies_every_finite_binade(ctx, name):
    """The direct weight gradients (wgrad_kernel, wgrad_ws_kernel, wgrad_ws6_kernel, thin_wgrad_mfma_kernel, gemv_bwd_kernel) with x = 1
    at a single pixel (VD.wgrad_copy_operands): every weight gradient is one gradient value, and the float64 reference holds its bits.
    fp32 kernels: every finite probe bit for bit, subnormals included; mode 6: the sum of the specification's planes bit for bit (exact
    from 2^-110 up to 0x7f7f0000).  The Winograd weight gradient adds the four gradients of a tile before it multiplies and is left out."""
    c = VD.BY_NAME[name]
    m6 = VD.mode6(c, "wgrad")
    values = VD.finite_probes()
    if not m6:
        values = np.concatenate([values, np.array(VD.TOP_PROBES, dtype=U32), np.array(VD.TOP_PROBES, dtype=U32) | U32(0x80000000)])
    seen = []
    for x, gy in VD.wgrad_copy_operands(c, values):
        op = dict(x=x, gy=gy, w=None)
        want = VD.reference(c, dict(x=x, gy=gy, w=np.zeros(VD.shapes(c)["w"], F32)), ["wgrad"])["wgrad"]
        assert np.array_equal(want.astype(F32).astype(np.float64), want), "a sum with one nonzero term is a float32"
        want = want.astype(F32)
        got = device_passes(ctx, c, op, ["wgrad"])["wgrad"]
        if m6:
            want = VD.split3_sum(want)
        at = VD.bits(want) << 1 != 0
        bad = VD.bits(got)[at] != VD.bits(want)[at]
        assert not bad.any(), "%s wgrad: %d of %d differ; first: want %08x got %08x" % (name, int(bad.sum()), int(at.sum()), VD.bits(want)[at][bad][0], VD.bits(got)[at][bad][0])
        assert not got[~at].any(), "%s wgrad: a gradient that copies a zero is not zero" % name
        seen.append(np.unique(VD.bits(want)[at]))
    seen = np.unique(np.concatenate(seen))
    e = exponent(seen)
    assert set(range(-133 if m6 else -149, 128)) <= set(e.tolist()), "a binade got no probe"
    print("value-domain probes %s-wgrad: %d distinct probe values copied bit for bit%s" % (name, len(seen), " (as the sum of their three planes)" if m6 else ""))


DIRECT_COPY_IDS = ["%s-%s" % (c.name, p) for c in VD.VCASES for p in copy_passes(c) if p not in c.wino]


@pytest.mark.parametrize("cp", DIRECT_COPY_IDS)
def test_one_hot_contraction_with_three_plane_operands_keeps_all_six_products(ctx, cp):
    """The one-hot weight is 1 + 2^-10 + 2^-19 (planes 1, 2^-10, 2^-19) and the probes are that value times 2^e: the product is
    1 + 2^-9 [h m' + m h'] + 2^-18 [h l' + l h'] + 2^-20 [m m'] + 2^-28 [m l' + l m'] + 2^-38 [l l'].  The six products of mode 6 sum
    to 1 + 2^-9 + 2^-18 + 2^-20 exactly (21 bits: exact in fp32 in any order), and that is also the fp32 rounding of the true
    product, so every direct kernel must deliver it bit for bit in both modes -- and each of the six products has a bit of its own:
    one that is missing (or counted twice) shows, which the a-priori bound of part 2 cannot see for the smallest of them."""
    name, p = cp.rsplit("-", 1)
    c = VD.BY_NAME[name]
    x0, prod = F32(VD.THREE_PLANE), F32(VD.THREE_PLANE_PRODUCT)
    assert np.float64(x0) * np.float64(x0) - np.float64(prod) == 2.0 ** -28 + 2.0 ** -38
    opn, S = VD.probe_operand(c, p)
    shape = VD.shapes(c)[opn]
    slots = VD.probe_slots(shape, S, VD.observed_channels(c))
    exps = np.array([-60, -1, 0, 1, 60])[np.arange(len(slots)) % 5]
    vals = np.ldexp(np.where(np.arange(len(slots)) % 2, -x0, x0), exps).astype(F32)
    a, used, v = VD.probe_rounds(shape, slots, VD.bits(vals))[0]
    s = VD.shapes(c)
    w = (VD.onehot_weights(c, p) * x0).astype(F32)
    op = dict(x=a if opn == "x" else np.zeros(s["x"], F32), gy=a if opn == "gy" else np.zeros(s["gy"], F32), w=w)
    got = device_passes(ctx, c, op, [p])[p]
    want = VD.onehot_expected(c, p, (a.astype(np.float64) / np.float64(x0) * np.float64(prod)).astype(F32))
    at = want != 0
    assert at.sum() >= len(slots)
    bad = VD.bits(got)[at] != VD.bits(want)[at]
    if bad.any():
        g, t = np.float64(got[at][bad][0]), np.float64(want[at][bad][0])
        raise AssertionError("%s: %d of %d products differ; first: got %r, want %r: (got - want) / want = %+.3e = %+.3f x 2^-20"
                             % (cp, int(bad.sum()), int(at.sum()), g, t, (g - t) / t, (g - t) / t * 2.0 ** 20))
    assert not got[~at].any()


def edge_run(ctx, c, p):
    """the non-finite probes (and the two finite ones beyond the exact split) on a background of small normal noise -> per round
    (float64 IEEE reference of the one-hot pass, device output); in mode 6 the reference treats a magnitude above 0x7f7f0000 as NaN,
    as the header documents"""
    name, S = VD.probe_operand(c, p)
    shape = VD.shapes(c)[name]
    rng = np.random.default_rng(VD.seed(c, 3))
    noise = (1e-3 * rng.standard_normal(shape)).astype(F32)
    rounds = VD.probe_rounds(shape, VD.sparse_slots(shape, S, VD.observed_channels(c)), VD.edge_probes(), noise=noise)
    w = VD.onehot_weights(c, p)
    s = VD.shapes(c)
    out = []
    for (a, slots, vals), (_, got) in zip(rounds, run_probe_rounds(ctx, c, p, rounds)):
        ar = a.copy()
        if VD.mode6(c, p):
            ar.reshape(-1)[(VD.bits(ar).reshape(-1) & 0x7fffffff) > VD.SPLIT_MAX] = np.nan
        op = dict(x=ar if name == "x" else np.zeros(s["x"], F32), gy=ar if name == "gy" else np.zeros(s["gy"], F32), w=w)
        folded = c.kind == "conv" and c.shape[6]        # a folded up-convolution has no product of a zero tap with a copy of the pixel
        with np.errstate(invalid="ignore"):
            out.append(((VD.reference_folded if folded else VD.reference)(c, op, [p])[p], got))
    return out


@pytest.mark.parametrize("cp", COPY_IDS)
def test_non_finite_operands_are_never_swallowed(ctx, cp):
    """+-inf, six NaN encodings (among them 0x7fffffff, 0xffffffff and 0x7fff8000, which the unguarded bf16 rounding wrapped to +-0),
    0x7f7f8000 and 0x7f7fffff against the float64 IEEE reference (inf * 0 = NaN in the other channels of the pixel):
    no finite output where the reference is not finite, anywhere; fp32 direct kernels: the same class (NaN, +inf, -inf) at every output
    and nothing else non-finite; mode 6 and Winograd: NaN or the reference's infinity, and nothing non-finite outside the reference's
    set dilated by one Winograd tile (mode 6 direct kernels: the exact set)."""
    name, p = cp.rsplit("-", 1)
    c = VD.BY_NAME[name]
    wino, m6 = p in c.wino, VD.mode6(c, p)
    runs = edge_run(ctx, c, p)
    assert sum(int((~np.isfinite(ref)).any()) for ref, _ in runs) >= 1
    for ref, got in runs:
        rn, gn = ~np.isfinite(ref), ~np.isfinite(got)
        swallowed = rn & ~gn
        assert not swallowed.any(), "%s: %d outputs are finite where the reference is not; first at %s: got %r, reference %r" % (
            cp, int(swallowed.sum()), np.argwhere(swallowed)[0], got[swallowed][0], ref[swallowed][0])
        extra = gn & ~VD.dilate(rn, 2 if wino else 0)
        assert not extra.any(), "%s: %d non-finite outputs outside the reference's set; first at %s" % (cp, int(extra.sum()), np.argwhere(extra)[0])
        if wino or m6:
            ok = np.isnan(got[rn]) | (got[rn] == ref[rn])
            assert ok.all(), "%s: neither NaN nor the reference's infinity" % cp
        else:
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == np.inf, ref == np.inf) and np.array_equal(got == -np.inf, ref == -np.inf), \
                "%s: the class of a non-finite output differs from the reference's" % cp


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. BatchNorm statistics at the edges
# ---------------------------------------------------------------------------------------------------------------------------------
import test_gpu_pointwise_paths as TQ
from gpu_util import BAR, close

RUNS = ((0.25, 0), (None, 1))       # (PReLU slope, accumulate) as run_bn


def adopt_branches(what, got, op, slope, acc, margin):
    """the reference with the device's PReLU decisions (test_batchnorm_large_offset's procedure): a decision that differs from the
    reference's own must lie within `margin` of the kink"""
    r = TQ.bn_reference(op, slope, acc)
    if slope is None:
        return r
    pos = got["y"].cpu().numpy() > 0
    flips = pos != (r["z"] > 0)
    assert (np.abs(r["z"])[flips] <= np.broadcast_to(margin, flips.shape)[flips]).all(), "%s: a branch decision far from the kink differs" % what
    assert flips.sum() <= 0.01 * flips.size
    return TQ.bn_reference(op, slope, acc, pos=pos)


@pytest.mark.parametrize("C", VD.BN_LADDERS)
@pytest.mark.parametrize("k", VD.BN_PIVOTS)
def test_batchnorm_pivot_far_from_the_mean(ctx, C, k):
    """Row 0 -- the pivot of the shifted sums -- k standard deviations from the mean: S2 carries (1 + k^2) times the mass and the
    variance comes from a cancellation done in float64.  Bars: bn_check's, plus the first-order effect of r fp32 additions per partial
    on that mass (VD.bn_pivot_bars; r = 18 for the column kernels, 64 for the float4 kernels at 4096 rows)."""
    M = 4096
    op = VD.bn_outlier_operands(M, C, k)
    t, dm, r = VD.bn_pivot_terms(op)
    print("bn pivot C=%d k=%d: r = %d, inflation %.1f .. %.1f, variance term %.3e, mean term %.3e" % (C, k, r, float((t / VD.U / r).min()), float((t / VD.U / r).max()), float(t.max()), float(dm.max())))
    for slope, acc in RUNS:
        del TQ.KEEP[:]
        got = TQ.bn_device(ctx, op, slope, acc)
        r0 = TQ.bn_reference(op, slope, acc)
        ref = adopt_branches("bn pivot", got, op, slope, acc, VD.bn_pivot_bars(op, r0, slope)["y"] + BAR["bn_y"])
        extra = VD.bn_pivot_bars(op, ref, slope)
        for key in ("mean", "invstd"):
            e = np.abs(got[key].cpu().numpy().astype(np.float64) - ref[key])
            print("bn pivot C=%d k=%d %s: max |err| / derived term = %.3f" % (C, k, key, float((e / extra[key]).max())))
        TQ.bn_check("bn pivot C=%d k=%d slope %s acc %d" % (C, k, slope, acc), got, ref, extra=extra)


@pytest.mark.parametrize("C", VD.BN_LADDERS)
@pytest.mark.parametrize("M", (2, 4096))
def test_batchnorm_constant_channels(ctx, M, C):
    """every fourth channel constant (0, 1000, -3.25): the deviations from the pivot are exactly zero, so mean is the constant, the
    variance exactly 0 (not a rounding residue cut off by the `var < 0` clamp), invstd = 1 / sqrt(eps) to fp32 rounding, y = PReLU(beta)
    exactly, no NaN; gx against float64 per channel at the existing bar, which scales with max |gx| of the channel, i.e. with invstd"""
    op, const = VD.bn_constant_operands(M, C)
    cc = sorted(const)
    for slope, acc in RUNS:
        del TQ.KEEP[:]
        got = TQ.bn_device(ctx, op, slope, acc)
        ref = TQ.bn_reference(op, slope, acc)
        # a channel at 1000 stores its mean, running mean and evaluate output at that magnitude: offset_bars' fp32 format terms for those
        # three (the terms for y, gx and ggamma are NOT taken: the mean of a constant channel is exact, and so is y, below)
        fmt = TQ.offset_bars(op, ref, slope)
        TQ.bn_check("bn constant %dx%d slope %s acc %d" % (M, C, slope, acc), got, ref, extra={key: fmt[key] for key in ("mean", "rm", "ye")})
        mean, inv, y, gx = (got[key].cpu().numpy() for key in ("mean", "invstd", "y", "gx"))
        assert np.array_equal(mean[cc], np.array([const[c] for c in cc], F32))
        want = 1.0 / np.sqrt(np.float64(F32(TQ.BN_EPS)))
        assert (np.abs(inv[cc].astype(np.float64) - want) <= 2 * VD.U * want).all(), inv[cc]
        beta = op["beta"][cc]
        assert np.array_equal(y[:, cc], np.broadcast_to(np.where(beta > 0, beta, F32(1.0 if slope is None else slope) * beta), (M, len(cc))))
        for c in cc:
            close(gx[:, c], ref["gx"][:, c], atol=BAR["bn_gx"] * max(1.0, float(np.abs(ref["gx"][:, c]).max())), what="bn constant gx channel %d" % c)
            assert np.abs(ref["gx"][:, c]).max() > 10 or M == 2, "the channel's gradient carries invstd"


@pytest.mark.parametrize("C", VD.BN_LADDERS)
@pytest.mark.parametrize("M", (1, 2))
def test_batchnorm_one_and_two_rows(ctx, M, C):
    """the unbiased running variance divides by max(M - 1, 1): at M = 1 the variance is 0 and the guard keeps it 0 (not 0 / 0)"""
    op = TQ.bn_operands(M, C, TQ.Src(31 + M + C))
    for slope, acc in RUNS:
        del TQ.KEEP[:]
        got = TQ.bn_device(ctx, op, slope, acc)
        ref = TQ.bn_reference(op, slope, acc)
        TQ.bn_check("bn %dx%d slope %s acc %d" % (M, C, slope, acc), got, ref)
        if M == 1:
            assert np.array_equal(got["mean"].cpu().numpy(), op["x"][0])
            close(got["rv"].cpu().numpy(), (1 - TQ.BN_MOM) * op["rv"].astype(np.float64), atol=0, rtol=BAR["bn_running_var_rtol"], what="running variance at M = 1")


@pytest.mark.parametrize("C", VD.BN_LADDERS)
def test_batchnorm_below_the_overflow_of_the_squared_deviation(ctx, C):
    """include/facegen_hip.h (fg_batchnorm_forward): the fp32 square of x - pivot overflows above 1.8e19.  One probe below it: the
    operands of bn_operands scaled by 2^56 (max |x - pivot| about 6e17, its square 2^118, a block's partial of 64 such squares finite).
    Every output finite and inside bn_check's bars, the quantities that scale with the data (mean, running mean, evaluate output: by
    2^56; gx: by 2^-56) compared after scaling back."""
    M, s = 4096, 2.0 ** 56
    op = TQ.bn_operands(M, C, TQ.Src(56 + C))
    op["x"] = np.ldexp(op["x"], 56)
    d = np.abs(op["x"].astype(np.float64) - op["x"][0].astype(np.float64)).max()
    print("bn 2^56 C=%d: max |x - pivot| = %.3e = 2^%.2f" % (C, d, np.log2(d)))
    assert VD.BN_D2_OVERFLOW / 64 < d < VD.BN_D2_OVERFLOW and np.float32(d) * np.float32(d) < np.inf
    with np.errstate(over="ignore"):
        assert np.float32(2e19) * np.float32(2e19) == np.inf and np.float32(VD.BN_D2_OVERFLOW) ** 2 < np.inf
    scale = dict(mean=1 / s, rm=1 / s, ye=1 / s, gx=s)
    for slope, acc in RUNS:
        del TQ.KEEP[:]
        got = TQ.bn_device(ctx, op, slope, acc)
        for key, v in got.items():
            assert v is None or bool(torch.isfinite(v).all()), key
        ref = adopt_branches("bn 2^56", got, op, slope, acc, BAR["bn_y"])
        got = {key: (v * scale[key] if (v is not None and key in scale) else v) for key, v in got.items()}
        ref = {key: (v * scale[key] if key in scale else v) for key, v in ref.items()}
        TQ.bn_check("bn 2^56 C=%d slope %s acc %d" % (C, slope, acc), got, ref)


def sync_bn_run(ctx, op, replicas):
    """a one-layer BatchNorm net on [M][C] rows (16 x 16 maps) driven through the sync-BN protocol by `replicas` nets in lock-step, each
    on its share of the rows -> the outputs of bn_device that a net exposes"""
    from face_generator_amd.runtime import DeviceNet
    from test_gpu_syncbn import lockstep
    M, C = op["x"].shape
    B = M // 256 // replicas
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(ctx.device)
    nets = []
    for r in range(replicas):
        dn = DeviceNet(ctx, [("BATCHNORM", C)], (C, 16, 16), B)
        wo, wn, bo, bn = dn.param_offsets(0)
        assert wn == C and bn == C
        dn.params[wo:wo + C] = put(op["gamma"]); dn.params[bo:bo + C] = put(op["beta"])
        dn.buffers[:C] = put(op["rm"]); dn.buffers[C:2 * C] = put(op["rv"])
        dn.params_changed()
        dn.enable_sync_bn(None)
        nets.append(dn)
    rows = M // replicas
    xs = [put(op["x"][r * rows:(r + 1) * rows]).view(B, 16, 16, C) for r in range(replicas)]
    gys = [put(op["gy"][r * rows:(r + 1) * rows]).view(B, 16, 16, C) for r in range(replicas)]
    lockstep([dn.forward_steps(x, train=True) for dn, x in zip(nets, xs)])
    y = torch.cat([dn._output_view().reshape(rows, C).clone() for dn in nets])
    gxs = [ctx.empty(B, 16, 16, C) for _ in nets]
    rcs = [dn._backward_call(gy, True, gx) for dn, gy, gx in zip(nets, gys, gxs)]
    while any(rc == 1 for rc in rcs):
        assert all(rc == 1 for rc in rcs), "replicas must pause at the same BatchNorm"
        bufs = [dn._sync_slice() for dn in nets]
        total = torch.stack(bufs).sum(0)
        for b in bufs:
            b.copy_(total)
        rcs = [dn.lib.fg_net_backward_resume(dn.h) for dn in nets]
    for rc in rcs:
        ctx.check(rc)
    wo, wn, bo, bn = nets[0].param_offsets(0)
    grads = sum(dn.grads.double() for dn in nets).float()
    for dn in nets[1:]:
        assert torch.equal(dn.buffers, nets[0].buffers), "every replica holds the global running statistics"
    return dict(y=y, ye=None, mean=None, invstd=None, rm=nets[0].buffers[:C], rv=nets[0].buffers[C:2 * C], gx=torch.cat([g.reshape(rows, C) for g in gxs]),
                gg=grads[wo:wo + C], gb=grads[bo:bo + C], gs=None)


@pytest.mark.parametrize("replicas", (1, 2))
def test_sync_batchnorm_at_a_large_offset(ctx, replicas):
    """x = 1000 + 0.05 N(0, 1) through bn_sync_local_kernel / bn_sync_global_kernel: the shifted partial sums are un-shifted to raw
    sum x and sum x^2 in float64 and the variance is E[x^2] - mean^2 in float64, which loses mean^2 / var 2^-53 = 4e-8 relative here --
    inside bn_invstd_rtol.  One replica, and two half-batch replicas in lock-step, against bn_reference at the bars of
    test_batchnorm_large_offset (offset_bars)."""
    M, C = 4096, 64
    op = TQ.bn_operands(M, C, TQ.Src(4160), offset=1000.0)
    ref = TQ.bn_reference(op, None, 0)
    x = op["x"].astype(np.float64)
    assert 2e-8 < (x.mean(0) ** 2 / x.var(0)).max() * 2.0 ** -53 < BAR["bn_invstd_rtol"] / 10
    got = sync_bn_run(ctx, op, replicas)
    # the running variance reads the un-shifted variance: its relative error is that of the variance, bounded by the bar of invstd x 2
    rv_new = (got["rv"].cpu().numpy().astype(np.float64) - (1 - TQ.BN_MOM) * op["rv"]) / TQ.BN_MOM
    var_err = np.abs(rv_new * (M - 1) / M / x.var(0) - 1)
    print("sync bn offset, %d replica(s): max relative error of the variance behind the running variance %.3e" % (replicas, float(var_err.max())))
    TQ.bn_check("sync bn offset, %d replica(s)" % replicas, got, ref, extra=TQ.offset_bars(op, ref, None))

