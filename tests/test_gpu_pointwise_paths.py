"""Module-level parity for the pointwise, BatchNorm, optimizer and RNG entries at the sizes and options where their launchers take
another path (tests/DISPATCH_COVERAGE.md, "Capped launchers"): above the grid cap of every capped launcher that a module-level
entry of include/facegen_hip.h reaches, the scalar BatchNorm reductions, the optimizer options nothing else sets, and Philox4x32-10
against an independent numpy implementation.

References are plain float64 numpy (for the optimizers: oracle.interruptable_adam / _sgd / _adagrad on float64 vectors).  Bars are
gpu_util.BAR's; where an entry has none the bar is written next to the case with its reason.

CAP_CASES, BN_CASES, OPT_CASES and RNG_CASES are module-level data: tests/dispatch_audit.py replays them in the planning-only context
(run_*(ctx, case, dry=True): the same calls on host tensors, no reference) and the census derives `operator` from what they launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import close, BAR

pytestmark = pytest.mark.gpu

F32 = np.float32
GRID_CAP = 4096 * 256
N1 = GRID_CAP + 259                 # scalar elementwise kernels: one trip of 4096 x 256 and a ragged second one
N4 = 4 * N1                         # kernels that work in float4s
U = 2.0 ** -24                      # unit roundoff of fp32


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


class Src:
    """seeded operands; dry: zeros of the same shapes (planning-only replay: nobody reads them)"""
    def __init__(self, seed, dry=False):
        self.rng, self.dry = np.random.default_rng(seed), dry

    def normal(self, *shape, scale=1.0):
        return np.zeros(shape, F32) if self.dry else (self.rng.standard_normal(shape, dtype=F32) * F32(scale))

    def keep(self, *shape, p=0.8):
        return np.zeros(shape, F32) if self.dry else (self.rng.random(shape, dtype=F32) < p).astype(F32)


KEEP = []                           # every operand of the running case: a temporary freed inside an argument list may be handed out again
                                    # by the caching allocator for the next argument of the same call


def hold(t):
    KEEP.append(t)
    return t


def put(ctx, a):
    return hold(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(ctx.device))


def out(ctx, *shape):
    return hold(torch.full(shape, float("nan"), dtype=torch.float32, device=ctx.device))      # an element nobody writes stays NaN


def P(t):
    return t.data_ptr() if t is not None else None


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[P(t) for t in ts])


def d64(a):
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# capped launchers above their cap.  A case: f(ctx, S) -> [(what, device result, lambda: float64 reference, atol, rtol)]
# ---------------------------------------------------------------------------------------------------------------------------------
def c_fill_axpby(ctx, S):
    lib, h = ctx.lib, ctx.h
    o = out(ctx, N1)
    ctx.check(lib.fg_fill(h, P(o), 1.5, N1))
    x, y = S.normal(N1), S.normal(N1)
    yd = put(ctx, y)
    ctx.check(lib.fg_axpby(h, 0.75, P(put(ctx, x)), -1.25, P(yd), N1))
    # two products and a sum, each rounded once (or contracted): 3 u (|a x| + |b y|)
    tol = lambda: 3 * U * (0.75 * np.abs(d64(x)) + 1.25 * np.abs(d64(y)))
    return [("fill", o, lambda: np.full(N1, 1.5), 0, 0), ("axpby", yd, lambda: 0.75 * d64(x) - 1.25 * d64(y), tol, 0)]


def c_layout(ctx, S):
    n, c, hh, ww = 3, 5, 263, 267                   # 1 053 315 elements
    x = S.normal(n, c, hh, ww)
    a, b = out(ctx, n, hh, ww, c), out(ctx, n, c, hh, ww)
    ctx.check(ctx.lib.fg_nchw_to_nhwc(ctx.h, P(put(ctx, x)), P(a), n, c, hh, ww))
    ctx.check(ctx.lib.fg_nhwc_to_nchw(ctx.h, P(a), P(b), n, c, hh, ww))
    return [("nchw_to_nhwc", a, lambda: x.transpose(0, 2, 3, 1), 0, 0), ("nhwc_to_nchw", b, lambda: x, 0, 0)]


def c_prelu(ctx, S):
    lib, h = ctx.lib, ctx.h
    x, gy, m = S.normal(N1), S.normal(N1), S.keep(N1, p=0.5)
    xd, md, sl = put(ctx, x), put(ctx, m), put(ctx, np.array([0.25], F32))
    y, gx, gs = out(ctx, N1), out(ctx, N1), out(ctx, 1)
    ctx.check(lib.fg_prelu_forward(h, P(xd), P(sl), P(md), 2.0, P(y), N1))
    ctx.check(lib.fg_prelu_backward(h, P(xd), P(put(ctx, gy)), P(sl), P(md), 2.0, P(gx), P(gs), 0.0, N1, P(out(ctx, 1024))))
    d = lambda: np.where(x > 0, 1.0, 0.25) * d64(m) * 2.0
    ref_gs = lambda: np.array([(d64(gy) * d64(m) * 2.0 * np.where(x > 0, 0.0, d64(x))).sum()])
    return [("prelu fwd", y, lambda: d64(x) * d(), BAR["prelu"], 0), ("prelu gx", gx, lambda: d64(gy) * d(), BAR["prelu"], 0),
            ("prelu gslope", gs, ref_gs, BAR["slope_grad"], 0)]


POOL = (3, 296, 296, 64)            # NHWC; the pooled map has 1 051 392 float4s
SMALL = (3, 70, 66, 77)             # 1 067 220 elements; its 2x map (3, 140, 132, 77) has 4 268 880


def up2(a):
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)


def pool_mean(a):
    B, H, W, C = a.shape
    return a.reshape(B, H // 2, 2, W // 2, 2, C).mean((2, 4))


def c_actpool(ctx, S):
    lib, h = ctx.lib, ctx.h
    B, H, W, C = POOL
    x, gy, m = S.normal(B, H, W, C), S.normal(B, H // 2, W // 2, C), S.keep(B, C)
    xd, md, sl = put(ctx, x), put(ctx, m), put(ctx, np.array([-0.1], F32))
    y, gx, gs = out(ctx, B, H // 2, W // 2, C), out(ctx, B, H, W, C), out(ctx, 1)
    ctx.check(lib.fg_actpool_forward(h, P(xd), P(sl), P(md), 1.25, P(y), B, H, W, C))
    ctx.check(lib.fg_actpool_backward(h, P(xd), P(put(ctx, gy)), P(sl), P(md), 1.25, P(gx), P(gs), 0.0, B, H, W, C, P(out(ctx, 1024))))
    a = np.float64(F32(-0.1))
    mm = lambda: d64(m)[:, None, None, :] * 1.25
    g = lambda: up2(d64(gy)) * 0.25 * mm()
    ref_gs = lambda: np.array([(g() * np.where(x > 0, 0.0, d64(x))).sum()])
    return [("actpool fwd", y, lambda: pool_mean(np.where(x > 0, d64(x), a * d64(x)) * mm()), BAR["prelu"], 0),
            ("actpool gx", gx, lambda: g() * np.where(x > 0, 1.0, a), BAR["prelu"], 0),
            ("actpool gslope", gs, ref_gs, BAR["slope_grad"], 0)]


def c_maxpool(ctx, S):
    lib, h = ctx.lib, ctx.h
    B, H, W, C = POOL
    x, gy = S.normal(B, H, W, C), S.normal(B, H // 2, W // 2, C)
    xd = put(ctx, x)
    y, gx = out(ctx, B, H // 2, W // 2, C), out(ctx, B, H, W, C)
    ctx.check(lib.fg_maxpool2x2_forward(h, P(xd), P(y), B, H, W, C))
    ctx.check(lib.fg_maxpool2x2_backward(h, P(xd), P(put(ctx, gy)), P(gx), B, H, W, C))
    win = lambda: x.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)

    def ref_gx():
        am = win().argmax(-1)                       # first maximum in scan order (dy, dx)
        g = np.zeros((B, H // 2, W // 2, C, 4))
        np.put_along_axis(g, am[..., None], d64(gy)[..., None], -1)
        return g.reshape(B, H // 2, W // 2, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, H, W, C)
    return [("maxpool fwd", y, lambda: win().max(-1), 0, 0), ("maxpool gx", gx, ref_gx, 0, 0)]      # copies: exact


def c_avgpool_upsample(ctx, S):
    lib, h = ctx.lib, ctx.h
    B, H, W, C = SMALL
    small, big = S.normal(B, H, W, C), S.normal(B, 2 * H, 2 * W, C)
    sd, bd = put(ctx, small), put(ctx, big)
    ap, apg, us, usg = out(ctx, B, H, W, C), out(ctx, B, 2 * H, 2 * W, C), out(ctx, B, 2 * H, 2 * W, C), out(ctx, B, H, W, C)
    ctx.check(lib.fg_avgpool2x2_forward(h, P(bd), P(ap), B, 2 * H, 2 * W, C))
    ctx.check(lib.fg_avgpool2x2_backward(h, P(sd), P(apg), B, 2 * H, 2 * W, C))
    ctx.check(lib.fg_upsample_nearest2x_forward(h, P(sd), P(us), B, H, W, C))
    ctx.check(lib.fg_upsample_nearest2x_backward(h, P(bd), P(usg), B, H, W, C))
    return [("avgpool fwd", ap, lambda: pool_mean(d64(big)), BAR["avgpool_fwd"], 0),
            ("avgpool bwd", apg, lambda: up2(d64(small)) * 0.25, BAR["avgpool_bwd"], 0),
            ("upsample fwd", us, lambda: up2(d64(small)), BAR["upsample_fwd"], 0),
            ("upsample bwd", usg, lambda: pool_mean(d64(big)) * 4.0, BAR["upsample_bwd"], 0)]


def c_spatial_dropout_view(ctx, S):
    lib, h = ctx.lib, ctx.h
    B, HW, C = 3, 4099, 86                          # 1 057 542 elements
    x, m = S.normal(B, HW, C), S.keep(B, C)
    y = out(ctx, B, HW, C)
    ctx.check(lib.fg_spatial_dropout_apply(h, P(put(ctx, x)), P(put(ctx, m)), 1.25, P(y), B, HW, C))
    b, hh, ww, nout, f = 3, 99, 99, 4, 3            # 1 058 508 elements
    c = nout * f * f
    v = S.normal(b, c, hh, ww)                      # the convolution's NCHW output
    vd = put(ctx, v.transpose(0, 2, 3, 1))
    u, back = out(ctx, b, hh * f, ww * f, nout), out(ctx, b, hh, ww, c)
    ctx.check(lib.fg_conv_upsample_view_forward(h, P(vd), P(u), b, hh, ww, c, f))
    ctx.check(lib.fg_conv_upsample_view_backward(h, P(u), P(back), b, hh, ww, c, f))
    # one product by 0 / 1 and one by 1.25: 1e-6, the bar test_gpu_memory_contract.py holds this entry to
    return [("spatial dropout", y, lambda: d64(x) * d64(m)[:, None, :] * 1.25, 1e-6, 0),
            ("view fwd", u, lambda: v.reshape(b, nout, hh * f, ww * f).transpose(0, 2, 3, 1), 0, 0),
            ("view bwd", back, lambda: v.transpose(0, 2, 3, 1), 0, 0)]


def c_sigmoid_leakyrelu(ctx, S):
    lib, h = ctx.lib, ctx.h
    x, gy = S.normal(N1, scale=3.0), S.normal(N1)
    xd, gd = put(ctx, x), put(ctx, gy)
    y, gx, yl, gl = out(ctx, N1), out(ctx, N1), out(ctx, N1), out(ctx, N1)
    ys = (1.0 / (1.0 + np.exp(-d64(x)))).astype(F32)
    ctx.check(lib.fg_sigmoid_forward(h, P(xd), P(y), N1))
    ctx.check(lib.fg_sigmoid_backward(h, P(put(ctx, ys)), P(gd), P(gx), N1))
    ctx.check(lib.fg_leakyrelu_forward(h, P(xd), 0.333, P(yl), N1))
    ctx.check(lib.fg_leakyrelu_backward(h, P(xd), P(gd), 0.333, P(gl), N1))
    s = np.float64(F32(0.333))
    return [("sigmoid fwd", y, lambda: 1.0 / (1.0 + np.exp(-d64(x))), BAR["sigmoid"], 0),
            ("sigmoid bwd", gx, lambda: d64(gy) * d64(ys) * (1.0 - d64(ys)), BAR["sigmoid"], 0),
            ("leakyrelu fwd", yl, lambda: np.where(x > 0, d64(x), s * d64(x)), BAR["leakyrelu"], 0),
            ("leakyrelu bwd", gl, lambda: np.where(x > 0, d64(gy), s * d64(gy)), BAR["leakyrelu"], 0)]


def c_dropout_concat_add(ctx, S):
    lib, h = ctx.lib, ctx.h
    x, m, b = S.normal(N1), S.keep(N1, p=0.5), S.normal(N1)
    xd, bd = put(ctx, x), put(ctx, b)
    y, s = out(ctx, N1), out(ctx, N1)
    ctx.check(lib.fg_dropout_apply(h, P(xd), P(put(ctx, m)), 2.0, P(y), N1))
    ctx.check(lib.fg_add(h, P(xd), P(bd), P(s), N1))
    npix, ca, cb = 116537, 4, 5                     # 1 048 833 elements
    a2, b2 = S.normal(npix, ca), S.normal(npix, cb)
    j, ga, gb = out(ctx, npix, ca + cb), out(ctx, npix, ca), out(ctx, npix, cb)
    ctx.check(lib.fg_concat_channels(h, P(put(ctx, a2)), P(put(ctx, b2)), P(j), npix, ca, cb))
    ctx.check(lib.fg_split_channels(h, P(j), P(ga), P(gb), npix, ca, cb))
    return [("dropout", y, lambda: d64(x) * d64(m) * 2.0, 0, 0), ("add", s, lambda: d64(x) + d64(b), lambda: U * np.abs(d64(x) + d64(b)), 0),
            ("concat", j, lambda: np.concatenate([a2, b2], 1), 0, 0), ("split a", ga, lambda: a2, 0, 0), ("split b", gb, lambda: b2, 0, 0)]


def c_rows_sum(ctx, S):
    lib, h = ctx.lib, ctx.h
    rows = 32768 + 37                               # launch_rows caps gridDim.y at 32768 rows
    res = []
    for widths in ((4, 8), (3, 5)):                 # 16-byte form, scalar form
        parts = [S.normal(rows, w) for w in widths]
        wd = (ctypes.c_int * len(widths))(*widths)
        j = out(ctx, rows, sum(widths))
        back = [out(ctx, rows, w) for w in widths]
        ctx.check(lib.fg_join_rows(h, ptrs([put(ctx, p) for p in parts]), wd, len(widths), P(j), rows))
        ctx.check(lib.fg_split_rows(h, P(j), ptrs(back), wd, len(widths), rows))
        res.append(("join %s" % (widths,), j, lambda parts=parts: np.concatenate(parts, 1), 0, 0))
        res += [("split %s part %d" % (widths, k), b, lambda p=p: p, 0, 0) for k, (b, p) in enumerate(zip(back, parts))]
    for count in (N4, N1):                          # sum_parts_kernel<4>, <1> (N1 is odd)
        ps = [S.normal(count) for _ in range(3)]
        o = out(ctx, count)
        ctx.check(lib.fg_sum_n(h, ptrs([put(ctx, p) for p in ps]), 3, P(o), count))
        res.append(("sum_n %d" % count, o, lambda ps=ps: ((ps[0] + ps[1]).astype(F32) + ps[2]).astype(F32), 0, 0))     # fp32 sums in this order
    return res


def c_scale_bilinear(ctx, S):
    from oracle import image_scale as IS
    n, c, hs, ws, hd, wd = 2, 3, 211, 199, 419, 419  # 1 053 366 outputs, a 2x-odd upscale
    x = S.normal(n, c, hs, ws)
    o = out(ctx, n, c, hd, wd)
    ctx.check(ctx.lib.fg_scale_bilinear(ctx.h, P(put(ctx, x)), P(o), n, c, hs, ws, hd, wd, 1))
    return [("scale_bilinear nchw", o, lambda: np.stack([IS.scale(img, wd, hd) for img in x]), 0, 0)]       # bit for bit, as test_gpu_image_scale.py


def penalty(p, g, gscale, l1, l2, clamp):
    gg = gscale * g + l1 * np.sign(p) + l2 * p
    return np.clip(gg, -clamp, clamp) if clamp else gg


def c_optimizers(ctx, S):
    """one step each at N4 + 3 (Adam: quads and a tail of 3) / N1 elements, bars of test_fused_adam_sgd_adagrad_match_reference_formulas"""
    lib, h = ctx.lib, ctx.h
    n = N4 + 3
    p, g = S.normal(n), S.normal(n)
    pd, md, vd = put(ctx, p), put(ctx, np.zeros(n, F32)), put(ctx, np.zeros(n, F32))
    ctx.check(lib.fg_adam_fused(h, P(pd), P(put(ctx, g)), P(md), P(vd), n, 1.0, 0.0, 1e-4, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1, None))

    @functools.lru_cache(None)
    def adam():
        pr, st = d64(p).copy(), {}
        O.interruptable_adam(lambda x: (0.0, penalty(x, d64(g), 1.0, 0.0, np.float64(F32(1e-4)), 1.0)), pr, {}, st)
        return pr, st
    res = [("adam p", pd, lambda: adam()[0], 2e-7, 2e-7), ("adam m", md, lambda: adam()[1]["m"], 1e-7, 1e-5), ("adam v", vd, lambda: adam()[1]["v"], 1e-12, 1e-5)]
    p1, g1 = p[:N1], g[:N1]
    ps, mom = put(ctx, p1), put(ctx, np.zeros(N1, F32))
    ctx.check(lib.fg_sgd_fused(h, P(ps), P(put(ctx, g1)), P(mom), N1, 1.0, 0.0, 0.0, 0.0, 0.02, 0.9, 0.9, 0.0, 0, 1))

    def sgd():
        pr = d64(p1).copy()
        O.interruptable_sgd(lambda x: (0.0, d64(g1)), pr, dict(learningRate=0.02, momentum=0.9), {})
        return pr
    pa, var = put(ctx, p1), put(ctx, np.zeros(N1, F32))
    ctx.check(lib.fg_adagrad_fused(h, P(pa), P(put(ctx, g1)), P(var), N1, 1.0, 0.0, 0.0, 0.0, 1e-3))

    def adagrad():
        pr = d64(p1).copy()
        O.interruptable_adagrad(lambda x: (0.0, d64(g1)), pr, {}, {})
        return pr
    o2 = out(ctx, 2)
    ctx.check(lib.fg_norms(h, P(put(ctx, p1)), N1, P(o2), P(out(ctx, 1024))))       # capped at 512 blocks
    return res + [("sgd p", ps, sgd, 1e-5, 0), ("adagrad p", pa, adagrad, 1e-6, 0),
                  ("norms", o2, lambda: np.array([np.abs(d64(p1)).sum(), (d64(p1) ** 2).sum()]), 0, BAR["norms_rtol"])]


def c_rng(ctx, S):
    n = N4 + 1                                      # 1 048 836 quads, the last one ragged
    o = out(ctx, n)
    ctx.check(ctx.lib.fg_rng_uniform(ctx.h, 77, 5, P(o), n, 0.0, 1.0))
    return [("rng uniform", o, lambda: ((philox_words(77, 5, (n + 3) // 4).reshape(-1)[:n] >> 8).astype(np.float64) * U), 0, 0)]      # bit for bit


CAP_CASES = [("fill-axpby", c_fill_axpby), ("layout", c_layout), ("prelu", c_prelu), ("actpool", c_actpool), ("maxpool", c_maxpool),
             ("avgpool-upsample", c_avgpool_upsample), ("spatial-dropout-view", c_spatial_dropout_view), ("sigmoid-leakyrelu", c_sigmoid_leakyrelu),
             ("dropout-concat-add", c_dropout_concat_add), ("rows-sum", c_rows_sum), ("scale-bilinear", c_scale_bilinear),
             ("optimizers", c_optimizers), ("rng", c_rng)]


def compare(results):
    for what, got, ref, atol, rtol in results:
        r = d64(ref())
        a = atol() if callable(atol) else atol
        g = got.cpu().numpy()
        assert not np.isnan(g).any(), "%s: %d of %d elements NaN (never written), first at %s" % (what, int(np.isnan(g).sum()), g.size, np.argwhere(np.isnan(g))[0])
        print("%s: max|err| %.3e (max|ref| %.3e)" % (what, float(np.abs(g.reshape(r.shape) - r).max()), float(np.abs(r).max())))
        close(g.reshape(r.shape), r, atol=a, rtol=rtol, what=what)


def run_cap(ctx, case, dry=False):
    del KEEP[:]
    return case[1](ctx, Src(len(case[0]) * 131 + 7, dry))


@pytest.mark.parametrize("case", CAP_CASES, ids=[c[0] for c in CAP_CASES])
def test_capped_launcher_above_its_cap(ctx, case):
    compare(run_cap(ctx, case))


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm ladders
# ---------------------------------------------------------------------------------------------------------------------------------
# (rows M, C)
BN_CASES = [(3, 12),                # fewer rows than the four row lanes; bn_apply_blocks unit 3
            (64 * 256 + 37, 96),    # cr_rowblocks at its cap with a ragged last block; two column blocks, the second half full
            (70, 2048),             # above cr4_ok's 1024: 32 column blocks
            (5000, 4),              # float4 corner: 1024 row lanes
            (130, 1024),            # float4 corner: 4 row lanes
            (2, 8),                 # float4 corner: smallest M with a defined unbiased variance
            (349600, 12),           # bn_apply above its 4096-block cap with unit 3
            (64 * 256 + 37, 8)]     # the float4 reductions above the row-block cap (rows_per = 65)
BN_EPS, BN_MOM = 1e-5, 0.1


def bn_operands(M, C, S, offset=None):
    x = S.normal(M, C, scale=1.7) + F32(0.9) if offset is None else (F32(offset) + F32(0.05) * S.normal(M, C))
    return dict(x=x.astype(F32), gy=S.normal(M, C), gamma=(1.0 + 0.3 * S.normal(C)).astype(F32), beta=S.normal(C, scale=0.3),
                rm=S.normal(C, scale=0.1), rv=(1.0 + 0.2 * np.abs(S.normal(C))).astype(F32), acc=S.normal(2 * C + 1))


def bn_reference(op, slope, acc, mean=None, pos=None):
    """float64 SpatialBatchNormalization [+ PReLU] on [M][C]: train outputs, statistics, gradients, evaluate output.
    mean: statistics override (the large-offset self-check feeds the fp32-rounded mean); pos: the PReLU's branch decisions z > 0 for
    the backward pass, taken from elsewhere (the large-offset case adopts the device's, as the net-level tests do)"""
    x, gy, ga, be = d64(op["x"]), d64(op["gy"]), d64(op["gamma"]), d64(op["beta"])
    M, C = x.shape
    mu = x.mean(0) if mean is None else d64(mean)
    var = ((x - x.mean(0)) ** 2).mean(0)
    inv = 1.0 / np.sqrt(var + BN_EPS)
    xh = (x - mu) * inv
    z = xh * ga + be
    a = 1.0 if slope is None else np.float64(F32(slope))
    y = np.where(z > 0, z, a * z)
    pos = z > 0 if pos is None else pos
    gz = np.where(pos, gy, a * gy)
    gg, gb = (gz * xh).sum(0), gz.sum(0)
    gx = (gz - gb / M - xh * gg / M) * ga * inv
    gs = (gy * np.where(pos, 0.0, z)).sum()
    r = dict(y=y, z=z, pos=pos, mean=mu, invstd=inv, rm=(1 - BN_MOM) * d64(op["rm"]) + BN_MOM * x.mean(0),
             rv=(1 - BN_MOM) * d64(op["rv"]) + BN_MOM * var * M / max(M - 1, 1), gx=gx, xh=xh, gz=gz,
             gg=acc * d64(op["acc"][:C]) + gg, gb=acc * d64(op["acc"][C:2 * C]) + gb, gs=acc * d64(op["acc"][2 * C]) + gs)
    ze = (x - d64(op["rm"])) / np.sqrt(d64(op["rv"]) + BN_EPS) * ga + be
    r["ye"] = np.where(ze > 0, ze, a * ze)
    return r


def bn_device(ctx, op, slope, acc):
    lib, h = ctx.lib, ctx.h
    M, C = op["x"].shape
    xd, gyd, ga, be = put(ctx, op["x"]), put(ctx, op["gy"]), put(ctx, op["gamma"]), put(ctx, op["beta"])
    sl = put(ctx, np.array([slope], F32)) if slope is not None else None
    rm, rv = put(ctx, op["rm"]), put(ctx, op["rv"])
    y, ye, mean, inv = out(ctx, M, C), out(ctx, M, C), out(ctx, C), out(ctx, C)
    ns = lib.fg_bn_scratch_floats(C)
    ctx.check(lib.fg_batchnorm_forward(h, P(xd), P(ye), M, C, P(ga), P(be), P(sl), P(out(ctx, C)), P(out(ctx, C)), P(rm), P(rv), BN_EPS, BN_MOM, 0, P(out(ctx, ns))))
    ctx.check(lib.fg_batchnorm_forward(h, P(xd), P(y), M, C, P(ga), P(be), P(sl), P(mean), P(inv), P(rm), P(rv), BN_EPS, BN_MOM, 1, P(out(ctx, ns))))
    gx = out(ctx, M, C)
    gg, gb, gs = put(ctx, op["acc"][:C]), put(ctx, op["acc"][C:2 * C]), put(ctx, op["acc"][2 * C:])
    ctx.check(lib.fg_batchnorm_backward(h, P(xd), P(gyd), P(gx), M, C, P(ga), P(be), P(sl), P(mean), P(inv), P(gg), P(gb),
                                        P(gs) if sl is not None else None, float(acc), P(out(ctx, ns))))
    return dict(y=y, ye=ye, mean=mean, invstd=inv, rm=rm, rv=rv, gx=gx, gg=gg, gb=gb, gs=gs if sl is not None else None)


def run_bn(ctx, case, dry=False):
    del KEEP[:]
    M, C = case
    op = bn_operands(M, C, Src(M + C, dry))
    return op, [(slope, acc, bn_device(ctx, op, slope, acc)) for slope, acc in ((0.25, 0), (None, 1))]


def bn_check(what, got, r, extra=None):
    """all outputs of test_batchnorm_prelu at its BAR entries; extra: {key: float64 array added to that key's bar}"""
    e = extra or {}
    sc = lambda k: max(1.0, float(np.abs(r[k]).max()))
    bars = dict(y=(BAR["bn_y"], 0), ye=(BAR["bn_y"], 0), mean=(BAR["bn_mean"], 0), invstd=(0, BAR["bn_invstd_rtol"]), rm=(BAR["bn_running_mean"], 0),
                rv=(0, BAR["bn_running_var_rtol"]), gx=(BAR["bn_gx"] * sc("gx"), 0), gg=(BAR["bn_gparam"] * sc("gg"), 0),
                gb=(BAR["bn_gparam"] * sc("gb"), 0), gs=(BAR["bn_gparam"] * max(1.0, abs(float(r["gs"]))), 0))
    for k, (atol, rtol) in bars.items():
        if got[k] is None:
            continue
        g = got[k].cpu().numpy().astype(np.float64).reshape(np.shape(r[k]))
        assert not np.isnan(g).any(), "%s %s: NaN" % (what, k)
        print("%s %s: max|err| %.3e, bar %.3e + %.1e rel" % (what, k, float(np.abs(g - r[k]).max()), float(np.max(atol + e.get(k, 0.0))), rtol))
        close(g, r[k], atol=atol + e.get(k, 0.0), rtol=rtol, what="%s %s" % (what, k))


@pytest.mark.parametrize("case", BN_CASES, ids=["%dx%d" % c for c in BN_CASES])
def test_batchnorm_ladders(ctx, case):
    op, runs = run_bn(ctx, case)
    for slope, acc, got in runs:
        bn_check("bn %dx%d slope %s acc %d" % (case + (slope, acc)), got, bn_reference(op, slope, acc))


OFFSET_CASE = (4096, 64)


def offset_bars(op, r, slope):
    """First-order effect of rounding the saved mean to fp32, per unit of xhat: d = |mean| 2^-24 invstd (half an ulp of the mean,
    in units of the standard deviation), propagated through each formula checked.  y = gamma xhat + beta moves by |gamma| d (the
    PReLU's slope is <= 1).  The rounding moves every row of a column by the same signed amount, so ggamma = sum gz xhat moves by
    |sum gz| d; gx = (gz - gbeta / M - xhat ggamma / M) gamma invstd by (|ggamma| + |xhat| |sum gz|) / M |gamma| invstd d (xhat and
    ggamma both move); gslope = sum over z <= 0 of gy z by |sum over z <= 0 of gy| |gamma| d per column.
    invstd, the running variance and gbeta do not read the saved mean and keep their bars; mean, the running mean and the evaluate
    output get the precision of fp32 at their magnitude (below)."""
    M = op["x"].shape[0]
    d = np.abs(r["mean"]) * U * r["invstd"]
    ga = np.abs(d64(op["gamma"]))
    gb = r["gz"].sum(0)
    # stored in fp32 at a magnitude of 1000 (mean), 100 (the updated running mean) and 1500 (the evaluate output, normalised by running
    # statistics that do not know the offset): half an ulp of the stored value, and for ye four roundings of terms of its size
    fmt = dict(mean=np.abs(r["mean"]) * U, rm=np.abs(r["rm"]) * U,
               ye=4 * U * (np.abs((d64(op["x"]) - d64(op["rm"])) / np.sqrt(d64(op["rv"]) + BN_EPS) * d64(op["gamma"])) + np.abs(d64(op["beta"]))))
    return dict(fmt, y=ga * d, gx=(np.abs((r["gz"] * r["xh"]).sum(0)) + np.abs(r["xh"]) * np.abs(gb)) / M * ga * r["invstd"] * d, gg=np.abs(gb) * d,
                gs=float((np.abs(np.where(r["pos"], 0.0, d64(op["gy"])).sum(0)) * ga * d).sum()) if slope is not None else 0.0)


def test_batchnorm_large_offset(ctx):
    """x = 1000 + 0.05 N(0, 1): what the pivot-shifted sums are for (a naive fp32 E[x^2] - E[x]^2 has no correct digit here).
    With the PReLU the backward pass branches on the sign of z, which the device recomputes from the fp32 mean: a unit within
    |gamma| d + BAR["bn_y"] of the kink may take the other branch, and invstd = 20 makes that an O(10) difference in gx.  So the
    reference takes its backward branches from the sign of the device's y, and every decision that differs from its own must lie
    within that distance of the kink."""
    M, C = OFFSET_CASE
    op = bn_operands(M, C, Src(4160), offset=1000.0)
    for slope, acc in ((0.25, 0), (None, 1)):
        got = bn_device(ctx, op, slope, acc)
        r = bn_reference(op, slope, acc)
        extra = offset_bars(op, r, slope)
        if slope is not None:
            pos = got["y"].cpu().numpy() > 0
            flips = pos != (r["z"] > 0)
            assert (np.abs(r["z"])[flips] <= (extra["y"] + BAR["bn_y"])[None, :].repeat(M, 0)[flips]).all(), "a branch decision far from the kink differs"
            print("bn offset: %d of %d PReLU decisions adopted from the device differ" % (int(flips.sum()), flips.size))
            assert flips.sum() <= 0.01 * flips.size
            r = bn_reference(op, slope, acc, pos=pos)
        bn_check("bn offset slope %s acc %d" % (slope, acc), got, r, extra=extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# optimizer options.  A case: (name, kind, n, options); three steps each, state carried over
# ---------------------------------------------------------------------------------------------------------------------------------
def _adam(name, n, **kw):
    return (name, "adam", n, dict(dict(gscale=1.0, l1=0.0, l2=0.0, clamp=0.0, lr=1e-3, b1=0.5, b2=0.9, eps=1e-3, ts=(1, 2, 1000), gout=True, gmag=1.0, special=False), **kw))


def _sgd(name, **kw):
    return (name, "sgd", 1003, dict(dict(gscale=1.0, l1=0.0, l2=0.0, clamp=0.0, lr=0.02, mom=0.9, damp=None, wd=0.0, nesterov=0, gmag=1.0, special=False), **kw))


OPT_CASES = [_adam("adam-n%d-%s" % (n, "gout" if go else "nogout"), n, gout=go) for n in (1, 2, 3, 7) for go in (True, False)] + [
    _adam("adam-l1-signed-zero", 7, l1=1e-3, special=True),
    _adam("adam-clamp-off", 7, clamp=0.0, gmag=50.0),
    _adam("adam-clamp-half", 7, clamp=0.5, gmag=50.0),
    _sgd("sgd-nesterov", nesterov=1, damp=0.0),
    _sgd("sgd-dampening", damp=0.3),
    _sgd("sgd-momentum0", mom=0.0),
    _sgd("sgd-weight-decay", wd=1e-3),
    _sgd("sgd-gscale", gscale=0.125),
    _sgd("sgd-l1-signed-zero", l1=1e-3, special=True),
    ("adagrad-gscale-l2-clamp", "adagrad", 1003, dict(gscale=0.125, l1=0.0, l2=1e-4, clamp=1.0, lr=1e-3, gmag=24.0, special=False)),
]


def run_opt(ctx, case, dry=False):
    """-> [(what, device tensor, float64 reference, atol, rtol)] after each of three steps.  Every vector sits at base + 1 float:
    aligned to 4 bytes and no more."""
    del KEEP[:]
    name, kind, n, o = case
    lib, h = ctx.lib, ctx.h
    S = Src(len(name) * 17 + n, dry)
    f = lambda v: np.float64(F32(v))

    def off1(a):                                    # a view at a 4-byte-only aligned address
        t = hold(torch.zeros(a.size + 5, dtype=torch.float32, device=ctx.device))
        k = 1 + (4 - (t.data_ptr() // 4) % 4) % 4   # data_ptr + 4 k bytes == 4 (mod 16)
        v = t[k:k + a.size]
        assert dry or v.data_ptr() % 16 == 4
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)))
        return v
    p0 = S.normal(n)
    if o["special"] and not dry:
        p0[:3] = np.array([0.0, -0.0, 1e-42], F32)[:min(3, n)]      # sign(+-0) = 0; a denormal keeps its sign
    pd, pr = off1(p0), d64(p0).copy()
    res = []
    pen = lambda x, g: penalty(x, g, f(o["gscale"]), f(o["l1"]), f(o["l2"]), f(o["clamp"]))
    if kind == "adam":
        md, vd, st = off1(np.zeros(n)), off1(np.zeros(n)), {}
        for t in o["ts"]:
            g = S.normal(n, scale=o["gmag"])
            go = off1(np.full(n, np.nan)) if o["gout"] else None
            ctx.check(lib.fg_adam_fused(h, P(pd), P(off1(g)), P(md), P(vd), n, o["gscale"], o["l1"], o["l2"], o["clamp"], o["lr"], o["b1"], o["b2"], o["eps"], t, P(go)))
            if dry:
                continue
            gbar = 4 * U * (np.abs(f(o["gscale"]) * d64(g)) + f(o["l1"]) + np.abs(f(o["l2"]) * pr))
            gp = pen(pr, d64(g))
            st["t"] = t - 1
            O.interruptable_adam(lambda x: (0.0, gp), pr, dict(learningRate=o["lr"], beta1=o["b1"], beta2=o["b2"], epsilon=o["eps"]), st)
            res += [("%s t=%d p" % (name, t), pd.clone(), pr.copy(), 2e-7, 2e-7), ("%s t=%d m" % (name, t), md.clone(), st["m"].copy(), 1e-7, 1e-5),
                    ("%s t=%d v" % (name, t), vd.clone(), st["v"].copy(), 1e-12, 1e-5)]
            if go is not None:                      # the penalised, clamped gradient: four fp32 roundings of terms of this size
                res.append(("%s t=%d g_out" % (name, t), go.clone(), gp.copy(), gbar, 0))
    elif kind == "sgd":
        pre = S.normal(n)
        mom, st = off1(pre), {}
        cfg = dict(learningRate=o["lr"], momentum=o["mom"], weightDecay=o["wd"], nesterov=bool(o["nesterov"]))
        if o["damp"] is not None:
            cfg["dampening"] = o["damp"]
        for step in range(3):
            g = S.normal(n, scale=o["gmag"])
            ctx.check(lib.fg_sgd_fused(h, P(pd), P(off1(g)), P(mom), n, o["gscale"], o["l1"], o["l2"], o["clamp"], o["lr"], o["mom"],
                                       o["mom"] if o["damp"] is None else o["damp"], o["wd"], o["nesterov"], 1 if step == 0 else 0))
            if dry:
                continue
            gp = pen(pr, d64(g))
            O.interruptable_sgd(lambda x: (0.0, gp), pr, cfg, st)
            res.append(("%s step %d p" % (name, step), pd.clone(), pr.copy(), 1e-5, 0))
            if o["mom"] == 0.0:
                res.append(("%s step %d momentum buffer untouched" % (name, step), mom.clone(), pre.copy(), 0, 0))
            else:
                res.append(("%s step %d momentum buffer" % (name, step), mom.clone(), st["dfdx"].copy(), 1e-5, 0))
    else:
        var, st = off1(np.zeros(n)), {}
        for step in range(3):
            g = S.normal(n, scale=o["gmag"])
            ctx.check(lib.fg_adagrad_fused(h, P(pd), P(off1(g)), P(var), n, o["gscale"], o["l1"], o["l2"], o["clamp"], o["lr"]))
            if dry:
                continue
            gp = pen(pr, d64(g))
            O.interruptable_adagrad(lambda x: (0.0, gp), pr, dict(learningRate=o["lr"]), st)
            res += [("%s step %d p" % (name, step), pd.clone(), pr.copy(), 1e-6, 0), ("%s step %d variance" % (name, step), var.clone(), st["paramVariance"].copy(), 0, 1e-5)]
    return res


@pytest.mark.parametrize("case", OPT_CASES, ids=[c[0] for c in OPT_CASES])
def test_optimizer_options(ctx, case):
    for what, got, ref, atol, rtol in run_opt(ctx, case):
        g = got.cpu().numpy()
        assert not np.isnan(g).any(), what
        if np.ndim(atol) == 0 and atol == 0 and rtol == 0:
            assert np.array_equal(g.view(np.int32), ref.astype(F32).view(np.int32)), "%s: bits differ" % what
        else:
            close(g, ref, atol=atol, rtol=rtol, what=what)


# ---------------------------------------------------------------------------------------------------------------------------------
# Philox4x32-10, from the algorithm's definition (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
# ---------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: [n][4] uint32, key: (k0, k1) -> [n][4] uint32"""
    c = [np.asarray(ctr, np.uint64)[:, i] & 0xFFFFFFFF for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]                   # 32 x 32 -> 64 bits, no overflow of uint64
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def philox_words(seed, offset, quads):
    """the library's stream: counter = (offset + quad as 64 bits in words 0 and 1, 0, 0), key = seed lo / hi"""
    q = (np.arange(quads, dtype=np.uint64) + np.uint64(offset % 2 ** 64))           # wraps mod 2^64 like the kernel's uint64
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.zeros_like(q), np.zeros_like(q)], 1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


TWO_PI_F = F32(6.28318530718)


def box_muller(words, dtype):
    """the formula of rng_kernel mode 2 on the same words, evaluated in `dtype`; u1, u2 and the fp32 constant are exact in both"""
    w = words.reshape(-1, 2)
    u1 = ((w[:, 0] >> 8).astype(np.float64) + 1.0) * U
    u2 = (w[:, 1] >> 8).astype(np.float64) * U
    u1, u2, tp = u1.astype(dtype), u2.astype(dtype), dtype(TWO_PI_F)
    rad = np.sqrt(dtype(-2.0) * np.log(u1))
    return np.stack([rad * np.cos(tp * u2), rad * np.sin(tp * u2)], 1).reshape(-1)


def normal_bar(words):
    """measured, not chosen: 4 x the largest deviation of a float32 numpy evaluation of the formula from the float64 one"""
    return 4.0 * float(np.abs(box_muller(words, np.float32).astype(np.float64) - box_muller(words, np.float64)).max())


@functools.lru_cache(None)
def measured_normal_bar():
    return normal_bar(philox_words(11, 0, NORMAL_N // 4).reshape(-1))


# (seed, offset, n)
RNG_CASES = [(1, 0, 1), (1, 0, 5), (2, 7, 1023), ((0xDEADBEEF << 32) | 0x12345678, 3, 1023), (5, 2 ** 32 - 2, 16), (9, 2 ** 40 + 3, 5),
             (0x8000000000000001, 2 ** 40 + 3, 1023)]
NORMAL_N = 1 << 16


def run_rng(ctx, case, dry=False):
    del KEEP[:]
    seed, offset, n = case
    lib, h = ctx.lib, ctx.h
    u01, u11, bern, nrm = out(ctx, n), out(ctx, n), out(ctx, n), out(ctx, n)
    ctx.check(lib.fg_rng_uniform(h, seed, offset, P(u01), n, 0.0, 1.0))
    ctx.check(lib.fg_rng_uniform(h, seed, offset, P(u11), n, -1.0, 1.0))
    ctx.check(lib.fg_rng_bernoulli(h, seed, offset, P(bern), n, 0.8))
    ctx.check(lib.fg_rng_normal(h, seed, offset, P(nrm), n, 0.0, 1.0))
    return u01, u11, bern, nrm


@pytest.mark.parametrize("case", RNG_CASES, ids=["seed%x-off%x-n%d" % c for c in RNG_CASES])
def test_philox_against_the_numpy_reference(ctx, case):
    seed, offset, n = case
    u01, u11, bern, nrm = (t.cpu().numpy() for t in run_rng(ctx, case))
    words = philox_words(seed, offset, (n + 3) // 4).reshape(-1)
    u = ((words >> 8).astype(np.float64) * U)[:n]
    assert np.array_equal(u01.astype(np.float64), u), "uniform(0, 1) is not (word >> 8) * 2^-24 bit for bit"
    assert np.array_equal(bern, (u.astype(F32) < F32(0.8)).astype(F32)), "bernoulli(0.8) is not u < 0.8f"
    close(u11, -1.0 + 2.0 * u, atol=2.0 ** -23, what="uniform(-1, 1)")
    wn = philox_words(seed, offset, (n + 3) // 4).reshape(-1)
    close(nrm, box_muller(wn, np.float64)[:n], atol=measured_normal_bar(), what="normal(0, 1)")


def test_normal_against_float64_box_muller(ctx):
    """65536 draws; the bar is normal_bar of these very words (tests/DISPATCH_COVERAGE.md records the figure)"""
    o = out(ctx, NORMAL_N)
    ctx.check(ctx.lib.fg_rng_normal(ctx.h, 11, 0, P(o), NORMAL_N, 0.0, 1.0))
    words = philox_words(11, 0, NORMAL_N // 4).reshape(-1)
    bar = measured_normal_bar()
    ref = box_muller(words, np.float64)
    print("fg_rng_normal: max|err| %.3e, bar %.3e" % (float(np.abs(o.cpu().numpy() - ref).max()), bar))
    close(o.cpu().numpy(), ref, atol=bar, what="normal(0, 1), 65536 draws")
    o2 = out(ctx, 1001)
    ctx.check(ctx.lib.fg_rng_normal(ctx.h, 11, 0, P(o2), 1001, 0.25, 0.005))
    close(o2.cpu().numpy(), 0.25 + 0.005 * ref[:1001], atol=0.005 * bar + 2 * U, what="normal(0.25, 0.005)")
