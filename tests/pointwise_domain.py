"""The value domain of the pointwise, pooling, optimizer, reduction and RNG kernels (tests/POINTWISE_DOMAIN.md): probes, cases and numpy
references shared by tests/test_gpu_pointwise_domain.py (device) and tests/test_pointwise_domain_host.py (CPU).

A case is (name, part, expect, run): run(ctx, dry) makes the calls and returns [Check]; with dry=True it makes the same calls on host
tensors in the planning-only context and returns nothing (the host test asserts that every kernel of `expect` is among the launches).
A reference is a float32 numpy RESTATEMENT of the kernel's expression -- every product and sum rounded once, in the kernel's order --
wherever the expression has no product feeding a sum (or the probes make that product exact), so that a contraction into an FMA
cannot change the bits; the host test holds the restatements to oracle/torch7_nn.py where the oracle defines the case.  Comparison
modes: "bits" (all 32 bits, NaN payloads included: the kernel copies), "nanbits" (NaN where the reference is NaN, whatever the
payload; the same 32 bits elsewhere, so the sign of a zero counts), "class" (NaN, +-inf, +-0, +-finite; finite values within the bar),
"value" (NaN where NaN, else numerically equal: +0 == -0), "close" (NaN where NaN, equal infinities, else within the bar of a float64
reference)."""
import collections
import ctypes

import numpy as np
import torch

import value_domain as VD
from gpu_util import BAR
from value_domain import F32, U32, bits

KEEP = []                           # every operand of the running case (see tests/test_gpu_pointwise_paths.py)
Check = collections.namedtuple("Check", "what got ref mode src atol rtol")
Case = collections.namedtuple("Case", "name part expect run")
CASES = []


def case(name, part, expect):
    def deco(f):
        CASES.append(Case(name, part, tuple(expect), f))
        return f
    return deco


def chk(what, got, ref, mode, src=None, atol=0.0, rtol=0.0):
    return Check(what, got, np.asarray(ref), mode, src or {}, atol, rtol)


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=U32).view(F32)


def quiet():
    return np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore")


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------
CLASS_NAMES = ("NaN", "+inf", "-inf", "+0", "-0", "+finite", "-finite")


def classes(a):
    a = f32(a)
    neg = np.signbit(a)
    c = np.where(neg, 6, 5)
    c = np.where(a == 0, np.where(neg, 4, 3), c)
    c = np.where(np.isinf(a), np.where(neg, 2, 1), c)
    return np.where(np.isnan(a), 0, c)


def mismatches(got, ref, mode, atol=0.0, rtol=0.0):
    """-> flat indices where `got` misses `ref` under `mode`"""
    g, r = f32(got).reshape(-1), f32(ref).reshape(-1)
    assert g.shape == r.shape, (g.shape, r.shape)
    rn, gn = np.isnan(r), np.isnan(g)
    if mode == "bits":
        bad = bits(g) != bits(r)
    elif mode == "nanbits":
        bad = np.where(rn, ~gn, bits(g) != bits(r))
    elif mode == "value":
        bad = np.where(rn, ~gn, gn | (g != r))
    elif mode in ("class", "close"):
        # class: the classes agree and finite values are within the bar; close: NaN where NaN, equal infinities, the rest within the
        # bar of the (float64) reference, whatever a value below the bar rounds to
        r64 = np.asarray(ref, np.float64).reshape(-1)
        with quiet():
            err = np.abs(g.astype(np.float64) - r64)
            far = err > np.broadcast_to(np.asarray(atol, np.float64), err.shape).reshape(-1) + rtol * np.abs(r64)
        if mode == "class":
            bad = (classes(g) != classes(r)) | (np.isfinite(r) & np.isfinite(g) & far)
        else:
            ok = (g.astype(np.float64) == r64) | (np.isfinite(err) & ~far)
            bad = np.where(np.isnan(r64), ~gn, gn | ~ok)
    else:
        raise ValueError(mode)
    return np.flatnonzero(bad)


def show(v):
    v = F32(v)
    return "%r (0x%08x)" % (float(v), int(np.array([v], F32).view(U32)[0]))


def verify(c):
    """assert one Check; the message names the probe: the operands of the first element that differs"""
    got = c.got.detach().cpu().numpy() if isinstance(c.got, torch.Tensor) else c.got
    bad = mismatches(got, c.ref, c.mode, c.atol, c.rtol)
    if bad.size == 0:
        return
    i = int(bad[0])
    g, r = f32(got).reshape(-1), f32(c.ref).reshape(-1)
    src = ", ".join("%s = %s" % (k, show(np.broadcast_to(v, c.ref.shape).reshape(-1)[i]) if np.size(v) > 1 else show(v)) for k, v in c.src.items())
    raise AssertionError("%s [%s]: %d of %d elements differ; first at %d: got %s, want %s; probe: %s"
                         % (c.what, c.mode, bad.size, g.size, i, show(g[i]), show(r[i]), src or "-"))


# ---------------------------------------------------------------------------------------------------------------------------------
# device plumbing (host tensors in the planning-only context)
# ---------------------------------------------------------------------------------------------------------------------------------
def hold(t):
    KEEP.append(t)
    return t


def P(t):
    return t.data_ptr() if t is not None else None


def put(ctx, a):
    return hold(torch.from_numpy(f32(a).copy()).to(ctx.device))


def off1(ctx, a, fill=None):
    """a float32 view at base + 1 float: aligned to 4 bytes and no more (tests/mem_contract.py's rule, as run_opt does it)"""
    a = f32(a) if fill is None else np.full(int(a), fill, F32)
    t = hold(torch.zeros(a.size + 5, dtype=torch.float32, device=ctx.device))
    k = 1 + (4 - (t.data_ptr() // 4) % 4) % 4
    v = t[k:k + a.size]
    assert v.data_ptr() % 16 == 4
    v.copy_(torch.from_numpy(a.reshape(-1).copy()))
    return v


def out1(ctx, n):
    return off1(ctx, n, fill=np.nan)                # an element nobody writes stays NaN ... where the reference has none


def out(ctx, *shape):
    return hold(torch.full(shape, 1e30, dtype=torch.float32, device=ctx.device))       # (a finite poison: NaN is a legitimate result here)


# ---------------------------------------------------------------------------------------------------------------------------------
# part 1: every 4-tuple of a palette of 8 as one 2x2 window
# ---------------------------------------------------------------------------------------------------------------------------------
PALETTE = np.array([0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x3f800000, 0x80000200], dtype=U32)
PALETTE_NAMES = ("NaN", "-NaN(1)", "+inf", "-inf", "+0", "-0", "1.0", "-0x1p-140")
WIN_SEED = 20261021
WIN_SHAPE = (1, 32, 32, 16)         # NHWC: 256 windows x 16 channels = 8^4
SLOPES = (0.25, 0.0, -0.5)


def window_tuples():
    """[4096][4] palette indices in scan order (dy, dx), in the permuted window order"""
    idx = np.stack(np.unravel_index(np.arange(8 ** 4), (8, 8, 8, 8)), 1)
    return idx[np.random.default_rng(WIN_SEED).permutation(8 ** 4)]


def windows(x):
    """[B][H][W][C] -> [B][H/2][W/2][C][4], slot = 2 dy + dx"""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def unwindows(w):
    B, H2, W2, C, _ = w.shape
    return np.ascontiguousarray(w.reshape(B, H2, W2, C, 2, 2).transpose(0, 1, 4, 2, 5, 3)).reshape(B, 2 * H2, 2 * W2, C)


def window_tensor():
    t = window_tuples().reshape(1, 16, 16, 16, 4)
    return unwindows(PALETTE[t]).view(F32)


def window_tensor_1ch():
    """the same 4096 windows as 16 one-channel images [16][32][32][1] (the input of a 1 -> 16 channel 1x1 convolution)"""
    t = window_tuples().reshape(16, 16, 16, 1, 4)
    return unwindows(PALETTE[t]).view(F32)


def pooled_noise(shape=(1, 16, 16, 16), seed=3):
    g = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    return np.where(g == 0, F32(1), g)


def max_slot(w):
    """THE RULE (include/facegen_hip.h, fg_maxpool2x2_*): the first NaN of the window if it holds one, otherwise the first maximum in
    scan order; a tie (-0 against +0 included) stays with the earlier slot.  w: [..., 4] -> slot index"""
    nan = np.isnan(w)
    with quiet():
        m = np.where(nan, -np.inf, w).argmax(-1)
    return np.where(nan.any(-1), nan.argmax(-1), m)


def take_slot(w, slot):
    return np.take_along_axis(w, slot[..., None], -1)[..., 0]


def scatter_slot(g, slot):
    """g at `slot`, +0 in the other three: [...] -> [..., 4]"""
    o = np.zeros(g.shape + (4,), F32)
    np.put_along_axis(o, slot[..., None], g[..., None], -1)
    return o


def prelu_ref(x, a, mask=None, mscale=1.0):
    """prelu_fwd_kernel: r = v > 0 ? v : a * v; r *= mask * mscale"""
    with quiet():
        r = np.where(x > 0, x, F32(a) * x).astype(F32)
        return r if mask is None else (r * (f32(mask) * F32(mscale))).astype(F32)


def prelu_bwd_ref(x, gy, a, mask=None, mscale=1.0):
    """prelu_bwd_kernel: g = gy * (mask * mscale); gx = v > 0 ? g : a * g"""
    with quiet():
        g = gy if mask is None else (gy * (f32(mask) * F32(mscale))).astype(F32)
        return np.where(x > 0, g, F32(a) * g).astype(F32)


def win_src(w):
    return {"slot%d" % k: w[..., k] for k in range(4)}


def full_src(w):
    return {"slot%d" % k: unwindows(np.repeat(w[..., k:k + 1], 4, -1)) for k in range(4)}


@case("maxpool", 1, ["maxpool_fwd_kernel", "maxpool_bwd_kernel"])
def run_maxpool(ctx, dry):
    x, gy = window_tensor(), pooled_noise()
    B, H, W, C = WIN_SHAPE
    xd, y, gx = put(ctx, x), out(ctx, B, H // 2, W // 2, C), out(ctx, B, H, W, C)
    ctx.check(ctx.lib.fg_maxpool2x2_forward(ctx.h, P(xd), P(y), B, H, W, C))
    ctx.check(ctx.lib.fg_maxpool2x2_backward(ctx.h, P(xd), P(put(ctx, gy)), P(gx), B, H, W, C))
    if dry:
        return []
    w = windows(x)
    slot = max_slot(w)
    return [chk("maxpool forward: the value is the slot's, bit for bit", y, take_slot(w, slot), "bits", win_src(w)),
            chk("maxpool backward: gy at the forward's slot, +0 in the other three", gx, unwindows(scatter_slot(gy, slot)), "bits", full_src(w))]


def pool4(w):
    """(p0 + p1) + (p2 + p3), fp32"""
    with quiet():
        return ((w[..., 0] + w[..., 1]).astype(F32) + (w[..., 2] + w[..., 3]).astype(F32)).astype(F32)


def up2(a):
    return np.repeat(np.repeat(a, 2, 1), 2, 2)


@case("avgpool-upsample", 1, ["avgpool_fwd_kernel", "avgpool_bwd_kernel", "upsample_fwd_kernel", "upsample_bwd_kernel"])
def run_avg_up(ctx, dry):
    x = window_tensor()
    small = np.ascontiguousarray(x[:, ::2, ::2, :])               # the windows' first slots: every palette value
    B, H, W, C = WIN_SHAPE
    xd, sd = put(ctx, x), put(ctx, small)
    ap, apg, us, usg = out(ctx, B, H // 2, W // 2, C), out(ctx, B, H, W, C), out(ctx, B, H, W, C), out(ctx, B, H // 2, W // 2, C)
    lib, h = ctx.lib, ctx.h
    ctx.check(lib.fg_avgpool2x2_forward(h, P(xd), P(ap), B, H, W, C))
    ctx.check(lib.fg_avgpool2x2_backward(h, P(sd), P(apg), B, H, W, C))
    ctx.check(lib.fg_upsample_nearest2x_forward(h, P(sd), P(us), B, H // 2, W // 2, C))
    ctx.check(lib.fg_upsample_nearest2x_backward(h, P(xd), P(usg), B, H // 2, W // 2, C))
    if dry:
        return []
    w = windows(x)
    with quiet():
        return [chk("avgpool forward 0.25 ((p0 + p1) + (p2 + p3))", ap, (F32(0.25) * pool4(w)).astype(F32), "nanbits", win_src(w)),
                chk("avgpool backward 0.25 gy", apg, (F32(0.25) * up2(small)).astype(F32), "nanbits", dict(gy=up2(small))),
                chk("upsample forward: a copy", us, up2(small), "bits", dict(x=up2(small))),
                chk("upsample backward (p0 + p1) + (p2 + p3)", usg, pool4(w), "nanbits", win_src(w))]


def actpool_ref(x, a, mask, mscale):
    """actpool_fwd_kernel: s = ((((0 + act0) + act1) + act2) + act3) * (0.25 * (mscale * mask[b][c]))"""
    w = windows(x)
    with quiet():
        act = np.where(w > 0, w, F32(a) * w).astype(F32)
        s = np.zeros(w.shape[:-1], F32)
        for k in range(4):
            s = (s + act[..., k]).astype(F32)
        m = (F32(mscale) * f32(mask)).astype(F32)[:, None, None, :]
        return (s * (F32(0.25) * m).astype(F32)).astype(F32)


def actpool_bwd_ref(x, gy, a, mask, mscale):
    """actpool_bwd_kernel: g = gy * (0.25 * (mscale * mask)); gx = v > 0 ? g : a * g"""
    with quiet():
        m = (F32(mscale) * f32(mask)).astype(F32)[:, None, None, :]
        g = up2((gy * (F32(0.25) * m).astype(F32)).astype(F32))
        return np.where(x > 0, g, F32(a) * g).astype(F32)


ACTPOOL_MASK = np.array([[1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0]], F32)


@case("actpool", 1, ["actpool_fwd_kernel", "actpool_bwd_kernel"])
def run_actpool(ctx, dry):
    x, gy = window_tensor(), pooled_noise()
    B, H, W, C = WIN_SHAPE
    xd, gd, md = put(ctx, x), put(ctx, gy), put(ctx, ACTPOOL_MASK)
    res = []
    for a in SLOPES:
        sl = put(ctx, np.array([a], F32))
        y, gx, gs = out(ctx, B, H // 2, W // 2, C), out(ctx, B, H, W, C), out(ctx, 1)
        ctx.check(ctx.lib.fg_actpool_forward(ctx.h, P(xd), P(sl), P(md), 1.25, P(y), B, H, W, C))
        ctx.check(ctx.lib.fg_actpool_backward(ctx.h, P(xd), P(gd), P(sl), P(md), 1.25, P(gx), P(gs), 0.0, B, H, W, C, P(out(ctx, 1024))))
        if dry:
            continue
        w = windows(x)
        res += [chk("actpool forward, slope %g" % a, y, actpool_ref(x, a, ACTPOOL_MASK, 1.25), "nanbits", win_src(w)),
                chk("actpool backward, slope %g" % a, gx, actpool_bwd_ref(x, gy, a, ACTPOOL_MASK, 1.25), "nanbits", dict(x=x, gy=up2(gy))),
                chk("actpool slope gradient with NaN inputs, slope %g" % a, gs, np.array([np.nan], F32), "class")]
    return res


# ---- the fused PReLU + max-pool stage of fg_net, given the window tensor as its pre-activation ----------------------------------------
# NET_CASES r8-actmaxpool / r8-actmaxpool-dropout with the producing convolution replaced by a 1 -> 16 channel 1x1 convolution of weight
# 1 and bias -0: the only convolution that hands a non-finite input on without 0 * inf in a neighbour.  Its output (exposed by
# fg_net_layer_output) is what the reference starts from; the host test asserts that it still holds the palette's classes.
ACTMAX_B = 16
ACTMAX_DIMS = (1, 32, 32)


def actmax_layers(dropout):
    return [("CONV", 1, 16, 1, 0, 0, 0), ("PRELU",), ("MAXPOOL2",)] + ([("DROPOUT", 0, 0, 0, 0, 0.5)] if dropout else [])


def actmax_mask():
    return (np.random.default_rng(11).random((ACTMAX_B, 16, 16, 16)) < 0.5).astype(F32)


def actmax_gy():
    """one nonzero channel per pooled pixel: the 1x1 data gradient sums the 16 channels, and a sum with one nonzero term is exact"""
    g = pooled_noise((ACTMAX_B, 16, 16, 1), seed=5)
    b, y, x = np.meshgrid(np.arange(ACTMAX_B), np.arange(16), np.arange(16), indexing="ij")
    hot = ((b + 3 * y + 5 * x) % 16)[..., None] == np.arange(16)
    return np.where(hot, g, F32(0)).astype(F32)


def actmax_reference(xpre, a, gy, mask, mscale):
    """-> (pooled output, input gradient [B][32][32][1]) of PReLU -> MaxPool [-> Dropout] behind the 1x1 convolution of weight 1"""
    w = windows(prelu_ref(xpre, a))
    slot = max_slot(w)
    pos = take_slot(windows(xpre), slot) > 0
    with quiet():
        k = None if mask is None else (f32(mask) * F32(mscale)).astype(F32)
        y = take_slot(w, slot) if k is None else (take_slot(w, slot) * k).astype(F32)
        g = gy if k is None else (gy * k).astype(F32)
        gpre = np.where(pos, g, F32(a) * g).astype(F32)                 # the gradient at the chosen slot, per channel
        gsum = gpre.astype(np.float64).sum(-1, keepdims=True).astype(F32)     # one nonzero term (asserted by the host test)
    # every channel of xpre is the same image, so the slot is the same in all 16 channels
    return y, unwindows(scatter_slot(gsum, slot[..., :1]))


def run_actmax(ctx, dry, dropout):
    import net_cases as NC
    layers, B = actmax_layers(dropout), ACTMAX_B
    x, gy, mask = window_tensor_1ch(), actmax_gy(), actmax_mask()
    res = []
    for a in SLOPES:
        dn = hold(NC.device_net(ctx, layers, ACTMAX_DIMS, B))
        wo, wn, bo, bn = dn.param_offsets(0)
        so = dn.param_offsets(1)[0]
        p = np.zeros(dn.n_params, F32)
        p[wo:wo + wn], p[bo:bo + bn], p[so] = 1.0, -0.0, a
        dn.params.copy_(torch.from_numpy(p))
        dn.params_changed()
        md = [put(ctx, mask.reshape(-1))] if dropout else None
        y = dn.forward(put(ctx, x), masks=md, train=True)
        if not dry:
            y, xpre = y.cpu().numpy().reshape(B, 16, 16, 16), dn.layer_output(0).cpu().numpy().reshape(B, 32, 32, 16)
        gx = dn.backward(put(ctx, gy), param_grads=True, input_grad=True)
        if dry:
            continue
        ry, rgx = actmax_reference(xpre, a, gy, mask if dropout else None, 2.0)
        wp = windows(xpre)
        tag = "fused PReLU + max-pool%s, slope %g" % (" + dropout" if dropout else "", a)
        res += [chk(tag + ": the pre-activation is the window tensor", xpre, np.broadcast_to(x, xpre.shape), "value", dict(x=np.broadcast_to(x, xpre.shape))),
                chk(tag + ": forward", y, ry, "nanbits", win_src(wp)),
                chk(tag + ": input gradient (gy through the forward's slot)", gx.cpu().numpy(), rgx, "value",
                    {k: v[..., :1] for k, v in full_src(wp).items()})]
    return res


@case("actmaxpool-net", 1, ["actmaxpool_fwd_kernel", "maxpool_prelu_bwd_kernel"])
def run_actmax_plain(ctx, dry):
    return run_actmax(ctx, dry, False)


@case("actmaxpool-dropout-net", 1, ["actmaxpool_fwd_kernel", "maxpool_prelu_bwd_kernel"])
def run_actmax_dropout(ctx, dry):
    return run_actmax(ctx, dry, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# part 2: element-wise kernels over every binade
# ---------------------------------------------------------------------------------------------------------------------------------
def probes():
    """VALUE_DOMAIN part 3: +-2^e for e = -149 .. 127 with random mantissas, +-0, the largest values, +-inf, six NaN patterns"""
    return np.concatenate([VD.finite_probes(), VD.edge_probes()]).view(F32)


def probes2():
    """a second operand: the same values, rolled, so that every class meets another one (0 * inf, inf - inf, ...)"""
    return np.roll(probes(), 7)


PRELU_SLOPES = (0.25, 0.0, -1.0, float("nan"), float("inf"))
MSCALES = (1.0, 1.25)


def masks01(n):
    m = (np.arange(n) % 2).astype(F32)
    return [m, (1 - m).astype(F32)]                 # between them every probe is kept once and dropped once


@case("prelu", 2, ["prelu_fwd_kernel", "prelu_bwd_kernel"])
def run_prelu(ctx, dry):
    x, gy = probes(), probes2()
    n = x.size
    xd, gd = off1(ctx, x), off1(ctx, gy)
    res = []
    for a in PRELU_SLOPES:
        sl = put(ctx, np.array([a], F32))
        for mask, ms in [(None, 1.0)] + [(m, s) for m in masks01(n) for s in MSCALES]:
            md = off1(ctx, mask) if mask is not None else None
            y, gx, gs = out1(ctx, n), out1(ctx, n), out(ctx, 1)
            ctx.check(ctx.lib.fg_prelu_forward(ctx.h, P(xd), P(sl), P(md), ms, P(y), n))
            ctx.check(ctx.lib.fg_prelu_backward(ctx.h, P(xd), P(gd), P(sl), P(md), ms, P(gx), P(gs), 0.0, n, P(out(ctx, 1024))))
            if dry:
                continue
            tag = "slope %g, %s" % (a, "no mask" if mask is None else "mask %d.., mscale %g" % (mask[0], ms))
            src = dict(x=x, mask=mask if mask is not None else F32(1))
            res += [chk("prelu forward, " + tag, y, prelu_ref(x, a, mask, ms), "nanbits", src),
                    chk("prelu backward, " + tag, gx, prelu_bwd_ref(x, gy, a, mask, ms), "nanbits", dict(src, gy=gy))]
    return res


def leakyrelu_ref(x, s):
    """LeakyReLU.lua:13-31 as leakyrelu_fwd_kernel states it: (|x| + x) / 2 + (|x| - x) (-s / 2).  One of the two terms is an exact zero
    for every finite x, so a contraction cannot move a bit.  +inf gives NaN (inf - inf) and x > FLT_MAX / 2 gives +inf: the reference's."""
    with quiet():
        av = np.abs(x)
        return (((av + x).astype(F32) * F32(0.5)).astype(F32) + ((av - x).astype(F32) * (-F32(s) * F32(0.5))).astype(F32)).astype(F32)


def leakyrelu_bwd_ref(x, gy, s):
    with quiet():
        return np.where(x >= 0, gy, (F32(s) * gy).astype(F32)).astype(F32)


def sigmoid_bwd_ref(y, gy):
    with quiet():
        return ((gy * y).astype(F32) * (F32(1) - y).astype(F32)).astype(F32)


def sigmoid_formula(x, dtype):
    """1 / (1 + exp(-x)) evaluated in `dtype`"""
    with quiet():
        x = np.asarray(x, dtype)
        return (dtype(1) / (dtype(1) + np.exp(-x))).astype(dtype)


def sigmoid_bar(x):
    """measured, not chosen: 4 x the largest deviation of a float32 numpy evaluation of the formula from the float64 one, over the
    finite probes (tests/test_gpu_pointwise_paths.py normal_bar got its bar the same way)"""
    fin = np.isfinite(x)
    return 4.0 * float(np.abs(sigmoid_formula(x[fin], np.float32).astype(np.float64) - sigmoid_formula(x[fin], np.float64)).max())


def sigmoid_checks(what, y, x):
    """exact at the non-finite inputs (0 at -inf, 1 at +inf, NaN at NaN); no NaN and within the measured bar of the float64 sigmoid at
    every finite one"""
    edge = ~np.isfinite(x)
    return [chk(what + ": 0 at -inf, 1 at +inf, NaN at NaN", y[edge], sigmoid_formula(x[edge], np.float32), "value", dict(x=x[edge])),
            chk(what + ": finite inputs against the float64 sigmoid", y[~edge], sigmoid_formula(x[~edge], np.float64), "close", dict(x=x[~edge]), atol=sigmoid_bar(x))]


@case("leakyrelu-sigmoid", 2, ["leakyrelu_fwd_kernel", "leakyrelu_bwd_kernel", "sigmoid_fwd_kernel", "sigmoid_bwd_kernel"])
def run_leaky_sigmoid(ctx, dry):
    x, gy = probes(), probes2()
    n, s = x.size, 0.2
    xd, gd = off1(ctx, x), off1(ctx, gy)
    yl, gl, ys, gs = out1(ctx, n), out1(ctx, n), out1(ctx, n), out1(ctx, n)
    lib, h = ctx.lib, ctx.h
    ctx.check(lib.fg_leakyrelu_forward(h, P(xd), s, P(yl), n))
    ctx.check(lib.fg_leakyrelu_backward(h, P(xd), P(gd), s, P(gl), n))
    ctx.check(lib.fg_sigmoid_forward(h, P(xd), P(ys), n))
    ctx.check(lib.fg_sigmoid_backward(h, P(xd), P(gd), P(gs), n))      # the probes as the saved output: the expression, not its domain
    if dry:
        return []
    return [chk("leakyrelu forward", yl, leakyrelu_ref(x, s), "nanbits", dict(x=x)),
            chk("leakyrelu backward", gl, leakyrelu_bwd_ref(x, gy, s), "nanbits", dict(x=x, gy=gy)),
            chk("sigmoid backward gy y (1 - y)", gs, sigmoid_bwd_ref(x, gy), "nanbits", dict(y=x, gy=gy))] + sigmoid_checks("sigmoid forward", ys.cpu().numpy(), x)


GEMV_SIG_LAYERS = [("LINEAR", 1, 1), ("SIGMOID",)]


@case("gemv-sigmoid-net", 2, ["gemv_fwd_kernel"])
def run_gemv_sigmoid(ctx, dry):
    """Linear(1 -> 1) of weight 1 and bias 0 + Sigmoid as one fg_net: gemv_fwd_kernel's own sigmoid on the probes (x * 1 + 0 = x)"""
    import net_cases as NC
    x = probes()
    dn = hold(NC.device_net(ctx, GEMV_SIG_LAYERS, (1, 1, 1), x.size))
    wo, wn, bo, bn = dn.param_offsets(0)
    p = np.zeros(dn.n_params, F32)
    p[wo] = 1.0
    dn.params.copy_(torch.from_numpy(p))
    dn.params_changed()
    y = dn.forward(put(ctx, x.reshape(-1, 1)), train=False)
    if dry:
        return []
    return sigmoid_checks("sigmoid of gemv_fwd_kernel", y.cpu().numpy().reshape(-1), x)


AXPBY = (0.75, -1.25)


def axpby_orders(x, y):
    """a x + b y in the three orders a compiler may choose: both products rounded; either product contracted into the sum"""
    a, b = F32(AXPBY[0]), F32(AXPBY[1])
    with quiet():
        ax, by = (a * x).astype(F32), (b * y).astype(F32)
        plain = (ax + by).astype(F32)
        f1 = (np.float64(a) * x.astype(np.float64) + by.astype(np.float64)).astype(F32)
        f2 = (np.float64(b) * y.astype(np.float64) + ax.astype(np.float64)).astype(F32)
    return plain, f1, f2


def axpby_y():
    """the second operand of fg_axpby: rolled so that no element's class depends on the order of evaluation (host test)"""
    y = np.roll(probes(), 13)
    y[:2] = [-0.0, 0.0]                             # against x = +0, -0: both signed zeros among the results
    return y


SPATIAL = (3, 5, 4)                 # B, HW, C of the spatial-dropout probe block


@case("dropout-add-axpby-sum", 2, ["mul_mask_kernel", "scale_mask_nc_kernel", "add_kernel", "axpby_kernel", "sum_parts_kernel"])
def run_linear_family(ctx, dry):
    x, z = probes(), probes2()
    n = x.size
    lib, h = ctx.lib, ctx.h
    xd, zd = off1(ctx, x), off1(ctx, z)
    res, m = [], masks01(n)[0]
    for mask in (None, m):
        y = out1(ctx, n)
        ctx.check(lib.fg_dropout_apply(h, P(xd), P(off1(ctx, mask)) if mask is not None else None, 2.0, P(y), n))
        if not dry:
            with quiet():
                ref = (x * ((mask * F32(2)).astype(F32) if mask is not None else F32(2))).astype(F32)
            res.append(chk("dropout x (mask scale), %s" % ("mask" if mask is not None else "no mask"), y, ref, "nanbits", dict(x=x, mask=mask if mask is not None else F32(1))))
    B, HW, C = SPATIAL
    k = B * HW * C
    sm = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 0, 1]], F32)
    ys = out1(ctx, k)
    ctx.check(lib.fg_spatial_dropout_apply(h, P(off1(ctx, x[-k:])), P(put(ctx, sm)), 1.25, P(ys), B, HW, C))
    s, s3 = out1(ctx, n), out1(ctx, n)
    ctx.check(lib.fg_add(h, P(xd), P(zd), P(s), n))
    yd = off1(ctx, axpby_y())
    ctx.check(lib.fg_axpby(h, AXPBY[0], P(xd), AXPBY[1], P(yd), n))
    w = np.roll(x, 23)
    parts = [xd, zd, off1(ctx, w)]
    ctx.check(lib.fg_sum_n(h, (ctypes.c_void_p * 3)(*[P(t) for t in parts]), 3, P(s3), n))
    if dry:
        return []
    with quiet():
        mm = np.broadcast_to((sm * F32(1.25)).astype(F32)[:, None, :], (B, HW, C)).reshape(-1)
        res += [chk("spatial dropout x (mask[b][c] mscale)", ys, (x[-k:] * mm).astype(F32), "nanbits", dict(x=x[-k:], mask=mm)),
                chk("add", s, (x + z).astype(F32), "nanbits", dict(a=x, b=z)),
                chk("axpby: class", yd, axpby_orders(x, axpby_y())[0], "class", dict(x=x, y=axpby_y()), atol=np.inf),
                chk("sum_n (p0 + p1) + p2", s3, ((x + z).astype(F32) + w).astype(F32), "nanbits", dict(p0=x, p1=z, p2=w))]
    return res


# ---- the PReLU slope gradient across its fused forms ----------------------------------------------------------------------------------
# A +inf in the gradient that reaches a PReLU.  prelu_bwd_kernel SKIPS a unit with a positive input (if (!(x > 0)) s = fma(x, g, s)); a
# fused form that multiplies by a selected zero instead makes 0 * inf = NaN there.  The layer behind the PReLU gets positive weights,
# so one +inf in the net's output gradient arrives as +inf at every unit of its receptive field -- positive and non-positive inputs
# alike -- and the slope gradient is -inf (sum of x g over x <= 0) in the un-fused form.  Every case runs with FG_FUSE_PRELU set (503)
# and cleared (502): the two words must give the same class, and 502 must give -inf.
# (case, the launch that holds the fused form: a name, or a pattern over the whole launch text where the instance matters -- the last
# template argument 2 is the act-backward epilogue).  r3-gemv-dropout-mask stands for the issue's r3-gemv-plain-inner: there the PReLU
# sits BEHIND the Linear(130 -> 1), so that net never launches gemv_bwd_act_kernel.
# Third entry: what prelu_bwd_kernel gives.  -inf where the PReLU has non-positive inputs; s-actbwd-on-igemm-linear feeds its PReLU a
# sigmoid's output, every input is positive, every unit is skipped and the sum is +0 -- a multiply by a selected zero gives NaN there
# all the same, and so do the tile's columns past N (32 of 64), whose accumulators are inf times zero-filled weights.
SLOPE_CASES = [("r9-act-on-splitsum-conv", "sum_splits_actbwd_kernel", -np.inf), ("r5-thinin-general-thinoutsig", "thin_in_mfma_kernel<*, 2>", -np.inf),
               ("r10-actbwd-on-thinout-7x7", "thin_in_mfma_lds_kernel<*, 2>", -np.inf), ("r10-actbwd-on-thinout-5x5-pow2", "thin_in_mfma_pad_kernel<*, 2>", -np.inf),
               ("s-actbwd-on-igemm-linear", "igemm_act_kernel<*, 2>", 0.0), ("r3-gemv-dropout-mask", "gemv_bwd_act_kernel", -np.inf)]


def slope_case_parts(name):
    """-> (case, index of its LAST PReLU, index of the parameter layer behind it)"""
    import net_cases as NC
    c = [c for c in NC.NET_CASES if c.name == name][0]
    i = max(k for k, l in enumerate(c.layers) if l[0] == "PRELU")
    j = min(k for k, l in enumerate(c.layers) if k > i and l[0] in ("CONV", "LINEAR"))
    return c, i, j


def run_slope_case(ctx, dry, name, unfused):
    import net_cases as NC
    c, i, j = slope_case_parts(name)
    first, outs = NC.walk(c.layers, c.dims)
    res, got = [], {}
    for fusion in (c.fusion, c.fusion & ~1):        # FG_FUSE_PRELU set (the case's own word) and cleared
        ctx.set_fusion(fusion)
        try:
            if dry:
                P32 = np.zeros(0, F32)
                x = np.zeros((c.batch,) + first.shape, F32)
                gy = np.zeros((c.batch,) + outs[-1].shape, F32)
                masks = NC.draw_masks(c.layers, c.dims, c.batch, np.random.default_rng(0))
            else:
                net, mods, Pv, G, x, gy, masks = NC.operands(c, np.float64)
                P32 = Pv.astype(F32)
            dn = hold(NC.device_net(ctx, c.layers, c.dims, c.batch))
            wo, wn, bo, bn = dn.param_offsets(j)
            so = dn.param_offsets(i)[0]
            if not dry:
                P32[wo:wo + wn] = np.abs(P32[wo:wo + wn]) + F32(0.01)
                # nothing behind that layer may turn the +inf into a NaN on its way back: a sigmoid's y (1 - y) is finite and positive
                gy = np.abs(gy) + F32(0.1)
                gy.reshape(c.batch, -1)[0, gy[0].size // 2] = np.inf
                dn.params.copy_(torch.from_numpy(P32))
            dn.params_changed()
            md = [put(ctx, m) for m in NC.device_masks(c.layers, c.dims, [np.ones_like(m) for m in masks])]
            dn.forward(put(ctx, NC.to_device(x, first)), masks=md or None, train=True)
            dn.grads.fill_(0)
            dn.backward(put(ctx, NC.to_device(gy, outs[-1])), param_grads=True, input_grad=False)
            if not dry:
                got[fusion & 1] = dn.grads[so:so + 1].cpu().numpy().copy()
        finally:
            ctx.set_fusion(503)
    if dry:
        return []
    return [chk("%s: slope gradient of the un-fused PReLU backward under a +inf gradient" % name, got[0], np.array([unfused], F32), "class"),
            chk("%s: slope gradient of the fused form has the class of prelu_bwd_kernel's" % name, got[1], got[0], "class")]


for _name, _kernel, _unfused in SLOPE_CASES:
    case("slope-" + _name, 2, [_kernel, "prelu_bwd_kernel"])(lambda ctx, dry, _n=_name, _u=_unfused: run_slope_case(ctx, dry, _n, _u))


# ---------------------------------------------------------------------------------------------------------------------------------
# part 3: penalty, clamp and the optimizers
# ---------------------------------------------------------------------------------------------------------------------------------
G_PROBES = f32([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e20, -1e20, 1e-42, -1e-42, 0.0, -0.0, 0.3, -0.3])
P_PROBES = f32([0.0, -0.0, 1e-42, -1e-42, 2.0, -2.0, np.nan])
OPT_N = 4 * 13 * 4 + 3              # quads and a tail of three: the 16-byte form and the scalar tail of adam_kernel
OPT_SETTINGS = [dict(clamp=cl, l1=pen, l2=pen, gscale=gs) for cl in (0.0, 1.0) for pen in (0.0, 1e-4) for gs in (1.0, 0.5)]
ADAM = dict(lr=1e-3, b1=0.5, b2=0.9, eps=1e-3, ts=(1, 2, 1000))      # the hyper-parameters of OPT_CASES: every term of the update visible


def opt_probes(n, step=0):
    """-> (p, g): element i holds pair (i + 5 step) of the 13 x 7 cross product (n = 211 holds every pair at least twice, in different
    lanes of a quad); n = 3 takes three non-finite pairs"""
    k = (np.arange(n) + 5 * step) % (G_PROBES.size * P_PROBES.size) if n > 3 else np.array([0, 1 * 7 + 4, 3 * 7 + 6]) + 7 * step
    return P_PROBES[k % P_PROBES.size].copy(), G_PROBES[(k // P_PROBES.size) % G_PROBES.size].copy()


def sgn(p):
    return np.where(p > 0, F32(1), np.where(p < 0, F32(-1), F32(0))).astype(F32)


def prep_grad_ref(g, p, o):
    """fg_prep_grad: g gscale; + (sign(p) l1 + p l2) where a penalty is set; np.clip where the clamp is set -- a NaN stays a NaN"""
    with quiet():
        g = (g * F32(o["gscale"])).astype(F32)
        if o["l1"] != 0 or o["l2"] != 0:
            g = (g + ((sgn(p) * F32(o["l1"])).astype(F32) + (p * F32(o["l2"])).astype(F32)).astype(F32)).astype(F32)
        return np.clip(g, -F32(o["clamp"]), F32(o["clamp"])).astype(F32) if o["clamp"] != 0 else g


def adam_ref(p, g, m, v, o, t, hp=ADAM):
    """one step of fg_adam_math in float32, every product and sum rounded (the kernel is compiled with fp contract(off)); the three
    scalars in double as fg_adam_scalars makes them -> (p, m, v, g_out)"""
    step = F32(hp["lr"] * np.sqrt(1.0 - hp["b2"] ** t) / (1.0 - hp["b1"] ** t))
    ob1, ob2, b1, b2, eps = F32(1.0 - hp["b1"]), F32(1.0 - hp["b2"]), F32(hp["b1"]), F32(hp["b2"]), F32(hp["eps"])
    gp = prep_grad_ref(g, p, o)
    with quiet():
        m = ((m * b1).astype(F32) + (ob1 * gp).astype(F32)).astype(F32)
        v = ((v * b2).astype(F32) + ((ob2 * gp).astype(F32) * gp).astype(F32)).astype(F32)
        denom = (np.sqrt(v).astype(F32) + eps).astype(F32)
        u = (step * (m / denom).astype(F32)).astype(F32)
        return (p - u).astype(F32), m, v, gp


SGD = dict(lr=0.02, mom=0.9, damp=0.0, nesterov=1)


def sgd_ref(p, g, mom, o, first, hp=SGD):
    """sgd_kernel in float32, un-contracted -> (p, momentum buffer)"""
    d = prep_grad_ref(g, p, o)
    with quiet():
        mv = d if first else ((mom * F32(hp["mom"])).astype(F32) + (F32(1.0 - hp["damp"]) * d).astype(F32)).astype(F32)
        d = (d + (F32(hp["mom"]) * mv).astype(F32)).astype(F32) if hp["nesterov"] else mv
        return (p - (F32(hp["lr"]) * d).astype(F32)).astype(F32), mv


def adagrad_ref(p, g, var, o, clr=1e-3):
    d = prep_grad_ref(g, p, o)
    with quiet():
        v = (var + (d * d).astype(F32)).astype(F32)
        return (p - (F32(clr) * (d / (np.sqrt(v).astype(F32) + F32(1e-10)).astype(F32)).astype(F32)).astype(F32)).astype(F32), v


ULPS = 4                            # roundings a contraction can move between the restatement and the kernel, per element and step


def magnitude(*arrays):
    """elementwise largest finite magnitude among the operands of an update"""
    with quiet():
        return np.max([np.abs(np.nan_to_num(a.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)) for a in arrays], axis=0)


def scaled_bar(scale, atol):
    """the absolute bar of test_optimizer_options wherever ULPS ulps of the operands lie under it (up to a magnitude of about 20 for
    1e-5: every clamp-on setting); beyond, ULPS x 2^-23 x the largest operand magnitude the element has seen -- a contraction moves
    a sum by an ulp of its operands, which no absolute 1e-5 can hold at 1e20, and a cancelling sum keeps that error"""
    return np.maximum(atol, ULPS * 2.0 ** -23 * scale)


def rule_checks(tag, o, p0, g, pn, state, gout):
    """the rule of the header, stated without the restatement: a NaN gradient gives NaN everywhere; +-inf under a clamp gives +-clamp"""
    res = []
    isn = np.isnan(g)
    want = lambda a: np.where(isn, F32(np.nan), a.cpu().numpy()).astype(F32)
    for what, a in [("parameter", pn)] + list(state) + ([("g_out", gout)] if gout is not None else []):
        res.append(chk("%s: a NaN gradient gives a NaN %s" % (tag, what), a, want(a), "nanbits", dict(g=g, p=p0)))
    if gout is not None and o["clamp"] != 0:
        sel = np.isinf(g) & ~np.isnan(p0)
        gg = gout.cpu().numpy()
        res.append(chk("%s: +-inf under the clamp gives +-clamp" % tag, gg, np.where(sel, np.sign(g) * F32(o["clamp"]), gg).astype(F32), "nanbits", dict(g=g, p=p0)))
    return res


def setting_tag(o):
    return "clamp %g, l1 = l2 = %g, gscale %g" % (o["clamp"], o["l1"], o["gscale"])


def run_adam_n(ctx, dry, n):
    res = []
    for o in OPT_SETTINGS:
        p0, _ = opt_probes(n)
        pd, md, vd = off1(ctx, p0), off1(ctx, np.zeros(n)), off1(ctx, np.zeros(n))
        pr, mr, vr = p0.copy(), np.zeros(n, F32), np.zeros(n, F32)
        for s, t in enumerate(ADAM["ts"]):
            _, g = opt_probes(n, s)
            go = out1(ctx, n)
            before = pr.copy()
            ctx.check(ctx.lib.fg_adam_fused(ctx.h, P(pd), P(off1(ctx, g)), P(md), P(vd), n, o["gscale"], o["l1"], o["l2"], o["clamp"],
                                            ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], t, P(go)))
            if dry:
                continue
            pr, mr, vr, gr = adam_ref(pr, g, mr, vr, o, t)
            tag = "adam n=%d t=%d, %s" % (n, t, setting_tag(o))
            src = dict(g=g, p=before)
            res += [chk(tag + ": p", pd.clone(), pr, "nanbits", src), chk(tag + ": m", md.clone(), mr, "nanbits", src),
                    chk(tag + ": v", vd.clone(), vr, "nanbits", src), chk(tag + ": g_out", go.clone(), gr, "nanbits", src)]
            if s == 0:
                res += rule_checks(tag, o, before, g, pd.clone(), [("first moment", md.clone()), ("second moment", vd.clone())], go.clone())
    return res


@case("adam", 3, ["adam_kernel"])
def run_adam(ctx, dry):
    return run_adam_n(ctx, dry, OPT_N)


@case("adam-n3", 3, ["adam_kernel"])
def run_adam3(ctx, dry):
    return run_adam_n(ctx, dry, 3)


@case("sgd-adagrad", 3, ["sgd_kernel", "adagrad_kernel"])
def run_sgd_adagrad(ctx, dry):
    res, n = [], OPT_N
    for o in OPT_SETTINGS:
        p0, _ = opt_probes(n)
        ps, mom, pa, var = off1(ctx, p0), off1(ctx, np.zeros(n)), off1(ctx, p0), off1(ctx, np.zeros(n))
        psr, momr, par, varr = p0.copy(), np.zeros(n, F32), p0.copy(), np.zeros(n, F32)
        seen_s, seen_a = magnitude(p0), magnitude(p0)
        for s in range(3):
            _, g = opt_probes(n, s)
            gd = off1(ctx, g)
            ctx.check(ctx.lib.fg_sgd_fused(ctx.h, P(ps), P(gd), P(mom), n, o["gscale"], o["l1"], o["l2"], o["clamp"], SGD["lr"], SGD["mom"],
                                           SGD["damp"], 0.0, SGD["nesterov"], 1 if s == 0 else 0))
            ctx.check(ctx.lib.fg_adagrad_fused(ctx.h, P(pa), P(gd), P(var), n, o["gscale"], o["l1"], o["l2"], o["clamp"], 1e-3))
            if dry:
                continue
            b_s, b_a = psr.copy(), par.copy()
            psr, momr = sgd_ref(psr, g, momr, o, s == 0)
            par, varr = adagrad_ref(par, g, varr, o)
            tag = "step %d, %s" % (s, setting_tag(o))
            seen_s = magnitude(seen_s, prep_grad_ref(g, b_s, o), psr, momr)
            seen_a = magnitude(seen_a, par)
            res += [chk("sgd %s: p" % tag, ps.clone(), psr, "class", dict(g=g, p=b_s), atol=scaled_bar(seen_s, 1e-5)),
                    chk("sgd %s: momentum buffer" % tag, mom.clone(), momr, "class", dict(g=g, p=b_s), atol=scaled_bar(seen_s, 1e-5)),
                    chk("adagrad %s: p" % tag, pa.clone(), par, "class", dict(g=g, p=b_a), atol=scaled_bar(seen_a, 1e-6)),
                    chk("adagrad %s: variance" % tag, var.clone(), varr, "class", dict(g=g, p=b_a), rtol=1e-5)]
            if s == 0:
                res += rule_checks("sgd " + tag, o, b_s, g, ps.clone(), [("momentum buffer", mom.clone())], None)
                res += rule_checks("adagrad " + tag, o, b_a, g, pa.clone(), [("variance", var.clone())], None)
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# part 4: reductions and the edges of the remaining entries
# ---------------------------------------------------------------------------------------------------------------------------------
NORMS_N = 1003


def norms_cases():
    base = np.random.default_rng(4).standard_normal(NORMS_N).astype(F32)
    one = lambda v: np.concatenate([base[:500], f32([v]), base[501:]])
    return [("one NaN", one(np.nan)), ("one +inf", one(np.inf)), ("one -inf", one(-np.inf)), ("all 2e19: the squares overflow", np.full(NORMS_N, 2e19, F32)),
            ("all 1.5e19: the squares are finite, their sum is not", np.full(NORMS_N, 1.5e19, F32)),
            ("all 1e-30: the squares underflow to zero", np.full(NORMS_N, 1e-30, F32)), ("all 1e-20: the squares are subnormal", np.full(NORMS_N, -1e-20, F32))]


def norms_ref(v):
    """float64 sums of |v| and of the fp32-rounded squares, stored as fp32: inf wherever the sum exceeds FLT_MAX, although the norm
    itself (its square root) is finite"""
    with quiet():
        return np.array([np.abs(v.astype(np.float64)).sum(), (v * v).astype(F32).astype(np.float64).sum()]).astype(F32)


@case("norms", 4, ["norms_partial_kernel", "norms_final_kernel"])
def run_norms(ctx, dry):
    res = []
    for what, v in norms_cases():
        o = out(ctx, 2)
        ctx.check(ctx.lib.fg_norms(ctx.h, P(off1(ctx, v)), v.size, P(o), P(out(ctx, 1024))))
        if not dry:
            # an FMA keeps the exact square where the reference rounds it to the subnormal grid: up to 2^-150 per term
            res.append(chk("norms, " + what, o, norms_ref(v), "class", dict(v=v[0]), atol=v.size * 2.0 ** -149, rtol=BAR["norms_rtol"]))
    return res


BCE_PROBS = f32([np.nan, -0.0, 1 + 2.0 ** -23, -1e-3, 0.0, 1.0, 0.5, 1e-13])
BCE_NS = (1, 5, 257)


def bce_ref(x, t):
    """bce_kernel in float32 (the loss summed in float64) -> (loss, grad, confusion[4])"""
    B, eps = x.size, F32(1e-12)
    with quiet():
        a, b = (x + eps).astype(F32), ((F32(1) - x).astype(F32) + eps).astype(F32)
        terms = ((t * np.log(a).astype(F32)).astype(F32) + ((F32(1) - t).astype(F32) * np.log(b).astype(F32)).astype(F32)).astype(F32)
        loss = F32(-(terms.astype(np.float64).sum()) / B)
        grad = ((-(t - x).astype(F32) / (b * a).astype(F32)).astype(F32) / F32(B)).astype(F32)
        conf = np.bincount(np.where(x > 0.5, 2, 0) + np.where(t > 0.5, 1, 0), minlength=4).astype(np.int32)
    return np.array([loss], F32), grad, conf


def bce_cases():
    """-> [(what, probabilities, targets)]: every probe alone with either target (n = 1); n = 5 and 257 with and without the NaN"""
    res = [("n=1 p=%r t=%d" % (float(p), t), f32([p]), f32([t])) for p in BCE_PROBS for t in (0, 1)]
    for n in BCE_NS[1:]:
        for lo in (0, 1):
            k = np.arange(n)
            res.append(("n=%d %s" % (n, "with NaN" if lo == 0 else "without NaN"), BCE_PROBS[lo + k % (BCE_PROBS.size - lo)].copy(), ((k // 3) % 2).astype(F32)))
    return res


@case("bce", 4, ["bce_kernel"])
def run_bce(ctx, dry):
    res = []
    for what, x, t in bce_cases():
        n = x.size
        loss, grad = out(ctx, 1), out1(ctx, n)
        conf = hold(torch.full((4,), -1, dtype=torch.int32, device=ctx.device))
        ctx.check(ctx.lib.fg_bce_forward_backward(ctx.h, P(off1(ctx, x)), P(off1(ctx, t)), n, P(loss), P(grad), P(conf)))
        if dry:
            continue
        rl, rg, rc = bce_ref(x, t)
        res += [chk("bce loss, " + what, loss, rl, "class", dict(p=x[0], t=t[0]), rtol=1e-5),
                chk("bce gradient, " + what, grad, rg, "class", dict(p=x, t=t), atol=1e-7, rtol=1e-5),
                chk("bce confusion counts, " + what, conf.cpu().numpy().astype(F32), rc.astype(F32), "bits", dict(p=x[0], t=t[0]))]
    return res


PARZEN = (5, 300)                   # n examples of 300 elements


def parzen_cases():
    n, e = PARZEN
    r = np.random.default_rng(8)
    gen, cond, fine = (r.standard_normal(s).astype(F32) for s in ((n, e), (e,), (e,)))
    def with_(rows, v):
        g = gen.copy()
        for i in rows: g[i, 17 * (i + 1)] = v
        return g
    return [("one NaN distance", with_([2], np.nan), cond, fine), ("every distance NaN", with_(range(n), np.nan), cond, fine),
            ("one -inf element", with_([1], -np.inf), cond, fine), ("NaN in the nearest row", with_([int(np.argmin(((gen + cond - fine) ** 2).sum(1)))], np.nan), cond, fine)]


def parzen_ref(gen, cond, fine):
    """dist[i] = sqrt(sum_e ((gen + cond) - fine)^2): the two differences in fp32, the sum in float64; min = fmin over (1e10, dist)"""
    with quiet():
        d = ((gen + cond).astype(F32) - fine).astype(F32).astype(np.float64)
        dist = np.sqrt((d * d).sum(1)).astype(F32)
    return dist, np.array([np.fmin.reduce(np.concatenate([f32([1e10]), dist]))], F32)


@case("parzen", 4, ["parzen_dist_kernel", "min_kernel"])
def run_parzen(ctx, dry):
    res = []
    n, e = PARZEN
    for what, gen, cond, fine in parzen_cases():
        dist, mn = out(ctx, n), out(ctx, 1)
        ctx.check(ctx.lib.fg_parzen_min_dist(ctx.h, P(put(ctx, gen)), P(put(ctx, cond)), P(put(ctx, fine)), n, e, P(dist), P(mn)))
        if dry:
            continue
        rd, rm = parzen_ref(gen, cond, fine)
        res += [chk("parzen distances, " + what, dist, rd, "class", rtol=1e-6), chk("parzen minimum: a NaN never wins, " + what, mn, rm, "class", rtol=1e-6)]
    return res


GRID = dict(k=4, c=3, h=5, w=6, nrow=2, padding=2)


def grid_cases():
    k, c, h, w = GRID["k"], GRID["c"], GRID["h"], GRID["w"]
    img = np.random.default_rng(9).uniform(-1, 1, (k, h, w, c)).astype(F32)
    def with_(v):
        a = img.copy()
        a[2, 3, 1, 2] = v
        return a
    return [("constant images", np.full_like(img, 0.375)), ("one NaN pixel", with_(np.nan)), ("one +inf pixel", with_(np.inf)), ("one -inf pixel", with_(-np.inf)),
            ("all -0", np.full_like(img, -0.0)), ("all NaN", np.full_like(img, np.nan))]


def grid_ref(img, normalize=1):
    """grid_minmax_kernel + grid_fill_kernel: fmin / fmax extrema (a NaN pixel is ignored; no finite pixel: +inf, -inf), padding = max,
    v = max == min ? 0 : (v - min) / (max - min) in fp32 -> (grid [c][GH][GW], [min, max])"""
    k, c, h, w, nrow, pad = (GRID[q] for q in ("k", "c", "h", "w", "nrow", "padding"))
    mn = np.fmin.reduce(np.concatenate([f32([np.inf]), img.reshape(-1)]))
    mx = np.fmax.reduce(np.concatenate([f32([-np.inf]), img.reshape(-1)]))
    xmaps = min(nrow, k)
    ymaps = (k + xmaps - 1) // xmaps
    g = np.full((c, ymaps * (h + pad), xmaps * (w + pad)), mx, F32)
    for j in range(k):
        y0, x0 = (j // xmaps) * (h + pad) + pad // 2, (j % xmaps) * (w + pad) + pad // 2
        g[:, y0:y0 + h, x0:x0 + w] = img[j].transpose(2, 0, 1)
    if normalize:
        with quiet():
            g = np.zeros_like(g) if mx == mn else ((g - mn).astype(F32) / (mx - mn)).astype(F32)
    return g, f32([mn, mx])


@case("image-grid", 4, ["grid_minmax_kernel", "grid_fill_kernel"])
def run_grid(ctx, dry):
    res = []
    k, c, h, w, nrow, pad = (GRID[q] for q in ("k", "c", "h", "w", "nrow", "padding"))
    order = hold(torch.arange(k, dtype=torch.int32).to(ctx.device))
    for what, img in grid_cases():
        rg, rmm = grid_ref(img)
        grid, mm = out(ctx, rg.size), out(ctx, 2)
        ctx.check(ctx.lib.fg_image_grid(ctx.h, P(put(ctx, img)), P(order), k, c, h, w, nrow, pad, 1, P(grid), P(mm)))
        if not dry:
            res += [chk("image grid, " + what, grid, rg, "nanbits"), chk("image grid extrema, " + what, mm, rmm, "bits")]
    return res


# ---- Philox at its extreme words ----------------------------------------------------------------------------------------------------
# found by philox_search() (the host test re-derives them): the first counters of seed 1 whose quad holds a word with (word >> 8) ==
# 0xFFFFFF (u = 1 - 2^-24, the largest uniform) and == 0 (u = 0)
RNG_SEED = 1
RNG_MAX = (6318945, 1)              # (offset = counter of the quad, word)
RNG_ZERO = (10460476, 3)
RNG_SEARCH = 11 << 20               # counters searched
RNG_PAIRS = ((-1.0, 1.0), (0.0, 1.0), (0.5, 1.5))
TWO_M24 = 2.0 ** -24


def philox_search(seed=RNG_SEED, upto=RNG_SEARCH, chunk=1 << 20):
    """-> (first (counter, word) with word >> 8 == 0xFFFFFF, first with word >> 8 == 0) over counters 0 .. upto"""
    import test_gpu_pointwise_paths as TQ
    hi = lo = None
    for c0 in range(0, upto, chunk):
        w = TQ.philox_words(seed, c0, chunk) >> 8
        for want, name in ((0xFFFFFF, "hi"), (0, "lo")):
            at = np.argwhere(w == want)
            if at.size and (hi if name == "hi" else lo) is None:
                v = (c0 + int(at[0][0]), int(at[0][1]))
                hi, lo = (v, lo) if name == "hi" else (hi, v)
    return hi, lo


def uniform_ref(words, lo, hi):
    """rng_kernel mode 0: lo + u (hi - lo), u = (word >> 8) 2^-24.  For the three pairs hi - lo is a power of two: the product is exact
    and a contraction cannot move a bit"""
    with quiet():
        u = ((words >> 8).astype(F32) * F32(TWO_M24)).astype(F32)
        return (F32(lo) + (u * (F32(hi) - F32(lo))).astype(F32)).astype(F32)


def rng_draws(ctx, offset):
    """-> {name: device tensor of 4 draws at this counter}"""
    lib, h, n = ctx.lib, ctx.h, 4
    res = {}
    for lo, hi in RNG_PAIRS:
        res["uniform(%g, %g)" % (lo, hi)] = o = out1(ctx, n)
        ctx.check(lib.fg_rng_uniform(h, RNG_SEED, offset, P(o), n, lo, hi))
    for keep in (0.0, 1.0, TWO_M24):
        res["bernoulli(%r)" % keep] = o = out1(ctx, n)
        ctx.check(lib.fg_rng_bernoulli(h, RNG_SEED, offset, P(o), n, keep))
    res["normal"] = o = out1(ctx, n)
    ctx.check(lib.fg_rng_normal(h, RNG_SEED, offset, P(o), n, 0.0, 1.0))
    return res


@case("rng-extremes", 4, ["rng_kernel"])
def run_rng(ctx, dry):
    import test_gpu_pointwise_paths as TQ
    res = []
    for what, (offset, word) in (("largest word", RNG_MAX), ("zero word", RNG_ZERO)):
        d = rng_draws(ctx, offset)
        if dry:
            continue
        w = TQ.philox_words(RNG_SEED, offset, 1).reshape(-1)
        u = ((w >> 8).astype(F32) * F32(TWO_M24)).astype(F32)
        for lo, hi in RNG_PAIRS:
            res.append(chk("%s: uniform(%g, %g)" % (what, lo, hi), d["uniform(%g, %g)" % (lo, hi)], uniform_ref(w, lo, hi), "bits", dict(word=w.astype(F32))))
        for keep in (0.0, 1.0, TWO_M24):
            res.append(chk("%s: bernoulli(keep = %r) is u < keep" % (what, keep), d["bernoulli(%r)" % keep], (u < F32(keep)).astype(F32), "bits", dict(u=u)))
        ref = TQ.box_muller(w, np.float64)
        assert np.isfinite(ref).all()
        res.append(chk("%s: normal is finite and within the measured bar" % what, d["normal"], ref, "close", dict(word=w.astype(F32)), atol=TQ.measured_normal_bar()))
    return res


# ---- the step level: the fused Adam + re-pack launch, a NaN through fg_step_D / fg_step_G, the library's own draws ---------------------
FG_FUSE_ADAM_PACK = 8
GAN_ADAM_CASE = "r1-3x3x3-b2-6-8"     # D: 176 parameters under Adam (gan_cases.ADAM_D); all 91 probe pairs fit


def gan_case(name, **kw):
    import gan_cases as GC
    return GC.BY_NAME[name]._replace(**kw)


def gan_device_inputs(ctx, case, it, edit=None):
    """tests/test_gpu_gan_steps.py device_inputs, with `edit(inputs)` applied to the oracle-shaped arrays first -> (arrays, device dict)"""
    import gan_cases as GC
    import net_cases as NC
    inp = GC.inputs(case, it)
    if edit:
        edit(inp)
    first = NC.walk(case.dlayers, case.ddims)[0]
    img = lambda k: put(ctx, NC.to_device(inp[k], first)) if k in inp else None
    nz = lambda k: put(ctx, inp[k].transpose(0, 2, 3, 1) if case.table else inp[k])
    masks = lambda k: [put(ctx, m) for m in NC.device_masks(case.dlayers, case.ddims, inp[k])]
    return inp, dict(B=inp["B"], real=img("real"), cond_real=img("cond_real"), cond_fake=img("cond_fake"), cond=img("cond"), noiseD=nz("noiseD"),
                     noiseG=nz("noiseG"), masksD=masks("masksD"), masksG=masks("masksG"))


def load_gan(st, gan):
    for dn, pv in ((gan.dnG, st.pG), (gan.dnD, st.pD)):
        dn.params.copy_(torch.from_numpy(pv.astype(F32)))
        dn.params_changed()


@case("gan-adam-pack", 3, ["pack_jobs_kernel"])
def run_gan_adam_pack(ctx, dry):
    """fg_gan_update on D's flat vectors holding the probes: the fused penalty + clamp + Adam + re-pack launch (FG_FUSE_ADAM_PACK) gives
    the bits of the restatement, as adam_kernel does"""
    import gan_cases as GC
    base = gan_case(GAN_ADAM_CASE)
    hp = dict(lr=base.optD[1]["learningRate"], b1=base.optD[1]["beta1"], b2=base.optD[1]["beta2"], eps=base.optD[1]["epsilon"])
    res = []
    ctx.set_fusion(503 | FG_FUSE_ADAM_PACK)
    try:
        for o in [o for o in OPT_SETTINGS if o["gscale"] == 1.0]:           # (gscale is 1 / world: one rank)
            c = base._replace(pen=dict(base.pen, D_L1=o["l1"], D_L2=o["l2"], D_clamp=o["clamp"]))
            gan = hold(GC.device_gan(ctx, c))
            n = gan.dnD.n_params
            inp, d = gan_device_inputs(ctx, c, 0)
            if not dry:
                load_gan(GC.oracle_gan(c), gan)
            pr, mr, vr = opt_probes(n)[0], np.zeros(n, F32), np.zeros(n, F32)
            for s in range(3):
                gan.step_D(d["B"], d["real"], None, None, d["noiseD"], None, gan.NO_UPDATE)      # leaves "gradients pending"
                _, g = opt_probes(n, s)
                if s == 0:
                    gan.dnD.params.copy_(torch.from_numpy(pr))
                gan.dnD.grads.copy_(torch.from_numpy(g))
                gan.update(0)
                if dry:
                    continue
                before = pr
                pr, mr, vr, _ = adam_ref(pr, g, mr, vr, o, s + 1, hp)
                st = gan.view("OPT_STATE_D").clone()
                tag, src = "fused Adam + re-pack t=%d, %s" % (s + 1, setting_tag(o)), dict(g=g, p=before)
                res += [chk(tag + ": p", gan.dnD.params.clone(), pr, "nanbits", src), chk(tag + ": m", st[:n], mr, "nanbits", src), chk(tag + ": v", st[n:2 * n], vr, "nanbits", src)]
                if s == 0:
                    res += rule_checks(tag, o, before, g, gan.dnD.params.clone(), [("first moment", st[:n].clone()), ("second moment", st[n:2 * n].clone())], None)
    finally:
        ctx.set_fusion(503)
    return res


E2E_RULES = [("adam", dict(learningRate=2e-3, beta1=0.5, beta2=0.99, epsilon=1e-6)), ("sgd", dict(learningRate=0.05, momentum=0.9)), ("adagrad", dict(learningRate=0.02))]
E2E_CASES = ("r1-3x3x3-b2-6-8", "r4-table-1ch")


def e2e_edit(which):
    def edit(inp):
        a = inp["real"] if which == "D" else inp["noiseG"]
        a.reshape(a.shape[0], -1)[0, a[0].size // 2] = np.nan
    return edit


def e2e_oracle(case, which):
    """the oracle's run of the same closure on the same inputs -> (its result dict, NaN set of the stepped net's parameters)"""
    import gan_cases as GC
    st = GC.oracle_gan(case)
    inp = GC.inputs(case, 0)
    e2e_edit(which)(inp)
    with quiet():
        ref = GC.oracle_step(st, case, which, inp, inp["masks" + which])
    return st, ref, np.isnan(st.pD if which == "D" else st.pG)


def run_e2e(ctx, dry, name):
    import gan_cases as GC
    res = []
    for rule in E2E_RULES:
        c = gan_case(name, optD=rule, optG=rule)
        assert c.pen["D_clamp"] == 1.0 and c.pen["G_clamp"] == 5.0          # train.lua's defaults
        for which in "DG":
            gan = hold(GC.device_gan(ctx, c))
            inp, d = gan_device_inputs(ctx, c, 0, e2e_edit(which))
            if not dry:
                load_gan(GC.oracle_gan(c), gan)
            dn, other = (gan.dnD, gan.dnG) if which == "D" else (gan.dnG, gan.dnD)
            o0, os0 = other.params.clone(), gan.view("OPT_STATE_" + "GD"["DG".index(which)]).clone()
            if which == "D":
                gan.step_D(d["B"], d["real"], d["cond_real"], d["cond_fake"], d["noiseD"], d["masksD"] or None)
            else:
                gan.step_G(d["B"], d["cond"], d["noiseG"], d["masksG"] or None)
            if dry:
                continue
            _, _, reached = e2e_oracle(c, which)
            tag = "%s, %s, %s-step with one NaN %s" % (name, rule[0], which, "pixel" if which == "D" else "noise element")
            p1 = dn.params.cpu().numpy()
            res += [chk(tag + ": FG_GAN_LOSS is NaN", gan.view("LOSS")["DG".index(which):][:1].clone(), f32([np.nan]), "nanbits"),
                    chk(tag + ": every parameter the NaN reaches (the oracle's set) is NaN", np.where(np.isnan(p1), F32(np.nan), F32(0)),
                        np.where(reached, F32(np.nan), F32(0)), "nanbits", dict(parameter_after=p1)),
                    chk(tag + ": the other net keeps its bits", other.params.clone(), o0.cpu().numpy(), "bits"),
                    chk(tag + ": the other net's optimizer state keeps its bits", gan.view("OPT_STATE_" + "GD"["DG".index(which)]).clone(), os0.cpu().numpy(), "bits")]
    return res


for _name in E2E_CASES:
    case("nan-step-" + _name, 3, ["bce_kernel", "adam_kernel", "sgd_kernel", "adagrad_kernel"])(lambda ctx, dry, _n=_name: run_e2e(ctx, dry, _n))


RNG_MULTI_CASE = "r5-one-dropout-library"


@case("rng-multi-extremes", 4, ["rng_multi_kernel"])
def run_rng_multi(ctx, dry):
    """the noise and the dropout mask of one D-step drawn by the library in ONE two-segment launch, keyed at the extreme counters: the
    noise of nn_utils.lua:9's range (-1, 1) at the largest word, Bernoulli(0.5) at the zero word"""
    import gan_cases as GC
    import test_gpu_pointwise_paths as TQ
    c = gan_case(RNG_MULTI_CASE)
    gan = hold(GC.device_gan(ctx, c))
    gan.set_seeds(RNG_SEED, RNG_MAX[0], RNG_SEED, RNG_ZERO[0])
    inp, d = gan_device_inputs(ctx, c, 0)
    B = d["B"]
    gan.step_D(B, d["real"])
    if dry:
        return []
    n = B // 2 * c.gdims[0]
    wn = TQ.philox_words(RNG_SEED, RNG_MAX[0], (n + 3) // 4).reshape(-1)[:n]
    m = gan.mask_view(0, B)
    wm = TQ.philox_words(RNG_SEED, RNG_ZERO[0], (m.numel() + 3) // 4).reshape(-1)[:m.numel()]
    keep = F32(ctx.lib.fg_net_mask_keep(gan.dnD.h, 0))
    noise = gan.view("NOISE", n).clone()
    um = ((wm >> 8).astype(F32) * F32(TWO_M24)).astype(F32)
    return [chk("rng_multi: uniform(-1, 1) at the largest word", noise, uniform_ref(wn, -1.0, 1.0), "bits", dict(word=wn.astype(F32))),
            chk("rng_multi: the noise range (-1, 1) never yields 1", (noise.cpu().numpy() < 1).astype(F32), np.ones(n, F32), "bits", dict(word=wn.astype(F32))),
            chk("rng_multi: bernoulli(keep) at the zero word", m.clone(), (um < keep).astype(F32), "bits", dict(u=um))]


BY_NAME = {c.name: c for c in CASES}


def run_case(ctx, c, dry=False):
    del KEEP[:]
    return c.run(ctx, dry)
