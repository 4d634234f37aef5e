"""The value domain of the contraction kernels and of BatchNorm (tests/VALUE_DOMAIN.md): case lists, float64 / numpy references and
a-priori bounds shared by tests/test_gpu_value_domain.py (device) and tests/test_value_domain_host.py (CPU).

One case per kernel family at the smallest geometry of the existing parity lists that reaches it (PATH_CASES, wino.CASES / UP_CASES /
WGRAD_CASES, BF16X6_SHAPES, LINEAR_CASES), under the math mode, fusion bits and hook of its source; `expect` names the kernel every
pass must launch (asserted planning-only by the host test).  Everything in here is numpy / torch-CPU; nothing touches a device."""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32, U32 = np.float32, np.uint32
U = 2.0 ** -24                      # unit roundoff of fp32
D = 503                             # FG_FUSE_DEFAULT
NOWINO = D & ~(32 | 64 | 128 | 256)
NOWINO_FWD = D & ~(32 | 64 | 128)   # tests/test_gpu_math_modes.py runs BF16X6_SHAPES with these bits cleared

VCase = collections.namedtuple("VCase", "name kind shape math fusion hook wino expect")


def vc(name, kind, shape, expect, math=0, fusion=D, hook=False, wino=()):
    return VCase(name, kind, tuple(shape), math, fusion, hook, tuple(wino), expect)


# expect: {pass: kernel name that must be among the launches of that pass}; only the passes named are run.
# wino: the passes that run in the Winograd domain (their bound is wino_bound's, their non-finite sets may dilate by a tile).
VCASES = [
    # ---- implicit GEMM on the fp32 matrix pipe
    vc("ws-lin", "lin", (16384, 32, 512), dict(fwd="igemm_ws_kernel")),                                            # PATH_CASES ws256x128-lin
    vc("ws64x3-lin", "lin", (8192, 32, 512), dict(fwd="igemm_ws64x3_kernel", dgrad="igemm_kernel", wgrad="wgrad_kernel")),   # ws64x3-tile5-lin; split-K dgrad
    vc("wgrad-ws", "conv", (16, 16, 16, 256, 128, 5, 1), dict(wgrad="wgrad_ws_kernel"), fusion=NOWINO_FWD),       # BF16X6_SHAPES[3], mode 0
    # ---- bf16x6 (mode 6): both tiles of igemm_ws6, forward and data gradient, with and without split-K; wgrad6
    vc("ws6-128-lin", "lin", (16384, 32, 512), dict(fwd="igemm_ws6_kernel"), math=6),                              # <128>, un-split
    vc("ws6-64-lin", "lin", (65536, 16, 64), dict(fwd="igemm_ws6_kernel", dgrad="igemm_ws6_kernel"), math=6),     # <64>, un-split (ws6-n64-lin)
    vc("ws6-64-splitk", "conv", (32, 16, 16, 16, 512, 3, 0), dict(fwd="igemm_kernel", dgrad="igemm_ws6_kernel"), math=6, fusion=NOWINO),   # ws6-splitk-16to512
    vc("ws6-128-splitk", "conv", (16, 16, 16, 256, 128, 5, 1), dict(fwd="igemm_ws6_kernel", dgrad="igemm_ws6_kernel", wgrad="wgrad_ws6_kernel"),
       math=6, fusion=NOWINO_FWD),                                                                                # BF16X6_SHAPES[3]: <128> split-K + wgrad6
    # ---- Winograd F(2x2, 3x3): 3x3, 5x5 (four groups), folded up-convolution (four parities / four stride-2 groups), weight gradient
    vc("wino-3x3", "conv", (2, 6, 10, 16, 24, 3, 0), dict(fwd="wino_kernel", dgrad="wino_kernel"), wino=("fwd", "dgrad")),     # wino.CASES[3]
    vc("wino-5x5", "conv", (2, 4, 8, 8, 8, 5, 0), dict(fwd="wino_kernel", dgrad="wino_kernel"), wino=("fwd", "dgrad")),        # wino.UP_CASES[8]
    vc("wino-up", "conv", (5, 6, 10, 16, 24, 5, 1), dict(fwd="wino_kernel", dgrad="wino_kernel"), wino=("fwd", "dgrad")),      # wino.UP_CASES[4]
    vc("wino-wgrad", "conv", (5, 4, 4, 128, 64, 3, 0), dict(wgrad="wino_wgrad_kernel"), hook=True, wino=("wgrad",)),           # wino.WGRAD_CASES[2]
    # ---- thin layers and the gemv pair
    vc("thin-slab", "conv", (4, 34, 24, 1, 64, 3, 0), dict(fwd="thin_in_mfma_kernel", dgrad="thin_out_slab_mfma_kernel", wgrad="thin_wgrad_mfma_kernel")),   # slab11-34x24
    vc("thin-tiled", "conv", (2, 33, 37, 3, 256, 3, 0), dict(fwd="thin_in_mfma_kernel", dgrad="thin_out_tiled_kernel", wgrad="thin_wgrad_mfma_kernel")),    # tiled33-33x37
    vc("gemv", "lin", (300, 606, 1), dict(fwd="gemv_fwd_kernel", dgrad="gemv_bwd_kernel", wgrad="gemv_bwd_kernel")),           # gemv-b300
]
BY_NAME = {c.name: c for c in VCASES}
PASS_ORDER = ("fwd", "dgrad", "wgrad")


def passes(c):
    return [p for p in PASS_ORDER if p in c.expect]


def mode6(c, p):
    """does pass p of the case run on split bf16 planes (the documented domain of fg_set_math(6))?"""
    return c.math == 6 and "6" in c.expect[p]


def seed(c, salt=0):
    return zlib.crc32(("%s/%d" % (c.name, salt)).encode())


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry, operands, float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def shapes(c):
    """-> dict(x=, w=, gy=) operand shapes (NHWC activations, reference weight layout)"""
    if c.kind == "lin":
        B, K, N = c.shape
        return dict(x=(B, K), w=(N, K), gy=(B, N))
    B, H, W, Cin, Cout, k, up = c.shape
    f = 2 if up else 1
    return dict(x=(B, H, W, Cin), w=(Cout, Cin, k, k), gy=(B, H * f, W * f, Cout))


def fan_in(c):
    return c.shape[1] if c.kind == "lin" else c.shape[3] * c.shape[5] ** 2


def reduction_length(c, p):
    """K of the a-priori bound: the number of products summed into one output"""
    if c.kind == "lin":
        B, K, N = c.shape
        return dict(fwd=K, dgrad=N, wgrad=B)[p]
    B, H, W, Cin, Cout, k, up = c.shape
    f2 = 4 if up else 1
    return dict(fwd=Cin * k * k, dgrad=Cout * k * k * f2, wgrad=B * H * W * f2)[p]


def unit_operands(c, salt=0):
    """the operands of the existing parity tests: standard-normal activations and gradients, uniform(-1/sqrt(fan_in), ..) weights"""
    rng = np.random.default_rng(seed(c, salt))
    s = shapes(c)
    b = 1.0 / np.sqrt(fan_in(c))
    return dict(x=rng.standard_normal(s["x"]).astype(F32), w=rng.uniform(-b, b, s["w"]).astype(F32), gy=rng.standard_normal(s["gy"]).astype(F32))


def wide_operands(c):
    """N(0, 1) * 2^e, e drawn per element: uniform in -12 .. 12 for activations and gradients, -6 .. 6 (times 1/sqrt(fan_in)) for weights"""
    rng = np.random.default_rng(seed(c, 7))
    s = shapes(c)
    draw = lambda shape, e: np.ldexp(rng.standard_normal(shape), rng.integers(-e, e + 1, shape)).astype(F32)
    return dict(x=draw(s["x"], 12), w=(draw(s["w"], 6) * F32(1.0 / np.sqrt(fan_in(c)))).astype(F32), gy=draw(s["gy"], 12))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def reference(c, op, which=None):
    """float64 results of the passes in `which` (default: the case's own) on float32 operands, NHWC / reference weight layout"""
    which = passes(c) if which is None else which
    x, w, gy = t64(op["x"]), t64(op["w"]), t64(op["gy"])
    out = {}
    if c.kind == "lin":
        if "fwd" in which: out["fwd"] = x @ w.t()
        if "dgrad" in which: out["dgrad"] = gy @ w
        if "wgrad" in which: out["wgrad"] = gy.t() @ x
        return {p: v.numpy() for p, v in out.items()}
    B, H, W, Cin, Cout, k, up = c.shape
    pad = (k - 1) // 2
    xr, gyr = x.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2)
    if up: xr = F.interpolate(xr, scale_factor=2, mode="nearest")
    if "fwd" in which:
        out["fwd"] = F.conv2d(xr, w, None, padding=pad).permute(0, 2, 3, 1)
    if "dgrad" in which:
        g = F.conv_transpose2d(gyr, w, padding=pad)
        if up: g = g.reshape(B, Cin, H, 2, W, 2).sum((3, 5))
        out["dgrad"] = g.permute(0, 2, 3, 1)
    if "wgrad" in which:
        out["wgrad"] = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, k, k), gyr, padding=pad)
    return {p: v.contiguous().numpy() for p, v in out.items()}


def abs_operands(op):
    return {k: np.abs(v) for k, v in op.items()}


def direct_bound(c, op, which=None):
    """(K + 16) 2^-24 A per output, A = the same contraction of |x|, |w| in float64: holds for any summation order and split-K"""
    A = reference(c, abs_operands(op), which)
    return {p: (reduction_length(c, p) + 16) * U * a for p, a in A.items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


# ---------------------------------------------------------------------------------------------------------------------------------
# part 1: power-of-two homogeneity
# ---------------------------------------------------------------------------------------------------------------------------------
SCALES = [(40, -8), (-40, 8), (-30, -30)]


def scaled_operands(op, a, b):
    """forward (2^a x, 2^b w), data gradient (2^a gy, 2^b w), weight gradient (2^a x, 2^b gy): every pass scales by 2^(a + b)"""
    return dict(x=np.ldexp(op["x"], a), w=np.ldexp(op["w"], b), gy=np.ldexp(op["gy"], a), gy_wgrad=np.ldexp(op["gy"], b))


# ---------------------------------------------------------------------------------------------------------------------------------
# part 3: fg_split3 as specification, one-hot weights, probes
# ---------------------------------------------------------------------------------------------------------------------------------
SPLIT_MAX = 0x7f7f0000              # the largest magnitude whose high plane is finite: splits exactly
EXACT_MIN_EXP = -100                # 2^-100 <= |x|: the band the issue pins as an exact copy in both modes


def bf16_rn(v):
    """float32 array -> bf16 bit patterns (uint32, low 16 bits), round to nearest even; NaN in gives a quiet NaN out"""
    u = bits(v).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(U32)


def bf16_value(p):
    return (p.astype(U32) << 16).view(F32)


def split3(v):
    """-> (h, m, l) bf16 bit patterns: h = rn(v), m = rn(v - h), l = rn((v - h) - m), all in fp32 arithmetic (csrc/igemm.hip fg_split3)"""
    v = np.ascontiguousarray(v, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        h = bf16_rn(v)
        r1 = (v - bf16_value(h)).astype(F32)
        m = bf16_rn(r1)
        r2 = (r1 - bf16_value(m)).astype(F32)
        return h, m, bf16_rn(r2)


def bf16_rn_unguarded(v):
    """the rounding before the NaN guard: the carry wraps 0x7fff8000 .. 0x7fffffff to +0 (and the negative ones to -0)"""
    u = bits(v).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(U32)


def plane_is_subnormal(p):
    return ((p & 0x7f80) == 0) & ((p & 0x7f) != 0)


NAN_PROBES = [0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xffffffff, 0x7fff8000]
INF_PROBES = [0x7f800000, 0xff800000]
TOP_PROBES = [0x7f7f8000, 0x7f7fffff]          # finite, beyond the exact split: mode 0 copies them, mode 6 documents NaN


def finite_probes():
    """+-2^e for e in -149 .. 127 with a random mantissa where there is room, +-0 and the largest value that splits exactly (uint32 bits)"""
    rng = np.random.default_rng(1611)
    out = [0x00000000, 0x80000000, SPLIT_MAX, SPLIT_MAX | 0x80000000]
    for e in range(-149, 128):
        for s in (0, 0x80000000):
            if e >= -126:
                mant = int(rng.integers(0, 1 << 23))
                if e == 127: mant &= 0x7effff                 # stays below SPLIT_MAX
                out.append(s | ((e + 127) << 23) | mant)
            else:
                top = 1 << (e + 149)
                out.append(s | top | int(rng.integers(0, top)))
    return np.array(out, dtype=U32)


def edge_probes():
    return np.array(TOP_PROBES + INF_PROBES + NAN_PROBES, dtype=U32)


def probe_operand(c, p):
    """which operand carries the probes in pass p, and its minimum probe distance: k pixels, no two in one 4x4 Winograd patch (a
    stride-2 group of the folded data gradient spans 7 pixels)"""
    name = "x" if p == "fwd" else "gy"
    if c.kind == "lin":
        return name, 1
    k, up = c.shape[5], c.shape[6]
    return name, (8 if (up and p == "dgrad") else max(k, 4))


def observed_channels(c):
    """the one-hot pass copies operand channel (o mod C): only the first min(Cin, Cout) channels of the operand reach an output"""
    return min(c.shape[1], c.shape[2]) if c.kind == "lin" else min(c.shape[3], c.shape[4])


def probe_slots(shape, S, nch=None):
    """flat indices of the probe positions of an operand: per (sample, channel) plane a grid of step S whose origin walks through all
    residues (every tile row / column residue, the first and the last tile), so no two probes of a plane share a window; only the
    first nch channels carry probes"""
    nch = shape[-1] if nch is None else nch
    if len(shape) == 2:
        return (np.arange(shape[0])[:, None] * shape[1] + np.arange(nch)[None, :]).reshape(-1)
    B, H, W, C = shape
    idx = []
    for b in range(B):
        for ch in range(nch):
            q = b * nch + ch
            oy, ox = q % S, ((q // 2) * (S - 1)) % S     # four consecutive planes reach the four tile residues (y mod 2, x mod 2)
            for y in range(oy, H, S):
                for x in range(ox, W, S):
                    idx.append(((b * H + y) * W + x) * C + ch)
    return np.array(idx, dtype=np.int64)


def sparse_slots(shape, S, nch=None):
    """as probe_slots, but one probe per PIXEL neighbourhood over all channels: for non-finite probes, whose 0 * inf reaches every
    output channel of every window that holds them"""
    nch = shape[-1] if nch is None else nch
    if len(shape) == 2:
        return np.arange(shape[0]) * shape[1] + (np.arange(shape[0]) % nch)            # one per row
    B, H, W, C = shape
    S = max(S, 8)
    idx = []
    for b in range(B):
        oy, ox = b % S, (b // S) % S
        for y in range(oy % min(S, H), H, S):
            for x in range(ox % min(S, W), W, S):
                idx.append(((b * H + y) * W + x) * C + (len(idx) % nch))
    return np.array(idx, dtype=np.int64)


def probe_rounds(shape, slots, values, noise=None):
    """-> [(operand float32, flat indices used, values placed)]: as many operands as it takes to place every value once"""
    out = []
    n = int(np.prod(shape))
    for i in range(0, len(values), len(slots)):
        v = values[i:i + len(slots)]
        a = np.zeros(n, dtype=F32) if noise is None else noise.copy().reshape(-1)
        a.view(U32)[slots[:len(v)]] = v
        out.append((a.reshape(shape), slots[:len(v)], v))
    return out


def onehot_weights(c, p):
    """forward: weight 1 at the centre tap from input channel o mod Cin to output channel o; data gradient: the mirror (from gradient
    channel i mod Cout to input channel i).  The pass is then a copy of its operand."""
    s = shapes(c)["w"]
    w = np.zeros(s, dtype=F32)
    N, K = s[0], s[1]
    ctr = () if c.kind == "lin" else (s[2] // 2, s[3] // 2)
    if p == "fwd":
        for o in range(N): w[(o, o % K) + ctr] = 1
    else:
        for i in range(K): w[(i % N, i) + ctr] = 1
    return w


def onehot_expected(c, p, a):
    """the copy the one-hot contraction makes of operand a (float32, exact: at most one nonzero term per sum on probe operands)"""
    s = shapes(c)
    if c.kind == "lin":
        N, K = s["w"]
        return a[:, np.arange(N) % K] if p == "fwd" else a[:, np.arange(K) % N]
    B, H, W, Cin, Cout, k, up = c.shape
    if p == "fwd":
        y = a[..., np.arange(Cout) % Cin]
        return np.repeat(np.repeat(y, 2, 1), 2, 2) if up else y
    g = a[..., np.arange(Cin) % Cout]
    if up:
        with np.errstate(invalid="ignore"):
            g = g.reshape(B, H, 2, W, 2, Cin).sum((2, 4), dtype=F32)
    return g


THREE_PLANE = 1.0 + 2.0 ** -10 + 2.0 ** -19                              # planes (1, 2^-10, 2^-19)
THREE_PLANE_PRODUCT = 1.0 + 2.0 ** -9 + 2.0 ** -18 + 2.0 ** -20          # its square without m l' + l m' (2^-28) and l l' (2^-38)


def split3_sum(v):
    """what a mode-6 contraction with an exact 1 makes of operand v: the sum of its three planes (exact in fp32: the planes of an
    operand below 2^-109 are multiples of 2^-133, those of a larger one do not overlap)"""
    h, m, l = split3(v)
    return (bf16_value(h).astype(np.float64) + bf16_value(m).astype(np.float64) + bf16_value(l).astype(np.float64)).astype(F32)


# What include/facegen_hip.h (fg_set_math) states about the bottom of the range, as measured on the one-hot pass and derived from the
# split arithmetic (VALUE_DOMAIN.md, "The bottom of the range"):
MODE6_EXACT_MIN_EXP = -110          # every |x| >= 2^-110 is a multiple of 2^-133, the resolution of a bf16 subnormal plane: exact
MODE6_ABS_ERR = 2.0 ** -134         # below: rounded to a multiple of 2^-133 (the planes ARE honoured by the matrix pipe, not flushed)
WINO_EXACT_MIN_EXP = -124           # the transformed one-hot taps are 1, 1/2 and 1/4: x / 4 is exact from 2^-124 up (ulp 2^-147)
WINO_ABS_ERR = 9 * 2.0 ** -150      # below: up to nine products, each rounded to the fp32 subnormal grid 2^-149


def subnormal_rule(c, p):
    """-> (smallest exponent from which the copy is exact, absolute error bound below it)"""
    if p in c.wino:
        return WINO_EXACT_MIN_EXP, WINO_ABS_ERR
    if mode6(c, p):
        return MODE6_EXACT_MIN_EXP, MODE6_ABS_ERR
    return -149, 0.0                # fp32 kernels (MFMA, thin, gemv): subnormal operands and results are exact, nothing is flushed


def reference_folded(c, op, which):
    """float64 reference of a folded up-convolution as the library defines it (include/facegen_hip.h: nearest-x2 folded into the taps):
    output parity (py, px) is the 3x3 convolution of the SOURCE image with the folded taps; the data gradient is the sum of the four
    transposed ones.  Equal to reference() on finite operands; on a non-finite source pixel it differs, because the unfolded form
    multiplies the three copies of that pixel by zero taps (NaN at the pixel itself) and the folded form has no such product."""
    B, H, W, Cin, Cout, k, up = c.shape
    assert up
    w = np.asarray(op["w"], np.float64)
    out = {}
    if "fwd" in which:
        x = t64(op["x"]).permute(0, 3, 1, 2)
        y = torch.zeros(B, Cout, 2 * H, 2 * W, dtype=torch.float64)
        for py in (0, 1):
            for px in (0, 1):
                y[:, :, py::2, px::2] = F.conv2d(x, torch.from_numpy(_folded_taps(w, py, px)), None, padding=1)
        out["fwd"] = y.permute(0, 2, 3, 1).contiguous().numpy()
    if "dgrad" in which:
        gy = t64(op["gy"]).permute(0, 3, 1, 2)
        g = None
        for py in (0, 1):
            for px in (0, 1):
                t = F.conv_transpose2d(gy[:, :, py::2, px::2].contiguous(), torch.from_numpy(_folded_taps(w, py, px)), padding=1)
                g = t if g is None else g + t
        out["dgrad"] = g.permute(0, 2, 3, 1).contiguous().numpy()
    return out


def wgrad_copy_operands(c, values):
    """The weight gradient as a copy of its gradient operand: x is 1 in every channel at ONE pixel of sample 0 (Linear: x[b][b] = 1), so
    gw[o][c][ty][tx] = gy[0][that pixel + pad - (ty, tx)][o] -- one nonzero term per sum.  Under a folded upsample the 1 becomes a 2x2
    block and a tap sums a 2x2 block of gy: the probes then sit on even rows and columns only, one per such block.
    -> [(x, gy)] per round; the expected bits are the float64 reference's (exact: a sum with one nonzero term)"""
    s = shapes(c)
    x = np.zeros(s["x"], F32)
    if c.kind == "lin":
        B, K, N = c.shape
        n = min(B, K)
        x[np.arange(n), np.arange(n)] = 1
        slots = (np.arange(n)[:, None] * N + np.arange(N)[None, :]).reshape(-1)
    else:
        B, H, W, Cin, Cout, k, up = c.shape
        pad, f = (k - 1) // 2, 2 if up else 1
        y0, x0 = H // 2, W // 2
        x[0, y0, x0, :] = 1
        ys = [y for y in range(f * y0 - pad, f * y0 + (f - 1) + pad + 1) if 0 <= y < f * H and y % f == 0]
        xs = [v for v in range(f * x0 - pad, f * x0 + (f - 1) + pad + 1) if 0 <= v < f * W and v % f == 0]
        slots = np.array([((0 * f * H + y) * f * W + v) * Cout + o for y in ys for v in xs for o in range(Cout)], dtype=np.int64)
    return [(x, gy) for gy, _, _ in probe_rounds(s["gy"], slots, values)]


def dilate(mask, r):
    """NHWC boolean mask grown by r pixels in H and W (any channel stays its own); 2-d masks are returned unchanged"""
    if mask.ndim != 4 or r == 0:
        return mask
    m = mask.copy()
    H, W = mask.shape[1], mask.shape[2]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            m[:, yd, xd] |= mask[:, ys, xs]
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# part 2, Winograd: the algorithm of csrc/wino.hip / wino_wgrad.hip in numpy, in float32 (emulation) or in float64 on absolute values
# with every subtraction turned into an addition (the a-priori bound)
# ---------------------------------------------------------------------------------------------------------------------------------
WINO_C = 16     # roundings besides the channel reduction, see VALUE_DOMAIN.md: tap fold 3 + G g G^T 4 + B^T d B 2 + A^T m A 4 + 3 spare


class _Ar:
    """arithmetic of one evaluation: dtype, and whether a - b means |a| + |b|"""
    def __init__(self, dtype, absolute):
        self.t, self.abs = dtype, absolute

    def sub(self, a, b):
        return (a + b) if self.abs else (a - b)

    def neg(self, a):
        return a if self.abs else -a


def _patches(x, oy, ox, sy=1, sx=1):
    """[B, H, W, C] -> [B, TH, TW, 4, 4, C]: element (i, j) of tile (ty, tx) is pixel (sy (2 ty + i) + oy, sx (2 tx + j) + ox), 0 outside;
    TH, TW: tiles of the OUTPUT map of the group's parity (H / (2 sy))"""
    B, H, W, C = x.shape
    TH, TW = H // (2 * sy), W // (2 * sx)
    d = np.zeros((B, TH, TW, 4, 4, C), dtype=x.dtype)
    for i in range(4):
        for j in range(4):
            for ty in range(TH):
                y = sy * (2 * ty + i) + oy
                if not 0 <= y < H: continue
                for tx in range(TW):
                    xx = sx * (2 * tx + j) + ox
                    if 0 <= xx < W: d[:, ty, tx, i, j] = x[:, y, xx]
    return d


def _bt_d_b(ar, d):
    """column pass then row pass, as WN_XFORM_STORE: (d0 - d2, d1 + d2, d2 - d1, d1 - d3)"""
    def one(a, ax):
        a0, a1, a2, a3 = (np.take(a, i, axis=ax) for i in range(4))
        return np.stack([ar.sub(a0, a2), a1 + a2, ar.sub(a2, a1), ar.sub(a1, a3)], axis=ax)
    return one(one(d, 3), 4)


def _g_g_gt(ar, t):
    """[..., 3, 3] -> [..., 4, 4], fg_wino_u16: r1 = 0.5 ((w0 + w2) + w1), r2 = 0.5 ((w0 + w2) - w1) along the columns, then the rows"""
    h = t.dtype.type(0.5)
    def one(a, ax):
        a0, a1, a2 = (np.take(a, i, axis=ax) for i in range(3))
        e = a0 + a2
        return np.stack([a0, h * (e + a1), h * ar.sub(e, a1), a2], axis=ax)
    return one(one(t, t.ndim - 1), t.ndim - 2)


def _at_m_a(ar, m):
    """[..., 4, 4] -> [..., 2, 2], the epilogue of wino_body: t0 = (m0 + m1) + m2, t1 = (m1 - m2) - m3 down the rows, then along them"""
    def one(a, ax):
        a0, a1, a2, a3 = (np.take(a, i, axis=ax) for i in range(4))
        return np.stack([(a0 + a1) + a2, ar.sub(ar.sub(a1, a2), a3)], axis=ax)
    return one(one(m, m.ndim - 2), m.ndim - 1)


def _fold_r(parity, d, pad):
    v = parity + d - pad
    return v >> 1 if v >= 0 else -((-v + 1) >> 1)


def _folded_taps(w, py, px):
    """the 3x3 kernel that output parity (py, px) of nearest-x2 + k x k applies to the SOURCE image (window origin -1)"""
    k = w.shape[2]
    pad = (k - 1) // 2
    t = np.zeros(w.shape[:2] + (3, 3), dtype=w.dtype)
    for dy in range(k):
        for dx in range(k):
            t[:, :, _fold_r(py, dy, pad) + 1, _fold_r(px, dx, pad) + 1] += w[:, :, dy, dx]
    return t


def _sub5(w, a, b):
    """sub-kernel (a, b) of the zero-extended 6x6 window of a 5x5 kernel"""
    t = np.zeros(w.shape[:2] + (3, 3), dtype=w.dtype)
    t[:, :, :3 - a, :3 - b] = w[:, :, 3 * a:3 * a + 3, 3 * b:3 * b + 3]
    return t


def _flipT(t):
    return np.ascontiguousarray(t[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def wino_plan(c, p, w):
    """-> [(output parity (py, px, stride), [(3x3 taps [N][C], input offset (oy, ox), input stride)])] as fill_wino lays the pass out"""
    B, H, W, Cin, Cout, k, up = c.shape
    if not up:
        wk = w if p == "fwd" else _flipT(w)
        if k == 3:
            return [((0, 0, 1), [(wk, (-1, -1), 1)])]
        return [((0, 0, 1), [(_sub5(wk, a, b), (3 * a - 2, 3 * b - 2), 1) for a in (0, 1) for b in (0, 1)])]
    if p == "fwd":
        return [((py, px, 2), [(_folded_taps(w, py, px), (-1, -1), 1)]) for py in (0, 1) for px in (0, 1)]
    return [((0, 0, 1), [(_flipT(_folded_taps(w, py, px)), (py - 2, px - 2), 2) for py in (0, 1) for px in (0, 1)])]


def wino_eval(c, p, a, w, dtype=F32, absolute=False):
    """forward / data gradient of a Winograd case evaluated as the kernel does: a = x (fwd) or gy (dgrad), NHWC"""
    ar = _Ar(dtype, absolute)
    a = (np.abs(a) if absolute else a).astype(dtype)
    w = (np.abs(w) if absolute else w).astype(dtype)
    B, H, W, Cin, Cout, k, up = c.shape
    N = Cout if p == "fwd" else Cin
    f = 2 if (up and p == "fwd") else 1
    out = np.zeros((B, H * f, W * f, N), dtype=dtype)
    for (py, px, st), groups in wino_plan(c, p, w):
        m = None
        for t, (oy, ox), s in groups:
            V = _bt_d_b(ar, _patches(a, oy, ox, s, s))                            # [B, TH, TW, 4, 4, C]
            Ut = _g_g_gt(ar, t)                                                   # [N, C, 4, 4]
            mm = np.einsum("btuijc,ncij->btuijn", V, Ut, optimize=True).astype(dtype)
            m = mm if m is None else (m + mm).astype(dtype)
        y = _at_m_a(ar, np.moveaxis(m, 5, 3))                                    # [B, TH, TW, N, 2, 2]
        Bq, TH, TW = y.shape[:3]
        y = y.transpose(0, 1, 4, 2, 5, 3).reshape(Bq, 2 * TH, 2 * TW, N)
        out[:, py::st, px::st] = y
    return out


def wino_wgrad_eval(c, x, gy, dtype=F32, absolute=False):
    """3x3 weight gradient in the Winograd domain: dU = sum over tiles of (A dY A^T) (.) (B^T d B), dg = G^T dU G"""
    ar = _Ar(dtype, absolute)
    x = (np.abs(x) if absolute else x).astype(dtype)
    gy = (np.abs(gy) if absolute else gy).astype(dtype)
    B, H, W, Cin, Cout, k, up = c.shape
    assert k == 3 and not up
    V = _bt_d_b(ar, _patches(x, -1, -1))
    dy = gy.reshape(B, H // 2, 2, W // 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5)   # [B, TH, TW, 2, 2, O]
    def a_one(a, ax):       # A = [1 0; 1 1; 1 -1; 0 -1]
        a0, a1 = np.take(a, 0, axis=ax), np.take(a, 1, axis=ax)
        return np.stack([a0, a0 + a1, ar.sub(a0, a1), ar.neg(a1)], axis=ax)
    dM = a_one(a_one(dy, 3), 4)
    dU = np.einsum("btuijo,btuijc->ocij", dM, V, optimize=True).astype(dtype)
    h = dtype(0.5)
    def g_one(a, ax):       # G^T: (d0 + (d1 + d2) / 2, (d1 - d2) / 2, (d1 + d2) / 2 + d3)
        a0, a1, a2, a3 = (np.take(a, i, axis=ax) for i in range(4))
        return np.stack([a0 + h * (a1 + a2), h * ar.sub(a1, a2), h * (a1 + a2) + a3], axis=ax)
    return g_one(g_one(dU, 2), 3)


def wino_channel_reduction(c, p):
    """K_c: products summed into one Winograd position"""
    B, H, W, Cin, Cout, k, up = c.shape
    if p == "wgrad":
        return B * (H // 2) * (W // 2)
    groups = 4 if (k == 5 and not up) or (up and p == "dgrad") else 1
    return groups * (Cin if p == "fwd" else Cout)


def wino_bound(c, op, p):
    """(K_c + c) 2^-24 times the algorithm on |x|, |w| with absolute-value matrices, in float64"""
    if p == "wgrad":
        A = wino_wgrad_eval(c, op["x"], op["gy"], np.float64, True)
    else:
        A = wino_eval(c, p, op["x"] if p == "fwd" else op["gy"], op["w"], np.float64, True)
    return (wino_channel_reduction(c, p) + WINO_C) * U * A


def bound(c, op, p):
    return wino_bound(c, op, p) if p in c.wino else direct_bound(c, op, [p])[p]


# ---------------------------------------------------------------------------------------------------------------------------------
# part 4: BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------
BN_LADDERS = (8, 96)               # C = 8: the float4 kernels (cr4_ok); C = 96: the column kernels
BN_ROWS = (1, 2, 4096)
BN_PIVOTS = (8, 64)                # row 0 (the pivot of the shifted sums) this many standard deviations from the mean
# 0, 1000 and -3.25 have squares whose fp32 sums are exact, so even un-shifted fp32 sums give them a zero variance; 1000.1 (rounded to
# fp32) does not, and C = 8 has two constant channels only: it comes first
BN_CONSTANTS = (1000.1, 1000.0, -3.25, 0.0)
# |x - pivot| above which the fp32 square of the deviation overflows (sqrt(FLT_MAX) = 1.8447e19); include/facegen_hip.h states 1.8e19
BN_D2_OVERFLOW = 1.8e19
BN_D2_PROBE = 2.0 ** 60            # 1.15e18: one probe below it; its square, 2^120, and the sum of 4096 such squares are finite


def cr_rowblocks(M):
    return min((M + 63) // 64, 256)                     # csrc/pointwise.hip


def bn_partition(M, C):
    """-> (row blocks, rows per block, row lanes of a block) of the statistics launch: C % 4 == 0 and 256 % (C / 4) == 0 take the
    float4 kernel (1024 threads = C / 4 channel quads x RY row lanes, combined one after the other), else 64 columns x 4 row lanes
    combined pairwise"""
    nrb = cr_rowblocks(M)
    per = (M + nrb - 1) // nrb
    f4 = C % 4 == 0 and 4 <= C <= 1024 and 256 % (C // 4) == 0
    return nrb, per, (1024 // (C // 4) if f4 else 4), f4


def bn_partial_adds(M, C):
    """r: fp32 additions behind one partial sum -- a lane's rows, then the lanes of the block that hold any"""
    nrb, per, RY, f4 = bn_partition(M, C)
    lane = (per + RY - 1) // RY
    return lane + (min(RY, per) - 1 if f4 else 2)


def bn_outlier_operands(M, C, k):
    """bn_operands' x ~ N(0.9, 1.7^2) with row 0 -- the pivot -- moved to mean + k std per channel, the sign alternating"""
    import test_gpu_pointwise_paths as TQ
    op = TQ.bn_operands(M, C, TQ.Src(1000 * k + M + C))
    x = op["x"].astype(np.float64)
    sign = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    op["x"][0] = (x[1:].mean(0) + sign * k * x[1:].std(0)).astype(F32)
    return op


def bn_constant_operands(M, C):
    """every fourth channel constant, at the values of BN_CONSTANTS in turn"""
    import test_gpu_pointwise_paths as TQ
    op = TQ.bn_operands(M, C, TQ.Src(77 + M + C))
    const = {}
    for i, c in enumerate(range(0, C, 4)):
        const[c] = float(F32(BN_CONSTANTS[i % len(BN_CONSTANTS)]))
        op["x"][:, c] = F32(const[c])
    return op, const


def bn_pivot_terms(op):
    """-> (t, dm, r): the relative error of the variance and the absolute error of the mean that r fp32 additions per partial leave in
    sums carrying S2 = sum (x - K)^2 = infl n var  (infl = 1 + k^2 for a pivot k standard deviations out):
      t = infl 2^-24 r        dm = sqrt(infl) std 2^-24 r   (sum |x - K| <= n sqrt(infl) std)"""
    x = op["x"].astype(np.float64)
    M, C = x.shape
    r = bn_partial_adds(M, C)
    var = x.var(0)
    infl = ((x - x[0]) ** 2).mean(0) / var
    return infl * U * r, np.sqrt(infl * var) * U * r, r


def bn_pivot_bars(op, ref, slope):
    """the terms of bn_pivot_terms propagated to first order through each formula bn_check compares (as offset_bars propagates the
    rounding of the saved mean): xhat = (x - mean) invstd moves by |xhat| t / 2 + invstd dm"""
    import test_gpu_pointwise_paths as TQ
    t, dm, r = bn_pivot_terms(op)
    M = op["x"].shape[0]
    ga, inv, xh, gz = np.abs(op["gamma"].astype(np.float64)), ref["invstd"], np.abs(ref["xh"]), ref["gz"]
    dxh = xh * t / 2 + inv * dm
    gg, gb = np.abs((gz * ref["xh"]).sum(0)), np.abs(gz.sum(0))
    dgg = gg * t / 2 + gb * inv * dm
    var = op["x"].astype(np.float64).var(0)
    neg = np.where(ref["pos"], 0.0, np.abs(op["gy"].astype(np.float64)))
    return dict(mean=dm, rm=TQ.BN_MOM * dm, invstd=inv * t / 2, rv=TQ.BN_MOM * var * M / max(M - 1, 1) * t, y=ga * dxh,
                gx=np.abs(ref["gx"]) * t / 2 + (dxh * gg + xh * dgg) / M * ga * inv, gg=dgg,
                gs=float((neg * ga * dxh).sum()) if slope is not None else 0.0)


def bn_shifted_pass_f32(x, pivot=None):
    """float32 emulation of bn_stats_partial_kernel / bn_stats4_partial_kernel + bn_stats_final_kernel: per-lane partial sums of
    d = x - x[0] and of d^2 (one rounding per fused multiply-add) in float32, the lanes of a block combined in float32, the blocks
    and the final formulas in float64 -> (mean, variance)"""
    M, C = x.shape
    nrb, per, RY, f4 = bn_partition(M, C)
    xs = np.zeros((nrb * per, C), F32)
    xs[:M] = x
    live = (np.arange(nrb * per) < M).reshape(nrb, per)
    steps = (per + RY - 1) // RY
    pad = steps * RY
    d = np.zeros((nrb, pad, C), F32)
    K = x[0] if pivot is None else np.broadcast_to(F32(pivot), (C,))
    d[:, :per] = (xs - K).astype(F32).reshape(nrb, per, C) * live[:, :, None]
    d = d.reshape(nrb, steps, RY, C)
    a1, a2 = np.zeros((nrb, RY, C), F32), np.zeros((nrb, RY, C), F32)
    for s in range(steps):
        a1 = (a1 + d[:, s]).astype(F32)
        a2 = (d[:, s].astype(np.float64) * d[:, s].astype(np.float64) + a2.astype(np.float64)).astype(F32)
    def combine(a):
        if not f4:
            return ((a[:, 0] + a[:, 1]).astype(F32) + (a[:, 2] + a[:, 3]).astype(F32)).astype(F32)
        t = a[:, 0]
        for j in range(1, RY):
            t = (t + a[:, j]).astype(F32)
        return t
    s1, s2 = combine(a1).astype(np.float64).sum(0), combine(a2).astype(np.float64).sum(0)
    n = float(M)
    return K.astype(np.float64) + s1 / n, np.maximum((s2 - s1 * s1 / n) / n, 0.0)
