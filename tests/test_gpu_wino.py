"""Winograd F(2x2, 3x3) (csrc/wino.hip; fg_set_fusion bits FG_FUSE_WINOGRAD / _UP / _5X5): forward and data gradient of
  * the 3x3 / pad 1 / stride 1 layers (models.lua:390-400, models_c2f.lua:124, 247-254),
  * the nearest-x2 + 5x5 up-convolutions (models.lua:63-64, 68-69): every output parity of the tap-folded layer is a 3x3 convolution
    of the source image -- four parities forward, four stride-2 input groups backward,
  * plain 5x5 / pad 2 layers (models_c2f.lua:125-126) as four 3x3 sub-kernels of the zero-extended 6x6 window,
against the oracle's direct convolution and against the library's own implicit GEMM (the bits cleared), on the same seeded inputs;
and their WEIGHT gradients in the Winograd domain (csrc/wino_wgrad.hip, bit FG_FUSE_WINOGRAD_WGRAD) against the oracle's
accGradParameters and the library's tap-by-tap contraction.

Tolerance: the transforms run in fp32 (B^T d B: two additions per value; G g G^T: halves and sums; A^T m A: sums of up to nine
products of transformed values), so a result differs from the direct convolution's by a few fp32 roundings of the LARGEST partial
sum, not of the result: the bar is 3e-5 * max|y| (the implicit GEMM meets 2e-5), stated per check below."""
import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import nhwc, nchw, dev, close, BAR

pytestmark = pytest.mark.gpu

FG_FUSE_WINOGRAD, FG_FUSE_WINOGRAD_UP, FG_FUSE_WINOGRAD_5X5, FG_FUSE_WINOGRAD_WGRAD, FG_FUSE_DEFAULT = 32, 64, 128, 256, 503
WINO_ALL = FG_FUSE_WINOGRAD | FG_FUSE_WINOGRAD_UP | FG_FUSE_WINOGRAD_5X5


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    yield c
    c.set_fusion(FG_FUSE_DEFAULT)


CASES = [
    # B, H, W, Cin, Cout
    (3, 8, 8, 64, 128),      # 48 tiles: one ragged block
    (2, 4, 4, 256, 512),     # D's deepest conv (models.lua:400): 8 tiles, 32 K chunks split over gridDim.y
    (5, 16, 16, 64, 128),    # 320 tiles = 5 blocks x 2 channel blocks
    (2, 6, 10, 16, 24),      # tile grid 3 x 5 (no power of two), 24 of 64 output channels live, two K chunks
    (1, 2, 2, 8, 8),         # a single tile, a single chunk
    (2, 64, 64, 64, 64),     # models_c2f.lua:124 / :247 at 64x64: 2048 tiles, un-split
    (9, 32, 32, 128, 256),   # models_c2f.lua:251: 2304 tiles = 36 blocks (no XCD remap: 36 % 8 != 0) x 4 channel blocks
    (16, 8, 8, 128, 256),    # D's d9 (models.lua:395): 256 tiles, split in two
]


@pytest.mark.parametrize("B,H,W,Cin,Cout", CASES)
def test_winograd_forward_and_data_gradient(ctx, B, H, W, Cin, Cout):
    from face_generator_amd import ops
    rng = np.random.default_rng(B * 1000 + H * 100 + Cin + Cout)
    conv = O.SpatialConvolution(Cin, Cout, 3, 3, 1, 1, 1, 1, rng)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    y = conv.forward(x)
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gx = conv.backward(x, gy)
    d = ctx.device
    w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
    got = {}
    for flags in (FG_FUSE_DEFAULT, FG_FUSE_DEFAULT & ~FG_FUSE_WINOGRAD):
        ctx.set_fusion(flags)
        got[flags] = (nchw(ops.conv2d_forward(nhwc(x, d), w_d, b_d)), nchw(ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W))))
    ctx.set_fusion(FG_FUSE_DEFAULT)
    yw, gw = got[FG_FUSE_DEFAULT]
    yi, gi = got[FG_FUSE_DEFAULT & ~FG_FUSE_WINOGRAD]
    sy, sg = max(np.abs(y).max(), 1.0), max(np.abs(gx).max(), 1.0)
    close(yw, y, atol=BAR["wino_fwd"] * sy, what="winograd forward vs oracle")
    close(gw, gx, atol=BAR["wino_dgrad"] * sg, what="winograd data gradient vs oracle")
    close(yi, y, atol=2e-5 * sy, what="implicit GEMM forward vs oracle")
    close(yw, yi, atol=3e-5 * sy, what="winograd vs implicit GEMM forward")
    close(gw, gi, atol=3e-5 * sg, what="winograd vs implicit GEMM data gradient")
    assert not np.array_equal(yw, yi), "both settings of FG_FUSE_WINOGRAD gave identical bits: the switch selected nothing"


def test_winograd_is_exact_on_small_integers(ctx):
    """Every intermediate of F(2x2, 3x3) on small-integer data with taps that are multiples of 4 is an integer below 2^24: the
    transforms, the 16 contractions and the output transform are then exact in fp32, so the result must equal the direct
    convolution BIT FOR BIT (pins the index maps -- tile decode, halo, position order, the 0 <-> 3 exchange of the flipped taps)."""
    from face_generator_amd import ops
    rng = np.random.default_rng(7)
    B, H, W, Cin, Cout = 3, 12, 8, 24, 40
    conv = O.SpatialConvolution(Cin, Cout, 3, 3, 1, 1, 1, 1, rng)
    conv.weight[...] = (4 * rng.integers(-2, 3, conv.weight.shape)).astype(np.float32)
    conv.bias[...] = rng.integers(-8, 9, conv.bias.shape).astype(np.float32)
    x = rng.integers(-3, 4, (B, Cin, H, W)).astype(np.float32)
    y = conv.forward(x)
    gy = rng.integers(-3, 4, y.shape).astype(np.float32)
    gx = conv.backward(x, gy)
    d = ctx.device
    ctx.set_fusion(FG_FUSE_DEFAULT)
    w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
    assert np.array_equal(nchw(ops.conv2d_forward(nhwc(x, d), w_d, b_d)), y)
    assert np.array_equal(nchw(ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W))), gx)


UP_CASES = [
    # B, H, W (source), Cin, Cout, k, folded nearest-x2
    (2, 8, 8, 128, 256, 5, 1),      # G's first up-convolution (models.lua:63-64)
    (3, 16, 16, 256, 128, 5, 1),    # G's second (models.lua:68-69): 192 tiles = 3 blocks x (4 parities x 2 channel blocks)
    (1, 4, 4, 32, 64, 5, 1),
    (2, 8, 8, 64, 64, 3, 1),        # a folded 3x3: the 3x3 window of each parity has zero taps
    (5, 6, 10, 16, 24, 5, 1),       # tile grid 3 x 5, ragged channel block
    (2, 6, 6, 32, 64, 5, 0),        # plain 5x5: four sub-kernels
    (3, 32, 32, 64, 128, 5, 0),     # models_c2f.lua:125 at 32x32
    (2, 16, 16, 128, 256, 5, 0),    # models_c2f.lua:126
    (2, 4, 8, 8, 8, 5, 0),
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,up", UP_CASES)
def test_winograd_up_and_5x5_layers(ctx, B, H, W, Cin, Cout, k, up):
    from face_generator_amd import ops
    rng = np.random.default_rng(B * 1000 + H * 100 + Cin + Cout + k + up)
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    ups = O.SpatialUpSamplingNearest(2)
    xu = ups.forward(x) if up else x
    y = conv.forward(xu)
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gxu = conv.backward(xu, gy)
    gx = ups.backward(x, gxu) if up else gxu
    d = ctx.device
    w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
    got = {}
    for flags in (FG_FUSE_DEFAULT, FG_FUSE_DEFAULT & ~WINO_ALL):
        ctx.set_fusion(flags)
        got[flags] = (nchw(ops.conv2d_forward(nhwc(x, d), w_d, b_d, upsample2x=bool(up))),
                      nchw(ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W), upsample2x=bool(up))))
    ctx.set_fusion(FG_FUSE_DEFAULT)
    yw, gw = got[FG_FUSE_DEFAULT]
    yi, gi = got[FG_FUSE_DEFAULT & ~WINO_ALL]
    sy, sg = max(np.abs(y).max(), 1.0), max(np.abs(gx).max(), 1.0)
    close(yw, y, atol=BAR["wino_fwd"] * sy, what="winograd forward vs oracle")
    close(gw, gx, atol=BAR["wino_dgrad"] * sg, what="winograd data gradient vs oracle")
    close(yw, yi, atol=3e-5 * sy, what="winograd vs implicit GEMM forward")
    close(gw, gi, atol=3e-5 * sg, what="winograd vs implicit GEMM data gradient")
    assert not np.array_equal(yw, yi), "both settings of the Winograd bits gave identical bits: the switch selected nothing"


@pytest.mark.parametrize("k,up", [(5, 1), (3, 1), (5, 0)])
def test_winograd_up_and_5x5_are_exact_on_small_integers(ctx, k, up):
    """As test_winograd_is_exact_on_small_integers, for the folded layers (the folded taps are sums of up to four multiples of 4) and
    for the four sub-kernels of a 5x5 layer: pins the parity -> output pixel map, the stride-2 sub-grid groups of the data gradient,
    the sub-kernel offsets (0 | 3) and the flipped 5x5 kernel's sub-kernels."""
    from face_generator_amd import ops
    rng = np.random.default_rng(70 + k + up)
    B, H, W, Cin, Cout = 3, 12, 8, 24, 40
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    conv.weight[...] = (4 * rng.integers(-2, 3, conv.weight.shape)).astype(np.float32)
    conv.bias[...] = rng.integers(-8, 9, conv.bias.shape).astype(np.float32)
    x = rng.integers(-3, 4, (B, Cin, H, W)).astype(np.float32)
    ups = O.SpatialUpSamplingNearest(2)
    xu = ups.forward(x) if up else x
    y = conv.forward(xu)
    gy = rng.integers(-3, 4, y.shape).astype(np.float32)
    gxu = conv.backward(xu, gy)
    gx = ups.backward(x, gxu) if up else gxu
    d = ctx.device
    ctx.set_fusion(FG_FUSE_DEFAULT)
    w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
    assert np.array_equal(nchw(ops.conv2d_forward(nhwc(x, d), w_d, b_d, upsample2x=bool(up))), y)
    assert np.array_equal(nchw(ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W), upsample2x=bool(up))), gx)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient in the Winograd domain (wino_wgrad.hip): dL/dU = sum over tiles of (A dY A^T) (.) (B^T d B), dL/dg = G^T dL/dU G
# ---------------------------------------------------------------------------------------------------------------------------------
import os
from contextlib import contextmanager


@contextmanager
def small_shapes_take_the_winograd_wgrad():
    """The library takes the Winograd weight gradient where it pays (>= 24 eight-tile chunks per block, >= 192 blocks); the test hook
    fg_test_set_wino_wgrad_thresholds lowers both planning thresholds so the small shapes below reach the kernel's corners (one chunk,
    odd chunk counts, a ragged last chunk, a single channel block)."""
    from face_generator_amd.runtime import get_context
    ctx = get_context(0)
    ctx.check(ctx.lib.fg_test_set_wino_wgrad_thresholds(ctx.h, 1, 1))
    try:
        yield
    finally:
        ctx.check(ctx.lib.fg_test_set_wino_wgrad_thresholds(ctx.h, 0, 0))


def _wgrad_both(ctx, x, gy, k, up):
    from face_generator_amd import ops
    d = ctx.device
    out = {}
    math = ctx.get_math()
    ctx.set_math(0)        # the Winograd weight gradient belongs to the fp32 mode (fg_set_math(6) keeps its own bf16x6 weight gradient)
    try:
        for flags in (FG_FUSE_DEFAULT, FG_FUSE_DEFAULT & ~FG_FUSE_WINOGRAD_WGRAD):
            ctx.set_fusion(flags)
            gw, gb = ops.conv2d_backward_weight(nhwc(x, d), nhwc(gy, d), k, upsample2x=bool(up))
            out[flags] = (gw.cpu().numpy(), gb.cpu().numpy())
    finally:
        ctx.set_fusion(FG_FUSE_DEFAULT)
        ctx.set_math(math)
    return out[FG_FUSE_DEFAULT], out[FG_FUSE_DEFAULT & ~FG_FUSE_WINOGRAD_WGRAD]


WGRAD_CASES = [
    # B, H, W (source), Cin, Cout, k, folded nearest-x2
    (3, 8, 8, 64, 64, 3, 0),        # 48 tiles = 6 chunks, one channel block
    (1, 4, 4, 64, 128, 3, 0),       # 4 tiles: half a chunk
    (5, 4, 4, 128, 64, 3, 0),       # 20 tiles: the last chunk holds 4
    (2, 16, 8, 64, 64, 3, 0),       # tile grid 8 x 4
    (2, 8, 8, 128, 256, 5, 1),      # G's first up-convolution (models.lua:63-64): four parities
    (3, 16, 16, 256, 128, 5, 1),    # G's second (models.lua:68-69)
    (2, 8, 8, 64, 64, 3, 1),        # folded 3x3: parities with zero taps
    (2, 8, 8, 64, 128, 5, 0),       # plain 5x5: four sub-kernel groups at offsets (3a - 2, 3b - 2)
    (7, 4, 4, 64, 64, 5, 0),        # 28 tiles = 3.5 chunks; every group's patches cross the border
    (9, 32, 32, 64, 128, 3, 0),     # models_c2f.lua:247-254 shape, split over the tiles
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,up", WGRAD_CASES)
def test_winograd_weight_gradient(ctx, B, H, W, Cin, Cout, k, up):
    rng = np.random.default_rng(B * 1000 + H * 100 + Cin + Cout + k + up + 5)
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    xu = O.SpatialUpSamplingNearest(2).forward(x) if up else x
    gy = rng.standard_normal((B, Cout, xu.shape[2], xu.shape[3])).astype(np.float32)
    conv.zeroGradParameters()
    conv.accGradParameters(xu, gy)
    with small_shapes_take_the_winograd_wgrad():
        (gw, gb), (gw0, gb0) = _wgrad_both(ctx, x, gy, k, up)
    # tolerance: the transformed operands are sums of up to 4 (dM) and 4 (V) values, the 16 position sums run over all tiles and
    # G^T . G mixes them with weights 1, 1/2, 1/4: a few fp32 roundings of the largest position sum -- 4e-5 * max|gradW| (the
    # tap-by-tap contraction meets 3e-5)
    sw, sb = max(np.abs(conv.gradWeight).max(), 1.0), max(np.abs(conv.gradBias).max(), 1.0)
    close(gw, conv.gradWeight, atol=BAR["wino_wgrad"] * sw, what="winograd weight gradient vs oracle")
    close(gw0, conv.gradWeight, atol=3e-5 * sw, what="tap-by-tap weight gradient vs oracle")
    close(gb, conv.gradBias, atol=3e-5 * sb, what="bias gradient (winograd kernel's partial sums) vs oracle")
    close(gb0, conv.gradBias, atol=3e-5 * sb, what="bias gradient vs oracle")
    assert not np.array_equal(gw, gw0), "both settings of FG_FUSE_WINOGRAD_WGRAD gave identical bits: the switch selected nothing"


@pytest.mark.parametrize("k,up", [(3, 0), (5, 1), (3, 1), (5, 0)])
def test_winograd_weight_gradient_is_exact_on_small_integers(ctx, k, up):
    """Small-integer x and gy: dM and V are integers, the 16 position sums are integers below 2^24, and G^T . G only halves and
    quarters them (exact in binary), so the Winograd-domain weight gradient must equal the direct one BIT FOR BIT -- pins the tile
    decode, the pair packing, the deferred signs of A's last row, the parity / group -> tap scatter and accGradParameters'
    accumulate (beta = 1) semantics."""
    from face_generator_amd import ops
    rng = np.random.default_rng(170 + k + up)
    B, H, W, Cin, Cout = 5, 8, 4, 64, 128
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    x = rng.integers(-3, 4, (B, Cin, H, W)).astype(np.float32)
    xu = O.SpatialUpSamplingNearest(2).forward(x) if up else x
    gy = rng.integers(-3, 4, (B, Cout, xu.shape[2], xu.shape[3])).astype(np.float32)
    conv.zeroGradParameters()
    conv.accGradParameters(xu, gy)
    d = ctx.device
    math = ctx.get_math()
    with small_shapes_take_the_winograd_wgrad():
        (gw, gb), (gw0, gb0) = _wgrad_both(ctx, x, gy, k, up)
        assert np.array_equal(gw, conv.gradWeight) and np.array_equal(gb, conv.gradBias)
        assert np.array_equal(gw0, conv.gradWeight) and np.array_equal(gb0, conv.gradBias)
        ctx.set_math(0)
        try:
            gw2, gb2 = ops.conv2d_backward_weight(nhwc(x, d), nhwc(gy, d), k, upsample2x=bool(up), gw=dev(gw, d), gb=dev(gb, d), beta=1.0)
        finally:
            ctx.set_math(math)
    assert np.array_equal(gw2.cpu().numpy(), 2 * conv.gradWeight) and np.array_equal(gb2.cpu().numpy(), 2 * conv.gradBias)


def test_winograd_weight_gradient_is_taken_at_the_baseline_shapes(ctx):
    """Without the knobs: G's second up-convolution at B = 32 (256 -> 128 on 16x16, models.lua:68-69) takes the Winograd kernel
    (different bits than the tap-by-tap contraction), D's 64 -> 128 layer on 16x16 (models.lua:390) does not (too few channel
    blocks: identical bits either way)."""
    rng = np.random.default_rng(99)
    for (B, H, W, Cin, Cout, k, up, taken) in [(32, 16, 16, 256, 128, 5, 1, True), (16, 16, 16, 64, 128, 3, 0, False)]:
        x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
        gy = rng.standard_normal((B, Cout, H * (2 if up else 1), W * (2 if up else 1))).astype(np.float32)
        (gw, gb), (gw0, gb0) = _wgrad_both(ctx, x, gy, k, up)
        close(gw, gw0, atol=4e-5 * max(np.abs(gw0).max(), 1.0), what="winograd vs tap-by-tap weight gradient")
        assert np.array_equal(gw, gw0) == (not taken)


# ---------------------------------------------------------------------------------------------------------------------------------
# error DISTRIBUTION against float64: the per-case bars above are relative to max|y| -- a few 1e-3
# absolute at K = 2 304 -- so a transform that rounded 3 x worse could hide inside them.  Here every layer shape of both workloads is
# measured against the float64 direct convolution in units of  u = eps32 * rms(y)  (one fp32 rounding of a typical output) and next to
# the library's own direct fp32 contraction (implicit GEMM, same data):
#   mean |err| <= 1.5 x the direct contraction's mean error,  max |err| <= 1.5 x its max error
#   mean |err| <= 3.0 u,  max |err| <= 24 u        (absolute ceilings, independent of the direct path)
# Measured (MI355X, round 6): Winograd mean 1.33 - 2.28 u, max 8.1 - 16.2 u at every K from 576 to 6 400 -- it does NOT grow with K (the
# 16 position sums are pairwise-like: 4 k-steps per MFMA, fp32 accumulators per position) -- while the direct fp32 contraction's
# sequential K loop goes from 1.2 u (K = 576) to 4.6 u (K = 6 400): ratio 1.15 at D's 3x3 layers, ~0.5 at the 5x5 layers.  (DESIGN
# up to round 5 said "1.7 x the direct convolution's rounding"; that was measured against max|y| at small K only.)
# Measured values: profiles/r06_wino_error.txt (scripts/wino_error_hist.py prints the same table).
# ---------------------------------------------------------------------------------------------------------------------------------
ERR_CASES = [
    # B, H, W (source), Cin, Cout, k, folded nearest-x2     -- every Winograd layer shape of configs[1] and configs[3]
    (8, 16, 16, 64, 128, 3, 0),     # D32b d5  (models.lua:390)
    (8, 8, 8, 128, 256, 3, 0),      # d9  (models.lua:395)
    (16, 4, 4, 256, 512, 3, 0),     # d13 (models.lua:400), split-K
    (4, 8, 8, 128, 256, 5, 1),      # G g5 (models.lua:63-64)
    (4, 16, 16, 256, 128, 5, 1),    # G g9 (models.lua:68-69)
    (1, 64, 64, 64, 128, 5, 0),     # c2f G_d (models_c2f.lua:125)
    (1, 64, 64, 128, 256, 5, 0),    # c2f G_d (models_c2f.lua:126)
    (2, 32, 32, 128, 256, 3, 0),    # c2f D_c (models_c2f.lua:251)
]


def wino_error_row(ctx, B, H, W, Cin, Cout, k, up):
    """-> dict of error statistics of the Winograd and the direct fp32 forward / data gradient against the float64 oracle."""
    from face_generator_amd import ops
    rng = np.random.default_rng(B * 7919 + H * 131 + Cin + 3 * Cout + k)
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, (k - 1) // 2, (k - 1) // 2, rng)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    xin = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) if up else x
    conv64 = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, (k - 1) // 2, (k - 1) // 2, rng).astype(np.float64)
    conv64.weight[...] = conv.weight; conv64.bias[...] = conv.bias
    y64 = conv64.forward(xin.astype(np.float64))
    gy = rng.standard_normal(y64.shape).astype(np.float32)
    g64 = conv64.backward(xin.astype(np.float64), gy.astype(np.float64))
    if up:
        g64 = g64.reshape(B, Cin, H, 2, W, 2).sum(axis=(3, 5))
    d = ctx.device
    w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
    res = {}
    for name, flags in (("wino", FG_FUSE_DEFAULT), ("direct", FG_FUSE_DEFAULT & ~WINO_ALL)):
        ctx.set_fusion(flags)
        y = nchw(ops.conv2d_forward(nhwc(x, d), w_d, b_d, upsample2x=bool(up))).astype(np.float64)
        g = nchw(ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W), upsample2x=bool(up))).astype(np.float64)
        res[name] = (np.abs(y - y64), np.abs(g - g64))
    ctx.set_fusion(FG_FUSE_DEFAULT)
    eps = float(np.finfo(np.float32).eps)
    row = {"K": k * k * Cin, "Kd": k * k * Cout}
    for which, ref, idx in (("fwd", y64, 0), ("dgrad", g64, 1)):
        u = eps * float(np.sqrt(np.mean(ref * ref)))
        for name in ("wino", "direct"):
            e = res[name][idx]
            row["%s_%s_mean_u" % (which, name)] = float(e.mean()) / u
            row["%s_%s_max_u" % (which, name)] = float(e.max()) / u
            row["%s_%s_p99_u" % (which, name)] = float(np.quantile(e, 0.99)) / u
    return row


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,up", ERR_CASES)
def test_winograd_error_distribution_against_float64(ctx, B, H, W, Cin, Cout, k, up):
    r = wino_error_row(ctx, B, H, W, Cin, Cout, k, up)
    for which, K in (("fwd", r["K"]), ("dgrad", r["Kd"])):
        wm, dm = r[which + "_wino_mean_u"], r[which + "_direct_mean_u"]
        wx, dx = r[which + "_wino_max_u"], r[which + "_direct_max_u"]
        msg = "%s K=%d: winograd mean %.2f u max %.1f u; direct mean %.2f u max %.1f u" % (which, K, wm, wx, dm, dx)
        assert wm <= 1.5 * dm and wx <= 1.5 * dx, msg
        assert wm <= 3.0 and wx <= 24.0, msg
        assert dm > 0.05, msg          # the direct path is not the float64 answer rounded once: the ratios above mean something
