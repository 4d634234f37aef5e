"""The fixed part of the Winograd kernels (csrc/wino.hip prologue; csrc/wino_wgrad.hip epilogue + wino_wgrad_finish_block):

  * wino_kernel requests the first chunk of U before any tile arithmetic and fills the output-row table behind the requests;
  * wino_wgrad_kernel stores the 16 positions of a channel pair as four planes of [pair][4] (lanes 16 bytes apart) and the finish
    pass reads them back from there; the sums, the signs and G^T (.) G are those of the layout before, in the same order.

Every case is held to the float64 oracle's direct convolution at the bars tests/test_gpu_wino.py uses for the same quantity
(gpu_util.BAR, imported, not restated) and, on small-integer data, to the direct convolution BIT FOR BIT: every intermediate is then
an integer (or, behind G^T . G, a multiple of 1/4) far below 2^24, so only a wrong index can show.

Shapes: the smallest at which each path of the prologue differs -- one tile / one (zero-padded odd) chunk / ragged channel block;
a ragged tile block on a tile grid that is no power of two (division decode) with 3 chunks and a ragged second channel block; exact
blocks with an even chunk count; few tiles and many channels (split K, uneven chunks per split); the four parities of a folded
up-convolution; the four K groups of a plain 5x5."""
import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import nhwc, nchw, dev, close, BAR
import test_gpu_wino as TW
import test_gpu_net_fusions as NF
import net_cases as NC

pytestmark = pytest.mark.gpu

FG_FUSE_DEFAULT, WINO_ALL = TW.FG_FUSE_DEFAULT, TW.WINO_ALL


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math, fusion = c.get_math(), c.get_fusion()
    yield c
    c.set_math(math); c.set_fusion(fusion)


SHAPES = [
    # B, H, W (source), Cin, Cout, k, folded nearest-x2
    (1, 2, 2, 8, 8, 3, 0),        # one tile, one chunk (the zero-padded odd chunk), ragged channel block
    (3, 6, 10, 24, 72, 3, 0),     # 45 tiles (ragged tile block), tile grid 3 x 5 (division decode), 3 chunks, second channel block ragged
    (2, 8, 8, 16, 64, 3, 0),      # exact blocks, even chunk count
    (2, 4, 4, 256, 64, 3, 0),     # few tiles, many channels: K split with uneven chunks per split
    (2, 4, 4, 16, 8, 5, 1),       # folded up-convolution: four parities
    (1, 6, 6, 8, 8, 5, 0),        # plain 5x5: four K groups
]
_IDS = ["%dx%dx%d_%dto%d_k%d%s" % (s[0], s[1], s[2], s[3], s[4], s[5], "up" if s[6] else "") for s in SHAPES]


def _layer(shape, integer, bias, seed):
    """-> (float32 conv, x, gy, float64 y, float64 gx) of one layer; integer: small-integer data, taps multiples of 4"""
    B, H, W, Cin, Cout, k, up = shape
    rng = np.random.default_rng(seed)
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    if integer:
        conv.weight[...] = (4 * rng.integers(-2, 3, conv.weight.shape)).astype(np.float32)
        conv.bias[...] = rng.integers(-8, 9, conv.bias.shape).astype(np.float32)
        x = rng.integers(-3, 4, (B, Cin, H, W)).astype(np.float32)
    else:
        x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    if not bias:
        conv.bias[...] = 0
    conv64 = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng).astype(np.float64)
    conv64.weight[...] = conv.weight; conv64.bias[...] = conv.bias
    xin = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) if up else x
    y = conv64.forward(xin.astype(np.float64))
    gy = (rng.integers(-3, 4, y.shape) if integer else rng.standard_normal(y.shape)).astype(np.float32)
    gx = conv64.backward(xin.astype(np.float64), gy.astype(np.float64))
    if up:
        gx = gx.reshape(B, Cin, H, 2, W, 2).sum(axis=(3, 5))
    return conv, x, gy, y, gx


def _fwd_dgrad(ctx, shape, conv, x, gy, bias, flags):
    from face_generator_amd import ops
    B, H, W, Cin, Cout, k, up = shape
    d = ctx.device
    ctx.set_fusion(flags)
    try:
        w_d = dev(conv.weight, d)
        b_d = dev(conv.bias, d) if bias else None
        return (nchw(ops.conv2d_forward(nhwc(x, d), w_d, b_d, upsample2x=bool(up))),
                nchw(ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W), upsample2x=bool(up))))
    finally:
        ctx.set_fusion(FG_FUSE_DEFAULT)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_forward_and_data_gradient_against_float64(ctx, shape, bias):
    conv, x, gy, y, gx = _layer(shape, False, bias, 1200 + sum(shape))
    yw, gw = _fwd_dgrad(ctx, shape, conv, x, gy, bias, FG_FUSE_DEFAULT)
    yi, gi = _fwd_dgrad(ctx, shape, conv, x, gy, bias, FG_FUSE_DEFAULT & ~WINO_ALL)
    sy, sg = max(np.abs(y).max(), 1.0), max(np.abs(gx).max(), 1.0)
    print("forward err %.3e (bar %.3e); data-gradient err %.3e (bar %.3e)"
          % (np.abs(yw - y).max(), BAR["wino_fwd"] * sy, np.abs(gw - gx).max(), BAR["wino_dgrad"] * sg))
    close(yw, y, atol=BAR["wino_fwd"] * sy, what="winograd forward vs float64 oracle")
    close(gw, gx, atol=BAR["wino_dgrad"] * sg, what="winograd data gradient vs float64 oracle")
    close(yw, yi, atol=3e-5 * sy, what="winograd vs implicit GEMM forward")
    close(gw, gi, atol=3e-5 * sg, what="winograd vs implicit GEMM data gradient")
    assert not np.array_equal(yw, yi), "the Winograd bits selected nothing: the case does not reach wino_kernel"


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_forward_and_data_gradient_exact_on_small_integers(ctx, shape, bias):
    conv, x, gy, y, gx = _layer(shape, True, bias, 2200 + sum(shape))
    yw, gw = _fwd_dgrad(ctx, shape, conv, x, gy, bias, FG_FUSE_DEFAULT)
    assert np.array_equal(yw.astype(np.float64), y), "forward differs from the direct convolution on small integers"
    assert np.array_equal(gw.astype(np.float64), gx), "data gradient differs from the direct convolution on small integers"


# ---- the three epilogues, as nets of tests/net_cases.py that reach them (tests/NET_FUSIONS.md rows 9, 10, 6) ---------------------------
EPILOGUE_CASES = ["r9-act-on-winograd",        # PReLU forward in the epilogue: wino_kernel<1>
                  "r10-actbwd-on-winograd",    # PReLU backward in the epilogue: wino_kernel<2>
                  "r6-bn-behind-winograd"]     # BatchNorm statistics of the raw accumulators: the late-bias path


@pytest.mark.parametrize("name", EPILOGUE_CASES)
def test_epilogue_nets_against_the_oracle(ctx, name):
    case = [c for c in NC.NET_CASES if c.name == name]
    assert len(case) == 1, "tests/net_cases.py no longer has the case %s" % name
    NF.test_net_case_against_the_float64_oracle(ctx, case[0])


# ---- weight gradient: wino_wgrad_kernel's epilogue (four planes of [pair][4]) + the finish pass (split sums, signs, G^T . G) ----------
WGRAD_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[5],      # (channel counts off the 64-blocks: the planner keeps these tap by tap)
                (7, 8, 8, 64, 64, 3, 0),      # 112 tiles = 14 chunks -> S = 14 splits of one chunk: S >= 12, S % 4 = 2 (the tail loop of the finish)
                (2, 4, 4, 64, 64, 5, 1),      # folded: four units meet in the finish pass's LDS
                (3, 4, 4, 64, 64, 5, 0)]      # plain 5x5: four groups, S = 6
_WIDS = ["%dx%dx%d_%dto%d_k%d%s" % (s[0], s[1], s[2], s[3], s[4], s[5], "up" if s[6] else "") for s in WGRAD_SHAPES]


def _wgrad_ref(shape, integer, seed):
    B, H, W, Cin, Cout, k, up = shape
    rng = np.random.default_rng(seed)
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng).astype(np.float64)
    x = (rng.integers(-3, 4, (B, Cin, H, W)) if integer else rng.standard_normal((B, Cin, H, W))).astype(np.float32)
    xu = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) if up else x
    gy = (rng.integers(-3, 4, (B, Cout, xu.shape[2], xu.shape[3])) if integer else rng.standard_normal((B, Cout, xu.shape[2], xu.shape[3]))).astype(np.float32)
    conv.zeroGradParameters()
    conv.accGradParameters(xu.astype(np.float64), gy.astype(np.float64))
    return x, gy, conv.gradWeight, conv.gradBias


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_WIDS)
def test_weight_gradient_against_float64(ctx, shape):
    B, H, W, Cin, Cout, k, up = shape
    x, gy, gw64, gb64 = _wgrad_ref(shape, False, 3200 + sum(shape))
    with TW.small_shapes_take_the_winograd_wgrad():
        (gw, gb), (gw0, gb0) = TW._wgrad_both(ctx, x, gy, k, up)
    sw, sb = max(np.abs(gw64).max(), 1.0), max(np.abs(gb64).max(), 1.0)
    print("weight-gradient err %.3e (bar %.3e); bias-gradient err %.3e (bar %.3e)"
          % (np.abs(gw - gw64).max(), BAR["wino_wgrad"] * sw, np.abs(gb - gb64).max(), BAR["conv_bgrad"] * sb))
    close(gw, gw64, atol=BAR["wino_wgrad"] * sw, what="weight gradient vs float64 oracle")
    close(gb, gb64, atol=BAR["conv_bgrad"] * sb, what="bias gradient vs float64 oracle")
    if Cin % 64 == 0 and Cout % 64 == 0:
        assert not np.array_equal(gw, gw0), "FG_FUSE_WINOGRAD_WGRAD selected nothing: the case does not reach wino_wgrad_kernel"


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_WIDS)
def test_weight_gradient_exact_on_small_integers(ctx, shape):
    from face_generator_amd import ops
    B, H, W, Cin, Cout, k, up = shape
    x, gy, gw64, gb64 = _wgrad_ref(shape, True, 4200 + sum(shape))
    d = ctx.device
    with TW.small_shapes_take_the_winograd_wgrad():
        (gw, gb), _ = TW._wgrad_both(ctx, x, gy, k, up)
        assert np.array_equal(gw.astype(np.float64), gw64) and np.array_equal(gb.astype(np.float64), gb64)
        if shape == (7, 8, 8, 64, 64, 3, 0):      # accGradParameters' accumulate (beta = 1) through the grouped-by-four finish loop and its tail
            math = ctx.get_math()
            ctx.set_math(0)
            try:
                gw2, gb2 = ops.conv2d_backward_weight(nhwc(x, d), nhwc(gy, d), k, upsample2x=bool(up), gw=dev(gw, d), gb=dev(gb, d), beta=1.0)
            finally:
                ctx.set_math(math)
            assert np.array_equal(gw2.cpu().numpy().astype(np.float64), 2 * gw64) and np.array_equal(gb2.cpu().numpy().astype(np.float64), 2 * gb64)
