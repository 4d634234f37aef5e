"""Operator-level parity for the kernel plans that the hand-picked lists of test_gpu_ops.py / test_gpu_wino.py / test_gpu_math_modes.py
never reach (tests/DISPATCH_COVERAGE.md): each case below was taken from the planning-only sweep of tests/dispatch_audit.py as a small
geometry -- in FLOPs of the pass -- at which the dispatcher picks the signature written next to it, and
tests/test_dispatch_coverage_host.py checks on the CPU that the case still takes that signature.

Reference: float64 on the CPU over the WHOLE output (torch conv2d / conv_transpose2d / conv2d_weight, plain double matmuls for
Linear) -- these kernels go wrong per tile, not per image.  Inputs as in test_gpu_ops.py (standard-normal activations and gradients,
the reference's uniform(-1/sqrt(fan_in), ..) parameters); bars are gpu_util.BAR's, scaled by max(1, max|reference|)."""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch7_nn as O
from gpu_util import close, BAR

pytestmark = pytest.mark.gpu

D = 503                     # FG_FUSE_DEFAULT
NOWINO = D & ~(32 | 64 | 128 | 256)
Case = collections.namedtuple("Case", "name kind shape math fusion expect")
# a signature: (launch-site text, block, dynamic LDS bytes); LDS None where it is a function of the map size (DISPATCH_COVERAGE.md)
WS, WS64, WS6 = "igemm_ws_kernel<BN>", "igemm_ws64x3_kernel<0>", "igemm_ws6_kernel<BN>"
IG = "(igemm_kernel<BM, BN, BK>)"


def conv(name, shape, expect, math=0, fusion=D):
    return Case(name, "conv", shape, math, fusion, expect)


def lin(name, shape, expect, math=0):
    return Case(name, "lin", shape, math, D, expect)


PATH_CASES = [
    # ---- wave-specialised implicit GEMM.  fp32: the 256 x 128 tile (igemm_ws, lds 123904) and the 256 x 64 three-stage tile
    # (igemm_ws64x3, lds 77824); math 6 (bf16x6): both LDS sizes of igemm_ws6 with their split-K grids, and the generic kernel's
    # 55808 / 74240 tiles.  Neighbouring cases share one shape (and one float64 reference) across the math modes.
    lin("ws256x128-lin", (16384, 32, 512), dict(fwd=[(WS, 512, 123904)])),
    lin("ws6-256x128-lin", (16384, 32, 512), dict(fwd=[(WS6, 512, 130048)]), math=6),
    lin("ws64x3-tile5-lin", (8192, 32, 512), dict(fwd=[(WS64, 512, 77824)])),
    lin("ig55808-lin-m6", (8192, 32, 512), dict(fwd=[(IG, 256, 55808)]), math=6),
    lin("ws64x3-n64-lin", (65536, 16, 64), dict(fwd=[(WS64, 512, 77824)], dgrad=[(WS64, 512, 77824)])),
    lin("ws6-n64-lin", (65536, 16, 64), dict(fwd=[(WS6, 512, 108544)], dgrad=[(WS6, 512, 108544)]), math=6),
    lin("ws-n192-lin", (65536, 16, 192), dict(fwd=[(WS, 512, 123904)], dgrad=[(WS64, 512, 77824)])),       # N % 128 == 64
    lin("ws6-n192-lin", (65536, 16, 192), dict(fwd=[(WS6, 512, 130048)], dgrad=[(WS6, 512, 108544)]), math=6),
    conv("ws256x128-conv3x3", (16, 32, 32, 32, 512, 3, 0), dict(fwd=[(WS, 512, 123904)]), fusion=NOWINO),
    conv("ws6-conv3x3", (16, 32, 32, 32, 512, 3, 0), dict(fwd=[(WS6, 512, 130048)], dgrad=[(WS6, 512, 108544)]), math=6, fusion=NOWINO),
    conv("ws256x128-dgrad-folded", (32, 64, 8, 512, 2, 3, 1), dict(fwd=[(WS64, 512, 77824)], dgrad=[(WS, 512, 123904)])),   # P = 4
    conv("ws64x3-dgrad-96to1", (24, 64, 64, 96, 1, 3, 0), dict(fwd=[(IG, 256, 55808)], dgrad=[(WS64, 512, 77824)])),
    conv("ig74240-dgrad-96to1-m6", (24, 64, 64, 96, 1, 3, 0), dict(dgrad=[(IG, 256, 74240)]), math=6),
    conv("ws64x3-folded-2to192", (14, 32, 64, 2, 192, 3, 1), dict(fwd=[(WS64, 512, 77824)])),              # P = 4, ragged Cin, N = 192
    conv("ws6-splitk-16to512", (32, 16, 16, 16, 512, 3, 0), dict(fwd=[(IG, 256, 55808)], dgrad=[(WS6, 512, 108544)]), math=6, fusion=NOWINO),
    conv("ws6-splitk-folded", (16, 16, 16, 32, 128, 3, 1), dict(dgrad=[(WS6, 512, 108544)]), math=6, fusion=NOWINO),
    conv("ws6-bn64-1to48-5x5", (8, 64, 16, 1, 48, 5, 0), dict(dgrad=[(WS6, 512, 108544)]), math=6),
    conv("ig55808-folded-12to1", (10, 64, 32, 12, 1, 3, 1), dict(fwd=[(IG, 256, 55808)])),
    # ---- long reductions at a tiny batch: the 128 x 128 split-K branch of choose_igemm and the capped split below it
    lin("splitk128-k33000", (4, 33000, 128), dict(fwd=[(IG, 256, 74240)])),        # 128 x 128 tiles (from 32768 features on), 61 uneven splits
    lin("splitk-k16384", (4, 16384, 128), dict(fwd=[(IG, 256, 69888)])),           # below that: 16 splits
    lin("splitk-k16384-n192", (4, 16384, 192), dict(fwd=[(IG, 256, 69888)], dgrad=[(IG, 256, 37120)])),
    lin("ig74240-lin-n2", (5364, 1615, 2), dict(dgrad=[(IG, 256, 74240)], wgrad=[("colsum_small_kernel<2>", 256, 0)])),
    # ---- Linear(K -> 1): the gemv pair
    lin("gemv-small", (5, 38, 1), dict(fwd=[("gemv_fwd_kernel", 64, 0)], dgrad=[("gemv_bwd_kernel", 256, None)])),
    lin("gemv-b300", (300, 606, 1), dict(fwd=[("gemv_fwd_kernel", 64, 0)], dgrad=[("gemv_bwd_kernel", 256, None)])),
    # (the backward keeps its rows in LDS: above 8192 rows it runs in chunks that accumulate -- one launch asked for more LDS than
    # a launch may have from B = 16129 on)
    lin("gemv-b20000", (20000, 70, 1), dict(fwd=[("gemv_fwd_kernel", 64, 0)], dgrad=[("gemv_bwd_kernel", 256, None)], wgrad=[("gemv_bwd_kernel", 256, None)])),
    # ---- thin layers: the instances behind the first choice of each ladder in thin.hip
    conv("slab13-64x64", (1, 64, 64, 3, 64, 3, 0), dict(dgrad=[("(thin_out_slab_mfma_kernel<1, 3>)", 256, None)])),
    conv("slab11-64x64-gray", (2, 64, 64, 1, 64, 3, 0), dict(dgrad=[("(thin_out_slab_mfma_kernel<1, 1>)", 256, None)])),
    conv("slab11-34x24", (4, 34, 24, 1, 64, 3, 0), dict(dgrad=[("(thin_out_slab_mfma_kernel<1, 1>)", 256, None)])),
    conv("slab23-6x30", (10, 6, 30, 3, 128, 3, 0), dict(dgrad=[("(thin_out_slab_mfma_kernel<2, 3>)", 256, None)])),
    conv("slab21-15x17", (5, 15, 17, 1, 128, 3, 0), dict(dgrad=[("(thin_out_slab_mfma_kernel<2, 1>)", 256, None)])),
    conv("slab11-fwd-19x13", (6, 19, 13, 64, 1, 3, 0), dict(fwd=[("(thin_out_slab_mfma_kernel<1, 1>)", 256, None)])),
    conv("tiled33-33x37", (2, 33, 37, 3, 256, 3, 0), dict(dgrad=[("(thin_out_tiled_kernel<3, 3>)", 256, 46656)])),
    conv("tiled31-33x37-gray", (2, 33, 37, 1, 256, 3, 0), dict(dgrad=[("(thin_out_tiled_kernel<3, 1>)", 256, 46656)])),
    conv("tiled33-fwd-512to3", (1, 5, 6, 512, 3, 3, 0), dict(fwd=[("(thin_out_tiled_kernel<3, 3>)", 256, 46656)])),
    conv("thinout3113-w2", (8, 8, 2, 64, 1, 3, 0), dict(fwd=[("(thin_out_kernel<3, 1, 1, 4>)", 256, 0)])),
    conv("thinout3134-w3", (17, 18, 3, 64, 3, 3, 0), dict(fwd=[("(thin_out_kernel<3, 1, 3, 4>)", 256, 0)])),
    conv("thinout3214-w2", (7, 8, 2, 1, 128, 3, 0), dict(dgrad=[("(thin_out_kernel<3, 2, 1, 4>)", 256, 0)])),
    conv("thinout3234-w2", (3, 8, 2, 128, 3, 3, 0), dict(fwd=[("(thin_out_kernel<3, 2, 3, 4>)", 256, 0)])),
    conv("win21-slab-bit-cleared", (4, 4, 8, 128, 1, 3, 0), dict(fwd=[("(thin_out_win_kernel<2, 1>)", 256, 0)]), fusion=D & ~2),
    conv("twgrad53-29x20", (2, 29, 20, 3, 256, 5, 0), dict(wgrad=[("(thin_wgrad_mfma_kernel<5, 3>)", 256, 0)])),
    conv("twgrad51-29x20-gray", (2, 29, 20, 1, 256, 5, 0), dict(wgrad=[("(thin_wgrad_mfma_kernel<5, 1>)", 256, 0)])),
    conv("twgrad711-pad-16x2", (1, 16, 2, 1, 128, 7, 0), dict(wgrad=[("(thin_wgrad_mfma_kernel<7, 1, 1>)", 256, 0)])),
    conv("colsum2-3to2-7x7", (3, 9, 9, 3, 2, 7, 0), dict(wgrad=[("colsum_small_kernel<2>", 256, 0)])),
    conv("colsum4-3to4", (1, 16, 4, 3, 4, 3, 0), dict(wgrad=[("colsum_small_kernel<4>", 256, 0)])),
    # ---- few channels on one side WITHOUT a full set of thin instances (the acceptance hole: forward ran, the weight gradient was
    # refused): ordinary convolutions now, all three passes
    conv("general-2to64", (7, 34, 14, 2, 64, 3, 0), dict(fwd=[(IG, 256, None)], wgrad=[("(wgrad_kernel<BT, BK, OCC>)", 256, None)])),
    conv("general-64to2-5x5", (3, 9, 11, 64, 2, 5, 0), dict(fwd=[(IG, 256, None)], wgrad=[("(wgrad_kernel<BT, BK, OCC>)", 256, None)])),
    conv("general-4to64-5x5", (3, 6, 6, 4, 64, 5, 0), dict(fwd=[(IG, 256, None)], wgrad=[("(wgrad_kernel<BT, BK, OCC>)", 256, None)])),
    conv("general-192to1", (2, 8, 8, 192, 1, 3, 0), dict(fwd=[(IG, 256, None)], dgrad=[(IG, 256, None)])),
    conv("general-3to192-7x7", (2, 7, 9, 3, 192, 7, 0), dict(fwd=[(IG, 256, None)], dgrad=[(IG, 256, None)])),
]


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math, fusion = c.get_math(), c.get_fusion()
    yield c
    c.set_math(math); c.set_fusion(fusion)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@functools.lru_cache(maxsize=1)
def operands_and_reference(kind, shape):
    """(float32 host operands, float64 references), computed once per geometry: neighbouring cases share it across the math modes"""
    if kind == "lin":
        B, K, N = shape
        rng = np.random.default_rng(B + K + N)
        m = O.Linear(K, N, rng)
        x = rng.standard_normal((B, K)).astype(np.float32)
        gy = rng.standard_normal((B, N)).astype(np.float32)
        x64, gy64, w64 = t64(x), t64(gy), t64(m.weight)
        return (x, gy, m.weight, m.bias), dict(fwd=x64 @ w64.t() + t64(m.bias), dgrad=gy64 @ w64, wgrad=gy64.t() @ x64, bgrad=gy64.sum(0))
    B, H, W, Cin, Cout, k, up = shape
    rng = np.random.default_rng(B * 1000 + H * 100 + Cin + Cout + k + up)
    pad, f = (k - 1) // 2, 2 if up else 1
    m = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)                # NHWC, the library's layout
    gy = rng.standard_normal((B, H * f, W * f, Cout)).astype(np.float32)
    w64 = t64(m.weight)
    xr, gyr = t64(x).permute(0, 3, 1, 2), t64(gy).permute(0, 3, 1, 2)
    if up: xr = F.interpolate(xr, scale_factor=2, mode="nearest")
    gxr = F.conv_transpose2d(gyr, w64, padding=pad)
    if up: gxr = gxr.reshape(B, Cin, H, 2, W, 2).sum((3, 5))
    return (x, gy, m.weight, m.bias), dict(fwd=F.conv2d(xr, w64, t64(m.bias), padding=pad).permute(0, 2, 3, 1), dgrad=gxr.permute(0, 2, 3, 1),
                                           wgrad=torch.nn.grad.conv2d_weight(xr, (Cout, Cin, k, k), gyr, padding=pad), bgrad=gyr.sum((0, 2, 3)))


def run_passes(ctx, c):
    """-> the four results of the library for the case's operands"""
    from face_generator_amd import ops
    (x, gy, w, b), _ = operands_and_reference(c.kind, c.shape)
    xd, gyd, wd, bd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ctx.device) for a in (x, gy, w, b))
    if c.kind == "lin":
        gw, gb = ops.linear_backward_weight(xd, gyd)
        return dict(fwd=ops.linear_forward(xd, wd, bd), dgrad=ops.linear_backward_data(gyd, wd), wgrad=gw, bgrad=gb)
    B, H, W, Cin, Cout, k, up = c.shape
    gw, gb = ops.conv2d_backward_weight(xd, gyd, k, upsample2x=bool(up))
    return dict(fwd=ops.conv2d_forward(xd, wd, bd, upsample2x=bool(up)), dgrad=ops.conv2d_backward_data(gyd, wd, (H, W), upsample2x=bool(up)),
                wgrad=gw, bgrad=gb)


BARS = dict(conv=dict(fwd="conv_fwd", dgrad="conv_dgrad", wgrad="conv_wgrad", bgrad="conv_bgrad"), lin=dict(fwd="lin", dgrad="lin", wgrad="lin", bgrad="lin"))


@pytest.mark.parametrize("case", PATH_CASES, ids=[c.name for c in PATH_CASES])
def test_dispatch_path_matches_float64(ctx, case):
    ctx.set_math(case.math); ctx.set_fusion(case.fusion)
    try:
        got = run_passes(ctx, case)
    finally:
        ctx.set_math(0); ctx.set_fusion(D)
    _, ref = operands_and_reference(case.kind, case.shape)
    worst = []
    for p in ("fwd", "dgrad", "wgrad", "bgrad"):
        r, g = ref[p].numpy(), got[p].cpu().numpy().astype(np.float64)
        scale = max(1.0, float(np.abs(r).max()))
        worst.append("%s %.2e of %.1e" % (p, float(np.abs(g - r).max()) / scale, BAR[BARS[case.kind][p]]))
    print("%s: max|err| / max(1, max|ref|): %s" % (case.name, "; ".join(worst)))
    for p in ("fwd", "dgrad", "wgrad", "bgrad"):
        r = ref[p].numpy()
        close(got[p].cpu().numpy(), r, atol=BAR[BARS[case.kind][p]] * max(1.0, float(np.abs(r).max())), what="%s %s" % (case.name, p))


def test_gray_coarse_to_fine_generator_forward_and_gradients(ctx):
    """models_c2f.lua's G_d on ONE image plane: its first layer is 2 -> 64 at 3x3 (noise + gray), a layer with few input channels and
    no thin weight-gradient instance.  fg_net_create used to plan it on the thin kernels, ran it forward and refused its backward;
    it is an implicit GEMM on zero-padded channel rows now.  Forward image and flat gradient against the oracle, as
    test_gpu_c2f.py does for the colour nets."""
    from face_generator_amd import models_c2f
    from gpu_util import nhwc, nchw
    from test_gpu_net import check_flat_grads, draw_kink_safe
    S, B = 16, 4
    rng = np.random.default_rng(516)
    G = O.create_G_d((1, S, S), rng)
    for m in G.inner.modules:
        if isinstance(m, O.PReLU):
            m.weight[0] = np.float32(rng.uniform(0.1, 0.4))
    pG, gG = G.getParameters()
    Gd = models_c2f.create_G((1, S, S), cuda=True, max_batch=B)
    p_d, _ = Gd.getParameters()
    assert p_d.numel() == pG.size
    p_d.copy_(torch.tensor(pG))
    dn = Gd.inner.device_net
    dn.params_changed()
    d = ctx.device
    cond = rng.uniform(0, 1, (B, 1, S, S)).astype(np.float32)
    noise, diff = draw_kink_safe(rng, lambda: rng.uniform(-1, 1, (B, 1, S, S)).astype(np.float32), lambda nz: G.forward([nz, cond]), [G.inner])
    gy = rng.standard_normal(diff.shape).astype(np.float32)
    gG[...] = 0
    G.backward([noise, cond], gy)
    y = dn.forward(Gd.combine_device(ctx, nhwc(noise, d), nhwc(cond, d)))
    close(nchw(y), diff, atol=2e-5 * max(1, np.abs(diff).max()), what="gray c2f G diff image")
    dn.backward(nhwc(gy, d), param_grads=True)
    check_flat_grads(dn.grads.cpu().numpy(), G.inner, "gray c2f G")
