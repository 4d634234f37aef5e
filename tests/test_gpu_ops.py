"""Module-level parity: each C-ABI operator of libfacegen_hip.so against the oracle (oracle/torch7_nn.py)
on the same seeded inputs.  fp32; tolerances stated per test."""
import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import nhwc, nchw, dev, close, BAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


CONV_CASES = [
    # B, H, W, Cin, Cout, k, upsample
    (2, 8, 8, 64, 128, 3, 0),
    (3, 6, 5, 32, 64, 3, 0),        # non power-of-two spatial dims, ragged M
    (2, 4, 4, 256, 512, 3, 0),      # D's deepest conv (models.lua:400)
    (5, 16, 16, 64, 128, 3, 0),
    (2, 8, 8, 128, 256, 5, 1),      # G: upsample-folded 5x5 (models.lua:63-64)
    (2, 16, 16, 256, 128, 5, 1),    # G: models.lua:68-69
    (1, 4, 4, 32, 64, 5, 1),
    (2, 6, 6, 32, 64, 5, 0),        # plain 5x5
    (1, 5, 5, 16, 64, 7, 0),        # 7x7 (c2f generator head family)
    (2, 8, 8, 64, 64, 3, 1),        # folded 3x3 (2x2 effective taps)
    (2, 32, 32, 3, 64, 3, 0),       # thin-in  (models.lua:385)
    (2, 32, 32, 128, 3, 3, 0),      # thin-out (models.lua:73)
    (2, 16, 16, 1, 64, 3, 0),       # gray
    (2, 16, 16, 128, 1, 3, 0),
    (2, 8, 8, 64, 3, 3, 0),         # thin-out with Cw = 64
    # M >= 4096 pixels: the wave-specialised weight gradients (the 256 x 128 tile, and the 128 x 64 tile whose 64-pixel K-step is
    # split over the MFMA waves -- models_c2f.lua:120-121, 246: the 64 -> 128 layers at 64x64 and 32x32)
    (2, 64, 64, 64, 128, 3, 0),
    (5, 32, 32, 64, 128, 5, 0),
    (2, 64, 32, 128, 256, 3, 0),
    (8, 32, 32, 64, 128, 3, 1),     # folded: four parities x 2x2 taps through the 128 x 64 tile
    # channel counts that are not multiples of 4 (round 5: the operand is copied into zero-padded rows, conv_ops.hip pad_operand)
    (2, 8, 8, 6, 10, 3, 0),
    (3, 6, 6, 1, 32, 3, 0),         # one input channel, not a thin-layer width
    (2, 8, 8, 30, 64, 5, 0),
    (2, 4, 4, 10, 6, 3, 1),         # folded upsample, both sides ragged
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,up", CONV_CASES)
def test_conv2d_forward_backward(ctx, B, H, W, Cin, Cout, k, up):
    from face_generator_amd import ops
    rng = np.random.default_rng(B * 1000 + H * 100 + Cin + Cout + k + up)
    pad = (k - 1) // 2
    conv = O.SpatialConvolution(Cin, Cout, k, k, 1, 1, pad, pad, rng)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    if up:
        ups = O.SpatialUpSamplingNearest(2)
        xu = ups.forward(x)
    else:
        xu = x
    y = conv.forward(xu)
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gxu = conv.backward(xu, gy)
    gx = ups.backward(x, gxu) if up else gxu
    d = ctx.device
    w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
    y_d = ops.conv2d_forward(nhwc(x, d), w_d, b_d, upsample2x=bool(up))
    scale = np.abs(y).max()
    close(nchw(y_d), y, atol=BAR["conv_fwd"] * max(scale, 1), what="conv fwd")
    gx_d = ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W), upsample2x=bool(up))
    close(nchw(gx_d), gx, atol=BAR["conv_dgrad"] * max(np.abs(gx).max(), 1), what="conv dgrad")
    gw_d, gb_d = ops.conv2d_backward_weight(nhwc(x, d), nhwc(gy, d), k, upsample2x=bool(up))
    close(gw_d.cpu().numpy(), conv.gradWeight, atol=BAR["conv_wgrad"] * max(np.abs(conv.gradWeight).max(), 1), what="conv wgrad")
    close(gb_d.cpu().numpy(), conv.gradBias, atol=BAR["conv_bgrad"] * max(np.abs(conv.gradBias).max(), 1), what="conv bgrad")
    # accumulate semantics (Torch accGradParameters): beta = 1 doubles
    gw2, gb2 = ops.conv2d_backward_weight(nhwc(x, d), nhwc(gy, d), k, upsample2x=bool(up), gw=gw_d.clone(),
                                          gb=gb_d.clone(), beta=1.0)
    close(gw2.cpu().numpy(), 2 * gw_d.cpu().numpy(), atol=BAR["conv_acc"] * max(np.abs(conv.gradWeight).max(), 1), what="acc")


LINEAR_CASES = [(4, 100, 8192), (6, 2048, 512), (128, 512, 512), (3, 64, 128), (130, 100, 256),
                (5, 50, 256), (4, 99, 8192), (7, 64, 10), (6, 33, 7)]      # --noiseDim 50 / 99 (nn_utils.lua:35-39); ragged both ways


@pytest.mark.parametrize("B,K,N", LINEAR_CASES)
def test_linear(ctx, B, K, N):
    from face_generator_amd import ops
    rng = np.random.default_rng(B + K + N)
    lin = O.Linear(K, N, rng)
    x = rng.standard_normal((B, K)).astype(np.float32)
    y = lin.forward(x)
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gx = lin.backward(x, gy)
    d = ctx.device
    w_d, b_d = dev(lin.weight, d), dev(lin.bias, d)
    close(ops.linear_forward(dev(x, d), w_d, b_d).cpu().numpy(), y, atol=BAR["lin"] * max(np.abs(y).max(), 1), what="lin fwd")
    close(ops.linear_backward_data(dev(gy, d), w_d).cpu().numpy(), gx, atol=BAR["lin"] * max(np.abs(gx).max(), 1), what="lin dgrad")
    gw, gb = ops.linear_backward_weight(dev(x, d), dev(gy, d))
    close(gw.cpu().numpy(), lin.gradWeight, atol=BAR["lin"] * max(np.abs(lin.gradWeight).max(), 1), what="lin wgrad")
    close(gb.cpu().numpy(), lin.gradBias, atol=BAR["lin"] * max(np.abs(lin.gradBias).max(), 1), what="lin bgrad")


@pytest.mark.parametrize("B,H,W,C,prelu", [(4, 16, 16, 256, True), (3, 7, 5, 128, True), (2, 8, 8, 64, False),
                                           (16, 32, 32, 128, True)])
def test_batchnorm_prelu(ctx, B, H, W, C, prelu):
    from face_generator_amd import ops
    rng = np.random.default_rng(C + B)
    bn = O.SpatialBatchNormalization(C, rng=rng)
    bn.bias[...] = rng.standard_normal(C).astype(np.float32) * 0.3
    pr = O.PReLU()
    x = (rng.standard_normal((B, C, H, W)) * 1.7 + 0.9).astype(np.float32)   # non-zero mean: exercises the shifted sums
    z = bn.forward(x)
    y = pr.forward(z) if prelu else z
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gz = pr.backward(z, gy) if prelu else gy
    gx = bn.backward(x, gz)
    d = ctx.device
    rm, rv = ctx.zeros(C), torch.ones(C, device=d)
    slope = dev(pr.weight, d) if prelu else None
    y_d, mean, invstd = ops.batchnorm_forward(nhwc(x, d), dev(bn.weight, d), dev(bn.bias, d), slope, rm, rv)
    close(nchw(y_d), y, atol=BAR["bn_y"], what="bn fwd")
    close(mean.cpu().numpy(), bn.save_mean, atol=BAR["bn_mean"], what="bn mean")
    close(invstd.cpu().numpy(), bn.save_invstd, atol=0, rtol=BAR["bn_invstd_rtol"], what="bn invstd")
    close(rm.cpu().numpy(), bn.running_mean, atol=BAR["bn_running_mean"], what="running_mean")
    close(rv.cpu().numpy(), bn.running_var, atol=0, rtol=BAR["bn_running_var_rtol"], what="running_var")
    gx_d, gg, gb, gs = ops.batchnorm_backward(nhwc(x, d), nhwc(gy, d), dev(bn.weight, d), dev(bn.bias, d), mean, invstd, slope)
    close(nchw(gx_d), gx, atol=BAR["bn_gx"] * max(1, np.abs(gx).max()), what="bn gx")
    close(gg.cpu().numpy(), bn.gradWeight, atol=BAR["bn_gparam"] * max(1, np.abs(bn.gradWeight).max()), what="bn ggamma")
    close(gb.cpu().numpy(), bn.gradBias, atol=BAR["bn_gparam"] * max(1, np.abs(bn.gradBias).max()), what="bn gbeta")
    if prelu:
        close(gs.cpu().numpy(), pr.gradWeight, atol=BAR["bn_gparam"] * max(1, abs(pr.gradWeight[0])), what="slope grad")
    # evaluate mode uses the running statistics (sample.lua path)
    bn.evaluate()
    ze = bn.forward(x)
    ye = pr.forward(ze) if prelu else ze
    ye_d, _, _ = ops.batchnorm_forward(nhwc(x, d), dev(bn.weight, d), dev(bn.bias, d), slope, rm, rv, train=False)
    close(nchw(ye_d), ye, atol=BAR["bn_y"], what="bn eval")


def test_prelu_dropout_and_actpool(ctx):
    from face_generator_amd import ops
    rng = np.random.default_rng(7)
    d = ctx.device
    # PReLU + Dropout(0.5) on [B,512]  (models.lua:407-408)
    x = rng.standard_normal((6, 512)).astype(np.float32)
    pr, dr = O.PReLU(), O.Dropout(0.5)
    pr.weight[0] = 0.3
    mask = (rng.random((6, 512)) < 0.5).astype(np.float32)
    dr.set_mask(mask)
    y = dr.forward(pr.forward(x))
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gx = pr.backward(x, dr.backward(pr.output, gy))
    sl = dev(pr.weight, d)
    close(ops.prelu_forward(dev(x, d), sl, dev(mask, d), 2.0).cpu().numpy(), y, atol=BAR["prelu"], what="prelu+drop fwd")
    gx_d, gs = ops.prelu_backward(dev(x, d), dev(gy, d), sl, dev(mask, d), 2.0)
    close(gx_d.cpu().numpy(), gx, atol=BAR["prelu"], what="prelu+drop gx")
    close(gs.cpu().numpy(), pr.gradWeight, atol=BAR["slope_grad"], what="prelu slope grad")
    # PReLU + SpatialDropout(0.2) + AvgPool  (models.lua:386-388)
    B, C, H, W = 3, 64, 8, 8
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    pr, sd, ap = O.PReLU(), O.SpatialDropout(0.2), O.SpatialAveragePooling()
    pr.weight[0] = -0.1
    m = (rng.random((B, C)) < 0.8).astype(np.float32)
    sd.set_mask(m)
    y = ap.forward(sd.forward(pr.forward(x)))
    gy = rng.standard_normal(y.shape).astype(np.float32)
    gx = pr.backward(x, sd.backward(pr.output, ap.backward(sd.output, gy)))
    sl = dev(pr.weight, d)
    close(nchw(ops.actpool_forward(nhwc(x, d), sl, dev(m, d))), y, atol=BAR["prelu"], what="actpool fwd")
    gx_d, gs = ops.actpool_backward(nhwc(x, d), nhwc(gy, d), sl, dev(m, d))
    close(nchw(gx_d), gx, atol=BAR["prelu"], what="actpool gx")
    close(gs.cpu().numpy(), pr.gradWeight, atol=BAR["slope_grad"], what="actpool slope grad")
    # evaluate mode: y = (1-p) * x, no mask
    sd.evaluate()
    ye = ap.forward(sd.forward(pr.forward(x)))
    close(nchw(ops.actpool_forward(nhwc(x, d), sl, None, 0.8)), ye, atol=1e-6, what="actpool eval")


def test_small_pointwise(ctx):
    rng = np.random.default_rng(8)
    d, lib = ctx.device, ctx.lib
    x = rng.standard_normal((2, 5, 6, 4)).astype(np.float32)   # NCHW
    xd = nhwc(x, d)
    B, C, H, W = x.shape
    y = ctx.empty(B, 2 * H, 2 * W, C)
    ctx.check(lib.fg_upsample_nearest2x_forward(ctx.h, xd.data_ptr(), y.data_ptr(), B, H, W, C))
    up = O.SpatialUpSamplingNearest(2)
    close(nchw(y), up.forward(x), atol=BAR["upsample_fwd"], what="upsample fwd")
    gy = rng.standard_normal((B, C, 2 * H, 2 * W)).astype(np.float32)
    gx = ctx.empty(B, H, W, C)
    ctx.check(lib.fg_upsample_nearest2x_backward(ctx.h, nhwc(gy, d).data_ptr(), gx.data_ptr(), B, H, W, C))
    close(nchw(gx), up.backward(x, gy), atol=BAR["upsample_bwd"], what="upsample bwd")
    ap = O.SpatialAveragePooling()
    yp = ctx.empty(B, H // 2, W // 2, C)
    ctx.check(lib.fg_avgpool2x2_forward(ctx.h, xd.data_ptr(), yp.data_ptr(), B, H, W, C))
    close(nchw(yp), ap.forward(x[:, :, :H // 2 * 2, :]), atol=BAR["avgpool_fwd"], what="avgpool fwd")
    g2 = rng.standard_normal((B, C, H // 2, W // 2)).astype(np.float32)
    gxp = ctx.empty(B, H, W, C)
    ctx.check(lib.fg_avgpool2x2_backward(ctx.h, nhwc(g2, d).data_ptr(), gxp.data_ptr(), B, H, W, C))
    close(nchw(gxp), ap.backward(x, g2), atol=BAR["avgpool_bwd"], what="avgpool bwd")
    sg = O.Sigmoid()
    ys = torch.empty_like(xd)
    ctx.check(lib.fg_sigmoid_forward(ctx.h, xd.data_ptr(), ys.data_ptr(), xd.numel()))
    close(nchw(ys), sg.forward(x), atol=BAR["sigmoid"], what="sigmoid")
    lr = O.LeakyReLU(0.333)
    yl = torch.empty_like(xd)
    ctx.check(lib.fg_leakyrelu_forward(ctx.h, xd.data_ptr(), 0.333, yl.data_ptr(), xd.numel()))
    close(nchw(yl), lr.forward(x), atol=BAR["leakyrelu"], what="leakyrelu")
    gl = torch.empty_like(xd)
    gyl = rng.standard_normal(x.shape).astype(np.float32)
    ctx.check(lib.fg_leakyrelu_backward(ctx.h, xd.data_ptr(), nhwc(gyl, d).data_ptr(), 0.333, gl.data_ptr(), xd.numel()))
    close(nchw(gl), lr.backward(x, gyl), atol=BAR["leakyrelu"], what="leakyrelu bwd")
    # layout round trip
    back = ctx.to_nchw(ctx.to_device_nhwc(torch.tensor(x)))
    close(back.cpu().numpy(), x, atol=0, what="nchw<->nhwc")
    close(nchw(ctx.to_device_nhwc(torch.tensor(x))), x, atol=0, what="nchw->nhwc")


def test_bce_and_confusion(ctx):
    from face_generator_amd.nn import BCECriterion
    rng = np.random.default_rng(9)
    for B in (4, 128, 1000):
        p = rng.uniform(0.001, 0.999, B).astype(np.float32)
        p[0] = 1e-9; p[1] = 1.0 - 1e-7
        t = (rng.random(B) < 0.5).astype(np.float32)
        crit = O.BCECriterion()
        f = crit.forward(p.reshape(B, 1), t)
        g = crit.backward(p.reshape(B, 1), t)
        loss, grad, conf = BCECriterion().forward_backward_device(ctx, dev(p, ctx.device), dev(t, ctx.device))
        assert abs(loss.item() - f) <= BAR["bce_loss_rtol"] * abs(f)          # loss: rel 1e-5
        close(grad.cpu().numpy(), g[:, 0], atol=BAR["bce_grad_atol"], rtol=BAR["bce_grad_rtol"], what="bce grad")
        want = np.zeros(4, np.int64)
        for i in range(B):
            want[(2 if p[i] > 0.5 else 0) + int(t[i])] += 1
        assert (conf.cpu().numpy() == want).all()


def test_fused_adam_sgd_adagrad_match_reference_formulas(ctx):
    rng = np.random.default_rng(10)
    n = 100003
    d = ctx.device
    p0 = rng.standard_normal(n).astype(np.float32)
    # Adam with L2 penalty + clamp (D's defaults: train.lua:29-37), 3 steps, tiny and large gradients
    p_ref = p0.copy(); st = {}
    p_d, m_d, v_d = dev(p0, d), ctx.zeros(n), ctx.zeros(n)
    for t in range(1, 4):
        g = (rng.standard_normal(n) * (1e-6 if t == 1 else 3.0)).astype(np.float32)
        def op(x, g=g):
            gg = g + np.sign(p_ref) * np.float32(0.0) + p_ref * np.float32(1e-4)
            return 0.0, np.clip(gg, -1, 1).astype(np.float32)
        O.interruptable_adam(op, p_ref, {}, st)
        gout = ctx.empty(n)
        ctx.check(ctx.lib.fg_adam_fused(ctx.h, p_d.data_ptr(), dev(g, d).data_ptr(), m_d.data_ptr(), v_d.data_ptr(), n,
                                        1.0, 0.0, 1e-4, 1.0, 1e-3, 0.9, 0.999, 1e-8, t, gout.data_ptr()))
        close(p_d.cpu().numpy(), p_ref, atol=2e-7, rtol=2e-7, what="adam p step %d" % t)   # abs <= 1e-6
        close(m_d.cpu().numpy(), st['m'], atol=1e-7, rtol=1e-5, what="adam m")
        close(v_d.cpu().numpy(), st['v'], atol=1e-12, rtol=1e-5, what="adam v")
    # gscale (1/world after an all-reduce sum)
    p2, m2, v2 = dev(p0, d), ctx.zeros(n), ctx.zeros(n)
    g = rng.standard_normal(n).astype(np.float32)
    ctx.check(ctx.lib.fg_adam_fused(ctx.h, p2.data_ptr(), dev(g * 8, d).data_ptr(), m2.data_ptr(), v2.data_ptr(), n,
                                    0.125, 0.0, 0.0, 0.0, 1e-3, 0.9, 0.999, 1e-8, 1, None))
    pr = p0.copy(); O.interruptable_adam(lambda x: (0.0, g), pr, {}, {})
    close(p2.cpu().numpy(), pr, atol=2e-7, rtol=2e-7, what="adam gscale")
    # SGD with momentum, Adagrad
    pr = p0.copy(); st = {}
    cfg = dict(learningRate=0.02, momentum=0.9)
    p_d, mom = dev(p0, d), ctx.zeros(n)
    for t in range(3):
        g = rng.standard_normal(n).astype(np.float32)
        O.interruptable_sgd(lambda x: (0.0, g), pr, cfg, st)
        ctx.check(ctx.lib.fg_sgd_fused(ctx.h, p_d.data_ptr(), dev(g, d).data_ptr(), mom.data_ptr(), n, 1.0, 0.0, 0.0, 0.0,
                                       0.02, 0.9, 0.9, 0.0, 0, 1 if t == 0 else 0))
        close(p_d.cpu().numpy(), pr, atol=1e-5, what="sgd")
    pr = p0.copy(); st = {}
    p_d, var = dev(p0, d), ctx.zeros(n)
    for t in range(3):
        g = rng.standard_normal(n).astype(np.float32)
        O.interruptable_adagrad(lambda x: (0.0, g), pr, {}, st)
        ctx.check(ctx.lib.fg_adagrad_fused(ctx.h, p_d.data_ptr(), dev(g, d).data_ptr(), var.data_ptr(), n, 1.0, 0.0, 0.0,
                                           0.0, 1e-3))
        close(p_d.cpu().numpy(), pr, atol=1e-6, what="adagrad")
    out = ctx.empty(2); scr = ctx.empty(1024)
    ctx.check(ctx.lib.fg_norms(ctx.h, dev(p0, d).data_ptr(), n, out.data_ptr(), scr.data_ptr()))
    o = out.cpu().numpy()
    assert abs(o[0] - np.abs(p0.astype(np.float64)).sum()) < BAR["norms_rtol"] * o[0]
    assert abs(o[1] - (p0.astype(np.float64) ** 2).sum()) < BAR["norms_rtol"] * o[1]


def test_philox_rng(ctx):
    a = ctx.uniform((1 << 20,), -1.0, 1.0, seed=1, offset=0).cpu().numpy()
    b = ctx.uniform((1 << 20,), -1.0, 1.0, seed=1, offset=0).cpu().numpy()
    c = ctx.uniform((1 << 20,), -1.0, 1.0, seed=2, offset=0).cpu().numpy()
    assert (a == b).all() and (a != c).mean() > 0.99          # counter based: reproducible, seed-sensitive
    assert a.min() >= -1 and a.max() < 1 and abs(a.mean()) < 5e-3 and abs(a.var() - 1 / 3) < 5e-3
    m = ctx.bernoulli((1 << 20,), 0.8, seed=3).cpu().numpy()
    assert set(np.unique(m)) <= {0.0, 1.0} and abs(m.mean() - 0.8) < 3e-3
    z = ctx.normal((1 << 20,), 0.0, 0.005, seed=4).cpu().numpy()
    assert abs(z.mean()) < 5e-5 and abs(z.std() - 0.005) < 5e-5
    # offset continues the stream (4 values per counter)
    d = ctx.uniform((1024,), -1.0, 1.0, seed=1, offset=256).cpu().numpy()
    assert (d == a[1024:2048]).all()


def _fuzz_cases():
    """Seeded random conv shapes: odd / non power-of-two maps, every channel-count class (thin in / thin out / 64-wide / 128+),
    all kernel sizes, folded upsample, and batch sizes on both sides of the thresholds that select the wave-specialised,
    split-K and bf16x6 kernels."""
    rng = np.random.default_rng(20260925)
    cases = []
    for _ in range(24):
        k = int(rng.choice([3, 3, 3, 5, 7]))
        kind = int(rng.integers(0, 5))
        if kind == 0:   cin, cout = int(rng.choice([1, 3, 4])), int(rng.choice([64, 128]))      # thin in
        elif kind == 1: cin, cout = int(rng.choice([64, 128])), int(rng.choice([1, 3]))         # thin out
        elif kind == 2: cin, cout = 64, int(rng.choice([64, 128]))
        else:           cin, cout = int(rng.choice([128, 256])), int(rng.choice([128, 256]))
        up = int(kind >= 2 and k != 7 and rng.random() < 0.4)
        h, w = int(rng.integers(3, 20)), int(rng.integers(3, 20))
        if rng.random() < 0.5: h, w = int(rng.choice([4, 8, 16])), int(rng.choice([4, 8, 16, 32]))
        b = int(rng.choice([1, 2, 3, 5, 16, 33, 64]))
        if b * h * w * max(cin, cout) * (4 if up else 1) > 6e6:     # keep the numpy reference to a second or two
            b = max(1, int(6e6 // (h * w * max(cin, cout) * (4 if up else 1))))
        cases.append((b, h, w, cin, cout, k, up))
    return cases


@pytest.mark.parametrize("math", [0, 6])
@pytest.mark.parametrize("case", _fuzz_cases())
def test_conv2d_random_shapes_both_math_modes(ctx, case, math):
    from face_generator_amd import ops
    B, H, W, Cin, Cout, k, up = case
    rng = np.random.default_rng(hash(case) % (2 ** 31))
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
    prev = ctx.get_math()
    ctx.set_math(math)
    try:
        w_d, b_d = dev(conv.weight, d), dev(conv.bias, d)
        y_d = ops.conv2d_forward(nhwc(x, d), w_d, b_d, upsample2x=bool(up))
        close(nchw(y_d), y, atol=2e-5 * max(np.abs(y).max(), 1), what="conv fwd %s" % (case,))
        gx_d = ops.conv2d_backward_data(nhwc(gy, d), w_d, (H, W), upsample2x=bool(up))
        close(nchw(gx_d), gx, atol=2e-5 * max(np.abs(gx).max(), 1), what="conv dgrad %s" % (case,))
        gw_d, gb_d = ops.conv2d_backward_weight(nhwc(x, d), nhwc(gy, d), k, upsample2x=bool(up))
        close(gw_d.cpu().numpy(), conv.gradWeight, atol=3e-5 * max(np.abs(conv.gradWeight).max(), 1), what="conv wgrad %s" % (case,))
        close(gb_d.cpu().numpy(), conv.gradBias, atol=3e-5 * max(np.abs(conv.gradBias).max(), 1), what="conv bgrad %s" % (case,))
    finally:
        ctx.set_math(prev)
