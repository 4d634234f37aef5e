"""The memory contract of the module-level entries of include/facegen_hip.h (tests/mem_contract.py): every operand sits in one guarded
arena at exactly the alignment the header promises, workspaces and scratch are exactly as long as the size functions state, and each
entry runs with its outputs and workspace pre-filled with NaN, 0 and 1e30 while the bytes behind its inputs hold NaN, 0 and a
pattern.  Guards untouched, inputs untouched, results bit-identical across the fills and free of NaN, and equal to the oracle at the
bars of tests/test_gpu_ops.py / tests/test_gpu_wino.py (gpu_util.BAR).  Accumulating outputs (beta / acc) get a fourth run with
beta = 1 on a known prefill.  One case per kernel family, at the smallest shape of the existing case lists that selects it.
The net, step and sampler levels: tests/test_gpu_memory_contract_nets.py; the size functions alone: tests/test_workspace_bounds_host.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from oracle import image_scale as IS
from gpu_util import close, BAR
from mem_contract import Arena, run_contract, run_accumulate

pytestmark = pytest.mark.gpu

WINO_BITS = 32 | 64 | 128 | 256


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def to_nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if a.ndim == 4 else a


def arena_for(ctx, *sizes):
    return Arena.sized(ctx.device, [int(s) for s in sizes])


def f64(t):
    return t.cpu().numpy().astype(np.float64)


# ---- convolution ------------------------------------------------------------------------------------------------------------------
CONV_CASES = {
    "generic": (2, 8, 8, 64, 128, 3, 0),
    "ragged_m_odd_map": (3, 6, 5, 32, 64, 3, 0),
    "split_k": (2, 4, 4, 256, 512, 3, 0),
    "folded_5x5": (1, 4, 4, 32, 64, 5, 1),
    "folded_3x3": (2, 8, 8, 64, 64, 3, 1),
    "plain_5x5": (2, 6, 6, 32, 64, 5, 0),
    "7x7": (1, 5, 5, 16, 64, 7, 0),
    "thin_in_3": (2, 32, 32, 3, 64, 3, 0),
    "thin_in_1": (2, 16, 16, 1, 64, 3, 0),
    "thin_out_3": (2, 32, 32, 128, 3, 3, 0),
    "thin_out_1": (2, 16, 16, 128, 1, 3, 0),
    "thin_out_cw64": (2, 8, 8, 64, 3, 3, 0),
    "thin_out_k5": (2, 9, 7, 64, 3, 5, 0),          # k = 5 on an odd map (the two-pass forward needs the net's scratch: nets module)
    "ragged_channels": (2, 8, 8, 6, 10, 3, 0),
    "ragged_one_in": (3, 6, 6, 1, 32, 3, 0),
    "ragged_folded": (2, 4, 4, 10, 6, 3, 1),
    "wave_specialised_wgrad": (2, 64, 64, 64, 128, 3, 0),
    # tests/test_gpu_wino.py WGRAD_CASES: half a chunk, a ragged last chunk, 5x5 groups crossing the border
    "wino_half_chunk": (1, 4, 4, 64, 128, 3, 0),
    "wino_ragged_chunk": (5, 4, 4, 128, 64, 3, 0),
    "wino_5x5_border": (7, 4, 4, 64, 64, 5, 0),
}
WINO_WGRAD_ONLY = ("wino_half_chunk", "wino_ragged_chunk", "wino_5x5_border")
MAIN = [n for n in CONV_CASES if n not in WINO_WGRAD_ONLY]
# (case, fusion: None = the context's default / "nowino" = Winograd bits cleared, math mode, fg_test_set_wino_wgrad_thresholds)
CONV_RUNS = [(n, None, 0, None) for n in MAIN] + [(n, "nowino", 0, None) for n in MAIN] + \
            [(n, None, 0, (1, 1)) for n in WINO_WGRAD_ONLY + ("generic", "split_k", "folded_5x5", "folded_3x3")] + \
            [(n, f, 6, None) for n in ("generic", "ragged_m_odd_map", "split_k") for f in (None, "nowino")]


@functools.lru_cache(maxsize=None)
def conv_ref(name):
    """the oracle of tests/test_gpu_ops.py::test_conv2d_forward_backward, once per shape"""
    B, H, W, Cin, Cout, k, up = CONV_CASES[name]
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
    return dict(x=to_nhwc(x), w=conv.weight.copy(), b=conv.bias.copy(), gy=to_nhwc(gy), y=to_nhwc(y), gx=to_nhwc(gx),
                gw=conv.gradWeight.copy(), gb=conv.gradBias.copy())


@pytest.mark.parametrize("name,fusion,math,thresholds", CONV_RUNS,
                         ids=["%s-%s-math%d%s" % (n, f or "default", m, "-thresholds1" if t else "") for n, f, m, t in CONV_RUNS])
def test_conv2d(ctx, name, fusion, math, thresholds):
    lib = ctx.lib
    B, H, W, Cin, Cout, k, up = CONV_CASES[name]
    pad = (k - 1) // 2
    r = conv_ref(name)
    prev_f, prev_m = ctx.get_fusion(), ctx.get_math()
    try:
        if fusion == "nowino":
            ctx.set_fusion(prev_f & ~WINO_BITS)
        ctx.set_math(math)
        if thresholds:
            ctx.check(lib.fg_test_set_wino_wgrad_thresholds(ctx.h, *thresholds))
        nb = lib.fg_conv2d_workspace_bytes(B, H, W, Cin, Cout, k, up)
        nws = (nb + 3) // 4
        ar = arena_for(ctx, *(r[n].size for n in ("x", "w", "b", "gy", "y", "gx", "gw", "gb")), nws)
        x, w, b, gy = (ar.put(r[n], name=n) for n in ("x", "w", "b", "gy"))
        y, gx, gw, gb = (ar.take(r[n].size, name=n) for n in ("y", "gx", "gw", "gb"))
        ws = ar.take(nws, name="workspace")
        ins = [x, w, b, gy]
        P = lambda t: t.data_ptr()
        what = "conv %s %s" % (name, CONV_CASES[name],)
        # with the thresholds lowered the weight gradient is the Winograd-domain one: its bar is that of tests/test_gpu_wino.py
        wino = thresholds is not None
        (yo,) = run_contract(ar, lambda: ctx.check(lib.fg_conv2d_forward(ctx.h, P(x), P(w), P(b), P(y), B, H, W, Cin, Cout, k, pad, up, P(ws), nws * 4)),
                             ins, [y], [ws], what=what + " forward")
        close(f64(yo).reshape(r["y"].shape), r["y"], atol=BAR["wino_fwd" if wino and name in WINO_WGRAD_ONLY else "conv_fwd"] * max(np.abs(r["y"]).max(), 1), what=what + " forward")
        (gxo,) = run_contract(ar, lambda: ctx.check(lib.fg_conv2d_backward_data(ctx.h, P(gy), P(w), P(gx), B, H, W, Cin, Cout, k, pad, up, P(ws), nws * 4)),
                              ins, [gx], [ws], what=what + " data gradient")
        close(f64(gxo).reshape(r["gx"].shape), r["gx"], atol=BAR["wino_dgrad" if wino and name in WINO_WGRAD_ONLY else "conv_dgrad"] * max(np.abs(r["gx"]).max(), 1),
              what=what + " data gradient")
        wg = lambda beta: ctx.check(lib.fg_conv2d_backward_weight(ctx.h, P(x), P(gy), P(gw), P(gb), beta, B, H, W, Cin, Cout, k, pad, up, P(ws), nws * 4))
        gwo, gbo = run_contract(ar, lambda: wg(0.0), ins, [gw, gb], [ws], what=what + " weight gradient, beta = 0")
        close(f64(gwo).reshape(r["gw"].shape), r["gw"], atol=BAR["wino_wgrad" if wino else "conv_wgrad"] * max(np.abs(r["gw"]).max(), 1), what=what + " weight gradient")
        close(f64(gbo), r["gb"], atol=BAR["conv_bgrad"] * max(np.abs(r["gb"]).max(), 1), what=what + " bias gradient")
        for (got, want), n in zip(run_accumulate(ar, lambda: wg(1.0), [gw, gb], [gwo, gbo], ins, [ws], what=what + " weight gradient"), ("gw", "gb")):
            close(got, want, atol=BAR["conv_acc"] * max(np.abs(r[n]).max(), 1), what=what + " beta = 1: prefill + " + n)
    finally:
        ctx.set_fusion(prev_f)
        ctx.set_math(prev_m)
        if thresholds:
            ctx.check(lib.fg_test_set_wino_wgrad_thresholds(ctx.h, 0, 0))


# ---- linear -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,N", [(3, 64, 128), (6, 33, 7), (5, 50, 256), (5, 50, 1)])      # N = 1: the gemv path, no workspace
def test_linear(ctx, B, K, N):
    lib = ctx.lib
    rng = np.random.default_rng(B + K + N)
    lin = O.Linear(K, N, rng)
    xh = rng.standard_normal((B, K)).astype(np.float32)
    yh = lin.forward(xh)
    gyh = rng.standard_normal(yh.shape).astype(np.float32)
    gxh = lin.backward(xh, gyh)
    nb = lib.fg_linear_workspace_bytes(B, K, N)
    nws = (nb + 3) // 4
    ar = arena_for(ctx, xh.size, lin.weight.size, N, gyh.size, yh.size, xh.size, lin.weight.size, N, nws)
    x, w, b, gy = ar.put(xh, name="x"), ar.put(lin.weight, name="w"), ar.put(lin.bias, name="b"), ar.put(gyh, name="gy")
    y, gx, gw, gb = ar.take(yh.size, name="y"), ar.take(xh.size, name="gx"), ar.take(lin.weight.size, name="gw"), ar.take(N, name="gb")
    ws = ar.take(nws, name="workspace")
    ins, P, what = [x, w, b, gy], (lambda t: t.data_ptr()), "linear (%d, %d, %d)" % (B, K, N)
    (yo,) = run_contract(ar, lambda: ctx.check(lib.fg_linear_forward(ctx.h, P(x), P(w), P(b), P(y), B, K, N, P(ws), nws * 4)), ins, [y], [ws], what=what + " forward")
    close(f64(yo).reshape(yh.shape), yh, atol=BAR["lin"] * max(np.abs(yh).max(), 1), what=what + " forward")
    (gxo,) = run_contract(ar, lambda: ctx.check(lib.fg_linear_backward_data(ctx.h, P(gy), P(w), P(gx), B, K, N, P(ws), nws * 4)), ins, [gx], [ws],
                          what=what + " data gradient")
    close(f64(gxo).reshape(gxh.shape), gxh, atol=BAR["lin"] * max(np.abs(gxh).max(), 1), what=what + " data gradient")
    wg = lambda beta: ctx.check(lib.fg_linear_backward_weight(ctx.h, P(x), P(gy), P(gw), P(gb), beta, B, K, N, P(ws), nws * 4))
    gwo, gbo = run_contract(ar, lambda: wg(0.0), ins, [gw, gb], [ws], what=what + " weight gradient, beta = 0")
    close(f64(gwo).reshape(lin.gradWeight.shape), lin.gradWeight, atol=BAR["lin"] * max(np.abs(lin.gradWeight).max(), 1), what=what + " weight gradient")
    close(f64(gbo), lin.gradBias, atol=BAR["lin"] * max(np.abs(lin.gradBias).max(), 1), what=what + " bias gradient")
    for (got, want), ref in zip(run_accumulate(ar, lambda: wg(1.0), [gw, gb], [gwo, gbo], ins, [ws], what=what + " weight gradient"),
                                (lin.gradWeight, lin.gradBias)):
        close(got, want, atol=BAR["conv_acc"] * max(np.abs(ref).max(), 1), what=what + " beta = 1")


# ---- BatchNorm (+ PReLU) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(3, 7, 5, 128), (2, 8, 8, 64)])
@pytest.mark.parametrize("prelu", [True, False])
def test_batchnorm(ctx, B, H, W, C, prelu):
    lib = ctx.lib
    rng = np.random.default_rng(C + B)
    bn = O.SpatialBatchNormalization(C, rng=rng)
    bn.bias[...] = rng.standard_normal(C).astype(np.float32) * 0.3
    pr = O.PReLU()
    xh = (rng.standard_normal((B, C, H, W)) * 1.7 + 0.9).astype(np.float32)
    z = bn.forward(xh)
    yh = pr.forward(z) if prelu else z
    gyh = rng.standard_normal(yh.shape).astype(np.float32)
    gxh = bn.backward(xh, pr.backward(z, gyh) if prelu else gyh)
    rows, n = B * H * W, xh.size
    nscr = lib.fg_bn_scratch_floats(C)
    ar = arena_for(ctx, n, C, C, 1, n, n, n, C, C, C, C, C, C, 1, nscr)
    x, gamma, beta, slope, gy = ar.put(to_nhwc(xh), name="x"), ar.put(bn.weight, name="gamma"), ar.put(bn.bias, name="beta"), ar.put(pr.weight, name="slope"), ar.put(to_nhwc(gyh), name="gy")
    y, gx, mean, invstd = ar.take(n, name="y"), ar.take(n, name="gx"), ar.take(C, name="save_mean"), ar.take(C, name="save_invstd")
    rm, rv = ar.take(C, name="running_mean"), ar.take(C, name="running_var")
    gg, gb, gs = ar.take(C, name="ggamma"), ar.take(C, name="gbeta"), ar.take(1, name="gslope")
    scr = ar.take(nscr, name="scratch")
    P, sl, what = (lambda t: t.data_ptr()), (slope.data_ptr() if prelu else None), "batchnorm (%d, %d, %d, %d)%s" % (B, H, W, C, " + PReLU" if prelu else "")
    ins = [x, gamma, beta, slope, gy]
    rm0, rv0 = torch.zeros(C), torch.ones(C)
    fwd = lambda train: ctx.check(lib.fg_batchnorm_forward(ctx.h, P(x), P(y), rows, C, P(gamma), P(beta), sl, P(mean), P(invstd), P(rm), P(rv), 1e-5, 0.1, train, P(scr)))
    yo, mo, io, rmo, rvo = run_contract(ar, lambda: fwd(1), ins, [y, mean, invstd], [scr], inout=[(rm, rm0), (rv, rv0)], what=what + " forward (train)")
    close(f64(yo).reshape(B, H, W, C), to_nhwc(yh), atol=BAR["bn_y"], what=what + " forward")
    close(f64(mo), bn.save_mean, atol=BAR["bn_mean"], what=what + " mean")
    close(f64(io), bn.save_invstd, atol=0, rtol=BAR["bn_invstd_rtol"], what=what + " invstd")
    close(f64(rmo), bn.running_mean, atol=BAR["bn_running_mean"], what=what + " running_mean")
    close(f64(rvo), bn.running_var, atol=0, rtol=BAR["bn_running_var_rtol"], what=what + " running_var")
    # backward: the saved statistics are inputs now; ggamma / gbeta / gslope poisoned with acc = 0
    mean.copy_(mo); invstd.copy_(io)
    bwd = lambda acc: ctx.check(lib.fg_batchnorm_backward(ctx.h, P(x), P(gy), P(gx), rows, C, P(gamma), P(beta), sl, P(mean), P(invstd), P(gg), P(gb),
                                                          P(gs) if prelu else None, acc, P(scr)))
    outs = [gx, gg, gb] + ([gs] if prelu else [])
    res = run_contract(ar, lambda: bwd(0.0), ins + [mean, invstd], outs, [scr], what=what + " backward, acc = 0")
    close(f64(res[0]).reshape(B, H, W, C), to_nhwc(gxh), atol=BAR["bn_gx"] * max(1, np.abs(gxh).max()), what=what + " gx")
    close(f64(res[1]), bn.gradWeight, atol=BAR["bn_gparam"] * max(1, np.abs(bn.gradWeight).max()), what=what + " ggamma")
    close(f64(res[2]), bn.gradBias, atol=BAR["bn_gparam"] * max(1, np.abs(bn.gradBias).max()), what=what + " gbeta")
    refs = [bn.gradWeight, bn.gradBias]
    if prelu:
        close(f64(res[3]), pr.gradWeight, atol=BAR["bn_gparam"] * max(1, abs(pr.gradWeight[0])), what=what + " gslope")
        refs.append(pr.gradWeight)
    for (got, want), ref in zip(run_accumulate(ar, lambda: bwd(1.0), outs[1:], res[1:], ins + [mean, invstd], [scr], what=what + " backward"), refs):
        close(got, want, atol=BAR["conv_acc"] * max(1, np.abs(ref).max()), what=what + " acc = 1")
    # evaluate mode reads the running statistics and writes neither them nor the saved ones' guards
    bn.evaluate()
    ze = bn.forward(xh)
    yeh = pr.forward(ze) if prelu else ze
    rm.copy_(rmo); rv.copy_(rvo)
    (ye,) = run_contract(ar, lambda: fwd(0), ins + [rm, rv], [y], [scr, mean, invstd], what=what + " forward (evaluate)")
    close(f64(ye).reshape(B, H, W, C), to_nhwc(yeh), atol=BAR["bn_y"], what=what + " evaluate")


# ---- PReLU (+ Dropout), PReLU + SpatialDropout + AvgPool ----------------------------------------------------------------------------
def test_prelu(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(7)
    xh = rng.standard_normal((6, 511)).astype(np.float32)                   # n = 3066: not a multiple of 4
    pr, dr = O.PReLU(), O.Dropout(0.5)
    pr.weight[0] = 0.3
    mh = (rng.random(xh.shape) < 0.5).astype(np.float32)
    dr.set_mask(mh)
    yh = dr.forward(pr.forward(xh))
    gyh = rng.standard_normal(yh.shape).astype(np.float32)
    gxh = pr.backward(xh, dr.backward(pr.output, gyh))
    n = xh.size
    ar = arena_for(ctx, n, 1, n, n, n, n, 1, 1024)
    x, slope, mask, gy = ar.put(xh, name="x"), ar.put(pr.weight, name="slope"), ar.put(mh, name="mask"), ar.put(gyh, name="gy")
    y, gx, gs, scr = ar.take(n, name="y"), ar.take(n, name="gx"), ar.take(1, name="gslope"), ar.take(1024, name="scratch")
    P, ins = (lambda t: t.data_ptr()), [x, slope, mask, gy]
    (yo,) = run_contract(ar, lambda: ctx.check(lib.fg_prelu_forward(ctx.h, P(x), P(slope), P(mask), 2.0, P(y), n)), ins, [y], what="prelu forward")
    close(f64(yo).reshape(yh.shape), yh, atol=BAR["prelu"], what="prelu forward")
    bwd = lambda acc: ctx.check(lib.fg_prelu_backward(ctx.h, P(x), P(gy), P(slope), P(mask), 2.0, P(gx), P(gs), acc, n, P(scr)))
    gxo, gso = run_contract(ar, lambda: bwd(0.0), ins, [gx, gs], [scr], what="prelu backward, acc = 0")
    close(f64(gxo).reshape(gxh.shape), gxh, atol=BAR["prelu"], what="prelu gx")
    close(f64(gso), pr.gradWeight, atol=BAR["slope_grad"], what="prelu slope gradient")
    ((got, want),) = run_accumulate(ar, lambda: bwd(1.0), [gs], [gso], ins, [scr], what="prelu backward")
    close(got, want, atol=BAR["slope_grad"], what="prelu acc = 1")


def test_actpool(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(8)
    B, C, H, W = 3, 64, 8, 6
    xh = rng.standard_normal((B, C, H, W)).astype(np.float32)
    pr, sd, ap = O.PReLU(), O.SpatialDropout(0.2), O.SpatialAveragePooling()
    pr.weight[0] = -0.1
    mh = (rng.random((B, C)) < 0.8).astype(np.float32)
    sd.set_mask(mh)
    yh = ap.forward(sd.forward(pr.forward(xh)))
    gyh = rng.standard_normal(yh.shape).astype(np.float32)
    gxh = pr.backward(xh, sd.backward(pr.output, ap.backward(sd.output, gyh)))
    ar = arena_for(ctx, xh.size, 1, mh.size, gyh.size, yh.size, xh.size, 1, 1024)
    x, slope, mask, gy = ar.put(to_nhwc(xh), name="x"), ar.put(pr.weight, name="slope"), ar.put(mh, name="mask"), ar.put(to_nhwc(gyh), name="gy")
    y, gx, gs, scr = ar.take(yh.size, name="y"), ar.take(xh.size, name="gx"), ar.take(1, name="gslope"), ar.take(1024, name="scratch")
    P, ins = (lambda t: t.data_ptr()), [x, slope, mask, gy]
    (yo,) = run_contract(ar, lambda: ctx.check(lib.fg_actpool_forward(ctx.h, P(x), P(slope), P(mask), 1.0, P(y), B, H, W, C)), ins, [y], what="actpool forward")
    close(f64(yo).reshape(to_nhwc(yh).shape), to_nhwc(yh), atol=BAR["prelu"], what="actpool forward")
    bwd = lambda acc: ctx.check(lib.fg_actpool_backward(ctx.h, P(x), P(gy), P(slope), P(mask), 1.0, P(gx), P(gs), acc, B, H, W, C, P(scr)))
    gxo, gso = run_contract(ar, lambda: bwd(0.0), ins, [gx, gs], [scr], what="actpool backward, acc = 0")
    close(f64(gxo).reshape(to_nhwc(gxh).shape), to_nhwc(gxh), atol=BAR["prelu"], what="actpool gx")
    close(f64(gso), pr.gradWeight, atol=BAR["slope_grad"], what="actpool slope gradient")
    ((got, want),) = run_accumulate(ar, lambda: bwd(1.0), [gs], [gso], ins, [scr], what="actpool backward")
    close(got, want, atol=BAR["slope_grad"], what="actpool acc = 1")


# ---- pointwise entries: (inputs) -> (outputs), exact numpy references ------------------------------------------------------------------
def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def check_simple(ctx, what, host_inputs, out_sizes, call, refs, atols, aligns=None, scratch=()):
    """host_inputs: numpy arrays; call(inputs, outputs, scratch) launches; refs: expected arrays (flattened compare)"""
    ar = arena_for(ctx, *[a.size for a in host_inputs], *out_sizes, *scratch)
    aligns = aligns or [256] * len(host_inputs)
    ins = [ar.put(a, align=al, name="input%d" % i) for i, (a, al) in enumerate(zip(host_inputs, aligns))]
    outs = [ar.take(n, name="output%d" % i) for i, n in enumerate(out_sizes)]
    scr = [ar.take(n, name="scratch%d" % i) for i, n in enumerate(scratch)]
    res = run_contract(ar, lambda: ctx.check(call(ins, outs, scr)), ins, outs, scr, what=what)
    for i, (r, ref, atol) in enumerate(zip(res, refs, atols)):
        if ref is None:
            continue
        if atol == 0:
            assert np.array_equal(r.cpu().numpy().reshape(-1), np.asarray(ref, np.float32).reshape(-1)), "%s: output %d differs from the reference" % (what, i)
        else:
            close(f64(r).reshape(-1), np.asarray(ref).reshape(-1), atol=atol, what="%s output %d" % (what, i))
    return res


def test_dropout_entries(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(21)
    B, HW, C = 3, 35, 6
    x = rng.standard_normal((B, HW, C)).astype(np.float32)
    m = (rng.random((B, C)) < 0.8).astype(np.float32)
    check_simple(ctx, "fg_spatial_dropout_apply", [x, m], [x.size],
                 lambda i, o, s: lib.fg_spatial_dropout_apply(h, i[0].data_ptr(), i[1].data_ptr(), 1.25, o[0].data_ptr(), B, HW, C),
                 [(x * m[:, None, :] * np.float32(1.25))], [1e-6])
    x = rng.standard_normal(1003).astype(np.float32)
    m = (rng.random(1003) < 0.5).astype(np.float32)
    check_simple(ctx, "fg_dropout_apply", [x, m], [x.size], lambda i, o, s: lib.fg_dropout_apply(h, i[0].data_ptr(), i[1].data_ptr(), 2.0, o[0].data_ptr(), 1003),
                 [x * m * np.float32(2.0)], [0])
    check_simple(ctx, "fg_dropout_apply (no mask)", [x], [x.size], lambda i, o, s: lib.fg_dropout_apply(h, i[0].data_ptr(), None, 0.5, o[0].data_ptr(), 1003),
                 [x * np.float32(0.5)], [0])


def test_pools_and_upsample(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(22)
    P = lambda t: t.data_ptr()
    ap, mp, up = O.SpatialAveragePooling(), O.SpatialMaxPooling(2, 2), O.SpatialUpSamplingNearest(2)
    # average pooling takes even maps only (an odd one is refused before anything is launched): 6 x 10, C not a multiple of 4
    B, C, H, W = 2, 6, 6, 10
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    g2 = rng.standard_normal((B, C, H // 2, W // 2)).astype(np.float32)
    check_simple(ctx, "fg_avgpool2x2_forward", [to_nhwc(x)], [g2.size], lambda i, o, s: lib.fg_avgpool2x2_forward(h, P(i[0]), P(o[0]), B, H, W, C),
                 [to_nhwc(ap.forward(x))], [BAR["avgpool_fwd"]])
    check_simple(ctx, "fg_avgpool2x2_backward", [to_nhwc(g2)], [x.size], lambda i, o, s: lib.fg_avgpool2x2_backward(h, P(i[0]), P(o[0]), B, H, W, C),
                 [to_nhwc(ap.backward(x, g2))], [BAR["avgpool_bwd"]])
    assert lib.fg_avgpool2x2_forward(h, 64, 64, B, 5, 6, C) < 0 and lib.fg_avgpool2x2_backward(h, 64, 64, B, 5, 6, C) < 0
    # max pooling: even maps too, and c % 4 == 0 in the forward pass (include/facegen_hip.h); the backward pass takes any c
    C8 = 8
    x8 = rng.standard_normal((B, C8, H, W)).astype(np.float32)
    g8 = rng.standard_normal((B, C8, H // 2, W // 2)).astype(np.float32)
    check_simple(ctx, "fg_maxpool2x2_forward", [to_nhwc(x8)], [g8.size], lambda i, o, s: lib.fg_maxpool2x2_forward(h, P(i[0]), P(o[0]), B, H, W, C8),
                 [to_nhwc(mp.forward(x8))], [0])
    mp.forward(x)
    check_simple(ctx, "fg_maxpool2x2_backward", [to_nhwc(x), to_nhwc(g2)], [x.size],
                 lambda i, o, s: lib.fg_maxpool2x2_backward(h, P(i[0]), P(i[1]), P(o[0]), B, H, W, C), [to_nhwc(mp.backward(x, g2))], [0])
    assert lib.fg_maxpool2x2_forward(h, 64, 64, B, 5, 6, C8) < 0 and lib.fg_maxpool2x2_forward(h, 64, 64, B, 6, 6, 6) < 0
    assert lib.fg_maxpool2x2_backward(h, 64, 64, 64, B, 5, 6, C8) < 0
    # up-sampling on an odd map: 5 x 6
    H, W = 5, 6
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    gy = rng.standard_normal((B, C, 2 * H, 2 * W)).astype(np.float32)
    check_simple(ctx, "fg_upsample_nearest2x_forward", [to_nhwc(x)], [gy.size], lambda i, o, s: lib.fg_upsample_nearest2x_forward(h, P(i[0]), P(o[0]), B, H, W, C),
                 [to_nhwc(up.forward(x))], [BAR["upsample_fwd"]])
    check_simple(ctx, "fg_upsample_nearest2x_backward", [to_nhwc(gy)], [x.size], lambda i, o, s: lib.fg_upsample_nearest2x_backward(h, P(i[0]), P(o[0]), B, H, W, C),
                 [to_nhwc(up.backward(x, gy))], [BAR["upsample_bwd"]])


def test_conv_upsample_view(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(23)
    B, hh, ww, C, f = 2, 3, 5, 8, 2
    v = rng.standard_normal((B, C, hh, ww)).astype(np.float32)                 # the convolution's NCHW output
    u = v.reshape(B, C // (f * f), hh * f, ww * f)                             # Tensor:view on contiguous NCHW memory
    P = lambda t: t.data_ptr()
    check_simple(ctx, "fg_conv_upsample_view_forward", [to_nhwc(v)], [v.size], lambda i, o, s: lib.fg_conv_upsample_view_forward(h, P(i[0]), P(o[0]), B, hh, ww, C, f),
                 [to_nhwc(u)], [0])
    check_simple(ctx, "fg_conv_upsample_view_backward", [to_nhwc(u)], [v.size], lambda i, o, s: lib.fg_conv_upsample_view_backward(h, P(i[0]), P(o[0]), B, hh, ww, C, f),
                 [to_nhwc(v)], [0])


def test_concat_split_add(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(24)
    npix, ca, cb = 37, 1, 3
    a, b = rng.standard_normal((npix, ca)).astype(np.float32), rng.standard_normal((npix, cb)).astype(np.float32)
    P = lambda t: t.data_ptr()
    j = np.concatenate([a, b], axis=1)
    check_simple(ctx, "fg_concat_channels", [a, b], [j.size], lambda i, o, s: lib.fg_concat_channels(h, P(i[0]), P(i[1]), P(o[0]), npix, ca, cb), [j], [0])
    check_simple(ctx, "fg_split_channels", [j], [a.size, b.size], lambda i, o, s: lib.fg_split_channels(h, P(i[0]), P(o[0]), P(o[1]), npix, ca, cb), [a, b], [0, 0])
    npix, ca, cb = 9, 6, 5
    a, b = rng.standard_normal((npix, ca)).astype(np.float32), rng.standard_normal((npix, cb)).astype(np.float32)
    j = np.concatenate([a, b], axis=1)
    check_simple(ctx, "fg_concat_channels (6 + 5)", [a, b], [j.size], lambda i, o, s: lib.fg_concat_channels(h, P(i[0]), P(i[1]), P(o[0]), npix, ca, cb), [j], [0])
    check_simple(ctx, "fg_split_channels (6 + 5)", [j], [a.size, b.size], lambda i, o, s: lib.fg_split_channels(h, P(i[0]), P(o[0]), P(o[1]), npix, ca, cb), [a, b], [0, 0])
    x, y = rng.standard_normal(1003).astype(np.float32), rng.standard_normal(1003).astype(np.float32)
    check_simple(ctx, "fg_add", [x, y], [1003], lambda i, o, s: lib.fg_add(h, P(i[0]), P(i[1]), P(o[0]), 1003), [x + y], [0])


@pytest.mark.parametrize("widths,rows,align", [((8, 128, 4), 5, 16), ((7, 128, 2), 5, 256), ((1, 2, 3, 5), 129, 256)])
def test_join_split_sum(ctx, widths, rows, align):
    """all widths multiples of 4 with the parts on exactly 16 bytes (the header's condition for 16-byte accesses), and ragged widths"""
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(sum(widths) + rows)
    parts = [rng.standard_normal((rows, w)).astype(np.float32) for w in widths]
    wd = (ctypes.c_int * len(widths))(*widths)
    j = np.concatenate(parts, axis=1)
    P = lambda t: t.data_ptr()
    check_simple(ctx, "fg_join_rows %s" % (widths,), parts, [j.size], lambda i, o, s: lib.fg_join_rows(h, _ptrs(i), wd, len(widths), P(o[0]), rows), [j], [0],
                 aligns=[align] * len(parts))
    check_simple(ctx, "fg_split_rows %s" % (widths,), [j], [p.size for p in parts], lambda i, o, s: lib.fg_split_rows(h, P(i[0]), _ptrs(o), wd, len(widths), rows),
                 parts, [0] * len(parts), aligns=[align])
    count = rows * widths[0] + (0 if align == 16 else 1)
    ps = [(rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in widths]
    want = ps[0].copy()
    for p in ps[1:]:
        want = (want + p).astype(np.float32)
    check_simple(ctx, "fg_sum_n n = %d" % len(ps), ps, [count], lambda i, o, s: lib.fg_sum_n(h, _ptrs(i), len(ps), P(o[0]), count), [want], [0], aligns=[align] * len(ps))


def test_sigmoid_leakyrelu(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(25)
    n = 1003
    x, gy = rng.standard_normal((n, 1)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32)
    sg, lr = O.Sigmoid(), O.LeakyReLU(0.333)
    ys = sg.forward(x)
    P = lambda t: t.data_ptr()
    check_simple(ctx, "fg_sigmoid_forward", [x], [n], lambda i, o, s: lib.fg_sigmoid_forward(h, P(i[0]), P(o[0]), n), [ys], [BAR["sigmoid"]])
    check_simple(ctx, "fg_sigmoid_backward", [ys, gy], [n], lambda i, o, s: lib.fg_sigmoid_backward(h, P(i[0]), P(i[1]), P(o[0]), n), [sg.backward(x, gy)], [BAR["sigmoid"]])
    check_simple(ctx, "fg_leakyrelu_forward", [x], [n], lambda i, o, s: lib.fg_leakyrelu_forward(h, P(i[0]), 0.333, P(o[0]), n), [lr.forward(x)], [BAR["leakyrelu"]])
    check_simple(ctx, "fg_leakyrelu_backward", [x, gy], [n], lambda i, o, s: lib.fg_leakyrelu_backward(h, P(i[0]), P(i[1]), 0.333, P(o[0]), n),
                 [lr.backward(x, gy)], [BAR["leakyrelu"]])


def test_bce(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(9)
    B = 5
    p = rng.uniform(0.001, 0.999, B).astype(np.float32)
    p[0] = 1e-9; p[1] = 1.0 - 1e-7
    t = (rng.random(B) < 0.5).astype(np.float32)
    crit = O.BCECriterion()
    f = crit.forward(p.reshape(B, 1), t)
    g = crit.backward(p.reshape(B, 1), t)
    P = lambda v: v.data_ptr()
    loss, grad, conf = check_simple(ctx, "fg_bce_forward_backward", [p, t], [1, B, 4],
                                    lambda i, o, s: lib.fg_bce_forward_backward(h, P(i[0]), P(i[1]), B, P(o[0]), P(o[1]), P(o[2])), [None, None, None], [0, 0, 0])
    assert abs(loss.item() - f) <= BAR["bce_loss_rtol"] * abs(f)
    close(f64(grad), g[:, 0], atol=BAR["bce_grad_atol"], rtol=BAR["bce_grad_rtol"], what="bce grad")
    want = np.zeros(4, np.int64)
    for i in range(B):
        want[(2 if p[i] > 0.5 else 0) + int(t[i])] += 1
    assert (conf.view(torch.int32).cpu().numpy() == want).all()


@pytest.mark.parametrize("n", [1003, 2049])
def test_optimizers_and_norms(ctx, n):
    """p, m, v are in-out (restored before every run, guarded); g is an input; the fill rule applies to g_out alone"""
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(10 + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    gh = (rng.standard_normal(n) * 3.0).astype(np.float32)
    ar = arena_for(ctx, n, n, n, n, n, 2, 1024)
    g = ar.put(gh, name="g")
    p, m, v, gout = ar.take(n, name="p"), ar.take(n, name="m"), ar.take(n, name="v"), ar.take(n, name="g_out")
    out2, scr = ar.take(2, name="norms"), ar.take(1024, name="scratch")
    P = lambda t: t.data_ptr()
    z, pt = torch.zeros(n), torch.tensor(p0)
    # Adam with L2 penalty + clamp, first step (tests/test_gpu_ops.py)
    p_ref, st = p0.copy(), {}
    O.interruptable_adam(lambda x: (0.0, np.clip(gh + p0 * np.float32(1e-4), -1, 1).astype(np.float32)), p_ref, {}, st)
    go, po, mo, vo = run_contract(ar, lambda: ctx.check(lib.fg_adam_fused(h, P(p), P(g), P(m), P(v), n, 1.0, 0.0, 1e-4, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1, P(gout))),
                                  [g], [gout], inout=[(p, pt), (m, z), (v, z)], what="fg_adam_fused n = %d" % n)
    close(f64(po), p_ref, atol=2e-7, rtol=2e-7, what="adam p")
    close(f64(mo), st['m'], atol=1e-7, rtol=1e-5, what="adam m")
    close(f64(vo), st['v'], atol=1e-12, rtol=1e-5, what="adam v")
    close(f64(go), np.clip(gh + p0 * np.float32(1e-4), -1, 1), atol=1e-6, what="adam g_out")
    p_ref = p0.copy()
    O.interruptable_sgd(lambda x: (0.0, gh), p_ref, dict(learningRate=0.02, momentum=0.9), {})
    po, mo = run_contract(ar, lambda: ctx.check(lib.fg_sgd_fused(h, P(p), P(g), P(m), n, 1.0, 0.0, 0.0, 0.0, 0.02, 0.9, 0.9, 0.0, 0, 1)),
                          [g], [], inout=[(p, pt), (m, z)], what="fg_sgd_fused n = %d" % n)
    close(f64(po), p_ref, atol=1e-5, what="sgd")
    p_ref = p0.copy()
    O.interruptable_adagrad(lambda x: (0.0, gh), p_ref, {}, {})
    po, vo = run_contract(ar, lambda: ctx.check(lib.fg_adagrad_fused(h, P(p), P(g), P(v), n, 1.0, 0.0, 0.0, 0.0, 1e-3)),
                          [g], [], inout=[(p, pt), (v, z)], what="fg_adagrad_fused n = %d" % n)
    close(f64(po), p_ref, atol=1e-6, what="adagrad")
    (o,) = run_contract(ar, lambda: ctx.check(lib.fg_norms(h, P(g), n, P(out2), P(scr))), [g], [out2], [scr], what="fg_norms n = %d" % n)
    o = o.cpu().numpy()
    assert abs(o[0] - np.abs(gh.astype(np.float64)).sum()) < BAR["norms_rtol"] * o[0]
    assert abs(o[1] - (gh.astype(np.float64) ** 2).sum()) < BAR["norms_rtol"] * o[1]


@pytest.mark.parametrize("n", [1, 5, 1023])
def test_rng(ctx, n):
    """the kernel works in quads: the last one is cut at n.  Reference: the first n values of a longer draw of the same stream."""
    lib, h = ctx.lib, ctx.h
    P = lambda t: t.data_ptr()
    for what, call, longer in (
            ("fg_rng_uniform", lambda o, k: lib.fg_rng_uniform(h, 5, 7, P(o), k, -1.0, 1.0), ctx.uniform((2048,), -1.0, 1.0, 5, 7)),
            ("fg_rng_bernoulli", lambda o, k: lib.fg_rng_bernoulli(h, 5, 7, P(o), k, 0.8), ctx.bernoulli((2048,), 0.8, 5, 7)),
            ("fg_rng_normal", lambda o, k: lib.fg_rng_normal(h, 5, 7, P(o), k, 0.5, 2.0), ctx.normal((2048,), 0.5, 2.0, 5, 7))):
        check_simple(ctx, "%s n = %d" % (what, n), [], [n], lambda i, o, s: call(o[0], n), [longer[:n].cpu().numpy()], [0])


def test_layout_fill_axpby(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(26)
    x = rng.standard_normal((3, 5, 7, 6)).astype(np.float32)                   # NCHW, c = 5
    n, c, hh, ww = x.shape
    P = lambda t: t.data_ptr()
    check_simple(ctx, "fg_nchw_to_nhwc", [x], [x.size], lambda i, o, s: lib.fg_nchw_to_nhwc(h, P(i[0]), P(o[0]), n, c, hh, ww), [to_nhwc(x)], [0])
    check_simple(ctx, "fg_nhwc_to_nchw", [to_nhwc(x)], [x.size], lambda i, o, s: lib.fg_nhwc_to_nchw(h, P(i[0]), P(o[0]), n, c, hh, ww), [x], [0])
    check_simple(ctx, "fg_fill", [], [1003], lambda i, o, s: lib.fg_fill(h, P(o[0]), 0.25, 1003), [np.full(1003, 0.25, np.float32)], [0])
    a, y0 = rng.standard_normal(1003).astype(np.float32), rng.standard_normal(1003).astype(np.float32)
    ar = arena_for(ctx, 1003, 1003)
    xa, y = ar.put(a, name="x"), ar.take(1003, name="y")
    (yo,) = run_contract(ar, lambda: ctx.check(lib.fg_axpby(h, 0.5, P(xa), 2.0, P(y), 1003)), [xa], [], inout=[(y, torch.tensor(y0))], what="fg_axpby")
    close(f64(yo), 0.5 * a.astype(np.float64) + 2.0 * y0, atol=1e-6, what="fg_axpby")
    # b = 0 overwrites: y may hold anything
    (yo,) = run_contract(ar, lambda: ctx.check(lib.fg_axpby(h, 0.5, P(xa), 0.0, P(y), 1003)), [xa], [y], what="fg_axpby, b = 0")
    assert np.array_equal(yo.cpu().numpy(), a * np.float32(0.5))


@pytest.mark.parametrize("hs,ws,hd,wd", [(5, 7, 9, 13), (9, 13, 4, 5)])
@pytest.mark.parametrize("layout", [0, 1])
def test_scale_bilinear(ctx, hs, ws, hd, wd, layout):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(hs * 1000 + ws * 10 + hd)
    N, C = 3, 3
    x = rng.standard_normal((N, C, hs, ws)).astype(np.float32)
    want = np.stack([IS.scale(img, wd, hd) for img in x])
    lay = (lambda a: a) if layout else to_nhwc
    P = lambda t: t.data_ptr()
    check_simple(ctx, "fg_scale_bilinear layout %d" % layout, [lay(x)], [want.size],
                 lambda i, o, s: lib.fg_scale_bilinear(h, P(i[0]), P(o[0]), N, C, hs, ws, hd, wd, layout), [lay(want)], [0])


@pytest.mark.parametrize("layout", [0, 1])
def test_c2f_coarse_diff(ctx, layout):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(27)
    N, C, S, cs = 3, 3, 10, 5
    fine = rng.uniform(0, 1, (N, C, S, S)).astype(np.float32)
    want_c, want_d = IS.to_result(fine, cs, S)
    lay = (lambda a: a) if layout else to_nhwc
    P = lambda t: t.data_ptr()
    check_simple(ctx, "fg_c2f_coarse_diff layout %d" % layout, [lay(fine)], [fine.size, fine.size],
                 lambda i, o, s: lib.fg_c2f_coarse_diff(h, P(i[0]), P(o[0]), P(o[1]), P(s[0]), N, C, S, cs, layout), [lay(want_c), lay(want_d)], [0, 0],
                 scratch=[N * C * cs * cs])                                       # tmp: exactly n * c * cs * cs floats


# gen + cond and the difference to `fine` are fp32 operations (2^-24 relative each, restated below), the squares are summed in double and
# the root is rounded to fp32 once (2^-24): a few 1e-7 relative in all -- 1e-6 of the largest distance
PARZEN_RTOL = 1e-6


def test_parzen_min_dist(ctx):
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(28)
    n, elems = 5, 3 * 7 * 7
    gen = rng.standard_normal((n, elems)).astype(np.float32)
    cond, fine = rng.standard_normal(elems).astype(np.float32), rng.standard_normal(elems).astype(np.float32)
    d = np.sqrt((((gen + cond).astype(np.float32).astype(np.float64) - fine) ** 2).sum(axis=1))
    P = lambda t: t.data_ptr()
    dist, mn = check_simple(ctx, "fg_parzen_min_dist", [gen, cond, fine], [n, 1],
                            lambda i, o, s: lib.fg_parzen_min_dist(h, P(i[0]), P(i[1]), P(i[2]), n, elems, P(o[0]), P(o[1])), [d, [d.min()]], [PARZEN_RTOL * d.max()] * 2)
    assert mn.item() == dist.min().item()


# ---- the module-level sampler operations and the copies ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 22, 257])
def test_rank_scores(ctx, n):
    from test_gpu_sampler import ref_order, planted_scores
    lib, h = ctx.lib, ctx.h
    s = planted_scores(n, 100 + n)                                             # exact ties, -0.0, NaN and infinities
    nscr = max(1, (lib.fg_rank_scores_workspace_bytes(n) + 3) // 4)
    P = lambda t: t.data_ptr()
    for ascending in (0, 1):
        (order,) = check_simple(ctx, "fg_rank_scores n = %d" % n, [s], [n],
                                lambda i, o, sc: lib.fg_rank_scores(h, P(i[0]), n, ascending, P(o[0]), P(sc[0]), lib.fg_rank_scores_workspace_bytes(n)),
                                [None], [0], scratch=[nscr])
        assert np.array_equal(order.view(torch.int32).cpu().numpy(), ref_order(s, bool(ascending)))


@pytest.mark.parametrize("case", [(12, 3, 8, 8, 10, 4, 2, True, 1), (12, 1, 8, 6, 7, 3, 0, False, 0), (12, 3, 5, 7, 11, 16, 3, True, 1)])
def test_image_grid(ctx, case):
    from test_gpu_sampler import ref_grid
    lib, h = ctx.lib, ctx.h
    n, c, hh, ww, k, nrow, padding, with_order, normalize = case
    rng = np.random.default_rng(7 + n + k + padding)
    imgs = rng.normal(0.3, 1.0, (n, hh, ww, c)).astype(np.float32)
    order = rng.permutation(n).astype(np.int32)
    want, want_mm = ref_grid(imgs, order if with_order else None, k, nrow, padding, normalize)
    P = lambda t: t.data_ptr()
    grid, mm = check_simple(ctx, "fg_image_grid %s" % (case,), [imgs, order], [want.size, 2],
                            lambda i, o, s: lib.fg_image_grid(h, P(i[0]), P(i[1]) if with_order else None, k, c, hh, ww, nrow, padding, normalize, P(o[0]), P(o[1])),
                            [None, want_mm], [0, 0])
    got = grid.cpu().numpy().reshape(want.shape)
    if normalize:                                                              # the bar of tests/test_gpu_sampler.py: one ulp of the normalised value
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    else:
        assert np.array_equal(got, want)


def test_d2d(ctx):
    lib, h = ctx.lib, ctx.h
    x = np.random.default_rng(29).standard_normal(1003).astype(np.float32)
    check_simple(ctx, "fg_d2d", [x], [1003], lambda i, o, s: lib.fg_d2d(h, o[0].data_ptr(), i[0].data_ptr(), 1003 * 4), [x], [0])
