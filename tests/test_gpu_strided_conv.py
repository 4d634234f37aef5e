"""Stride-2 convolutions at operator level: a one-layer net [FG_CONV a=cin b=cout c=k d=(k-1)/2 p=2] -- the only public way to a
strided convolution, fg_conv2d_* has no stride -- forward, input gradient, weight gradient and bias gradient against
oracle.torch7_nn.SpatialConvolution(dw=2, dh=2) evaluated in float64 (weights, activations and accumulated gradients all double).
Bars: gpu_util.BAR["conv_fwd" | "conv_dgrad" | "conv_wgrad" | "conv_bgrad"] x max(1, max|reference|), as
tests/test_gpu_dispatch_paths.py holds its PATH_CASES.

STRIDED_CASES is module-level data: tests/dispatch_audit.py replays it in the planning-only context and
tests/test_dispatch_coverage_host.py asserts that every signature the strided sweep reaches is run by one of these cases.

The stride-2 data gradient is the stride-1 data gradient of the zero-inserted output gradient, which zero_insert2_kernel writes into
the net's workspace.  Its launch is capped at 4096 blocks of 256 threads of one float4: the CAP case has 4 718 592 floats there,
12.5 % above the cap.  It runs with every vector of the net in the guarded arena of tests/mem_contract.py and the workspace NaN before
the forward pass, so a tail the kernel does not write reads as NaN (or as a partial sum the forward pass left), never as the zeros a
fresh allocation may hold."""
import functools

import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import close, BAR

pytestmark = pytest.mark.gpu

# (B, H, W, cin, cout, k)
CAP_CASE = (9, 64, 64, 8, 128, 3)
STRIDED_CASES = [
    (2, 2, 2, 8, 16, 3),            # a 1x1 output
    (3, 6, 10, 6, 10, 3),           # odd 3x5 output, ragged channels on both sides, Cout % 4 == 2: zero_insert2_scalar_kernel
    (2, 8, 8, 3, 64, 5),            # a pair that is "thin" at stride 1
    (2, 8, 8, 64, 3, 3),            # Cout = 3
    (2, 12, 4, 16, 32, 7),          # k = 7: 49 tap groups
    (5, 16, 16, 128, 128, 3),       # the 16-px discriminators' own layer at an odd batch
    CAP_CASE,                       # zero-inserted gradient of 1 179 648 quads against the cap of 1 048 576
    # ---- from the strided sweep of tests/dispatch_audit.py: signatures the cases above do not reach
    (2, 10, 2, 5, 2, 3),            # bwd: colsum_small_kernel<2> (bias gradient of 2 outputs)
    (19, 6, 30, 1, 1, 5),           # bwd: colsum_small_kernel<1>, 1 -> 1
    (30, 24, 14, 1, 4, 5),          # bwd: colsum_small_kernel<4>
    (5, 12, 26, 1, 20, 3),          # bwd: colsum_final_kernel at 20 outputs
    (48, 32, 32, 128, 2, 3),        # bwd: igemm_kernel, lds 55808 (data gradient over 2 zero-padded channels)
    (24, 32, 32, 320, 5, 3),        # bwd: igemm_kernel, lds 74240; Cout = 5: the scalar zero insert over 122 880 floats
    (18, 64, 64, 2, 15, 3),         # Cout = 15: the scalar zero insert above its cap (1 105 920 elements against 1 048 576)
    (4, 32, 32, 128, 256, 3),       # math 6, bwd: wgrad_ws6_kernel lds 116736 + wgrad_finish_kernel at block 128
    (8, 32, 32, 4, 16, 7),          # math 6, bwd: igemm_ws6_kernel lds 108544
]
# every case but the CAP case also runs in math 6 (fp32 emulated on the bf16 matrix pipe: other contraction kernels), at the same bars
RUNS = [(c, m) for c in STRIDED_CASES if c != CAP_CASE for m in (0, 6)]


def case_id(c):
    return "x".join(str(v) for v in c)


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math = c.get_math()
    yield c
    c.set_math(math)


@functools.lru_cache(maxsize=2)
def operands_and_reference(case):
    """(float32 NCHW operands, float64 references): x, gy, weight, bias; y, gx, gw, gb"""
    B, H, W, cin, cout, k = case
    rng = np.random.default_rng(B * 1000 + H * 100 + W * 10 + cin + cout + k)
    m = O.SpatialConvolution(cin, cout, k, k, 2, 2, (k - 1) // 2, rng=rng)
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    gy = rng.standard_normal((B, cout, H // 2, W // 2)).astype(np.float32)
    w32, b32 = m.weight.copy(), m.bias.copy()
    m.weight, m.bias = w32.astype(np.float64), b32.astype(np.float64)
    m.gradWeight, m.gradBias = np.zeros_like(m.weight), np.zeros_like(m.bias)
    x64, gy64 = x.astype(np.float64), gy.astype(np.float64)
    y = m.updateOutput(x64).copy()
    gx = m.updateGradInput(x64, gy64).copy()
    m.accGradParameters(x64, gy64)
    assert y.dtype == gx.dtype == m.gradWeight.dtype == m.gradBias.dtype == np.float64
    return (x, gy, w32, b32), dict(fwd=y, dgrad=gx, wgrad=m.gradWeight.copy(), bgrad=m.gradBias.copy())


def run_layer(ctx, case, guarded=False):
    """-> the four results of the library (NCHW numpy) for the case's operands"""
    from face_generator_amd.runtime import DeviceNet
    from gpu_util import nhwc, nchw
    B, H, W, cin, cout, k = case
    (x, gy, w, b), _ = operands_and_reference(case)
    dn = DeviceNet(ctx, [("CONV", cin, cout, k, (k - 1) // 2, 2)], (cin, H, W), B)
    assert (dn.out_c, dn.out_h, dn.out_w) == (cout, H // 2, W // 2) and dn.n_params == w.size + b.size
    xd, gyd = nhwc(x, ctx.device), nhwc(gy, ctx.device)
    ar = None
    if guarded:
        from mem_contract import Arena
        from test_gpu_memory_contract_nets import net_sizes, rehouse
        ar = Arena.sized(ctx.device, net_sizes(dn) + [xd.numel()])
        rehouse(ctx, ar, dn, "strided")
        gx = ar.take(xd.numel(), name="gx")
        gx.fill_(float("nan"))
        dn.ws.fill_(float("nan"))
    dn.params.copy_(torch.from_numpy(np.concatenate([w.reshape(-1), b.reshape(-1)])))
    dn.params_changed()
    dn.grads.zero_()
    y = nchw(dn.forward(xd).clone().view(B, H // 2, W // 2, cout))       # (a 1x1 map comes back as [B][C])
    if guarded:
        dn._drain(dn._backward_call(gyd, True, gx), lambda: ctx.lib.fg_net_backward_resume(dn.h))
        torch.cuda.synchronize()
        ar.assert_guards("strided %s" % case_id(case))
        gx = gx.view(xd.shape)
    else:
        gx = dn.backward(gyd, param_grads=True, input_grad=True)
    g = dn.grads.cpu().numpy()
    return dict(fwd=y, dgrad=nchw(gx), wgrad=g[:w.size].reshape(w.shape), bgrad=g[w.size:])


def check(case, got, ref, passes=("fwd", "dgrad", "wgrad", "bgrad"), tag=""):
    worst = []
    for p in passes:
        r, g = ref[p], got[p].astype(np.float64)
        scale = max(1.0, float(np.abs(r).max()))
        worst.append("%s %.2e of %.1e" % (p, float(np.nanmax(np.abs(g - r))) / scale, BAR["conv_" + p]))
    print("strided %s%s: max|err| / max(1, max|ref|): %s" % (case_id(case), tag, "; ".join(worst)))
    for p in passes:
        r = ref[p]
        assert not np.isnan(got[p]).any(), "strided %s%s %s: %d NaN, first at %s" % (
            case_id(case), tag, p, int(np.isnan(got[p]).sum()), np.argwhere(np.isnan(got[p]))[0])
        close(got[p], r, atol=BAR["conv_" + p] * max(1.0, float(np.abs(r).max())), what="strided %s%s %s" % (case_id(case), tag, p))


@pytest.mark.parametrize("case,math", RUNS, ids=["%s-math%d" % (case_id(c), m) for c, m in RUNS])
def test_strided_conv_matches_float64(ctx, case, math):
    _, ref = operands_and_reference(case)
    ctx.set_math(math)
    try:
        got = run_layer(ctx, case)
    finally:
        ctx.set_math(0)
    check(case, got, ref, tag=" math %d" % math)


def test_strided_conv_above_the_zero_insert_grid_cap(ctx):
    """B * H * W * Cout = 4 718 592 > 4096 blocks x 256 threads x 4 floats.  The input gradient of the samples whose zero-inserted
    gradient lies below the cap (the first eight) is compared first and apart, so that a failure says which part is wrong."""
    case = CAP_CASE
    B, H, W, cin, cout, k = case
    assert B * H * W * cout > 4096 * 256 * 4 and (B - 1) * H * W * cout <= 4096 * 256 * 4
    _, ref = operands_and_reference(case)
    got = run_layer(ctx, case, guarded=True)
    head = {p: (v[:B - 1] if p == "dgrad" else v) for p, v in got.items()}
    rhead = {p: (v[:B - 1] if p == "dgrad" else v) for p, v in ref.items()}
    check(case, head, rhead, passes=("dgrad",), tag=" samples 0..%d" % (B - 2))
    check(case, got, ref)
