"""The memory contract (tests/mem_contract.py) at the net, step and sampler level of include/facegen_hip.h: parameters, gradients,
BatchNorm buffers and every workspace live in one guarded arena, the workspaces are exactly fg_net_workspace_bytes /
fg_gan_workspace_bytes / fg_sampler_workspace_bytes long and poisoned (NaN, 0, 1e30) before every forward / before the step or sampler
object is created -- not between a forward and its backward: saved statistics, masks and parked partials legitimately live there.
Outputs, gradients, updated parameters, losses and rankings must be bit-identical across the fills and free of NaN, the inputs and
every guard untouched.  Nets sized for max_batch run at smaller batches too (the sampler's tail, a short last batch).  What the nets
compute is checked against the oracle elsewhere (tests/test_gpu_net.py, test_gpu_branched.py, test_gpu_c2f.py, test_gpu_sampler.py)."""
import ctypes

import pytest
import torch

from mem_contract import Arena, FILLS, TAIL_FILLS, PATTERN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def P(t):
    return t.data_ptr() if t is not None else None


def bits(t):
    return t.contiguous().view(torch.int32)


def build_pair(ctx, kind, max_batch, seed=5):
    """-> (dnG, dnD, S, C): the device plans of a generator / discriminator pair with seeded non-trivial weights"""
    from face_generator_amd import models, models_c2f, nn_utils
    gen = torch.Generator().manual_seed(seed)
    if kind == "c2f16":
        G, D = models_c2f.create_G((3, 16, 16), gen=gen), models_c2f.create_D((3, 16, 16), gen=gen)
    else:
        s = 16 if kind == "px16" else 32                   # px16: create_D16_d, an nn.ConcatTable discriminator compiled to one plan
        G, D = models.create_G((3, s, s), 100, gen=gen), models.create_D((3, s, s))
        nn_utils.initializeWeights(D, 0.05, 0.01, gen=gen)
    G.cuda(ctx, max_batch=max_batch); D.cuda(ctx, max_batch=max_batch)
    dnG, dnD = G._inner().device_net, D._inner().device_net
    return dnG, dnD, dnD.in_h, dnD.in_c


def net_sizes(dn):
    return [dn.n_params, dn.n_params, max(dn.n_buffers, 1), dn.ws.numel()]


def rehouse(ctx, ar, dn, name):
    """moves a DeviceNet's vectors and its workspace into the arena (exact sizes, 256-byte aligned) and re-binds them"""
    params, grads = ar.take(dn.n_params, name=name + ".params"), ar.take(dn.n_params, name=name + ".grads")
    buffers = ar.take(max(dn.n_buffers, 1), name=name + ".buffers")
    ws = ar.take(dn.ws.numel(), name=name + ".workspace")
    assert dn.ws.numel() * 4 - ctx.lib.fg_net_workspace_bytes(dn.h, dn.max_batch) in (0, 1, 2, 3)
    params.copy_(dn.params); grads.zero_(); buffers.copy_(dn.buffers)
    dn.params, dn.grads, dn.buffers, dn.ws = params, grads, buffers, ws
    ctx.check(ctx.lib.fg_net_bind(dn.h, P(params), P(grads), P(buffers)))
    dn.params_changed()
    return params.clone(), buffers.clone()


def compare(first, res, what):
    for key in first:
        a, b = first[key], res[key]
        assert not bool(torch.isnan(b).any()) if b.dtype == torch.float32 else True, "%s: NaN in %s" % (what, key)
        if not torch.equal(bits(a), bits(b)):
            d = torch.nonzero(bits(a).reshape(-1) != bits(b).reshape(-1)).reshape(-1)
            raise AssertionError("%s: %s depends on what the workspaces / outputs held before: %d of %d elements differ, first at %d"
                                 % (what, key, d.numel(), a.numel(), int(d[0])))


# ---- fg_net_forward / fg_net_backward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", ["default", 0])
@pytest.mark.parametrize("kind", ["px32", "px16", "c2f16"])
def test_net_forward_backward(ctx, kind, fusion):
    lib, MAXB = ctx.lib, 8
    prev = ctx.get_fusion()
    try:
        if fusion == 0:
            ctx.set_fusion(0)                              # read when a net is created (its packs) and per call
        dnG, dnD, S, C = build_pair(ctx, kind, MAXB)
        for which, dn in (("G", dnG), ("D", dnD)):
            in_shape = (dn.in_h, dn.in_w, dn.in_c) if dn.in_h * dn.in_w > 1 else (dn.in_c,)
            n_in = dn.in_c * dn.in_h * dn.in_w
            n_out = dn.out_c * dn.out_h * dn.out_w
            msizes = [lib.fg_net_mask_elems(dn.h, i, MAXB) for i in range(dn.n_masks)]
            ar = Arena.sized(ctx.device, net_sizes(dn) + 2 * ([MAXB * n_in] * 2 + [MAXB * n_out] + msizes))       # operands of both batches
            p0, b0 = rehouse(ctx, ar, dn, which)
            for b in (MAXB, 3):
                what = "%s %s, fusion %s, batch %d of max_batch %d" % (kind, which, fusion, b, MAXB)
                x = ar.put(ctx.uniform((b,) + in_shape, -1.0 if which == "G" else 0.0, 1.0, seed=11 + b), name=which + ".x")
                gy = ar.put(ctx.normal((b, n_out), 0.0, 1.0, seed=12 + b), name=which + ".gy")
                gx = ar.take(b * n_in, name=which + ".gx")
                masks = [ar.put(ctx.bernoulli((lib.fg_net_mask_elems(dn.h, i, b),), lib.fg_net_mask_keep(dn.h, i), seed=20 + i), name="%s.mask%d" % (which, i))
                         for i in range(dn.n_masks)]
                ins = [x, gy, dn.params] + masks
                snap = [bits(v).clone() for v in ins]
                first = None
                for i, fill in enumerate(FILLS):
                    tag = "%s [prefill %r]" % (what, fill)
                    dn.buffers.copy_(b0)                   # the running statistics are in-out
                    for v in (dn.ws, dn.grads, gx):
                        v.fill_(fill)
                    for v in ins:
                        ar.fill_tail(v, TAIL_FILLS[i])
                    ye = dn.forward(x.view((b,) + in_shape), train=False).clone()
                    dn.ws.fill_(fill)
                    y = dn.forward(x.view((b,) + in_shape), masks=masks or None, train=True).clone()
                    dn._drain(dn._backward_call(gy.view(y.shape), True, gx), lambda: lib.fg_net_backward_resume(dn.h))   # FG_BWD_PARAM_GRADS | _INPUT_GRAD
                    torch.cuda.synchronize()
                    ar.assert_guards(tag)
                    for k, (v, s0) in enumerate(zip(ins, snap)):
                        assert torch.equal(bits(v), s0), "%s: input %d was written" % (tag, k)
                    res = dict(evaluate_output=ye, output=y, grads=dn.grads.clone(), gx=gx.clone(), buffers=dn.buffers.clone())
                    first = first or res
                    compare(first, res, tag)
                for v in ins:
                    ar.fill_tail(v, PATTERN)
    finally:
        ctx.set_fusion(prev)


def test_net_forward_to_an_output_on_16_bytes(ctx):
    """fg_net_forward_to: the last stage writes `out` ("device, NHWC, 16-byte aligned") instead of the workspace -- same bits as
    fg_net_forward leaves in the workspace, at a batch below max_batch, with `out` on exactly 16 bytes"""
    lib, MAXB, b = ctx.lib, 8, 3
    dnG, _, S, C = build_pair(ctx, "px32", MAXB)
    n_out = dnG.out_c * dnG.out_h * dnG.out_w
    ar = Arena.sized(ctx.device, net_sizes(dnG) + [b * 100, b * n_out])
    rehouse(ctx, ar, dnG, "G")
    x = ar.put(ctx.uniform((b, 100), -1.0, 1.0, seed=14), name="x")
    out = ar.take(b * n_out, align=16, name="out")
    ins = [x, dnG.params, dnG.buffers]
    snap = [bits(v).clone() for v in ins]
    first = None
    for i, fill in enumerate(FILLS):
        tag = "fg_net_forward_to [prefill %r]" % fill
        for v in ins:
            ar.fill_tail(v, TAIL_FILLS[i])
        dnG.ws.fill_(fill)
        want = dnG.forward(x, train=False).clone()
        dnG.ws.fill_(fill); out.fill_(fill)
        off = ctypes.c_longlong()
        ctx.check(lib.fg_net_forward_to(dnG.h, b, P(x), P(dnG.ws), dnG.ws.numel() * 4, 0, None, 0, ctypes.byref(off), P(out)))
        torch.cuda.synchronize()
        ar.assert_guards(tag)
        for k, (v, s0) in enumerate(zip(ins, snap)):
            assert torch.equal(bits(v), s0), "%s: input %d was written" % (tag, k)
        assert torch.equal(bits(out), bits(want.reshape(-1))), tag + ": differs from fg_net_forward"
        res = dict(out=out.clone())
        first = first or res
        compare(first, res, tag)


# ---- fg_gan_* ---------------------------------------------------------------------------------------------------------------------
BUF = dict(D_INPUT=0, LOSS=3, CONFUSION=4, D_OUTPUT=7)


@pytest.mark.parametrize("kind,B", [("px32", 8), ("c2f16", 4)])
def test_gan_steps(ctx, kind, B):
    lib = ctx.lib
    table = 1 if kind == "c2f16" else 0
    dnG, dnD, S, C = build_pair(ctx, kind, B)
    nstep = (lib.fg_gan_workspace_bytes(dnG.h, dnD.h, table, B) + 3) // 4
    img = B * S * S * C
    ar = Arena.sized(ctx.device, net_sizes(dnG) + net_sizes(dnD) + [nstep] + [img] * 4)
    pG0, bG0 = rehouse(ctx, ar, dnG, "G")
    pD0, bD0 = rehouse(ctx, ar, dnD, "D")
    step = ar.take(nstep, name="step workspace")
    real = ar.put(ctx.uniform((B // 2, S, S, C), 0.0, 1.0, seed=9), name="real")
    conds = [ar.put(ctx.uniform((n, S, S, C), 0.0, 1.0, seed=30 + i), name="cond%d" % i) for i, n in enumerate((B // 2, B // 2, B))] if table else [None] * 3
    ins = [real] + [c for c in conds if c is not None]
    snap = [bits(v).clone() for v in ins]
    first = None
    for i, fill in enumerate(FILLS[:2]):
        tag = "fg_gan %s B = %d [prefill %r]" % (kind, B, fill)
        for dn, p0, b0 in ((dnG, pG0, bG0), (dnD, pD0, bD0)):
            dn.params.copy_(p0); dn.buffers.copy_(b0); dn.params_changed()
            dn.grads.fill_(fill); dn.ws.fill_(fill)
        step.fill_(fill)
        for v in ins:
            ar.fill_tail(v, TAIL_FILLS[i])
        h = ctypes.c_void_p()
        ctx.check(lib.fg_gan_create(ctx.h, dnG.h, dnD.h, table, B, P(step), nstep * 4, ctypes.byref(h)))
        try:
            ctx.check(lib.fg_gan_bind_workspaces(h, P(dnG.ws), dnG.ws.numel() * 4, P(dnD.ws), dnD.ws.numel() * 4))
            ctx.check(lib.fg_gan_set_seeds(h, 3, 0, 777, 0))
            view = lambda what: _gan_view(ctx, h, what, step, dnD)
            ctx.check(lib.fg_step_D(h, B, P(real), P(conds[0]), P(conds[1]), None, None, 0))
            res = dict(d_out=view("D_OUTPUT")[:B].clone(), d_loss=view("LOSS").clone(), confusion=view("CONFUSION").clone())
            ctx.check(lib.fg_step_G(h, B, P(conds[2]), None, None, 0))
            ctx.check(lib.fg_gan_finish_pending(h))
            torch.cuda.synchronize()
            res.update(g_out=view("D_OUTPUT")[:B].clone(), loss=view("LOSS").clone(), samples=view("D_INPUT")[:img].clone(),
                       pG=dnG.params.clone(), pD=dnD.params.clone(), bnG=dnG.buffers.clone(), bnD=dnD.buffers.clone())
        finally:
            lib.fg_gan_destroy(h)
        ar.assert_guards(tag)
        for k, (v, s0) in enumerate(zip(ins, snap)):
            assert torch.equal(bits(v), s0), "%s: input %d was written" % (tag, k)
        assert not torch.equal(res["pG"], pG0) and not torch.equal(res["pD"], pD0), "the steps updated nothing"
        first = first or res
        compare(first, res, tag)


def _gan_view(ctx, h, what, step, dnD):
    off, cnt = ctypes.c_longlong(), ctypes.c_longlong()
    ctx.check(ctx.lib.fg_gan_buffer(h, BUF[what], ctypes.byref(off), ctypes.byref(cnt)))
    base = dnD.ws if what == "D_OUTPUT" else step           # D's probabilities live in D's own workspace
    return base[off.value: off.value + cnt.value]


# ---- fg_sampler_* -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [8, 6])                   # 22 = 2 x 8 + 6 (chunk % 4 == 0), 3 x 6 + 4 (the copy path of fg_sample_score)
def test_sampler(ctx, chunk):
    lib, N = ctx.lib, 22
    dnG, dnD, S, C = build_pair(ctx, "px32", chunk)
    nsm = (lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, N) + 3) // 4
    ar = Arena.sized(ctx.device, net_sizes(dnG) + net_sizes(dnD) + [nsm, N * 100])
    pG0, bG0 = rehouse(ctx, ar, dnG, "G")
    pD0, bD0 = rehouse(ctx, ar, dnD, "D")
    ws = ar.take(nsm, name="sampler workspace")
    noise = ar.put(ctx.uniform((N, 100), -1.0, 1.0, seed=41), align=16, name="noise")     # "device [n][noiseDim] (16-byte aligned)"
    ins = [noise, dnG.params, dnD.params, dnG.buffers, dnD.buffers]
    snap = [bits(v).clone() for v in ins]
    first = None
    for i, fill in enumerate(FILLS):
        tag = "fg_sampler chunk %d [prefill %r]" % (chunk, fill)
        for v in (ws, dnG.ws, dnD.ws):
            v.fill_(fill)
        for v in ins:
            ar.fill_tail(v, TAIL_FILLS[i])
        h = ctypes.c_void_p()
        ctx.check(lib.fg_sampler_create(ctx.h, dnG.h, dnD.h, N, chunk, P(ws), nsm * 4, ctypes.byref(h)))
        try:
            ctx.check(lib.fg_sampler_bind_workspaces(h, P(dnG.ws), dnG.ws.numel() * 4, P(dnD.ws), dnD.ws.numel() * 4))
            ctx.check(lib.fg_sampler_set_seed(h, 11, 0))
            res = {}
            for run, nz in (("drawn noise", None), ("caller's noise", noise)):
                ctx.check(lib.fg_sample(h, N, P(nz)))
                torch.cuda.synchronize()
                for what, idx in (("NOISE", 0), ("IMAGES", 1), ("PREDS", 2), ("ORDER_DESC", 3), ("ORDER_ASC", 4)):
                    off, cnt = ctypes.c_longlong(), ctypes.c_longlong()
                    ctx.check(lib.fg_sampler_buffer(h, idx, ctypes.byref(off), ctypes.byref(cnt)))
                    if what != "NOISE" or nz is None:
                        t = ws[off.value: off.value + cnt.value].clone()
                        res["%s, %s" % (what, run)] = t.view(torch.int32) if what.startswith("ORDER") else t
        finally:
            lib.fg_sampler_destroy(h)
        ar.assert_guards(tag)
        for k, (v, s0) in enumerate(zip(ins, snap)):
            assert torch.equal(bits(v), s0), "%s: input %d (noise, parameters, running statistics) was written" % (tag, k)
        for key in ("ORDER_DESC, drawn noise", "ORDER_ASC, caller's noise"):
            assert sorted(res[key].tolist()) == list(range(N)), key
        first = first or res
        compare(first, res, tag)
