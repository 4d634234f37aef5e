"""Every stage fusion of fg_net on small nets off the models' shapes: NET_CASES of tests/net_cases.py, each against the float64 oracle
of the same layer list, parameters, inputs and masks (tests/NET_FUSIONS.md has the table of decisions and case names).

Per case: train forward -- the net output and every stage output fg_net_layer_output exposes, layer by layer, so that a wrong fused
stage is named; the BatchNorm running statistics after that pass; backward with FG_BWD_PARAM_GRADS | FG_BWD_INPUT_GRAD against the
oracle's backward on the device's PReLU / max-pool decisions (adopted decisions that differ from the oracle's own: at most max(1,
1e-5 of the units)); the same backward with the two flags in two calls, bit for bit; fg_net_backward_range split at every stage
boundary (a PReLU at a boundary leaves its neighbour's epilogue: held to the oracle, not to the unsplit run); evaluate forward, layer
by layer.  Bars: gpu_util.assert_net_bars, the project's net-level bars.  A case with a fused and an un-fused fusion word is two
cases, each held to the oracle.  Every case runs with every vector of the net in the arena of tests/mem_contract.py and a NaN
workspace of exactly fg_net_workspace_bytes; for the cases marked `guarded` the scratch slices their stages borrow are the point."""
import numpy as np
import pytest
import torch

import net_cases as NC
from gpu_util import close, dev, assert_net_bars, BAR

pytestmark = pytest.mark.gpu

# cases that take the fallback bar of NET_FUSIONS.md ("Measured bars"): {case name: factor x the float32 oracle's own error}.  Empty:
# every case meets the project's bars.
FALLBACK = {}


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math, fusion = c.get_math(), c.get_fusion()
    yield c
    c.set_math(math); c.set_fusion(fusion)


def layer_outputs(dn, case, outs, B):
    """{layer index: oracle-shaped float32 array} for every layer whose output the plan exposes"""
    res = {}
    for i, l in enumerate(case.layers):
        if l[0] in NC.MARKERS:
            continue
        t = NC.exposed(dn, i)
        if t is not None:
            res[i] = NC.from_device(t.cpu().numpy().reshape(B, -1), outs[i])
    # the last layer always ends a stage: an entry that refused every layer would otherwise leave nothing to compare
    assert len(case.layers) - 1 in res and len(res) >= 1, "%s: fg_net_layer_output exposes %s" % (case.name, sorted(res))
    return res


def compare_layers(what, got, mods):
    worst = (-1.0, None)
    for i, a in sorted(got.items()):
        ref = mods[i].output
        assert np.isfinite(a).all(), "%s: output of layer %d (%s): %d values are not finite" % (what, i, type(mods[i]).__name__, int((~np.isfinite(a)).sum()))
        e = float(np.abs(a - ref.reshape(a.shape)).max())
        worst = (e, i) if e > worst[0] else worst
        close(a, ref.reshape(a.shape), atol=1e-5, what="%s: output of layer %d (%s)" % (what, i, type(mods[i]).__name__))
    print("%s: %d layer outputs compared, worst %.3e at layer %s (bar 1e-5)" % (what, len(got), worst[0], worst[1]))


@pytest.mark.parametrize("case", NC.NET_CASES, ids=[c.name for c in NC.NET_CASES])
def test_net_case_against_the_float64_oracle(ctx, case):
    from oracle import torch7_nn as O
    lib, d, B = ctx.lib, ctx.device, case.batch
    ctx.set_math(case.math); ctx.set_fusion(case.fusion)         # the fusion bits are read when a net is created
    try:
        net, mods, P, G, x, gy, masks = NC.operands(case, np.float64)
        first, outs = NC.walk(case.layers, case.dims)
        dn = NC.device_net(ctx, case.layers, case.dims, B)
        assert dn.n_params == P.size and dn.n_masks == len(masks)
        xd = dev(NC.to_device(x, first), d)
        gyd = dev(NC.to_device(gy, outs[-1]), d)
        md = [dev(m, d) for m in NC.device_masks(case.layers, case.dims, masks)]
        dn.params.copy_(torch.from_numpy(P.astype(np.float32)))
        bns = [m for m in mods if isinstance(m, O.SpatialBatchNormalization)]
        if bns:                       # the running statistics the oracle starts from
            dn.buffers.copy_(torch.from_numpy(np.concatenate([np.concatenate([m.running_mean, m.running_var]) for m in bns]).astype(np.float32)))
        # every case runs in the guarded arena (an overrun of any stage lands inside the allocation and is reported); `guarded` in
        # NET_CASES marks the ones whose borrowed scratch slices are the reason they exist
        from mem_contract import Arena
        from test_gpu_memory_contract_nets import net_sizes, rehouse
        ar = Arena.sized(ctx.device, net_sizes(dn) + [xd.numel()])
        rehouse(ctx, ar, dn, case.name)
        gx = ar.take(xd.numel(), name="gx")
        dn.ws.fill_(float("nan"))
        dn.params_changed()
        P32 = P.astype(np.float32)

        # ---- forward (train) ------------------------------------------------------------------------------------------------
        y = dn.forward(xd, masks=md or None, train=True)
        yh = NC.from_device(y.cpu().numpy().reshape(B, -1), outs[-1])
        got = layer_outputs(dn, case, outs, B)
        buffers = dn.buffers.clone()
        NC.adopt(ctx, dn, case.layers, case.dims, mods, x, P32)
        out, gin = NC.oracle_pass(net, G, x, gy, masks)
        flips, units = NC.flips(net)
        NC.adopt(ctx, dn, case.layers, case.dims, mods, x, P32, clear=True)
        compare_layers(case.name + " train", got, mods)
        assert flips <= max(1, 1e-5 * units), "%d of %d PReLU decisions adopted from the device differ from the oracle's" % (flips, units)
        off = 0
        for m in bns:                 # running statistics after ONE train forward
            rm, rv = buffers[off:off + m.nf].cpu().numpy(), buffers[off + m.nf:off + 2 * m.nf].cpu().numpy()
            close(rm, m.running_mean, atol=BAR["bn_running_mean"], what=case.name + " running_mean")
            close(rv, m.running_var, atol=0.0, rtol=BAR["bn_running_var_rtol"], what=case.name + " running_var")
            off += 2 * m.nf

        # ---- backward, both flags ---------------------------------------------------------------------------------------------
        resume = lambda: lib.fg_net_backward_resume(dn.h)
        ns = lib.fg_net_num_stages(dn.h)

        def backward(flags, a=None, b=0):
            gxa = gx if flags & 2 else None
            dn._drain(dn._backward_call(gyd, bool(flags & 1), gxa, a, b), resume)

        dn.grads.fill_(float("nan")); gx.fill_(float("nan"))
        backward(3)
        g3, gx3 = dn.grads.clone(), gx.clone()
        gxh = NC.from_device(gx3.cpu().numpy().reshape(B, -1), first)
        e32 = None
        if case.name in FALLBACK:
            e32 = NC.reference_errors(case)
        _bars(case, net, yh, out, gxh, gin, g3.cpu().numpy(), e32)
        # ---- the two flags in two calls: the same bits ------------------------------------------------------------------------
        dn.grads.fill_(float("nan")); gx.fill_(float("nan"))
        backward(1)
        assert torch.equal(dn.grads.view(torch.int32), g3.view(torch.int32)), "%s: FG_BWD_PARAM_GRADS alone gives other gradients" % case.name
        assert bool(torch.isnan(gx).all()), "%s: FG_BWD_PARAM_GRADS alone wrote the input gradient" % case.name
        dn.grads.fill_(float("nan"))
        backward(2)
        assert torch.equal(gx.view(torch.int32), gx3.view(torch.int32)), "%s: FG_BWD_INPUT_GRAD alone gives another input gradient" % case.name
        assert bool(torch.isnan(dn.grads).all()), "%s: FG_BWD_INPUT_GRAD alone wrote parameter gradients" % case.name
        # ---- fg_net_backward_range split at every stage boundary --------------------------------------------------------------
        for s in range(1, ns):
            dn.grads.fill_(float("nan")); gx.fill_(float("nan"))
            backward(3, ns - 1, s)
            backward(3, s - 1, 0)
            _bars(case, net, yh, out, NC.from_device(gx.cpu().numpy().reshape(B, -1), first), gin, dn.grads.cpu().numpy(), e32,
                  what="%s split at stage %d" % (case.name, s), quiet=True)

        # ---- forward (evaluate): the running statistics of the train pass -----------------------------------------------------
        net.evaluate()
        oute = net.forward(x.astype(np.float64))
        ye = dn.forward(xd, train=False)
        gote = layer_outputs(dn, case, outs, B)
        assert bool(torch.isfinite(ye).all()), "%s: evaluate outputs are not finite" % case.name
        close(NC.from_device(ye.cpu().numpy().reshape(B, -1), outs[-1]), oute, atol=1e-5, what=case.name + " evaluate outputs")
        compare_layers(case.name + " evaluate", gote, mods)
        assert torch.equal(dn.buffers, buffers), "%s: an evaluate forward moved the running statistics" % case.name
        torch.cuda.synchronize()
        ar.assert_guards(case.name)
    finally:
        ctx.set_math(0); ctx.set_fusion(503)


def _bars(case, net, yh, out, gxh, gin, got, e32, what=None, quiet=False):
    what = what or case.name
    for name, v in (("outputs", yh), ("input gradient", gxh), ("parameter gradients", got)):       # (NaN compares as equal to nothing)
        assert np.isfinite(v).all(), "%s: %d of %d %s are not finite, first at %s" % (what, int((~np.isfinite(v)).sum()), v.size, name, np.argwhere(~np.isfinite(v))[0])
    if e32 is None:
        if quiet:
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                return assert_net_bars(what, net, yh, out, gxh, gin, got)
        return assert_net_bars(what, net, yh, out, gxh, gin, got)
    # the fallback bar of tests/NET_FUSIONS.md: the project's bar or FALLBACK[case] x the float32 oracle's own error, whichever is larger
    f = FALLBACK[case.name]
    close(yh, out, atol=max(1e-5, f * e32["outputs"]), what=what + " outputs")
    close(gxh, gin, atol=max(1e-4 * np.abs(gin).max() + 1e-7, f * e32["input_gradient"]), what=what + " input gradient")
    gmax = max([float(np.abs(getattr(m, gn)).max()) for (m, pn, gn) in net.parameters()] + [0.0])
    from oracle import torch7_nn as O
    for (m, pn, o, e) in NC.tensor_errors(net, got):
        r = getattr(m, "gradWeight" if pn == "weight" else "gradBias")
        tol = 1e-4 * np.abs(r).max() + 1e-7 + (32 * 6e-8 * getattr(m, "gw_cond", 0.0) if isinstance(m, O.PReLU) else 0.0)
        tol = max(tol, 2e-6 * gmax, f * e32["tensors"][o])
        assert e <= tol, "%s %s.%s @%d: err %.3e tol %.3e" % (what, type(m).__name__, pn, o, e, tol)
