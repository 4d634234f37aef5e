"""The sync-BN walk of fg_net on small nets: SYNC_CASES of tests/sync_cases.py, R DeviceNets in one process driven in lock-step, the
"all-reduce" a float64 sum of their exchange buffers at every pause, against the float64 oracle of the same layer list on the GLOBAL
batch (tests/SYNC_BN.md has the table of cases and properties).

Per case: train forward -- the replicas' outputs and every exposed layer output concatenated in shard order, on the devices' PReLU /
pool decisions; the running statistics, bit-equal across the replicas and against the oracle's global-batch ones; backward with
flags 3 (the float64 sum of the replicas' flat gradients and the concatenated input gradient against the oracle's), flags 1 and 2
bit for bit, fg_net_backward_range split at every stage boundary with each half driven through its own pauses; the pause protocol
(one pause per BatchNorm, every replica at the same point, fg_net_sync_count = 2 C + 1, slot [2 C] = the replica's own rows); the
buffer discipline (NaN before every pass: [0, count) finite at a pause, nothing past the count written, no NaN in any output);
two replicas on the same shard bit-equal to one; evaluate with sync on; the redirected output of fg_net_forward_to across the
pauses; the capacity refusal.  Bars: gpu_util.assert_net_bars and compare_layers' 1e-5.  Every vector of every replica, the
exchange buffers and the redirected outputs live in the arena of tests/mem_contract.py; the workspaces hold NaN and are exactly
fg_net_workspace_bytes long."""
import ctypes

import numpy as np
import pytest
import torch

import net_cases as NC
import sync_cases as SC
from gpu_util import close, dev, assert_net_bars, BAR
from test_gpu_net_fusions import compare_layers, layer_outputs

pytestmark = pytest.mark.gpu

# cases that take the fallback bar of SYNC_BN.md ("Measured bars"): {case name: factor x the float32 oracle's own error}, the factor
# that tests/NET_FUSIONS.md wires.  One: the bias of the convolution in front of the BatchNorm has the gradient 0 -- a sum of
# 131 072 x 16 cancelling terms -- and the float32 ORACLE misses the project's bar on it (6.6e-3 against 5.4e-3).
FALLBACK = {"sync-bf16x6-b64-per-shard": 4}


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math, fusion = c.get_math(), c.get_fusion()
    yield c
    c.set_math(math); c.set_fusion(fusion)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class Replica:
    """one DeviceNet on rows lo..hi of the global batch, every vector in the arena"""

    def __init__(self, ctx, ar, case, r, dn, lo, hi, x, gy, masks, first, outs, cap):
        from test_gpu_memory_contract_nets import rehouse
        d = ctx.device
        self.ctx, self.lib, self.r, self.B, self.name = ctx, ctx.lib, r, hi - lo, "%s[%d]" % (case.name, r)
        self.dn = dn
        self.xd = dev(NC.to_device(x[lo:hi], first), d)
        self.gyd = dev(NC.to_device(gy[lo:hi], outs[-1]), d)
        self.md = [dev(m, d) for m in SC.shard_masks(case, masks, lo, hi)]
        rehouse(ctx, ar, dn, self.name)
        self.gx = ar.take(self.xd.numel(), name=self.name + ".gx")
        self.sync32 = ar.take(2 * cap, name=self.name + ".sync")            # (256-byte aligned: doubles)
        self.sync = self.sync32.view(torch.float64)
        self.out = ar.take(self.gyd.numel(), align=16, name=self.name + ".out")    # fg_net_forward_to: "16-byte aligned"
        self.off = ctypes.c_longlong()
        self.mp = (ctypes.c_void_p * max(1, len(self.md)))(*[m.data_ptr() for m in self.md])
        self.sync_on(cap)

    def sync_on(self, cap):
        self.ctx.check(self.lib.fg_net_set_sync_bn(self.dn.h, 1, self.sync.data_ptr(), cap))

    def sync_off(self):
        self.ctx.check(self.lib.fg_net_set_sync_bn(self.dn.h, 0, None, 0))

    # raw return codes: the lock-step driver below looks at every one
    def forward(self, train=True, out=None, x=None, B=None):
        dn, x, B = self.dn, self.xd if x is None else x, self.B if B is None else B
        dn._batch, dn._x, dn._off = B, x, self.off
        nm = len(self.md) if train else 0
        return self.lib.fg_net_forward_to(dn.h, B, x.data_ptr(), dn.ws.data_ptr(), dn.ws.numel() * 4, 1 if train else 0, self.mp if nm else None, nm,
                                          ctypes.byref(self.off), out.data_ptr() if out is not None else None)

    def forward_resume(self):
        return self.lib.fg_net_forward_resume(self.dn.h, ctypes.byref(self.off))

    def backward(self, flags, a=None, b=0):
        dn = self.dn
        a = self.lib.fg_net_num_stages(dn.h) - 1 if a is None else a
        return self.lib.fg_net_backward_range(dn.h, dn._batch, dn._x.data_ptr(), self.gyd.data_ptr(), dn.ws.data_ptr(), dn.ws.numel() * 4, flags,
                                              self.gx.data_ptr() if flags & 2 else None, a, b)

    def backward_resume(self):
        return self.lib.fg_net_backward_resume(self.dn.h)

    def output(self):
        return self.dn._output_view().reshape(self.dn._batch, -1)


def drive(reps, start, resume, rows_of=None, what=""):
    """All replicas through one pass in lock-step.  `start` / `resume`: replica -> return code.  At every pause: every replica is
    paused, at the same fg_net_sync_count; [0, count) of its buffer is finite and slot [count - 1] holds its own rows; what lies past
    the count is bit for bit what it was when the pass began or what the previous pause left.  Then the float64 sum goes to every
    replica.  -> the counts of the pauses."""
    lib, ctx = reps[0].lib, reps[0].ctx
    counts = []
    before = [bits(r.sync).clone() for r in reps]
    rcs = [start(r) for r in reps]
    while True:
        assert len(set(rcs)) == 1, "%s: the replicas return %s at pause %d" % (what, rcs, len(counts))
        if rcs[0] != SC.FG_PAUSED_SYNC:
            ctx.check(rcs[0])
            break
        cs = [lib.fg_net_sync_count(r.dn.h) for r in reps]
        assert len(set(cs)) == 1, "%s: fg_net_sync_count %s at pause %d" % (what, cs, len(counts))
        n = cs[0]
        assert 3 <= n <= reps[0].sync.numel() and n % 2 == 1, (what, n)
        for r, b in zip(reps, before):
            head = r.sync[:n]
            assert bool(torch.isfinite(head).all()), "%s: replica %d: %d of the %d values left at pause %d are not finite" % (
                what, r.r, int((~torch.isfinite(head)).sum()), n, len(counts))
            assert torch.equal(bits(r.sync)[n:], b[n:]), "%s: replica %d wrote past fg_net_sync_count = %d at pause %d" % (what, r.r, n, len(counts))
            if rows_of is not None:
                want = rows_of(r, len(counts), n)
                assert float(head[n - 1]) == want, "%s: replica %d: slot [2C] holds %r, its own rows are %d" % (what, r.r, float(head[n - 1]), want)
        total = torch.stack([r.sync[:n] for r in reps]).sum(0)
        for r in reps:
            r.sync[:n].copy_(total)
        before = [bits(r.sync).clone() for r in reps]
        counts.append(n)
        rcs = [resume(r) for r in reps]
    return counts


def poison(reps):
    for r in reps:
        r.sync.fill_(float("nan"))


def _bars(case, net, yh, out, gxh, gin, got, e32, what=None, quiet=False):
    """test_gpu_net_fusions._bars with this module's FALLBACK"""
    what = what or case.name
    for name, v in (("outputs", yh), ("input gradient", gxh), ("parameter gradients", got)):
        assert np.isfinite(v).all(), "%s: %d of %d %s are not finite, first at %s" % (what, int((~np.isfinite(v)).sum()), v.size, name, np.argwhere(~np.isfinite(v))[0])
    if e32 is None:
        if quiet:
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                return assert_net_bars(what, net, yh, out, gxh, gin, got)
        return assert_net_bars(what, net, yh, out, gxh, gin, got)
    from oracle import torch7_nn as O
    f = FALLBACK[case.name]
    close(yh, out, atol=max(1e-5, f * e32["outputs"]), what=what + " outputs")
    close(gxh, gin, atol=max(1e-4 * np.abs(gin).max() + 1e-7, f * e32["input_gradient"]), what=what + " input gradient")
    gmax = max([float(np.abs(getattr(m, gn)).max()) for (m, pn, gn) in net.parameters()] + [0.0])
    for (m, pn, o, e) in NC.tensor_errors(net, got):
        r = getattr(m, "gradWeight" if pn == "weight" else "gradBias")
        tol = 1e-4 * np.abs(r).max() + 1e-7 + (32 * 6e-8 * getattr(m, "gw_cond", 0.0) if isinstance(m, O.PReLU) else 0.0)
        tol = max(tol, 2e-6 * gmax, f * e32["tensors"][o])
        assert e <= tol, "%s %s.%s @%d: err %.3e tol %.3e" % (what, type(m).__name__, pn, o, e, tol)


def running(case, buffers):
    """[(running_mean, running_var)] per BatchNorm from a buffers vector"""
    res, off = [], 0
    for _, C, _ in SC.batchnorms(case):
        res.append((buffers[off:off + C], buffers[off + C:off + 2 * C]))
        off += 2 * C
    return res


@pytest.mark.parametrize("case", SC.SYNC_CASES, ids=[c.name for c in SC.SYNC_CASES])
def test_sync_case_against_the_float64_oracle_on_the_global_batch(ctx, case):
    from oracle import torch7_nn as O
    from mem_contract import Arena
    lib, d, B = ctx.lib, ctx.device, case.batch
    ctx.set_math(case.math); ctx.set_fusion(case.fusion)         # the fusion bits are read when a net is created
    try:
        net, mods, P, G, x, gy, masks = NC.operands(case, np.float64)
        first, outs = NC.walk(case.layers, case.dims)
        bnl, cap, want = SC.batchnorms(case), SC.capacity(case), SC.sync_counts(case)
        bns = [mods[i] for i, _, _ in bnl]
        P32 = P.astype(np.float32)
        buf0 = np.concatenate([np.concatenate([m.running_mean, m.running_var]) for m in bns]).astype(np.float32)
        n_in, n_out = int(np.prod(first.shape)), int(np.prod(outs[-1].shape))
        nets = [NC.device_net(ctx, case.layers, case.dims, s) for s in case.shards]
        sizes = []
        for dn, s in zip(nets, case.shards):
            sizes += [dn.n_params, dn.n_params, max(dn.n_buffers, 1), dn.ws.numel(), s * n_in, 2 * cap, s * n_out]
        ar = Arena.sized(d, sizes)
        reps = [Replica(ctx, ar, case, r, dn, lo, hi, x, gy, masks, first, outs, cap) for r, (dn, (lo, hi)) in enumerate(zip(nets, SC.bounds(case)))]
        ns = lib.fg_net_num_stages(reps[0].dn.h)

        def reset():
            for r in reps:
                assert r.dn.n_params == P.size and r.dn.n_masks == len(masks)
                r.dn.params.copy_(torch.from_numpy(P32)); r.dn.buffers.copy_(torch.from_numpy(buf0))
                r.dn.ws.fill_(float("nan")); r.dn.params_changed()

        reset()
        rows_fwd = lambda r, k, n: r.dn._batch * bnl[k][2]
        rows_bwd = lambda r, k, n: r.dn._batch * bnl[len(bnl) - 1 - k][2]

        # ---- forward (train) ------------------------------------------------------------------------------------------------
        poison(reps)
        got = drive(reps, lambda r: r.forward(), lambda r: r.forward_resume(), rows_fwd, case.name + " forward")
        assert got == want, "%s: a forward paused at fg_net_sync_count %s, the BatchNorms are %s" % (case.name, got, want)
        ys = [r.output().clone() for r in reps]
        yh = NC.from_device(torch.cat(ys).cpu().numpy(), outs[-1])
        per = [layer_outputs(r.dn, case, outs, r.B) for r in reps]
        assert all(sorted(p) == sorted(per[0]) for p in per)
        layers = {i: np.concatenate([p[i] for p in per], 0) for i in per[0]}
        buffers = [r.dn.buffers.clone() for r in reps]
        saved = [saved_stats(ctx, r.dn, bnl) for r in reps]
        SC.adopt_shards(ctx, [r.dn for r in reps], case, mods, x, P32)
        out, gin = NC.oracle_pass(net, G, x, gy, masks)
        flips, units = NC.flips(net)
        SC.clear_adopted(mods)
        compare_layers(case.name + " train", layers, mods)
        assert flips <= max(1, 1e-5 * units), "%d of %d PReLU decisions adopted from the devices differ from the oracle's" % (flips, units)
        # ---- running statistics: the global-batch ones on every replica --------------------------------------------------------
        for r, b in zip(reps[1:], buffers[1:]):
            assert torch.equal(bits(b), bits(buffers[0])), "%s: the running statistics of replica %d differ from replica 0's" % (case.name, r.r)
            for a, c in zip(saved[0], saved[r.r]):
                assert torch.equal(bits(a), bits(c)), "%s: the saved mean / invstd of replica %d differ from replica 0's" % (case.name, r.r)
        for m, (rm, rv) in zip(bns, running(case, buffers[0].cpu().numpy())):
            print("%s: running_mean err %.3e (bar %.0e), running_var rel err %.3e (bar %.0e)" % (
                case.name, np.abs(rm - m.running_mean).max(), BAR["bn_running_mean"], (np.abs(rv - m.running_var) / np.abs(m.running_var)).max(), BAR["bn_running_var_rtol"]))
            close(rm, m.running_mean, atol=BAR["bn_running_mean"], what=case.name + " running_mean")
            close(rv, m.running_var, atol=0.0, rtol=BAR["bn_running_var_rtol"], what=case.name + " running_var")

        # ---- backward, both flags ---------------------------------------------------------------------------------------------
        def backward(flags, a=None, b=0, what="backward"):
            poison(reps)
            return drive(reps, lambda r: r.backward(flags, a, b), lambda r: r.backward_resume(), None if a is not None else rows_bwd,
                         "%s %s flags %d" % (case.name, what, flags))

        def nan_fill():
            for r in reps:
                r.dn.grads.fill_(float("nan")); r.gx.fill_(float("nan"))

        def results():
            gsum = sum(r.dn.grads.cpu().numpy().astype(np.float64) for r in reps)
            return gsum, NC.from_device(torch.cat([r.gx.reshape(r.B, -1) for r in reps]).cpu().numpy(), first)

        nan_fill()
        assert backward(3) == want[::-1], "%s: the pauses of a backward" % case.name
        g3, gx3 = [r.dn.grads.clone() for r in reps], [r.gx.clone() for r in reps]
        gsum, gxh = results()
        e32 = NC.reference_errors(case) if case.name in FALLBACK else None
        _bars(case, net, yh, out, gxh, gin, gsum, e32)
        # ---- the two flags in two calls: the same bits ------------------------------------------------------------------------
        nan_fill()
        assert backward(1) == want[::-1]
        for r in reps:
            assert torch.equal(bits(r.dn.grads), bits(g3[r.r])), "%s: FG_BWD_PARAM_GRADS alone gives other gradients" % r.name
            assert bool(torch.isnan(r.gx).all()), "%s: FG_BWD_PARAM_GRADS alone wrote the input gradient" % r.name
            r.dn.grads.fill_(float("nan"))
        assert backward(2) == want[::-1]
        for r in reps:
            assert torch.equal(bits(r.gx), bits(gx3[r.r])), "%s: FG_BWD_INPUT_GRAD alone gives another input gradient" % r.name
            assert bool(torch.isnan(r.dn.grads).all()), "%s: FG_BWD_INPUT_GRAD alone wrote parameter gradients" % r.name
        # ---- fg_net_backward_range split at every stage boundary, each half through its own pauses -----------------------------
        for s in range(1, ns):
            nan_fill()
            got = backward(3, ns - 1, s, "range") + backward(3, s - 1, 0, "range")
            assert got == want[::-1], "%s split at stage %d: pauses %s" % (case.name, s, got)
            gsum, gxs = results()
            _bars(case, net, yh, out, gxs, gin, gsum, e32, what="%s split at stage %d" % (case.name, s), quiet=True)

        # ---- evaluate with sync on: no pause, the bits of evaluate with sync off, the running statistics stay ------------------
        r0 = reps[0]
        poison(reps)
        rc = r0.forward(train=False)
        assert rc == SC.FG_OK, "%s: an evaluate forward with sync on returns %d" % (case.name, rc)
        ye = r0.output().clone()
        assert bool(torch.isnan(r0.sync).all()), "%s: an evaluate forward wrote the exchange buffer" % case.name
        r0.sync_off()
        assert r0.forward(train=False) == SC.FG_OK
        assert bool(torch.isfinite(ye).all()) and torch.equal(bits(ye), bits(r0.output())), "%s: evaluate with sync on gives other bits than with sync off" % case.name
        assert torch.equal(bits(r0.dn.buffers), bits(buffers[0])), "%s: an evaluate forward moved the running statistics" % case.name
        r0.sync_on(cap)

        # ---- with sync on the producing convolution writes no epilogue statistics (`!n->sync_bn` in ST_CONV) -------------------
        # Nothing reads them under sync, so no value shows them; the workspace does.  Where the plain forward takes its statistics from
        # the producer's epilogue (SC.EPILOGUE_CASES, held to the planning-only log by the host test) it writes a slice of the
        # workspace that no kernel of the sync forward writes: from NaN workspaces, some float is finite behind the plain forward
        # and still NaN behind the sync one.
        if case.name in SC.EPILOGUE_CASES:
            written = {}
            for on in (True, False):
                r0.dn.ws.fill_(float("nan")); poison([r0])
                r0.sync_on(cap) if on else r0.sync_off()
                drive([r0], lambda r: r.forward(), lambda r: r.forward_resume(), None, case.name + " epilogue")
                written[on] = torch.isfinite(r0.dn.ws)
            only = int((written[False] & ~written[True]).sum())
            print("%s: %d floats of the workspace are written by the plain forward alone (the epilogue's statistics)" % (case.name, only))
            assert only > 0, "%s: with sync on the workspace holds everything the plain forward writes: the epilogue statistics were written" % case.name
            r0.sync_on(cap)

        # ---- the redirected output of fg_net_forward_to across the pauses ------------------------------------------------------
        reset(); poison(reps)
        for r in reps:
            r.out.fill_(float("nan"))
        got = drive(reps, lambda r: r.forward(out=r.out), lambda r: r.forward_resume(), rows_fwd, case.name + " forward_to")
        assert got == want
        last = len(case.layers) - 1
        for r in reps:
            assert torch.equal(bits(r.out), bits(ys[r.r].reshape(-1))), "%s: fg_net_forward_to leaves other bits than fg_net_forward" % r.name
            rc = lib.fg_net_layer_output(r.dn.h, last, None, None, None, None)
            assert rc == SC.FG_ERR_INVALID and "redirected" in lib.fg_last_error(ctx.h).decode(), (r.name, rc)
            assert torch.equal(bits(r.dn.buffers), bits(buffers[r.r])), "%s: the running statistics behind fg_net_forward_to" % r.name
        torch.cuda.synchronize()
        ar.assert_guards(case.name + " fg_net_forward_to")       # nothing past B * C * H * W floats of the caller's buffer

        # ---- two replicas on the same shard: the bits of one replica on it -----------------------------------------------------
        if len(reps) >= 2:
            duplicate_shards(ctx, case, reps, reset, net, mods, x, masks, bnl, buf0)

        # ---- capacity: 2 C doubles for the widest BatchNorm ---------------------------------------------------------------------
        k = want.index(max(want))
        reset(); poison([r0])
        r0.sync_on(cap - 1)
        tail = bits(r0.sync)[cap - 1:].clone()
        seen = []
        rc = r0.forward()
        while rc == SC.FG_PAUSED_SYNC:
            seen.append(lib.fg_net_sync_count(r0.dn.h)); rc = r0.forward_resume()
        assert rc == SC.FG_ERR_WORKSPACE and seen == want[:k], "%s: capacity %d: return code %d behind the pauses %s" % (case.name, cap - 1, rc, seen)
        assert r0.forward_resume() == SC.FG_ERR_INVALID and r0.backward(3) == SC.FG_ERR_INVALID
        assert torch.equal(bits(r0.sync)[cap - 1:], tail), "%s: the double past a capacity of %d was written" % (case.name, cap - 1)
        r0.sync_on(cap)
        rc = r0.forward()
        while rc == SC.FG_PAUSED_SYNC:
            rc = r0.forward_resume()
        ctx.check(rc)
        assert bool(torch.isfinite(r0.output()).all())
        torch.cuda.synchronize()
        ar.assert_guards(case.name)
    finally:
        ctx.set_math(0); ctx.set_fusion(503)


def saved_stats(ctx, dn, bnl):
    """[mean | invstd] of every BatchNorm as the last train forward left them in the workspace (fg_net_bn_saved_stats), clones"""
    res = []
    for i, C, _ in bnl:
        mo, io, cc = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
        ctx.check(ctx.lib.fg_net_bn_saved_stats(dn.h, i, ctypes.byref(mo), ctypes.byref(io), ctypes.byref(cc)))
        assert cc.value == C
        res.append(torch.cat([dn.ws[mo.value:mo.value + C], dn.ws[io.value:io.value + C]]).clone())
    return res


def duplicate_shards(ctx, case, reps, reset, net, mods, x, masks, bnl, buf0):
    """Replicas 0 and 1 both on the first s rows of the batch against replica 0 alone on them: doubling both sums and the row count is
    exact in fp64, so outputs, saved mean and invstd, input gradient and running mean are bit-equal; the running variance differs
    by the unbiased factor n / (n - 1) alone and is held to the float64 oracle on the doubled batch."""
    from oracle import torch7_nn as O
    a, b = reps[0], reps[1]
    s = min(a.B, b.B)
    d = ctx.device
    first, outs = NC.walk(case.layers, case.dims)
    xs, gys = a.xd[:s].contiguous(), a.gyd[:s].contiguous()
    ms = [dev(m, d) for m in SC.shard_masks(case, masks, 0, s)]

    def run(group):
        reset(); poison(group)
        for r in group:
            r.saved_md, r.saved_gy, r.saved_mp = r.md, r.gyd, r.mp
            r.md, r.gyd = ms, gys
            r.mp = (ctypes.c_void_p * max(1, len(ms)))(*[m.data_ptr() for m in ms])
            r.gx.fill_(float("nan"))
        try:
            drive(group, lambda r: r.forward(x=xs, B=s), lambda r: r.forward_resume(), lambda r, k, n: s * bnl[k][2], case.name + " duplicate forward")
            res = [dict(y=r.output().clone(), saved=saved_stats(ctx, r.dn, bnl), buffers=r.dn.buffers.clone()) for r in group]
            poison(group)
            drive(group, lambda r: r.backward(3), lambda r: r.backward_resume(), lambda r, k, n: s * bnl[len(bnl) - 1 - k][2], case.name + " duplicate backward")
            for r, e in zip(group, res):
                e["gx"], e["grads"] = r.gx[:s * xs[0].numel()].clone(), r.dn.grads.clone()
        finally:
            for r in group:
                r.md, r.gyd, r.mp = r.saved_md, r.saved_gy, r.saved_mp
        return res

    one = run([a])[0]
    two = run([a, b])
    C2 = [c for _, c, _ in bnl]
    for k, e in enumerate(two):
        what = "%s: replica %d of two on the same shard" % (case.name, k)
        assert torch.equal(bits(e["y"]), bits(one["y"])), what + ": other outputs than one replica on it"
        for u, v in zip(e["saved"], one["saved"]):
            assert torch.equal(bits(u), bits(v)), what + ": other saved mean / invstd"
        assert torch.equal(bits(e["gx"]), bits(one["gx"])), what + ": another input gradient"
        assert torch.equal(bits(e["grads"]), bits(one["grads"])), what + ": other local parameter gradients"
        for (rm2, _), (rm1, _) in zip(running(case, e["buffers"]), running(case, one["buffers"])):
            assert torch.equal(bits(rm2), bits(rm1)), what + ": another running mean"
    # the running variances: the float64 oracle on the batch of s rows and on the same rows twice
    for rows, e in ((1, one), (2, two[0])):
        bns = [mods[i] for i, _, _ in bnl]
        off = 0
        for m in bns:
            m.running_mean[...] = buf0[off:off + m.nf]; m.running_var[...] = buf0[off + m.nf:off + 2 * m.nf]
            off += 2 * m.nf
        O.set_dropout_masks(net, [np.concatenate([m[:s]] * rows, 0) for m in masks])
        net.training()
        net.forward(np.concatenate([x[:s]] * rows, 0).astype(np.float64))
        for m, (rm, rv) in zip(bns, running(case, e["buffers"].cpu().numpy())):
            close(rm, m.running_mean, atol=BAR["bn_running_mean"], what="%s: running_mean, %d x the shard" % (case.name, rows))
            close(rv, m.running_var, atol=0.0, rtol=BAR["bn_running_var_rtol"], what="%s: running_var, %d x the shard" % (case.name, rows))
    assert C2 and any(not torch.equal(bits(u[1]), bits(v[1])) for u, v in zip(running(case, two[0]["buffers"]), running(case, one["buffers"]))), \
        "%s: the running variance of 2 n rows equals the one of n rows: the row count was not summed" % case.name
