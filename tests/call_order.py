"""Does an object with a past still give the right answer?  The scenarios of tests/CALL_ORDER.md, written once and run twice:
on the device (tests/test_gpu_call_order.py compares what they return) and on a planning-only context with FG_LAUNCH_LOG=1
(tests/test_call_order_host.py compares the launch logs of the marked probes and the return codes).  Helper module, imported like
gpu_util / mem_contract; `python tests/call_order.py host` is the child program of the host test.

The reference is a FRESH TWIN: an object of the same specs, created under the same fusion word AFTER the used object ran its history,
bound to copies of the used object's vectors as they stand at that moment (parameters, gradients, BatchNorm buffers; for a gan the
optimizer state, the step counts and explicit noise / masks), its workspaces pre-filled with NaN.  Both run the same probe; everything the
probe produces must be bit-equal.  The one exception (tests/test_gpu_fusion.py::prelu_fused_equals_separate): where a scenario moves a
PReLU backward out of its neighbour's epilogue the slope gradients are held to 2e-3 * scale + 1e-6 and everything else stays bit-equal."""
import contextlib
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FG_FUSE_PRELU, FG_FUSE_WFINISH_BATCH, FG_FUSE_ADAM_PACK, FG_FUSE_DEFAULT = 1, 4, 8, 503
WINO_ALL = 32 | 64 | 128 | 256
FG_ERR_INVALID, FG_ERR_WORKSPACE, FG_PAUSED_SYNC = -1, -5, 1
NAN = float("nan")
DRY = False          # the host run: nothing is computed, so no tensor is compared (the logs and the return codes are)

# kind -> (max_batch, the smaller odd probe batch)
KINDS = dict(G32=(8, 3), D32=(8, 3), c2fG=(4, 3), c2fD=(4, 3), D16b=(8, 5))
PAIRS = dict(px32=("G32", "D32", 0, 8), c2f=("c2fG", "c2fD", 1, 4))       # G, D, table_inputs, B


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


class Inp:
    def __init__(self, x, gy, masks):
        self.x, self.gy, self.masks = x, gy, masks


class Env:
    """one context + the cached base nets (specs and seeded parameters from the builders of the parity tests)"""

    def __init__(self, ctx, log=None):
        self.ctx, self.lib, self.log = ctx, ctx.lib, log
        self._base = {}

    # ---- markers of the host run -----------------------------------------------------------------------------------------------
    def say(self, s):
        if self.log is not None:
            self.log.write("fg-co " + s + "\n")
            self.log.flush()

    @contextlib.contextmanager
    def probe(self, who, tag):
        self.say("probe %s %s" % (who, tag))
        try:
            yield
        finally:
            self.say("probe end")

    @contextlib.contextmanager
    def fusion(self, flags):
        prev = self.ctx.get_fusion()
        if flags is not None:
            self.ctx.set_fusion(flags)
        try:
            yield
        finally:
            self.ctx.set_fusion(prev)

    @contextlib.contextmanager
    def math(self, mode):
        prev = self.ctx.get_math()
        self.ctx.set_math(mode)
        try:
            yield
        finally:
            self.ctx.set_math(prev)

    # ---- nets --------------------------------------------------------------------------------------------------------------------
    def base(self, kind):
        """-> (DeviceNet holding the seeded parameters, the oracle net of the same structure or None)"""
        if kind not in self._base:
            ctx = self.ctx
            with self.fusion(FG_FUSE_DEFAULT):
                if kind in ("G32", "D32"):
                    import test_gpu_net as T
                    st, Gd, Dd, _ = T.build(ctx, 3, 8, seed=4242)
                    self._base["G32"], self._base["D32"] = (Gd.device_net, st.G, st.gG), (Dd.device_net, st.D, st.gD)
                elif kind in ("c2fG", "c2fD"):
                    import test_gpu_c2f as T
                    st, Gd, Dd, _ = T.build(ctx, 16, 4, seed=4243)
                    self._base["c2fG"], self._base["c2fD"] = (Gd.inner.device_net, None, None), (Dd.inner.device_net, None, None)
                else:
                    import numpy as np
                    from face_generator_amd import models
                    from test_branched_host import ORACLES
                    from test_gpu_net import _fill_nontrivial
                    rng = np.random.default_rng(4244)
                    D = ORACLES["create_D16_b"]((3, 16, 16), rng)
                    _fill_nontrivial(D, rng)
                    pD, _ = D.getParameters()
                    Dd = models.create_D16_b((3, 16, 16)).cuda(ctx, max_batch=8)
                    Dd.getParameters()[0].copy_(torch.tensor(pD))
                    self._base["D16b"] = (Dd.device_net, None, None)
        return self._base[kind]

    def net(self, kind, create_fusion=None):
        """a fresh net of that kind, created under `create_fusion` (None: the default word), holding the base parameters"""
        from face_generator_amd.runtime import DeviceNet
        b = self.base(kind)[0]
        with self.fusion(FG_FUSE_DEFAULT if create_fusion is None else create_fusion):
            dn = DeviceNet(self.ctx, b.layers, (b.in_c, b.in_h, b.in_w), KINDS[kind][0])
        dn.params.copy_(b.params)
        dn.params_changed()
        dn.kind, dn.create_fusion = kind, create_fusion
        return dn

    def twin(self, dn):
        """created NOW, under the creation word of `dn`, bound to copies of its vectors as they stand; workspace NaN"""
        from face_generator_amd.runtime import DeviceNet
        with self.fusion(FG_FUSE_DEFAULT if dn.create_fusion is None else dn.create_fusion):
            t = DeviceNet(self.ctx, dn.layers, (dn.in_c, dn.in_h, dn.in_w), dn.max_batch)
        t.params.copy_(dn.params); t.grads.copy_(dn.grads); t.buffers.copy_(dn.buffers)
        t.params_changed()
        t.ws.fill_(NAN)
        t.kind, t.create_fusion = dn.kind, dn.create_fusion
        return t

    def inputs(self, dn, b, seed=1):
        ctx, lib = self.ctx, self.lib
        shape = (b, dn.in_h, dn.in_w, dn.in_c) if dn.in_h * dn.in_w > 1 else (b, dn.in_c)
        oshape = (b, dn.out_h, dn.out_w, dn.out_c) if dn.out_h * dn.out_w > 1 else (b, dn.out_c)
        x = ctx.uniform(shape, -1.0 if dn.kind in ("G32", "c2fG") else 0.0, 1.0, seed=1000 * seed + b)
        gy = ctx.normal(oshape, 0.0, 1.0, seed=1000 * seed + 100 + b)
        masks = [ctx.bernoulli((lib.fg_net_mask_elems(dn.h, i, b),), lib.fg_net_mask_keep(dn.h, i), seed=1000 * seed + 200 + 10 * i + b)
                 for i in range(dn.n_masks)]
        return Inp(x, gy, masks)


# ---- one net: calls, results, comparison --------------------------------------------------------------------------------------------
def forward_rc(dn, inp, train=True):
    return dn._forward_call(inp.x, inp.masks or None, train)


def forward_to_rc(dn, inp, out, train=True):
    B = inp.x.shape[0]
    mp = (ctypes.c_void_p * dn.n_masks)(*[m.data_ptr() for m in inp.masks]) if (train and dn.n_masks) else None
    dn._off, dn._batch, dn._x, dn._masks = ctypes.c_longlong(), B, inp.x, inp.masks
    return dn.lib.fg_net_forward_to(dn.h, B, inp.x.data_ptr(), dn.ws.data_ptr(), dn.ws.numel() * 4, 1 if train else 0, mp,
                                    dn.n_masks if mp is not None else 0, ctypes.byref(dn._off), out.data_ptr())


def backward_rc(dn, inp, flags=3, gx=None, stage_from=None, stage_to=0, batch=None):
    lib = dn.lib
    if stage_from is None:
        stage_from = lib.fg_net_num_stages(dn.h) - 1
    return lib.fg_net_backward_range(dn.h, dn._batch if batch is None else batch, inp.x.data_ptr(), inp.gy.data_ptr(), dn.ws.data_ptr(),
                                     dn.ws.numel() * 4, flags, gx.data_ptr() if gx is not None else None, stage_from, stage_to)


def new_gx(env, inp):
    gx = env.ctx.empty(*inp.x.shape)
    gx.fill_(NAN)
    return gx


def fb(env, dn, inp, flags=3):
    """a piece of history: train forward + backward, results dropped"""
    env.ctx.check(forward_rc(dn, inp))
    env.ctx.check(backward_rc(dn, inp, flags, new_gx(env, inp) if flags & 2 else None))


def forward_results(dn, train=True, redirected=None):
    lib, B, res = dn.lib, dn._batch, {}
    res["output"] = (redirected if redirected is not None else dn._output_view()).reshape(-1).clone()
    off, c, h, w, o2 = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    for li, l in enumerate(dn.layers):
        if lib.fg_net_layer_output(dn.h, li, ctypes.byref(off), ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)) == 0:
            res["layer%d" % li] = dn.ws[off.value: off.value + B * c.value * h.value * w.value].clone()
        if train and l[0] == "BATCHNORM":
            dn.ctx.check(lib.fg_net_bn_saved_stats(dn.h, li, ctypes.byref(off), ctypes.byref(o2), ctypes.byref(c)))
            res["bn%d.mean" % li] = dn.ws[off.value: off.value + c.value].clone()
            res["bn%d.invstd" % li] = dn.ws[o2.value: o2.value + c.value].clone()
    return res


def probe(env, dn, inp, train=True, flags=3, back=True):
    """the standard probe: a forward [+ a backward with both flags]; -> everything it produced, cloned"""
    env.ctx.check(forward_rc(dn, inp, train))
    res = forward_results(dn, train)
    if back and train:
        gx = new_gx(env, inp)
        env.ctx.check(backward_rc(dn, inp, flags, gx if flags & 2 else None))
        res["gx"], res["grads"] = gx.reshape(-1).clone(), dn.grads.clone()
    res["buffers"] = dn.buffers.clone()
    return res


def slope_indices(dn):
    return [dn.param_offsets(li)[0] for li, l in enumerate(dn.layers) if l[0] == "PRELU" and dn.param_offsets(li)[0] >= 0]


def diff(tag, a, b, slopes=None, keys=None):
    """-> messages, one per tensor of a that is not bit-equal to b's (slopes: flat indices of `grads` held to the PReLU bar instead)"""
    msgs = []
    if DRY:
        return msgs
    for k in (keys or a.keys()):
        if k not in b:
            msgs.append("%s: %s missing on one side" % (tag, k))
            continue
        x, y = a[k], b[k]
        if x.shape != y.shape:
            msgs.append("%s: %s shapes %s / %s" % (tag, k, tuple(x.shape), tuple(y.shape)))
            continue
        if x.dtype == torch.float32 and bool(torch.isnan(y).any()):
            msgs.append("%s: %s holds %d NaN on the twin" % (tag, k, int(torch.isnan(y).sum())))
        if k == "grads" and slopes:
            keep = torch.ones(x.numel(), dtype=torch.bool, device=x.device)
            keep[slopes] = False
            for i in slopes:
                xa, ya = float(x[i]), float(y[i])
                scale = max(abs(xa), abs(ya), 1e-30)
                if not abs(xa - ya) <= 2e-3 * scale + 1e-6:
                    msgs.append("%s: slope gradient at %d: %.8g vs %.8g (bar %.3g)" % (tag, i, xa, ya, 2e-3 * scale + 1e-6))
            x, y = x[keep], y[keep]
        ne = bits(x).reshape(-1) != bits(y).reshape(-1)
        if bool(ne.any()):
            i = int(torch.nonzero(ne).reshape(-1)[0])
            msgs.append("%s: %s differs in %d of %d elements, first at %d (%r vs %r)"
                        % (tag, k, int(ne.sum()), x.numel(), i, float(x.reshape(-1)[i]), float(y.reshape(-1)[i])))
    return msgs


def check(env, used, inp, tag, msgs, used_fn=probe, twin_fn=None, slopes=None, **kw):
    """the twin is created now; then the probe runs on the used object and on the twin"""
    twin = env.twin(used)
    with env.probe("used", tag):
        ru = used_fn(env, used, inp, **kw)
    with env.probe("twin", tag):
        rt = (twin_fn or used_fn)(env, twin, inp, **kw)
    msgs += diff(tag, ru, rt, slopes)
    return ru, rt


# ---- net scenarios: f(env, kind) -> list of mismatch messages ----------------------------------------------------------------------
def s01_batch_history(env, kind):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    iM, io = env.inputs(dn, M), env.inputs(dn, odd)
    fb(env, dn, iM); fb(env, dn, io)
    check(env, dn, iM, "after B=%d, %d: probe at %d" % (M, odd, M), msgs)
    check(env, dn, io, "then probe at %d" % odd, msgs)
    check(env, dn, iM, "and at %d again" % M, msgs)
    env.ctx.check(forward_rc(dn, io))                                   # a forward with no backward
    check(env, dn, iM, "after a forward without backward", msgs)
    return msgs


def s02_mode_history(env, kind):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    iM, io, i2 = env.inputs(dn, M), env.inputs(dn, odd), env.inputs(dn, 2)
    fb(env, dn, iM)                                                     # moves the running statistics
    for i in (env.inputs(dn, M - 2 if M > 4 else M), i2):               # the sampler: evaluate mode, a chunk and a tail
        env.ctx.check(forward_rc(dn, i, train=False))
    rc = backward_rc(dn, i2, 3, new_gx(env, i2))
    if rc != FG_ERR_INVALID:
        msgs.append("backward after an evaluate forward returned %d" % rc)
    check(env, dn, iM, "train probe after evaluate forwards", msgs)
    fb(env, dn, io)
    check(env, dn, io, "evaluate probe after train passes", msgs, train=False)
    check(env, dn, iM, "evaluate probe at max_batch", msgs, train=False)
    return msgs


def s03_repeated_backward(env, kind):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    for b in (M, odd):
        inp = env.inputs(dn, b)
        env.ctx.check(forward_rc(dn, inp))
        res = []
        for rep, who in enumerate(("twin", "used")):                    # the first backward is the reference of the second
            gx = new_gx(env, inp)
            with env.probe(who, "repeated backward at B=%d" % b):
                env.ctx.check(backward_rc(dn, inp, 3, gx))
            res.append(dict(gx=gx.clone(), grads=dn.grads.clone()))
            dn.grads.fill_(7.0)                                         # overwritten, not accumulated
        msgs += diff("second backward at B=%d" % b, res[1], res[0])
    return msgs


def s04_split_flags(env, kind):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    for b in (M, odd):
        inp = env.inputs(dn, b)
        twin = env.twin(dn)
        env.ctx.check(forward_rc(dn, inp))
        gx = new_gx(env, inp)
        env.ctx.check(backward_rc(dn, inp, 1, None))
        env.ctx.check(backward_rc(dn, inp, 2, gx))
        rt = probe(env, twin, inp)
        msgs += diff("param grads, then input grad at B=%d" % b, dict(gx=gx.reshape(-1), grads=dn.grads), rt, keys=("gx", "grads"))
        check(env, dn, inp, "probe after split flags at B=%d" % b, msgs)
    return msgs


def s05_ranged_backward(env, kind):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    ns, slopes = env.lib.fg_net_num_stages(dn.h), slope_indices(dn)
    for b in (M, odd):
        inp = env.inputs(dn, b)
        ref = probe(env, env.twin(dn), inp)                             # the single call, on a fresh net
        cuts = [[(ns - 1, k), (k - 1, 0)] for k in range(1, ns)] + [[(s, s) for s in range(ns - 1, -1, -1)]]
        for cut in cuts:
            env.ctx.check(forward_rc(dn, inp))
            gx = new_gx(env, inp)
            dn.grads.fill_(NAN)
            for (a, z) in cut:
                env.ctx.check(backward_rc(dn, inp, 3, gx, a, z))
            msgs += diff("B=%d ranges %s" % (b, cut if len(cut) == 2 else "one stage at a time"),
                         dict(gx=gx.reshape(-1), grads=dn.grads), ref, slopes, keys=("gx", "grads"))
        env.ctx.check(forward_rc(dn, inp))
        env.ctx.check(backward_rc(dn, inp, 3, new_gx(env, inp), ns - 1, ns // 2))     # abandoned
        check(env, dn, inp, "probe after an abandoned range at B=%d" % b, msgs)
    return msgs


def _fwd_then_bwd_in(fwd_math=None, bwd_math=None, fwd_fusion=None, bwd_fusion=None):
    def run(env, dn, inp):
        ctx = env.ctx
        m0, f0 = ctx.get_math(), ctx.get_fusion()
        try:
            if fwd_math is not None: ctx.set_math(fwd_math)
            if fwd_fusion is not None: ctx.set_fusion(fwd_fusion)
            ctx.check(forward_rc(dn, inp))
            res = forward_results(dn)
            if bwd_math is not None: ctx.set_math(bwd_math)
            if bwd_fusion is not None: ctx.set_fusion(bwd_fusion)
            gx = new_gx(env, inp)
            ctx.check(backward_rc(dn, inp, 3, gx))
            res.update(gx=gx.reshape(-1).clone(), grads=dn.grads.clone(), buffers=dn.buffers.clone())
            return res
        finally:
            ctx.set_math(m0); ctx.set_fusion(f0)
    return run


# the math-mode scenarios create their nets with the Winograd bits cleared AS WELL: those bits win over fg_set_math (facegen_hip.h), and
# with them most contractions of these nets never look at the bf16x6 planes
NO_WINO = FG_FUSE_DEFAULT & ~WINO_ALL


def s06_math_mode(env, kind, results=None):
    M, odd = KINDS[kind]
    msgs = []
    for cf in (None, NO_WINO):
        with env.fusion(FG_FUSE_DEFAULT if cf is None else cf):
            dn = env.net(kind, cf)
            iM, io = env.inputs(dn, M), env.inputs(dn, odd)
            tag = "created with fusion %s: " % ("default" if cf is None else "without Winograd")
            with env.math(6):
                fb(env, dn, iM); fb(env, dn, io)
            with env.math(0):
                r60 = check(env, dn, iM, tag + "mode 6 history, probe in mode 0", msgs)[0]
                fb(env, dn, io)
            with env.math(6):
                r06 = check(env, dn, iM, tag + "mode 0 history, probe in mode 6", msgs)[0]
                check(env, dn, io, tag + "mode 6 probe at the odd batch", msgs)
            r0b = check(env, dn, iM, tag + "forward in mode 0, backward in mode 6", msgs, used_fn=_fwd_then_bwd_in(0, 6))[0]
            r6b = check(env, dn, iM, tag + "forward in mode 6, backward in mode 0", msgs, used_fn=_fwd_then_bwd_in(6, 0))[0]
            if results is not None:
                results[cf] = (dn, iM, dict(mode6_then_0=r60, mode0_then_6=r06, fwd0_bwd6=r0b, fwd6_bwd0=r6b))
    return msgs


def s07_fusion_word(env, kind, results=None):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    iM, io = env.inputs(dn, M), env.inputs(dn, odd)
    slopes = slope_indices(dn)
    with env.fusion(FG_FUSE_DEFAULT & ~FG_FUSE_PRELU):
        fb(env, dn, iM); fb(env, dn, io)
    check(env, dn, iM, "FG_FUSE_PRELU cleared, then default: probe", msgs)
    with env.fusion(FG_FUSE_DEFAULT & ~FG_FUSE_PRELU):
        check(env, dn, io, "default, then FG_FUSE_PRELU cleared: probe", msgs)
    # the bit cleared between forward and backward, against the unswitched run
    twin = env.twin(dn)
    ru = _fwd_then_bwd_in(bwd_fusion=FG_FUSE_DEFAULT & ~FG_FUSE_PRELU)(env, dn, iM)
    msgs += diff("FG_FUSE_PRELU cleared between forward and backward", ru, probe(env, twin, iM), slopes)
    check(env, dn, iM, "probe after the switch between the passes", msgs)
    # created without the arena for parked weight-gradient partials, run with the bit set
    dn2 = env.net(kind, FG_FUSE_DEFAULT & ~FG_FUSE_WFINISH_BATCH)
    fb(env, dn2, io)
    r = check(env, dn2, iM, "created with FG_FUSE_WFINISH_BATCH cleared, run with it set", msgs)[0]
    if results is not None:
        results["wfinish"] = (dn2, iM, r)
    return msgs


def _move_host_write(env, dn):
    dn.params.mul_(1.03125)
    dn.params_changed()


def _move_bind(env, dn):
    p2 = (dn.params * 0.96875).contiguous()
    env.ctx.check(env.lib.fg_net_bind(dn.h, p2.data_ptr(), dn.grads.data_ptr(), dn.buffers.data_ptr()))
    dn.params = p2


def s08_params_moved(env, kind):
    """the host-side moves; the optimizer moves are g08_optimizer_moves"""
    M, odd = KINDS[kind]
    msgs = []
    for mode, cf in ((0, None), (6, NO_WINO)):
        with env.fusion(FG_FUSE_DEFAULT if cf is None else cf), env.math(mode):
            dn = env.net(kind, cf)
            iM, io = env.inputs(dn, M), env.inputs(dn, odd)
            fb(env, dn, iM)
            for name, move in (("a host write + fg_net_params_changed", _move_host_write), ("fg_net_bind to another vector", _move_bind)):
                move(env, dn)
                check(env, dn, iM, "math %d: %s" % (mode, name), msgs)
                fb(env, dn, io)
    return msgs


def s09_forward_to(env, kind):
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    last = len(dn.layers) - 1
    for b in (M, odd):
        inp = env.inputs(dn, b)
        ext = env.ctx.empty(b * dn.out_c * dn.out_h * dn.out_w)
        ext.fill_(NAN)
        env.ctx.check(forward_to_rc(dn, inp, ext))
        if env.lib.fg_net_layer_output(dn.h, last, None, None, None, None) != FG_ERR_INVALID:
            msgs.append("fg_net_layer_output of the last layer is legal while the output is redirected")
        ru, rt = check(env, dn, inp, "a plain forward after fg_net_forward_to at B=%d" % b, msgs)
        if env.lib.fg_net_layer_output(dn.h, last, None, None, None, None) != 0:
            msgs.append("fg_net_layer_output of the last layer stays refused after a plain forward")

        def to_ext(env, d, inp):
            ext.fill_(NAN)
            env.ctx.check(forward_to_rc(d, inp, ext))
            res = forward_results(d, redirected=ext)
            gx = new_gx(env, inp)
            env.ctx.check(backward_rc(d, inp, 3, gx))
            res.update(gx=gx.reshape(-1).clone(), grads=d.grads.clone(), buffers=d.buffers.clone())
            return res
        check(env, dn, inp, "fg_net_forward_to + backward at B=%d against forward + backward" % b, msgs, used_fn=to_ext, twin_fn=probe)
    return msgs


def s10_abandoned_pause(env, kind):
    """kinds with a SpatialBatchNormalization only"""
    M, odd = KINDS[kind]
    dn, msgs = env.net(kind), []
    lib = env.lib
    cmax = max(l[1] for l in dn.layers if l[0] == "BATCHNORM")
    buf = torch.zeros(2 * cmax + 2, dtype=torch.float64, device=env.ctx.device)
    iM, io = env.inputs(dn, M), env.inputs(dn, odd)
    fb(env, dn, iM)
    env.ctx.check(lib.fg_net_set_sync_bn(dn.h, 1, buf.data_ptr(), buf.numel()))
    rc = forward_rc(dn, io)
    if rc != FG_PAUSED_SYNC:
        msgs.append("the forward did not pause at the first BatchNorm (rc %d)" % rc)
    rc = backward_rc(dn, io, 3, new_gx(env, io))
    if rc != FG_ERR_INVALID:
        msgs.append("a backward behind a paused, unfinished forward returned %d" % rc)
    env.ctx.check(lib.fg_net_set_sync_bn(dn.h, 0, None, 0))            # the pause is dropped
    check(env, dn, iM, "probe after an abandoned paused forward", msgs)
    env.ctx.check(lib.fg_net_set_sync_bn(dn.h, 1, buf.data_ptr(), buf.numel()))
    rc = forward_rc(dn, io)
    while rc == FG_PAUSED_SYNC:                                         # one rank: the local sums are the global ones
        rc = dn._forward_resume()
    env.ctx.check(rc)
    rc = backward_rc(dn, io, 3, new_gx(env, io))
    if rc != FG_PAUSED_SYNC:
        msgs.append("the backward did not pause at the last BatchNorm (rc %d)" % rc)
    env.ctx.check(lib.fg_net_set_sync_bn(dn.h, 0, None, 0))
    if lib.fg_net_forward_resume(dn.h, None) != FG_ERR_INVALID:
        msgs.append("fg_net_forward_resume accepted while a BACKWARD is paused")
    check(env, dn, iM, "probe after an abandoned paused backward", msgs)
    if lib.fg_net_backward_resume(dn.h) != FG_ERR_INVALID:
        msgs.append("fg_net_backward_resume accepted after a fresh forward + backward")
    return msgs


ALL_KINDS = tuple(KINDS)
NET_SCENARIOS = [("batch_history", s01_batch_history, ALL_KINDS), ("mode_history", s02_mode_history, ALL_KINDS),
                 ("repeated_backward", s03_repeated_backward, ALL_KINDS), ("split_flags", s04_split_flags, ALL_KINDS),
                 ("ranged_backward", s05_ranged_backward, ALL_KINDS), ("math_mode", s06_math_mode, ALL_KINDS),
                 ("fusion_word", s07_fusion_word, ALL_KINDS), ("params_moved", s08_params_moved, ALL_KINDS),
                 ("forward_to", s09_forward_to, ALL_KINDS), ("abandoned_pause", s10_abandoned_pause, ("G32",))]


# ---- gan and sampler ---------------------------------------------------------------------------------------------------------------
class _FillFirst:
    """the library as `owner` sees it: its fg_*_create entry fills owner.ws with NaN first -- behind the allocation, in front of whatever
    the C object initialises for itself.  Nothing else is touched (no torch function is replaced)."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in ("fg_gan_create", "fg_sampler_create"):
            return f

        def create(*a):
            self._owner.ws.fill_(NAN)
            return f(*a)
        return create


def _poisoned(cls):
    """FusedGan / Sampler whose own workspace holds NaN before the C object is created"""
    class Poisoned(cls):
        lib = property(lambda self: self._fill_first, lambda self, lib: setattr(self, "_fill_first", _FillFirst(lib, self)))
    return Poisoned


ADAM = ("adam", {})
SGD_MOM = ("sgd", dict(learningRate=0.01, momentum=0.5, learningRateDecay=1e-3))
ADAGRAD = ("adagrad", dict(learningRate=0.01, learningRateDecay=0.05))


class Rig:
    def __init__(self, env, pair, opt=ADAM, nets=None):
        from face_generator_amd.runtime import FusedGan
        kG, kD, self.table, self.B = PAIRS[pair]
        self.env, self.pair = env, pair
        self.dnG, self.dnD = nets or (env.net(kG), env.net(kD))
        self.gan = FusedGan(env.ctx, self.dnG, self.dnD, self.table, self.B)
        self.opt = [opt, opt]
        for w in (0, 1):
            self.gan.set_optimizer(w, *opt)
        self.gan.set_penalty(0, 1e-5, 1e-4, 1.0)
        self.gan.set_penalty(1, 0.0, 1e-5, 5.0)
        self.gan.set_seeds(3, 0, 777, 0)

    def set_optimizer(self, w, opt):
        self.opt[w] = opt
        self.gan.set_optimizer(w, *opt)

    def twin(self):
        """fresh nets and a fresh gan restored from this one: vectors, optimizer configuration, state and step counts"""
        env = self.env
        t = Rig.__new__(Rig)
        from face_generator_amd.runtime import FusedGan
        t.env, t.pair, t.table, t.B = env, self.pair, self.table, self.B
        t.dnG, t.dnD = env.twin(self.dnG), env.twin(self.dnD)
        t.gan = _poisoned(FusedGan)(env.ctx, t.dnG, t.dnD, t.table, t.B)
        t.opt = list(self.opt)
        for w in (0, 1):
            t.gan.set_optimizer(w, *t.opt[w])
            t.gan.view("OPT_STATE_" + "DG"[w]).copy_(self.gan.view("OPT_STATE_" + "DG"[w]))
            env.ctx.check(env.lib.fg_gan_set_optimizer_steps(t.gan.h, w, self.gan.steps(w)))
        t.gan.set_penalty(0, 1e-5, 1e-4, 1.0)
        t.gan.set_penalty(1, 0.0, 1e-5, 5.0)
        t.gan.set_seeds(3, 0, 777, 0)
        return t

    def _masks(self, B, seed):
        lib, dn = self.env.lib, self.dnD
        return [self.env.ctx.bernoulli((lib.fg_net_mask_elems(dn.h, i, B),), lib.fg_net_mask_keep(dn.h, i), seed=seed + i) for i in range(dn.n_masks)]

    def step_D(self, it, B=None, flags=0, noise=True):
        B, u = B or self.B, self.env.ctx.uniform
        S, C = self.dnD.in_h, self.dnD.in_c
        real = u((B // 2, S, S, C), -1.0 if self.table else 0.0, 1.0, seed=100 + it)
        cr, cf = (u((B // 2, S, S, C), 0.0, 1.0, seed=110 + it), u((B // 2, S, S, C), 0.0, 1.0, seed=120 + it)) if self.table else (None, None)
        nz = u((B // 2, S, S, 1) if self.table else (B // 2, self.dnG.in_c), -1.0, 1.0, seed=130 + it) if noise else None
        self.gan.step_D(B, real, cr, cf, nz, self._masks(B, 1600 + 10 * it), flags)
        return self.results(B, "D", gated=bool(flags & 1))

    def step_G(self, it, B=None, flags=0, noise=True):
        B, u = B or self.B, self.env.ctx.uniform
        S, C = self.dnD.in_h, self.dnD.in_c
        cond = u((B, S, S, C), 0.0, 1.0, seed=140 + it) if self.table else None
        nz = u((B, S, S, 1) if self.table else (B, self.dnG.in_c), -1.0, 1.0, seed=150 + it) if noise else None
        self.gan.step_G(B, cond, nz, self._masks(B, 1700 + 10 * it), flags)
        return self.results(B, "G")

    def results(self, B, which, gated=False):
        g, img = self.gan, B * self.dnD.in_c * self.dnD.in_h * self.dnD.in_w
        res = dict(pD=self.dnD.params, pG=self.dnG.params, gD=self.dnD.grads, gG=self.dnG.grads, bnD=self.dnD.buffers, bnG=self.dnG.buffers,
                   optD=g.view("OPT_STATE_D"), optG=g.view("OPT_STATE_G"), d_output=g.view("D_OUTPUT", B),
                   steps=torch.tensor([g.steps(0), g.steps(1)], dtype=torch.int32))
        if which == "D":
            # int[4..7], the counts of the global batch, are the gate's: only a FG_STEP_NO_UPDATE step writes them (facegen_hip.h)
            res.update(loss=g.view("LOSS")[0:1], confusion=g.view("CONFUSION").view(torch.int32)[:8 if gated else 4])
        else:
            res.update(loss=g.view("LOSS")[1:2], samples=g.view("D_INPUT", img), d_grad_input=g.view("D_GRAD_INPUT", img))
        return {k: v.clone() for k, v in res.items()}


def both(env, used, twin, tag, msgs, fn):
    with env.probe("used", tag):
        ru = fn(used)
    with env.probe("twin", tag):
        rt = fn(twin)
    msgs += diff(tag, ru, rt)
    return ru, rt


def g11_no_update(env, pair):
    msgs, r = [], Rig(env, pair)
    r.step_D(0); r.step_G(0)
    p0 = r.dnD.params.clone()
    r.step_D(1, flags=1)                                                # the gate said no: never updated
    if r.gan.steps(0) != 1 or not torch.equal(bits(p0), bits(r.dnD.params)):
        msgs.append("a FG_STEP_NO_UPDATE step moved D's parameters or its step count")
    t = r.twin()
    both(env, r, t, "a normal D-step after a FG_STEP_NO_UPDATE step that was never applied", msgs, lambda g: g.step_D(2))
    if r.gan.steps(0) != 2:
        msgs.append("the step count after the update is %d, not 2" % r.gan.steps(0))
    rc = env.lib.fg_gan_update(r.gan.h, 0)
    if rc != FG_ERR_INVALID:
        msgs.append("fg_gan_update(D) behind a step that consumed the gradients returned %d" % rc)
    # the update issued after an intervening G-step
    t = r.twin()
    r.step_D(3, flags=1); t.step_D(3, flags=1)
    r.step_G(3)
    with env.probe("used", "fg_gan_update(D) after a G-step"):
        r.gan.update(0)
    with env.probe("twin", "fg_gan_update(D) after a G-step"):
        t.gan.update(0)
    keys = ("pD", "optD", "gD", "bnD")
    msgs += diff("fg_gan_update(D) after an intervening G-step", r.results(r.B, "D"), t.results(t.B, "D"), keys=keys)
    if (r.gan.steps(0), t.gan.steps(0)) != (3, 3):
        msgs.append("step counts %d / %d, not 3" % (r.gan.steps(0), t.gan.steps(0)))
    return msgs


def g12_save_restore(env, pair):
    msgs = []
    for opt in (ADAM, SGD_MOM, ADAGRAD):
        r = Rig(env, pair, opt)
        for it in range(2):
            r.step_D(it); r.step_G(it)
        t = r.twin()                                                    # = save + restore into fresh objects
        if (t.gan.steps(0), t.gan.steps(1)) != (2, 2):
            msgs.append("%s: fg_gan_set_optimizer_steps left %d / %d" % (opt[0], t.gan.steps(0), t.gan.steps(1)))
        both(env, r, t, "%s: D-step of iteration three" % opt[0], msgs, lambda g: g.step_D(2))
        both(env, r, t, "%s: G-step of iteration three" % opt[0], msgs, lambda g: g.step_G(2))
    return msgs


def g13_set_optimizer_midrun(env, pair):
    msgs, r = [], Rig(env, pair)
    for it in range(2):
        r.step_D(it); r.step_G(it)
    # the same rule with other hyper-parameters: state and step count stay
    before = r.gan.view("OPT_STATE_G").clone()
    r.set_optimizer(1, ("adam", dict(learningRate=2e-3, beta1=0.5)))
    if r.gan.steps(1) != 2 or not torch.equal(bits(before), bits(r.gan.view("OPT_STATE_G"))):
        msgs.append("fg_gan_set_optimizer with the same rule touched the state or the step count")
    # another rule: state zeroed, step count 0, SGD's first-step rule armed again
    r.set_optimizer(0, SGD_MOM)
    if r.gan.steps(0) != 0:
        msgs.append("fg_gan_set_optimizer to another rule left the step count at %d" % r.gan.steps(0))
    if not env.ctx.dry and bool((bits(r.gan.view("OPT_STATE_D")) != 0).any()):
        msgs.append("fg_gan_set_optimizer to another rule left optimizer state behind")
    t = r.twin()
    both(env, r, t, "D-step after the change of rule", msgs, lambda g: g.step_D(2))
    both(env, r, t, "G-step after the change of hyper-parameters", msgs, lambda g: g.step_G(2))
    both(env, r, t, "the second D-step of the new rule", msgs, lambda g: g.step_D(3))
    return msgs


def g14_tail_batch(env, pair):
    msgs, r = [], Rig(env, pair)
    B, Bt = r.B, r.B // 2
    r.step_D(0); r.step_G(0)
    t = r.twin()
    both(env, r, t, "D-step at the tail batch %d after steps at %d" % (Bt, B), msgs, lambda g: g.step_D(1, B=Bt))
    both(env, r, t, "G-step at the tail batch", msgs, lambda g: g.step_G(1, B=Bt))
    both(env, r, t, "and at the full batch again", msgs, lambda g: g.step_D(2))
    # library-drawn noise behind that history: fg_rng_uniform(seed, offset) with the offset advanced by ceil(count / 4) per draw
    nz = r.dnG.in_h * r.dnG.in_w if r.table else r.dnG.in_c
    r.gan.set_seeds(91, 0, 777, 0)
    r.step_D(3, noise=False); r.step_G(3, noise=False); r.step_D(4, B=Bt, noise=False)
    off = (B // 2 * nz + 3) // 4 + (B * nz + 3) // 4
    want = env.ctx.uniform((Bt // 2 * nz,), -1.0, 1.0, seed=91, offset=off)
    msgs += diff("library-drawn noise of the third closure", dict(noise=r.gan.view("NOISE", Bt // 2 * nz).clone()), dict(noise=want))
    return msgs


def g15_sampler_between_steps(env, pair):
    from face_generator_amd.runtime import Sampler
    msgs, r = [], Rig(env, pair)
    N, chunk = 14, 6                                                    # two chunks and a tail of 2
    s = Sampler(env.ctx, r.dnG, r.dnD, N, chunk)
    r.step_D(0); r.step_G(0); r.step_D(1)
    t = r.twin()
    noise = env.ctx.uniform((N, r.dnG.in_c), -1.0, 1.0, seed=55)
    ts = _poisoned(Sampler)(env.ctx, env.twin(r.dnG), env.twin(r.dnD), N, chunk)

    def run(smp):
        smp.sample(N, noise)
        return {k: smp.view(k).clone() for k in ("IMAGES", "PREDS", "ORDER_DESC", "ORDER_ASC")}
    with env.probe("used", "fg_sample on nets in training"):
        ru = run(s)
    with env.probe("twin", "fg_sample on nets in training"):
        rt = run(ts)
    msgs += diff("fg_sample between a D-step and a G-step", ru, rt)
    both(env, r, t, "G-step behind the sampler", msgs, lambda g: g.step_G(1))
    both(env, r, t, "the next D-step", msgs, lambda g: g.step_D(2))
    s.set_seed(7, 0); ts.set_seed(7, 0)
    r.step_G(2)

    def drawn(smp):
        smp.sample(N)
        return {k: smp.view(k).clone() for k in ("NOISE", "IMAGES", "PREDS", "ORDER_DESC")}
    ts2 = _poisoned(Sampler)(env.ctx, env.twin(r.dnG), env.twin(r.dnD), N, chunk)
    ts2.set_seed(7, 0)
    msgs += diff("fg_sample with drawn noise, an epoch later", drawn(s), drawn(ts2))
    return msgs


OPT_MOVES = [(mode, cf, name, opt, word) for mode, cf in ((0, None), (6, NO_WINO))
             for name, opt, word in (("Adam with FG_FUSE_ADAM_PACK", ADAM, FG_FUSE_ADAM_PACK), ("Adam without FG_FUSE_ADAM_PACK", ADAM, 0),
                                     ("SGD with momentum", SGD_MOM, 0), ("Adagrad", ADAGRAD, 0))]


def g08_optimizer_moves(env, pair, cases=None):
    """scenario 8, the optimizer's moves: after fg_gan_update the nets alone equal twins bound to copies of the vectors"""
    msgs = []
    kG, kD, _, B = PAIRS[pair]
    for mode, cf, name, opt, word in (OPT_MOVES if cases is None else [OPT_MOVES[i] for i in cases]):
        base = (FG_FUSE_DEFAULT if cf is None else cf) | word
        with env.fusion(base), env.math(mode):
            r = Rig(env, pair, opt, nets=(env.net(kG, base), env.net(kD, base)))
            # (at max_batch: the only size at which a contraction of these nets reads the bf16x6 planes of its weights)
            iG, iD = env.inputs(r.dnG, KINDS[kG][0], 7), env.inputs(r.dnD, KINDS[kD][0], 7)
            for it in range(2):
                r.step_D(it, flags=1)
                env.say("update D %s" % name)
                r.gan.update(0)
                env.say("update end")
                check(env, r.dnD, iD, "math %d, %s: D alone after update %d" % (mode, name, it), msgs)
                r.step_G(it, flags=1)
                env.say("update G %s" % name)
                r.gan.update(1)
                env.say("update end")
                check(env, r.dnG, iG, "math %d, %s: G alone after update %d" % (mode, name, it), msgs)
    return msgs


GAN_SCENARIOS = [("no_update", g11_no_update, ("px32", "c2f")), ("save_restore", g12_save_restore, ("px32", "c2f")),
                 ("set_optimizer_midrun", g13_set_optimizer_midrun, ("px32", "c2f")), ("tail_batch", g14_tail_batch, ("px32", "c2f")),
                 ("sampler_between_steps", g15_sampler_between_steps, ("px32",)), ("optimizer_moves", g08_optimizer_moves, ("px32", "c2f"))]


# ---- return codes (host) ------------------------------------------------------------------------------------------------------------
def return_codes(env):
    """-> {name: return code}; every one of them must be FG_ERR_INVALID unless the name says otherwise"""
    lib, out = env.lib, {}
    dn = env.net("G32")
    M, odd = KINDS["G32"]
    iM, io = env.inputs(dn, M), env.inputs(dn, odd)
    ns = lib.fg_net_num_stages(dn.h)
    out["backward before any forward"] = backward_rc(dn, iM, 3, new_gx(env, iM), batch=M)
    fb(env, dn, iM)
    out["fg_net_forward_resume, not paused"] = lib.fg_net_forward_resume(dn.h, None)
    out["fg_net_backward_resume, not paused"] = lib.fg_net_backward_resume(dn.h)
    out["fg_net_backward_range out of order"] = backward_rc(dn, iM, 3, new_gx(env, iM), ns - 3, 0)
    env.ctx.check(backward_rc(dn, iM, 3, new_gx(env, iM), ns - 1, ns - 2))
    out["fg_net_backward_range skipping a stage"] = backward_rc(dn, iM, 3, new_gx(env, iM), ns - 4, 0)
    out["fg_net_backward_range repeating a stage"] = backward_rc(dn, iM, 3, new_gx(env, iM), ns - 2, 0)
    env.ctx.check(forward_rc(dn, iM))
    out["fg_net_backward_range continuing a range across a fresh forward"] = backward_rc(dn, iM, 3, new_gx(env, iM), ns - 3, 0)
    out["backward at another batch"] = backward_rc(dn, io, 3, new_gx(env, io), batch=odd)
    env.ctx.check(forward_rc(dn, io, train=False))
    out["backward after an evaluate forward"] = backward_rc(dn, io, 3, new_gx(env, io))
    # the refused forward: the plan of the refused call must not stand in for a forward that never ran
    fb(env, dn, iM)
    off = ctypes.c_longlong()
    out["FG_ERR_WORKSPACE: forward into a workspace of 4096 bytes"] = lib.fg_net_forward(dn.h, odd, io.x.data_ptr(), dn.ws.data_ptr(), 4096, 1, None, 0, ctypes.byref(off))
    out["backward at the batch of a forward refused for its workspace"] = backward_rc(dn, io, 3, new_gx(env, io), batch=odd)
    out["backward_range at the batch of a forward refused for its workspace"] = backward_rc(dn, io, 3, new_gx(env, io), ns - 1, ns - 1, batch=odd)
    out["backward at the batch of the last SUCCESSFUL forward, behind the refused one"] = backward_rc(dn, iM, 3, new_gx(env, iM), batch=M)
    env.ctx.check(forward_rc(dn, io))
    out["FG_OK: backward once a forward succeeded"] = backward_rc(dn, io, 3, new_gx(env, io))
    out["FG_ERR_INVALID: forward refused for batch 0"] = lib.fg_net_forward(dn.h, 0, io.x.data_ptr(), dn.ws.data_ptr(), dn.ws.numel() * 4, 1, None, 0, ctypes.byref(off))
    out["backward behind a forward refused for its batch"] = backward_rc(dn, io, 3, new_gx(env, io))
    dD = env.net("D32")
    iD = env.inputs(dD, 3)
    fb(env, dD, iD)
    out["FG_ERR_INVALID: train forward without its dropout masks"] = lib.fg_net_forward(dD.h, 3, iD.x.data_ptr(), dD.ws.data_ptr(), dD.ws.numel() * 4, 1, None, 0, ctypes.byref(off))
    out["backward behind a forward refused for its masks"] = backward_rc(dD, iD, 3, new_gx(env, iD))
    # a refused forward abandons a paused pass like any other: make_plan has published ITS batch, no _resume may run over that plan
    dn = env.net("G32")
    buf = torch.zeros(2 * max(l[1] for l in dn.layers if l[0] == "BATCHNORM") + 2, dtype=torch.float64, device=env.ctx.device)
    env.ctx.check(lib.fg_net_set_sync_bn(dn.h, 1, buf.data_ptr(), buf.numel()))
    refused = lambda: lib.fg_net_forward(dn.h, odd, io.x.data_ptr(), dn.ws.data_ptr(), 4096, 1, None, 0, ctypes.byref(off))
    out["FG_PAUSED_SYNC: a forward with sync-BN pauses at the first BatchNorm"] = forward_rc(dn, iM)
    out["FG_ERR_WORKSPACE: a refused forward behind the paused forward"] = refused()
    out["fg_net_forward_resume behind a refused forward that followed the paused one"] = lib.fg_net_forward_resume(dn.h, None)
    rc = forward_rc(dn, iM)
    while rc == FG_PAUSED_SYNC:
        rc = dn._forward_resume()
    env.ctx.check(rc)
    out["FG_PAUSED_SYNC: a backward with sync-BN pauses at the last BatchNorm"] = backward_rc(dn, iM, 3, new_gx(env, iM))
    out["FG_ERR_WORKSPACE: a refused forward behind the paused backward"] = refused()
    out["fg_net_backward_resume behind a refused forward that followed the paused backward"] = lib.fg_net_backward_resume(dn.h)
    env.ctx.check(lib.fg_net_set_sync_bn(dn.h, 0, None, 0))
    r = Rig(env, "px32")
    out["fg_gan_update(D), nothing pending"] = lib.fg_gan_update(r.gan.h, 0)
    out["fg_gan_update(G), nothing pending"] = lib.fg_gan_update(r.gan.h, 1)
    r.step_D(0, flags=1)
    out["FG_OK: fg_gan_update(D) behind a FG_STEP_NO_UPDATE step"] = lib.fg_gan_update(r.gan.h, 0)
    out["fg_gan_update(D) a second time"] = lib.fg_gan_update(r.gan.h, 0)
    r.step_D(1, flags=1); r.step_D(2)
    out["fg_gan_update(D) behind a normal step that overwrote the held gradients"] = lib.fg_gan_update(r.gan.h, 0)
    # refused steps: the codes, and the offsets of the random streams behind them (noise and masks NULL: the library draws)
    r = Rig(env, "px32")
    g, real = r.gan, env.ctx.uniform((r.B // 2, r.dnD.in_h, r.dnD.in_w, r.dnD.in_c), 0.0, 1.0, seed=9)
    g._bind()
    D = lambda B, x=real: lib.fg_step_D(g.h, B, x.data_ptr() if x is not None else None, None, None, None, None, 0)
    G = lambda B: lib.fg_step_G(g.h, B, None, None, None, 0)

    def offsets():
        a, b = ctypes.c_longlong(), ctypes.c_longlong()
        env.ctx.check(lib.fg_gan_get_offsets(g.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value
    env.ctx.check(D(r.B)); env.ctx.check(G(r.B))
    before = offsets()
    out["fg_step_D at an odd batch"] = D(r.B - 1)
    out["fg_step_G above max_batch"] = G(r.B + 2)
    out["fg_step_D with a null real"] = D(r.B, None)
    key = g._bound
    env.ctx.check(lib.fg_gan_bind_workspaces(g.h, key[0], key[1] * 4, key[2], 4096))
    out["FG_ERR_WORKSPACE: fg_step_D behind its draw, D's workspace bound too small"] = D(r.B)
    out["FG_ERR_WORKSPACE: fg_step_G behind its draw, D's workspace bound too small"] = G(r.B)
    env.ctx.check(lib.fg_gan_bind_workspaces(g.h, *[k * (4 if i % 2 else 1) for i, k in enumerate(key)]))
    out["FG_OK: the offsets of the random streams behind five refused steps are those in front of them"] = 0 if (offsets() == before and before[0] > 0 and before[1] > 0) else -1
    out["FG_OK: fg_step_D once its workspaces are bound again"] = D(r.B)
    return out


# ---- the ledger ----------------------------------------------------------------------------------------------------------------------
STRUCTS = [("net.hip", "Stage"), ("net.hip", "fg_net"), ("step.hip", "OptCfg"), ("step.hip", "fg_gan"), ("sample.hip", "fg_sampler")]


def struct_fields(fn, name):
    """the member names of `struct name` in csrc/fn"""
    import re
    t = open(os.path.join(ROOT, "face_generator_amd", "csrc", fn)).read()
    i = t.index("struct %s {" % name)
    body = re.sub(r"//[^\n]*", "", t[i:t.index("\n};", i)].split("{", 1)[1])
    out = []
    for stmt in body.split(";"):
        stmt = re.sub(r"<[^>]*>", "", re.sub(r"=[^,]*", "", re.sub(r"\{[^}]*\}", "", stmt.strip())))
        out += re.findall(r"[\*\s,]([A-Za-z_]\w*)\s*(?:\[[^\]]*\])*\s*(?=,|$)", " " + stmt) if stmt else []
    return out


def host_main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from face_generator_amd.runtime import get_context
    global DRY
    DRY = True
    only = sys.argv[2:]                                                  # scenario names (default: all)
    env = Env(get_context(-1), sys.stderr)
    for name, fn, kinds in NET_SCENARIOS + GAN_SCENARIOS:
        if only and name not in only:
            continue
        for k in kinds:
            env.say("scenario %s %s" % (name, k))
            for m in fn(env, k):
                env.say("mismatch " + m)
    if not only or "return_codes" in only:
        env.say("scenario return_codes -")
        for name, rc in return_codes(env).items():
            env.say("rc %d %s" % (rc, name))
    env.say("done")


if __name__ == "__main__":
    host_main()
