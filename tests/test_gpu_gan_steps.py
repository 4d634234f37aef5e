"""The step level (fg_gan_create, fg_step_D, fg_step_G, fg_gan_update, gan_optimize of csrc/step.hip) on small G / D pairs off the
models' shapes: GAN_CASES of tests/gan_cases.py, each against the float64 oracle of the same pair (oracle.torch7_nn.step_D / step_G /
step_D_c2f / step_G_c2f).  tests/GAN_STEPS.md has the table of decisions and case names.

Per closure, from the device's own parameters, running statistics, optimizer state and step count: the samples and D's outputs (1e-5),
the BCE loss (1e-5 relative), the confusion counts (exact), the raw flat gradient read behind the step (gpu_util.assert_net_bars per
parameter tensor, the oracle on the device's PReLU decisions, at most max(1, 1e-5 of the units) of them differing from its own), D's
input gradient in a G-step, the BatchNorm running statistics of both nets, the noise and masks the library drew (bit for bit against
fg_rng_uniform / fg_rng_bernoulli at the documented offsets, and fed to the oracle) -- and, separately from the gradient, the UPDATE:
the case's interruptable_* rule of the oracle in float64 with the penalty and clamp of feval_D / feval_G_on_D, applied to the device's
own gradient, parameters, state and step count, must give the device's parameters and FG_GAN_OPT_STATE_* behind the step, at the bars
tests/test_gpu_pointwise_paths.py holds the same kernels to.  The net that is not stepped keeps its parameters, state and step count
bit for bit.  Every case runs with every vector of both nets and all three workspaces in the guarded arena of tests/mem_contract.py,
each exactly as long as its size function states, the workspaces full of NaN before the step object is created."""
import ctypes

import numpy as np
import pytest
import torch

import gan_cases as GC
import net_cases as NC
import sync_cases as SC
from gpu_util import close, dev, assert_net_bars, BAR
from mem_contract import Arena

pytestmark = pytest.mark.gpu

# bars of the optimizer rows of tests/test_gpu_pointwise_paths.py (run_opt): {rule: ((p atol, p rtol), [(state part, atol, rtol)])}
OPT_BARS = dict(adam=((2e-7, 2e-7), [("m", 1e-7, 1e-5), ("v", 1e-12, 1e-5)]), sgd=((1e-5, 0.0), [("momentum buffer", 1e-5, 0.0)]),
                adagrad=((1e-6, 0.0), [("variance", 0.0, 1e-5)]))
# cases that take the fallback bar of GAN_STEPS.md ("Measured bars"): empty -- every case meets the bars above
FALLBACK = {}


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    c.set_math(0); c.set_fusion(503)
    return c


@pytest.fixture(scope="module")
def comm(ctx):
    """a real one-rank communicator (fg_comm_create, as tests/test_gpu_dist.py makes it)"""
    buf, h = ctypes.create_string_buffer(128), ctypes.c_void_p()
    rc = ctx.lib.fg_comm_unique_id(ctx.h, buf, 128)
    if rc == -4:
        pytest.skip("RCCL cannot be bound: " + ctx.lib.fg_last_error(ctx.h).decode())
    ctx.check(rc)
    ctx.check(ctx.lib.fg_comm_create(ctx.h, buf.raw, 128, 0, 1, ctypes.byref(h)))
    yield h
    torch.cuda.synchronize()
    ctx.check(ctx.lib.fg_comm_destroy(h))


def inner(net):
    return getattr(net, "inner", net)


def bn_modules(net):
    from oracle import torch7_nn as O
    return [m for m in O.walk_modules(inner(net)) if isinstance(m, O.SpatialBatchNormalization)]


def load(st, gan):
    """the oracle's parameters and running statistics -> the device"""
    for dn, p, net in ((gan.dnG, st.pG, st.G), (gan.dnD, st.pD, st.D)):
        dn.params.copy_(torch.from_numpy(p.astype(np.float32)))
        if bn_modules(net):
            dn.buffers.copy_(torch.from_numpy(np.concatenate([np.concatenate([m.running_mean, m.running_var]) for m in bn_modules(net)]).astype(np.float32)))
        dn.params_changed()


def sync(st, gan):
    """the device's parameters and running statistics -> the oracle"""
    for dn, p, net in ((gan.dnG, st.pG, st.G), (gan.dnD, st.pD, st.D)):
        p[...] = dn.params.cpu().numpy()
        b, off = dn.buffers.cpu().numpy(), 0
        for m in bn_modules(net):
            m.running_mean[...] = b[off:off + m.nf]; m.running_var[...] = b[off + m.nf:off + 2 * m.nf]
            off += 2 * m.nf


def check_bn(what, st, gan):
    for dn, net in ((gan.dnG, st.G), (gan.dnD, st.D)):
        b, off = dn.buffers.cpu().numpy(), 0
        for m in bn_modules(net):
            close(b[off:off + m.nf], m.running_mean, atol=BAR["bn_running_mean"], what=what + " running_mean")
            close(b[off + m.nf:off + 2 * m.nf], m.running_var, atol=0.0, rtol=BAR["bn_running_var_rtol"], what=what + " running_var")
            off += 2 * m.nf


class Operands:
    """the device operands of a case, views of the arena sized for max_batch; a closure at a smaller batch uses their heads"""

    def __init__(self, ctx, case, ar, gan):
        M, img = case.max_batch, int(np.prod(case.ddims))
        nz = int(np.prod(GC.noise_shape(case, 1)))
        t = lambda n, name: ar.take(max(1, n), name=name)
        self.real, self.noise = t(M // 2 * img, "real"), t(M * nz, "noise")
        self.cond_real, self.cond_fake, self.cond = (t(M // 2 * img, "cond_real"), t(M // 2 * img, "cond_fake"), t(M * img, "cond")) if case.table else (None, None, None)
        self.masks = [t(ctx.lib.fg_net_mask_elems(gan.dnD.h, i, M), "mask%d" % i) for i in range(gan.dnD.n_masks)]
        self.case, self.first = case, NC.walk(case.dlayers, case.ddims)[0]

    @staticmethod
    def sizes(ctx, case, dnD_masks):
        M, img = case.max_batch, int(np.prod(case.ddims))
        nz = int(np.prod(GC.noise_shape(case, 1)))
        return [M // 2 * img, M * nz] + ([M // 2 * img, M // 2 * img, M * img] if case.table else []) + dnD_masks

    def put(self, view, a, out=None):
        """oracle-shaped numpy -> the head of a view, in the device's layout"""
        a = NC.to_device(a, out) if out is not None else a
        v = view[:a.size]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1))
        return v

    def image(self, view, a):
        return self.put(view, a, self.first)

    def noise_in(self, a):
        return self.put(self.noise, a.transpose(0, 2, 3, 1) if self.case.table else a)


def mask_sizes(ctx, case):
    dn = NC.device_net(ctx, case.dlayers, case.ddims, 2)
    return [ctx.lib.fg_net_mask_elems(dn.h, i, case.max_batch) for i in range(dn.n_masks)]


def oracle_masks(case, dev_masks, B):
    """what the library drew, in the oracle's shapes (the reverse of net_cases.device_masks)"""
    first, outs = NC.walk(case.dlayers, case.ddims)
    it, res = iter(dev_masks), []
    for i, l in enumerate(case.dlayers):
        if l[0] == "SPATIAL_DROPOUT":
            res.append(next(it).reshape(B, outs[i].chw[0]))
        elif l[0] == "DROPOUT":
            res.append(NC.from_device(next(it).reshape(B, -1), outs[i]))
    return res


class Run:
    """one case on the device and in the oracle, closure by closure"""

    def __init__(self, ctx, case, comm=None, arena=True, sync_bn=0, overlap=None, gscale=1.0):
        """sync_bn, overlap: what fg_gan_set_comm gets beside `comm` (overlap: default the case's own); gscale: the 1 / world by which
        gan_optimize scales the gradient in front of penalty and clamp (fg_prep_grad) -- check_update applies it to the device's raw
        gradient in the same place"""
        self.ctx, self.case = ctx, case
        self.overlap, self.gscale = (case.overlap if overlap is None else overlap), gscale
        self.st = GC.oracle_gan(case, np.float64)
        self.real_opt = self.st.opt
        self.raw_opt = dict(self.st.opt, D_L1=0.0, D_L2=0.0, G_L1=0.0, G_L2=0.0, D_clamp=0.0, G_clamp=0.0)
        self.ar = Arena.sized(ctx.device, GC.arena_sizes(ctx, case) + Operands.sizes(ctx, case, mask_sizes(ctx, case))) if arena else None
        self.gan = GC.device_gan(ctx, case, self.ar)
        if arena:
            self.op = Operands(ctx, case, self.ar, self.gan)
        load(self.st, self.gan)
        if arena:
            self.gan.dnG.ws.fill_(float("nan")); self.gan.dnD.ws.fill_(float("nan"))
        if self.overlap is not None and comm is not None:
            ctx.check(ctx.lib.fg_gan_set_comm(self.gan.h, comm, sync_bn, self.overlap))
        self.noise_off, self.mask_off = 0, 0
        self.held = None
        self.global_conf = [0, 0, 0, 0]

    def guards(self, what):
        torch.cuda.synchronize()
        self.ar.assert_guards(what)
        for dn in (self.gan.dnG, self.gan.dnD):
            assert bool(torch.isfinite(dn.params).all()), what + ": parameters are not finite"

    def closure(self, it, which):
        ctx, case, gan, st, op = self.ctx, self.case, self.gan, self.st, self.op
        from oracle import torch7_nn as O
        inp = GC.inputs(case, it)
        B, w = inp["B"], "DG".index(which)
        h = B // 2
        rows = h if which == "D" else B
        what = "%s iteration %d %s-step at B = %d" % (case.name, it, which, B)
        dn, other = (gan.dnD, gan.dnG) if which == "D" else (gan.dnG, gan.dnD)
        sync(st, gan)
        p0, s0, t0 = dn.params.clone(), gan.view("OPT_STATE_" + which).clone(), gan.steps(w)
        o0, os0, ot0 = other.params.clone(), gan.view("OPT_STATE_" + "GD"[w]).clone(), gan.steps(1 - w)
        explicit = case.masks == "explicit"
        gate = case.gate[which][it] if case.gate else None
        flags = gan.NO_UPDATE if case.gate else 0
        nz = op.noise_in(inp["noise" + which]) if explicit else None
        md = [op.put(v, m) for v, m in zip(op.masks, NC.device_masks(case.dlayers, case.ddims, inp["masks" + which]))] if explicit else None
        # ---- the device ---------------------------------------------------------------------------------------------------------
        if which == "D":
            cr, cf = (op.image(op.cond_real, inp["cond_real"]), op.image(op.cond_fake, inp["cond_fake"])) if case.table else (None, None)
            gan.step_D(B, op.image(op.real, inp["real"]), cr, cf, nz, md, flags)
        else:
            gan.step_G(B, op.image(op.cond, inp["cond"]) if case.table else None, nz, md, flags)
        if self.overlap:
            gan.finish_pending()               # D's deferred update lands here, inside the closure that formed its gradient
        self.guards(what)
        # ---- what the library drew: the documented streams, then the oracle's inputs ------------------------------------------------
        noise_o, masks_o = inp["noise" + which], inp["masks" + which]
        if not explicit:
            n = rows * int(np.prod(GC.noise_shape(case, 1)))
            got = gan.view("NOISE", n)
            assert torch.equal(got, ctx.uniform((n,), -1.0, 1.0, 3 + case.seed, self.noise_off)), what + ": the noise is not fg_rng_uniform at offset %d" % self.noise_off
            self.noise_off += (n + 3) // 4
            noise_o = got.cpu().numpy().reshape(GC.noise_shape(case, rows))
            dm = []
            for i in range(gan.n_masks):
                m = gan.mask_view(i, B)
                keep = ctx.lib.fg_net_mask_keep(gan.dnD.h, i)
                assert torch.equal(m, ctx.bernoulli((m.numel(),), keep, 777 + case.seed, self.mask_off)), what + ": mask %d is not fg_rng_bernoulli at offset %d" % (i, self.mask_off)
                self.mask_off += (m.numel() + 3) // 4
                dm.append(m.cpu().numpy())
            masks_o = oracle_masks(case, dm, B)
        # ---- the oracle on the device's PReLU decisions, raw gradient (no penalty, no clamp) -------------------------------------------
        gm, dmods = st.mods
        img = int(np.prod(case.ddims))
        d_input = NC.from_device(gan.view("D_INPUT", B * img).cpu().numpy().reshape(B, -1), op.first)
        if case.table:
            cond = np.concatenate([inp["cond_real"], inp["cond_fake"]]) if which == "D" else inp["cond"]
            xD = (np.concatenate([inp["real"], d_input[h:]]) if which == "D" else d_input) + cond
        else:
            xD = d_input
        NC.adopt(ctx, gan.dnD, case.dlayers, case.ddims, dmods, xD.astype(np.float32), p0.cpu().numpy() if which == "D" else o0.cpu().numpy())
        if which == "G":
            xG = np.concatenate([noise_o, inp["cond"]], 1) if case.table else noise_o
            NC.adopt(ctx, gan.dnG, case.glayers, case.gdims, gm, xG.astype(np.float32), p0.cpu().numpy())
        st.opt = self.raw_opt
        ref = GC.oracle_step(st, case, which, inp, masks_o, noise=noise_o)
        st.opt = self.real_opt
        fl = [NC.flips(inner(n)) for n in ((st.D,) + ((st.G,) if which == "G" else ()))]
        flips, units = sum(f[0] for f in fl), sum(f[1] for f in fl)
        NC.adopt(ctx, gan.dnD, case.dlayers, case.ddims, dmods, xD, None, clear=True)
        if which == "G":
            NC.adopt(ctx, gan.dnG, case.glayers, case.gdims, gm, xG, None, clear=True)
        assert flips <= max(1, 1e-5 * units), "%s: %d of %d PReLU decisions adopted from the device differ from the oracle's" % (what, flips, units)
        # ---- forward results ----------------------------------------------------------------------------------------------------------
        out = gan.view("D_OUTPUT", B).cpu().numpy().reshape(ref["out"].shape)
        loss = float(gan.view("LOSS")[w])
        assert abs(loss - ref["f_bce"]) <= 1e-5 * abs(ref["f_bce"]), "%s: BCE %.9g, oracle %.9g" % (what, loss, ref["f_bce"])
        conf = gan.view("CONFUSION").view(torch.int32).cpu().tolist()
        got = dn.grads.cpu().numpy()
        assert np.isfinite(got).all(), what + ": the gradient is not finite"
        oD, oG = inner(st.D), inner(st.G)
        if which == "D":
            if case.table:
                close(d_input[h:], ref["inputs"][h:], atol=1e-5, what=what + " fakes")
            else:
                close(d_input, ref["inputs"], atol=1e-5, what=what + " batch")
                assert np.array_equal(d_input[:h], inp["real"]), what + ": the real half"
            assert conf[:4] == [int(v) for v in ref["conf"].reshape(-1)], "%s: confusion %s, oracle %s" % (what, conf[:4], ref["conf"].reshape(-1))
            if flags:
                self.global_conf = conf[:4]
            assert conf[4:] == self.global_conf, "%s: global confusion counts %s" % (what, conf[4:])
            assert_net_bars(what + " D", oD, out, ref["out"], np.zeros(1), np.zeros(1), got)       # (a D-step forms no input gradient)
        else:
            close(d_input, ref["samples"], atol=1e-5, what=what + " samples")
            close(out, ref["out"], atol=1e-5, what=what + " D outputs")
            gin = st.D.gradInput[0] if case.table else oD.modules[0].gradInput
            gx = NC.from_device(gan.view("D_GRAD_INPUT", B * img).cpu().numpy().reshape(B, -1), op.first)
            close(gx, gin.reshape(gx.shape), atol=1e-4 * np.abs(gin).max() + 1e-7, what=what + " FG_GAN_D_GRAD_INPUT")
            assert_net_bars(what + " G", oG, d_input, ref["samples"], np.zeros(1), np.zeros(1), got)       # (nor a G-step one of G)
            assert conf[4:] == self.global_conf and sum(conf[:4]) in (0, case.iters[it]), what + ": a G-step wrote confusion counts"
        check_bn(what, st, gan)
        # ---- the net that is not stepped ----------------------------------------------------------------------------------------------
        if self.held is None or which == "G":
            assert torch.equal(other.params, o0) and torch.equal(gan.view("OPT_STATE_" + "GD"[w]), os0) and gan.steps(1 - w) == ot0, what + ": the other net moved"
        # ---- the update, separated from the gradient --------------------------------------------------------------------------------------
        if flags:
            assert torch.equal(dn.params, p0) and torch.equal(gan.view("OPT_STATE_" + which), s0) and gan.steps(w) == t0, what + ": FG_STEP_NO_UPDATE moved the net"
            if gate is True:
                gan.update(w)
                self.guards(what + " fg_gan_update")
            elif gate == "held":
                self.held = dn.grads.clone()
        if not flags or gate is True:
            self.check_update(what, which, p0, s0, t0, got)
        if which == "D" and self.held is not None:
            # a G gradient held across this D-step: fg_gan_update(G) applies it to G as it stands now
            dnG = gan.dnG
            assert torch.equal(dnG.grads, self.held), what + ": the D-step disturbed the gradient held for fg_gan_update(G)"
            pG0, sG0, tG0 = dnG.params.clone(), gan.view("OPT_STATE_G").clone(), gan.steps(1)
            gan.update(1)
            self.guards(what + " fg_gan_update(G)")
            self.check_update(what + ", held G gradient", "G", pG0, sG0, tG0, self.held.cpu().numpy())
            self.held = None

    def check_update(self, what, which, p0, s0, t0, g_dev):
        case, gan = self.case, self.gan
        w = "DG".index(which)
        dn = gan.dnD if which == "D" else gan.dnG
        method = (case.optD if which == "D" else case.optG)[0]
        p64 = p0.cpu().numpy().astype(np.float64)
        gp = GC.penalised(case.pen, which, p64, g_dev.astype(np.float64) * self.gscale)     # scale, then penalty, then clamp: fg_prep_grad
        x1, s1 = GC.apply_rule(case, which, p64, gp, s0.cpu().numpy(), t0)
        assert gan.steps(w) == t0 + 1, "%s: step count %d behind an update at %d" % (what, gan.steps(w), t0)
        (pa, pr), parts = OPT_BARS[method]
        n = p64.size
        p1, st1 = dn.params.cpu().numpy(), gan.view("OPT_STATE_" + which).cpu().numpy()
        print("%s %s update t = %d: max|dp| %.3e, max|p err| %.3e (bar %.1e + %.1e rel)" % (what, method, t0 + 1, np.abs(p1 - p64).max(), np.abs(p1 - x1).max(), pa, pr))
        assert np.abs(p1 - p64).max() > 0, what + ": the update moved nothing"
        close(p1, x1, atol=pa, rtol=pr, what="%s %s parameters at t = %d" % (what, method, t0 + 1))
        cfg = (case.optD if which == "D" else case.optG)[1]
        for k, (name, a, r) in enumerate(parts):
            if method == "sgd" and cfg.get("momentum", 0) == 0:
                assert np.array_equal(st1, s0.cpu().numpy()), what + ": plain SGD wrote its state buffer"
                continue
            close(st1[k * n:(k + 1) * n], s1[k * n:(k + 1) * n], atol=a, rtol=r, what="%s %s %s at t = %d" % (what, method, name, t0 + 1))
        assert np.array_equal(st1[len(parts) * n:], s0.cpu().numpy()[len(parts) * n:]), what + ": the unused half of the state buffer was written"


@pytest.mark.parametrize("case", GC.GAN_CASES, ids=[c.name for c in GC.GAN_CASES])
def test_gan_case_against_the_float64_oracle(ctx, case, request):
    comm = request.getfixturevalue("comm") if case.overlap is not None else None
    run = Run(ctx, case, comm)
    try:
        for it in range(len(case.iters)):
            run.closure(it, "D")
            run.closure(it, "G")
        assert run.held is None
        # FG_GAN_D_OUTPUT: the batch of the last closure
        off, cnt = ctypes.c_longlong(), ctypes.c_longlong()
        ctx.check(ctx.lib.fg_gan_buffer(run.gan.h, 7, ctypes.byref(off), ctypes.byref(cnt)))
        assert cnt.value == case.iters[-1]
    finally:
        if comm is not None:
            ctx.check(ctx.lib.fg_gan_set_comm(run.gan.h, None, 0, 1))


# ---- bit-level statements ------------------------------------------------------------------------------------------------------------
def snapshot(gan, B, img):
    torch.cuda.synchronize()
    return dict(pG=gan.dnG.params.clone(), pD=gan.dnD.params.clone(), gD=gan.dnD.grads.clone(), gG=gan.dnG.grads.clone(), bnG=gan.dnG.buffers.clone(),
                bnD=gan.dnD.buffers.clone(), d_out=gan.view("D_OUTPUT", B).clone(), loss=gan.view("LOSS").clone(), conf=gan.view("CONFUSION").view(torch.int32)[:4].clone(),
                optD=gan.view("OPT_STATE_D").clone(), optG=gan.view("OPT_STATE_G").clone(), d_input=gan.view("D_INPUT", B * img).clone())


def same(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s: %s differs" % (what, k)


def device_inputs(ctx, case, it):
    """the case's inputs of one iteration on the device, in the device's layout"""
    inp = GC.inputs(case, it)
    first = NC.walk(case.dlayers, case.ddims)[0]
    d = ctx.device
    img = lambda k: dev(NC.to_device(inp[k], first), d) if k in inp else None
    nz = lambda k: dev(inp[k].transpose(0, 2, 3, 1) if case.table else inp[k], d)
    masks = lambda k: [dev(m, d) for m in NC.device_masks(case.dlayers, case.ddims, inp[k])]
    return dict(B=inp["B"], real=img("real"), cond_real=img("cond_real"), cond_fake=img("cond_fake"), cond=img("cond"), noiseD=nz("noiseD"), noiseG=nz("noiseG"),
                masksD=masks("masksD"), masksG=masks("masksG"))


class HostDriven:
    """the two closures built from the net-level entries, the criterion and the fused optimizer entries: the same kernels in the same
    order as fg_step_D / fg_step_G, the batch assembled by torch (exact copies and additions)"""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.dnG = NC.device_net(ctx, case.glayers, case.gdims, case.max_batch)
        self.dnD = NC.device_net(ctx, case.dlayers, case.ddims, case.max_batch)
        self.state = [ctx.zeros(2 * self.dnD.n_params), ctx.zeros(2 * self.dnG.n_params)]
        self.steps, self.loss, self.conf = [0, 0], ctx.zeros(2), torch.zeros(4, dtype=torch.int32, device=ctx.device)

    def criterion(self, out, target, w, conf):
        B = out.numel()
        grad = self.ctx.empty(B)
        self.ctx.check(self.ctx.lib.fg_bce_forward_backward(self.ctx.h, out.data_ptr(), target.data_ptr(), B, self.loss[w:].data_ptr(), grad.data_ptr(),
                                                            self.conf.data_ptr() if conf else None))
        return grad

    def optimize(self, w):
        lib, h, case = self.ctx.lib, self.ctx.h, self.case
        dn = self.dnG if w else self.dnD
        method, cfg = case.optG if w else case.optD
        which = "DG"[w]
        l1, l2, clamp = case.pen[which + "_L1"], case.pen[which + "_L2"], case.pen[which + "_clamp"]
        pen = l1 != 0 or l2 != 0
        l1m, l2m = ((l2 if w else l1) if pen else 0.0), (l2 if pen else 0.0)
        n, s, P = dn.n_params, self.state[w], (lambda t: t.data_ptr())
        lr = cfg.get("learningRate", 1e-3)
        if method == "adam":
            self.steps[w] += 1
            rc = lib.fg_adam_fused(h, P(dn.params), P(dn.grads), P(s), P(s[n:]), n, 1.0, l1m, l2m, clamp, lr, cfg.get("beta1", 0.9), cfg.get("beta2", 0.999), cfg.get("epsilon", 1e-8),
                                   self.steps[w], None)
        elif method == "sgd":
            mom = cfg.get("momentum", 0)
            clr = lr / (1.0 + self.steps[w] * cfg.get("learningRateDecay", 0.0))
            rc = lib.fg_sgd_fused(h, P(dn.params), P(dn.grads), P(s) if mom else None, n, 1.0, l1m, l2m, clamp, float(np.float32(clr)), mom, cfg.get("dampening", mom),
                                  cfg.get("weightDecay", 0.0), 1 if cfg.get("nesterov") else 0, 1 if (mom and self.steps[w] == 0) else 0)
            self.steps[w] += 1
        else:
            clr = lr / (1.0 + self.steps[w] * cfg.get("learningRateDecay", 0.0))
            rc = lib.fg_adagrad_fused(h, P(dn.params), P(dn.grads), P(s), n, 1.0, l1m, l2m, clamp, float(np.float32(clr)))
            self.steps[w] += 1
        self.ctx.check(rc)
        dn.params_changed()

    def g_input(self, noise, cond):
        return torch.cat([noise, cond], dim=3).contiguous() if self.case.table else noise

    def step_D(self, i):
        B, h = i["B"], i["B"] // 2
        fake = self.dnG.forward(self.g_input(i["noiseD"], i["cond_fake"]), train=True).reshape(h, -1)
        x = torch.cat([i["real"].reshape(h, -1), fake], 0)
        if self.case.table:
            x = x + torch.cat([i["cond_real"].reshape(h, -1), i["cond_fake"].reshape(h, -1)], 0)
        self.d_input = torch.cat([i["real"].reshape(h, -1), fake], 0).clone()
        x = x.reshape((B,) + tuple(i["real"].shape[1:])).contiguous()
        out = self.dnD.forward(x, masks=i["masksD"] or None, train=True)
        target = torch.cat([torch.ones(h), torch.zeros(h)]).to(self.ctx.device)
        self.d_out = out.reshape(-1).clone()
        self.dnD.backward(self.criterion(out, target, 0, True), param_grads=True)
        self.optimize(0)

    def step_G(self, i):
        B = i["B"]
        gin = self.g_input(i["noiseG"], i["cond"])
        samples = self.dnG.forward(gin, train=True).clone()
        self.d_input = samples.reshape(B, -1).clone()
        x = samples + i["cond"] if self.case.table else samples
        out = self.dnD.forward(x.contiguous(), masks=i["masksG"] or None, train=True)
        self.d_out = out.reshape(-1).clone()
        gx = self.dnD.backward(self.criterion(out, torch.ones(B, device=self.ctx.device), 1, False), param_grads=False, input_grad=True)
        self.dnG._x = gin                     # (D's forward went through another net: G's own input is what its backward reads)
        self.dnG.backward(gx, param_grads=True)
        self.optimize(1)

    def snapshot(self, B):
        torch.cuda.synchronize()
        return dict(pG=self.dnG.params.clone(), pD=self.dnD.params.clone(), gD=self.dnD.grads.clone(), gG=self.dnG.grads.clone(), bnG=self.dnG.buffers.clone(),
                    bnD=self.dnD.buffers.clone(), d_out=self.d_out.clone(), loss=self.loss.clone(), conf=self.conf.clone(), optD=self.state[0].clone(),
                    optG=self.state[1].clone(), d_input=self.d_input.reshape(-1).clone())


BITWISE = ["r1-3x3x3-b2-6-8", "r1-1x5x5-b2-4", "r1-1x4x4-aligned", "r1-2x3x5-nonsquare", "r2-general-conv-5ch", "r2-bn-prelu-last", "r3-bn-both-nets", "r4-table-1ch",
           "r4-table-3ch", "r5-one-dropout-explicit", "r9-sgd-momentum-vs-adam", "r9-sgd-nesterov-vs-sgd-decay", "r10-D-L1-and-L2", "r10-G-L2-drives-the-sign-term"]


@pytest.mark.parametrize("name", BITWISE)
def test_fused_steps_equal_host_driven_closures(ctx, name):
    """what tests/test_gpu_step_abi.py states at 32 px, on small pairs: the same kernels in the same order give the same bits -- at every
    residue of (B/2) * C*H*W modulo 4.  Where the second half of D's batch starts on 16 bytes G's last stage writes it in place; elsewhere
    G keeps its output and copy_kernel places it: nothing depends on where the second half starts."""
    case = GC.BY_NAME[name]._replace(masks="explicit")
    st = GC.oracle_gan(case, np.float64)
    gan = GC.device_gan(ctx, case)
    hd = HostDriven(ctx, case)
    load(st, gan)
    hd.gan = None
    for dn, src in ((hd.dnG, gan.dnG), (hd.dnD, gan.dnD)):
        dn.params.copy_(src.params); dn.buffers.copy_(src.buffers); dn.params_changed()
    img = int(np.prod(case.ddims))
    residues = set()
    for it in range(len(case.iters)):
        i = device_inputs(ctx, case, it)
        B = i["B"]
        residues.add((B // 2) * img % 4)
        gan.step_D(B, i["real"], i["cond_real"], i["cond_fake"], i["noiseD"], i["masksD"] or None)
        hd.step_D(i)
        a, b = snapshot(gan, B, img), hd.snapshot(B)
        if case.table:                        # (table mode: the real half of FG_GAN_D_INPUT is not written, the sum is what D reads)
            a["d_input"], b["d_input"] = a["d_input"][(B // 2) * img:], b["d_input"][(B // 2) * img:]
        same(a, b, "%s iteration %d D-step at B = %d" % (name, it, B))
        gan.step_G(B, i["cond"], i["noiseG"], i["masksG"] or None)
        hd.step_G(i)
        same(snapshot(gan, B, img), hd.snapshot(B), "%s iteration %d G-step at B = %d" % (name, it, B))
    print("%s: (B/2) * C*H*W mod 4 in %s" % (name, sorted(residues)))


def test_the_bitwise_cases_cover_every_residue():
    seen = set()
    for n in BITWISE:
        c = GC.BY_NAME[n]
        seen |= {(c.table, (B // 2) * int(np.prod(c.ddims)) % 4) for B in c.iters}
    assert seen >= {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3)}


@pytest.mark.parametrize("name", ["r1-3x3x3-b2-6-8", "r1-1x5x5-b2-4", "r4-table-1ch"])
def test_a_step_does_not_depend_on_the_batch_the_object_was_built_for(ctx, name):
    """a D-step and a G-step at batch B in a step object built for B and in one built for 2 B + 2: every buffer behind D's batch starts
    elsewhere, the bits are the same"""
    case = GC.BY_NAME[name]._replace(masks="explicit")
    img = int(np.prod(case.ddims))
    for it, B in enumerate(case.iters):
        if (B // 2) * img % 4 == 0:
            continue
        res = []
        for M in (B, 2 * B + 2):
            c = case._replace(max_batch=M)
            gan = GC.device_gan(ctx, c)
            load(GC.oracle_gan(c, np.float64), gan)
            i = device_inputs(ctx, case, it)
            gan.step_D(B, i["real"], i["cond_real"], i["cond_fake"], i["noiseD"], i["masksD"] or None)
            d = snapshot(gan, B, img)
            gan.step_G(B, i["cond"], i["noiseG"], i["masksG"] or None)
            res.append((d, snapshot(gan, B, img)))
        for k in (0, 1):
            a, b = res[0][k], res[1][k]
            if case.table and k == 0:
                a["d_input"], b["d_input"] = a["d_input"][(B // 2) * img:], b["d_input"][(B // 2) * img:]
            same(a, b, "%s B = %d, max_batch %d against %d, %s-step" % (name, B, B, 2 * B + 2, "DG"[k]))


def test_a_refused_step_and_the_bits_of_the_next_one(ctx):
    """the GPU half of (c) of tests/test_gan_steps_host.py: steps refused for an odd batch, a batch above max_batch, a null `real` and a
    bound workspace that is too small (behind the draw; the second behind G's forward too) leave noise, masks and every result of the
    next accepted steps what they are on a twin that was never refused"""
    case = GC.BY_NAME["r7-tail-then-max"]
    lib, img, M = ctx.lib, int(np.prod(case.ddims)), case.max_batch
    res = []
    for refuse in (True, False):
        gan = GC.device_gan(ctx, case)
        load(GC.oracle_gan(case, np.float64), gan)
        i = device_inputs(ctx, case, 1)
        gan.step_D(M, i["real"]); gan.step_G(M)
        if refuse:
            D = lambda B, x=i["real"]: lib.fg_step_D(gan.h, B, x.data_ptr() if x is not None else None, None, None, None, None, 0)
            G = lambda B: lib.fg_step_G(gan.h, B, None, None, None, 0)
            key = gan._bound
            assert D(M - 1) == -1 and G(M + 2) == -1 and D(M, None) == -1
            ctx.check(lib.fg_gan_bind_workspaces(gan.h, key[0], key[1] * 4, key[2], 64))
            assert D(M) == -5 and G(M) == -5
            ctx.check(lib.fg_gan_bind_workspaces(gan.h, key[0], 64, key[2], key[3] * 4))
            assert D(M) == -5 and G(M) == -5
            ctx.check(lib.fg_gan_bind_workspaces(gan.h, key[0], key[1] * 4, key[2], key[3] * 4))
        out = []
        for B in (M, 4):
            gan.step_D(B, i["real"][:B // 2])
            s = snapshot(gan, B, img)
            s.update(noise=gan.view("NOISE", B // 2 * case.gdims[0]).clone(), mask=gan.mask_view(0, B).clone())
            gan.step_G(B)
            t = snapshot(gan, B, img)
            t.update(noise=gan.view("NOISE", B * case.gdims[0]).clone(), mask=gan.mask_view(0, B).clone())
            out += [s, t]
        res.append(out)
    for k, (a, b) in enumerate(zip(*res)):
        same(a, b, "closure %d behind the refused steps" % k)
    assert not torch.equal(res[0][0]["noise"], res[0][2]["noise"][:res[0][0]["noise"].numel()])


def test_overlap_on_a_one_rank_communicator_gives_the_bits_of_no_communicator(ctx, comm):
    """fg_gan_set_comm(overlap = 0, 1, 2) on a real one-rank communicator: blocking exchange, no exchange (one rank), and the N > 1 path
    -- D's all-reduce on the side stream with its update deferred into the next G-step, G's backward in ranges with one all-reduce per
    bucket -- give the parameters, state and results of the run without a communicator, bit for bit, over two iterations; so does G's
    backward in two buckets (a target of a third of the vector: the cut lies between a convolution and the BatchNorm stage below it).
    With a target of one parameter every stage is a bucket, and a cut between a PReLU stage and the convolution above it takes the
    PReLU's backward out of that convolution's epilogue (fg_net_backward_range, include/facegen_hip.h): the slope's gradient is then
    summed in another order.  There every entry of G's gradient but the PReLU slopes keeps its bits, and the slopes stay within the
    slope bar of gpu_util.assert_net_bars; tests/test_gpu_gan_steps.py::test_gan_case_against_the_float64_oracle holds that run
    (`r11-overlapped-3-buckets`) to the oracle.  This pins the ranged backward and the stream joins; it does not pin the bucket
    RANGES (a one-rank sum is the identity): tests/test_gan_steps_host.py holds those."""
    case = GC.BY_NAME["r11-overlapped-3-buckets"]._replace(masks="explicit")
    img = int(np.prod(case.ddims))
    nP = GC.oracle_gan(case).pG.size
    res, first = {}, {}
    for tag, ov, bucket in (("none", None, 0), ("blocking", 0, 0), ("one-rank", 1, 0), ("overlapped", 2, 0), ("overlapped, 2 buckets", 2, nP // 3),
                            ("overlapped, every stage a bucket", 2, 1)):
        gan = GC.device_gan(ctx, case._replace(bucket=bucket))
        load(GC.oracle_gan(case, np.float64), gan)
        if ov is not None:
            ctx.check(ctx.lib.fg_gan_set_comm(gan.h, comm, 0, ov))
        try:
            for it in range(len(case.iters)):
                i = device_inputs(ctx, case, it)
                gan.step_D(i["B"], i["real"], None, None, i["noiseD"], i["masksD"])
                assert gan.pending() == (ov == 2), tag
                gan.step_G(i["B"], None, i["noiseG"], i["masksG"])
                assert not gan.pending()
                if it == 0:
                    first[tag] = snapshot(gan, i["B"], img)
            res[tag] = snapshot(gan, i["B"], img)
        finally:
            ctx.check(ctx.lib.fg_gan_set_comm(gan.h, None, 0, 1))
        slopes = [gan.dnG.param_offsets(k)[0] for k, l in enumerate(case.glayers) if l[0] == "PRELU"]
    for tag in res:
        if tag != "overlapped, every stage a bucket":
            same(res["none"], res[tag], tag)
    a, b = first["none"], first["overlapped, every stage a bucket"]
    same({k: v for k, v in a.items() if k not in ("gG", "pG", "optG")}, {k: v for k, v in b.items() if k not in ("gG", "pG", "optG")}, "every stage a bucket, iteration 0")
    differ = torch.nonzero(a["gG"].view(torch.int32) != b["gG"].view(torch.int32)).reshape(-1).cpu().tolist()
    print("every stage a bucket: gradient entries whose bits differ from the unsplit backward: %s (PReLU slopes at %s)" % (differ, slopes))
    assert set(differ) <= set(slopes), "entries %s of G's gradient differ, PReLU slopes are at %s" % (differ, slopes)
    ga, gb = a["gG"].cpu().numpy().astype(np.float64), b["gG"].cpu().numpy().astype(np.float64)
    for k in differ:
        assert abs(ga[k] - gb[k]) <= 1e-4 * abs(ga[k]) + 1e-7, (k, ga[k], gb[k])


@pytest.fixture(scope="module")
def planned_schedules():
    """{(case, overlap, bucket): lines of fg_comm_schedule} from ONE planning-only child process (tests/dispatch_audit.py
    sync_gan_replay): the text every rank of the job must produce"""
    import dispatch_audit as A
    return {(j["case"], j["overlap"], j["bucket"]): j["schedule"] for j in A.sync_gan_replay()}


@pytest.mark.parametrize("name", SC.SYNC_STEP_CASES)
def test_sync_bn_steps_on_a_dry_two_rank_communicator(ctx, name, planned_schedules):
    """The step-level sync path on one GPU: a transport-less communicator (fg_comm_create_dry), rank 0 of 2, on the device context makes
    fg_gan_set_comm(..., sync_bn = 1, ...) stick.  gan_drain then pauses under fg_net_forward_to (G's redirected output), under D's
    passes and under the bucketed fg_net_backward_range of G; D's update is deferred (overlap 1); gan_optimize scales by 1 / 2.  Every
    collective is recorded and skipped, so BatchNorm sees the local batch and the gradient stays local: the float64-oracle comparison
    of Run.closure applies unchanged, the update from the device's gradient x 1 / 2.  Overlap 0 and 1 give the same bits; the runs
    with G's backward cut into buckets are held to the oracle alone (a cut at a PReLU stage moves its backward out of the
    neighbour's epilogue).  The schedule recorded on the device is the text the planning-only context gives for the same settings."""
    from face_generator_amd.distributed import DryCollective
    base = GC.BY_NAME[name]._replace(masks="explicit", overlap=None, bucket=0)
    assert any(l[0] == "BATCHNORM" for l in base.glayers + base.dlayers)
    img = int(np.prod(base.ddims))
    nP = GC.oracle_gan(base).pG.size
    final = {}
    for overlap, bucket in SC.step_settings(name):
        case = base._replace(bucket=SC.bucket_target(bucket, nP))
        coll = DryCollective(ctx, 0, SC.STEP_WORLD)
        run = Run(ctx, case, coll.h, sync_bn=1, overlap=overlap, gscale=1.0 / SC.STEP_WORLD)
        try:
            sb = run.gan.view("SYNC_BUF")
            assert sb.numel() >= 2 * max(SC.step_f64_counts(case)), "FG_GAN_SYNC_BUF of %d floats" % sb.numel()
            for it in range(len(case.iters)):
                run.closure(it, "D")
                run.closure(it, "G")
            assert not run.gan.pending()
            final[overlap, bucket] = snapshot(run.gan, case.iters[-1], img)
            got = coll.schedule(reset=True)
            want = planned_schedules[name, overlap, bucket]
            assert got == want, "%s overlap %d bucket %s: the schedule on the device\n%s\nthe planning-only one\n%s" % (name, overlap, bucket, "\n".join(got), "\n".join(want))
            f64 = [int(l.split()[3]) for l in got if l.split()[2] == "f64"]
            assert f64 == SC.step_f64_counts(case) and f64, (name, f64)
        finally:
            ctx.check(ctx.lib.fg_gan_set_comm(run.gan.h, None, 0, 1))
            coll.close()
    a, b = final[0, None], final[1, None]
    keys = ("pG", "pD", "optD", "optG", "bnG", "bnD")
    same({k: a[k] for k in keys}, {k: b[k] for k in keys}, "%s: overlap 1 against overlap 0" % name)


def test_nesterov_with_dampening_is_refused(ctx):
    """interruptable_sgd asserts "Nesterov momentum requires a momentum and zero dampening"; dampening < 0 means = momentum"""
    case = GC.BY_NAME["r9-sgd-nesterov-vs-sgd-decay"]._replace(optD=("sgd", dict(learningRate=0.05, momentum=0.8, nesterov=True)))
    gan = GC.device_gan(ctx, case)
    load(GC.oracle_gan(case, np.float64), gan)
    i = device_inputs(ctx, case, 0)
    p0 = gan.dnD.params.clone()
    gan._bind()
    rc = ctx.lib.fg_step_D(gan.h, i["B"], i["real"].data_ptr(), None, None, i["noiseD"].data_ptr(), None, 0)
    assert rc == -1 and "Nesterov" in ctx.lib.fg_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    assert torch.equal(gan.dnD.params, p0) and gan.steps(0) == 0


# ---- fg_bce_forward_backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_bce_against_numpy(ctx, n):
    """nn.BCECriterion with the confusion counts, against numpy in float64 with the eps additions made in float32 as BCECriterion.forward
    of the oracle makes them: probabilities that include exactly 0, 1, 0.5 and 1e-13, targets 0 / 1; confusion_dev and grad_dev each
    NULL in one row.  Bars: counts exact, gradient and loss 1e-6 relative."""
    rng = np.random.default_rng(n)
    x = rng.uniform(0, 1, n).astype(np.float32)
    special = np.array([0.0, 1.0, 0.5, 1e-13, 1.0, 0.0, 0.5], np.float32)
    x[:min(n, special.size)] = special[:n]
    t = (rng.random(n) < 0.5).astype(np.float32)
    t[:min(n, 7)] = [1, 0, 1, 0, 1, 0, 0][:n]    # a certain miss of either kind (x = 0 with target 1, x = 1 with target 0) comes first
    eps = np.float32(1e-12)
    a, b = (x + eps).astype(np.float64), ((np.float32(1) - x) + eps).astype(np.float64)
    t64 = t.astype(np.float64)
    loss = -(t64 * np.log(a) + (1 - t64) * np.log(b)).sum() / n
    grad = -(t64 - x.astype(np.float64)) / (b * a) / n
    conf = [int((((x > 0.5) == p) & ((t > 0.5) == q)).sum()) for p in (False, True) for q in (False, True)]
    xd, td = dev(x, ctx.device), dev(t, ctx.device)
    for with_grad, with_conf in ((True, True), (False, True), (True, False)):
        ld, gd = ctx.zeros(1), torch.full((n,), float("nan"), device=ctx.device)
        cd = torch.full((4,), -1, dtype=torch.int32, device=ctx.device)
        ctx.check(ctx.lib.fg_bce_forward_backward(ctx.h, xd.data_ptr(), td.data_ptr(), n, ld.data_ptr(), gd.data_ptr() if with_grad else None, cd.data_ptr() if with_conf else None))
        torch.cuda.synchronize()
        got = float(ld[0])
        assert np.isfinite(got) and (not with_grad or bool(torch.isfinite(gd).all())), "bce n = %d: not finite" % n
        print("bce n = %d: loss %.9g (reference %.9g, relative error %.2e)" % (n, got, loss, abs(got - loss) / abs(loss)))
        assert abs(got - loss) <= 1e-6 * abs(loss)
        if with_grad:
            close(gd.cpu().numpy(), grad, atol=0.0, rtol=1e-6, what="bce gradient, n = %d" % n)
        else:
            assert bool(torch.isnan(gd).all())
        assert cd.cpu().tolist() == (conf if with_conf else [-1] * 4)
