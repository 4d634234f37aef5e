"""GPU parity of nn.ConcatTable discriminators compiled to ONE device plan (FG_CONCAT_TABLE / FG_BRANCH / FG_JOIN_TABLE): the join /
split / sum kernels alone, every compiled discriminator of models.lua:110-316 against the float32 oracle, the one-plan net against
the host-walked composite, the fused step entries (fg_step_D / fg_step_G) at 16 px, B = 128 against the float64 oracle and one
adversarial.train epoch at scale 16.  The bars are the project's existing ones (tests/test_gpu_net.py, tests/test_gpu_baseline_sizes.py)."""
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import nhwc, nchw, dev, close, close_after_first_adam_step
from gpu_util import forward_backward_against_oracle as _forward_backward_against_oracle
from test_gpu_net import _fill_nontrivial
from test_gpu_baseline_sizes import check_every_tensor, assert_flips_bounded, f64_state, floor_for, adam_from
from test_gpu_train_epoch import ListDataset, Recorder, load_state
from test_branched_host import ORACLES, _flat_modules

pytestmark = pytest.mark.gpu

# create_D32 (models.lua:322-376) has no device plan (54-channel max-pool): a host-side model only
NETS = [("create_D16_d", 3), ("create_D16_d", 1), ("create_D16", 3), ("create_D16", 1), ("create_D16_b", 3), ("create_D16_c", 3)]


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


# ---- item 10: the kernels alone ------------------------------------------------------------------------------------------------
def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


@pytest.mark.parametrize("rows", [1, 129])
@pytest.mark.parametrize("widths", [(128, 1024), (4, 8), (5, 3), (1024, 1024, 1024), (7, 128, 2), (12, 4, 4, 8), (1, 2, 3, 5), (512, 512, 1024, 6)])
def test_join_split_rows_bit_exact(ctx, widths, rows):
    lib, d = ctx.lib, ctx.device
    rng = np.random.default_rng(sum(widths) + rows)
    parts = [rng.standard_normal((rows, w)).astype(np.float32) for w in widths]
    pd = [dev(p, d) for p in parts]
    wd = (ctypes.c_int * len(widths))(*widths)
    out = torch.full((rows, sum(widths)), float("nan"), device=d)
    ctx.check(lib.fg_join_rows(ctx.h, _ptrs(pd), wd, len(widths), out.data_ptr(), rows))
    want = np.concatenate(parts, axis=1)
    assert np.array_equal(out.cpu().numpy(), want)
    back = [torch.full((rows, w), float("nan"), device=d) for w in widths]
    ctx.check(lib.fg_split_rows(ctx.h, out.data_ptr(), _ptrs(back), wd, len(widths), rows))
    for b, w in zip(back, np.split(want, np.cumsum(widths)[:-1], axis=1)):
        assert np.array_equal(b.cpu().numpy(), w)
    # a part nobody asked for is skipped, the others are still written
    back = [torch.full((rows, w), 7.0, device=d) for w in widths]
    ctx.check(lib.fg_split_rows(ctx.h, out.data_ptr(), _ptrs([None] + back[1:]), wd, len(widths), rows))
    assert float(back[0].min()) == 7.0 and np.array_equal(back[-1].cpu().numpy(), parts[-1])
    # unaligned part pointers take the scalar path
    if len(widths) == 2 and widths[0] % 4 == 0:
        buf = torch.zeros(rows * widths[0] + 1, device=d)
        buf[1:] = pd[0].reshape(-1)
        out2 = torch.zeros_like(out)
        ctx.check(lib.fg_join_rows(ctx.h, _ptrs([buf[1:], pd[1]]), wd, 2, out2.data_ptr(), rows))
        assert np.array_equal(out2.cpu().numpy(), want)


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("count", [1, 7, 129 * 768, 129 * 768 + 2])
def test_sum_n_adds_in_the_documented_order(ctx, n, count):
    """out = ((p0 + p1) + p2) + p3 in float32, bit for bit"""
    rng = np.random.default_rng(n * 1000 + count % 977)
    parts = [(rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(n)]
    pd = [dev(p, ctx.device) for p in parts]
    out = torch.full((count,), float("nan"), device=ctx.device)
    ctx.check(ctx.lib.fg_sum_n(ctx.h, _ptrs(pd), n, out.data_ptr(), count))
    want = parts[0].copy()
    for p in parts[1:]:
        want = (want + p).astype(np.float32)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- the risk of the issue: the 5x5 layers with 32 channels no compiled net had met (models.lua:125-128), as a plain chain ----------
@pytest.mark.parametrize("C", [3, 1])
def test_chain_of_the_new_channel_counts(ctx, C):
    """conv5x5(C -> 32) - PReLU - conv5x5(32 -> 64) - PReLU - MaxPool - View - Linear against the oracle at the bars of
    tests/test_gpu_net.py:279-297"""
    from face_generator_amd import nn
    B = 8
    rng = np.random.default_rng(4100 + C)
    net = O.Sequential(O.SpatialConvolution(C, 32, 5, 5, 1, 1, 2, None, rng), O.PReLU(), O.SpatialConvolution(32, 64, 5, 5, 1, 1, 2, None, rng),
                       O.PReLU(), O.SpatialMaxPooling(2, 2), O.View(64 * 64), O.Linear(64 * 64, 128, rng))
    _fill_nontrivial(net, rng)
    dn = nn.Sequential()
    for m in (nn.SpatialConvolution(C, 32, 5, 5, 1, 1, 2), nn.PReLU(), nn.SpatialConvolution(32, 64, 5, 5, 1, 1, 2), nn.PReLU(),
              nn.SpatialMaxPooling(2, 2), nn.View(64 * 64), nn.Linear(64 * 64, 128)):
        dn.add(m)
    dn.input_dims = (C, 16, 16)
    dn.cuda(ctx, max_batch=B)
    _forward_backward_against_oracle(ctx, "5x5 chain C=%d" % C, net, dn, (C, 16, 16), B, rng, [])


def _masks_for(dn, B, rng):
    return [(rng.random((B, dn.mask_shape(i, B)[0] // B)) < 0.5).astype(np.float32) for i in range(dn.n_masks)]


# ---- item 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C", NETS)
def test_table_discriminators_forward_backward(ctx, name, C):
    from face_generator_amd import models
    from face_generator_amd.runtime import DeviceNet
    B, dims = 8, (C, 16, 16)
    rng = np.random.default_rng(7000 + len(name) * 10 + C)
    D = ORACLES[name](dims, rng)
    _fill_nontrivial(D, rng)
    Dd = getattr(models, name)(dims).cuda(ctx, max_batch=B)
    assert isinstance(Dd.device_net, DeviceNet)
    _forward_backward_against_oracle(ctx, "%s C=%d" % (name, C), D, Dd, dims, B, rng, _masks_for(Dd.device_net, B, rng))


# ---- item 6 ----------------------------------------------------------------------------------------------------------------------
def test_one_plan_equals_the_composite_route(ctx):
    """Same parameters, inputs and masks through the one-plan net and through cuda(composite=True): the same kernels run on the same
    numbers in both, so the results are compared bit for bit."""
    from face_generator_amd import models
    from face_generator_amd.runtime import DeviceNet, CompositeDeviceNet
    B, dims = 8, (3, 16, 16)
    rng = np.random.default_rng(7100)
    D = O.create_D16_d(dims, rng)
    _fill_nontrivial(D, rng)
    pD, _ = D.getParameters()
    one = models.create_D(dims).cuda(ctx, max_batch=B)
    comp = models.create_D(dims).cuda(ctx, max_batch=B, composite=True)
    assert isinstance(one.device_net, DeviceNet) and isinstance(comp.device_net, CompositeDeviceNet)
    x = nhwc(rng.uniform(0, 1, (B,) + dims).astype(np.float32), ctx.device)
    gy = dev(rng.standard_normal((B, 1)).astype(np.float32), ctx.device)
    masks = [dev(m.reshape(-1), ctx.device) for m in _masks_for(one.device_net, B, rng)]
    res = []
    for net in (one, comp):
        p, g = net.getParameters()
        p.copy_(torch.tensor(pD)); net.device_net.params_changed()
        y = net.device_net.forward(x, masks=masks, train=True).clone()
        gx = net.device_net.backward(gy, param_grads=True, input_grad=True).clone()
        res.append((y.reshape(-1), gx.reshape(-1), g.clone()))
    for what, a, b in zip(("outputs", "input gradient", "flat parameter gradient"), res[0], res[1]):
        print("one plan vs composite, %s: max |difference| %.3e" % (what, float((a - b).abs().max())))
    for what, a, b in zip(("outputs", "input gradient", "flat parameter gradient"), res[0], res[1]):
        assert torch.equal(a, b), what


# ---- the oracle on the device's PReLU / max-pool decisions (oracle/device_branches.py), for a table net --------------------
def _sequentials(onet):
    return [onet] + list(onet.modules[0].modules)


def adopt_table_branches(dn, onet, also=(), clear=False, params=None):
    """oracle/device_branches.py for a table net: the flat layer index of the device plan names the module inside its branch.
    `params`: the flat parameter vector as it was during the forward (a fused step updates it right after the backward)."""
    P = dn.params.cpu().numpy() if params is None else params
    fms = [_flat_modules(o) for o in (onet,) + tuple(also)]
    for i, m in enumerate(fms[0]):
        if isinstance(m, O.PReLU):
            pos = None if clear else nchw(dn.layer_output(i - 1)) > 0
            for fm in fms:
                fm[i].pos_override = pos
        elif isinstance(m, O.SpatialMaxPooling):
            idx = None
            if not clear:
                try:
                    x = nchw(dn.layer_output(i - 1))
                except Exception:                 # PReLU + MaxPool is one stage: re-evaluate prelu(x) the way the kernel does
                    xpre = nchw(dn.layer_output(i - 2)).astype(np.float32)
                    a = np.float32(P[dn.param_offsets(i - 1)[0]])
                    x = np.where(xpre > 0, xpre, (a * xpre).astype(np.float32)).astype(np.float32)
                n, c, h, w = x.shape
                idx = x.reshape(n, c, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4).argmax(axis=-1)
            for fm in fms:
                fm[i].indices_override = idx


def table_flips(onet):
    flips = units = 0
    for s in _sequentials(onet):
        for m, x in zip(s.modules, s._inputs):
            if isinstance(m, O.PReLU):
                units += int(x.size)
                if m.pos_override is not None:
                    flips += int(((x > 0) != m.pos_override.reshape(x.shape)).sum())
    return flips, units


# ---- item 7 ----------------------------------------------------------------------------------------------------------------------
def _gan16(ctx, name, C, B, seed):
    from face_generator_amd import models, adversarial
    rng = np.random.default_rng(seed)
    dims = (C, 16, 16)
    G = O.create_G16(dims, 100, rng, weight_init_=False); D = ORACLES[name](dims, rng)
    st = O.GanState(G, D)
    Gd = models.create_G(dims, 100).cuda(ctx, max_batch=B)
    Dd = getattr(models, name)(dims).cuda(ctx, max_batch=B)
    Gd.getParameters()[0].copy_(torch.tensor(st.pG)); Dd.getParameters()[0].copy_(torch.tensor(st.pD))
    Gd.device_net.params_changed(); Dd.device_net.params_changed()
    tr = adversarial.Trainer(ctx, Gd, Dd, dict(batchSize=B, noiseDim=100))
    return st, Gd, Dd, tr, rng


@pytest.mark.parametrize("name", ["create_D16_d", "create_D16", "create_D16_b", "create_D16_c"])
def test_fused_steps_at_16px(ctx, name):
    B, C = 8, 3
    st, Gd, Dd, tr, rng = _gan16(ctx, name, C, B, 7200 + len(name))
    assert tr.gan is not None, "a ConcatTable discriminator must train through fg_step_D / fg_step_G"
    d = ctx.device
    real = rng.uniform(0, 1, (B // 2, C, 16, 16)).astype(np.float32)
    nz = rng.uniform(-1, 1, (B // 2, 100)).astype(np.float32)
    masks = _masks_for(Dd.device_net, B, rng)
    ref = O.step_D(st, real, nz, masks)
    got = tr.step_D(nhwc(real, d), dev(nz, d), [dev(m.reshape(-1), d) for m in masks], keep_grad=True)
    close(got["outputs"].cpu().numpy().reshape(-1), ref["out"].reshape(-1), atol=1e-5, what="16px D-step outputs")
    assert abs(got["loss"].item() - ref["f_bce"]) <= 1e-5 * abs(ref["f_bce"])
    close(got["grad"].cpu().numpy(), ref["grad"], atol=1e-4 * np.abs(ref["grad"]).max() + 1e-7, what="16px D-step flat grad")
    nz2 = rng.uniform(-1, 1, (B, 100)).astype(np.float32)
    ref = O.step_G(st, nz2, masks)
    got = tr.step_G(dev(nz2, d), [dev(m.reshape(-1), d) for m in masks])
    close(nchw(got["samples"]), ref["samples"], atol=1e-5, what="16px G-step samples")
    close(got["outputs"].cpu().numpy().reshape(-1), ref["out"].reshape(-1), atol=1e-5, what="16px G-step D outputs")
    # the library draws noise and masks (one Philox launch per closure); what it drew is fed to the oracle.  Two iterations from the
    # device's state: the fused Adam + re-pack of the branched flat vector at t = 2 and t = 3 for D (t = 1 was the step above)
    nD, nG = st.pD.size, st.pG.size
    for it in range(2):
        for which, dn, p, ad, n in (("D", Dd.device_net, st.pD, st.adamD, nD), ("G", Gd.device_net, st.pG, st.adamG, nG)):
            os_ = tr.gan.view("OPT_STATE_" + which)
            p[...] = dn.params.cpu().numpy()
            if tr.gan.steps(0 if which == "D" else 1) > 0:
                ad.update(t=tr.gan.steps(0 if which == "D" else 1), m=os_[:n].cpu().numpy().copy(), v=os_[n:2 * n].cpu().numpy().copy(),
                          denom=np.zeros(n, np.float32))
        p0, m0, v0, t0 = st.pD.copy(), st.adamD["m"].copy(), st.adamD["v"].copy(), st.adamD["t"]
        real = rng.uniform(0, 1, (B // 2, C, 16, 16)).astype(np.float32)
        r = tr.step_D(nhwc(real, d), None, keep_grad=True)
        nzl = r["noise"].cpu().numpy().reshape(B // 2, 100)
        ml = [m.cpu().numpy().reshape(B, -1) for m in r["masks"]]
        assert len(ml) == Dd.device_net.n_masks and all(set(np.unique(m)) <= {0.0, 1.0} for m in ml)
        # gradients are compared on the device's PReLU / max-pool decisions (one unit within rounding of the kink moves a whole bias
        # entry), under the project's bound on how many decisions may differ
        adopt_table_branches(Dd.device_net, st.D, params=p0)
        ref = O.step_D(st, real, nzl, ml)
        assert_flips_bounded("%s library-drawn D-step %d" % (name, it), st.D, *table_flips(st.D))
        adopt_table_branches(Dd.device_net, st.D, clear=True)
        gD = r["grad"].cpu().numpy()
        close(r["outputs"].cpu().numpy().reshape(-1), ref["out"].reshape(-1), atol=1e-5, what="library-drawn D-step outputs, iteration %d" % it)
        close(gD, ref["grad"], atol=1e-4 * np.abs(ref["grad"]).max() + 1e-7, what="library-drawn D-step flat grad, iteration %d" % it)
        close(Dd.device_net.params.cpu().numpy(), adam_from(p0, gD, m0, v0, t0), atol=1e-6, what="D Adam + re-pack at t = %d" % (t0 + 1))
        st.pD[...] = Dd.device_net.params.cpu().numpy()
        r = tr.step_G(B)
        nzl = r["noise"].cpu().numpy().reshape(B, 100)
        ml = [m.cpu().numpy().reshape(B, -1) for m in r["masks"]]
        ref = O.step_G(st, nzl, ml)
        close(nchw(r["samples"]), ref["samples"], atol=1e-5, what="library-drawn G-step samples, iteration %d" % it)
        # D's packed weights come from the fused update: its outputs on G's samples pin the re-pack of every branch
        close(r["outputs"].cpu().numpy().reshape(-1), ref["out"].reshape(-1), atol=1e-5, what="library-drawn G-step D outputs, iteration %d" % it)


# ---- item 8 ----------------------------------------------------------------------------------------------------------------------
def test_16px_full_step_at_batch_128_against_the_float64_oracle(ctx):
    """G16 + D16_d at (3, 16, 16), B = 128: D-step and G-step, every parameter tensor of both flat gradients against the float64
    oracle at the frozen bars of tests/test_gpu_baseline_sizes.py::check_every_tensor; the oracle adopts the device's PReLU
    decisions (a few of ~10^6 units sit within rounding of the kink), bounded by assert_flips_bounded."""
    from oracle.device_branches import adopt_device_branches
    B, C = 128, 3
    st, Gd, Dd, tr, rng = _gan16(ctx, "create_D16_d", C, B, 7300)
    for net in (st.G, st.D):
        _fill_nontrivial(net, rng)
    Gd.getParameters()[0].copy_(torch.tensor(st.pG)); Dd.getParameters()[0].copy_(torch.tensor(st.pD))
    Gd.device_net.params_changed(); Dd.device_net.params_changed()
    assert tr.gan is not None
    st64 = f64_state(st)
    d, dnG, dnD = ctx.device, Gd.device_net, Dd.device_net
    real = rng.uniform(0, 1, (B // 2, C, 16, 16)).astype(np.float32)
    nz = rng.uniform(-1, 1, (B // 2, 100)).astype(np.float32)
    masks = _masks_for(dnD, B, rng)
    got = tr.step_D(nhwc(real, d), dev(nz, d), [dev(m.reshape(-1), d) for m in masks], keep_grad=True)
    adopt_table_branches(dnD, st.D, also=[st64.D])
    ref = O.step_D(st, real, nz, masks)
    assert_flips_bounded("16px B=128 D-step D", st.D, *table_flips(st.D))
    close(got["outputs"].cpu().numpy().reshape(-1), ref["out"].reshape(-1), atol=1e-5, what="D-step D outputs (16px, B=128)")
    assert abs(got["loss"].item() - ref["f_bce"]) <= 1e-5 * abs(ref["f_bce"])
    gD = got["grad"].cpu().numpy()
    close(gD, ref["grad"], atol=1e-4 * np.abs(ref["grad"]).max() + 1e-7, what="D-step flat gradient (16px, B=128)")
    close_after_first_adam_step(Dd.getParameters()[0].cpu().numpy(), st.pD, gD, ref["grad"], "D params after Adam (16px, B=128)")
    r64 = O.step_D(st64, real.astype(np.float64), nz.astype(np.float64), masks)
    close(gD, r64["grad"], atol=1e-4 * np.abs(r64["grad"]).max() + 1e-7, what="D-step flat gradient vs the float64 oracle")
    check_every_tensor("16px B=128 D-step", gD, st64.D, ref["grad"], floor=floor_for(ctx))
    st64.pG[...] = st.pG; st64.pD[...] = st.pD
    adopt_table_branches(dnD, st.D, also=[st64.D], clear=True)
    Dd.getParameters()[0].copy_(torch.tensor(st.pD)); dnD.params_changed()
    pG_before = dnG.params.clone()
    nz2 = rng.uniform(-1, 1, (B, 100)).astype(np.float32)
    masks2 = _masks_for(dnD, B, rng)
    got = tr.step_G(dev(nz2, d), [dev(m.reshape(-1), d) for m in masks2], keep_grad=True)
    adopt_table_branches(dnD, st.D, also=[st64.D])
    adopt_device_branches(ctx, dnG, st.G, params=pG_before, also=[st64.G])
    ref = O.step_G(st, nz2, masks2)
    assert_flips_bounded("16px B=128 G-step D", st.D, *table_flips(st.D))
    assert_flips_bounded("16px B=128 G-step G", st.G)
    close(nchw(got["samples"]), ref["samples"], atol=1e-5, what="G-step samples (16px, B=128)")
    close(got["outputs"].cpu().numpy().reshape(-1), ref["out"].reshape(-1), atol=1e-5, what="G-step D outputs (16px, B=128)")
    gG = got["grad"].cpu().numpy()
    close(gG, ref["grad"], atol=1e-4 * np.abs(ref["grad"]).max() + 1e-7, what="G-step flat gradient (16px, B=128)")
    r64 = O.step_G(st64, nz2.astype(np.float64), masks2)
    close(gG, r64["grad"], atol=1e-4 * np.abs(r64["grad"]).max() + 1e-7, what="G-step flat gradient vs the float64 oracle")
    check_every_tensor("16px B=128 G-step", gG, st64.G, ref["grad"], floor=floor_for(ctx))


# ---- item 9 ----------------------------------------------------------------------------------------------------------------------
def test_adversarial_train_epoch_at_scale_16(ctx, tmp_path):
    """One `adversarial.train` epoch at 16 px (grayscale, batch 16, the shape of
    tests/test_gpu_train_epoch.py::test_adversarial_train_epoch_config1_gray_batch16) through the fused entries, against
    oracle.train_epoch at that test's bars."""
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.state import S
    B, C, N = 16, 1, 40
    rng = np.random.default_rng(7400)
    G = O.create_G16((C, 16, 16), 100, rng, weight_init_=False)
    D = O.create_D16_d((C, 16, 16), rng)
    st = O.GanState(G, D)
    S.reset()
    adversarial.accs.clear()
    S.OPT.update(batchSize=B, noiseDim=100, N_epoch=51, saveFreq=100, save=str(tmp_path), seed=7, grayscale=True, scale=16)
    S.IMG_DIMENSIONS = (C, 16, 16)
    S.rng = random.Random(7)
    Gd = models.create_G((C, 16, 16), 100)
    Dd = models.create_D((C, 16, 16))
    S.MODEL_G = nn_utils.activateCuda(Gd)
    S.MODEL_D = nn_utils.activateCuda(Dd)
    S.MODEL_G.getParameters()[0].copy_(torch.tensor(st.pG)); S.MODEL_D.getParameters()[0].copy_(torch.tensor(st.pD))
    dnG, dnD = Gd.device_net, Dd.device_net
    dnG.params_changed(); dnD.params_changed()
    data = ListDataset([rng.uniform(0, 1, (C, 16, 16)).astype(np.float32) for _ in range(N)])
    tr = S.trainer()
    assert tr.gan is not None
    rec = Recorder(tr, dnG, dnD)
    max_acc, interval = 0.6, 3
    replay = random.Random(7)
    G_bns = [m for m in st.G.modules if isinstance(m, O.SpatialBatchNormalization)]
    oracle_accs = []
    tV = adversarial.train(data, max_acc, interval)
    steps = rec.steps

    def before_step(kind, k):
        s = steps[k]
        assert s["kind"] == kind, "step %d: device ran a %s-step, the reference loop a %s-step" % (k, s["kind"], kind)
        load_state(st, s["state"], G_bns)

    noise_q = [(s["noise"] if s["noise"] is not None else (s["args"][1] if s["kind"] == "D" else s["args"][0])).reshape(-1, 100) for s in steps]
    mask_q = [s["masks"] for s in steps]
    qi = dict(n=0, m=0)

    def draw_noise(n):
        z = noise_q[qi["n"]]; qi["n"] += 1
        assert z.shape[0] == n
        return z

    def draw_masks(b):
        m = mask_q[qi["m"]]; qi["m"] += 1
        return [mm.reshape(b, -1) for mm in m]

    log = O.train_epoch(st, data, dict(S.OPT), max_acc, interval, oracle_accs, lambda n: replay.randrange(n), draw_noise, draw_masks, before_step)
    assert sum(len(it["D"]) + len(it["G"]) for it in log["iters"]) == len(steps)
    assert [it["batch"] for it in log["iters"]] == [16, 16, 16, 16, 16, 10]
    k = 0
    for it in log["iters"]:
        for r in it["D"]:
            s = steps[k]; k += 1
            close(s["out"], r["out"].reshape(-1), atol=1e-5, what="16px epoch D-step outputs")
            assert abs(s["loss"] - r["f_bce"]) <= 1e-5 * abs(r["f_bce"])
            assert (s["conf"] == r["conf"]).all() and s["trained"] == r["trained"]
        for r in it["G"]:
            s = steps[k]; k += 1
            close(s["samples"], r["samples"], atol=1e-5, what="16px epoch G-step samples")
            close(s["out"], r["out"].reshape(-1), atol=1e-5, what="16px epoch G-step D outputs")
            assert abs(s["loss"] - r["f_bce"]) <= 1e-5 * abs(r["f_bce"])
    assert abs(tV - log["totalValid"]) < 1e-12
    assert adversarial.accs == oracle_accs
    S.reset()
