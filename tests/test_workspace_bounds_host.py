"""CPU-only: the size functions of include/facegen_hip.h against the library's own host-side size checks, in a planning-only context
(FG_DEVICE_NONE: no kernel runs, every plan is built and every scratch slice is checked as on the GPU).  A caller that hands an entry
exactly fg_*_workspace_bytes must never see FG_ERR_WORKSPACE -- for any shape, math mode, fusion setting or planning threshold, and
for any batch up to the one a net / step / sampler workspace was sized for.  What the kernels then write into those bytes is checked
on the device (tests/test_gpu_memory_contract.py).  (Like tests/test_sampler_host.py this module uses the process-wide planning-only
context.)"""
import itertools

import pytest
import torch

FG_OK, FG_ERR_UNSUPPORTED, FG_ERR_WORKSPACE = 0, -4, -5
FG_FUSE_ALL = 511

BATCHES = (1, 2, 3, 5, 16, 33, 128)
MAPS = ((2, 2), (3, 3), (4, 4), (6, 5), (5, 7), (8, 8), (16, 16), (17, 13), (32, 32), (31, 33), (64, 32), (64, 64))
CHANNELS = ((1, 64), (3, 64), (4, 128), (3, 128),                      # thin in   (the classes of test_gpu_ops._fuzz_cases)
            (64, 1), (128, 3), (64, 3), (128, 1),                      # thin out
            (64, 64), (64, 128),                                       # 64-wide
            (128, 128), (128, 256), (256, 128), (256, 256), (256, 512),
            (6, 10), (1, 32), (30, 64), (10, 6), (54, 54), (32, 54), (5, 3))      # ragged: a zero-padded copy at the tail of the scratch


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


@pytest.fixture()
def settings(plan_ctx):
    """restores math mode, fusion flags and the Winograd weight-gradient thresholds"""
    lib, h = plan_ctx.lib, plan_ctx.h
    math, fusion = plan_ctx.get_math(), plan_ctx.get_fusion()
    try:
        yield [(m, f, t) for m in (0, 6) for f in (0, fusion, FG_FUSE_ALL) for t in ((0, 0), (1, 1))]
    finally:
        plan_ctx.set_math(math)
        plan_ctx.set_fusion(fusion)
        lib.fg_test_set_wino_wgrad_thresholds(h, 0, 0)


def _apply(ctx, setting):
    m, f, t = setting
    ctx.set_math(m)
    ctx.set_fusion(f)
    ctx.check(ctx.lib.fg_test_set_wino_wgrad_thresholds(ctx.h, *t))


def test_conv2d_entries_accept_exactly_the_stated_workspace(plan_ctx, settings):
    lib, h = plan_ctx.lib, plan_ctx.h
    tok = torch.zeros(64).data_ptr()                      # operand tokens: nothing dereferences them in a planning-only context
    shapes = [(b, hh, ww, ci, co, k, up) for b in BATCHES for (hh, ww) in MAPS for (ci, co) in CHANNELS for k in (3, 5, 7) for up in (0, 1)]
    assert len(shapes) >= 5000
    ran, refused, bad = 0, 0, []
    for setting in settings:
        _apply(plan_ctx, setting)
        for (b, hh, ww, ci, co, k, up) in shapes:
            pad = (k - 1) // 2
            nb = lib.fg_conv2d_workspace_bytes(b, hh, ww, ci, co, k, up)
            rcs = (lib.fg_conv2d_forward(h, tok, tok, tok, tok, b, hh, ww, ci, co, k, pad, up, tok, nb),
                   lib.fg_conv2d_backward_data(h, tok, tok, tok, b, hh, ww, ci, co, k, pad, up, tok, nb),
                   lib.fg_conv2d_backward_weight(h, tok, tok, tok, tok, 0.0, b, hh, ww, ci, co, k, pad, up, tok, nb))
            # a refusal for want of a kernel (a thin layer behind a folded up-sampling, too many fold groups, the thin weight gradient
            # of 4 channels at k > 3) is no statement about sizes; anything else but FG_OK is
            refused += sum(rc == FG_ERR_UNSUPPORTED for rc in rcs)
            ran += sum(rc == FG_OK for rc in rcs)
            if any(rc not in (FG_OK, FG_ERR_UNSUPPORTED) for rc in rcs):
                bad.append(((b, hh, ww, ci, co, k, up), setting, rcs, nb, lib.fg_last_error(h).decode()))
    assert not bad, "%d shape x setting pairs refused exactly fg_conv2d_workspace_bytes (%d passes ran); first: %s" % (len(bad), ran, bad[:5])
    assert ran >= 3 * 4000 * len(settings) and refused < ran, (ran, refused)


def test_linear_entries_accept_exactly_the_stated_workspace(plan_ctx, settings):
    lib, h = plan_ctx.lib, plan_ctx.h
    tok = torch.zeros(64).data_ptr()
    bad, ran = [], 0
    for setting in settings:
        _apply(plan_ctx, setting)
        for b, k, n in itertools.product(BATCHES + (4, 6, 130), (1, 3, 33, 50, 64, 99, 100, 128, 512, 2048, 8192), (1, 7, 10, 64, 128, 256, 512, 1024, 8192)):
            nb = lib.fg_linear_workspace_bytes(b, k, n)
            rcs = (lib.fg_linear_forward(h, tok, tok, tok, tok, b, k, n, tok, nb), lib.fg_linear_backward_data(h, tok, tok, tok, b, k, n, tok, nb),
                   lib.fg_linear_backward_weight(h, tok, tok, tok, tok, 0.0, b, k, n, tok, nb))
            ran += 1
            if rcs != (FG_OK,) * 3:
                bad.append(((b, k, n), setting, rcs, nb, lib.fg_last_error(h).decode()))
    assert not bad, "%d of %d: first %s" % (len(bad), ran, bad[:5])


def _models():
    """every net face_generator_amd/models.py and models_c2f.py can build and compile to one device plan: (name, constructor, input shape
    per sample on the device).  create_D32 has no device plan (tests/test_gpu_branched.py)."""
    from face_generator_amd import models, models_c2f
    out = []
    for c in (3, 1):
        for s in (32, 16):
            out.append(("create_G %dx%dx%d" % (c, s, s), lambda c=c, s=s: models.create_G((c, s, s), 100), (100,)))
        out.append(("create_D32b c%d" % c, lambda c=c: models.create_D32b((c, 32, 32)), (32, 32, c)))
        for name in ("create_D16_d", "create_D16", "create_D16_b", "create_D16_c"):
            out.append(("%s c%d" % (name, c), lambda c=c, name=name: getattr(models, name)((c, 16, 16)), (16, 16, c)))
    for s in (16, 32):
        out.append(("c2f create_G %d" % s, lambda s=s: models_c2f.create_G((3, s, s)), (s, s, 4)))
        out.append(("c2f create_D %d" % s, lambda s=s: models_c2f.create_D((3, s, s)), (s, s, 3)))
    return out


@pytest.mark.parametrize("max_batch", [8, 128])
def test_net_workspace_covers_every_smaller_batch(plan_ctx, max_batch):
    """a workspace of exactly fg_net_workspace_bytes(net, max_batch) takes every batch from 1 to max_batch -- forward in train and in
    evaluate mode, and backward -- and fg_net_workspace_bytes does not shrink as the batch grows"""
    lib = plan_ctx.lib
    bad = []
    for name, make, in_shape in _models():
        dn = make().cuda(plan_ctx, max_batch=max_batch)._inner().device_net
        full = lib.fg_net_workspace_bytes(dn.h, max_batch)
        assert dn.ws.numel() == (full + 3) // 4 and dn.max_batch == max_batch
        prev = 0
        for b in range(1, max_batch + 1):
            nb = lib.fg_net_workspace_bytes(dn.h, b)
            if nb > full or nb < prev:
                bad.append((name, b, "fg_net_workspace_bytes %d; at %d: %d, at %d: %d" % (nb, b - 1, prev, max_batch, full)))
            prev = nb
            x = torch.zeros((b,) + in_shape)
            try:
                dn.forward(x, train=False)
                y = dn.forward(x, train=True)
                dn.backward(torch.zeros_like(y), param_grads=True, input_grad=True)
            except Exception as e:                         # FgError carries the library's message
                bad.append((name, b, str(e)))
            assert dn.max_batch == max_batch               # nothing re-reserved behind the test's back
    assert not bad, "%d failures; first: %s" % (len(bad), bad[:6])


def _pair(ctx, kind, max_batch):
    from face_generator_amd import models, models_c2f
    if kind == "c2f":
        G, D = models_c2f.create_G((3, 16, 16)), models_c2f.create_D((3, 16, 16))
    else:
        s = 16 if kind == "px16" else 32
        G, D = models.create_G((3, s, s), 100), models.create_D((3, s, s))
    return G.cuda(ctx, max_batch=max_batch)._inner().device_net, D.cuda(ctx, max_batch=max_batch)._inner().device_net


@pytest.mark.parametrize("kind,max_batch", [("px32", 8), ("px32", 128), ("px16", 8), ("px16", 128), ("c2f", 8), ("c2f", 128)])
def test_step_workspace_covers_every_smaller_batch(plan_ctx, kind, max_batch):
    from face_generator_amd.runtime import FusedGan
    lib = plan_ctx.lib
    dnG, dnD = _pair(plan_ctx, kind, max_batch)
    table = 1 if kind == "c2f" else 0
    gan = FusedGan(plan_ctx, dnG, dnD, table, max_batch)
    full = lib.fg_gan_workspace_bytes(dnG.h, dnD.h, table, max_batch)
    s, c = dnD.in_h, dnD.in_c
    bad, prev = [], 0
    for b in range(2, max_batch + 1, 2):
        nb = lib.fg_gan_workspace_bytes(dnG.h, dnD.h, table, b)
        if nb > full or nb < prev:
            bad.append((b, "fg_gan_workspace_bytes %d after %d, %d at max_batch" % (nb, prev, full)))
        prev = nb
        img = lambda n: torch.zeros(n, s, s, c)
        try:
            if table:
                gan.step_D(b, img(b // 2), img(b // 2), img(b // 2))
                gan.step_G(b, img(b))
            else:
                gan.step_D(b, img(b // 2))
                gan.step_G(b)
            gan.finish_pending()
        except Exception as e:
            bad.append((b, str(e)))
    assert not bad, "%d failures; first: %s" % (len(bad), bad[:6])


@pytest.mark.parametrize("kind,max_images,chunk", [("px32", 22, 8), ("px32", 22, 6), ("px16", 40, 16), ("px32", 300, 128)])
def test_sampler_workspace_covers_every_smaller_count(plan_ctx, kind, max_images, chunk):
    from face_generator_amd.runtime import Sampler
    lib = plan_ctx.lib
    dnG, dnD = _pair(plan_ctx, kind, chunk)
    dnG.train = dnD.train = False
    sm = Sampler(plan_ctx, dnG, dnD, max_images, chunk)
    full = lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, max_images)
    bad, prev = [], 0
    for n in range(1, max_images + 1):
        nb = lib.fg_sampler_workspace_bytes(dnG.h, dnD.h, n)
        if nb > full or nb < prev:
            bad.append((n, "fg_sampler_workspace_bytes %d after %d, %d at max_images" % (nb, prev, full)))
        prev = nb
        try:
            sm.sample(n)
            sm.score(n, images=torch.zeros(n, dnD.in_h, dnD.in_w, dnD.in_c))
        except Exception as e:
            bad.append((n, str(e)))
    assert not bad, "%d failures; first: %s" % (len(bad), bad[:6])
