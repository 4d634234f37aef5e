import numpy as np
import torch


# The bars of the module-level parity tests (tests/test_gpu_ops.py), named so that tests/test_gpu_memory_contract.py holds the same
# entries to the same bars without restating them.  conv_* / lin / bn_gx / bn_gparam scale with max(1, max|reference|); *_rtol are relative.
BAR = dict(conv_fwd=2e-5, conv_dgrad=2e-5, conv_wgrad=3e-5, conv_bgrad=3e-5, conv_acc=1e-5, lin=2e-5,
           bn_y=2e-5, bn_mean=1e-6, bn_invstd_rtol=2e-6, bn_running_mean=1e-6, bn_running_var_rtol=1e-5, bn_gx=3e-5, bn_gparam=2e-5,
           prelu=1e-6, slope_grad=1e-4, upsample_fwd=0.0, upsample_bwd=1e-6, avgpool_fwd=1e-6, avgpool_bwd=1e-7, sigmoid=1e-6,
           leakyrelu=1e-6,
           wino_fwd=3e-5, wino_dgrad=3e-5, wino_wgrad=4e-5,       # tests/test_gpu_wino.py: the Winograd kernels against the oracle
           bce_loss_rtol=1e-5, bce_grad_atol=1e-7, bce_grad_rtol=1e-5, norms_rtol=1e-5)


def nhwc(a, dev):
    """numpy NCHW -> device NHWC tensor (test plumbing only)."""
    t = torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    return t.permute(0, 2, 3, 1).contiguous() if t.dim() == 4 else t


def nchw(t):
    """device NHWC tensor -> numpy NCHW."""
    if t.dim() == 4:
        t = t.permute(0, 3, 1, 2)
    return t.contiguous().cpu().numpy()


def dev(a, device):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)


def close(a, b, atol, rtol=0.0, what=""):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError("%s: %d/%d elements differ; worst at %s: got %.8g want %.8g (|err| %.3g, max|ref| %.3g)"
                             % (what, bad.sum(), bad.size, i, a[i], b[i], err[i], np.abs(b).max()))


def close_after_first_adam_step(p_dev, p_ref, g_dev, g_ref, what, lr=1e-3, beta2=0.999, eps=1e-8, atol=2e-6):
    """Parameters after the FIRST Adam step from zero state (interruptable_optimizers.lua:72-90): dp = -lr * g / (|g| +
    eps / sqrt(1 - beta2)), i.e. essentially -lr * sign(g).  Where |g| is of the order of eps the step is a steep function
    of g, so two fp32 computations of the same gradient (different summation orders) may legitimately land 1e-6..1e-3 apart
    on that parameter.  Bar: 2e-6 plus exactly the spread the two gradients themselves imply -- this still pins the
    optimizer arithmetic, without demanding bit-equal near-zero gradients."""
    g_dev = np.asarray(g_dev, np.float64); g_ref = np.asarray(g_ref, np.float64)
    e = eps / np.sqrt(1.0 - beta2)
    f = lambda g: g / (np.abs(g) + e)
    tol = atol + 1.01 * lr * np.abs(f(g_dev) - f(g_ref))
    err = np.abs(np.asarray(p_dev, np.float64) - np.asarray(p_ref, np.float64))
    bad = err > tol
    if bad.any():
        i = int(np.argmax(err - tol))
        raise AssertionError("%s: %d/%d parameters differ beyond the Adam-sensitivity bound; worst at %d: |err| %.3g tol %.3g "
                             "(g_dev %.3e g_ref %.3e)" % (what, bad.sum(), bad.size, i, err[i], tol[i], g_dev[i], g_ref[i]))


from oracle.device_branches import adopt_device_branches, count_branch_flips, count_branch_units   # noqa: E402,F401  (shared with smoke())


def oracle_backward_on_device_branches(ctx, dn, net, x, gy, gflat=None, max_flip_frac=1e-5):
    """Small-batch gradient tests (round 5): the device runs first, then the oracle re-runs its forward on the DEVICE's PReLU /
    max-pool branch decisions and takes its backward from there -- the procedure of the BASELINE-size tests.  Before round 5 these
    tests re-drew their inputs until no oracle pre-activation sat within 1e-7 (relative) of a kink; a Winograd contraction rounds
    ~1.7 x more than the direct convolution (tests/test_gpu_wino.py), which that margin does not cover, and a margin that would
    cover it is never met by a million units.  The number of adopted decisions that differ from the oracle's own is asserted
    (<= max(1, 1e-5 of the units)): the hook cannot hide a wrong kernel.  BatchNorm running statistics are restored (the re-run is
    a second train-mode forward).  Returns the oracle's input gradient."""
    from oracle import torch7_nn as O
    bns = [m for m in O.walk_modules(net) if isinstance(m, O.SpatialBatchNormalization)]
    saved = [(m.running_mean.copy(), m.running_var.copy()) for m in bns]
    adopt_device_branches(ctx, dn, net)
    try:
        net.forward(x)
        for m, (rm, rv) in zip(bns, saved):
            m.running_mean, m.running_var = rm, rv
        if gflat is not None:
            gflat[...] = 0
        gin = net.backward(x, gy)
        flips, units = count_branch_flips(net), count_branch_units(net)
    finally:
        adopt_device_branches(ctx, dn, net, clear=True)
    assert flips <= max(1, max_flip_frac * units), "%d of %d PReLU decisions adopted from the device differ from the oracle's" % (flips, units)
    return gin


def assert_net_bars(what, D, y, out, gx, gin, got):
    """The project's net-level bars (tests/test_gpu_net.py:279-297): outputs 1e-5; input gradient 1e-4 max|g| + 1e-7; every parameter
    tensor's gradient 1e-4 max|g_tensor| + 1e-7 (a PReLU slope: + 32 x 6e-8 x the conditioning of its sum), floored at 2e-6 max|g_net|.
    D: the oracle after its backward; y, gx, got: the device's output, input gradient (both shaped like the oracle's) and flat
    parameter gradient."""
    from oracle import torch7_nn as O
    e_out = np.abs(y - out).max()
    e_in = np.abs(gx - gin).max()
    print("%s: output err %.3e (bar 1e-5); input-gradient err %.3e (bar %.3e)" % (what, e_out, e_in, 1e-4 * np.abs(gin).max() + 1e-7))
    ref = np.concatenate([getattr(m, gn).reshape(-1) for (m, pn, gn) in D.parameters()]) if D.parameters() else np.zeros(0)
    off, gmax, rows = 0, (np.abs(ref).max() if ref.size else 0.0), []
    for (m, pn, gn) in D.parameters():
        r = getattr(m, gn).reshape(-1)
        e = np.abs(got[off:off + r.size] - r).max()
        tol = 1e-4 * np.abs(r).max() + 1e-7 + (32 * 6e-8 * getattr(m, "gw_cond", 0.0) if isinstance(m, O.PReLU) else 0.0)
        tol = max(tol, 2e-6 * gmax)
        rows.append((e / tol, "%s %s.%s @%d: err %.3e tol %.3e (max|g_tensor| %.3e, max|g_net| %.3e)" % (what, type(m).__name__, pn, off, e, tol, np.abs(r).max(), gmax)))
        off += r.size
    if rows:
        print("%s: worst parameter tensor: %s" % (what, max(rows)[1]))
    close(y, out, atol=1e-5, what=what + " outputs")
    close(gx, gin, atol=1e-4 * np.abs(gin).max() + 1e-7, what=what + " input gradient")
    bad = [r[1] for r in rows if r[0] > 1]
    assert not bad, "\n".join(bad)


def forward_backward_against_oracle(ctx, what, D, Dd, dims, B, rng, masks):
    """a compiled net (Dd, face_generator_amd.nn) against its float32 oracle D: train forward, backward, evaluate forward"""
    from oracle import torch7_nn as O
    pD, gD = D.getParameters()
    p, g = Dd.getParameters()
    assert p.numel() == pD.size
    p.copy_(torch.tensor(pD)); Dd.device_net.params_changed()
    if masks:
        O.set_dropout_masks(D, masks)
    x = rng.uniform(0, 1, (B,) + tuple(dims)).astype(np.float32)
    out = D.forward(x)
    gy = rng.standard_normal(out.shape).astype(np.float32)
    gD[...] = 0
    gin = D.backward(x, gy)
    dm = [dev(m.reshape(-1), ctx.device) for m in masks]
    y = Dd.device_net.forward(nhwc(x, ctx.device), masks=dm or None, train=True)
    gx = Dd.device_net.backward(dev(gy, ctx.device), param_grads=True, input_grad=True)
    assert_net_bars(what, D, y.cpu().numpy().reshape(out.shape), out, nchw(gx), gin, g.cpu().numpy())
    D.evaluate(); Dd.evaluate()
    close(Dd.device_net.forward(nhwc(x, ctx.device)).cpu().numpy().reshape(out.shape), D.forward(x), atol=1e-5, what=what + " evaluate")
    D.training(); Dd.training()
    return x, gy, dm
