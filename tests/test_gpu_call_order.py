"""Call-order independence on the device: a net, a gan or a sampler that has a PAST gives the bits of a fresh twin.  The scenarios live
in tests/call_order.py (shared with the host test, which compares their launch logs); tests/CALL_ORDER.md is the ledger: which state
field of fg_net / Stage / fg_gan / fg_sampler each scenario would see stale.

Reference: the fresh twin (created after the history, under the same creation-time fusion word, bound to copies of the used object's
vectors as they stand, workspaces full of NaN), and bit equality of everything the probe produces -- output, every layer output that
ends a stage, the saved BatchNorm statistics, the running statistics, the input gradient, the flat gradient vector; for a gan both
parameter vectors, both optimizer states, the step counts, loss, confusion counts, D's output and the samples.  The two other bars are
borrowed, not invented: the PReLU slope gradient where a scenario moves a PReLU backward out of its neighbour's epilogue
(2e-3 * scale + 1e-6, tests/test_gpu_fusion.py::prelu_fused_equals_separate) and, for runs whose math mode or fusion word differs from
the reference run BY DESIGN, the per-tensor bar of tests/test_gpu_net.py::check_flat_grads against the all-mode-0 / created-with-the-bit run
(the slope gradients of the nets created without Winograd at the slope bar there: another kernel by design, tests/CALL_ORDER.md)."""
import pytest
import torch

import call_order as CO
from gpu_util import nchw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from face_generator_amd.runtime import get_context
    ctx = get_context(0)
    yield CO.Env(ctx)
    ctx.set_fusion(CO.FG_FUSE_DEFAULT)
    ctx.set_math(0)


@pytest.fixture(autouse=True)
def stop_at_a_device_fault():
    """a mismatch is a finding and the module goes on; a device fault is not run over"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, nothing more is run: %s" % e, returncode=3)


def report(msgs):
    for m in msgs:
        print(m)
    assert not msgs, "%d mismatches against the fresh twin:\n%s" % (len(msgs), "\n".join(msgs[:20]))


def within_flat_grad_bar(env, kind, create_fusion, inp, runs, what, slope_bar=False):
    """`runs` {name: results} against a fresh net of the same creation word run in math mode 0 under the default fusion word, at the
    per-tensor bar of test_gpu_net.check_flat_grads.  The oracle net supplies the tensor boundaries and, from ONE backward on the
    device's PReLU decisions of THIS reference run (this creation word, these inputs: nothing is kept from an earlier call), the
    condition scale of every slope gradient (gw_cond); its gradients are then REPLACED by the device's all-mode-0 ones, which are the
    reference here.
    slope_bar: the PReLU slope gradients are held to 2e-3 * scale + 1e-6 (test_gpu_fusion.py::prelu_fused_equals_separate) instead --
    for the nets created without Winograd, where in mode 6 the gradient every one of those sums is taken over comes out of another
    kernel by design (igemm_ws6_kernel, tests/CALL_ORDER.md); every other tensor keeps the bar of check_flat_grads."""
    from oracle import torch7_nn as O
    from gpu_util import oracle_backward_on_device_branches
    from test_gpu_net import check_flat_grads
    _, onet, gflat = env.base(kind)
    B = inp.x.shape[0]
    with env.fusion(CO.FG_FUSE_DEFAULT if create_fusion is None else create_fusion), env.math(0):
        dn0 = env.net(kind, create_fusion)
        r0 = CO.probe(env, dn0, inp)
        env.ctx.check(CO.forward_rc(dn0, inp))
        if inp.masks:
            O.set_dropout_masks(onet, [m.cpu().numpy().reshape(B, -1) for m in inp.masks])
        oracle_backward_on_device_branches(env.ctx, dn0, onet, nchw(inp.x), nchw(inp.gy), gflat)
    ref = r0["grads"].cpu().numpy()
    gflat[...] = ref
    slopes = CO.slope_indices(dn0) if slope_bar else []
    bad = []
    for name, r in runs.items():
        # (printed with every figure: PReLU inputs on opposite sides of the kink in the two runs, where a layer output shows them)
        flips = sum(int(((r0[k] > 0) != (r[k] > 0)).sum()) for li, l in enumerate(dn0.layers)
                    for k in ["layer%d" % (li - 1)] if l[0] == "PRELU" and k in r0 and k in r)
        dg = (r["grads"] - r0["grads"]).abs()
        print("%s %s, %s: max |grads - reference| %.3e at %d (max |reference| %.3e); %d visible PReLU decisions differ"
              % (kind, what, name, float(dg.max()), int(dg.argmax()), float(r0["grads"].abs().max()), flips))
        got = r["grads"].cpu().numpy().copy()
        for i in slopes:
            a, b = float(got[i]), float(ref[i])
            bar = 2e-3 * max(abs(a), abs(b)) + 1e-6
            print("%s %s, %s: slope gradient at %d: %.8g, reference %.8g, |difference| %.3e (bar %.3e)" % (kind, what, name, i, a, b, abs(a - b), bar))
            if not abs(a - b) <= bar:
                bad.append("%s %s, %s: slope gradient at %d: %.8g vs %.8g (bar %.3g)" % (kind, what, name, i, a, b, bar))
            got[i] = ref[i]                                   # held to the bar above, not to check_flat_grads' as well
        try:
            check_flat_grads(got, onet, "%s %s, %s" % (kind, what, name))
        except AssertionError as e:
            print(e)
            bad.append(str(e))
    return bad


NET_CASES = [(name, k) for name, _, kinds in CO.NET_SCENARIOS for k in kinds]
FN = {name: fn for name, fn, _ in CO.NET_SCENARIOS + CO.GAN_SCENARIOS}


@pytest.mark.parametrize("name,kind", NET_CASES)
def test_net_with_a_past_equals_its_fresh_twin(env, name, kind):
    results = {}
    if name in ("math_mode", "fusion_word"):
        msgs = FN[name](env, kind, results)
    else:
        msgs = FN[name](env, kind)
    report(msgs)
    bad = []
    if kind in ("G32", "D32"):          # the nets test_gpu_net.check_flat_grads knows how to walk
        if name == "math_mode":
            # the nets as every other test creates them, and the nets created without the Winograd bits, where mode 6 really acts:
            # igemm_ws6_kernel reads the weight planes in the forward and in the data gradient (slope bar there, tests/CALL_ORDER.md)
            bad += within_flat_grad_bar(env, kind, None, results[None][1], results[None][2], "math modes switched, created with the default word")
            bad += within_flat_grad_bar(env, kind, CO.NO_WINO, results[CO.NO_WINO][1], results[CO.NO_WINO][2],
                                        "math modes switched, created without Winograd", slope_bar=True)
        if name == "fusion_word":
            dn, inp, r = results["wfinish"]
            bad += within_flat_grad_bar(env, kind, None, inp, {"created without FG_FUSE_WFINISH_BATCH": r}, "fusion word")
    assert not bad, "\n".join(bad)


GAN_CASES = [(name, p) for name, _, pairs in CO.GAN_SCENARIOS for p in pairs if name != "optimizer_moves"]


@pytest.mark.parametrize("name,pair", GAN_CASES)
def test_gan_with_a_past_equals_its_fresh_twin(env, name, pair):
    report(FN[name](env, pair))


@pytest.mark.parametrize("case", range(len(CO.OPT_MOVES)), ids=["math%d-%s" % (c[0], c[2].replace(" ", "_")) for c in CO.OPT_MOVES])
@pytest.mark.parametrize("pair", ["px32", "c2f"])
def test_nets_behind_an_optimizer_update_equal_twins_bound_to_the_vector(env, pair, case):
    report(CO.g08_optimizer_moves(env, pair, [case]))
