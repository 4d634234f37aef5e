"""The sampler level on the device (include/facegen_hip.h: fg_rank_scores, fg_image_grid, fg_sampler_*, fg_sample*) -- sample.lua:80-89
and nn_utils.lua:35-118 without a host round trip:
  * ranking, element for element against numpy.lexsort on the header's tie rule;
  * the display grid against a numpy restatement of the header's description of image.toDisplayTensor (kept below: the `image`
    package is not vendored in the reference -- parity unpinned, like image.scale);
  * images and scores against the oracle nets in evaluate mode (bars of test_gpu_train_epoch.py: 2e-5 / 2e-5);
  * the drawn noise, the identity with the module-level path at equal chunking, the composition of fg_sample, the orders, a caller's
    batch, and that sampling changes nothing the nets own.
Oracle nets: initial weights scaled (G x 2, D x 3) so that the images are not flat grey (std 0.12 .. 0.16) and D's probabilities
spread (n22: 0.88 .. 0.95, n1024: 0.33 .. 0.71, px16: 0.20 .. 0.73) instead of sitting at 0.4979 +- 1e-7, where no ranking could be
compared; BatchNorm running statistics re-drawn.  The seeds were picked on the oracle alone (CPU): its score gap at every tested
top-k boundary is 2.8e-4 or more (n22: 1.6e-3 / 5.4e-3, n1024: 9.1e-4 / 2.8e-4, px16: 5.0e-3 / 1.5e-2), well above the 4e-5 under
which a boundary is not decidable."""
import functools

import numpy as np
import pytest
import torch

from oracle import torch7_nn as O
from gpu_util import nhwc, nchw, dev, close

pytestmark = pytest.mark.gpu

IMG_ATOL = PRED_ATOL = 2e-5
GAP = 4e-5                      # twice the prediction bar: below it the oracle's own top-k boundary is not decidable on the device
CASES = {
    "n22": dict(seed=2310, S=32, N=22, chunk=8, k=10),
    "n1024": dict(seed=2314, S=32, N=1024, chunk=128, k=64),
    "px16": dict(seed=2312, S=16, N=40, chunk=16, k=10),
}


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


# ---- references -------------------------------------------------------------------------------------------------------------------
def ref_order(scores, ascending):
    """the header's rule: (score, index low -> high), -0 == +0, NaN last in both directions"""
    s = np.asarray(scores, np.float32)
    nan = np.isnan(s)
    v = np.where(nan, np.float32(0), s) + np.float32(0)          # -0.0 + 0.0 = +0.0
    return np.lexsort((np.arange(s.size), v if ascending else -v, nan))


def ref_grid(images_nhwc, order, k, nrow, padding, normalize):
    """image.toDisplayTensor{input, nrow, padding} as include/facegen_hip.h states it"""
    sel = images_nhwc[np.asarray(order[:k])] if order is not None else images_nhwc[:k]
    mn, mx = sel.min(), sel.max()
    _, h, w, c = sel.shape
    xmaps = min(nrow, k)
    ymaps = -(-k // xmaps)
    grid = np.full((c, ymaps * (h + padding), xmaps * (w + padding)), mx, np.float32)
    for j in range(k):
        r, col = divmod(j, xmaps)
        y0, x0 = r * (h + padding) + padding // 2, col * (w + padding) + padding // 2
        grid[:, y0:y0 + h, x0:x0 + w] = sel[j].transpose(2, 0, 1)
    if normalize:
        grid = np.zeros_like(grid) if mx == mn else ((grid - mn) / (mx - mn)).astype(np.float32)
    return grid, np.array([mn, mx], np.float32)


def oracle_nets(seed, S):
    rng = np.random.default_rng(seed)
    if S == 32:
        G = O.create_G32((3, S, S), 100, rng, weight_init_=False)
        D = O.create_D32b((3, S, S), rng)
    else:
        G = O.create_G16((3, S, S), 100, rng, weight_init_=False)
        D = O.create_D16_d((3, S, S), rng)
    st = O.GanState(G, D)
    st.pG *= 2.0
    st.pD *= 3.0
    for m in O.walk_modules(G):
        if isinstance(m, O.SpatialBatchNormalization):
            m.running_mean[...] = rng.normal(0, 0.05, m.nf).astype(np.float32)
            m.running_var[...] = rng.uniform(0.5, 1.5, m.nf).astype(np.float32)
    G.evaluate(); D.evaluate()
    return st, rng


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    c = CASES[name]
    st, rng = oracle_nets(c["seed"], c["S"])
    N, bs = c["N"], c["chunk"]
    z = rng.uniform(-1, 1, (N, 100)).astype(np.float32)
    images = np.concatenate([st.G.forward(z[i:i + bs]) for i in range(0, N, bs)])
    preds = np.concatenate([st.D.forward(images[i:i + bs]) for i in range(0, N, bs)]).reshape(-1)
    return dict(st=st, z=z, images=images, preds=preds)


def device_nets(ctx, st, S, max_batch, train=False):
    """the device twins of an oracle pair: same flat parameters, same running statistics"""
    from face_generator_amd import models
    G = models.create_G((3, S, S), 100).cuda(ctx, max_batch=max_batch)
    D = models.create_D((3, S, S)).cuda(ctx, max_batch=max_batch)
    G.getParameters()[0].copy_(torch.tensor(st.pG)); D.getParameters()[0].copy_(torch.tensor(st.pD))
    bns = [m for m in O.walk_modules(st.G) if isinstance(m, O.SpatialBatchNormalization)]
    buf = np.concatenate([np.concatenate([m.running_mean, m.running_var]) for m in bns]).astype(np.float32)
    dnG, dnD = G._inner().device_net, D._inner().device_net
    assert dnG.n_buffers == buf.size
    dnG.buffers.copy_(torch.tensor(buf))
    dnG.params_changed(); dnD.params_changed()
    if train:
        G.training(); D.training()
    else:
        G.evaluate(); D.evaluate()
    return G, D


@functools.lru_cache(maxsize=None)
def device_case(name):
    from face_generator_amd.runtime import get_context, Sampler
    ctx = get_context(0)
    c, o = CASES[name], oracle_case(name)
    G, D = device_nets(ctx, o["st"], c["S"], c["chunk"])
    sm = Sampler(ctx, G._inner().device_net, D._inner().device_net, c["N"], c["chunk"])
    sm.sample(c["N"], noise=dev(o["z"], ctx.device))
    ctx.sync()
    return dict(G=G, D=D, sm=sm, images=nchw(sm.view("IMAGES")), preds=sm.view("PREDS").cpu().numpy().copy(),
                desc=sm.view("ORDER_DESC").cpu().numpy().copy(), asc=sm.view("ORDER_ASC").cpu().numpy().copy())


# ---- ranking ----------------------------------------------------------------------------------------------------------------------
def planted_scores(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-1, 1, n).astype(np.float32)
    for value, share in ((1.0, 0.2), (0.0, 0.08), (-0.0, 0.08)):             # runs of exact ties, D's saturated 1.0f above all
        m = max(1, int(n * share))
        start = int(rng.integers(0, n - m + 1))
        s[start:start + m] = value
        s[rng.integers(0, n, max(1, m // 4))] = value                        # ... and scattered ones
    if n >= 8:
        s[rng.integers(0, n, 3)] = np.nan
        s[rng.integers(0, n)] = np.inf
        s[rng.integers(0, n)] = -np.inf
    return s


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1024, 8192, 8193, 65536])
def test_rank_scores_equals_lexsort(ctx, n):
    lib = ctx.lib
    s = planted_scores(n, 100 + n)
    sd = dev(s, ctx.device)
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), s.view(np.uint32))        # -0.0 and the NaNs arrive as they are
    nbytes = lib.fg_rank_scores_workspace_bytes(n)
    scratch = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=ctx.device)
    for ascending in (0, 1):
        out = torch.full((n + 2,), -7, dtype=torch.int32, device=ctx.device)
        ctx.check(lib.fg_rank_scores(ctx.h, sd.data_ptr(), n, ascending, out.data_ptr() + 4, scratch.data_ptr(), nbytes))
        got = out.cpu().numpy()
        assert got[0] == -7 and got[-1] == -7                                         # nothing outside order_out[0..n-1]
        want = ref_order(s, bool(ascending))
        assert np.array_equal(got[1:-1], want), (n, ascending, np.flatnonzero(got[1:-1] != want)[:5])
    # scratch is optional
    out = torch.empty(n, dtype=torch.int32, device=ctx.device)
    ctx.check(lib.fg_rank_scores(ctx.h, sd.data_ptr(), n, 0, out.data_ptr(), None, 0))
    assert np.array_equal(out.cpu().numpy(), ref_order(s, False))


# ---- grid -------------------------------------------------------------------------------------------------------------------------
GRIDS = [  # (n images, c, h, w, k, nrow, padding, with order, normalize, constant)
    (12, 3, 8, 8, 10, 4, 0, True, 1, False),
    (12, 3, 8, 8, 10, 4, 2, True, 1, False),
    (12, 1, 8, 6, 7, 3, 2, False, 1, False),
    (12, 1, 8, 6, 7, 3, 0, True, 0, False),
    (12, 3, 5, 7, 11, 16, 3, False, 0, False),          # nrow > k: one row of k cells; odd padding
    (9, 3, 4, 4, 9, 3, 2, True, 1, True),               # max == min
    (300, 3, 16, 16, 300, 17, 1, True, 1, False),       # more images than reduction blocks
    (64, 3, 32, 32, 64, 8, 0, True, 1, False),          # sample.lua:87
]


@pytest.mark.parametrize("case", GRIDS, ids=lambda c: "n%d_c%d_%dx%d_k%d_row%d_pad%d_ord%d_norm%d_const%d" % tuple(int(v) for v in c))
def test_image_grid_equals_restatement(ctx, case):
    n, c, h, w, k, nrow, padding, with_order, normalize, constant = case
    rng = np.random.default_rng(7 + n + k + padding)
    imgs = np.full((n, h, w, c), 0.375, np.float32) if constant else rng.normal(0.3, 1.0, (n, h, w, c)).astype(np.float32)
    order = rng.permutation(n).astype(np.int32) if with_order else None
    want, want_mm = ref_grid(imgs, order, k, nrow, padding, normalize)
    xd = dev(imgs, ctx.device)
    od = torch.tensor(order, dtype=torch.int32, device=ctx.device) if with_order else None
    out = torch.full((want.size + 2,), -7.0, dtype=torch.float32, device=ctx.device)
    mm = torch.zeros(2, dtype=torch.float32, device=ctx.device)
    ctx.check(ctx.lib.fg_image_grid(ctx.h, xd.data_ptr(), od.data_ptr() if with_order else None, k, c, h, w, nrow, padding, normalize,
                                    out.data_ptr() + 4, mm.data_ptr()))
    got = out.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    got = got[1:-1].reshape(want.shape)
    assert np.array_equal(mm.cpu().numpy(), want_mm)
    if normalize and not constant:
        ulp = np.spacing(np.abs(want).astype(np.float32))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (err <= ulp).all(), (err.max(), np.unravel_index(np.argmax(err - ulp), err.shape))
        assert got.min() == 0.0 and got.max() == 1.0
    else:
        assert np.array_equal(got, want)
    if constant:
        assert not got.any()
    # minmax_out is optional
    out2 = torch.empty(want.size, dtype=torch.float32, device=ctx.device)
    ctx.check(ctx.lib.fg_image_grid(ctx.h, xd.data_ptr(), od.data_ptr() if with_order else None, k, c, h, w, nrow, padding, normalize,
                                    out2.data_ptr(), None))
    assert np.array_equal(out2.cpu().numpy().reshape(want.shape), got)


# ---- generation and scores --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_images_and_scores_match_the_oracle(ctx, name):
    o, d = oracle_case(name), device_case(name)
    print("%s: oracle images std %.3f, predictions %.4f .. %.4f" % (name, o["images"].std(), o["preds"].min(), o["preds"].max()))
    print("%s: max |image err| %.3g, max |prediction err| %.3g" % (name, np.abs(d["images"] - o["images"]).max(), np.abs(d["preds"] - o["preds"]).max()))
    assert o["images"].std() > 0.05 and o["preds"].std() > 1e-3                       # not a degenerate case
    close(d["images"], o["images"], atol=IMG_ATOL, what="%s: IMAGES (evaluate mode, chunks of %d)" % (name, CASES[name]["chunk"]))
    close(d["preds"], o["preds"], atol=PRED_ATOL, what="%s: PREDS" % name)


def test_drawn_noise_is_fg_rng_uniform(ctx):
    d = device_case("n22")
    sm = d["sm"]
    seed, offset, N = 77, 12345, 22
    sm.set_seed(seed, offset)
    sm.generate(N)
    want = ctx.uniform((N, 100), -1.0, 1.0, seed, offset)
    assert torch.equal(sm.view("NOISE"), want)
    first = sm.view("IMAGES").clone()
    sm.generate(N)                                                                    # the offset advanced like S.next_noise's
    assert torch.equal(sm.view("NOISE"), ctx.uniform((N, 100), -1.0, 1.0, seed, offset + (N * 100 + 3) // 4))
    assert not torch.equal(sm.view("IMAGES"), first)
    sm.set_seed(seed, offset)
    sm.generate(N)
    assert torch.equal(sm.view("IMAGES"), first)
    sm.generate(N, noise=want)                                                        # the caller's noise: same images
    assert torch.equal(sm.view("IMAGES"), first)


def test_identity_with_the_module_level_path(ctx):
    """At equal chunking IMAGES and PREDS are bit for bit what nn_utils.createImagesFromNoise and the prediction loop of
    sortImagesByPrediction give on the same noise; nn_utils.sampleRanked returns them with both rankings."""
    from face_generator_amd import nn_utils
    from face_generator_amd.state import S
    c, o = CASES["n22"], oracle_case("n22")
    N, bs, k = c["N"], c["chunk"], c["k"]
    S.reset()
    S.OPT.update(batchSize=bs, noiseDim=100)
    G, D = device_nets(ctx, o["st"], 32, bs)
    S.MODEL_G, S.MODEL_D = nn_utils.activateCuda(G, max_batch=bs), nn_utils.activateCuda(D, max_batch=bs)
    nn_utils.switchToEvaluationMode()
    S.noise_seed, S.noise_offset = 5, 40
    noise = nn_utils.createNoiseInputs(N)
    imgs = nn_utils.createImagesFromNoise(noise)
    preds = torch.cat([S.MODEL_D.forward(imgs[i:i + bs]).reshape(-1) for i in range(0, N, bs)])
    end_offset = S.noise_offset
    S.noise_offset = 40
    images, best, best_p, worst, worst_p = nn_utils.sampleRanked(N, k)
    assert S.noise_offset == end_offset
    sm = nn_utils.sampler(N)
    assert torch.equal(sm.view("NOISE").cpu(), noise)
    assert torch.equal(images, imgs), "IMAGES differ from createImagesFromNoise"
    assert torch.equal(sm.view("PREDS").cpu(), preds), "PREDS differ from the prediction loop of sortImagesByPrediction"
    p = preds.numpy()
    for got, got_p, asc in ((best, best_p, False), (worst, worst_p, True)):
        order = ref_order(p, asc)[:k]
        assert len(got) == k and got_p == [float(p[i]) for i in order]
        for a, i in zip(got, order):
            assert torch.equal(a, imgs[i])
    S.reset()


def test_fg_sample_is_generate_score_and_two_rankings(ctx):
    d = device_case("n22")
    sm, N = d["sm"], 22
    z = dev(oracle_case("n22")["z"], ctx.device)
    for noise in (z, None):
        sm.set_seed(9, 0)
        sm.sample(N, noise=noise)
        whole = {w: sm.view(w).clone() for w in ("IMAGES", "PREDS", "ORDER_DESC", "ORDER_ASC")}
        for w in whole:
            sm.view(w).fill_(0)
        sm.set_seed(9, 0)
        sm.generate(N, noise=noise)
        sm.score()
        sm.rank(False)
        sm.rank(True)
        for w in whole:
            assert torch.equal(sm.view(w), whole[w]), w


def test_orders_are_sorts_of_the_device_scores_and_agree_with_the_oracle():
    fallbacks, pairs = [], 0
    for name in sorted(CASES):
        c, o, d = CASES[name], oracle_case(name), device_case(name)
        k = c["k"]
        assert np.array_equal(d["desc"], ref_order(d["preds"], False)), name
        assert np.array_equal(d["asc"], ref_order(d["preds"], True)), name
        assert sorted(d["desc"].tolist()) == list(range(c["N"]))
        for which, asc in (("desc", False), ("asc", True)):
            pairs += 1
            want = ref_order(o["preds"], asc)
            gap = abs(float(o["preds"][want[k - 1]]) - float(o["preds"][want[k]]))
            print("%s %s: oracle gap at the k = %d boundary %.3g" % (name, which, k, gap))
            if gap > GAP:
                assert set(d[which][:k].tolist()) == set(want[:k].tolist()), (name, which)
            else:
                fallbacks.append((name, which, gap))
    assert pairs == 6 and len(fallbacks) <= 1, fallbacks


def test_scoring_a_callers_batch(ctx):
    """visualizeProgress scores a batch of its own: the samples with one planted image whose oracle score is known."""
    c, o, d = CASES["n22"], oracle_case("n22"), device_case("n22")
    sm, N, at = d["sm"], 22, 13
    rng = np.random.default_rng(5)
    planted = rng.uniform(0, 1, (1, 3, 32, 32)).astype(np.float32)                    # a synthetic non-face
    batch = o["images"].copy()
    batch[at] = planted[0]
    p_ref = o["preds"].copy()
    # the oracle scores chunk by chunk; in evaluate mode a sample's score does not depend on its neighbours
    p_ref[at] = float(o["st"].D.forward(batch[8:16]).reshape(-1)[at - 8])
    assert abs(p_ref[at] - o["preds"][at]) > 1e-3
    sm.generate(N, noise=dev(o["z"], ctx.device))                                     # (earlier tests drew other images into it)
    own = sm.view("IMAGES").clone()
    sm.score(N, images=nhwc(batch, ctx.device))
    sm.rank(False)
    got = sm.view("PREDS").cpu().numpy()
    close(got, p_ref, atol=PRED_ATOL, what="PREDS of a caller's batch")
    assert abs(got[at] - p_ref[at]) <= PRED_ATOL
    order = sm.view("ORDER_DESC").cpu().numpy()
    want = ref_order(got, False)
    assert np.array_equal(order, want) and int(np.flatnonzero(order == at)[0]) == int(np.flatnonzero(want == at)[0])
    assert torch.equal(sm.view("IMAGES"), own)                                        # the sampler's own images were not touched
    sm.score()                                                                        # back to its own
    assert np.array_equal(sm.view("PREDS").cpu().numpy(), d["preds"])


def test_sampling_leaves_the_nets_alone(ctx):
    """Evaluate mode: parameters and BatchNorm running statistics are bit for bit what they were, and a D-step / G-step pair after
    sampling gives what the same pair gives without it."""
    from face_generator_amd import adversarial
    from face_generator_amd.runtime import Sampler
    o = oracle_case("n22")
    B = 8
    real = ctx.uniform((B // 2, 32, 32, 3), 0.0, 1.0, seed=9)
    outs = []
    for with_sampling in (False, True):
        G, D = device_nets(ctx, o["st"], 32, B, train=True)
        dnG, dnD = G._inner().device_net, D._inner().device_net
        tr = adversarial.Trainer(ctx, G, D, dict(batchSize=B, noiseDim=100))
        assert tr.gan is not None
        tr.gan.set_seeds(3, 0, 777, 0)
        if with_sampling:
            before = [t.clone() for t in (dnG.params, dnD.params, dnG.buffers, dnG.grads, dnD.grads)]
            sm = Sampler(ctx, dnG, dnD, 64, B)
            sm.set_seed(11, 0)
            sm.sample(22)
            imgs = sm.view("IMAGES").clone()
            for a, b in zip(before, (dnG.params, dnD.params, dnG.buffers, dnG.grads, dnD.grads)):
                assert torch.equal(a, b)
            assert float(imgs.std()) > 0.05
        r1 = tr.step_D(real, None)
        d_out, d_loss = r1["outputs"].clone(), r1["loss"].clone()
        r2 = tr.step_G(B)
        tr.finish_pending()
        outs.append(dict(pG=dnG.params.clone(), pD=dnD.params.clone(), bn=dnG.buffers.clone(), d_out=d_out, d_loss=d_loss,
                         g_out=r2["outputs"].clone(), g_loss=r2["loss"].clone(), samples=r2["samples"].clone()))
        if with_sampling:                                                             # and sampling again after training still works
            sm.sample(22)
            assert not torch.equal(sm.view("IMAGES"), imgs)
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), "a step after sampling differs in %s" % key
