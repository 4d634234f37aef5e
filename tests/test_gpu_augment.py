"""fg_warp_images on the device (include/facegen_hip.h) and the per-batch augmentation of a set resident in HBM (runtime.Augmenter,
DeviceDataset(augment=)): the kernel against the header's contract restated in numpy fp32 (tests/test_augment_host.py warp_ref),
bit for bit, and against scipy's float64 map_coordinates within a derived bar; against fg_gather_images at the identity; its memory
contract (guards, exact sizes, poison, matrices of NaN / inf / 1e30); DeviceDataset.gather with an augmenter against the restatement
applied to the host copy; and an epoch of adversarial.train on an augmented resident set against the same epoch fed from the host
with images the test warped itself, bit for bit."""
import contextlib
import io
import random

import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, NAN_BITS
from test_augment_host import warp_ref, warp_ref64, fixed_matrices, BAR_64
from test_gpu_dataset import lay, off_by, bits, gather, same_bits, final_state, compare_states, LAYOUTS

pytestmark = pytest.mark.gpu

# (c, hs, ws, ho, wo, n_set): odd sizes, a crop by the matrix alone (40 -> 32), the models' largest image, the LDS limit (4 x 64 x 64)
SHAPES = [(1, 5, 7, 4, 6, 5), (3, 5, 7, 5, 7, 9), (2, 9, 9, 9, 9, 17), (3, 16, 16, 16, 16, 50), (3, 40, 40, 32, 32, 23), (3, 64, 64, 64, 64, 11),
          (4, 64, 64, 32, 32, 6)]
N_OUT = (1, 3, 37)
RESIDUES = ((0, 0), (1, 2), (2, 3), (3, 1))             # floats that the bases of set / out lie behind a 16-byte boundary


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def warp(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, out_dev, ho, wo, ol, fill):
    P = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    ctx.check(ctx.lib.fg_warp_images(ctx.h, P(set_dev), n_set, c, hs, ws, sl, P(idx_dev), P(mats_dev), P(gains_dev), n, P(out_dev), ho, wo, ol, fill))


def images_01(rng, shape):
    """finite pixels in [0, 1], some of them exactly 0 and exactly 1"""
    x = rng.uniform(0, 1, shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, flat.size // 16)] = 0.0
    flat[rng.integers(0, flat.size, flat.size // 16)] = 1.0
    return x


def matrix_pool(hs, ws, ho, wo, seed):
    """the 12 fixed matrices (identity, flips, integer and half-pixel shifts, rotations of 8 and 90 degrees, zoom 0.5 and 2) and 25
    draws of Augmenter with their gains: 37 transforms"""
    from face_generator_amd.runtime import Augmenter
    fixed = fixed_matrices(hs, ws, ho, wo)
    mats, gains = Augmenter((ho, wo), seed=seed).draw(37 - len(fixed), (hs, ws))
    # (gains of at most 1.1, the bar's premise; a pixel of exactly 1 under a gain above 1 meets the clamp)
    g = np.concatenate([np.array([1.0, 0.9, 1.1, 0.0, 1.1, 1.0, 1.05, 0.95, 1.0, 1.1, 0.9, 1.0], dtype=np.float32)[:len(fixed)], gains])
    return np.concatenate([fixed, mats]), g


@pytest.mark.parametrize("c,hs,ws,ho,wo,n_set", SHAPES)
def test_warp_equals_the_fp32_restatement_bit_for_bit(ctx, c, hs, ws, ho, wo, n_set):
    """n in {1, 3, 37} x the four layout pairs x both fills x gains NULL / given x the bases of set and out at every residue of 4
    floats; every call's n transforms are a window of the pool, all 37 at n = 37.  The n = 37 results are also held against the
    float64 reference within BAR_64."""
    rng = np.random.default_rng(100 + c * hs + wo)
    x = images_01(rng, (n_set, c, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, ho, wo, seed=c + hs)
    eo = c * ho * wo
    sets = {(sl, r): off_by(ctx, lay(x, sl), r) for sl in (0, 1) for r in range(4)}
    calls, worst64 = 0, 0.0
    for n in N_OUT:
        for k, fill in enumerate((0, 1)):
            start = (5 * n + 7 * k) % 37
            pick = (start + np.arange(n)) % 37
            mats, g = pool_m[pick], pool_g[pick]
            idx = rng.integers(0, n_set, n).astype(np.int32)
            idx_dev, mats_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, mats, g))
            for gains, gains_dev in ((None, None), (g, g_dev)):
                want = warp_ref(x, idx, mats, gains, ho, wo, fill)
                if n == 37:
                    d = float(np.abs(want.astype(np.float64) - warp_ref64(x, idx, mats, gains, ho, wo, fill)).max())
                    worst64 = max(worst64, d)
                for sl, ol in LAYOUTS:
                    want_bits = bits(lay(want, ol)).reshape(-1)
                    for rs, ro in RESIDUES:
                        out = torch.full((n * eo + ro,), -7.0, device=ctx.device)[ro:]
                        assert out.data_ptr() % 16 == 4 * ro and sets[sl, rs].data_ptr() % 16 == 4 * rs
                        warp(ctx, sets[sl, rs], n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, out, ho, wo, ol, fill)
                        got = bits(out.cpu().numpy())
                        calls += 1
                        if not np.array_equal(got, want_bits):
                            bad = np.nonzero(got != want_bits)[0]
                            raise AssertionError("layouts %d -> %d, fill %d, gains %s, n = %d, set + %d, out + %d floats: %d of %d floats differ "
                                                 "from the restatement, first at %d: %r against %r"
                                                 % (sl, ol, fill, gains is not None, n, rs, ro, bad.size, got.size, bad[0],
                                                    float(got.view(np.float32)[bad[0]]), float(want_bits.view(np.float32)[bad[0]])))
    print("(%d, %dx%d -> %dx%d): %d calls bit-exact; the kernel's values against float64 scipy: worst |difference| %.3g" % (c, hs, ws, ho, wo, calls, worst64))
    assert calls == 3 * 2 * 2 * 4 * 4
    assert worst64 <= BAR_64          # the kernel's bits are the restatement's, so this is the kernel's distance too


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,h,w", [(3, 32, 32), (3, 5, 7), (1, 16, 16), (4, 64, 64)])
def test_the_identity_without_gains_is_the_gather(ctx, sl, ol, c, h, w):
    """mats NULL, and an explicit identity matrix: fg_gather_images bit for bit, for repeated indices and for indices outside the set
    (a NaN image; the set lies between guard bands, its neighbours come out intact)"""
    rng = np.random.default_rng(21)
    n_set = 5
    x = images_01(rng, (n_set, c, h, w))
    idx = np.array([0, 4, 4, -1, 2, n_set, 1, 2 ** 31 - 1, 4, -2 ** 31, 3, 3], dtype=np.int32)
    n, e = idx.size, c * h * w
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (n, 1))
    ar = Arena.sized(ctx.device, [x.size, n, 6 * n, n * e, n * e])
    set_dev = ar.put(lay(x, sl), name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(ident, align=4, name="mats")
    out, ref = ar.take(n * e, name="out"), ar.take(n * e, name="gathered")
    gather(ctx, set_dev, n_set, c, h, w, sl, idx_dev, n, ref, ol)
    want = bits(ref.cpu().numpy()).reshape(n, e)
    for j, i in enumerate(idx.tolist()):
        assert (want[j] == NAN_BITS).all() != (0 <= i < n_set)
    for m in (None, mats_dev):
        for fill in (0, 1):
            out.fill_(-7.0)
            warp(ctx, set_dev, n_set, c, h, w, sl, idx_dev, m, None, n, out, h, w, ol, fill)
            torch.cuda.synchronize()
            ar.assert_guards("fg_warp_images at the identity with indices outside the set")
            got = bits(out.cpu().numpy()).reshape(n, e)
            assert np.array_equal(got, want), "mats %s, fill %d: images %s differ from fg_gather_images" % (
                "NULL" if m is None else "identity", fill, sorted(set(np.nonzero(got != want)[0].tolist())))


WILD = np.array([[np.nan, 0, 0, 0, 1, 0], [1, 0, 0, 0, np.nan, 0], [1, 0, np.inf, 0, 1, 0], [1, 0, 0, 0, 1, -np.inf], [np.inf, 0, 0, 0, 1, 0],
                 [1e30, 0, 1e30, 0, 1, 0], [1, 0, 0, -1e30, 1, -1e30], [1, 0, -1e30, 0, 1, 1e30], [1e30, 1e30, 1e30, 0, 1, 0],
                 [1, 0, 3e9, 0, 1, -3e9], [1, 0, -1, 0, 1, -1], [1, 0, 0.5, 0, 1, 0]], dtype=np.float32)


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,hs,ws,ho,wo,align", [(3, 33, 17, 20, 12, 256), (3, 40, 40, 32, 32, 256), (4, 16, 16, 16, 16, 4), (1, 5, 7, 9, 11, 8),
                                                 (4, 64, 64, 8, 8, 16)])
def test_memory_contract(ctx, sl, ol, c, hs, ws, ho, wo, align):
    """every operand exactly as long as the header says, between guard bands; the bands behind set / idx / mats / gains hold NaN in
    the first run, out holds NaN, 0, 1e30 in turn: nothing outside out is written, the inputs are left alone, the result does not
    depend on what out or the floats behind the inputs held, and it is the restatement's.  Then matrices of NaN, +-inf, +-1e30 and
    3e9 (beyond int32): 0 with fill 0, the clamped tap with fill 1, and the guards stay intact."""
    from face_generator_amd.runtime import Augmenter
    rng = np.random.default_rng(5)
    n_set, n = 9, 12
    x = images_01(rng, (n_set, c, hs, ws))
    idx = np.array([8, 0, 3, 3, 8, 1, 7, 8, 0, 2, 8, 5], dtype=np.int32)
    mats, gains = Augmenter((ho, wo), seed=align).draw(n, (hs, ws))
    ar = Arena.sized(ctx.device, [x.size, n, 6 * n, n, n * c * ho * wo])
    set_dev = ar.put(lay(x, sl), align=align, name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(mats, align=4, name="mats")
    gains_dev = ar.put(gains, align=4, name="gains")
    out = ar.take(n * c * ho * wo, align=align, name="out")
    for fill in (0, 1):
        for m_host in (mats, WILD):
            mats_dev.copy_(torch.as_tensor(m_host))
            for g_host, g_dev in ((gains, gains_dev), (None, None)):
                what = "fg_warp_images %d -> %d (%d, %dx%d -> %dx%d) fill %d%s%s" % (sl, ol, c, hs, ws, ho, wo, fill, " wild matrices" if m_host is WILD else "",
                                                                                  "" if g_host is not None else " no gains")
                (got,) = run_contract(ar, lambda: warp(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, g_dev, n, out, ho, wo, ol, fill),
                                      [set_dev, idx_dev, mats_dev] + ([g_dev] if g_dev is not None else []), [out], what=what)
                want = warp_ref(x, idx, m_host, g_host, ho, wo, fill)
                assert np.array_equal(bits(got.cpu().numpy()), bits(lay(want, ol)).reshape(-1)), what
                if m_host is WILD and fill == 0:
                    assert not want[:10].any() and want[10:].any()      # the first ten read nothing: 0; the last two are ordinary shifts


def test_a_source_image_above_the_lds_limit_is_refused_on_the_device(ctx):
    from face_generator_amd.runtime import FgError
    t = torch.zeros(2 * 16388, device=ctx.device)
    i = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    with pytest.raises(FgError, match="16388"):
        warp(ctx, t, 1, 1, 4, 4097, 1, i, None, None, 1, t[16388:], 4, 4097, 1, 0)


@pytest.mark.parametrize("c,hs,ws,out_hw,fill", [(3, 40, 40, (32, 32), "constant"), (1, 16, 16, (16, 16), "edge"), (3, 33, 17, (20, 12), "constant")])
def test_device_dataset_gather_with_an_augmenter_equals_the_restatement_on_the_host_copy(ctx, c, hs, ws, out_hw, fill):
    from face_generator_amd import ops
    from face_generator_amd.runtime import Augmenter, DeviceDataset
    x = images_01(np.random.default_rng(31), (19, c, hs, ws))
    plain = DeviceDataset(ctx, x)
    ds = DeviceDataset(ctx, x, augment=Augmenter(out_hw, seed=77, fill=fill))
    twin = Augmenter(out_hw, seed=77, fill=fill)
    for picks, layout in (([3, 18, 0, 3, 7], "nhwc"), (list(range(19)), "nchw"), ([5], "nhwc"),
                          (torch.tensor([1, 1, 2], dtype=torch.int32, device=ctx.device), "nchw")):
        got = ds.gather(picks, layout=layout)
        host_picks = picks.tolist() if torch.is_tensor(picks) else picks
        mats, gains = twin.draw(len(host_picks), (hs, ws))
        want = warp_ref(x, host_picks, mats, gains, out_hw[0], out_hw[1], twin.fill_code)
        assert tuple(got.shape) == ((len(host_picks),) + out_hw + (c,) if layout == "nhwc" else (len(host_picks), c) + out_hw)
        same_bits(got.cpu(), torch.as_tensor(lay(want, 0 if layout == "nhwc" else 1)), "gather(%s, %s) under Augmenter(seed=77)" % (host_picks, layout))
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    # the stored images: augment=False, no augmenter, [i] and rows() -- what fg_gather_images gives today
    for stored in (ds.gather([4, 4, 18], augment=False), plain.gather([4, 4, 18])):
        same_bits(stored.cpu(), torch.as_tensor(lay(x[[4, 4, 18]], 0)), "the un-augmented gather")
    same_bits(ds[6], torch.as_tensor(x[6]), "ds[6]")
    same_bits(ds.rows(2, 5).cpu(), torch.as_tensor(x[2:5]), "rows(2, 5)")
    ds.set_augment(None)
    same_bits(ds.gather([9, 0]).cpu(), torch.as_tensor(lay(x[[9, 0]], 0)), "after set_augment(None)")
    # ops.warp_images: the thin wrapper, a set in NHWC, the identity
    idx = torch.tensor([2, 0], dtype=torch.int32, device=ctx.device)
    same_bits(ops.warp_images(torch.as_tensor(lay(x, 0)).to(ctx.device), idx, set_layout="nhwc", out_layout="nchw", ctx=ctx).cpu(), torch.as_tensor(x[[2, 0]]),
              "ops.warp_images at the identity")


# ---------------------------------------------------------------------------------------------------------------------------------
# an epoch on an augmented resident set against the same epoch fed from the host
# ---------------------------------------------------------------------------------------------------------------------------------
class HostWarpedDataset:
    """dataset[i] as the test computes it: image i under the next draw of an Augmenter of its own, warped by the restatement"""

    def __init__(self, images, augmenter):
        self.images, self.aug = images, augmenter

    def size(self):
        return len(self.images)

    def __getitem__(self, i):
        mats, gains = self.aug.draw(1, self.images.shape[2:])
        return warp_ref(self.images, [i], mats, gains, self.aug.out_hw[0], self.aug.out_hw[1], self.aug.fill_code)[0]


def epoch(ctx, px, make_data, tmp_path):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.state import S
    S.reset()
    adversarial.accs.clear()
    S.OPT.update(batchSize=16, noiseDim=100, N_epoch=51, saveFreq=1000, save=str(tmp_path), seed=7, grayscale=True, scale=px, D_iterations=2)
    S.IMG_DIMENSIONS = (1, px, px)
    torch.manual_seed(4100)
    Gd, Dd = models.create_G((1, px, px), 100), models.create_D((1, px, px))
    S.MODEL_G, S.MODEL_D = nn_utils.activateCuda(Gd), nn_utils.activateCuda(Dd)
    S.set_dist(None)
    dnG, dnD = Gd.device_net, Dd.device_net
    start = (dnG.params.cpu(), dnD.params.cpu())
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        adversarial.train(make_data(), 1.01, 3)
    st = final_state(S._trainer, dnG, dnD, text.getvalue())
    st["accs"] = list(adversarial.accs)
    return st, start


@pytest.mark.parametrize("px", [16, 32])
def test_adversarial_train_epoch_on_an_augmented_resident_set_equals_the_host_fed_epoch(ctx, tmp_path, px):
    """grayscale, batch 16, N_epoch = 51 (16 x 5, 10, skip), D_iterations = 2, as tests/test_gpu_dataset.py runs it; the set is stored
    with a margin of 4 px per side and cropped by the matrices.  Fresh nets and the same seeds three times: an augmented
    DeviceDataset, a host dataset whose [i] the test warps itself with the same draws, and the un-augmented DeviceDataset for the
    S.rng picks."""
    from face_generator_amd.runtime import Augmenter, DeviceDataset
    images = images_01(np.random.default_rng(9), (23, 1, px + 8, px + 8))
    aug = Augmenter((px, px), seed=5)
    res, start_r = epoch(ctx, px, lambda: DeviceDataset(ctx, images, augment=aug), tmp_path)
    host, start_h = epoch(ctx, px, lambda: HostWarpedDataset(images, Augmenter((px, px), seed=5)), tmp_path)
    plain, _ = epoch(ctx, px, lambda: DeviceDataset(ctx, images[:, :, 4:-4, 4:-4]), tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    same_bits(start_h[1], start_r[1], "initial D parameters")
    assert host["countTrainedD"] == (12, 12)
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    compare_states(host, res)
    twin = Augmenter((px, px), seed=5)
    twin.draw(2 * (5 * 8 + 5), (px + 8, px + 8))
    assert twin.rng.getstate() == aug.rng.getstate()                       # one transform per real image of the epoch
    assert res["rng"] == plain["rng"] and res["noise_offset"] == plain["noise_offset"]     # the picks are one stream with and without
    assert not torch.equal(res["pD"], plain["pD"])                          # ... and the augmentation did reach the training
