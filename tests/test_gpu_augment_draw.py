"""fg_draw_transforms on the device (include/facegen_hip.h) and runtime.DeviceAugmenter: the kernel against the header's contract
restated in numpy (tests/test_augment_draw_host.py: Philox, picks, the polynomial sin / cos, the float64 matrix), bit for bit; its
memory contract (guards, exact sizes, poison, 4-byte-odd bases, gains NULL); the prefix property across the counter's carry;
DeviceDataset.gather and AugmentedResult.gather_fields with a DeviceAugmenter against fg_warp_images / fg_warp_c2f fed with the
restated matrices; set_state; and an epoch of adversarial.train on a device-drawn augmented resident set against the same epoch fed
from the host with images the test warped itself."""
import contextlib
import io

import numpy as np
import pytest
import torch

import gan_cases as GC
from mem_contract import Arena, run_contract
from test_augment_draw_host import restated, spec_dict, SPECS
from test_augment_host import warp_ref
from test_gpu_dataset import lay, bits, same_bits, final_state, compare_states, LAYOUTS
from test_gpu_augment import images_01

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 255, 256, 257, 1000)             # one block, the block's edge, two blocks, four
OFFSETS = (0, 5, 2 ** 32 - 2, 2 ** 40 + 3)      # the counter's carry into its high word inside a draw, a high word that is set
SEEDS = (43, (0xDEADBEEF << 32) | 0x12345678)
IMAGES = [((32, 32), (32, 32)), ((40, 40), (32, 32)), ((5, 7), (3, 4))]      # source -> output; odd sizes: the integer centre


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def c_spec(spec):
    from face_generator_amd import _lib
    s = _lib.AugmentSpec()
    for k, v in spec.items():
        setattr(s, k, v)
    return s


def draw(ctx, spec, seed, offset, n, src_hw, out_hw, mats, gains):
    import ctypes
    ctx.check(ctx.lib.fg_draw_transforms(ctx.h, ctypes.byref(c_spec(spec)), seed, offset, n, src_hw[0], src_hw[1], out_hw[0], out_hw[1], mats.data_ptr(),
                                         None if gains is None else gains.data_ptr()))


def check(got_m, got_g, want_m, want_g, what):
    for name, got, want in (("mats", got_m, want_m), ("gains", got_g, want_g)):
        if got is None:
            continue
        g, w = bits(got.cpu().numpy()).reshape(-1), bits(want).reshape(-1)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError("%s: %d of %d %s differ from the restatement, first at %d: %r against %r" % (
                what, bad.size, g.size, name, bad[0], float(g.view(np.float32)[bad[0]]), float(w.view(np.float32)[bad[0]])))


@pytest.mark.parametrize("src_hw,out_hw", IMAGES)
@pytest.mark.parametrize("name", sorted(SPECS))
def test_draw_equals_the_restatement_bit_for_bit(ctx, name, src_hw, out_hw):
    """n in {1, 3, 255, 256, 257, 1000} x four offsets, the seed alternating between a small one and one with a high word; gains given,
    at n = 257 also NULL; mats and gains behind a 16-byte boundary by 0 or 1 float"""
    spec, calls = SPECS[name], 0
    for i, n in enumerate(SIZES):
        for k, offset in enumerate(OFFSETS):
            seed, odd = SEEDS[(i + k) % 2], (i + k // 2) % 2
            want_m, want_g = restated(spec, seed, offset, n, src_hw[0], src_hw[1], out_hw[0], out_hw[1])
            for with_gains in ((True, False) if n == 257 else (True,)):
                mats = torch.full((6 * n + 4 + odd,), -7.0, device=ctx.device)[4 + odd:]
                gains = torch.full((n + 4 + odd,), -7.0, device=ctx.device)[4 + odd:] if with_gains else None
                assert mats.data_ptr() % 8 == 4 * odd
                draw(ctx, spec, seed, offset, n, src_hw, out_hw, mats, gains)
                check(mats, gains, want_m, want_g, "%s %s -> %s, n = %d, seed %#x, offset %#x, %s" % (name, src_hw, out_hw, n, seed, offset,
                                                                                                   "gains" if with_gains else "no gains"))
                calls += 1
    assert calls == len(SIZES) * len(OFFSETS) + len(OFFSETS)
    if name == "neutral":
        ident = np.array([1, 0, (src_hw[1] - out_hw[1]) / 2.0, 0, 1, (src_hw[0] - out_hw[0]) / 2.0], dtype=np.float32)
        assert np.array_equal(mats.cpu().numpy().reshape(-1, 6), np.tile(ident, (SIZES[-1], 1))) and bool((gains == 1.0).all())


@pytest.mark.parametrize("n,with_gains", [(1, True), (257, True), (259, False)])
def test_memory_contract(ctx, n, with_gains):
    """mats and gains exactly as long as the header says, at a 4-byte-odd base between guard bands, holding NaN, 0 and 1e30 in turn:
    exactly mats[0 .. 6n) and gains[0 .. n) are written, whatever they held, and they are the restatement's"""
    spec, seed, offset = SPECS["everything"], SEEDS[1], 2 ** 32 - 2
    ar = Arena.sized(ctx.device, [6 * n, n])
    mats = ar.take(6 * n, align=4, name="mats")
    gains = ar.take(n, align=4, name="gains")
    assert mats.data_ptr() % 8 == 4 and gains.data_ptr() % 8 == 4
    outs = [mats, gains] if with_gains else [mats]
    res = run_contract(ar, lambda: draw(ctx, spec, seed, offset, n, (40, 40), (32, 32), mats, gains if with_gains else None), [], outs,
                       what="fg_draw_transforms n = %d%s" % (n, "" if with_gains else ", gains NULL"))
    want_m, want_g = restated(spec, seed, offset, n, 40, 40, 32, 32)
    check(res[0], res[1] if with_gains else None, want_m, want_g, "under the memory contract")
    if not with_gains:                  # the view that was not handed over still holds the arena's pattern
        assert bool((gains.view(torch.int32) == 0x5A5AA5A5).all())


def test_a_draw_is_a_prefix_of_a_longer_one_across_the_counters_carry(ctx):
    spec, seed = SPECS["everything"], SEEDS[1]
    for offset in (2 ** 32 - 2, 2 ** 64 - 4, 7):
        one = torch.empty(7 * 300, device=ctx.device)
        draw(ctx, spec, seed, offset, 300, (40, 40), (32, 32), one[:1800], one[1800:])
        two = torch.empty(7 * 300, device=ctx.device)
        draw(ctx, spec, seed, offset, 257, (40, 40), (32, 32), two[:6 * 257], two[1800:1800 + 257])
        draw(ctx, spec, seed, (offset + 3 * 257) % 2 ** 64, 43, (40, 40), (32, 32), two[6 * 257:1800], two[1800 + 257:])
        same_bits(one.cpu(), two.cpu(), "257 + 43 images against 300 at offset %#x" % offset)


def test_a_draw_above_the_grid_cap_walks_the_grid(ctx):
    """4096 blocks x 256 threads + 259 images: the threads of the first 259 images take a second one each.  Held against two draws
    below the cap (exactly 4096 blocks, and 259 images at offset + 3 x 2^20) by the prefix property, the tail and the images around
    the cap also against the restatement"""
    spec, seed, offset, cap = SPECS["everything"], SEEDS[1], 2 ** 32 - 2, 4096 * 256
    n = cap + 259
    one, two = torch.full((7 * n + 1,), -7.0, device=ctx.device), torch.full((7 * n + 1,), -7.0, device=ctx.device)
    draw(ctx, spec, seed, offset, n, (40, 40), (32, 32), one[:6 * n], one[6 * n:7 * n])
    draw(ctx, spec, seed, offset, cap, (40, 40), (32, 32), two[:6 * cap], two[6 * n:6 * n + cap])
    draw(ctx, spec, seed, offset + 3 * cap, 259, (40, 40), (32, 32), two[6 * cap:6 * n], two[6 * n + cap:7 * n])
    assert bool(torch.equal(one.view(torch.int32), two.view(torch.int32))) and float(one[-1]) == -7.0
    want_m, want_g = restated(spec, seed, offset + 3 * (cap - 300), 559, 40, 40, 32, 32)
    check(one[6 * (cap - 300):6 * n], one[6 * n + cap - 300:7 * n], want_m, want_g, "images 2^20 - 300 .. 2^20 + 259 of one draw")


def test_the_spec_is_refused_on_the_device_as_in_planning(ctx):
    from face_generator_amd.runtime import FgError
    out = torch.full((16,), -7.0, device=ctx.device)
    for bad in (dict(shear_hi=90), dict(zoom_lo=0.0), dict(gain_lo=float("nan")), dict(tx_lo=1, tx_hi=0), dict(hflip=2)):
        with pytest.raises(FgError, match="fg_draw_transforms"):
            draw(ctx, dict(SPECS["defaults"], **bad), 1, 0, 2, (8, 8), (8, 8), out, None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# DeviceAugmenter on the two datasets
# ---------------------------------------------------------------------------------------------------------------------------------
def no_host_draw(monkeypatch):
    """the host paths a gather must not take: Augmenter.draw / draw_one, and DeviceAugmenter.draw (a read-back)"""
    from face_generator_amd import runtime

    def boom(*a, **k):
        raise AssertionError("a host draw inside a gather with a DeviceAugmenter")
    for cls, name in ((runtime.Augmenter, "draw"), (runtime.Augmenter, "matrix"), (runtime.DeviceAugmenter, "draw")):
        monkeypatch.setattr(cls, name, boom)


def no_upload(*a, **k):
    raise AssertionError("a copy or a conversion through torch inside a gather with a DeviceAugmenter and device indices")


def test_device_dataset_gather_with_a_device_augmenter_equals_the_warp_under_the_restated_matrices(ctx, monkeypatch):
    """a set of 7 images of 3 x 6 x 8, batches of 4 x 6, both layouts; every gather is fg_warp_images under the matrices the
    restatement gives for (seed, offset), and the offset moves by 3n.  (The launch list -- the draw kernel, then one warp kernel --
    is read from the planning-only log in tests/test_augment_draw_host.py, the switch being read when the context is created; here
    the host draws are made to raise, and with indices on the device so is every way of torch's to bring host data over.)"""
    from face_generator_amd import ops
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset
    x = images_01(np.random.default_rng(31), (7, 3, 6, 8))
    kw = dict(vflip=True, scale_axis_equally=False, rotation_deg=20, shear_deg=5, translation_x_px=1, translation_y_px=(0, 1), seed=SEEDS[1],
              offset=2 ** 32 - 5)
    aug = DeviceAugmenter((4, 6), **kw)
    spec, offset = spec_dict(aug.spec()), 2 ** 32 - 5
    ds = DeviceDataset(ctx, x, augment=aug)
    no_host_draw(monkeypatch)
    for picks, layout in (([3, 6, 0, 3], "nhwc"), (list(range(7)), "nchw"), ([5], "nhwc"), (torch.tensor([1, 1, 2], dtype=torch.int32, device=ctx.device), "nchw")):
        n = len(picks)
        if torch.is_tensor(picks):          # indices already on the device: the whole gather moves nothing from the host through torch
            with monkeypatch.context() as m:
                for owner, name in ((torch.Tensor, "to"), (torch.Tensor, "cuda"), (torch.Tensor, "copy_"), (torch, "cat"), (torch, "from_numpy"),
                                    (torch, "as_tensor"), (torch, "tensor")):
                    m.setattr(owner, name, no_upload)
                got = ds.gather(picks, layout=layout)
        else:
            got = ds.gather(picks, layout=layout)
        mats, gains = restated(spec, SEEDS[1], offset, n, 6, 8, 4, 6)
        idx = torch.as_tensor(picks, dtype=torch.int32).to(ctx.device)
        want = ops.warp_images(ds.images, idx, torch.as_tensor(mats).to(ctx.device), torch.as_tensor(gains).to(ctx.device), out_hw=(4, 6), out_layout=layout, ctx=ctx)
        assert tuple(got.shape) == ((n, 4, 6, 3) if layout == "nhwc" else (n, 3, 4, 6))
        same_bits(got.cpu(), want.cpu(), "gather(%s, %s) at offset %#x" % (list(picks), layout, offset))
        host = warp_ref(x, [int(i) for i in picks], mats, gains, 4, 6, 0)
        same_bits(got.cpu(), torch.as_tensor(lay(host, 0 if layout == "nhwc" else 1)), "... and the warp's own restatement")
        offset += 3 * n
        assert aug.state() == (SEEDS[1], offset)
    same_bits(ds.gather([4, 4], augment=False).cpu(), torch.as_tensor(lay(x[[4, 4]], 0)), "the stored images")
    assert aug.state() == (SEEDS[1], offset)


def test_gather_fields_with_a_device_augmenter_equals_warp_c2f_under_the_restated_matrices(ctx, monkeypatch):
    """3 x 10 x 10 -> s = 8, cs = 4: both fields of a pull stem from ONE draw, and the offset moves by 3n once"""
    from face_generator_amd import dataset_c2f, ops
    from face_generator_amd.runtime import DeviceAugmenter
    x = images_01(np.random.default_rng(32), (9, 3, 10, 10))
    aug = DeviceAugmenter((8, 8), rotation_deg=30, seed=77, offset=11)
    res = dataset_c2f.toResultAugmented(x, 4, 8, aug, ctx=ctx)
    spec, offset = spec_dict(aug.spec()), 11
    no_host_draw(monkeypatch)
    for picks, fields, layout in (([3, 8, 0, 3, 7], ("diff", "coarse"), "nhwc"), (list(range(9)), ("fine", "coarse", "diff"), "nchw"), ([5], ("coarse",), "nhwc")):
        n = len(picks)
        got = res.gather_fields(picks, fields, layout=layout)
        mats, gains = restated(spec, 77, offset, n, 10, 10, 8, 8)
        idx = torch.as_tensor(picks, dtype=torch.int32).to(ctx.device)
        want = ops.warp_c2f(res.set.images, idx, 8, 4, mats=torch.as_tensor(mats).to(ctx.device), gains=torch.as_tensor(gains).to(ctx.device), fields=fields,
                            out_layout=layout, ctx=ctx)
        for f, g, w in zip(fields, got, want):
            same_bits(g.cpu(), w.cpu(), "gather_fields(%s, %r, %s): %s" % (picks, fields, layout, f))
        offset += 3 * n
        assert aug.state() == (77, offset)
    fine, coarse, diff = (t.cpu().numpy() for t in res.gather_fields([0, 6, 8, 6], ("fine", "coarse", "diff")))
    assert np.array_equal(bits(diff), bits(fine - coarse)) and diff.any() and aug.state() == (77, offset + 12)


def test_set_state_continues_a_run_bit_for_bit(ctx):
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset
    x = images_01(np.random.default_rng(33), (7, 3, 6, 8))
    a = DeviceDataset(ctx, x, augment=DeviceAugmenter((4, 6), seed=9, offset=2 ** 32 - 7))
    first, second = a.gather([0, 1, 2, 3]), a.gather([4, 5, 6, 0])
    b = DeviceDataset(ctx, x, augment=DeviceAugmenter((4, 6), seed=9, offset=2 ** 32 - 7))
    same_bits(b.gather([0, 1, 2, 3]).cpu(), first.cpu(), "the first batch")
    saved = b.augment.state()
    assert saved == (9, 2 ** 32 - 7 + 12)
    c = DeviceDataset(ctx, x, augment=DeviceAugmenter((4, 6)))               # a fresh object, another seed until the state is restored
    c.augment.set_state(*saved)
    same_bits(c.gather([4, 5, 6, 0]).cpu(), second.cpu(), "the second batch after a save and restore into a fresh object")
    assert c.augment.state() == a.augment.state()
    assert not torch.equal(first, a.gather([0, 1, 2, 3]))                   # a fresh transform per pull
    # draw() reads back the numbers draw_device() leaves on the device
    d, e = DeviceAugmenter((4, 6), seed=9, offset=3), DeviceAugmenter((4, 6), seed=9, offset=3)
    both = d.draw_device(ctx, 5, (6, 8)).cpu().numpy()
    mats, gains = e.draw(5, (6, 8), ctx=ctx)
    assert np.array_equal(bits(both[:30].reshape(5, 6)), bits(mats)) and np.array_equal(bits(both[30:]), bits(gains)) and d.state() == e.state() == (9, 18)


# ---------------------------------------------------------------------------------------------------------------------------------
# an epoch of adversarial.train on a small G / D pair of tests/gan_cases.py
# ---------------------------------------------------------------------------------------------------------------------------------
PAIR = GC.BY_NAME["r3-bn-inner-3ch"]             # G: Linear, View(4, 3, 3), BatchNorm, PReLU, conv 4 -> 3, Sigmoid; D: an MLP on 3 x 3 x 3


def sequential(dims, layers):
    """the nn modules of a case's layer list (the kinds PAIR uses)"""
    from face_generator_amd import nn
    net = nn.Sequential()
    for l in layers:
        kind = l[0]
        if kind == "LINEAR":
            net.add(nn.Linear(l[1], l[2]))
        elif kind == "VIEW":
            net.add(nn.View(*[v for v in l[1:] if v]))
        elif kind == "PRELU":
            net.add(nn.PReLU())
        elif kind == "SIGMOID":
            net.add(nn.Sigmoid())
        elif kind == "BATCHNORM":
            net.add(nn.SpatialBatchNormalization(l[1]))
        elif kind == "CONV":
            assert tuple(l[5:]) == (0, 0)
            net.add(nn.SpatialConvolution(l[1], l[2], l[3], l[3], 1, 1, l[4]))
        else:
            raise AssertionError(kind)
    net.input_dims = tuple(dims)
    return net


class HostWarpedDataset:
    """dataset[i] as the test computes it: image i under the next transform of the restated stream, warped by the warp's restatement"""

    def __init__(self, images, spec, seed, offset, out_hw):
        self.images, self.spec, self.seed, self.offset, self.out_hw, self.pulled = images, spec, seed, offset, out_hw, 0

    def size(self):
        return len(self.images)

    def __getitem__(self, i):
        hs, ws = self.images.shape[2:]
        mats, gains = restated(self.spec, self.seed, self.offset, 1, hs, ws, self.out_hw[0], self.out_hw[1])
        self.offset, self.pulled = (self.offset + 3) % 2 ** 64, self.pulled + 1
        return warp_ref(self.images, [i], mats, gains, self.out_hw[0], self.out_hw[1], 0)[0]


def epoch(ctx, make_data, tmp_path):
    from face_generator_amd import nn_utils, adversarial
    from face_generator_amd.state import S
    S.reset()
    adversarial.accs.clear()
    c, h, w = PAIR.ddims
    S.OPT.update(batchSize=PAIR.max_batch, noiseDim=PAIR.gdims[0], N_epoch=20, saveFreq=1000, save=str(tmp_path), seed=7, grayscale=False, scale=h, D_iterations=2)
    S.IMG_DIMENSIONS = (c, h, w)
    torch.manual_seed(4100)
    Gd, Dd = sequential(PAIR.gdims, PAIR.glayers), sequential(PAIR.ddims, PAIR.dlayers)
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


def test_adversarial_train_epoch_on_a_device_drawn_set_equals_the_host_fed_epoch(ctx, tmp_path):
    """batch 6, N_epoch = 20 (6 x 5, then 5 -> 4, then 2: skip), D_iterations = 2; the set is stored with a margin of 1 px per side.
    Fresh nets and the same seeds three times: a DeviceDataset with a DeviceAugmenter, a host dataset whose [i] the test warps itself
    under the restated transform of the same (seed, offset), and the un-augmented DeviceDataset for the S.rng picks.  Parameters,
    BatchNorm buffers, optimizer state, confusion counts: bit for bit."""
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset
    c, h, w = PAIR.ddims
    images = images_01(np.random.default_rng(9), (13, c, h + 2, w + 2))
    kw = dict(rotation_deg=20, translation_x_px=1, translation_y_px=1, seed=5, offset=2 ** 32 - 20)
    aug = DeviceAugmenter((h, w), **kw)
    spec = spec_dict(aug.spec())
    res, start_r = epoch(ctx, lambda: DeviceDataset(ctx, images, augment=aug), tmp_path)
    host_data = HostWarpedDataset(images, spec, 5, 2 ** 32 - 20, (h, w))
    host, start_h = epoch(ctx, lambda: host_data, tmp_path)
    plain, _ = epoch(ctx, lambda: DeviceDataset(ctx, images[:, :, 1:-1, 1:-1]), tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    same_bits(start_h[1], start_r[1], "initial D parameters")
    assert host["countTrainedD"] == (12, 12) and host["bufG"].numel() == 8
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    compare_states(host, res)
    assert host_data.pulled == 2 * (5 * 3 + 2)                              # one transform per real image of the epoch
    assert aug.state() == (5, host_data.offset)
    assert res["rng"] == plain["rng"] and res["noise_offset"] == plain["noise_offset"]     # the picks are one stream with and without
    assert not torch.equal(res["pD"], plain["pD"])                          # ... and the augmentation did reach the training
