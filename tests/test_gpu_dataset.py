"""fg_gather_images on the device (include/facegen_hip.h) and the training set resident in HBM (runtime.DeviceDataset,
dataset_c2f.toResultResident): the gather against numpy indexing and `transpose`, bit for bit; its memory contract (guards, a set at
the very end of its allocation, indices outside the set); and the loops that use it -- adversarial.train, adversarial_c2f.train,
approxParzen, findClosestNeighboursOf -- against the same loops fed from the host, bit for bit: the host-fed loop is the oracle."""
import contextlib
import ctypes
import io
import re

import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, NAN_BITS

pytestmark = pytest.mark.gpu

LAYOUTS = [(1, 0), (0, 1), (1, 1), (0, 0)]            # (set_layout, out_layout); 1 = [c][h][w], 0 = [h][w][c]
CHANNELS = (1, 3, 4, 5)
SIZES = ((1, 1), (5, 7), (16, 16), (32, 32), (33, 17))
N_SET = (1, 7, 40)
N_OUT = (1, 3, 64, 257)


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def lay(x_nchw, layout):
    """[n][c][h][w] numpy -> the array in `layout`"""
    return np.ascontiguousarray(x_nchw if layout == 1 else x_nchw.transpose(0, 2, 3, 1))


def patterns(rng, n_set, n):
    """ascending, reversed, all equal, random with repeats, first-and-last only"""
    asc = np.arange(n) % n_set
    return dict(ascending=asc, reversed=(n_set - 1 - asc), equal=np.full(n, n_set // 2), random=rng.integers(0, n_set, n),
                ends=np.where(np.arange(n) % 2 == 0, 0, n_set - 1))


def off_by(ctx, array, off, dtype=torch.float32):
    """the array on the device, `off` floats behind a 512-byte aligned base (torch's allocations are)"""
    t = torch.as_tensor(array).reshape(-1)
    buf = torch.empty(t.numel() + off, dtype=dtype, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    buf[off:].copy_(t)
    return buf[off:]


def gather(ctx, set_dev, n_set, c, h, w, sl, idx_dev, n, out_dev, ol):
    P = lambda t: t if isinstance(t, int) else t.data_ptr()
    ctx.check(ctx.lib.fg_gather_images(ctx.h, P(set_dev), n_set, c, h, w, sl, P(idx_dev), n, P(out_dev), ol))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("sl,ol", LAYOUTS)
def test_gather_equals_numpy_indexing_bit_for_bit(ctx, sl, ol):
    """every c x (h, w) x n_set x n x index pattern, with the bases of set / out / both one float off 16 bytes: the 4-byte instances
    move the same elements as the 16-byte ones.  The values are distinct per element (a counter) so that any misplaced float shows."""
    rng = np.random.default_rng(31 + 2 * sl + ol)
    calls = 0
    for c in CHANNELS:
        for h, w in SIZES:
            for n_set in N_SET:
                x = (np.arange(n_set * c * h * w, dtype=np.float32) + 0.25).reshape(n_set, c, h, w)
                x[0].reshape(-1)[::3] *= -1.0
                src = lay(x, sl)
                sets = [off_by(ctx, src, 0), off_by(ctx, src, 1)]
                for n in N_OUT:
                    outs = [torch.empty(n * c * h * w + 1, device=ctx.device)[o:] for o in (0, 1)]
                    for name, idx in patterns(rng, n_set, n).items():
                        idx = idx.astype(np.int32)
                        want = bits(lay(x[idx], ol)).reshape(-1)
                        idx_dev = torch.as_tensor(idx).to(ctx.device)
                        for so, oo in ((0, 0), (1, 0), (0, 1), (1, 1)):
                            outs[oo].fill_(-7.0)
                            gather(ctx, sets[so], n_set, c, h, w, sl, idx_dev, n, outs[oo][:n * c * h * w], ol)
                            got = bits(outs[oo][:n * c * h * w].cpu().numpy())
                            calls += 1
                            if not np.array_equal(got, want):
                                bad = np.nonzero(got != want)[0]
                                raise AssertionError("layouts %d -> %d, c = %d, %dx%d, n_set = %d, n = %d, %s, set + %d, out + %d floats: %d of "
                                                     "%d floats differ, first at %d" % (sl, ol, c, h, w, n_set, n, name, so, oo, bad.size, want.size, bad[0]))
    assert calls == 4 * 5 * 3 * 4 * 5 * 4


# The unit of work of one block and pass: a transposing gather takes one LDS tile of one image -- 1024 pixels for c <= 4, 512 for
# c <= 8, 256 above, by up to 32 channels; the row copy takes 4096 floats of one image.  The grids are capped at 4096 blocks.
# 4096 + 259 images of 3 x 5 x 7 floats are one unit each: 259 units lie above the cap.  1500 images of 3 x 47 x 47 (2209 pixels: 3
# tiles each) are 4500 units whose image changes inside a block's walk (4096 is no multiple of 3); 2100 images of 5 x 33 x 17 (561
# pixels: 2 tiles of 512) are 4200; 1100 images of 4 x 40 x 40 floats (6400: 2 units each) do the same to the row copy.
@pytest.mark.parametrize("sl,ol,c,h,w,n", [(1, 0, 3, 5, 7, 4355), (0, 1, 3, 5, 7, 4355), (1, 1, 3, 5, 7, 4355), (1, 0, 3, 47, 47, 1500),
                                           (0, 1, 3, 47, 47, 1500), (1, 0, 5, 33, 17, 2100), (0, 1, 5, 33, 17, 2100),
                                           (0, 0, 4, 40, 40, 1100), (1, 0, 40, 20, 20, 2100), (0, 1, 40, 20, 20, 2100)])
def test_gather_above_the_grid_cap(ctx, sl, ol, c, h, w, n):
    """(the last two cases: 40 channels are two channel chunks of the LDS tile, 400 pixels two tiles of 256: 4 units per image, 8400 units)"""
    rng = np.random.default_rng(77)
    n_set = 37
    x = rng.standard_normal((n_set, c, h, w)).astype(np.float32)
    idx = rng.integers(0, n_set, n).astype(np.int32)
    set_dev, idx_dev = off_by(ctx, lay(x, sl), 0), torch.as_tensor(idx).to(ctx.device)
    out = torch.full((n * c * h * w,), -7.0, device=ctx.device)
    gather(ctx, set_dev, n_set, c, h, w, sl, idx_dev, n, out, ol)
    assert np.array_equal(bits(out.cpu().numpy()), bits(lay(x[idx], ol)).reshape(-1))


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,h,w,align", [(3, 33, 17, 256), (3, 32, 32, 256), (4, 16, 16, 4), (40, 9, 8, 16)])
def test_memory_contract(ctx, sl, ol, c, h, w, align):
    """nothing outside out[0 .. n * c * h * w) is written, set and idx are left alone, and the result does not depend on what out or
    the floats behind set held"""
    rng = np.random.default_rng(5)
    n_set, n = 9, 6
    x = rng.standard_normal((n_set, c, h, w)).astype(np.float32)
    idx = np.array([8, 0, 3, 3, 8, 1], dtype=np.int32)
    ar = Arena.sized(ctx.device, [x.size, n, n * c * h * w])
    set_dev = ar.put(lay(x, sl), align=align, name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    out = ar.take(n * c * h * w, align=align, name="out")
    (got,) = run_contract(ar, lambda: gather(ctx, set_dev, n_set, c, h, w, sl, idx_dev, n, out, ol), [set_dev, idx_dev], [out],
                          what="fg_gather_images %d -> %d (%d, %d, %d)" % (sl, ol, c, h, w))
    assert np.array_equal(bits(got.cpu().numpy()), bits(lay(x[idx], ol)).reshape(-1))


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,h,w", [(3, 32, 32), (3, 33, 17), (1, 16, 16)])
def test_set_at_the_very_end_of_its_allocation(ctx, sl, ol, c, h, w):
    """the set's last float is the last float of an allocation of its own (fg_malloc of a whole number of 2 MiB, not a slice of a
    caching allocator's block): a read behind the set would leave the allocation.  Every index is used, the last image most."""
    rng = np.random.default_rng(6)
    n_set = 11
    x = rng.standard_normal((n_set, c, h, w)).astype(np.float32)
    src = lay(x, sl)
    nbytes = 4 << 20
    whole = ctypes.c_void_p()
    ctx.check(ctx.lib.fg_malloc(ctx.h, nbytes, ctypes.byref(whole)))
    try:
        set_ptr = whole.value + nbytes - src.nbytes
        ctx.check(ctx.lib.fg_h2d(ctx.h, set_ptr, src.ctypes.data, src.nbytes))
        ctx.sync()
        idx = np.array(list(range(n_set)) + [n_set - 1] * 9, dtype=np.int32)
        out = torch.empty(idx.size * c * h * w, device=ctx.device)
        gather(ctx, set_ptr, n_set, c, h, w, sl, torch.as_tensor(idx).to(ctx.device), idx.size, out, ol)
        assert np.array_equal(bits(out.cpu().numpy()), bits(lay(x[idx], ol)).reshape(-1))
    finally:
        ctx.check(ctx.lib.fg_free(ctx.h, whole))


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,h,w", [(3, 32, 32), (3, 5, 7), (1, 16, 16)])
def test_an_index_outside_the_set_gives_a_nan_image_and_intact_neighbours(ctx, sl, ol, c, h, w):
    rng = np.random.default_rng(8)
    n_set = 5
    x = rng.standard_normal((n_set, c, h, w)).astype(np.float32)
    idx = np.array([0, -1, 2, n_set, 1, 2 ** 31 - 1, n_set - 1, -2 ** 31], dtype=np.int32)
    n, e = idx.size, c * h * w
    ar = Arena.sized(ctx.device, [x.size, n, n * e])
    set_dev = ar.put(lay(x, sl), name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    out = ar.take(n * e, name="out")
    out.fill_(-7.0)
    gather(ctx, set_dev, n_set, c, h, w, sl, idx_dev, n, out, ol)
    torch.cuda.synchronize()
    ar.assert_guards("fg_gather_images with indices outside the set")
    got = bits(out.cpu().numpy()).reshape(n, e)
    for j, i in enumerate(idx.tolist()):
        if 0 <= i < n_set:
            assert np.array_equal(got[j], bits(lay(x[i:i + 1], ol)).reshape(-1)), "image %d (index %d)" % (j, i)
        else:
            assert (got[j] == NAN_BITS).all(), "image %d (index %d) is not all quiet NaN" % (j, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# the loops: resident against host-fed, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
class ListDataset:
    def __init__(self, items):
        self.items = items

    def size(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def same_bits(a, b, what):
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        ai, bi = (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(ai, bi), "%s: %d of %d elements differ" % (what, int((ai != bi).sum()), ai.numel())
    else:
        assert a == b, "%s: %r != %r" % (what, a, b)


def final_state(tr, dnG, dnD, text):
    from face_generator_amd.state import S
    tr.finish_pending()
    st = dict(pG=dnG.params.cpu(), pD=dnD.params.cpu(), bufG=dnG.buffers.cpu(), bufD=dnD.buffers.cpu(), confusion=list(S.CONFUSION),
              rng=S.rng.getstate(), noise_offset=S.noise_offset, epoch=S.EPOCH)
    for w in ("D", "G"):
        a = tr.optstate["adam"][w]
        assert a.get("t", 0) > 0 and "m" in a and "v" in a, "the %s optimizer never stepped" % w
        st["t" + w], st["m" + w], st["v" + w] = a["t"], a["m"].cpu(), a["v"].cpu()
    if tr.gan is not None:
        st["steps"] = (tr.gan.steps(0), tr.gan.steps(1))
    m = re.search(r"trained D (\d+) of (\d+) times", text)
    if m:
        st["countTrainedD"] = (int(m.group(1)), int(m.group(2)))
    return st


def compare_states(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        same_bits(a[k], b[k], k)


def adversarial_epoch(ctx, px, C, images, resident, gate, tmp_path):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import DeviceDataset
    from face_generator_amd.state import S
    S.reset()
    adversarial.accs.clear()
    S.OPT.update(batchSize=16, noiseDim=100, N_epoch=51, saveFreq=1000, save=str(tmp_path), seed=7, grayscale=C == 1, scale=px,
                 D_iterations=2)
    S.IMG_DIMENSIONS = (C, px, px)
    torch.manual_seed(4100)
    Gd, Dd = models.create_G((C, px, px), 100), models.create_D((C, px, px))
    S.MODEL_G, S.MODEL_D = nn_utils.activateCuda(Gd), nn_utils.activateCuda(Dd)
    S.set_dist(None)                        # the picks, the noise and the dropout masks keyed by OPT.seed, as a training run does
    dnG, dnD = Gd.device_net, Dd.device_net
    start = (dnG.params.cpu(), dnD.params.cpu())
    data = DeviceDataset(ctx, images) if resident else ListDataset(list(images))
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        adversarial.train(data, gate if gate is not None else 1.01, 3)
    st = final_state(S._trainer, dnG, dnD, text.getvalue())
    st["accs"] = list(adversarial.accs)
    return st, start


@pytest.mark.parametrize("px,C,gate", [(32, 1, None), (32, 1, 0.6), (16, 1, None), (16, 3, 0.6)])
def test_adversarial_train_epoch_resident_equals_host_fed(ctx, tmp_path, px, C, gate):
    """32 px grayscale (G32 + D32b) and the 16-px pair (G16 + create_D16_d), batch 16, N_epoch = 51 (16 x 5, 10, skip), D_iterations = 2,
    once each with the maxAccuracyD gate on (0.6 over the last 3 closures, as tests/test_gpu_train_epoch.py sets it; at 32 px it is asked at
    every closure and lets all 12 updates through, at 16 px RGB it holds 5 of the 12 back): fresh nets, the same seeds, one epoch from a
    host list and one from a DeviceDataset"""
    images = np.random.default_rng(9).uniform(0, 1, (23, C, px, px)).astype(np.float32)
    host, start_h = adversarial_epoch(ctx, px, C, images, False, gate, tmp_path)
    res, start_r = adversarial_epoch(ctx, px, C, images, True, gate, tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    same_bits(start_h[1], start_r[1], "initial D parameters")
    assert "countTrainedD" in host and host["countTrainedD"][1] == 12
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    print("trained D %d of %d times (maxAccuracyD %s)" % (host["countTrainedD"] + (gate,)))
    if (px, C) == (16, 3):
        assert 0 < host["countTrainedD"][0] < 12, "the gate neither held an update back nor let one through"
    compare_states(host, res)


def c2f_setup(ctx, Sz, B, tmp_path):
    from face_generator_amd import models_c2f, adversarial_c2f
    from face_generator_amd.state import S
    S.reset()
    S.OPT.update(batchSize=B, N_epoch=15, D_iterations=2, G_iterations=1, saveFreq=1000, save=str(tmp_path), seed=3,
                 coarseSize=Sz // 2, fineSize=Sz)
    S.IMG_DIMENSIONS = (3, Sz, Sz)
    torch.manual_seed(4200)
    S.MODEL_G = models_c2f.create_G((3, Sz, Sz), cuda=True, max_batch=B)
    S.MODEL_D = models_c2f.create_D((3, Sz, Sz), cuda=True, max_batch=B)
    S.set_dist(None)
    S._trainer = adversarial_c2f.TrainerC2F(ctx, S.MODEL_G, S.MODEL_D, S.OPT)
    return S.MODEL_G.inner.device_net, S.MODEL_D.inner.device_net


def c2f_epoch(ctx, fine, resident, tmp_path):
    from face_generator_amd import adversarial_c2f, dataset_c2f
    from face_generator_amd.state import S
    Sz = fine.shape[-1]
    dnG, dnD = c2f_setup(ctx, Sz, 8, tmp_path)
    start = (dnG.params.cpu(), dnD.params.cpu())
    data = (dataset_c2f.toResultResident if resident else dataset_c2f.toResult)(fine, Sz // 2, Sz, ctx=ctx)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        adversarial_c2f.train(data)
    st = final_state(S._trainer, dnG, dnD, text.getvalue())
    # approxParzen on the trained nets, from the state the epoch left
    adversarial_c2f.best_dist = -1.0        # (no .bestnet from a test)
    with contextlib.redirect_stdout(io.StringIO()):
        st["parzen"] = adversarial_c2f.approxParzen(data, 3, 5)
    st["rng_after_parzen"], st["noise_after_parzen"] = S.rng.getstate(), S.noise_offset
    return st, start, data


def test_c2f_train_epoch_and_parzen_resident_equal_host_fed(ctx, tmp_path):
    """adversarial_c2f.train at S = 16, batch 8, N_epoch = 15 (8, 8, 6, skip), D_iterations = 2, then approxParzen(3, 5)"""
    fine = torch.tensor(np.random.default_rng(10).uniform(0, 1, (11, 3, 16, 16)).astype(np.float32))
    host, start_h, data_h = c2f_epoch(ctx, fine, False, tmp_path)
    res, start_r, data_r = c2f_epoch(ctx, fine, True, tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    assert host["steps"] == (6, 3) if "steps" in host else host["tD"] == 6
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    assert host["parzen"].shape == (3,) and bool((host["parzen"] > 0).all()) and bool((host["parzen"] < 1e9).all())
    compare_states(host, res)
    # the resident sets hold what toResult computed, and [i] hands out the same examples
    for f in ("fine", "coarse", "diff"):
        same_bits(getattr(data_r, f).images.cpu(), getattr(data_h, f), "resident ." + f)
    ex_h, ex_r = data_h[7], data_r[7]
    for f in ("fine", "coarse", "diff"):
        same_bits(getattr(ex_r, f), getattr(ex_h, f), "example ." + f)


@pytest.mark.parametrize("chunk", [7, 64, 299, 300, 8192])
def test_closest_neighbours_over_a_device_dataset_equal_the_host_set(ctx, chunk):
    """300 rows with duplicates and a NaN row, cut unevenly: the same (index, distance) bits as over the host tensor, and the neighbour
    images are the set's rows"""
    from face_generator_amd import nn_utils
    from face_generator_amd.runtime import DeviceDataset
    rng = np.random.default_rng(12)
    N, C, H, W, q = 300, 3, 8, 8, 5
    x = rng.uniform(0, 1, (N, C, H, W)).astype(np.float32)
    x[200] = x[17]; x[250] = x[17]; x[299] = x[3]                       # duplicates: the earliest wins
    x[100, 1, 2, 3] = np.nan                                             # a row that can never win
    queries = x[[17, 3, 100, 120, 299]] + rng.normal(0, 1e-3, (q, C, H, W)).astype(np.float32)
    queries[2] = x[100]; queries[2, 1, 2, 3] = 0.5
    qd = torch.as_tensor(np.ascontiguousarray(queries.transpose(0, 2, 3, 1))).to(ctx.device)
    host_set = torch.as_tensor(x)
    found_h, nb_h = nn_utils.findClosestNeighboursOf(qd, host_set, chunk_rows=chunk, ctx=ctx)
    found_r, nb_r = nn_utils.findClosestNeighboursOf(qd, DeviceDataset(ctx, x), chunk_rows=chunk, ctx=ctx)
    assert [i for i, _ in found_h] == [17, 3, found_h[2][0], 120, 3] and found_h[2][0] != 100
    assert [(i, np.float32(d).view(np.int32)) for i, d in found_h] == [(i, np.float32(d).view(np.int32)) for i, d in found_r]
    assert nb_r.device.type == "cuda" and tuple(nb_r.shape) == (q, C, H, W)
    same_bits(nb_r.cpu(), nb_h, "neighbour images")
    same_bits(nb_r.cpu(), host_set[[i for i, _ in found_r]], "neighbour images against the set's rows")


def test_device_dataset_scales_like_fg_scale_bilinear(ctx):
    from face_generator_amd import ops
    from face_generator_amd.runtime import DeviceDataset
    x = np.random.default_rng(13).uniform(0, 1, (9, 3, 64, 64)).astype(np.float32)
    ds = DeviceDataset(ctx, x, scale=32)
    want = ops.scale_bilinear(torch.as_tensor(x).to(ctx.device), 32, 32, layout="nchw", ctx=ctx)
    assert (ds.size(), ds.c, ds.h, ds.w) == (9, 3, 32, 32)
    same_bits(ds.images.cpu(), want.cpu(), "DeviceDataset(scale = 32)")
    same_bits(ds[4], want[4].cpu(), "ds[4]")
    got = ds.gather([8, 0, 8])
    same_bits(got.cpu(), want[[8, 0, 8]].permute(0, 2, 3, 1).contiguous().cpu(), "gather of the scaled set")
    same_bits(DeviceDataset(ctx, x, scale=64).images.cpu(), torch.as_tensor(x), "scale equal to the size: stored as given")
