"""Grayscale from resident byte sets, on the device: fg_warp_images_u8_y, fg_warp_c2f_u8_y and fg_warp_faces_u8_y
(include/facegen_hip.h) and gray=True of runtime.DeviceDataset / PhotoDataset and the dataset_c2f results.  The decode of R, G, B
bytes against the numpy restatement of Y; every entry against its fp32 sibling at c = 1 on the float set Y(bytes), bit for bit, over
the set layouts, fills, gains, field subsets and the load widths; reads that stay inside the set; indices outside the set and wild
matrices; the classes against their twins; an epoch of adversarial.train and of adversarial_c2f.train on a gray byte photo set
against the same epoch on the float luma set.  There is no tolerance anywhere: every comparison is on int32 bits."""
import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, NAN_BITS
from test_gpu_dataset import lay, bits, same_bits, compare_states
from test_gpu_augment import matrix_pool, WILD, epoch
import test_gpu_augment_c2f
from test_gpu_augment_c2f import c2f_epoch
from test_u8_sets_host import decode
from test_gray_sets_host import luma, luma_set

pytestmark = pytest.mark.gpu

FIELDS = ("fine", "coarse", "diff")
SUBSETS = [("fine",), ("coarse",), ("diff",), ("fine", "coarse"), ("fine", "diff"), ("coarse", "diff"), ("fine", "coarse", "diff")]
N_SET = 5
N_OUT = (1, 3, 37)
RESIDUES = (0, 1, 4)          # bytes that the set's base lies behind a 16-byte boundary: 16-byte loads, byte loads, 4-byte loads
# (hs, ws, ho, wo): a crop by the matrix; 99 pixels, byte loads at any base; 36 pixels, 4-byte but not 16-byte; 16-byte; above the
# 3-channel limit; the limit, more than one round of the copy
IMAGES = [(40, 40, 32, 32), (9, 11, 7, 5), (6, 6, 6, 6), (16, 16, 16, 16), (100, 90, 64, 64), (128, 128, 32, 32)]
# (hs, ws, s, cs); the last is above 64 KB of LDS
C2F = [(40, 40, 32, 16), (9, 11, 4, 2), (128, 128, 64, 32)]
# (hs, ws, hw, ww, s, cs); the last two at n in (1, 37)
FACES = [(40, 40, 32, 32, 32, 16), (9, 11, 7, 5, 4, 2), (20, 20, 8, 8, 16, 0), (97, 131, 84, 84, 64, 32), (250, 250, 84, 84, 32, 16)]


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def P(t):
    return None if t is None else t.data_ptr()


def byte_set(ctx, b, residue, pad=0):
    """the bytes on the device, their base `residue` bytes behind a 16-byte boundary, `pad` further bytes on either side -> (set, buffer)"""
    flat = torch.as_tensor(np.ascontiguousarray(b)).reshape(-1)
    buf = torch.zeros(pad + 16 + flat.numel() + pad + 16, dtype=torch.uint8, device=ctx.device)
    at = (-buf.data_ptr() - pad) % 16 + pad + residue
    view = buf[at:at + flat.numel()]
    assert view.data_ptr() % 16 == residue and at >= pad and at + flat.numel() + pad <= buf.numel()
    view.copy_(flat)
    return view, buf


def random_bytes(rng, shape):
    """random bytes with runs of 0 and 255 mixed in"""
    b = rng.integers(0, 256, shape, dtype=np.uint8)
    flat = b.reshape(-1)
    for v in (0, 255):
        for at in rng.integers(0, flat.size, max(1, flat.size // 64)):
            flat[at:at + int(rng.integers(1, 9))] = v
    return b


class Entry:
    """a _u8_y entry and its fp32 sibling at c = 1 behind one signature: run(luma, set, sl, idx, mats, gains, n, outs, fill) with outs =
    {field: tensor} (fg_warp_images: the field is "fine")"""

    def __init__(self, ctx, name, hs, ws, *sizes, n_set=N_SET):
        self.ctx, self.name, self.hs, self.ws, self.sizes, self.n_set = ctx, name, hs, ws, sizes, n_set
        self.out_hw = sizes[:2] if name == "fg_warp_images" else (sizes[-2], sizes[-2])
        self.fields = ("fine",) if name == "fg_warp_images" or sizes[-1] == 0 else FIELDS
        self.eo = self.out_hw[0] * self.out_hw[1]

    def run(self, y, set_dev, sl, idx, mats, gains, n, outs, fill):
        assert set_dev.dtype == (torch.uint8 if y else torch.float32)
        if y:
            fn = getattr(self.ctx.lib, self.name + "_u8_y")
            head, tail = (self.ctx.h, set_dev.data_ptr(), self.n_set, self.hs, self.ws, sl, P(idx), P(mats), P(gains), n), (fill,)
        else:                               # one channel: the layouts are one order
            fn = getattr(self.ctx.lib, self.name)
            head, tail = (self.ctx.h, set_dev.data_ptr(), self.n_set, 1, self.hs, self.ws, 1, P(idx), P(mats), P(gains), n), (1, fill)
        if self.name == "fg_warp_images":
            rc = fn(*head, P(outs["fine"]), self.sizes[0], self.sizes[1], *tail)
        else:
            rc = fn(*head, *self.sizes, P(outs.get("fine")), P(outs.get("coarse")), P(outs.get("diff")), *tail)
        self.ctx.check(rc)

    def subsets(self):
        return SUBSETS if len(self.fields) == 3 else [("fine",)]


def ibits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the decode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residue", RESIDUES)
@pytest.mark.parametrize("sl", (0, 1))
def test_the_identity_call_decodes_to_the_numpy_luma(ctx, sl, residue):
    """a 3 x 16 x 16 image whose planes are the bytes 0 .. 255 in three different orders, and one with R = G = B, through the copy into
    LDS (fg_warp_images_u8_y), the c2f `fine` field at s = 16 / cs = 8 and the taps from global memory (fg_warp_faces_u8_y with hw = ww
    = s = 16, cs = 0): the numpy Y, all 256 pixels of each"""
    v = np.arange(256, dtype=np.uint8)
    b = np.stack([np.stack([v, v[::-1], (v.astype(np.int32) * 37 + 11).astype(np.uint8)]), np.stack([v, v, v])]).reshape(2, 3, 16, 16)
    assert all(sorted(p.reshape(-1).tolist()) == list(range(256)) for p in b[0]) and len({p.tobytes() for p in b[0]}) == 3
    want = bits(luma_set(b)).reshape(2, 256)
    assert np.array_equal(want[1], bits(luma(v, v, v)))
    set_dev, _ = byte_set(ctx, lay(b, sl), residue)
    lib, h = ctx.lib, ctx.h
    for k in (0, 1):
        idx = torch.full((1,), k, dtype=torch.int32, device=ctx.device)
        for fill in (0, 1):
            outs = [torch.full((256,), -7.0, device=ctx.device) for _ in range(3)]
            ctx.check(lib.fg_warp_images_u8_y(h, set_dev.data_ptr(), 2, 16, 16, sl, idx.data_ptr(), None, None, 1, outs[0].data_ptr(), 16, 16, fill))
            ctx.check(lib.fg_warp_c2f_u8_y(h, set_dev.data_ptr(), 2, 16, 16, sl, idx.data_ptr(), None, None, 1, 16, 8, outs[1].data_ptr(), None, None, fill))
            ctx.check(lib.fg_warp_faces_u8_y(h, set_dev.data_ptr(), 2, 16, 16, sl, idx.data_ptr(), None, None, 1, 16, 16, 16, 0, outs[2].data_ptr(), None,
                                             None, fill))
            for name, out in zip(("fg_warp_images_u8_y", "fg_warp_c2f_u8_y fine", "fg_warp_faces_u8_y"), outs):
                got = bits(out.cpu().numpy())
                bad = np.nonzero(got != want[k])[0]
                assert bad.size == 0, "%s, layout %d, fill %d, base + %d, image %d: %d of the 256 pixels are another float, first %d: %r against %r" % (
                    name, sl, fill, residue, k, bad.size, bad[0], float(got.view(np.float32)[bad[0]]), float(want[k].view(np.float32)[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. bits against the sibling
# ---------------------------------------------------------------------------------------------------------------------------------
def against_the_sibling(ctx, e, window_hw, n_out, seed):
    """n x both fills x mats NULL where the sizes allow it x gains NULL / given x both set layouts x every field subset x the set's
    base at residues 0, 1, 4 of 16.  The sibling runs once per (n, fill, mats, gains), with every field, on the numpy luma"""
    rng = np.random.default_rng(seed)
    hs, ws = e.hs, e.ws
    b = random_bytes(rng, (N_SET, 3, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, window_hw[0], window_hw[1], seed=1 + hs)
    sets8 = {(sl, r): byte_set(ctx, lay(b, sl), r)[0] for sl in (0, 1) for r in RESIDUES}
    set32 = torch.as_tensor(luma_set(b)).to(ctx.device)
    identity_fits = window_hw == (hs, ws)
    calls = 0
    for n in n_out:
        want = {f: torch.empty(n * e.eo, device=ctx.device) for f in e.fields}
        got = {f: torch.empty(n * e.eo, device=ctx.device) for f in e.fields}
        for k, fill in enumerate((0, 1)):
            pick = ((5 * n + 7 * k) % 37 + np.arange(n)) % 37
            idx = torch.as_tensor(rng.integers(0, N_SET, n).astype(np.int32)).to(ctx.device)
            mats, g = (torch.as_tensor(a[pick]).to(ctx.device) for a in (pool_m, pool_g))
            for m in (mats, None) if identity_fits else (mats,):
                for gains in (None, g):
                    for t in want.values():
                        t.fill_(-7.0)
                    e.run(False, set32, 1, idx, m, gains, n, want, fill)
                    assert not any(bool((t == -7.0).any()) for t in want.values()), "the fp32 entry left part of its outputs unwritten"
                    for sl in (0, 1):
                        for sub in e.subsets():
                            for r in RESIDUES:
                                for t in got.values():
                                    t.fill_(-7.0)
                                e.run(True, sets8[sl, r], sl, idx, m, gains, n, {f: got[f] for f in sub}, fill)
                                calls += 1
                                for f in e.fields:
                                    if f not in sub:
                                        assert bool((got[f] == -7.0).all()), "%s_u8_y: %s was not asked for and was written" % (e.name, f)
                                    elif not torch.equal(ibits(got[f]), ibits(want[f])):
                                        bad = torch.nonzero(ibits(got[f]) != ibits(want[f])).reshape(-1)
                                        raise AssertionError(
                                            "%s_u8_y %s, set layout %d, fill %d, mats %s, gains %s, n = %d, fields %s, set + %d bytes: %s: %d of %d floats "
                                            "differ from the fp32 entry on Y, first at %d: %r against %r"
                                            % (e.name, (hs, ws) + e.sizes, sl, fill, m is not None, gains is not None, n, sub, r, f, bad.numel(),
                                               got[f].numel(), int(bad[0]), float(got[f][bad[0]]), float(want[f][bad[0]])))
    per_n = 2 * (2 if identity_fits else 1) * 2 * 2 * len(e.subsets()) * 3
    assert calls == len(n_out) * per_n
    return calls


@pytest.mark.parametrize("hs,ws,ho,wo", IMAGES)
def test_warp_images_u8_y_equals_the_fp32_entry_on_the_luma_bit_for_bit(ctx, hs, ws, ho, wo):
    e = Entry(ctx, "fg_warp_images", hs, ws, ho, wo)
    calls = against_the_sibling(ctx, e, (ho, wo), N_OUT, 500 + hs + wo)
    print("fg_warp_images_u8_y (%dx%d -> %dx%d): %d calls bit-exact" % (hs, ws, ho, wo, calls))


@pytest.mark.parametrize("hs,ws,s,cs", C2F)
def test_warp_c2f_u8_y_equals_the_fp32_entry_on_the_luma_bit_for_bit(ctx, hs, ws, s, cs):
    e = Entry(ctx, "fg_warp_c2f", hs, ws, s, cs)
    calls = against_the_sibling(ctx, e, (s, s), N_OUT, 600 + hs + s)
    print("fg_warp_c2f_u8_y (%dx%d -> %d / %d): %d calls bit-exact" % (hs, ws, s, cs, calls))


@pytest.mark.parametrize("hs,ws,hw,ww,s,cs", FACES)
def test_warp_faces_u8_y_equals_the_fp32_entry_on_the_luma_bit_for_bit(ctx, hs, ws, hw, ww, s, cs):
    e = Entry(ctx, "fg_warp_faces", hs, ws, hw, ww, s, cs)
    calls = against_the_sibling(ctx, e, (hw, ww), (1, 37) if hs * ws > 64 * 64 else N_OUT, 700 + hs + s)
    print("fg_warp_faces_u8_y (%dx%d -> %dx%d -> %d / %d): %d calls bit-exact" % (hs, ws, hw, ww, s, cs, calls))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reads stay inside the set; nothing but the requested outputs is written
# ---------------------------------------------------------------------------------------------------------------------------------
SURROUNDINGS = (0x00, 0xFF, None)         # what the bytes in front of and behind the set hold in run 1, 2, 3 (None: a pattern)


@pytest.mark.parametrize("residue", RESIDUES)
@pytest.mark.parametrize("h,w", [(7, 5), (128, 128)])
@pytest.mark.parametrize("name", ["fg_warp_images", "fg_warp_c2f", "fg_warp_faces"])
def test_reads_stay_inside_the_set_and_writes_inside_the_outputs(ctx, name, h, w, residue):
    """the set lies inside a larger byte buffer whose other bytes change from run to run (0x00, 0xFF, a pattern): a wide load over the
    tail of the last image, or in front of the first, would enter the luma.  The outputs lie in an Arena between guard bands and hold
    NaN, 0 and 1e30 before the three runs (run_contract): the runs agree bit for bit, they are the sibling's bits, the guards and
    the inputs are intact, and a field that was not asked for does not exist for the entry.  35 pixels per image (byte loads at any
    base) and 16384 (16-byte, byte and 4-byte loads at residues 0, 1 and 4)."""
    s = min(h, w, 64)                       # the c2f fields are square: 5 of 7 x 5, 64 of 128 x 128
    sizes = dict(fg_warp_images=(h, w), fg_warp_c2f=(min(h, w), 2), fg_warp_faces=(h, w, s, 2))[name]
    n_set = 3
    e = Entry(ctx, name, h, w, *sizes, n_set=n_set)
    rng = np.random.default_rng(h + residue)
    b = rng.integers(0, 256, (n_set, 3, h, w), dtype=np.uint8)
    idx = np.array([n_set - 1, 0, n_set - 1, 1, 0, n_set - 1], dtype=np.int32)         # the first image and the last: the set's two ends
    n = idx.size
    window = sizes[:2] if name != "fg_warp_c2f" else (sizes[0], sizes[0])
    pool_m, pool_g = matrix_pool(h, w, window[0], window[1], seed=3)
    pad = 4096
    asked = ("fine",) if name == "fg_warp_images" else ("fine", "diff") if name == "fg_warp_c2f" else ("coarse",)
    ar = Arena.sized(ctx.device, [n, 6 * n, n] + [n * e.eo] * len(asked))
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(pool_m[:n], align=4, name="mats")
    gains_dev = ar.put(pool_g[:n], align=4, name="gains")
    outs = {f: ar.take(n * e.eo, align=4, name=f) for f in asked}
    set32 = torch.as_tensor(luma_set(b)).to(ctx.device)
    for sl in (0, 1):
        set8, buf = byte_set(ctx, lay(b, sl), residue, pad=pad)
        lo = set8.data_ptr() - buf.data_ptr()
        pattern = torch.as_tensor(rng.integers(1, 255, buf.numel(), dtype=np.uint8)).to(ctx.device)
        for m, g in ((mats_dev, gains_dev), (None, None)) if window == (h, w) else ((mats_dev, gains_dev),):
            run = [0]

            def call():
                keep = set8.clone()
                around = SURROUNDINGS[run[0] % 3]
                if around is None:
                    buf.copy_(pattern)
                else:
                    buf.fill_(around)
                set8.copy_(keep)
                run[0] += 1
                e.run(True, set8, sl, idx_dev, m, g, n, outs, 0)
            what = "%s_u8_y layout %d (%dx%d) set + %d bytes" % (name, sl, h, w, residue)
            got = run_contract(ar, call, [idx_dev, mats_dev, gains_dev], [outs[f] for f in asked], what=what)
            assert run[0] == 3
            assert torch.equal(buf[lo:lo + b.size].cpu(), torch.as_tensor(lay(b, sl)).reshape(-1)), what + ": the set was written"
            assert torch.equal(buf[:lo], pattern[:lo]) and torch.equal(buf[lo + b.size:], pattern[lo + b.size:]), what + ": the bytes around the set were written"
            want = {f: torch.empty(n * e.eo, device=ctx.device) for f in asked}
            e.run(False, set32, 1, idx_dev, m, g, n, want, 0)
            for f, t in zip(asked, got):
                assert torch.equal(ibits(t), ibits(want[f])), "%s: %s differs from the fp32 entry" % (what, f)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. hostile inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sl", (0, 1))
@pytest.mark.parametrize("name,sizes", [("fg_warp_images", (40, 40, 32, 32)), ("fg_warp_c2f", (40, 40, 32, 16)), ("fg_warp_faces", (97, 131, 84, 84, 32, 16))])
def test_indices_outside_the_set_give_nan_images_and_wild_matrices_give_what_the_sibling_gives(ctx, name, sizes, sl):
    """indices -1 and n_set: a quiet-NaN image in every requested field, the neighbours intact (the set lies inside a buffer of 0xFF:
    read, the bytes behind it would be white).  Matrices of NaN, +-inf, +-1e30 and 3e9: the sibling's bits, for both fills."""
    e = Entry(ctx, name, *sizes)
    hs, ws = sizes[:2]
    rng = np.random.default_rng(17)
    b = rng.integers(0, 256, (N_SET, 3, hs, ws), dtype=np.uint8)
    set8, buf = byte_set(ctx, lay(b, sl), 4, pad=4096)
    keep = set8.clone()
    buf.fill_(0xFF)
    set8.copy_(keep)
    set32 = torch.as_tensor(luma_set(b)).to(ctx.device)
    window = sizes[2:4] if name != "fg_warp_c2f" else (sizes[2], sizes[2])
    pool_m, pool_g = matrix_pool(hs, ws, window[0], window[1], seed=11)
    idx = np.array([0, -1, 4, N_SET, 2, 2, -2 ** 31, 1, 2 ** 31 - 1, 3, 4, 0], dtype=np.int32)
    n = idx.size
    assert n == len(WILD)
    idx_dev = torch.as_tensor(idx).to(ctx.device)
    inside = torch.as_tensor(np.clip(idx, 0, N_SET - 1)).to(ctx.device)
    g = torch.as_tensor(pool_g[:n]).to(ctx.device)
    for fill in (0, 1):
        for what, i_dev, m_host in (("indices outside the set", idx_dev, pool_m[:n]), ("wild matrices", inside, WILD)):
            m = torch.as_tensor(np.ascontiguousarray(m_host, dtype=np.float32)).to(ctx.device)
            for gains in (g, None):
                for sub in e.subsets():
                    got = {f: torch.full((n * e.eo,), -7.0, device=ctx.device) for f in sub}
                    want = {f: torch.full((n * e.eo,), -7.0, device=ctx.device) for f in sub}
                    e.run(True, set8, sl, i_dev, m, gains, n, got, fill)
                    e.run(False, set32, 1, i_dev, m, gains, n, want, fill)
                    for f in sub:
                        tag = "%s_u8_y layout %d fill %d, %s, gains %s, %s" % (name, sl, fill, what, gains is not None, f)
                        rows = ibits(got[f]).reshape(n, e.eo)
                        if i_dev is idx_dev:
                            for j, i in enumerate(idx.tolist()):
                                assert bool((rows[j] == NAN_BITS).all()) != (0 <= i < N_SET), "%s: image %d (index %d)" % (tag, j, i)
                        assert torch.equal(ibits(got[f]), ibits(want[f])), "%s differs from the fp32 entry" % tag


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the classes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_classes_on_gray_sets_hand_out_the_bits_of_a_one_channel_set(ctx):
    """DeviceDataset, PhotoDataset, AugmentedResult and PhotoResult three times each -- storage="u8", gray=True on the bytes,
    storage="f32", gray=True on b / 255, and the ordinary one-channel set built from the numpy luma -- under DeviceAugmenters at one
    (seed, offset): gathers, gather_fields, rows and ds[i]"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset, PhotoDataset
    rng = np.random.default_rng(41)
    b = random_bytes(rng, (9, 3, 40, 40))
    x, y = decode(b), luma_set(b)
    picks = [3, 8, 0, 3, 7]
    dev_picks = torch.tensor([1, 1, 2], dtype=torch.int32, device=ctx.device)
    KW = (("u8 gray", b, dict(storage="u8", gray=True)), ("f32 gray", x, dict(storage="f32", gray=True)), ("luma", y, {}))

    def aug(hw):
        a = DeviceAugmenter(hw, seed=77)
        a.set_state(77, 30)
        return a

    def agree(what, call):
        """call(object) -> a tensor or a sequence of tensors: the three objects give the same bits"""
        res = [call(o) for o in what[1]]
        res = [[r] if torch.is_tensor(r) else list(r) for r in res]
        for tag, r in zip(("u8 gray", "f32 gray"), res[:2]):
            assert len(r) == len(res[2])
            for k, (got, want) in enumerate(zip(r, res[2])):
                same_bits(got.cpu(), want.cpu(), "%s, %s against the luma set, result %d" % (what[0], tag, k))
    # DeviceDataset
    sets = [DeviceDataset(ctx, v, augment=aug((32, 32)), **kw) for _, v, kw in KW]
    assert sets[0].images.dtype == torch.uint8 and sets[0].images.numel() == b.size and [s.c for s in sets] == [1, 1, 1]
    assert [s.set_c for s in sets] == [3, 3, 1] and tuple(sets[1].images.shape) == (9, 1, 40, 40)
    same_bits(sets[1].images.cpu(), torch.as_tensor(y), "the luma formed at construction")
    for p, layout in ((picks, "nhwc"), (list(range(9)), "nchw"), ([5], "nhwc"), (dev_picks, "nchw")):
        agree(("DeviceDataset.gather(%s, %s)" % (p, layout), sets), lambda d: d.gather(p, layout=layout))
        agree(("the un-augmented gather", sets), lambda d: d.gather(p, layout=layout, augment=False))
    assert sets[0].augment.state() == sets[2].augment.state() == sets[1].augment.state() != (77, 30)
    out = ctx.empty(2, 40, 40, 1)
    assert sets[0].gather([4, 6], out=out, augment=False).data_ptr() == out.data_ptr()
    same_bits(out.cpu(), torch.as_tensor(lay(y[[4, 6]], 0)), "gather(out=): the luma itself")
    agree(("ds[6]", sets), lambda d: d[6])
    same_bits(sets[0][6], torch.as_tensor(y[6]), "ds[6]")
    agree(("rows(2, 5)", sets), lambda d: d.rows(2, 5).contiguous())
    same_bits(sets[0].rows(0, 9).cpu(), torch.as_tensor(y), "rows(0, 9)")
    # PhotoDataset
    photos = [PhotoDataset(ctx, v, (24, 24), 16, augment=aug((24, 24)), **kw) for _, v, kw in KW]
    assert photos[0].photos.dtype == torch.uint8 and [s.c for s in photos] == [1, 1, 1]
    for p, layout in ((picks, "nhwc"), (dev_picks, "nchw")):
        agree(("PhotoDataset.gather(%s, %s)" % (p, layout), photos), lambda d: d.gather(p, layout=layout))
        for fields in (("diff", "coarse"), ("fine", "coarse", "diff"), ("coarse",)):
            agree(("PhotoDataset.gather_fields(%s)" % (fields,), photos), lambda d: d.gather_fields(p, fields, coarse_scale=8, layout=layout))
    assert photos[0].augment.state() == photos[2].augment.state()
    agree(("photos[6]", photos), lambda d: d[6])
    agree(("PhotoDataset.rows(4, 9)", photos), lambda d: d.rows(4, 9))
    agree(("the un-augmented pull", photos), lambda d: d.gather([4, 4, 6], augment=False))
    # AugmentedResult and PhotoResult
    aug_res = [dataset_c2f.toResultAugmented(v, 16, 32, aug((32, 32)), ctx=ctx, **kw) for _, v, kw in KW]
    photo_res = [dataset_c2f.toResultPhotos(v, (24, 24), 8, 16, aug((24, 24)), ctx=ctx, **kw) for _, v, kw in KW]
    assert aug_res[0].set.images.dtype == torch.uint8 and photo_res[0].set.photos.dtype == torch.uint8
    for res, what in ((aug_res, "AugmentedResult"), (photo_res, "PhotoResult")):
        for p, layout in ((picks, "nhwc"), (dev_picks, "nchw")):
            for fields in (("diff", "coarse"), ("fine",), ("fine", "coarse", "diff")):
                agree(("%s.gather_fields(%s, %s)" % (what, p, fields), res), lambda r: r.gather_fields(p, fields, layout=layout))
            agree((what + ".gather", res), lambda r: r.gather(p, "diff", layout=layout))
        agree((what + "[4]", res), lambda r: [getattr(r[4], f) for f in FIELDS])
        assert res[0].augment.state() == res[2].augment.state()


def test_nearest_search_streams_a_gray_byte_set_chunk_by_chunk(ctx):
    """rows(lo, hi) of a gray byte set are device floats of one channel, so findClosestNeighboursOf works on it as on the float set"""
    from face_generator_amd import nn_utils
    from face_generator_amd.runtime import DeviceDataset
    rng = np.random.default_rng(8)
    b = rng.integers(0, 256, (37, 3, 16, 16), dtype=np.uint8)
    y = luma_set(b)
    queries = (torch.as_tensor(lay(y[[5, 30, 11]], 0)) + 0.001).to(ctx.device)         # device NHWC
    found8, near8 = nn_utils.findClosestNeighboursOf(queries, DeviceDataset(ctx, b, storage="u8", gray=True), chunk_rows=10, ctx=ctx)
    found32, near32 = nn_utils.findClosestNeighboursOf(queries, DeviceDataset(ctx, y), chunk_rows=10, ctx=ctx)
    assert [i for i, _ in found8] == [5, 30, 11] and found8 == found32          # indices and distances, float for float
    same_bits(near8.cpu(), near32.cpu(), "the neighbours")
    same_bits(near8.cpu(), torch.as_tensor(y[[5, 30, 11]]), "the neighbours are the luma images")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. epochs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adversarial_train_epoch_on_a_gray_byte_photo_set_equals_the_epoch_on_the_luma_set(ctx, tmp_path):
    """grayscale 32 x 32, batch 16, N_epoch = 51, D_iterations = 2, as tests/test_gpu_augment.py runs it, on RGB photos of 56 x 60 with
    a face window of 40 x 40: fresh nets and the same seeds twice, once on the R, G, B bytes and once on their float luma"""
    from face_generator_amd.runtime import Augmenter, PhotoDataset
    b = np.random.default_rng(9).integers(0, 256, (23, 3, 56, 60), dtype=np.uint8)
    aug8, aug32 = Augmenter((40, 40), seed=5), Augmenter((40, 40), seed=5)
    made = []

    def make(photos, aug, **kw):
        made.append(PhotoDataset(ctx, photos, (40, 40), 32, augment=aug, **kw))
        return made[-1]
    u8, start8 = epoch(ctx, 32, lambda: make(b, aug8, storage="u8", gray=True), tmp_path)
    f32, start32 = epoch(ctx, 32, lambda: make(luma_set(b), aug32), tmp_path)
    assert made[0].photos.dtype == torch.uint8 and made[0].c == 1 and made[1].photos.dtype == torch.float32 and made[1].c == 1
    same_bits(start32[0], start8[0], "initial G parameters")
    same_bits(start32[1], start8[1], "initial D parameters")
    assert f32["countTrainedD"] == (12, 12)
    assert not torch.equal(f32["pD"], start32[1]) and not torch.equal(f32["pG"], start32[0])
    compare_states(f32, u8)
    assert aug8.rng.getstate() == aug32.rng.getstate()


def gray_c2f_setup(ctx, Sz, B, tmp_path):
    """test_gpu_dataset.c2f_setup with one-channel nets"""
    from face_generator_amd import models_c2f, adversarial_c2f
    from face_generator_amd.state import S
    S.reset()
    S.OPT.update(batchSize=B, N_epoch=15, D_iterations=2, G_iterations=1, saveFreq=1000, save=str(tmp_path), seed=3, coarseSize=Sz // 2, fineSize=Sz)
    S.IMG_DIMENSIONS = (1, Sz, Sz)
    torch.manual_seed(4200)
    S.MODEL_G = models_c2f.create_G((1, Sz, Sz), cuda=True, max_batch=B)
    S.MODEL_D = models_c2f.create_D((1, Sz, Sz), cuda=True, max_batch=B)
    S.set_dist(None)
    S._trainer = adversarial_c2f.TrainerC2F(ctx, S.MODEL_G, S.MODEL_D, S.OPT)
    return S.MODEL_G.inner.device_net, S.MODEL_D.inner.device_net


def test_c2f_train_epoch_on_a_gray_byte_photo_result_equals_the_epoch_on_the_luma_set(ctx, tmp_path, monkeypatch):
    """adversarial_c2f.train at S = 16, cs = 8, batch 8, N_epoch = 20, D_iterations = 2 on one-channel nets, then approxParzen(3, 4), as
    c2f_epoch runs them, on RGB photos of 30 x 34 with a face window of 20 x 20"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    monkeypatch.setattr(test_gpu_augment_c2f, "c2f_setup", gray_c2f_setup)
    b = np.random.default_rng(10).integers(0, 256, (11, 3, 30, 34), dtype=np.uint8)
    aug8, aug32 = Augmenter((20, 20), seed=5), Augmenter((20, 20), seed=5)
    u8, start8, data8 = c2f_epoch(ctx, lambda: dataset_c2f.toResultPhotos(b, (20, 20), 8, 16, aug8, ctx=ctx, storage="u8", gray=True), tmp_path)
    f32, start32, data32 = c2f_epoch(ctx, lambda: dataset_c2f.toResultPhotos(luma_set(b), (20, 20), 8, 16, aug32, ctx=ctx), tmp_path)
    assert data8.set.photos.dtype == torch.uint8 and data8.set.c == 1 and data32.set.c == 1
    same_bits(start32[0], start8[0], "initial G parameters")
    same_bits(start32[1], start8[1], "initial D parameters")
    assert not torch.equal(f32["pD"], start32[1]) and not torch.equal(f32["pG"], start32[0])
    assert f32["parzen"].shape == (3,) and bool((f32["parzen"] > 0).all())
    compare_states(f32, u8)
    assert aug8.rng.getstate() == aug32.rng.getstate()
