"""The resident sets held as 8-bit pixels, on the device: fg_warp_images_u8, fg_warp_c2f_u8 and fg_warp_faces_u8
(include/facegen_hip.h) and storage="u8" of runtime.DeviceDataset / PhotoDataset and the dataset_c2f results.  The decode of all 256
bytes against the division numpy makes; every entry against its fp32 sibling on the float set b / 255, bit for bit, over the
layouts, fills, gains, field subsets and the three load widths; reads that stay inside the set; indices outside the set and wild
matrices; the classes against their fp32 twins; an epoch of adversarial.train and of adversarial_c2f.train on a byte set against the
same epoch on the float set.  There is no tolerance anywhere: every comparison is on int32 bits."""
import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, NAN_BITS
from test_gpu_dataset import lay, bits, same_bits, compare_states, LAYOUTS
from test_gpu_augment import matrix_pool, WILD, epoch
from test_gpu_augment_c2f import c2f_epoch
from test_u8_sets_host import decode

pytestmark = pytest.mark.gpu

FIELDS = ("fine", "coarse", "diff")
SUBSETS = [("fine",), ("coarse",), ("diff",), ("fine", "coarse"), ("fine", "diff"), ("coarse", "diff"), ("fine", "coarse", "diff")]
N_SET = 5
N_OUT = (1, 3, 37)
RESIDUES = (0, 1, 4)          # bytes that the set's base lies behind a 16-byte boundary: 16-byte loads, byte loads, 4-byte loads
# (c, hs, ws, ho, wo): a crop by the matrix alone; ragged; 105 bytes per image; the limit
IMAGES = [(3, 40, 40, 32, 32), (1, 9, 11, 7, 5), (3, 7, 5, 7, 5), (4, 64, 64, 64, 64)]
# (c, hs, ws, s, cs); the last is above 64 KB of LDS
C2F = [(3, 40, 40, 32, 16), (1, 9, 11, 4, 2), (3, 64, 64, 64, 32)]
# (c, hs, ws, hw, ww, s, cs); the last two are photos beyond the limit of the other two entries, run at n in {1, 37}
FACES = [(3, 40, 40, 32, 32, 32, 16), (1, 9, 11, 7, 5, 4, 2), (3, 20, 20, 8, 8, 16, 8), (3, 97, 131, 84, 84, 64, 32), (3, 250, 250, 84, 84, 32, 16)]


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


class Entry:
    """an entry and its sibling behind one signature: run(u8, set, sl, idx, mats, gains, n, outs, ol, fill) with outs = {field: tensor}
    (fg_warp_images: the field is "fine")"""

    def __init__(self, ctx, name, c, hs, ws, *sizes):
        self.ctx, self.name, self.c, self.hs, self.ws, self.sizes = ctx, name, c, hs, ws, sizes
        self.out_hw = sizes[:2] if name == "fg_warp_images" else (sizes[-2], sizes[-2])
        self.fields = ("fine",) if name == "fg_warp_images" or sizes[-1] == 0 else FIELDS
        self.eo = c * self.out_hw[0] * self.out_hw[1]

    def run(self, u8, set_dev, sl, idx, mats, gains, n, outs, ol, fill):
        fn = getattr(self.ctx.lib, self.name + ("_u8" if u8 else ""))
        assert set_dev.dtype == (torch.uint8 if u8 else torch.float32)
        head = (self.ctx.h, set_dev.data_ptr(), N_SET, self.c, self.hs, self.ws, sl, P(idx), P(mats), P(gains), n)
        if self.name == "fg_warp_images":
            rc = fn(*head, P(outs["fine"]), self.sizes[0], self.sizes[1], ol, fill)
        else:
            rc = fn(*head, *self.sizes, P(outs.get("fine")), P(outs.get("coarse")), P(outs.get("diff")), ol, fill)
        self.ctx.check(rc)

    def subsets(self):
        return SUBSETS if len(self.fields) == 3 else [("fine",)]


def ibits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the decode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residue", RESIDUES)
def test_the_identity_call_decodes_every_byte_to_the_float_numpy_divides_it_to(ctx, residue):
    """a 1 x 16 x 16 image of the bytes 0 .. 255 through the copy into LDS (fg_warp_images_u8), the c2f `fine` field at s = 16 / cs = 8
    and the taps from global memory (fg_warp_faces_u8 with hw = ww = s = 16, cs = 0): np.float32(b) / np.float32(255), all 256 of
    them -- which the product with the reciprocal misses for 126"""
    b = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    want = bits(np.arange(256).astype(np.float32) / np.float32(255))
    assert want.shape == (256,) and np.array_equal(want, bits(decode(b)).reshape(-1))
    set_dev, _ = byte_set(ctx, b, residue)
    idx = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    lib, h = ctx.lib, ctx.h
    for fill in (0, 1):
        outs = [torch.full((256,), -7.0, device=ctx.device) for _ in range(3)]
        ctx.check(lib.fg_warp_images_u8(h, set_dev.data_ptr(), 1, 1, 16, 16, 1, idx.data_ptr(), None, None, 1, outs[0].data_ptr(), 16, 16, 1, fill))
        ctx.check(lib.fg_warp_c2f_u8(h, set_dev.data_ptr(), 1, 1, 16, 16, 1, idx.data_ptr(), None, None, 1, 16, 8, outs[1].data_ptr(), None, None, 1, fill))
        ctx.check(lib.fg_warp_faces_u8(h, set_dev.data_ptr(), 1, 1, 16, 16, 1, idx.data_ptr(), None, None, 1, 16, 16, 16, 0, outs[2].data_ptr(), None, None,
                                       1, fill))
        for name, out in zip(("fg_warp_images_u8", "fg_warp_c2f_u8 fine", "fg_warp_faces_u8"), outs):
            got = bits(out.cpu().numpy())
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "%s, fill %d, base + %d: %d of the 256 bytes decode to another float, first %d: %r against %r" % (
                name, fill, residue, bad.size, bad[0], float(got.view(np.float32)[bad[0]]), float(want.view(np.float32)[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. bits against the sibling
# ---------------------------------------------------------------------------------------------------------------------------------
def against_the_sibling(ctx, e, window_hw, n_out, seed):
    """n x both fills x gains NULL / given x the four layout pairs x every field subset x the set's base at residues 0, 1, 4 of 16;
    then mats == NULL where the sizes allow it.  The sibling runs once per (n, fill, gains, layouts), with every field"""
    rng = np.random.default_rng(seed)
    c, hs, ws = e.c, e.hs, e.ws
    b = rng.integers(0, 256, (N_SET, c, hs, ws), dtype=np.uint8)
    b.reshape(-1)[rng.integers(0, b.size, b.size // 16)] = 0
    b.reshape(-1)[rng.integers(0, b.size, b.size // 16)] = 255
    x = decode(b)
    pool_m, pool_g = matrix_pool(hs, ws, window_hw[0], window_hw[1], seed=c + hs)
    sets8 = {(sl, r): byte_set(ctx, lay(b, sl), r)[0] for sl in (0, 1) for r in RESIDUES}
    sets32 = {sl: torch.as_tensor(lay(x, sl)).to(ctx.device) for sl in (0, 1)}
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
                    for sl, ol in LAYOUTS:
                        for t in want.values():
                            t.fill_(-7.0)
                        e.run(False, sets32[sl], sl, idx, m, gains, n, want, ol, fill)
                        assert not any(bool((t == -7.0).any()) for t in want.values()), "the fp32 entry left part of its outputs unwritten"
                        for sub in e.subsets():
                            for r in RESIDUES:
                                for t in got.values():
                                    t.fill_(-7.0)
                                e.run(True, sets8[sl, r], sl, idx, m, gains, n, {f: got[f] for f in sub}, ol, fill)
                                calls += 1
                                for f in e.fields:
                                    if f not in sub:
                                        assert bool((got[f] == -7.0).all()), "%s: %s was not asked for and was written" % (e.name, f)
                                    elif not torch.equal(ibits(got[f]), ibits(want[f])):
                                        bad = torch.nonzero(ibits(got[f]) != ibits(want[f])).reshape(-1)
                                        raise AssertionError(
                                            "%s_u8 %s, layouts %d -> %d, fill %d, mats %s, gains %s, n = %d, fields %s, set + %d bytes: %s: %d of %d floats "
                                            "differ from the fp32 entry on b / 255, first at %d: %r against %r"
                                            % (e.name, (c, hs, ws) + e.sizes, sl, ol, fill, m is not None, gains is not None, n, sub, r, f, bad.numel(),
                                               got[f].numel(), int(bad[0]), float(got[f][bad[0]]), float(want[f][bad[0]])))
    per_n = 2 * (2 if identity_fits else 1) * 2 * 4 * len(e.subsets()) * 3
    assert calls == len(n_out) * per_n
    return calls


@pytest.mark.parametrize("c,hs,ws,ho,wo", IMAGES)
def test_warp_images_u8_equals_the_fp32_entry_on_the_decoded_set_bit_for_bit(ctx, c, hs, ws, ho, wo):
    e = Entry(ctx, "fg_warp_images", c, hs, ws, ho, wo)
    calls = against_the_sibling(ctx, e, (ho, wo), N_OUT, 500 + c * hs + wo)
    print("fg_warp_images_u8 (%d, %dx%d -> %dx%d): %d calls bit-exact" % (c, hs, ws, ho, wo, calls))


@pytest.mark.parametrize("c,hs,ws,s,cs", C2F)
def test_warp_c2f_u8_equals_the_fp32_entry_on_the_decoded_set_bit_for_bit(ctx, c, hs, ws, s, cs):
    e = Entry(ctx, "fg_warp_c2f", c, hs, ws, s, cs)
    calls = against_the_sibling(ctx, e, (s, s), N_OUT, 600 + c * hs + s)
    print("fg_warp_c2f_u8 (%d, %dx%d -> %d / %d): %d calls bit-exact" % (c, hs, ws, s, cs, calls))


@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", FACES)
def test_warp_faces_u8_equals_the_fp32_entry_on_the_decoded_set_bit_for_bit(ctx, c, hs, ws, hw, ww, s, cs):
    e = Entry(ctx, "fg_warp_faces", c, hs, ws, hw, ww, s, cs)
    calls = against_the_sibling(ctx, e, (hw, ww), (1, 37) if hs * ws > 64 * 64 else N_OUT, 700 + c * hs + s)
    print("fg_warp_faces_u8 (%d, %dx%d -> %dx%d -> %d / %d): %d calls bit-exact" % (c, hs, ws, hw, ww, s, cs, calls))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reads stay inside the set; nothing but the requested outputs is written
# ---------------------------------------------------------------------------------------------------------------------------------
SURROUNDINGS = (0x00, 0xFF, None)         # what the bytes in front of and behind the set hold in run 1, 2, 3 (None: a pattern)


@pytest.mark.parametrize("residue", RESIDUES)
@pytest.mark.parametrize("c,h,w", [(3, 7, 5), (4, 64, 64)])
@pytest.mark.parametrize("name", ["fg_warp_images", "fg_warp_c2f", "fg_warp_faces"])
def test_reads_stay_inside_the_set_and_writes_inside_the_outputs(ctx, name, c, h, w, residue):
    """the set lies inside a larger byte buffer whose other bytes change from run to run (0x00, 0xFF, a pattern): a wide load over the
    tail of the last image, or in front of the first, would decode them.  The outputs lie in an Arena between guard bands and hold
    NaN, 0 and 1e30 before the three runs (run_contract): the runs agree bit for bit, they are the sibling's bits, the guards and
    the inputs are intact, and a field that was not asked for does not exist for the entry.  105 bytes per image (byte loads at any
    base) and 16384 (16-byte, byte and 4-byte loads at residues 0, 1 and 4)."""
    s = min(h, w)                           # the c2f fields are square: 5 of 7 x 5, 64 of 64 x 64
    sizes = dict(fg_warp_images=(h, w), fg_warp_c2f=(s, 2), fg_warp_faces=(h, w, s, 2))[name]
    e = Entry(ctx, name, c, h, w, *sizes)
    rng = np.random.default_rng(c * h + residue)
    b = rng.integers(0, 256, (N_SET, c, h, w), dtype=np.uint8)
    idx = np.array([N_SET - 1, 0, N_SET - 1, 2, 0, N_SET - 1], dtype=np.int32)        # the first image and the last: the set's two ends
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
    for sl, ol in LAYOUTS:
        set8, buf = byte_set(ctx, lay(b, sl), residue, pad=pad)
        lo = set8.data_ptr() - buf.data_ptr()
        set32 = torch.as_tensor(lay(decode(b), sl)).to(ctx.device)
        pattern = torch.as_tensor(rng.integers(1, 255, buf.numel(), dtype=np.uint8)).to(ctx.device)
        for m, g in ((mats_dev, gains_dev), (None, None)) if window == (h, w) else ((mats_dev, gains_dev),):
            run = [0]

            def call():
                keep = set8.clone()
                s = SURROUNDINGS[run[0] % 3]
                if s is None:
                    buf.copy_(pattern)
                else:
                    buf.fill_(s)
                set8.copy_(keep)
                run[0] += 1
                e.run(True, set8, sl, idx_dev, m, g, n, outs, ol, 0)
            what = "%s_u8 %d -> %d (%d, %dx%d) set + %d bytes" % (name, sl, ol, c, h, w, residue)
            got = run_contract(ar, call, [idx_dev, mats_dev, gains_dev], [outs[f] for f in asked], what=what)
            assert run[0] == 3
            assert torch.equal(buf[lo:lo + b.size].cpu(), torch.as_tensor(lay(b, sl)).reshape(-1)), what + ": the set was written"
            assert torch.equal(buf[:lo], pattern[:lo]) and torch.equal(buf[lo + b.size:], pattern[lo + b.size:]), what + ": the bytes around the set were written"
            want = {f: torch.empty(n * e.eo, device=ctx.device) for f in asked}
            e.run(False, set32, sl, idx_dev, m, g, n, want, ol, 0)
            for f, t in zip(asked, got):
                assert torch.equal(ibits(t), ibits(want[f])), "%s: %s differs from the fp32 entry" % (what, f)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. hostile inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("name,sizes", [("fg_warp_images", (3, 40, 40, 32, 32)), ("fg_warp_c2f", (3, 40, 40, 32, 16)), ("fg_warp_faces", (3, 97, 131, 84, 84, 32, 16))])
def test_indices_outside_the_set_give_nan_images_and_wild_matrices_give_what_the_sibling_gives(ctx, name, sizes, sl, ol):
    """indices -1 and n_set: a quiet-NaN image in every requested field, the neighbours intact (the set lies inside a buffer of 0xFF:
    read, the bytes behind it would decode to 1).  Matrices of NaN, +-inf, +-1e30 and 3e9: the sibling's bits, for both fills."""
    e = Entry(ctx, name, *sizes)
    c, hs, ws = sizes[:3]
    rng = np.random.default_rng(17)
    b = rng.integers(0, 256, (N_SET, c, hs, ws), dtype=np.uint8)
    set8, buf = byte_set(ctx, lay(b, sl), 4, pad=4096)
    keep = set8.clone()
    buf.fill_(0xFF)
    set8.copy_(keep)
    set32 = torch.as_tensor(lay(decode(b), sl)).to(ctx.device)
    window = sizes[3:5] if name != "fg_warp_c2f" else (sizes[3], sizes[3])
    pool_m, pool_g = matrix_pool(hs, ws, window[0], window[1], seed=11)
    idx = np.array([0, -1, 4, N_SET, 2, 2, -2 ** 31, 1, 2 ** 31 - 1, 3, 4, 0], dtype=np.int32)
    n = idx.size
    assert n == len(WILD)
    idx_dev = torch.as_tensor(idx).to(ctx.device)
    inside = torch.as_tensor(np.clip(idx, 0, N_SET - 1)).to(ctx.device)
    g = torch.as_tensor(pool_g[:n]).to(ctx.device)
    for fill in (0, 1):
        for what, i_dev, m_host in (("indices outside the set", idx_dev, pool_m[:n]), ("wild matrices", inside, WILD)):
            m = torch.as_tensor(m_host).to(ctx.device)
            for gains in (g, None):
                for sub in e.subsets():
                    got = {f: torch.full((n * e.eo,), -7.0, device=ctx.device) for f in sub}
                    want = {f: torch.full((n * e.eo,), -7.0, device=ctx.device) for f in sub}
                    e.run(True, set8, sl, i_dev, m, gains, n, got, ol, fill)
                    e.run(False, set32, sl, i_dev, m, gains, n, want, ol, fill)
                    for f in sub:
                        tag = "%s_u8 %d -> %d fill %d, %s, gains %s, %s" % (name, sl, ol, fill, what, gains is not None, f)
                        rows = ibits(got[f]).reshape(n, e.eo)
                        if i_dev is idx_dev:
                            for j, i in enumerate(idx.tolist()):
                                assert bool((rows[j] == NAN_BITS).all()) != (0 <= i < N_SET), "%s: image %d (index %d)" % (tag, j, i)
                        assert torch.equal(ibits(got[f]), ibits(want[f])), "%s differs from the fp32 entry" % tag


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the classes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_classes_on_a_byte_set_hand_out_the_bits_of_their_fp32_twins(ctx):
    """DeviceDataset, PhotoDataset, AugmentedResult and PhotoResult with storage="u8" against the same classes on b / 255, each pair
    under DeviceAugmenters at one (seed, offset): gathers, gather_fields, rows and ds[i]"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset, PhotoDataset, FgError
    rng = np.random.default_rng(41)
    b = rng.integers(0, 256, (9, 3, 40, 40), dtype=np.uint8)
    x = decode(b)
    picks = [3, 8, 0, 3, 7]
    dev_picks = torch.tensor([1, 1, 2], dtype=torch.int32, device=ctx.device)

    def augs(hw):
        a, t = DeviceAugmenter(hw, seed=77), DeviceAugmenter(hw, seed=77)
        a.set_state(77, 30)
        t.set_state(77, 30)
        return a, t
    # DeviceDataset
    a, t = augs((32, 32))
    d8, d32 = DeviceDataset(ctx, b, augment=a, storage="u8"), DeviceDataset(ctx, x, augment=t)
    assert d8.images.dtype == torch.uint8 and d8.images.numel() == b.size and d8.images.element_size() == 1
    for p, layout in ((picks, "nhwc"), (list(range(9)), "nchw"), ([5], "nhwc"), (dev_picks, "nchw")):
        same_bits(d8.gather(p, layout=layout).cpu(), d32.gather(p, layout=layout).cpu(), "DeviceDataset.gather(%s, %s)" % (p, layout))
        same_bits(d8.gather(p, layout=layout, augment=False).cpu(), d32.gather(p, layout=layout, augment=False).cpu(), "the un-augmented gather")
    assert a.state() == t.state() and a.state() != (77, 30)
    out = ctx.empty(2, 40, 40, 3)
    assert d8.gather([4, 6], out=out, augment=False).data_ptr() == out.data_ptr()
    same_bits(out.cpu(), torch.as_tensor(lay(x[[4, 6]], 0)), "gather(out=): the decoded images themselves")
    same_bits(d8[6], torch.as_tensor(x[6]), "ds[6]")
    same_bits(d8.rows(2, 5).cpu(), torch.as_tensor(x[2:5]), "rows(2, 5)")
    same_bits(d8.rows(0, 9).cpu(), d32.rows(0, 9).cpu().contiguous(), "rows(0, 9)")
    big = DeviceDataset(ctx, np.zeros((2, 1, 4, 4097), dtype=np.uint8), storage="u8")
    with pytest.raises(FgError, match="fg_warp_images_u8.*16388"):
        big.gather([0])
    # PhotoDataset
    a, t = augs((24, 24))
    p8, p32 = PhotoDataset(ctx, b, (24, 24), 16, augment=a, storage="u8"), PhotoDataset(ctx, x, (24, 24), 16, augment=t)
    assert p8.photos.dtype == torch.uint8
    for p, layout in ((picks, "nhwc"), (dev_picks, "nchw")):
        same_bits(p8.gather(p, layout=layout).cpu(), p32.gather(p, layout=layout).cpu(), "PhotoDataset.gather(%s, %s)" % (p, layout))
        for fields in (("diff", "coarse"), ("fine", "coarse", "diff"), ("coarse",)):
            for g8, g32, f in zip(p8.gather_fields(p, fields, coarse_scale=8, layout=layout), p32.gather_fields(p, fields, coarse_scale=8, layout=layout), fields):
                same_bits(g8.cpu(), g32.cpu(), "PhotoDataset.gather_fields(%s): %s" % (fields, f))
    assert a.state() == t.state()
    same_bits(p8[6], p32[6], "photos[6]")
    same_bits(p8.rows(4, 9).cpu(), p32.rows(4, 9).cpu(), "PhotoDataset.rows(4, 9)")
    same_bits(p8.gather([4, 4, 6], augment=False).cpu(), p32.gather([4, 4, 6], augment=False).cpu(), "the un-augmented pull")
    # AugmentedResult and PhotoResult
    a, t = augs((32, 32))
    r8 = dataset_c2f.toResultAugmented(b, 16, 32, a, ctx=ctx, storage="u8")
    r32 = dataset_c2f.toResultAugmented(x, 16, 32, t, ctx=ctx)
    a2, t2 = augs((24, 24))
    q8 = dataset_c2f.toResultPhotos(b, (24, 24), 8, 16, a2, ctx=ctx, storage="u8")
    q32 = dataset_c2f.toResultPhotos(x, (24, 24), 8, 16, t2, ctx=ctx)
    assert r8.set.images.dtype == torch.uint8 and q8.set.photos.dtype == torch.uint8
    for u, f32, what in ((r8, r32, "AugmentedResult"), (q8, q32, "PhotoResult")):
        for p, layout in ((picks, "nhwc"), (dev_picks, "nchw")):
            for fields in (("diff", "coarse"), ("fine",), ("fine", "coarse", "diff")):
                for g8, g32, f in zip(u.gather_fields(p, fields, layout=layout), f32.gather_fields(p, fields, layout=layout), fields):
                    same_bits(g8.cpu(), g32.cpu(), "%s.gather_fields(%s, %s): %s" % (what, p, fields, f))
            same_bits(u.gather(p, "diff", layout=layout).cpu(), f32.gather(p, "diff", layout=layout).cpu(), what + ".gather")
        e8, e32 = u[4], f32[4]
        for f in FIELDS:
            same_bits(getattr(e8, f), getattr(e32, f), "%s[4].%s" % (what, f))
    assert a.state() == t.state() and a2.state() == t2.state()


def test_nearest_search_streams_a_byte_set_chunk_by_chunk(ctx):
    """rows(lo, hi) of a byte set are decoded device floats, so findClosestNeighboursOf works on it as on the float set"""
    from face_generator_amd import nn_utils
    from face_generator_amd.runtime import DeviceDataset
    rng = np.random.default_rng(8)
    b = rng.integers(0, 256, (37, 1, 16, 16), dtype=np.uint8)
    x = decode(b)
    queries = (torch.as_tensor(lay(x[[5, 30, 11]], 0)) + 0.001).to(ctx.device)         # device NHWC
    found8, near8 = nn_utils.findClosestNeighboursOf(queries, DeviceDataset(ctx, b, storage="u8"), chunk_rows=10, ctx=ctx)
    found32, near32 = nn_utils.findClosestNeighboursOf(queries, DeviceDataset(ctx, x), chunk_rows=10, ctx=ctx)
    assert [i for i, _ in found8] == [5, 30, 11] and found8 == found32          # indices and distances, float for float
    same_bits(near8.cpu(), near32.cpu(), "the neighbours")
    same_bits(near8.cpu(), torch.as_tensor(x[[5, 30, 11]]), "the neighbours are the decoded images")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. epochs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adversarial_train_epoch_on_a_byte_photo_set_equals_the_epoch_on_the_float_set(ctx, tmp_path):
    """grayscale 16 x 16, batch 16, N_epoch = 51, D_iterations = 2, as tests/test_gpu_photo_faces.py runs it, on photos of 40 x 44 with
    a face window of 24 x 24: fresh nets and the same seeds twice, once on the bytes and once on b / 255"""
    from face_generator_amd.runtime import Augmenter, PhotoDataset
    b = np.random.default_rng(9).integers(0, 256, (23, 1, 40, 44), dtype=np.uint8)
    aug8, aug32 = Augmenter((24, 24), seed=5), Augmenter((24, 24), seed=5)
    made = []

    def make(photos, aug, **kw):
        made.append(PhotoDataset(ctx, photos, (24, 24), 16, augment=aug, **kw))
        return made[-1]
    u8, start8 = epoch(ctx, 16, lambda: make(b, aug8, storage="u8"), tmp_path)
    f32, start32 = epoch(ctx, 16, lambda: make(decode(b), aug32), tmp_path)
    assert made[0].photos.dtype == torch.uint8 and made[1].photos.dtype == torch.float32
    same_bits(start32[0], start8[0], "initial G parameters")
    same_bits(start32[1], start8[1], "initial D parameters")
    assert f32["countTrainedD"] == (12, 12)
    assert not torch.equal(f32["pD"], start32[1]) and not torch.equal(f32["pG"], start32[0])
    compare_states(f32, u8)
    assert aug8.rng.getstate() == aug32.rng.getstate()


def test_c2f_train_epoch_on_a_byte_photo_result_equals_the_epoch_on_the_float_set(ctx, tmp_path):
    """adversarial_c2f.train at S = 16, cs = 8, batch 8, N_epoch = 20, D_iterations = 2, then approxParzen(3, 4), as
    tests/test_gpu_photo_faces.py runs them, on photos of 30 x 34 with a face window of 20 x 20"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    b = np.random.default_rng(10).integers(0, 256, (11, 3, 30, 34), dtype=np.uint8)
    aug8, aug32 = Augmenter((20, 20), seed=5), Augmenter((20, 20), seed=5)
    u8, start8, data8 = c2f_epoch(ctx, lambda: dataset_c2f.toResultPhotos(b, (20, 20), 8, 16, aug8, ctx=ctx, storage="u8"), tmp_path)
    f32, start32, _ = c2f_epoch(ctx, lambda: dataset_c2f.toResultPhotos(decode(b), (20, 20), 8, 16, aug32, ctx=ctx), tmp_path)
    assert data8.set.photos.dtype == torch.uint8
    same_bits(start32[0], start8[0], "initial G parameters")
    same_bits(start32[1], start8[1], "initial D parameters")
    assert not torch.equal(f32["pD"], start32[1]) and not torch.equal(f32["pG"], start32[0])
    assert f32["parzen"].shape == (3,) and bool((f32["parzen"] > 0).all())
    compare_states(f32, u8)
    assert aug8.rng.getstate() == aug32.rng.getstate()


def test_c2f_train_epoch_on_a_byte_augmented_result_equals_the_epoch_on_the_float_set(ctx, tmp_path):
    """the same epoch on an AugmentedResult (fg_warp_c2f_u8): a set of 20 x 20 stored with a margin of 2 px per side"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    b = np.random.default_rng(10).integers(0, 256, (11, 3, 20, 20), dtype=np.uint8)
    aug8, aug32 = Augmenter((16, 16), seed=5), Augmenter((16, 16), seed=5)
    u8, start8, data8 = c2f_epoch(ctx, lambda: dataset_c2f.toResultAugmented(b, 8, 16, aug8, ctx=ctx, storage="u8"), tmp_path)
    f32, start32, _ = c2f_epoch(ctx, lambda: dataset_c2f.toResultAugmented(decode(b), 8, 16, aug32, ctx=ctx), tmp_path)
    assert data8.set.images.dtype == torch.uint8
    same_bits(start32[0], start8[0], "initial G parameters")
    assert not torch.equal(f32["pD"], start32[1]) and not torch.equal(f32["pG"], start32[0])
    compare_states(f32, u8)
    assert aug8.rng.getstate() == aug32.rng.getstate()
