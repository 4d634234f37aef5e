"""fg_warp_faces on the device (include/facegen_hip.h) and faces augmented from photo-sized sources (runtime.PhotoDataset,
dataset_c2f.PhotoResult): the entry against the composition it replaces where that exists -- fg_warp_images to the window, then
fg_scale_bilinear, then fg_c2f_coarse_diff -- bit for bit; against the restatement in numpy fp32 (tests/test_photo_faces_host.py
faces_ref) on photos no other entry takes, bit for bit, and against the float64 pipeline within a derived bar; its memory contract
(guards, exact sizes, poison in what was not asked for, indices outside the set, matrices of NaN / inf / 1e30, windows half and wholly
outside the photo); that it is stateless; PhotoDataset.gather against the restatement on the host copy; and an epoch of
adversarial.train on a PhotoDataset and of adversarial_c2f.train on a PhotoResult against the same epochs fed from the host with
faces the test made itself."""
import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, NAN_BITS
from test_augment_host import fixed_matrices
from test_photo_faces_host import faces_ref, faces_ref64, BAR_FACES, BAR_FACES_DIFF
from test_gpu_dataset import lay, off_by, bits, same_bits, compare_states, LAYOUTS
from test_gpu_augment import images_01, matrix_pool, warp, WILD, epoch
from test_gpu_augment_c2f import c2f_epoch

pytestmark = pytest.mark.gpu

FIELDS = ("fine", "coarse", "diff")
SUBSETS = [("fine",), ("coarse",), ("diff",), ("fine", "coarse"), ("fine", "diff"), ("coarse", "diff"), ("fine", "coarse", "diff")]
# (c, hs, ws, hw, ww, s, cs), sources inside the limit of fg_warp_images: no scale stage; a fractional box mean; ragged with a
# non-square window; an up-scaling stage 2; the old limit; no fields
COMPOSED = [(3, 40, 40, 32, 32, 32, 16), (3, 64, 64, 42, 42, 32, 16), (1, 9, 11, 7, 5, 4, 2), (3, 20, 20, 8, 8, 16, 8), (4, 64, 64, 64, 64, 64, 32),
            (3, 40, 40, 32, 32, 32, 0)]
# photos beyond that limit: the case the entry exists for
PHOTOS = [(3, 250, 250, 84, 84, 64, 32), (3, 250, 250, 84, 84, 32, 16), (1, 300, 200, 84, 84, 32, 0), (3, 97, 131, 84, 84, 64, 32)]
N_OUT = (1, 3, 37)


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def P(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def warp_faces(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, hw, ww, s, cs, fine, coarse, diff, ol, fill):
    ctx.check(ctx.lib.fg_warp_faces(ctx.h, P(set_dev), n_set, c, hs, ws, sl, P(idx_dev), P(mats_dev), P(gains_dev), n, hw, ww, s, cs, P(fine),
                                    P(coarse), P(diff), ol, fill))


def composition(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, hw, ww, s, cs, fill):
    """today's entries through HBM, all channel-major: fg_warp_images to the window, fg_scale_bilinear to s x s, fg_c2f_coarse_diff
    -> {field: float32 [n][c][s][s]} on the host"""
    window = torch.full((n * c * hw * ww,), -7.0, device=ctx.device)
    fine, coarse, diff, tmp = (torch.full((m,), -7.0, device=ctx.device) for m in (n * c * s * s,) * 3 + (max(n * c * cs * cs, 1),))
    warp(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, window, hw, ww, 1, fill)
    ctx.check(ctx.lib.fg_scale_bilinear(ctx.h, window.data_ptr(), fine.data_ptr(), n, c, hw, ww, s, s, 1))
    out = dict(fine=fine)
    if cs:
        ctx.check(ctx.lib.fg_c2f_coarse_diff(ctx.h, fine.data_ptr(), coarse.data_ptr(), diff.data_ptr(), tmp.data_ptr(), n, c, s, cs, 1))
        out.update(coarse=coarse, diff=diff)
    return {f: t.cpu().numpy().reshape(n, c, s, s) for f, t in out.items()}


def check_fields(got, want, ol, what):
    for f, g in got.items():
        g, w = bits(g.cpu().numpy()).reshape(-1), bits(lay(want[f], ol)).reshape(-1)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError("%s: %s: %d of %d floats differ, first at %d: %r against %r"
                                 % (what, f, bad.size, g.size, bad[0], float(g.view(np.float32)[bad[0]]), float(w.view(np.float32)[bad[0]])))


@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", COMPOSED)
def test_warp_faces_equals_the_composition_on_the_device_bit_for_bit(ctx, c, hs, ws, hw, ww, s, cs):
    """n in {1, 3, 37} x both fills x gains NULL / given x the four layout pairs x every non-empty subset of the outputs (fine alone
    with cs = 0); the composition is computed once per (n, fill, gains, set layout), channel-major, and laid out on the host"""
    rng = np.random.default_rng(300 + c * hs + s + cs)
    n_set = 5
    x = images_01(rng, (n_set, c, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, hw, ww, seed=c + hs)
    sets = {sl: torch.as_tensor(lay(x, sl)).to(ctx.device) for sl in (0, 1)}
    subsets = SUBSETS if cs else [("fine",)]
    eo, calls = c * s * s, 0
    for n in N_OUT:
        for k, fill in enumerate((0, 1)):
            pick = ((5 * n + 7 * k) % 37 + np.arange(n)) % 37
            idx = rng.integers(0, n_set, n).astype(np.int32)
            idx_dev, m_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, pool_m[pick], pool_g[pick]))
            for gains_dev in (None, g_dev):
                for sl, ol in LAYOUTS:
                    want = composition(ctx, sets[sl], n_set, c, hs, ws, sl, idx_dev, m_dev, gains_dev, n, hw, ww, s, cs, fill)
                    for subset in subsets:
                        out = {f: torch.full((n * eo,), -7.0, device=ctx.device) for f in subset}
                        warp_faces(ctx, sets[sl], n_set, c, hs, ws, sl, idx_dev, m_dev, gains_dev, n, hw, ww, s, cs, out.get("fine"),
                                   out.get("coarse"), out.get("diff"), ol, fill)
                        calls += 1
                        check_fields(out, want, ol, "%r, layouts %d -> %d, fill %d, gains %s, n = %d, against the composition"
                                     % (subset, sl, ol, fill, gains_dev is not None, n))
    assert calls == 3 * 2 * 2 * 4 * len(subsets)
    if hs == hw and ws == ww:               # without matrices: the identity on a window of the photo's size
        idx_dev = torch.as_tensor(np.arange(n_set, dtype=np.int32)).to(ctx.device)
        for sl, ol in LAYOUTS:
            want = composition(ctx, sets[sl], n_set, c, hs, ws, sl, idx_dev, None, None, n_set, hw, ww, s, cs, 0)
            out = {f: torch.full((n_set * eo,), -7.0, device=ctx.device) for f in subsets[-1]}
            warp_faces(ctx, sets[sl], n_set, c, hs, ws, sl, idx_dev, None, None, n_set, hw, ww, s, cs, out.get("fine"), out.get("coarse"),
                       out.get("diff"), ol, 1)
            check_fields(out, want, ol, "mats NULL, layouts %d -> %d" % (sl, ol))


@pytest.fixture(scope="module")
def photo_refs():
    """faces_ref of a shape's calls, computed once per (shape, n, fill, gains) and shared by the layout pairs"""
    return {}


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", PHOTOS)
def test_warp_faces_equals_the_restatement_on_photos_bit_for_bit(ctx, photo_refs, sl, ol, c, hs, ws, hw, ww, s, cs):
    """photos above the 16384 floats of fg_warp_images: n_set = 5, n in {1, 3, 37} from the pool of 37 transforms, both fills, gains
    NULL and given, the bases of set and outputs at residues 0 and 1 of 4 floats, all requested fields of one call.

    At n = 37 the restatement is also held against the float64 pipeline (warp_ref64, then float64 image.scale; faces_ref64).  The
    kernel's bits are the restatement's, so this is the kernel's distance too.  The bar (tests/test_photo_faces_host.py BAR_FACES):
    BAR_64 is derived for coordinates below 128; a photo of up to 512 pixels a side has coordinate roundings four times as large
    (2^-16 instead of 2^-18), the rest of that derivation carries over: 4 * BAR_64 for the window.  Every image.scale pass is a
    convex combination of its source (box mean or linear interpolation, non-negative weights that sum to 1), so it passes a
    distance on without enlarging it and adds under 2.5e-5 of its own (the plan's position in fp32 times the slope, and the roundings
    of a 5 x 5 box): 1e-4 for the three of them.  diff = fine - coarse has the sum of the two distances."""
    shape = (c, hs, ws, hw, ww, s, cs)
    rng = np.random.default_rng(400 + hs + s + cs)
    n_set = 5
    x = images_01(rng, (n_set, c, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, hw, ww, seed=hs + s)
    fields = FIELDS if cs else ("fine",)
    eo = c * s * s
    for n in N_OUT:
        for k, fill in enumerate((0, 1)):
            pick = ((5 * n + 7 * k) % 37 + np.arange(n)) % 37
            idx = rng.integers(0, n_set, n).astype(np.int32)
            idx_dev, m_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, pool_m[pick], pool_g[pick]))
            for gains, gains_dev in ((None, None), (pool_g[pick], g_dev)):
                key = (shape, n, fill, gains is not None)
                if key not in photo_refs:
                    want = faces_ref(x, idx, pool_m[pick], gains, hw, ww, s, cs, fill)
                    if n == 37:
                        w64 = faces_ref64(x, idx, pool_m[pick], gains, hw, ww, s, cs, fill)
                        for f in fields:
                            d = float(np.abs(want[f].astype(np.float64) - w64[f]).max())
                            print("%r fill %d gains %s: %s against the float64 pipeline: worst |difference| %.3g" % (shape, fill, gains is not None, f, d))
                            assert d <= (BAR_FACES_DIFF if f == "diff" else BAR_FACES), (f, d)
                    photo_refs[key] = want
                want = photo_refs[key]
                for r in (0, 1):
                    set_dev = off_by(ctx, lay(x, sl), r)
                    out = {f: torch.full((n * eo + r,), -7.0, device=ctx.device)[r:] for f in fields}
                    assert set_dev.data_ptr() % 16 == 4 * r and all(t.data_ptr() % 16 == 4 * r for t in out.values())
                    warp_faces(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, m_dev, gains_dev, n, hw, ww, s, cs, out.get("fine"), out.get("coarse"),
                               out.get("diff"), ol, fill)
                    check_fields(out, want, ol, "%r, layouts %d -> %d, fill %d, gains %s, n = %d, bases + %d floats, against the restatement"
                                 % (shape, sl, ol, fill, gains is not None, n, r))


@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", [(1, 3, 33100, 1, 33000, 8, 4), (1, 2, 35400, 1, 35296, 64, 32), (1, 1, 40000, 1, 36000, 4, 0),
                                                (1, 40000, 2, 36000, 1, 4, 2)])
def test_a_wide_flat_window_equals_the_restatement_bit_for_bit(ctx, c, hs, ws, hw, ww, s, cs):
    """a window side above 32767, up to the largest window the entry accepts (1 x 1 x 35296 -> 64 -> 32 takes exactly 163840 bytes
    of LDS): the two sides reach the kernel in 16 unsigned bits each, and every size the entry accepts must run.  Identity with the
    crop's offset, a flip, a half-pixel shift and both zooms, both fills, gains NULL and given, against faces_ref."""
    rng = np.random.default_rng(600 + ww + hw)
    n_set = 2
    x = images_01(rng, (n_set, c, hs, ws))
    mats = fixed_matrices(hs, ws, hw, ww)[[0, 1, 5, 10, 11]]
    n = len(mats)
    gains = np.array([1.0, 0.9, 1.1, 1.05, 0.0], dtype=np.float32)
    idx = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    fields = FIELDS if cs else ("fine",)
    set_dev = torch.as_tensor(x).to(ctx.device)
    idx_dev, m_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, mats, gains))
    for fill in (0, 1):
        for g_host, gains_dev in ((None, None), (gains, g_dev)):
            want = faces_ref(x, idx, mats, g_host, hw, ww, s, cs, fill)
            assert want["fine"][:4].any()
            out = {f: torch.full((n * c * s * s,), -7.0, device=ctx.device) for f in fields}
            warp_faces(ctx, set_dev, n_set, c, hs, ws, 1, idx_dev, m_dev, gains_dev, n, hw, ww, s, cs, out.get("fine"), out.get("coarse"),
                       out.get("diff"), 1, fill)
            check_fields(out, want, 1, "%r, fill %d, gains %s, against the restatement" % ((c, hs, ws, hw, ww, s, cs), fill, g_host is not None))


def outside_matrices(hs, ws, hw, ww):
    """windows half outside (right, bottom, upper left corner) and wholly outside (right, left, below, above) the photo, unit scale"""
    oy = (hs - hw) / 2.0
    ox = (ws - ww) / 2.0
    return np.array([[1, 0, ws - ww / 2.0, 0, 1, oy], [1, 0, ox, 0, 1, hs - hw / 2.0], [1, 0, -ww / 2.0, 0, 1, -hw / 2.0],
                     [1, 0, ws + 5, 0, 1, oy], [1, 0, -ww - 5, 0, 1, oy], [1, 0, ox, 0, 1, hs + 5], [1, 0, ox, 0, 1, -hw - 5]], dtype=np.float32)


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs,align", [(3, 40, 40, 32, 32, 32, 16, 256), (1, 9, 11, 7, 5, 4, 2, 4), (3, 97, 131, 84, 84, 32, 16, 8),
                                                      (3, 64, 64, 42, 42, 32, 0, 16)])
def test_memory_contract_and_hostile_matrices(ctx, sl, ol, c, hs, ws, hw, ww, s, cs, align):
    """every operand exactly as long as the header says, between guard bands; run_contract pre-fills the requested outputs with NaN,
    0 and 1e30 in turn and the bands behind the inputs with NaN first: nothing outside the requested outputs is written, the inputs
    are left alone, the result depends on nothing it did not write and holds no NaN.  An output that is not asked for (NULL) keeps
    its poison.  Drawn matrices, matrices of NaN, +-inf, +-1e30 and 3e9, and windows half and wholly outside the photo, under both
    fills: the restatement's bits, for every shape.  Beside that, spelled out: a window wholly outside is all 0 under fill 0 (every
    shape); under fill 1 it is the photo's edge column, pixel for pixel, which is asserted directly only where no scale stage and no
    gain stand between the window and the face (the shape with hw == ww == s, the calls without gains) -- elsewhere the edge
    property rests on the comparison with faces_ref alone."""
    from face_generator_amd.runtime import Augmenter
    rng = np.random.default_rng(5)
    n_set, n = 9, 12
    e = n * c * s * s
    fields = FIELDS if cs else ("fine",)
    subsets = [("fine", "coarse", "diff"), ("coarse",), ("diff", "coarse"), ("fine",)] if cs else [("fine",)]
    x = images_01(rng, (n_set, c, hs, ws))
    idx = np.array([8, 0, 3, 3, 8, 1, 7, 8, 0, 2, 8, 5], dtype=np.int32)
    mats, gains = Augmenter((hw, ww), seed=align).draw(n, (hs, ws))
    outside = np.concatenate([outside_matrices(hs, ws, hw, ww), mats[:5]])
    ar = Arena.sized(ctx.device, [x.size, n, 6 * n, n] + [e] * len(fields))
    set_dev = ar.put(lay(x, sl), align=align, name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(mats, align=4, name="mats")
    gains_dev = ar.put(gains, align=4, name="gains")
    out = {f: ar.take(e, align=align, name=f) for f in fields}
    poison = torch.tensor(0x7FA00001, dtype=torch.int32)
    for fill in (0, 1):
        for tag, m_host in (("drawn", mats), ("wild", WILD), ("outside", outside)):
            mats_dev.copy_(torch.as_tensor(m_host))
            for k, subset in enumerate(subsets):
                g_host, g_dev = (gains, gains_dev) if (k + fill) % 2 == 0 else (None, None)
                what = "fg_warp_faces %d -> %d %r fill %d %r %s matrices%s" % (sl, ol, (c, hs, ws, hw, ww, s, cs), fill, subset, tag,
                                                                             "" if g_dev is not None else " no gains")
                idle = [f for f in fields if f not in subset]
                for f in idle:
                    out[f].view(torch.int32).fill_(int(poison))
                ptr = {f: (out[f] if f in subset else None) for f in FIELDS}
                got = run_contract(ar, lambda: warp_faces(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, g_dev, n, hw, ww, s, cs, ptr["fine"],
                                                           ptr["coarse"], ptr["diff"], ol, fill),
                                   [set_dev, idx_dev, mats_dev] + ([g_dev] if g_dev is not None else []), [out[f] for f in subset], what=what)
                for f in idle:
                    assert bool((out[f].view(torch.int32) == int(poison)).all()), "%s: %s was not asked for and was written" % (what, f)
                want = faces_ref(x, idx, m_host, g_host, hw, ww, s, cs, fill)
                check_fields(dict(zip(subset, got)), want, ol, what)
                for f, g in zip(subset, got):
                    assert bool(torch.isfinite(g).all()), "%s: %s is not finite" % (what, f)
                if tag == "wild" and fill == 0:
                    assert not want["fine"][:10].any() and want["fine"][10:].any()  # the first ten read nothing: 0
                if tag == "outside" and "fine" in subset:
                    g = got[subset.index("fine")].cpu().numpy()
                    fine = g.reshape(n, c, s, s) if ol else g.reshape(n, s, s, c).transpose(0, 3, 1, 2)
                    if fill == 0:
                        assert not fine[3:7].any() and fine[0].any() and fine[1].any() and fine[2].any()
                    elif g_host is None and hw == s and ww == s:          # the copy stage: the edge itself, pixel for pixel
                        oy = (hs - hw) // 2
                        right = x[idx[3]][:, oy:oy + hw, ws - 1]
                        assert np.array_equal(fine[3], np.broadcast_to(right[:, :, None], fine[3].shape))
                        left = x[idx[4]][:, oy:oy + hw, 0]
                        assert np.array_equal(fine[4], np.broadcast_to(left[:, :, None], fine[4].shape))


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", [(3, 97, 131, 84, 84, 32, 16), (1, 9, 11, 7, 5, 4, 2), (3, 40, 40, 32, 32, 32, 0)])
def test_an_index_outside_the_set_gives_nan_faces_in_every_requested_output(ctx, sl, ol, c, hs, ws, hw, ww, s, cs):
    """0x7fc00000 in face j of every requested output, the neighbours (repeated indices among them) are the restatement's, what is
    not asked for keeps its value and the guards around the set (which the outside indices would leave by far) stay intact"""
    rng = np.random.default_rng(21)
    n_set = 5
    x = images_01(rng, (n_set, c, hs, ws))
    idx = np.array([0, 4, 4, -1, 2, n_set, 1, 2 ** 31 - 1, 4, -2 ** 31, 3, 3], dtype=np.int32)
    inside = (idx >= 0) & (idx < n_set)
    n, eo = idx.size, c * s * s
    fields = FIELDS if cs else ("fine",)
    mats = fixed_matrices(hs, ws, hw, ww)[:n]
    ar = Arena.sized(ctx.device, [x.size, n, 6 * n] + [n * eo] * len(fields))
    set_dev = ar.put(lay(x, sl), name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(mats, align=4, name="mats")
    out = {f: ar.take(n * eo, name=f) for f in fields}
    want = faces_ref(x, idx, mats, None, hw, ww, s, cs, 0)
    for subset in ([("fine", "coarse", "diff"), ("coarse",), ("diff", "fine")] if cs else [("fine",)]):
        for f in fields:
            out[f].fill_(-7.0)
        warp_faces(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, None, n, hw, ww, s, cs, *[out[f] if f in subset else None for f in FIELDS], ol, 0)
        torch.cuda.synchronize()
        ar.assert_guards("fg_warp_faces with indices outside the set, %r" % (subset,))
        for f in fields:
            got = bits(out[f].cpu().numpy()).reshape(n, eo)
            if f not in subset:
                assert (got == np.float32(-7.0).view(np.int32)).all(), "%s was not asked for and was written" % f
                continue
            assert (got[~inside] == NAN_BITS).all(), "%s: a face of an index outside the set is not all quiet NaN" % f
            assert np.array_equal(got, bits(lay(want[f], ol)).reshape(n, eo)), "%s: a neighbour of a NaN face differs" % f


@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", [(3, 97, 131, 84, 84, 32, 16), (1, 9, 11, 7, 5, 4, 0)])
def test_the_entry_is_stateless(ctx, c, hs, ws, hw, ww, s, cs):
    """the same call twice gives equal bits; n faces, then m faces at shifted pointers, equal one call of n + m"""
    rng = np.random.default_rng(8)
    n_set, n, m = 5, 7, 5
    x = images_01(rng, (n_set, c, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, hw, ww, seed=2)
    idx = rng.integers(0, n_set, n + m).astype(np.int32)
    set_dev = torch.as_tensor(x).to(ctx.device)
    idx_dev, m_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, pool_m[:n + m], pool_g[:n + m]))
    fields = FIELDS if cs else ("fine",)
    eo = c * s * s

    def run(first, count, out):
        warp_faces(ctx, set_dev, n_set, c, hs, ws, 1, idx_dev[first:], m_dev[first:], g_dev[first:], count, hw, ww, s, cs,
                   *[out[f][first * eo:] if f in out else None for f in FIELDS], 0, 0)
    one, again, split = ({f: torch.full(((n + m) * eo,), -7.0, device=ctx.device) for f in fields} for _ in range(3))
    run(0, n + m, one)
    run(0, n + m, again)
    run(0, n, split)
    run(n, m, split)
    for f in fields:
        same_bits(one[f].cpu(), again[f].cpu(), "%s of the same call twice" % f)
        same_bits(one[f].cpu(), split[f].cpu(), "%s of %d + %d faces against one call" % (f, n, m))
        assert bool(torch.isfinite(one[f]).all()) and float(one[f].abs().max()) > 0


def test_sizes_above_a_compute_units_lds_are_refused_on_the_device_and_the_siblings_keep_their_limit(ctx):
    from face_generator_amd.runtime import FgError
    t = torch.zeros(3 * 74 * 74, device=ctx.device)
    i = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    with pytest.raises(FgError, match="163840"):
        warp_faces(ctx, t, 1, 3, 4, 4, 1, i, t, None, 1, 4, 4, 128, 64, t, None, None, 1, 0)
    with pytest.raises(FgError, match="16428"):
        warp(ctx, t, 1, 3, 74, 74, 1, i, t, None, 1, t, 8, 8, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# PhotoDataset / PhotoResult
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_draw", [False, True])
@pytest.mark.parametrize("c,hs,ws,window,s,fill", [(3, 250, 250, (84, 84), 32, "constant"), (1, 40, 44, (20, 18), 16, "edge")])
def test_photo_dataset_gather_equals_the_restatement_on_the_host_copy(ctx, c, hs, ws, window, s, fill, device_draw):
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter, PhotoDataset
    make = (lambda: DeviceAugmenter(window, seed=77, fill=fill)) if device_draw else (lambda: Augmenter(window, seed=77, fill=fill))
    x = images_01(np.random.default_rng(31), (7, c, hs, ws))
    ds, twin = PhotoDataset(ctx, x, window, s, augment=make()), make()
    draw = (lambda k: twin.draw(k, (hs, ws), ctx=ctx)) if device_draw else (lambda k: twin.draw(k, (hs, ws)))
    for picks, layout in (([3, 6, 0, 3, 5], "nhwc"), (list(range(7)), "nchw"), ([5], "nhwc"),
                          (torch.tensor([1, 1, 2], dtype=torch.int32, device=ctx.device), "nchw")):
        got = ds.gather(picks, layout=layout)
        host_picks = picks.tolist() if torch.is_tensor(picks) else picks
        mats, gains = draw(len(host_picks))
        want = faces_ref(x, host_picks, mats, gains, window[0], window[1], s, 0, twin.fill_code)["fine"]
        assert tuple(got.shape) == ((len(host_picks), s, s, c) if layout == "nhwc" else (len(host_picks), c, s, s))
        same_bits(got.cpu(), torch.as_tensor(lay(want, 0 if layout == "nhwc" else 1)), "gather(%s, %s)" % (host_picks, layout))
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert twin.state() == ds.augment.state() if device_draw else twin.rng.getstate() == ds.augment.rng.getstate()
    # the stored faces: the central window under the identity, no gains
    ident = np.tile(np.array([1, 0, (ws - window[1]) / 2.0, 0, 1, (hs - window[0]) / 2.0], dtype=np.float32), (3, 1))
    central = faces_ref(x, [4, 4, 6], ident, None, window[0], window[1], s, 0, 0)["fine"]
    same_bits(ds.gather([4, 4, 6], augment=False).cpu(), torch.as_tensor(lay(central, 0)), "the un-augmented pull")
    same_bits(PhotoDataset(ctx, x, window, s).gather([4, 4, 6], layout="nchw").cpu(), torch.as_tensor(central), "a set without an augmenter")
    same_bits(ds[6], torch.as_tensor(central[2]), "ds[6]")
    same_bits(ds.rows(4, 7).cpu()[[0, 2]], torch.as_tensor(central[[0, 2]]), "rows(4, 7)")


class HostFacesDataset:
    """dataset[i] as the test computes it: the face of photo i under the next draw of an Augmenter of its own, by the restatement"""

    def __init__(self, photos, window, s, augmenter):
        self.photos, self.window, self.s, self.aug = photos, window, s, augmenter

    def size(self):
        return len(self.photos)

    def __getitem__(self, i):
        mats, gains = self.aug.draw(1, self.photos.shape[2:])
        return faces_ref(self.photos, [i], mats, gains, self.window[0], self.window[1], self.s, 0, self.aug.fill_code)["fine"][0]


def test_adversarial_train_epoch_on_a_photo_dataset_equals_the_host_fed_epoch(ctx, tmp_path):
    """grayscale 16 x 16, batch 16, N_epoch = 51, D_iterations = 2, as tests/test_gpu_augment.py runs it, on photos of 40 x 44 with a
    face window of 24 x 24.  Fresh nets and the same seeds twice: a PhotoDataset, and a host dataset whose [i] the test makes itself
    with the same draws."""
    from face_generator_amd.runtime import Augmenter, PhotoDataset
    photos = images_01(np.random.default_rng(9), (23, 1, 40, 44))
    aug = Augmenter((24, 24), seed=5)
    res, start_r = epoch(ctx, 16, lambda: PhotoDataset(ctx, photos, (24, 24), 16, augment=aug), tmp_path)
    host, start_h = epoch(ctx, 16, lambda: HostFacesDataset(photos, (24, 24), 16, Augmenter((24, 24), seed=5)), tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    same_bits(start_h[1], start_r[1], "initial D parameters")
    assert host["countTrainedD"] == (12, 12)
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    compare_states(host, res)
    twin = Augmenter((24, 24), seed=5)
    twin.draw(2 * (5 * 8 + 5), (40, 44))
    assert twin.rng.getstate() == aug.rng.getstate()                       # one transform per real face of the epoch


class HostPhotoC2F:
    """the examples of a PhotoResult as the test computes them, in the order the host-fed loop pulls (tests/test_gpu_augment_c2f.py
    HostC2FDataset: a .coarse read takes over the oldest transform a .diff read of the same pick left behind, and draws otherwise)"""

    class Lazy:
        def __init__(self, owner, i):
            self.owner, self.i, self.fields = owner, i, None

        def __getattr__(self, field):
            if field not in FIELDS:
                raise AttributeError(field)
            if self.fields is None:
                o = self.owner
                if field == "coarse" and o.left_by_diff:
                    i, t = o.left_by_diff.pop(0)
                    assert i == self.i
                else:
                    t = o.aug.draw(1, o.photos.shape[2:])
                    if field == "diff":
                        o.left_by_diff.append((self.i, t))
                self.fields = {f: v[0] for f, v in faces_ref(o.photos, [self.i], t[0], t[1], o.window[0], o.window[1], o.s, o.cs, o.aug.fill_code).items()}
            return self.fields[field]

    def __init__(self, photos, window, s, cs, augmenter):
        self.photos, self.window, self.s, self.cs, self.aug, self.left_by_diff = photos, window, s, cs, augmenter, []

    def size(self):
        return len(self.photos)

    def __getitem__(self, i):
        return HostPhotoC2F.Lazy(self, i)


def test_c2f_train_epoch_on_a_photo_result_equals_the_host_fed_loop(ctx, tmp_path):
    """adversarial_c2f.train at S = 16, cs = 8, batch 8, N_epoch = 20, D_iterations = 2, then approxParzen(3, 4), as
    tests/test_gpu_augment_c2f.py runs them, on photos of 30 x 34 with a face window of 20 x 20"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    photos = images_01(np.random.default_rng(10), (11, 3, 30, 34))
    aug = Augmenter((20, 20), seed=5)
    res, start_r, _ = c2f_epoch(ctx, lambda: dataset_c2f.toResultPhotos(photos, (20, 20), 8, 16, aug, ctx=ctx), tmp_path)
    host_data = HostPhotoC2F(photos, (20, 20), 16, 8, Augmenter((20, 20), seed=5))
    host, start_h, _ = c2f_epoch(ctx, lambda: host_data, tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    same_bits(start_h[1], start_r[1], "initial D parameters")
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    assert host["parzen"].shape == (3,) and bool((host["parzen"] > 0).all()) and bool((host["parzen"] < 1e9).all())
    assert host_data.left_by_diff == []
    compare_states(host, res)
    twin = Augmenter((20, 20), seed=5)
    twin.draw(4 * (2 * (4 + 4) + 8) + (2 * (2 + 2) + 4) + 3, (30, 34))      # per iteration 2 x (half + half) + B, then one per parzen sample
    assert twin.rng.getstate() == aug.rng.getstate()
