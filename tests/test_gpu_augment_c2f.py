"""fg_warp_c2f on the device (include/facegen_hip.h) and the coarse-to-fine set augmented per batch (dataset_c2f.AugmentedResult):
the entry against the composition it replaces -- fg_warp_images, then fg_c2f_coarse_diff on its output -- bit for bit; against the
two restatements in numpy fp32 (tests/test_augment_host.py warp_ref, then oracle.image_scale.to_result), bit for bit; its memory
contract (guards, exact sizes, poison in what was not asked for, indices outside the set, matrices of NaN / inf / 1e30);
AugmentedResult.gather_fields against the restatements applied to the host copy; and an epoch of adversarial_c2f.train plus
approxParzen on an AugmentedResult against the same loops fed from the host with examples the test warped and scaled itself."""
import contextlib
import io

import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, NAN_BITS
from oracle import image_scale
from test_augment_host import warp_ref, fixed_matrices
from test_gpu_dataset import lay, off_by, bits, same_bits, final_state, compare_states, c2f_setup, LAYOUTS
from test_gpu_augment import images_01, warp, WILD

pytestmark = pytest.mark.gpu

# (c, hs, ws, s, cs, n_set): odd s with cs not dividing it; fractional box ends; cs = 1 (the src_len == 1 branch going up); cs == s
# (coarse equals fine, diff is +0); a crop by the matrix; the model's own size; both LDS limits (4 x 64 x 64 in, 4 x 64 x 64 out)
SHAPES = [(1, 5, 7, 4, 2, 5), (3, 7, 5, 5, 3, 9), (2, 9, 9, 6, 4, 7), (3, 12, 12, 8, 1, 4), (1, 6, 6, 6, 6, 3), (3, 16, 16, 16, 8, 20),
          (3, 40, 40, 32, 16, 6), (3, 64, 64, 64, 32, 5), (4, 64, 64, 64, 32, 3)]
SUBSETS = [("fine", "coarse", "diff"), ("coarse",), ("diff", "coarse"), ("fine", "coarse")]
FIELDS = ("fine", "coarse", "diff")


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def P(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def warp_c2f(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, s, cs, fine, coarse, diff, ol, fill):
    ctx.check(ctx.lib.fg_warp_c2f(ctx.h, P(set_dev), n_set, c, hs, ws, sl, P(idx_dev), P(mats_dev), P(gains_dev), n, s, cs, P(fine), P(coarse),
                                  P(diff), ol, fill))


def composition(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, s, cs, ol, fill):
    """today's entries: fg_warp_images into a fine batch, then the two launches of fg_c2f_coarse_diff -> {field: int32 bits, flat}"""
    e = n * c * s * s
    fine, coarse, diff, tmp = (torch.full((m,), -7.0, device=ctx.device) for m in (e, e, e, n * c * cs * cs))
    warp(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, fine, s, s, ol, fill)
    ctx.check(ctx.lib.fg_c2f_coarse_diff(ctx.h, fine.data_ptr(), coarse.data_ptr(), diff.data_ptr(), tmp.data_ptr(), n, c, s, cs, ol))
    return dict(fine=bits(fine.cpu().numpy()), coarse=bits(coarse.cpu().numpy()), diff=bits(diff.cpu().numpy()))


def restated(x, idx, mats, gains, s, cs, fill):
    """the header's contract in numpy fp32: warp_ref, then dataset._toResult as oracle.image_scale restates it -> {field: [n][c][s][s]}"""
    fine = warp_ref(x, idx, mats, gains, s, s, fill)
    coarse, diff = image_scale.to_result(fine, cs, s)
    return dict(fine=fine, coarse=coarse, diff=diff)


def matrix_pool(hs, ws, s, seed):
    """the 12 fixed matrices and 25 draws of Augmenter with their gains: 37 transforms"""
    from face_generator_amd.runtime import Augmenter
    fixed = fixed_matrices(hs, ws, s, s)
    mats, gains = Augmenter((s, s), seed=seed).draw(37 - len(fixed), (hs, ws))
    g = np.concatenate([np.array([1.0, 0.9, 1.1, 0.0, 1.1, 1.0, 1.05, 0.95, 1.0, 1.1, 0.9, 1.0], dtype=np.float32)[:len(fixed)], gains])
    return np.concatenate([fixed, mats]), g


@pytest.mark.parametrize("c,hs,ws,s,cs,n_set", SHAPES)
def test_warp_c2f_equals_warp_images_then_coarse_diff_bit_for_bit(ctx, c, hs, ws, s, cs, n_set):
    """n in {1, 5} x both fills x (matrices without gains, matrices with gains, and no matrices where hs == ws == s) x the four layout
    pairs; each of these 16 or 24 x 4 combinations makes four calls, one per output subset, and the bases of set / fine / coarse /
    diff walk the four residues of 16 bytes from call to call, so that every subset meets every residue on every operand.  The
    reference of a combination is the composition in the same out_layout, computed once per (n, fill, transform mode, layouts)."""
    rng = np.random.default_rng(200 + c * hs + s + cs)
    x = images_01(rng, (n_set, c, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, s, seed=c + hs)
    eo = c * s * s
    sets = {(sl, r): off_by(ctx, lay(x, sl), r) for sl in (0, 1) for r in range(4)}
    modes = ["mats", "mats+gains"] + (["gains"] if hs == ws == s else [])
    calls, combo, seen = 0, 0, set()
    for n in (1, 5):
        for fill in (0, 1):
            start = (5 * n + 7 * fill) % 37
            pick = (start + np.arange(n)) % 37
            idx = rng.integers(0, n_set, n).astype(np.int32)
            idx_dev, m_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, pool_m[pick], pool_g[pick]))
            for mode in modes:
                mats_dev, gains_dev = (m_dev if "mats" in mode else None), (g_dev if "gains" in mode else None)
                for sl, ol in LAYOUTS:
                    want = composition(ctx, sets[sl, 0], n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, s, cs, ol, fill)
                    for k, subset in enumerate(SUBSETS):
                        r = [(combo + k + d) % 4 for d in (0, 1, 2, 3)]          # residues of set, fine, coarse, diff
                        out = {f: torch.full((n * eo + ro,), -7.0, device=ctx.device)[ro:] for f, ro in zip(FIELDS, r[1:]) if f in subset}
                        for f, ro in zip(FIELDS, r[1:]):
                            assert f not in out or out[f].data_ptr() % 16 == 4 * ro
                        warp_c2f(ctx, sets[sl, r[0]], n_set, c, hs, ws, sl, idx_dev, mats_dev, gains_dev, n, s, cs, out.get("fine"),
                                 out.get("coarse"), out.get("diff"), ol, fill)
                        calls += 1
                        seen.add((subset, tuple(r)))
                        for f in subset:
                            got = bits(out[f].cpu().numpy())
                            if not np.array_equal(got, want[f]):
                                bad = np.nonzero(got != want[f])[0]
                                raise AssertionError("%s of %r: layouts %d -> %d, fill %d, %s, n = %d, residues %r: %d of %d floats differ from the "
                                                     "composition, first at %d: %r against %r"
                                                     % (f, subset, sl, ol, fill, mode, n, r, bad.size, got.size, bad[0],
                                                        float(got.view(np.float32)[bad[0]]), float(want[f].view(np.float32)[bad[0]])))
                    combo += 1
                    if cs == s:
                        assert np.array_equal(want["coarse"], want["fine"]) and not want["diff"].any()     # diff is +0, bit for bit
    assert calls == 2 * 2 * len(modes) * 4 * 4 and len(seen) == 16


@pytest.mark.parametrize("c,hs,ws,s,cs,n_set", [SHAPES[1], SHAPES[6]])
@pytest.mark.parametrize("sl,ol", LAYOUTS)
def test_warp_c2f_equals_the_numpy_restatements_bit_for_bit(ctx, sl, ol, c, hs, ws, s, cs, n_set):
    """warp_ref followed by oracle.image_scale.to_result: what the header states, without a kernel of the library in the reference"""
    rng = np.random.default_rng(7 * c + s)
    x = images_01(rng, (n_set, c, hs, ws))
    pool_m, pool_g = matrix_pool(hs, ws, s, seed=s)
    n = 37
    idx = rng.integers(0, n_set, n).astype(np.int32)
    set_dev = torch.as_tensor(lay(x, sl)).to(ctx.device)
    idx_dev, m_dev, g_dev = (torch.as_tensor(a).to(ctx.device) for a in (idx, pool_m, pool_g))
    for fill in (0, 1):
        for gains, gains_dev in ((None, None), (pool_g, g_dev)):
            want = restated(x, idx, pool_m, gains, s, cs, fill)
            out = {f: torch.full((n * c * s * s,), -7.0, device=ctx.device) for f in FIELDS}
            warp_c2f(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, m_dev, gains_dev, n, s, cs, out["fine"], out["coarse"], out["diff"], ol, fill)
            for f in FIELDS:
                got, w = bits(out[f].cpu().numpy()), bits(lay(want[f], ol)).reshape(-1)
                assert np.array_equal(got, w), "%s, fill %d, gains %s: %d of %d floats differ from the restatement" % (
                    f, fill, gains is not None, int((got != w).sum()), got.size)


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,hs,ws,s,cs,align", [(3, 40, 40, 32, 16, 256), (3, 7, 5, 5, 3, 8), (1, 5, 7, 4, 2, 4), (4, 64, 64, 64, 32, 16)])
def test_memory_contract(ctx, sl, ol, c, hs, ws, s, cs, align):
    """every operand exactly as long as the header says, between guard bands; run_contract pre-fills the requested outputs with NaN,
    0 and 1e30 in turn and the bands behind the inputs with NaN first: nothing outside the requested outputs is written, the inputs
    are left alone, the result depends on nothing it did not write and holds no NaN.  An output that is not asked for (NULL) keeps
    its poison.  Matrices of NaN, +-inf, +-1e30 and 3e9 under both fills: finite results, intact guards.  The results are the
    composition's."""
    from face_generator_amd.runtime import Augmenter
    rng = np.random.default_rng(5)
    n_set, n = 9, 12
    e = n * c * s * s
    x = images_01(rng, (n_set, c, hs, ws))
    idx = np.array([8, 0, 3, 3, 8, 1, 7, 8, 0, 2, 8, 5], dtype=np.int32)
    mats, gains = Augmenter((s, s), seed=align).draw(n, (hs, ws))
    ar = Arena.sized(ctx.device, [x.size, n, 6 * n, n, e, e, e])
    set_dev = ar.put(lay(x, sl), align=align, name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(mats, align=4, name="mats")
    gains_dev = ar.put(gains, align=4, name="gains")
    out = {f: ar.take(e, align=align, name=f) for f in FIELDS}
    poison = torch.tensor(0x7FA00001, dtype=torch.int32)
    for fill in (0, 1):
        for m_host in (mats, WILD):
            mats_dev.copy_(torch.as_tensor(m_host))
            for k, subset in enumerate(SUBSETS):
                g_dev = gains_dev if (k + fill) % 2 == 0 else None
                what = "fg_warp_c2f %d -> %d (%d, %dx%d -> %d, coarse %d) fill %d %r%s%s" % (sl, ol, c, hs, ws, s, cs, fill, subset,
                                                                                          " wild matrices" if m_host is WILD else "",
                                                                                          "" if g_dev is not None else " no gains")
                idle = [f for f in FIELDS if f not in subset]
                for f in idle:
                    out[f].view(torch.int32).fill_(int(poison))
                ptr = {f: (out[f] if f in subset else None) for f in FIELDS}
                got = run_contract(ar, lambda: warp_c2f(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, g_dev, n, s, cs, ptr["fine"],
                                                         ptr["coarse"], ptr["diff"], ol, fill),
                                   [set_dev, idx_dev, mats_dev] + ([g_dev] if g_dev is not None else []), [out[f] for f in subset], what=what)
                for f in idle:
                    assert bool((out[f].view(torch.int32) == int(poison)).all()), "%s: %s was not asked for and was written" % (what, f)
                want = composition(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, g_dev, n, s, cs, ol, fill)
                for f, g in zip(subset, got):
                    assert bool(torch.isfinite(g).all()), "%s: %s is not finite" % (what, f)
                    assert np.array_equal(bits(g.cpu().numpy()), want[f]), "%s: %s differs from the composition" % (what, f)


@pytest.mark.parametrize("sl,ol", LAYOUTS)
@pytest.mark.parametrize("c,hs,ws,s,cs", [(3, 20, 20, 16, 8), (1, 5, 7, 4, 2), (4, 64, 64, 64, 32)])
def test_an_index_outside_the_set_gives_nan_images_in_every_requested_output(ctx, sl, ol, c, hs, ws, s, cs):
    """0x7fc00000 in image j of every requested output, the neighbours are the composition's, what is not asked for keeps its poison
    and the guards around the set (which the outside indices would leave by far) stay intact"""
    rng = np.random.default_rng(21)
    n_set = 5
    x = images_01(rng, (n_set, c, hs, ws))
    idx = np.array([0, 4, 4, -1, 2, n_set, 1, 2 ** 31 - 1, 4, -2 ** 31, 3, 3], dtype=np.int32)
    inside = (idx >= 0) & (idx < n_set)
    n, eo = idx.size, c * s * s
    mats = fixed_matrices(hs, ws, s, s)[:n]
    ar = Arena.sized(ctx.device, [x.size, n, 6 * n, n * eo, n * eo, n * eo])
    set_dev = ar.put(lay(x, sl), name="set")
    idx_dev = ar.put(idx, align=4, name="idx").view(torch.int32)
    mats_dev = ar.put(mats, align=4, name="mats")
    out = {f: ar.take(n * eo, name=f) for f in FIELDS}
    safe_dev = torch.as_tensor(np.where(inside, idx, 0).astype(np.int32)).to(ctx.device)
    want = composition(ctx, set_dev, n_set, c, hs, ws, sl, safe_dev, mats_dev, None, n, s, cs, ol, 0)
    for subset in SUBSETS:
        for f in FIELDS:
            out[f].fill_(-7.0)
        warp_c2f(ctx, set_dev, n_set, c, hs, ws, sl, idx_dev, mats_dev, None, n, s, cs, *[out[f] if f in subset else None for f in FIELDS], ol, 0)
        torch.cuda.synchronize()
        ar.assert_guards("fg_warp_c2f with indices outside the set, %r" % (subset,))
        for f in FIELDS:
            got = bits(out[f].cpu().numpy()).reshape(n, eo)
            if f not in subset:
                assert (got == np.float32(-7.0).view(np.int32)).all(), "%s was not asked for and was written" % f
                continue
            assert (got[~inside] == NAN_BITS).all(), "%s: an image of an index outside the set is not all quiet NaN" % f
            assert np.array_equal(got[inside], want[f].reshape(n, eo)[inside]), "%s: a neighbour of a NaN image differs" % f


def test_sizes_above_the_lds_limits_are_refused_on_the_device(ctx):
    from face_generator_amd.runtime import FgError
    t = torch.zeros(2 * 16388, device=ctx.device)
    i = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    with pytest.raises(FgError, match="16388"):
        warp_c2f(ctx, t, 1, 1, 4, 4097, 1, i, t, None, 1, 4, 2, t[16388:], None, None, 1, 0)
    with pytest.raises(FgError, match="16900"):
        warp_c2f(ctx, t, 1, 1, 4, 4, 1, i, t, None, 1, 130, 2, t[16388:], None, None, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# AugmentedResult
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,hs,s,cs,fill", [(3, 20, 16, 8, "constant"), (1, 16, 16, 5, "edge"), (3, 40, 32, 16, "constant")])
def test_gather_fields_equals_the_restatements_on_the_host_copy(ctx, c, hs, s, cs, fill):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    x = images_01(np.random.default_rng(31), (13, c, hs, hs))
    res = dataset_c2f.toResultAugmented(x, cs, s, Augmenter((s, s), seed=77, fill=fill), ctx=ctx)
    twin = Augmenter((s, s), seed=77, fill=fill)
    assert res.size() == len(res) == 13
    for picks, fields, layout in (([3, 12, 0, 3, 7], ("diff", "coarse"), "nhwc"), (list(range(13)), ("fine", "coarse", "diff"), "nchw"),
                                  ([5], ("coarse",), "nhwc"), (torch.tensor([1, 1, 2], dtype=torch.int32, device=ctx.device), ("coarse", "fine"), "nchw")):
        got = res.gather_fields(picks, fields, layout=layout)
        host_picks = picks.tolist() if torch.is_tensor(picks) else picks
        mats, gains = twin.draw(len(host_picks), (hs, hs))
        want = restated(x, host_picks, mats, gains, s, cs, twin.fill_code)
        assert len(got) == len(fields)
        for f, g in zip(fields, got):
            assert tuple(g.shape) == ((len(host_picks), s, s, c) if layout == "nhwc" else (len(host_picks), c, s, s))
            same_bits(g.cpu(), torch.as_tensor(lay(want[f], 0 if layout == "nhwc" else 1)), "gather_fields(%s, %r, %s): %s" % (host_picks, fields, layout, f))
    # diff and coarse of one call stem from one transform: fine - coarse of the same call, recomputed on the host, is diff
    fine, coarse, diff = (t.cpu().numpy() for t in res.gather_fields([0, 6, 12, 6], ("fine", "coarse", "diff")))
    twin.draw(4, (hs, hs))
    assert np.array_equal(bits(diff), bits(fine - coarse)) and (fine - coarse).dtype == np.float32 and diff.any()
    # gather is the one-field form, [i] the example of one fresh transform
    one = res.gather([2, 9], "diff", layout="nchw")
    mats, gains = twin.draw(2, (hs, hs))
    same_bits(one.cpu(), torch.as_tensor(restated(x, [2, 9], mats, gains, s, cs, twin.fill_code)["diff"]), "gather(.., 'diff')")
    ex = res[4]
    mats, gains = twin.draw(1, (hs, hs))
    want = restated(x, [4], mats, gains, s, cs, twin.fill_code)
    for f in FIELDS:
        same_bits(getattr(ex, f), torch.as_tensor(want[f][0]), "res[4]." + f)
    assert twin.rng.getstate() == res.augment.rng.getstate()


# ---------------------------------------------------------------------------------------------------------------------------------
# an epoch and approxParzen on an AugmentedResult against the same loops fed from the host
# ---------------------------------------------------------------------------------------------------------------------------------
class HostC2FDataset:
    """dataset[i] as the test computes it, in the order the host-fed loops pull: an example is warped (warp_ref) and scaled
    (oracle.image_scale) when its first field is read, under the next draw of an Augmenter of the test's own.  The real half of a D
    iteration reads .diff of its picks and then .coarse of the same picks from fresh examples: a .coarse read takes over the oldest
    transform a .diff read left behind, if there is one, and draws otherwise (the fake half's and G's conds; approxParzen reads
    .coarse and .fine of one example)."""

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
                    t = o.aug.draw(1, o.images.shape[2:])
                    if field == "diff":
                        o.left_by_diff.append((self.i, t))
                self.fields = {f: v[0] for f, v in restated(o.images, [self.i], t[0], t[1], o.s, o.cs, o.aug.fill_code).items()}
            return self.fields[field]

    def __init__(self, images, s, cs, augmenter):
        self.images, self.s, self.cs, self.aug, self.left_by_diff = images, s, cs, augmenter, []

    def size(self):
        return len(self.images)

    def __getitem__(self, i):
        return HostC2FDataset.Lazy(self, i)


def c2f_epoch(ctx, make_data, tmp_path):
    from face_generator_amd import adversarial_c2f
    from face_generator_amd.state import S
    dnG, dnD = c2f_setup(ctx, 16, 8, tmp_path)
    S.OPT["N_epoch"] = 20                   # batches of 8, 8, 8, 8 and 4
    start = (dnG.params.cpu(), dnD.params.cpu())
    data = make_data()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        adversarial_c2f.train(data)
    st = final_state(S._trainer, dnG, dnD, text.getvalue())
    adversarial_c2f.best_dist = -1.0        # (no .bestnet from a test)
    with contextlib.redirect_stdout(io.StringIO()):
        st["parzen"] = adversarial_c2f.approxParzen(data, 3, 4)
    st["rng_after_parzen"], st["noise_after_parzen"] = S.rng.getstate(), S.noise_offset
    return st, start, data


def test_c2f_train_epoch_and_parzen_on_an_augmented_result_equal_the_host_fed_loops(ctx, tmp_path):
    """adversarial_c2f.train at S = 16, cs = 8, batch 8, N_epoch = 20, D_iterations = 2 on a set stored with a margin of 2 px per side,
    then approxParzen(3, 4).  Fresh nets and the same seeds three times: an AugmentedResult, a host dataset whose examples the test
    warps and scales itself with the same draws, and the un-augmented ResidentResult for the S.rng picks."""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    images = images_01(np.random.default_rng(10), (11, 3, 20, 20))
    aug = Augmenter((16, 16), seed=5)
    res, start_r, _ = c2f_epoch(ctx, lambda: dataset_c2f.toResultAugmented(images, 8, 16, aug, ctx=ctx), tmp_path)
    host_data = HostC2FDataset(images, 16, 8, Augmenter((16, 16), seed=5))
    host, start_h, _ = c2f_epoch(ctx, lambda: host_data, tmp_path)
    plain, _, _ = c2f_epoch(ctx, lambda: dataset_c2f.toResultResident(torch.as_tensor(images[:, :, 2:-2, 2:-2]), 8, 16, ctx=ctx), tmp_path)
    same_bits(start_h[0], start_r[0], "initial G parameters")
    same_bits(start_h[1], start_r[1], "initial D parameters")
    assert host["steps"] == (10, 5) if "steps" in host else host["tD"] == 10
    assert not torch.equal(host["pD"], start_h[1]) and not torch.equal(host["pG"], start_h[0])
    assert host["parzen"].shape == (3,) and bool((host["parzen"] > 0).all()) and bool((host["parzen"] < 1e9).all())
    assert host_data.left_by_diff == []
    compare_states(host, res)
    twin = Augmenter((16, 16), seed=5)
    twin.draw(4 * (2 * (4 + 4) + 8) + (2 * (2 + 2) + 4) + 3, (20, 20))      # per iteration 2 x (half + half) + B, then one per parzen sample
    assert twin.rng.getstate() == aug.rng.getstate()
    assert res["rng"] == plain["rng"] and res["noise_offset"] == plain["noise_offset"]     # the picks are one stream with and without
    assert res["rng_after_parzen"] == plain["rng_after_parzen"]
    assert not torch.equal(res["pD"], plain["pD"])                          # ... and the augmentation did reach the training
