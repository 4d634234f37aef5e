"""CPU-only checks of the references that tests/test_gpu_pointwise_paths.py holds the device to: the numpy Philox4x32-10 against the
Random123 known answers, the measured Box-Muller bar, and the large-offset BatchNorm bar against the float64 reference fed with the
fp32-rounded mean."""
import numpy as np

import test_gpu_pointwise_paths as T


def words(s):
    return [int(w, 16) for w in s.split()]


def test_numpy_philox_gives_the_random123_known_answers():
    kat = [("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = T.philox4x32_10(np.array([words(ctr)], np.uint32), words(key))
        assert [int(v) for v in got[0]] == words(want), (ctr, key, ["%08x" % int(v) for v in got[0]])
    # all three in one call (the vectorised form), and the library's counter layout: the carry into the second counter word
    got = T.philox4x32_10(np.array([words(c) for c, _, _ in kat[:1]] * 3, np.uint32), (0, 0))
    assert (got == got[0]).all()
    a = T.philox_words(5, 2 ** 32 - 2, 4)
    assert (a[2] == T.philox4x32_10(np.array([[0, 1, 0, 0]], np.uint32), (5, 0))[0]).all()
    assert (a[1] == T.philox4x32_10(np.array([[0xFFFFFFFF, 0, 0, 0]], np.uint32), (5, 0))[0]).all()
    seed = (0xDEADBEEF << 32) | 0x12345678
    assert (T.philox_words(seed, 2 ** 40 + 3, 1)[0] == T.philox4x32_10(np.array([[3, 256, 0, 0]], np.uint32), (0x12345678, 0xDEADBEEF))[0]).all()


def test_the_box_muller_bar_is_the_one_the_ledger_records():
    bar = T.measured_normal_bar()
    print("4 x max|float32 - float64 Box-Muller| over %d draws: %.3e" % (T.NORMAL_N, bar))
    assert 0 < bar < 1e-4                    # |z| <= 5.8: a handful of fp32 ulps of that
    text = open(__import__("dispatch_audit").LEDGER).read()
    assert "%.3e" % bar in text, "tests/DISPATCH_COVERAGE.md does not record the measured bar %.3e" % bar


def test_the_large_offset_bar_covers_the_fp32_rounded_mean():
    """the float64 reference fed with the saved mean rounded to fp32 stays inside bar + first-order term, for every output the term
    is added to; and a naive fp32 E[x^2] - E[x]^2 fails the variance outright at this offset"""
    M, C = T.OFFSET_CASE
    op = T.bn_operands(M, C, T.Src(4160), offset=1000.0)
    x32 = op["x"]
    naive = (x32 * x32).mean(0, dtype=np.float32) - x32.mean(0, dtype=np.float32) ** 2
    true = T.d64(x32).var(0)
    assert (np.abs(naive - true) > 10 * true).any()
    for slope in (0.25, None):
        r32 = T.bn_reference(op, slope, 0, mean=T.bn_reference(op, slope, 0)["mean"].astype(np.float32))
        r = T.bn_reference(op, slope, 0, pos=r32["z"] > 0)          # the backward branches of the rounded-mean run (see the GPU test)
        extra = T.offset_bars(op, r, slope)
        assert set(extra) == {"y", "gx", "gg", "gs", "mean", "rm", "ye"}
        for k, e in extra.items():
            if k == "gs" and slope is None:
                continue                     # no PReLU: no slope gradient
            base = dict(y=T.BAR["bn_y"], gx=T.BAR["bn_gx"] * max(1.0, np.abs(r["gx"]).max()), gg=T.BAR["bn_gparam"] * max(1.0, np.abs(r["gg"]).max()),
                        gs=T.BAR["bn_gparam"] * max(1.0, abs(float(r["gs"]))), mean=T.BAR["bn_mean"], rm=T.BAR["bn_running_mean"], ye=T.BAR["bn_y"])[k]
            dev = np.abs(r32[k] - r[k])
            print("slope %s %s: moved by %.3e, first-order term %.3e, bar %.3e" % (slope, k, float(np.max(dev)), float(np.max(e)), base))
            assert (dev <= base + e).all(), (slope, k, float(np.max(dev - e)))
