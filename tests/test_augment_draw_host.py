"""CPU-only: fg_draw_transforms (include/facegen_hip.h) and runtime.DeviceAugmenter in a planning-only context (FG_DEVICE_NONE): the
declaration and the export, every refusal with its code and message and without a launch, the launch list of a draw, the Lua side
as far as parsing goes -- and the header's contract restated in numpy (Philox4x32-10, the picks, sin / cos of whole degrees by the
stated polynomial, the matrix in float64 with every operation rounded on its own), which tests/test_gpu_augment_draw.py holds the
device to bit for bit.  The restatement is checked here against libm, against runtime.Augmenter.matrix on the same picks, and on
the known answers (identity, mirror, range ends, the counter's carry)."""
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_ERR_INVALID = -1
LAUNCH_RE = re.compile(r"^fg-launch (.*) grid=(\d+),(\d+),(\d+) block=(\d+) lds=(\d+)$")
DRAW_KERNEL = "draw_transforms_kernel"               # the launch-site text
SPEC_FIELDS = ("hflip", "vflip", "zoom_equal", "zoom_lo", "zoom_hi", "rot_lo", "rot_hi", "shear_lo", "shear_hi", "tx_lo", "tx_hi", "ty_lo", "ty_hi",
               "gain_lo", "gain_hi")
# the reference's call (dataset/generate_dataset.py:43-48) at 32 x 32: round(5 * 32 / 84) = 2 px
DEFAULTS = dict(hflip=1, vflip=0, zoom_equal=1, zoom_lo=0.82, zoom_hi=1.10, rot_lo=-8, rot_hi=8, shear_lo=0, shear_hi=0, tx_lo=-2, tx_hi=2,
                ty_lo=-2, ty_hi=2, gain_lo=1.0 - 0.1, gain_hi=1.0 + 0.1)
EVERYTHING = dict(hflip=1, vflip=1, zoom_equal=0, zoom_lo=0.5, zoom_hi=2.0, rot_lo=-200, rot_hi=500, shear_lo=-10, shear_hi=10, tx_lo=-3, tx_hi=7,
                  ty_lo=-6, ty_hi=1, gain_lo=0.0, gain_hi=1.5)
NEUTRAL = dict(hflip=0, vflip=0, zoom_equal=1, zoom_lo=1.0, zoom_hi=1.0, rot_lo=0, rot_hi=0, shear_lo=0, shear_hi=0, tx_lo=0, tx_hi=0, ty_lo=0,
               ty_hi=0, gain_lo=1.0, gain_hi=1.0)
SINGLE = dict(hflip=0, vflip=0, zoom_equal=0, zoom_lo=0.9, zoom_hi=0.9, rot_lo=37, rot_hi=37, shear_lo=-5, shear_hi=-5, tx_lo=3, tx_hi=3, ty_lo=-1,
              ty_hi=-1, gain_lo=1.25, gain_hi=1.25)
SPECS = dict(defaults=DEFAULTS, everything=EVERYTHING, neutral=NEUTRAL, single=SINGLE)


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract in numpy: Philox4x32-10 from its definition, then the header operation by operation
# ---------------------------------------------------------------------------------------------------------------------------------
def philox_quads(seed, first, count):
    """quads first .. first + count - 1 (modulo 2^64) of the library's stream -> uint32 [count][4]: counter = (quad lo, quad hi, 0, 0),
    key = (seed lo, seed hi), ten rounds"""
    q = [(first + i) % 2 ** 64 for i in range(count)]
    c = [np.array([v & 0xFFFFFFFF for v in q], dtype=np.uint64), np.array([v >> 32 for v in q], dtype=np.uint64),
         np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def words(seed, offset, n):
    """image j owns the quads offset + 3j .. offset + 3j + 2 -> uint32 [n][12]"""
    return philox_quads(seed, offset, 3 * n).reshape(n, 12)


D = float.fromhex("0x1.1df46a2529d39p-6")
SIN_C = [(-1.0) ** i / math.factorial(2 * i + 1) for i in range(9)]         # a float by an exact integer: rounded once
COS_C = [(-1.0) ** i / math.factorial(2 * i) for i in range(10)]


def poly_sin(x):
    z = x * x
    p = np.full_like(x, SIN_C[8])
    for i in range(7, -1, -1):
        p = p * z + SIN_C[i]
    return x * p


def poly_cos(x):
    z = x * x
    p = np.full_like(x, COS_C[9])
    for i in range(8, -1, -1):
        p = p * z + COS_C[i]
    return p


def sincos_deg(k):
    """k: integers (any sign) -> (sin, cos) of k degrees, float64, as the header defines them"""
    k = np.asarray(k, dtype=np.int64)
    m = np.mod(k, 360)
    q, r = m // 90, m % 90
    low = r <= 45
    x = np.where(low, r, 90 - r).astype(np.float64) * D
    S, C = poly_sin(x), poly_cos(x)
    s0, c0 = np.where(low, S, C), np.where(low, C, S)
    s = np.select([q == 0, q == 1, q == 2, q == 3], [s0, c0, 0.0 - s0, 0.0 - c0])
    c = np.select([q == 0, q == 1, q == 2, q == 3], [c0, 0.0 - s0, 0.0 - c0, s0])
    return s, c


def int_pick(w, lo, hi):
    return lo + ((w.astype(np.uint64) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)


def picks_of(spec, seed, offset, n):
    """-> dict of arrays [n]: hf, vf (bool), zx, zy, gain (float64), rot, sh, tx, ty (int64)"""
    w = words(seed, offset, n)
    u = lambda col: (w[:, col] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    p = dict(hf=(w[:, 0] >> np.uint32(31) == 1) & bool(spec["hflip"]), vf=(w[:, 1] >> np.uint32(31) == 1) & bool(spec["vflip"]))
    p["zx"] = spec["zoom_lo"] + u(2) * (spec["zoom_hi"] - spec["zoom_lo"])
    p["zy"] = p["zx"] if spec["zoom_equal"] else spec["zoom_lo"] + u(3) * (spec["zoom_hi"] - spec["zoom_lo"])
    p["rot"], p["sh"] = int_pick(w[:, 4], spec["rot_lo"], spec["rot_hi"]), int_pick(w[:, 5], spec["shear_lo"], spec["shear_hi"])
    p["tx"], p["ty"] = int_pick(w[:, 6], spec["tx_lo"], spec["tx_hi"]), int_pick(w[:, 7], spec["ty_lo"], spec["ty_hi"])
    p["gain"] = spec["gain_lo"] + u(8) * (spec["gain_hi"] - spec["gain_lo"])
    return p


def matrices_of(p, hs, ws, ho, wo, sincos=sincos_deg):
    """the header's matrix in float64, one numpy operation per rounding -> float64 [n][6]"""
    zx, zy = p["zx"], p["zy"]
    sr, cr = sincos(p["rot"])
    srs, crs = sincos(p["rot"] + p["sh"])
    a, b, c, d = zx * cr, 0.0 - zy * srs, zx * sr, zy * crs
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, (0.0 - b) / det, (0.0 - c) / det, a / det
    cx, cy = wo // 2, ho // 2
    qx, qy = (cx + p["tx"]).astype(np.float64), (cy + p["ty"]).astype(np.float64)
    m = [ia + 0.0, ib + 0.0, (cx - (ia * qx + ib * qy)) + (ws - wo) / 2.0, ic + 0.0, id_ + 0.0, (cy - (ic * qx + id_ * qy)) + (hs - ho) / 2.0]
    hf, vf = p["hf"], p["vf"]
    m[0], m[1], m[2] = np.where(hf, 0.0 - m[0], m[0]), np.where(hf, 0.0 - m[1], m[1]), np.where(hf, (ws - 1) - m[2], m[2])
    m[3], m[4], m[5] = np.where(vf, 0.0 - m[3], m[3]), np.where(vf, 0.0 - m[4], m[4]), np.where(vf, (hs - 1) - m[5], m[5])
    return np.stack(m, 1)


def restated(spec, seed, offset, n, hs, ws, ho, wo):
    """fg_draw_transforms -> (mats float32 [n][6], gains float32 [n])"""
    p = picks_of(spec, seed, offset, n)
    with np.errstate(all="ignore"):
        return matrices_of(p, hs, ws, ho, wo).astype(np.float32), p["gain"].astype(np.float32)


def spec_dict(cspec):
    """an _lib.AugmentSpec -> the dict the restatement takes"""
    return {k: getattr(cspec, k) for k in SPEC_FIELDS}


def ordered(a):
    """float32 -> int64 that counts representable numbers (the distance of two floats in ulp, across zero as well)"""
    i = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def test_header_declares_and_library_exports_the_entry(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    assert "fg_draw_transforms" in decls and hasattr(plan_ctx.lib, "fg_draw_transforms")
    assert decls["fg_draw_transforms"][2] == ["ctx", "spec", "seed", "offset", "n", "hs", "ws", "ho", "wo", "mats", "gains"]
    hdr = open(_lib.HEADER).read()
    doc = hdr[hdr.index("the random transforms of dataset/generate_dataset.py"):hdr.index("int fg_draw_transforms")]
    for word in ("0x1.1df46a2529d39p-6", ">> 32", "offset + 3j", "contract", "FG_ERR_INVALID", "generate_dataset.py", "w >> 31", "2^-24",
                 "runtime.Augmenter.matrix", "typedef struct fg_augment_spec"):
        assert word in doc, word
    assert [f for f, _ in _lib.AugmentSpec._fields_] == list(SPEC_FIELDS)
    struct = re.sub(r"/\*.*?\*/", "", doc[doc.index("typedef struct fg_augment_spec"):], flags=re.S)
    assert re.findall(r"\b(?:int|double)\s+([^;]+);", struct) == ["hflip, vflip", "zoom_equal", "zoom_lo, zoom_hi", "rot_lo, rot_hi", "shear_lo, shear_hi",
                                                                 "tx_lo, tx_hi, ty_lo, ty_hi", "gain_lo, gain_hi"]


CHILD = r"""
import ctypes, sys, torch
sys.path.insert(0, %r)
from face_generator_amd import _lib
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib = ctx.lib
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
BASE = %r
M, G = torch.zeros(6 * 300), torch.zeros(300)
def call(tag, spec=True, mats=True, gains=True, n=4, hs=40, ws=40, ho=32, wo=32, h=True, **kw):
    s = _lib.AugmentSpec()
    for k, v in dict(BASE, **kw).items():
        setattr(s, k, v)
    mark(tag)
    rc = lib.fg_draw_transforms(ctx.h if h else None, ctypes.byref(s) if spec else None, 43, 5, n, hs, ws, ho, wo, M.data_ptr() if mats else None,
                                G.data_ptr() if gains else None)
    print("%%s\t%%d\t%%s" %% (tag, rc, lib.fg_last_error(ctx.h if h else None).decode()))
inf, nan = float("inf"), float("nan")
call("good")
call("null-ctx", h=False); call("null-spec", spec=False); call("null-mats", mats=False); call("n=-1", n=-1)
for k in ("hs", "ws", "ho", "wo"):
    for v in (0, -1):
        call("%%s=%%d" %% (k, v), **{k: v})
for k in ("hflip", "vflip", "zoom_equal"):
    for v in (-1, 2):
        call("%%s=%%d" %% (k, v), **{k: v})
call("zoom-lo>hi", zoom_lo=1.2, zoom_hi=1.1); call("zoom-0", zoom_lo=0.0); call("zoom-neg", zoom_lo=-0.5); call("zoom-nan", zoom_lo=nan)
call("zoom-hi-nan", zoom_hi=nan); call("zoom-inf", zoom_hi=inf)
call("gain-lo>hi", gain_lo=1.2, gain_hi=1.1); call("gain-neg", gain_lo=-0.1); call("gain-nan", gain_hi=nan); call("gain-inf", gain_hi=inf)
call("gain-lo-nan", gain_lo=nan)
call("rot-lo>hi", rot_lo=9, rot_hi=8); call("shear-lo>hi", shear_lo=1, shear_hi=0); call("tx-lo>hi", tx_lo=3, tx_hi=2); call("ty-lo>hi", ty_lo=3, ty_hi=2)
call("shear--90", shear_lo=-90); call("shear-90", shear_hi=90)
call("rot-wide", rot_lo=-2 ** 31, rot_hi=2 ** 31 - 1); call("tx-wide", tx_lo=-2 ** 30, tx_hi=2 ** 30); call("ty-wide", ty_lo=-2 ** 30 - 1, ty_hi=2 ** 30 - 1)
call("n=0", n=0)
call("no-gains", gains=False)
call("rot-2^31-values", rot_lo=-2 ** 30, rot_hi=2 ** 30 - 1)
call("shear-ends", shear_lo=-89, shear_hi=89)
call("gain-0", gain_lo=0.0, gain_hi=0.0)
for n in (1, 256, 257):
    call("n=%%d" %% n, n=n)
mark("end")
"""


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, DEFAULTS)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = l.split()[1]
            sections[cur] = []
        elif cur is not None and l.startswith("fg-launch"):
            m = LAUNCH_RE.match(l)
            assert m, l
            sections[cur].append((m.group(1),) + tuple(int(v) for v in m.groups()[1:]))
    rcs = {}
    for l in r.stdout.splitlines():
        tag, rc, msg = l.split("\t")
        assert tag not in rcs
        rcs[tag] = (int(rc), msg)
    return sections, rcs


def test_every_refusal_returns_its_code_names_the_entry_and_launches_nothing(child):
    sections, rcs = child
    refused = ["null-spec", "null-mats", "n=-1", "zoom-lo>hi", "zoom-0", "zoom-neg", "zoom-nan", "zoom-hi-nan", "zoom-inf", "gain-lo>hi", "gain-neg",
               "gain-nan", "gain-inf", "gain-lo-nan", "rot-lo>hi", "shear-lo>hi", "tx-lo>hi", "ty-lo>hi", "shear--90", "shear-90", "rot-wide", "tx-wide",
               "ty-wide"]
    refused += ["%s=%d" % (k, v) for k in ("hs", "ws", "ho", "wo") for v in (0, -1)]
    refused += ["%s=%d" % (k, v) for k in ("hflip", "vflip", "zoom_equal") for v in (-1, 2)]
    assert len(refused) == 37
    for tag in refused:
        rc, msg = rcs[tag]
        assert rc == FG_ERR_INVALID, (tag, rc)
        assert "fg_draw_transforms" in msg, (tag, msg)
        assert sections[tag] == [], (tag, sections[tag])
    rc, msg = rcs["null-ctx"]
    assert rc == FG_ERR_INVALID and "fg_draw_transforms" in msg and sections["null-ctx"] == []


def test_an_empty_draw_launches_nothing_and_a_draw_is_one_launch_of_one_thread_per_image(child):
    sections, rcs = child
    assert rcs["n=0"][0] == 0 and sections["n=0"] == []
    for tag, blocks in (("good", 1), ("no-gains", 1), ("rot-2^31-values", 1), ("shear-ends", 1), ("gain-0", 1), ("n=1", 1), ("n=256", 1), ("n=257", 2)):
        assert rcs[tag][0] == 0, (tag, rcs[tag])
        assert sections[tag] == [(DRAW_KERNEL, blocks, 1, 1, 256, 0)], (tag, sections[tag])


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_polynomial_is_libm_within_1e_15_and_exact_at_the_multiples_of_90():
    k = np.arange(-400, 401)
    s, c = sincos_deg(k)
    worst = max(max(abs(float(s[i]) - math.sin(math.radians(int(k[i])))), abs(float(c[i]) - math.cos(math.radians(int(k[i]))))) for i in range(k.size))
    print("polynomial against libm, k = -400 .. 400: worst |difference| %.3g" % worst)
    assert worst <= 1e-15
    exact = {0: (0.0, 1.0), 90: (1.0, 0.0), 180: (0.0, -1.0), 270: (-1.0, 0.0)}
    for i in np.nonzero(k % 90 == 0)[0]:
        assert (float(s[i]), float(c[i])) == exact[int(k[i]) % 360], int(k[i])
    assert D == math.pi / 180 and len(SIN_C) == 9 and len(COS_C) == 10 and SIN_C[1] == -1.0 / 6.0 and COS_C[9] == -1.0 / 6402373705728000.0


@pytest.mark.parametrize("name,hs,ws,ho,wo", [("defaults", 32, 32, 32, 32), ("defaults", 40, 40, 32, 32), ("everything", 40, 40, 32, 32), ("everything", 5, 7, 3, 4),
                                              ("single", 9, 8, 5, 7)])
def test_the_matrices_agree_with_augmenter_matrix_on_the_same_picks_within_one_ulp(name, hs, ws, ho, wo):
    """runtime.Augmenter.matrix takes sin and cos from libm; on the picks of the restatement both give the same fp32 matrix, at most
    one ulp apart in an entry.  Where the rotation, or rotation + shear, is a multiple of 90 degrees the header's sin / cos are exactly
    0 and +-1 while libm, handed the rounded radians, returns 6.1e-17 for cos(pi / 2) and up to 3.7e-16 for sin(3 pi) (-200 .. 510
    degrees): an entry that is exactly 0 here and 1e-16 there has no distance in ulp, and the difference is libm's.  Those picks are
    held to an absolute bar instead: 3.7e-16 x 1 / zoom (at most 2) x a coordinate (at most 40) = 3e-14, rounded up to 1e-13."""
    from face_generator_amd.runtime import Augmenter
    spec, n = SPECS[name], 3000
    p = picks_of(spec, 9, 11, n)
    mine = matrices_of(p, hs, ws, ho, wo).astype(np.float32)
    host = Augmenter((ho, wo))
    theirs = np.array([host.matrix((bool(p["hf"][j]), bool(p["vf"][j]), float(p["zx"][j]), float(p["zy"][j]), int(p["rot"][j]), int(p["sh"][j]),
                                    int(p["tx"][j]), int(p["ty"][j]), None), (hs, ws)) for j in range(n)], dtype=np.float64).astype(np.float32)
    quadrant = (p["rot"] % 90 == 0) | ((p["rot"] + p["sh"]) % 90 == 0)
    quadrant &= (p["rot"] != 0) | (p["sh"] != 0)                             # sin(0) = 0 and cos(0) = 1 in libm as well
    ulps = np.abs(ordered(mine) - ordered(theirs))
    apart = ulps[~quadrant]
    print("%s %dx%d -> %dx%d: %d of %d entries differ, by at most %d ulp; %d picks at a multiple of 90 degrees" % (
        name, hs, ws, ho, wo, int((apart > 0).sum()), apart.size, int(apart.max()), int(quadrant.sum())))
    assert int(apart.max()) <= 1
    assert (~quadrant).sum() >= 0.9 * n
    # at a multiple of 90 degrees: one ulp as everywhere, or -- an entry that is 0 on one side -- the absolute bar
    absolute = np.abs(mine[quadrant].astype(np.float64) - theirs[quadrant].astype(np.float64))
    assert bool(((ulps[quadrant] <= 1) | (absolute <= 1e-13)).all())


@pytest.mark.parametrize("hs,ws,ho,wo", [(32, 32, 32, 32), (40, 40, 32, 32), (5, 7, 3, 4), (9, 9, 9, 9), (41, 40, 32, 32)])
def test_a_neutral_spec_is_the_exact_identity_and_a_flip_the_exact_mirror(hs, ws, ho, wo):
    mats, gains = restated(NEUTRAL, 43, 0, 50, hs, ws, ho, wo)
    ident = np.array([1, 0, (ws - wo) / 2.0, 0, 1, (hs - ho) / 2.0], dtype=np.float32)
    assert np.array_equal(mats, np.tile(ident, (50, 1))) and not np.signbit(mats).any()
    assert np.array_equal(gains, np.ones(50, dtype=np.float32))
    mats, _ = restated(dict(NEUTRAL, hflip=1), 43, 0, 50, hs, ws, ho, wo)
    flipped = words(43, 0, 50)[:, 0] >> 31 == 1
    assert 10 < flipped.sum() < 40
    mirror = np.array([-1, 0, (ws - 1) - (ws - wo) / 2.0, 0, 1, (hs - ho) / 2.0], dtype=np.float32)
    assert np.array_equal(mats[flipped], np.tile(mirror, (int(flipped.sum()), 1))) and np.array_equal(mats[~flipped], np.tile(ident, (int((~flipped).sum()), 1)))
    mats, _ = restated(dict(NEUTRAL, vflip=1), 43, 0, 50, hs, ws, ho, wo)
    flipped = words(43, 0, 50)[:, 1] >> 31 == 1
    mirror = np.array([1, 0, (ws - wo) / 2.0, 0, -1, (hs - 1) - (hs - ho) / 2.0], dtype=np.float32)
    assert np.array_equal(mats[flipped], np.tile(mirror, (int(flipped.sum()), 1))) and np.array_equal(mats[~flipped], np.tile(ident, (int((~flipped).sum()), 1)))


def test_the_picks_of_4096_draws_stay_inside_their_ranges_and_reach_both_ends():
    p = picks_of(DEFAULTS, 43, 0, 4096)
    for key, lo, hi in (("rot", -8, 8), ("tx", -2, 2), ("ty", -2, 2), ("sh", 0, 0)):
        assert int(p[key].min()) == lo and int(p[key].max()) == hi, key
    assert set(p["rot"].tolist()) == set(range(-8, 9))
    for key, lo, hi in (("zx", 0.82, 1.10), ("gain", 0.9, 1.1)):
        assert lo <= float(p[key].min()) < lo + 0.01 and hi - 0.01 < float(p[key].max()) <= hi, key
    assert p["zy"] is p["zx"] and not p["vf"].any() and 1800 < int(p["hf"].sum()) < 2300
    p = picks_of(EVERYTHING, 43, 0, 4096)
    for key, lo, hi in (("rot", -200, 500), ("sh", -10, 10), ("tx", -3, 7), ("ty", -6, 1)):
        assert int(p[key].min()) == lo and int(p[key].max()) == hi, key
    assert not np.array_equal(p["zx"], p["zy"]) and 0.5 <= float(p["zy"].min()) and float(p["zy"].max()) <= 2.0 and p["vf"].any()
    # the ends of a pick: word 0 gives lo, word 2^32 - 1 gives hi, for a range of 2^31 values as well
    w = np.array([0, 2 ** 32 - 1, 2 ** 31], dtype=np.uint32)
    assert int_pick(w, -8, 8).tolist() == [-8, 8, 0] and int_pick(w, -2 ** 30, 2 ** 30 - 1).tolist() == [-2 ** 30, 2 ** 30 - 1, 0]


def test_a_draw_is_a_prefix_of_a_longer_one_across_the_counters_carry():
    import test_gpu_pointwise_paths as T
    seed = (0xDEADBEEF << 32) | 0x12345678
    for offset in (0, 5, 2 ** 32 - 2, 2 ** 40 + 3, 2 ** 64 - 4):
        # the words are the library's stream, by the numpy Philox the RNG entries are held to
        want = T.philox_words(seed, offset, 27)
        assert np.array_equal(words(seed, offset, 9).reshape(27, 4), want), offset
        m9, g9 = restated(EVERYTHING, seed, offset, 9, 40, 40, 32, 32)
        m5, g5 = restated(EVERYTHING, seed, offset, 5, 40, 40, 32, 32)
        m4, g4 = restated(EVERYTHING, seed, (offset + 15) % 2 ** 64, 4, 40, 40, 32, 32)
        assert np.array_equal(np.concatenate([m5, m4]).view(np.int32), m9.view(np.int32)) and np.array_equal(np.concatenate([g5, g4]), g9), offset
    hi = philox_quads(seed, 2 ** 32 - 1, 2)
    assert not np.array_equal(hi[1], philox_quads(seed, 0, 1)[0])            # quad 2^32 is not quad 0: the carry reaches word 1


# ---------------------------------------------------------------------------------------------------------------------------------
# DeviceAugmenter
# ---------------------------------------------------------------------------------------------------------------------------------
def test_device_augmenter_takes_augmenters_arguments_and_refuses_fractions(plan_ctx):
    import inspect
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter, FgError
    a, d = inspect.signature(Augmenter.__init__).parameters, inspect.signature(DeviceAugmenter.__init__).parameters
    assert list(d)[:-1] == list(a) and list(d)[-1] == "offset" and d["offset"].default == 0
    assert all(d[k].default == a[k].default for k in a)
    for kw in (dict(rotation_deg=(-7.5, 7.5)), dict(shear_deg=2.5), dict(translation_x_px=(0, 1.5)), dict(translation_y_px=0.25)):
        with pytest.raises(FgError, match="whole"):
            DeviceAugmenter((32, 32), **kw)
    aug = DeviceAugmenter((32, 32))
    assert spec_dict(aug.spec()) == DEFAULTS and aug.state() == (43, 0) and isinstance(aug, Augmenter)
    wide = DeviceAugmenter((5, 7), hflip=False, vflip=True, scale_to_percent=(0.5, 2.0), scale_axis_equally=False, rotation_deg=(-200.0, 500), shear_deg=10,
                           translation_x_px=(-3, 7), translation_y_px=(-6, 1), brightness_change=0.25, fill="edge", seed=2 ** 63 + 5, offset=2 ** 32 - 2)
    assert spec_dict(wide.spec()) == dict(EVERYTHING, hflip=0, gain_lo=0.75, gain_hi=1.25) and wide.state() == (2 ** 63 + 5, 2 ** 32 - 2) and wide.fill_code == 1
    with pytest.raises(FgError):
        wide.set_state(-1, 0)
    with pytest.raises(FgError):
        wide.set_state(1, 2 ** 64)
    with pytest.raises(FgError):
        wide.draw_one()
    # the entry refuses what the constructor lets through: a shear of 90 degrees has no inverse
    with pytest.raises(FgError, match="fg_draw_transforms"):
        DeviceAugmenter((8, 8), shear_deg=90).draw_device(plan_ctx, 2, (8, 8))


def test_device_augmenter_rides_where_an_augmenter_does_and_leaves_every_host_rng_alone(plan_ctx):
    from face_generator_amd import dataset_c2f, ops
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset
    from face_generator_amd.state import S
    S.reset()
    S.rng = random.Random(11)
    before = S.rng.getstate()
    py_state, np_state, torch_state = random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state()
    x = np.random.default_rng(2).uniform(0, 1, (5, 3, 12, 12)).astype(np.float32)
    aug = DeviceAugmenter((8, 8), seed=3, offset=2 ** 64 - 6)
    own = aug.rng.getstate()
    ds = DeviceDataset(plan_ctx, x, augment=aug)                            # set_augment's type check
    assert ds.gather([0, 4, 4]).shape == (3, 8, 8, 3) and aug.state() == (3, 3)          # 3n quads on, modulo 2^64
    assert ds.gather([1], layout="nchw").shape == (1, 3, 8, 8) and ds.gather([]).shape == (0, 8, 8, 3) and aug.state() == (3, 6)
    assert ds.gather([2, 3], augment=False).shape == (2, 12, 12, 3) and aug.state() == (3, 6)
    ds.set_augment(None)
    ds.set_augment(aug)
    res = dataset_c2f.toResultAugmented(x, 4, 8, DeviceAugmenter((8, 8), seed=4), ctx=plan_ctx)        # AugmentedResult's type check
    diff, coarse = res.gather_fields([0, 1, 1, 3], ("diff", "coarse"))
    assert diff.shape == coarse.shape == (4, 8, 8, 3) and res.augment.state() == (4, 12)            # one draw for both fields
    assert res.gather([2], "fine", layout="nchw").shape == (1, 3, 8, 8) and res.augment.state() == (4, 15)
    both = aug.draw_device(plan_ctx, 5, (12, 12))
    assert both.shape == (35,) and both.dtype == torch.float32 and aug.state() == (3, 21)
    mats, gains = aug.draw(2, (12, 12), ctx=plan_ctx)
    assert mats.shape == (2, 6) and gains.shape == (2,) and mats.dtype == gains.dtype == np.float32 and aug.state() == (3, 27)
    m, g = ops.draw_transforms(aug, 4, (12, 12), None, 7, 9, ctx=plan_ctx)
    assert m.shape == (4, 6) and g.shape == (4,) and aug.state() == (3, 27)                           # the wrapper is stateless
    m, g = ops.draw_transforms(aug.spec(), 0, (12, 12), (8, 8), 7, 9, ctx=plan_ctx)
    assert m.shape == (0, 6) and g.shape == (0,)
    fresh = DeviceAugmenter((8, 8))
    fresh.set_state(*aug.state())
    assert fresh.state() == (3, 27)
    assert aug.rng.getstate() == own                                         # not even its own random.Random moves
    assert S.rng.getstate() == before and random.getstate() == py_state
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


GATHER_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from face_generator_amd import dataset_c2f
from face_generator_amd.runtime import get_context, DeviceAugmenter, DeviceDataset
ctx = get_context(-1)
x = np.zeros((7, 3, 6, 8), dtype=np.float32)
ds = DeviceDataset(ctx, x, augment=DeviceAugmenter((4, 6)))
res = dataset_c2f.toResultAugmented(np.zeros((7, 3, 10, 10), dtype=np.float32), 4, 8, DeviceAugmenter((8, 8)), ctx=ctx)
sys.stderr.write("fg-mark gather\n"); sys.stderr.flush()
ds.gather([0, 1, 2, 3])
sys.stderr.write("fg-mark fields\n"); sys.stderr.flush()
res.gather_fields([0, 1, 2], ("diff", "coarse"))
sys.stderr.write("fg-mark end\n"); sys.stderr.flush()
"""


def test_a_gather_with_a_device_augmenter_is_the_draw_kernel_and_one_warp_kernel():
    r = subprocess.run([sys.executable, "-c", GATHER_CHILD % ROOT], env=dict(os.environ, FG_LAUNCH_LOG="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = sections.setdefault(l.split()[1], [])
        elif cur is not None and l.startswith("fg-launch"):
            name = LAUNCH_RE.match(l).group(1)
            cur.append(name if name == DRAW_KERNEL else re.match(r"\(?\s*([A-Za-z_]\w*)", name).group(1))
    assert sections["gather"] == [DRAW_KERNEL, "warp_images_kernel"], sections
    assert sections["fields"] == [DRAW_KERNEL, "warp_c2f_kernel"], sections


# ---------------------------------------------------------------------------------------------------------------------------------
def test_lua_side_parses_and_binds_the_entry():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    fg = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    parsed = lua_parser.parse(fg)
    names = [q for (_, q, _, _) in parsed.functions]
    assert "M.drawTransforms" in names and "M.augmenter" in names
    for probe in ("function M.drawTransforms(spec, seed, offset, n, hs, ws, ho, wo)", "function M.augmenter(outH, outW, opts)",
                  "C.fg_draw_transforms(ctx, cspec, seed, offset, n, hs, ws, ho, wo, mats.ptr, gains.ptr)", "return draw, state",
                  "offset = offset + 3 * n"):
        assert probe in fg, probe
    for name in ("hflip", "vflip", "scale_to_percent", "scale_axis_equally", "rotation_deg", "shear_deg", "translation_x_px", "translation_y_px",
                 "brightness_change"):
        assert "opts." + name in fg, name
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", fg, re.S).group(1)
    assert "int fg_draw_transforms(fg_ctx* ctx, const fg_augment_spec* spec, uint64_t seed, uint64_t offset, int n, int hs, int ws, int ho, int wo, " \
           "float* mats, float* gains);" in cdef
    assert "typedef struct fg_augment_spec { int hflip, vflip; int zoom_equal; double zoom_lo, zoom_hi; int rot_lo, rot_hi; int shear_lo, shear_hi; " \
           "int tx_lo, tx_hi, ty_lo, ty_hi; double gain_lo, gain_hi; } fg_augment_spec;" in cdef
    assert cdef.index("} fg_augment_spec;") < cdef.index("int fg_draw_transforms(")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"
    # the c2f loop says how to pass it, and FG.augmentedResult still takes any draw function
    c2f = open(os.path.join(ROOT, "lua", "adversarial_c2f_hip.lua")).read()
    lua_parser.parse(c2f)
    assert "FG.augmenter(" in c2f and "function M.augmentedResult(fineImages, coarseScale, fineScale, draw, fill)" in fg
