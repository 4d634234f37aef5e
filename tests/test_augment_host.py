"""CPU-only: fg_warp_images (include/facegen_hip.h) and the per-batch augmentation of a set resident in HBM (runtime.Augmenter,
DeviceDataset(augment=)) in a planning-only context (FG_DEVICE_NONE): the declaration and the export, every refusal with its code and
message and without a launch, the launch list of one warp per layout pair, the Augmenter's draws and matrices against a float64
restatement, S.rng left alone, the refusal of dataset_c2f.toResultResident, and the Lua side as far as parsing goes.

The two references of the kernel live here and are imported by tests/test_gpu_augment.py: warp_ref, the header's contract restated
in numpy fp32 in the stated operation order (the kernel must match it bit for bit), and warp_ref64, scipy.ndimage.map_coordinates
in float64 (an independent pin: order=1, mode "grid-constant" with cval 0 for fill 0, "nearest" for fill 1).  They are compared
with each other here, on the CPU, within the bar the GPU test holds the kernel to."""
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
FG_ERR_INVALID, FG_ERR_UNSUPPORTED = -1, -4
LAUNCH_RE = re.compile(r"^fg-launch \(?\s*([A-Za-z_]\w*)[^)]*\)? grid=(\d+),(\d+),(\d+) block=(\d+) lds=(\d+)$")
NAN_BITS = 0x7FC00000
# |fp32 restatement - float64 reference| for finite pixels in [0, 1]: a coordinate below 128 takes four fp32 roundings (two
# products, two sums: at most 4 x 2^-18 = 1.5e-5, 3e-5 with the fraction's subtraction), a bilinear surface over values in [0, 1]
# has slope at most 1 per pixel and axis (6e-5 for both), the gain is at most 1.1 and the interpolation's own roundings are a few ulp
BAR_64 = 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the contract in numpy fp32, (b) the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def warp_ref(x, idx, mats, gains, ho, wo, fill):
    """x: float32 [n_set][c][hs][ws]; idx: ints; mats: float32 [n][6] or None; gains: float32 [n] or None -> float32 [n][c][ho][wo].
    Every operation is one fp32 ufunc, in the order include/facegen_hip.h states."""
    f32 = np.float32
    n_set, c, hs, ws = x.shape
    out = np.empty((len(idx), c, ho, wo), dtype=f32)
    xf, yf = np.arange(wo, dtype=f32)[None, :], np.arange(ho, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        for j, i in enumerate(idx):
            if not 0 <= int(i) < n_set:
                out[j].view(np.int32)[...] = NAN_BITS
                continue
            img = x[int(i)]
            m = np.array([1, 0, 0, 0, 1, 0], dtype=f32) if mats is None else np.asarray(mats[j], dtype=f32)
            sx = (m[0] * xf + m[1] * yf) + m[2]
            sy = (m[3] * xf + m[4] * yf) + m[5]
            assert sx.dtype == f32 and sy.dtype == f32
            if fill == 1:
                sx = np.fmin(np.fmax(sx, f32(0)), f32(ws - 1))
                sy = np.fmin(np.fmax(sy, f32(0)), f32(hs - 1))
                inside = np.ones((ho, wo), dtype=bool)
            else:
                inside = (sx > f32(-1)) & (sx < f32(ws)) & (sy > f32(-1)) & (sy < f32(hs))
                sx, sy = np.where(inside, sx, f32(0)), np.where(inside, sy, f32(0))         # (no conversion of what failed the test)
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0f, sy - y0f
            x0, y0 = x0f.astype(np.int32), y0f.astype(np.int32)

            def tap(yi, xi):
                ok = (yi >= 0) & (yi < hs) & (xi >= 0) & (xi < ws)
                return np.where(ok[None], img[:, np.clip(yi, 0, hs - 1), np.clip(xi, 0, ws - 1)], f32(0))
            a, b, cc, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
            top = a + (b - a) * fx[None]
            bot = cc + (d - cc) * fx[None]
            v = top + (bot - top) * fy[None]
            v = np.where(inside[None], v, f32(0))
            if gains is not None:
                v = np.fmin(np.fmax(v * f32(gains[j]), f32(0)), f32(1))
            assert v.dtype == f32
            out[j] = v
    return out


def warp_ref64(x, idx, mats, gains, ho, wo, fill):
    """the same map in float64 through scipy (finite matrices, indices inside the set)"""
    from scipy.ndimage import map_coordinates
    n_set, c, hs, ws = x.shape
    out = np.empty((len(idx), c, ho, wo), dtype=np.float64)
    yy, xx = np.meshgrid(np.arange(ho, dtype=np.float64), np.arange(wo, dtype=np.float64), indexing="ij")
    for j, i in enumerate(idx):
        m = np.array([1, 0, 0, 0, 1, 0], dtype=np.float64) if mats is None else np.asarray(mats[j], dtype=np.float64)
        sx, sy = m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]
        for ch in range(c):
            v = map_coordinates(x[int(i), ch].astype(np.float64), [sy, sx], order=1, **(dict(mode="nearest") if fill == 1 else
                                                                                       dict(mode="grid-constant", cval=0.0)))
            out[j, ch] = v if gains is None else np.clip(v * float(gains[j]), 0.0, 1.0)
    return out


def fixed_matrices(hs, ws, ho, wo):
    """identity (with the crop's offset), both flips, integer and half-pixel shifts, rotations of 8 and 90 degrees about the centre,
    zoom 0.5 and 2: float32 [k][6], output pixel -> source pixel"""
    ox, oy = (ws - wo) / 2.0, (hs - ho) / 2.0
    cx, cy = (wo - 1) / 2.0, (ho - 1) / 2.0
    out = [[1, 0, ox, 0, 1, oy], [-1, 0, ws - 1 - ox, 0, 1, oy], [1, 0, ox, 0, -1, hs - 1 - oy], [1, 0, ox + 2, 0, 1, oy - 1],
           [1, 0, ox - 3, 0, 1, oy + 1], [1, 0, ox + 0.5, 0, 1, oy + 0.5], [1, 0, ox - 0.5, 0, 1, oy + 1.5]]
    for deg in (8, -8, 90):
        r = math.radians(deg)
        co, si = math.cos(r), math.sin(r)
        out.append([co, -si, cx + ox - co * cx + si * cy, si, co, cy + oy - si * cx - co * cy])
    for z in (0.5, 2.0):
        out.append([z, 0, cx + ox - z * cx, 0, z, cy + oy - z * cy])
    return np.array(out, dtype=np.float32)


def augmenter_restated(pick, out_hw, src_hw):
    """the matrix of one pick, float64, written independently of runtime.Augmenter.matrix: homogeneous 3 x 3 matrices, np.linalg.inv"""
    hf, vf, zx, zy, rot, sh, tx, ty, _ = pick
    (ho, wo), (hs, ws) = out_hw, src_hw
    r, s = np.deg2rad(rot), np.deg2rad(sh)
    A = np.array([[zx * np.cos(r), -zy * np.sin(r + s), tx], [zx * np.sin(r), zy * np.cos(r + s), ty], [0, 0, 1]], dtype=np.float64)
    cx, cy = int(wo / 2), int(ho / 2)

    def shift(dx, dy):
        return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], dtype=np.float64)
    inv = np.linalg.inv(shift(cx, cy) @ A @ shift(-cx, -cy))
    inv = shift((ws - wo) / 2.0, (hs - ho) / 2.0) @ inv
    if hf:
        inv = np.array([[-1, 0, ws - 1], [0, 1, 0], [0, 0, 1]], dtype=np.float64) @ inv
    if vf:
        inv = np.array([[1, 0, 0], [0, -1, hs - 1], [0, 0, 1]], dtype=np.float64) @ inv
    return inv[:2]


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
    assert "fg_warp_images" in decls and hasattr(plan_ctx.lib, "fg_warp_images")
    assert decls["fg_warp_images"][2] == ["ctx", "set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "out", "ho", "wo",
                                          "out_layout", "fill"]
    hdr = open(_lib.HEADER).read()
    doc = hdr[hdr.index("dataset[i] under a fresh random transform"):hdr.index("int fg_warp_images")]
    for word in ("generate_dataset.py", "sx = (m0*x + m1*y) + m2", "sy = (m3*x + m4*y) + m5", "top = a + (b - a)*fx", "fminf(fmaxf(v * gains[j], 0), 1)",
                 "quiet-NaN", "16384", "FG_ERR_UNSUPPORTED", "FG_ERR_INVALID", "16-byte"):
        assert word in doc, word


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: None if t is None else t.data_ptr())
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
n_set, c, hs, ws, ho, wo, n = 7, 3, 6, 8, 4, 6, 4
S, O, I = torch.zeros(n_set * c * hs * ws + 4), torch.zeros(n * c * hs * ws + 4), torch.zeros(n, dtype=torch.int32)
M, G = torch.zeros(6 * n), torch.ones(n)
good = dict(set=S, n_set=n_set, c=c, hs=hs, ws=ws, set_layout=1, idx=I, mats=M, gains=G, n=n, out=O, ho=ho, wo=wo, out_layout=0, fill=0)
def call(**kw):
    a = dict(good, **kw)
    for k in ("set", "idx", "mats", "gains", "out"):
        a[k] = P(a[k])
    return lib.fg_warp_images(ctx.h, *[a[k] for k in good])
def report(tag, rc):
    print("%%s\t%%d\t%%s" %% (tag, rc, lib.fg_last_error(ctx.h).decode()))
mark("good"); report("good", call())
for k in ("set", "idx", "out"):
    mark("null-" + k); report("null-" + k, call(**{k: None}))
for k in ("n_set", "c", "hs", "ws", "ho", "wo"):
    for v in (0, -1):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("n=-1"); report("n=-1", call(n=-1))
for k in ("set_layout", "out_layout", "fill"):
    for v in (-1, 2):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("no-mats-sizes"); report("no-mats-sizes", call(mats=None))
mark("no-mats-width"); report("no-mats-width", call(mats=None, ho=hs))
mark("out-2^31"); report("out-2^31", call(ho=1 << 15, wo=1 << 15))
mark("lds-16385"); report("lds-16385", call(c=1, hs=5, ws=3277))
mark("lds-big"); report("lds-big", call(c=3, hs=128, ws=128))
mark("lds-huge"); report("lds-huge", call(c=1 << 30, hs=1 << 30, ws=1 << 30))
mark("null-ctx"); print("null-ctx\t%%d\t" %% lib.fg_warp_images(None, P(S), n_set, c, hs, ws, 1, P(I), P(M), P(G), n, P(O), ho, wo, 0, 0))
mark("n=0"); report("n=0", call(n=0))
mark("lds-16384"); report("lds-16384", call(c=4, hs=64, ws=64, ho=2, wo=2, n_set=1))
mark("no-mats"); report("no-mats", call(mats=None, ho=hs, wo=ws))
mark("no-gains"); report("no-gains", call(gains=None))
for sl in (0, 1):
    for ol in (0, 1):
        for off in (0, 1):
            for fill in (0, 1):
                mark("lay-%%d-%%d-%%d-%%d" %% (sl, ol, off, fill))
                report("lay", call(set_layout=sl, out_layout=ol, set=S[off:], out=O[off:], fill=fill))
mark("gray"); report("gray", call(c=1, set_layout=0, out_layout=1))
mark("end")
"""


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = l.split()[1]
            sections[cur] = []
        elif cur is not None and l.startswith("fg-launch"):
            m = LAUNCH_RE.match(l)
            assert m, l
            sections[cur].append((m.group(1),) + tuple(int(v) for v in m.groups()[1:]) + (l,))
    rcs = {}
    for l in r.stdout.splitlines():
        tag, rc, msg = l.split("\t")
        rcs.setdefault(tag, []).append((int(rc), msg))
    return sections, rcs


def test_every_refusal_returns_its_code_names_the_entry_and_launches_nothing(child):
    sections, rcs = child
    assert rcs["good"] == [(0, rcs["good"][0][1])]
    invalid = ["null-set", "null-idx", "null-out", "n=-1", "no-mats-sizes", "no-mats-width", "out-2^31"]
    invalid += ["%s=%d" % (k, v) for k in ("n_set", "c", "hs", "ws", "ho", "wo") for v in (0, -1)]
    invalid += ["%s=%d" % (k, v) for k in ("set_layout", "out_layout", "fill") for v in (-1, 2)]
    for tag in invalid:
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_INVALID, (tag, rc)
        assert "fg_warp_images" in msg, (tag, msg)
        assert sections[tag] == [], (tag, sections[tag])
    for tag, size in (("lds-16385", "16385"), ("lds-big", "49152"), ("lds-huge", "")):
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_UNSUPPORTED and "fg_warp_images" in msg and size in msg and "16384" in msg, (tag, rc, msg)
        assert sections[tag] == [], (tag, sections[tag])
    assert rcs["null-ctx"][0][0] == FG_ERR_INVALID and sections["null-ctx"] == []


def test_an_empty_batch_launches_nothing_and_a_warp_is_one_launch_of_the_warp_kernel(child):
    sections, rcs = child
    assert rcs["n=0"][0][0] == 0 and sections["n=0"] == []
    assert all(rc == 0 for rc, _ in rcs["lay"]) and len(rcs["lay"]) == 16
    for tag in ("good", "no-mats", "no-gains", "lds-16384", "gray"):
        assert rcs[tag][0][0] == 0 and len(sections[tag]) == 1 and sections[tag][0][0] == "warp_images_kernel", (tag, rcs[tag], sections[tag])
    assert sections["lds-16384"][0][5] == 65536          # the 64 KB a launch gets without an attribute change
    inst = {(1, 1): "<true, true>", (1, 0): "<true, false>", (0, 1): "<false, true>", (0, 0): "<false, false>"}
    for (sl, ol), text in inst.items():
        for off in (0, 1):
            for fill in (0, 1):
                (name, gx, gy, gz, block, lds, line), = sections["lay-%d-%d-%d-%d" % (sl, ol, off, fill)]
                assert name == "warp_images_kernel" and text in line, line
                assert (gx, gy, gz, block) == (4, 1, 1, 256), line          # one block per output image: the exact count
                assert lds == 3 * 6 * 8 * 4, line                           # the source image
    assert "<true, true>" in sections["gray"][0][-1]                       # one channel: the two layouts are one order


# ---------------------------------------------------------------------------------------------------------------------------------
# Augmenter
# ---------------------------------------------------------------------------------------------------------------------------------
class CountingRandom:
    """a random.Random behind a log of the calls made to it (a proxy, not a subclass: a subclass that overrides random() makes
    randint() draw through it)"""

    def __init__(self, seed):
        self.inner, self.calls = random.Random(seed), []

    def uniform(self, a, b):
        self.calls.append("uniform")
        return self.inner.uniform(a, b)

    def random(self):
        self.calls.append("random")
        return self.inner.random()

    def randint(self, a, b):
        self.calls.append("randint")
        return self.inner.randint(a, b)


def test_the_same_seed_gives_the_same_draws_and_another_seed_others():
    from face_generator_amd.runtime import Augmenter
    a, b, c = Augmenter((32, 32)), Augmenter((32, 32), seed=43), Augmenter((32, 32), seed=44)
    ma, ga = a.draw(9, (40, 40))
    mb, gb = b.draw(9, (40, 40))
    mc, gc = c.draw(9, (40, 40))
    assert ma.dtype == ga.dtype == np.float32 and ma.shape == (9, 6) and ga.shape == (9,)
    assert np.array_equal(ma, mb) and np.array_equal(ga, gb) and not np.array_equal(ma, mc) and not np.array_equal(ga, gc)
    m2, g2 = a.draw(9, (40, 40))                                            # a fresh transform per call
    assert not np.array_equal(ma, m2)
    assert (ga >= np.float32(0.9)).all() and (ga <= np.float32(1.1)).all() and len(set(ga.tolist())) == 9
    assert (a.tx, a.ty) == ((-2, 2), (-2, 2)) and Augmenter((64, 64)).tx == (-4, 4) and Augmenter((16, 16)).ty == (-1, 1)   # round(5 * side / 84)


@pytest.mark.parametrize("hflip,vflip,equal,draws", [(True, False, True, ["random", "uniform"]), (False, False, True, ["uniform"]),
                                                     (True, True, False, ["random", "random", "uniform", "uniform"]),
                                                     (False, True, False, ["random", "uniform", "uniform"])])
def test_the_draw_count_per_image_follows_the_enabled_options(hflip, vflip, equal, draws):
    """flips only for the enabled axes, a second zoom unless both axes zoom equally, then rotation, shear, tx, ty, brightness"""
    from face_generator_amd.runtime import Augmenter
    aug = Augmenter((16, 16), hflip=hflip, vflip=vflip, scale_axis_equally=equal)
    aug.rng = CountingRandom(5)
    aug.draw(3, (16, 16))
    assert aug.rng.calls == (draws + ["randint"] * 4 + ["uniform"]) * 3


def test_neutral_parameters_give_exact_identities_and_flip_only_the_exact_mirror():
    from face_generator_amd.runtime import Augmenter
    neutral = dict(scale_to_percent=(1.0, 1.0), rotation_deg=0, shear_deg=0, translation_x_px=0, translation_y_px=0, brightness_change=0.0)
    for hw in ((32, 32), (5, 7), (9, 9), (64, 48)):
        mats, gains = Augmenter(hw, hflip=False, **neutral).draw(6, hw)
        assert np.array_equal(mats, np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (6, 1))) and not np.signbit(mats).any()
        assert np.array_equal(gains, np.ones(6, dtype=np.float32))
        mats, _ = Augmenter(hw, hflip=True, **neutral).draw(40, hw)
        flipped = (mats[:, 0] == -1)
        assert 5 < flipped.sum() < 35
        assert np.array_equal(mats[flipped], np.tile(np.array([-1, 0, hw[1] - 1, 0, 1, 0], dtype=np.float32), (int(flipped.sum()), 1)))
        assert np.array_equal(mats[~flipped], np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (int((~flipped).sum()), 1)))
        mats, _ = Augmenter(hw, hflip=False, vflip=True, **neutral).draw(40, hw)
        assert {tuple(m) for m in mats.tolist()} == {(1, 0, 0, 0, 1, 0), (1, 0, 0, 0, -1, hw[0] - 1)}
    # a set with a margin: the identity is the centred crop
    mats, _ = Augmenter((32, 32), hflip=False, **neutral).draw(2, (40, 41))
    assert np.array_equal(mats[0], np.array([1, 0, 4.5, 0, 1, 4], dtype=np.float32))


@pytest.mark.parametrize("kw,out_hw,src_hw", [(dict(), (32, 32), (32, 32)), (dict(), (32, 32), (40, 40)), (dict(vflip=True, scale_axis_equally=False,
                                              shear_deg=5, rotation_deg=(-20, 30)), (5, 7), (9, 8)), (dict(scale_to_percent=0.7, translation_x_px=(0, 3)), (64, 64), (64, 64))])
def test_the_matrices_equal_a_float64_restatement_rounded_to_fp32(kw, out_hw, src_hw):
    from face_generator_amd.runtime import Augmenter
    a, b = Augmenter(out_hw, seed=9, **kw), Augmenter(out_hw, seed=9, **kw)
    mats, gains = a.draw(50, src_hw)
    picks = [b.draw_one() for _ in range(50)]
    want = np.stack([augmenter_restated(p, out_hw, src_hw).reshape(6) for p in picks])
    assert np.array_equal(mats, want.astype(np.float32))
    assert np.array_equal(gains, np.array([p[8] for p in picks]).astype(np.float32))
    lo, hi = a.scale
    assert all(lo <= p[2] <= hi and a.rotation[0] <= p[4] <= a.rotation[1] and a.tx[0] <= p[6] <= a.tx[1] for p in picks)
    if not kw:
        assert (lo, hi) == (0.82, 1.10) and a.rotation == (-8, 8) and a.shear == (0, 0) and {p[1] for p in picks} == {False}
        assert {p[0] for p in picks} == {False, True} and all(p[2] == p[3] for p in picks)
    # the forward map of a pick sends the centre to the centre plus the translation: invert the restated matrix at that point
    p = picks[0]
    m = augmenter_restated((False, False) + p[2:], out_hw, out_hw)
    cx, cy = int(out_hw[1] / 2), int(out_hw[0] / 2)
    back = m @ np.array([cx + p[6], cy + p[7], 1.0])
    assert np.allclose(back, [cx, cy], atol=1e-9)


def test_the_augmenter_rides_on_the_dataset_and_leaves_the_loops_rng_alone(plan_ctx):
    from face_generator_amd.runtime import Augmenter, DeviceDataset, FgError
    from face_generator_amd.state import S
    S.reset()
    S.rng = random.Random(11)
    before = S.rng.getstate()
    py_state, np_state, torch_state = random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state()
    x = np.random.default_rng(2).uniform(0, 1, (5, 3, 12, 12)).astype(np.float32)
    ds = DeviceDataset(plan_ctx, x, augment=Augmenter((8, 8), seed=3))
    assert ds.gather([0, 4, 4]).shape == (3, 8, 8, 3) and ds.gather([1], layout="nchw").shape == (1, 3, 8, 8)
    assert ds.gather([]).shape == (0, 8, 8, 3)
    assert ds.gather([2, 3], augment=False).shape == (2, 12, 12, 3)         # the stored images, at their own size
    assert np.array_equal(ds[3].numpy(), x[3]) and np.array_equal(ds.rows(1, 3).numpy(), x[1:3])
    out = torch.zeros(2 * 3 * 8 * 8)
    assert ds.gather([1, 2], out=out).data_ptr() == out.data_ptr()
    with pytest.raises(FgError):
        ds.gather([0], out=torch.zeros(2 * 3 * 12 * 12))
    with pytest.raises(IndexError):
        ds.gather([5])
    # the third draw of the dataset's augmenter is the third draw of a fresh one: gather([]) drew nothing, gather(augment=False) neither
    twin = Augmenter((8, 8), seed=3)
    for n in (3, 1, 2):
        twin.draw(n, (12, 12))
    assert twin.rng.getstate() == ds.augment.rng.getstate()
    ds.set_augment(None)
    assert ds.gather([0]).shape == (1, 12, 12, 3)
    with pytest.raises(FgError):
        ds.set_augment("flip")
    assert S.rng.getstate() == before and random.getstate() == py_state
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


def test_resident_and_augmented_adversarial_train_draw_the_same_indices(plan_ctx):
    """the math.random picks of adversarial.train are one stream with and without augmentation"""
    import test_dataset_host as TD
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import Augmenter, DeviceDataset
    from face_generator_amd.state import S
    plain, plain_state = TD._draws_of_adversarial(plan_ctx, True, False)
    S.reset()
    adversarial.accs.clear()
    S.OPT.update(batchSize=16, noiseDim=100, N_epoch=51, saveFreq=1000, seed=11, grayscale=True, D_iterations=2)
    S.IMG_DIMENSIONS = (1, 32, 32)
    torch.manual_seed(5)
    S.MODEL_G = nn_utils.activateCuda(models.create_G((1, 32, 32), 100))
    S.MODEL_D = nn_utils.activateCuda(models.create_D((1, 32, 32)))
    S.rng = TD.RecordingRandom(11)
    images = np.random.default_rng(3).uniform(0, 1, (23, 1, 40, 40)).astype(np.float32)
    aug = Augmenter((32, 32))
    adversarial.train(DeviceDataset(plan_ctx, images, augment=aug), 1.01, 3)
    assert S.rng.log == plain and S.rng.getstate() == plain_state
    twin = Augmenter((32, 32))
    twin.draw(2 * (5 * 8 + 5), (40, 40))                                    # one transform per real image of the epoch
    assert twin.rng.getstate() == aug.rng.getstate()


def test_to_result_resident_refuses_an_augmenter(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, DeviceDataset, FgError
    fine = torch.rand(6, 3, 16, 16)
    with pytest.raises(FgError, match="augment"):
        dataset_c2f.toResultResident(fine, 8, 16, ctx=plan_ctx, augment=Augmenter((16, 16)))
    with pytest.raises(FgError, match="augment"):
        dataset_c2f.toResultResident(DeviceDataset(plan_ctx, fine, augment=Augmenter((16, 16))), 8, 16, ctx=plan_ctx)
    assert dataset_c2f.toResultResident(DeviceDataset(plan_ctx, fine), 8, 16, ctx=plan_ctx).size() == 6


# ---------------------------------------------------------------------------------------------------------------------------------
# the two references against each other
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_fp32_restatement_agrees_with_the_float64_reference():
    """200 random transforms of Augmenter in the reference's ranges (and wider ones), 5x7 to 64x64, c = 1 and 3, both fills; the fixed
    matrices; identity, mirror and integer shifts exactly"""
    from face_generator_amd.runtime import Augmenter
    rng = np.random.default_rng(17)
    worst, count = 0.0, 0
    shapes = [(1, 5, 7, 4, 6), (3, 5, 7, 5, 7), (3, 16, 16, 16, 16), (3, 40, 40, 32, 32), (1, 64, 64, 64, 64), (3, 33, 17, 20, 12)]
    for k, (c, hs, ws, ho, wo) in enumerate(shapes):
        x = rng.uniform(0, 1, (4, c, hs, ws)).astype(np.float32)
        wide = dict(rotation_deg=45, scale_to_percent=(0.5, 2.0), vflip=True, scale_axis_equally=False, shear_deg=10) if k % 2 else {}
        mats, gains = Augmenter((ho, wo), seed=k, **wide).draw(34, (hs, ws))
        idx = rng.integers(0, 4, 34)
        for fill in (0, 1):
            a = warp_ref(x, idx, mats, gains, ho, wo, fill)
            b = warp_ref64(x, idx, mats, gains, ho, wo, fill)
            worst = max(worst, float(np.abs(a - b).max()))
            count += 34
        fixed = fixed_matrices(hs, ws, ho, wo)
        idx = np.arange(len(fixed)) % 4
        for fill in (0, 1):
            a, b = warp_ref(x, idx, fixed, None, ho, wo, fill), warp_ref64(x, idx, fixed, None, ho, wo, fill)
            worst = max(worst, float(np.abs(a - b).max()))
            if (hs - ho) % 2 == 0 and (ws - wo) % 2 == 0:
                assert np.array_equal(a[:5].astype(np.float64), b[:5]), "identity, mirrors and integer shifts are exact"
    print("fp32 restatement against float64 scipy over %d random transforms: worst |difference| %.3g" % (count, worst))
    assert count >= 400 and worst <= BAR_64


def test_the_restatement_on_known_answers():
    x = np.arange(2 * 1 * 3 * 4, dtype=np.float32).reshape(2, 1, 3, 4) / 32
    ident = warp_ref(x, [1, 0, 1], None, None, 3, 4, 0)
    assert np.array_equal(ident, x[[1, 0, 1]])
    mirror = warp_ref(x, [0], np.array([[-1, 0, 3, 0, 1, 0]], dtype=np.float32), None, 3, 4, 0)
    assert np.array_equal(mirror[0], x[0][:, :, ::-1])
    half = warp_ref(x, [0], np.array([[1, 0, 0.5, 0, 1, 0]], dtype=np.float32), None, 3, 4, 0)
    assert np.array_equal(half[0, 0, :, :3], (x[0, 0, :, :3] + x[0, 0, :, 1:]) / 2) and np.array_equal(half[0, 0, :, 3], x[0, 0, :, 3] / 2)
    edge = warp_ref(x, [0], np.array([[1, 0, 0.5, 0, 1, 0]], dtype=np.float32), None, 3, 4, 1)
    assert np.array_equal(edge[0, 0, :, 3], x[0, 0, :, 3])
    shifted = warp_ref(x, [0], np.array([[1, 0, -1, 0, 1, 2]], dtype=np.float32), None, 3, 4, 0)
    assert np.array_equal(shifted[0, 0, 0, 1:], x[0, 0, 2, :3]) and not shifted[0, 0, 1:].any() and not shifted[0, 0, :, 0].any()
    bright = warp_ref(x, [1], None, np.array([2.0], dtype=np.float32), 3, 4, 0)
    assert np.array_equal(bright[0], np.minimum(x[1] * 2, 1))
    outside = warp_ref(x, [2, -1, 0], None, None, 3, 4, 0)
    assert (outside[:2].view(np.int32) == NAN_BITS).all() and np.array_equal(outside[2], x[0])
    wild = np.array([[np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [1e30, 0, 1e30, 0, 1, 0], [1, 0, 0, 0, -1e30, -np.inf]], dtype=np.float32)
    assert not warp_ref(x, [0, 1, 0, 1], wild, None, 3, 4, 0).any()
    clamped = warp_ref(x, [0, 1, 0, 1], wild, None, 3, 4, 1)
    assert np.array_equal(clamped[0, 0], np.repeat(x[0, 0, :, :1], 4, axis=1))         # a NaN column becomes column 0
    assert np.array_equal(clamped[1, 0], np.repeat(x[1, 0, :, 3:], 4, axis=1))         # +inf: the last column


# ---------------------------------------------------------------------------------------------------------------------------------
def test_lua_side_parses_and_binds_the_entry():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    fg = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    lua_parser.parse(fg)
    for probe in ("function M.warpImages(set, nSet, c, hs, ws, setLayout, idx, mats, gains, n, out, ho, wo, outLayout, fill)",
                  "function Dataset:gatherWarped(idx, n, mats, gains, out, outLayout, fill)", "C.fg_warp_images(ctx,"):
        assert probe in fg, probe
    assert "int fg_warp_images(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx, " \
           "const float* mats, const float* gains, int n, float* out, int ho, int wo, int out_layout, int fill);" in fg      # the generated cdef
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"
    # gatherWarped is a method beside gather, which is still there word for word
    assert "function Dataset:gather(picks, n, outLayout)" in fg and "function M.gatherImages(set, nSet, c, h, w, setLayout, idx, n, out, outLayout)" in fg
