"""CPU-only: fg_warp_faces (include/facegen_hip.h) and faces augmented from photo-sized sources (runtime.PhotoDataset,
dataset_c2f.PhotoResult) in a planning-only context (FG_DEVICE_NONE): the declaration and the export, every refusal with its code and
message and without a launch, the launch list of one call per layout pair and at the LDS limit, the draws of a pull, S.rng left
alone, the guards of the constructors, and the Lua side as far as parsing goes.

The two references of the kernel live here and are imported by tests/test_gpu_photo_faces.py: faces_ref, the header's contract
restated in numpy fp32 (tests/test_augment_host.py warp_ref, then oracle.image_scale for the scale stage and dataset._toResult), which
the kernel must match bit for bit, and faces_ref64, the same pipeline in float64 (scipy's map_coordinates, then image.scale written
as an integral of the piecewise-constant source / a linear interpolation).  They are compared with each other here, on the CPU,
within the bar the GPU test uses."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import image_scale
from test_augment_host import LAUNCH_RE, FG_ERR_INVALID, FG_ERR_UNSUPPORTED, NAN_BITS, BAR_64, CountingRandom, warp_ref, warp_ref64, fixed_matrices
from test_gpu_augment import images_01

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "hw", "ww", "s", "cs", "fine", "coarse", "diff",
        "out_layout", "fill"]
FIELDS = ("fine", "coarse", "diff")
# |fp32 restatement - float64 pipeline| for finite pixels in [0, 1], photos of at most 512 pixels a side.
# Stage 1: BAR_64 is derived for coordinates below 128, whose fp32 roundings are at most 2^-18 each; below 512 they are at most 2^-16
#   each, four times as large, and everything else in that derivation (four roundings, the fraction, slope 1 per pixel and axis, a
#   gain of at most 1.1) carries over: 4 * BAR_64.
# Stages 2 and 3: each image.scale pass is a convex combination of its source pixels (non-negative weights that sum to 1, box mean or
#   linear interpolation), so it does not enlarge a difference between its sources; it adds its own: the plan's position di * scale
#   in fp32 (below 128: 2^-18, times a slope of at most 1.1 per pixel, per axis) and a handful of roundings of sums below 8 (2^-21
#   each, a 5 x 5 box and two divisions: under 40 of them), together under 2.5e-5 per image.scale.  Three of them (window -> s,
#   s -> cs, cs -> s) stay under 1e-4.  diff = fine - coarse adds the two distances.
BAR_FACES = 4 * BAR_64 + 1e-4
BAR_FACES_DIFF = 2 * BAR_FACES


def faces_ref(x, idx, mats, gains, hw, ww, s, cs, fill):
    """x: float32 photos [n_set][c][hs][ws] -> {field: float32 [n][c][s][s]}, the header's contract: warp_ref to the hw x ww window,
    image.scale to s x s, then (cs > 0) dataset._toResult; an index outside the set gives quiet-NaN images in every field"""
    window = warp_ref(x, idx, mats, gains, hw, ww, fill)
    fine = np.stack([image_scale.scale(w, s, s) for w in window]).astype(np.float32)
    out = dict(fine=fine)
    if cs:
        out["coarse"], out["diff"] = image_scale.to_result(fine, cs, s)
    for j, i in enumerate(idx):
        if not 0 <= int(i) < x.shape[0]:
            for f in out:
                out[f][j].view(np.int32)[...] = NAN_BITS
    return out


def scale64_axis(src, dst_len, axis):
    """image.scale along one axis in float64, written independently of the C loop: up-scaling interpolates at di * (src - 1) / (dst -
    1), down-scaling is the mean of the piecewise-constant source over [di * src / dst, (di + 1) * src / dst)"""
    src = np.moveaxis(np.asarray(src, np.float64), axis, -1)
    n = src.shape[-1]
    if dst_len == n:
        out = src.copy()
    elif dst_len > n:
        pos = np.arange(dst_len) * ((n - 1) / (dst_len - 1)) if n > 1 else np.zeros(dst_len)
        i0 = np.minimum(np.floor(pos).astype(int), n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        f = pos - i0
        out = src[..., i0] * (1 - f) + src[..., i1] * f
    else:
        edges = np.arange(dst_len + 1) * (n / dst_len)
        cum = np.concatenate([np.zeros(src.shape[:-1] + (1,)), np.cumsum(src, axis=-1)], axis=-1)       # integral up to pixel k

        def integral(t):
            k = np.minimum(np.floor(t).astype(int), n - 1)
            return cum[..., k] + src[..., k] * (t - k)
        out = (integral(edges[1:]) - integral(edges[:-1])) / (n / dst_len)
    return np.moveaxis(out, -1, axis)


def scale64(img, width, height):
    return scale64_axis(scale64_axis(img, width, img.ndim - 1), height, img.ndim - 2)


def faces_ref64(x, idx, mats, gains, hw, ww, s, cs, fill):
    """the pipeline in float64 (finite matrices, indices inside the set)"""
    fine = scale64(warp_ref64(x, idx, mats, gains, hw, ww, fill), s, s)
    out = dict(fine=fine)
    if cs:
        out["coarse"] = scale64(scale64(fine, cs, cs), s, s)
        out["diff"] = fine - out["coarse"]
    return out


@pytest.mark.parametrize("c,hs,ws,hw,ww,s,cs", [(3, 97, 131, 84, 84, 64, 32), (1, 40, 30, 21, 17, 8, 3), (2, 20, 20, 8, 8, 16, 8)])
def test_the_two_references_agree_within_the_bar(c, hs, ws, hw, ww, s, cs):
    rng = np.random.default_rng(3)
    x = images_01(rng, (3, c, hs, ws))
    mats = fixed_matrices(hs, ws, hw, ww)
    idx = rng.integers(0, 3, len(mats))
    gains = np.linspace(0.9, 1.1, len(mats)).astype(np.float32)
    for fill in (0, 1):
        a, b = faces_ref(x, idx, mats, gains, hw, ww, s, cs, fill), faces_ref64(x, idx, mats, gains, hw, ww, s, cs, fill)
        for f in FIELDS:
            assert a[f].dtype == np.float32 and a[f].shape == (len(mats), c, s, s)
            assert float(np.abs(a[f] - b[f]).max()) <= (BAR_FACES_DIFF if f == "diff" else BAR_FACES), (f, fill)
    # the scale stage alone, against the oracle: a box mean, an interpolation and the copy
    img = images_01(rng, (2, 21, 17))
    for w, h in ((8, 8), (30, 40), (17, 21), (5, 40)):
        assert float(np.abs(image_scale.scale(img, w, h) - scale64(img, w, h)).max()) <= 2.5e-5


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def lds_bytes(c, hw, ww, s, cs):
    """the formula of the header"""
    floats = (max(c * hw * ww, c * cs * cs) + 3) // 4 * 4 + c * s * s
    return (4 * floats + 28 * (3 * s + cs) + 15) // 16 * 16


def test_header_declares_and_library_exports_the_entry(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    assert "fg_warp_faces" in decls and hasattr(plan_ctx.lib, "fg_warp_faces")
    assert decls["fg_warp_faces"][2] == ARGS
    hdr = open(_lib.HEADER).read()
    doc = hdr[hdr.index("a face under a fresh random transform, cut from a photo of any size"):hdr.index("int fg_warp_faces")]
    for word in ("generate_dataset.py", "dataset.lua:95", "fg_warp_images", "fg_scale_bilinear", "fg_c2f_coarse_diff", "bit for bit",
                 "image.scale(W, s, s)", "image.scale(image.scale(F, cs, cs), s, s)", "0x7fc00000", "NULL", "ANY size", "FG_ERR_UNSUPPORTED",
                 "FG_ERR_INVALID", "163840", "one launch", "one block per face", "4 bytes", "2^31", "addresses nothing",
                 "4 * (roundup4(max(c*hw*ww, c*cs*cs)) + c*s*s) + 28 * (3*s + cs)"):
        assert word in doc, word
    assert lds_bytes(3, 84, 84, 64, 32) == 140096 and "140096" in doc
    # the siblings keep their limit
    assert "c * hs * ws > 16384 floats" in hdr and "c * hs * ws > 16384 or c * s * s > 16384" in hdr


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: None if t is None else t.data_ptr())
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
n_set, c, hs, ws, hw, ww, s, cs, n = 7, 3, 30, 40, 6, 8, 4, 2, 4
S, I = torch.zeros(3 * 30 * 40 + 4), torch.zeros(n, dtype=torch.int32)
F, C, D = (torch.zeros(n * 4 * 64 * 64 + 4) for _ in range(3))
M, G = torch.zeros(6 * n), torch.ones(n)
good = dict(set=S, n_set=n_set, c=c, hs=hs, ws=ws, set_layout=1, idx=I, mats=M, gains=G, n=n, hw=hw, ww=ww, s=s, cs=cs, fine=F, coarse=C,
            diff=D, out_layout=0, fill=0)
def call(**kw):
    a = dict(good, **kw)
    for k in ("set", "idx", "mats", "gains", "fine", "coarse", "diff"):
        a[k] = P(a[k])
    return lib.fg_warp_faces(ctx.h, *[a[k] for k in good])
def report(tag, rc):
    print("%%s\t%%d\t%%s" %% (tag, rc, lib.fg_last_error(ctx.h).decode()))
mark("good"); report("good", call())
for k in ("set", "idx"):
    mark("null-" + k); report("null-" + k, call(**{k: None}))
mark("null-outputs"); report("null-outputs", call(fine=None, coarse=None, diff=None))
for k in ("n_set", "c", "hs", "ws", "hw", "ww", "s"):
    for v in (0, -1):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("cs=-1"); report("cs=-1", call(cs=-1, coarse=None, diff=None))
mark("n=-1"); report("n=-1", call(n=-1))
for k in ("set_layout", "out_layout", "fill"):
    for v in (-1, 2):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("cs>s"); report("cs>s", call(cs=s + 1))
mark("cs0-coarse"); report("cs0-coarse", call(cs=0, diff=None))
mark("cs0-diff"); report("cs0-diff", call(cs=0, coarse=None))
mark("cs0-no-fine"); report("cs0-no-fine", call(cs=0, fine=None, coarse=None, diff=None))
mark("no-mats-sizes"); report("no-mats-sizes", call(mats=None))
mark("no-mats-width"); report("no-mats-width", call(mats=None, hw=hs))
mark("photo-2^31"); report("photo-2^31", call(c=2, hs=1 << 15, ws=1 << 15))
mark("photo-huge"); report("photo-huge", call(c=1 << 30, hs=1 << 30, ws=1 << 30))
mark("null-ctx"); print("null-ctx\t%%d\t%%s" %% (lib.fg_warp_faces(None, P(S), n_set, c, hs, ws, 1, P(I), P(M), P(G), n, hw, ww, s, cs, P(F), P(C), P(D), 0, 0),
                                                 lib.fg_last_error(None).decode()))
mark("window-200"); report("window-200", call(hs=250, ws=250, hw=200, ww=200, s=64, cs=32))
mark("face-128"); report("face-128", call(hw=8, ww=8, s=128, cs=2))
mark("just-above"); report("just-above", call(c=1, hw=1, ww=35297, s=64, cs=32))
mark("sum-above"); report("sum-above", call(hs=250, ws=250, hw=84, ww=84, s=80, cs=40))
mark("window-huge"); report("window-huge", call(hw=1 << 30, ww=1 << 30, s=1 << 30, cs=1 << 30))
mark("n=0"); report("n=0", call(n=0))
mark("just-fits"); report("just-fits", call(c=1, hw=1, ww=35296, s=64, cs=32))
mark("lfw-64"); report("lfw-64", call(hs=250, ws=250, hw=84, ww=84, s=64, cs=32))
mark("lfw-32"); report("lfw-32", call(hs=250, ws=250, hw=84, ww=84, s=32, cs=0, coarse=None, diff=None))
mark("photo-big"); report("photo-big", call(c=1, hs=1 << 15, ws=(1 << 16) - 1))
mark("old-limit"); report("old-limit", call(c=4, hs=64, ws=64, hw=64, ww=64, s=64, cs=32, n_set=1, set_layout=0, out_layout=1))
mark("no-mats"); report("no-mats", call(mats=None, hw=hs, ww=ws))
mark("no-gains"); report("no-gains", call(gains=None))
for name, kw in (("only-coarse", dict(fine=None, diff=None)), ("diff-coarse", dict(fine=None)), ("only-fine", dict(coarse=None, diff=None))):
    mark(name); report(name, call(**kw))
for sl in (0, 1):
    for ol in (0, 1):
        for off in (0, 1):
            for fill in (0, 1):
                mark("lay-%%d-%%d-%%d-%%d" %% (sl, ol, off, fill))
                report("lay", call(set_layout=sl, out_layout=ol, set=S[off:], fine=F[off:], coarse=C[off:], diff=D[off:], fill=fill))
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
    invalid = ["null-set", "null-idx", "null-outputs", "cs=-1", "n=-1", "cs>s", "cs0-coarse", "cs0-diff", "cs0-no-fine", "no-mats-sizes",
               "no-mats-width", "photo-2^31", "photo-huge", "null-ctx"]
    invalid += ["%s=%d" % (k, v) for k in ("n_set", "c", "hs", "ws", "hw", "ww", "s") for v in (0, -1)]
    invalid += ["%s=%d" % (k, v) for k in ("set_layout", "out_layout", "fill") for v in (-1, 2)]
    for tag in invalid:
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_INVALID, (tag, rc, msg)
        assert "fg_warp_faces" in msg, (tag, msg)
        assert sections[tag] == [], (tag, sections[tag])
    assert "2^31" in rcs["photo-2^31"][0][1]
    for tag, sizes in (("window-200", ("3 x 200 x 200", "3 x 64 x 64")), ("face-128", ("3 x 8 x 8", "3 x 128 x 128")),
                       ("just-above", ("1 x 1 x 35297", "1 x 64 x 64", "1 x 32 x 32", "224 scale plans", "%d bytes" % lds_bytes(1, 1, 35297, 64, 32))),
                       ("sum-above", ("3 x 84 x 84", "3 x 80 x 80", "3 x 40 x 40", "%d bytes" % lds_bytes(3, 84, 84, 80, 40))), ("window-huge", ())):
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_UNSUPPORTED and "fg_warp_faces" in msg and "163840" in msg and all(s in msg for s in sizes), (tag, rc, msg)
        assert sections[tag] == [], (tag, sections[tag])
    assert lds_bytes(1, 1, 35297, 64, 32) > 163840 >= lds_bytes(1, 1, 35296, 64, 32) and lds_bytes(3, 8, 8, 128, 2) > 163840


def test_an_empty_batch_launches_nothing_and_a_call_is_one_launch_of_one_block_per_face(child):
    sections, rcs = child
    assert rcs["n=0"][0][0] == 0 and sections["n=0"] == []
    assert all(rc == 0 for rc, _ in rcs["lay"]) and len(rcs["lay"]) == 16
    for tag in ("good", "no-mats", "no-gains", "just-fits", "lfw-64", "lfw-32", "photo-big", "old-limit", "gray", "only-coarse", "diff-coarse",
                "only-fine"):
        assert rcs[tag][0][0] == 0 and len(sections[tag]) == 1 and sections[tag][0][0] == "warp_faces_kernel", (tag, rcs[tag], sections[tag])
        assert sections[tag][0][1:5] == (4, 1, 1, 256), sections[tag]       # one block of 256 threads per face: the exact count
        assert sections[tag][0][5] <= 163840, sections[tag]
    inst = {(1, 1): "<true, true>", (1, 0): "<true, false>", (0, 1): "<false, true>", (0, 0): "<false, false>"}
    for (sl, ol), text in inst.items():
        for off in (0, 1):
            for fill in (0, 1):
                (name, gx, gy, gz, block, lds, line), = sections["lay-%d-%d-%d-%d" % (sl, ol, off, fill)]
                assert name == "warp_faces_kernel" and text in line, line
                assert (gx, gy, gz, block) == (4, 1, 1, 256), line
                assert lds == lds_bytes(3, 6, 8, 4, 2) == (3 * 6 * 8 + 3 * 4 * 4) * 4 + (3 * 4 + 2) * 28 + 8, line
    assert "<false, true>" in sections["old-limit"][0][-1]
    assert "<true, true>" in sections["gray"][0][-1]                           # one channel: the two layouts are one order
    assert sections["lfw-64"][0][5] == 140096 and sections["lfw-32"][0][5] == lds_bytes(3, 84, 84, 32, 0)
    assert sections["just-fits"][0][5] == lds_bytes(1, 1, 35296, 64, 32) <= 163840
    assert sections["no-mats"][0][5] == lds_bytes(3, 30, 40, 4, 2)          # the window is the photo
    # above the 64 KB a launch gets by default the limit of each instance is raised, once per context
    import re
    src = open(os.path.join(ROOT, "face_generator_amd", "csrc", "image.hip")).read()
    launcher = src[src.index("int fg_launch_warp_faces("):]
    launcher = launcher[:launcher.index("\n}\n")]
    assert re.search(r"fg_attr_first\(ctx, &attr_key\)\)\s*\\?\s*FG_HIP\(ctx, hipFuncSetAttribute\(\(const void\*\)warp_faces_kernel<SN, ON>,\s*"
                     r"hipFuncAttributeMaxDynamicSharedMemorySize", launcher), launcher
    # one launch site, expanded once per pair of layouts
    assert launcher.count("hipLaunchKernelGGL(") == 1 and "FG_BY_LAYOUT(set_nchw, out_nchw, FACES)" in launcher
    by_layout = src[src.index("#define FG_BY_LAYOUT("):]
    by_layout = by_layout[:by_layout.index("\n//")]
    assert all("LAUNCH(%s, %s);" % p in by_layout for p in (("true", "true"), ("true", "false"), ("false", "true"), ("false", "false"))), by_layout


def test_the_siblings_still_refuse_sources_above_their_limit(plan_ctx):
    lib, h = plan_ctx.lib, plan_ctx.h
    t, i = torch.zeros(3 * 74 * 74), torch.zeros(1, dtype=torch.int32)
    assert lib.fg_warp_images(h, t.data_ptr(), 1, 3, 74, 74, 1, i.data_ptr(), t.data_ptr(), None, 1, t.data_ptr(), 8, 8, 1, 0) == FG_ERR_UNSUPPORTED
    assert lib.fg_warp_c2f(h, t.data_ptr(), 1, 3, 74, 74, 1, i.data_ptr(), t.data_ptr(), None, 1, 8, 4, t.data_ptr(), None, None, 1, 0) == FG_ERR_UNSUPPORTED
    assert lib.fg_warp_faces(h, t.data_ptr(), 1, 3, 74, 74, 1, i.data_ptr(), t.data_ptr(), None, 1, 8, 8, 8, 4, t.data_ptr(), None, None, 1, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# PhotoDataset / PhotoResult
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_pull_draws_once_and_leaves_the_loops_rng_alone(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter, PhotoDataset, FgError, is_resident
    from face_generator_amd.state import S
    S.reset()
    S.rng = random.Random(11)
    before = S.rng.getstate()
    py_state, np_state, torch_state = random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state()
    x = np.random.default_rng(2).uniform(0, 1, (5, 3, 30, 34)).astype(np.float32)
    ds = PhotoDataset(plan_ctx, x, (20, 18), 8, augment=Augmenter((20, 18), seed=3))
    assert ds.size() == len(ds) == 5 and (ds.c, ds.h, ds.w) == (3, 8, 8) and tuple(ds.photos.shape) == (5, 3, 30, 34)
    assert is_resident(ds)
    ds.augment.rng = CountingRandom(3)
    per_image = 7                           # flip, zoom, rotation, shear, tx, ty, brightness
    for picks, layout, shape in (([0, 4, 4], "nhwc", (3, 8, 8, 3)), ([1], "nchw", (1, 3, 8, 8)), ([2, 3, 0, 1], "nhwc", (4, 8, 8, 3))):
        ds.augment.rng.calls.clear()
        got = ds.gather(picks, layout=layout)
        assert len(ds.augment.rng.calls) == per_image * len(picks) and tuple(got.shape) == shape
    ds.augment.rng.calls.clear()
    assert tuple(ds.gather([], layout="nhwc").shape) == (0, 8, 8, 3) and ds.augment.rng.calls == []
    assert tuple(ds.gather([1, 2], augment=False).shape) == (2, 8, 8, 3) and tuple(ds[3].shape) == (3, 8, 8) and tuple(ds.rows(1, 4).shape) == (3, 3, 8, 8)
    assert ds.augment.rng.calls == []       # the stored faces: no draw
    out = plan_ctx.empty(2, 8, 8, 3)
    assert ds.gather([0, 1], out=out).data_ptr() == out.data_ptr()
    with pytest.raises(IndexError):
        ds.gather([5])
    with pytest.raises(IndexError):
        ds[5]
    with pytest.raises(FgError):
        ds.gather([0], layout="chw")
    # the draws of a twin: against the photo size, in window geometry
    ds2 = PhotoDataset(plan_ctx, x, (20, 18), 8, augment=Augmenter((20, 18), seed=3))
    twin = Augmenter((20, 18), seed=3)
    for k in (3, 1, 4):
        ds2.gather(list(range(k)))
        twin.draw(k, (30, 34))
    assert twin.rng.getstate() == ds2.augment.rng.getstate()
    # a DeviceAugmenter: one launch of the draw per pull, 3 quads per face
    dev = PhotoDataset(plan_ctx, x, (20, 18), 8, augment=DeviceAugmenter((20, 18), seed=3))
    dev.gather([0, 1, 2])
    dev.gather([4])
    assert dev.augment.state() == (3, 12)
    # the result: fields of one draw
    res = dataset_c2f.toResultPhotos(x, (20, 18), 4, 8, Augmenter((20, 18), seed=3), ctx=plan_ctx)
    assert isinstance(res, dataset_c2f.PhotoResult) and res.size() == len(res) == 5 and is_resident(res)
    assert callable(res.gather_fields) and (res.coarseScale, res.fineScale) == (4, 8)
    res.augment.rng = CountingRandom(3)
    for picks, fields in (([0, 4, 4], ("diff", "coarse")), ([1], ("fine",)), ([2, 3, 0, 1], ("fine", "coarse", "diff"))):
        res.augment.rng.calls.clear()
        got = res.gather_fields(picks, fields)
        assert len(res.augment.rng.calls) == per_image * len(picks), (picks, fields)
        assert len(got) == len(fields) and all(tuple(g.shape) == (len(picks), 8, 8, 3) for g in got)
        assert len({g.data_ptr() for g in got}) == len(fields)
    assert tuple(res.gather([1, 2, 2], "coarse", layout="nchw").shape) == (3, 3, 8, 8)
    res.augment.rng.calls.clear()
    ex = res[3]
    assert len(res.augment.rng.calls) == per_image and all(tuple(getattr(ex, f).shape) == (3, 8, 8) for f in FIELDS)
    for bad in ((), ("fine", "fine"), ("sharp",)):
        with pytest.raises(FgError):
            res.gather_fields([0], bad)
    with pytest.raises(IndexError):
        res[5]
    assert dataset_c2f.toResultPhotos(ds, (20, 18), 4, 8, None, ctx=plan_ctx).set is ds
    assert S.rng.getstate() == before and random.getstate() == py_state
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


def test_the_constructors_guard_window_augmenter_and_scales(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, PhotoDataset, FgError
    x = torch.rand(6, 3, 30, 34)
    with pytest.raises(FgError, match="20x18"):
        PhotoDataset(plan_ctx, x, (20, 18), 8, augment=Augmenter((8, 8)))              # drawn for the face, not for the window
    with pytest.raises(FgError):
        PhotoDataset(plan_ctx, x, (20, 18), 8, augment=Augmenter((18, 20)))
    with pytest.raises(FgError):
        PhotoDataset(plan_ctx, x, (20, 18), 8, augment="flip")
    with pytest.raises(FgError):
        PhotoDataset(plan_ctx, x, (20, 18), (8, 6))
    with pytest.raises(FgError):
        PhotoDataset(plan_ctx, x, (0, 18), 8)
    with pytest.raises(FgError):
        PhotoDataset(plan_ctx, x[0], (20, 18), 8)
    ds = PhotoDataset(plan_ctx, x, 20, 8)
    assert ds.window_hw == (20, 20) and ds.augment is None
    with pytest.raises(FgError):
        ds.set_augment(Augmenter((8, 8)))
    ds.set_augment(Augmenter((20, 20)))
    for cs in (0, 9):
        with pytest.raises(FgError):
            dataset_c2f.PhotoResult(ds, cs)
    with pytest.raises(FgError):
        dataset_c2f.PhotoResult(x, 4)
    with pytest.raises(FgError):
        dataset_c2f.toResultPhotos(ds, 20, 4, 16, None, ctx=plan_ctx)                   # the set hands out 8 x 8 faces
    with pytest.raises(FgError):
        dataset_c2f.toResultPhotos(x, (20, 18), 4, 8, Augmenter((8, 8)), ctx=plan_ctx)
    # a window above what a compute unit holds is refused by the entry, with its message
    big = PhotoDataset(plan_ctx, torch.rand(2, 3, 250, 250), 200, 64)
    with pytest.raises(FgError, match="163840"):
        big.gather([0])


def test_the_identity_pull_is_the_central_window(plan_ctx):
    """(planning-only: the matrices that would be uploaded) [1, 0, (ws - ww) / 2, 0, 1, (hs - hw) / 2], no gains, one buffer of the
    largest n so far, sliced"""
    from face_generator_amd.runtime import PhotoDataset
    ds = PhotoDataset(plan_ctx, torch.rand(2, 3, 250, 250), 84, 64)
    mats, gains, fill = ds.transforms(3)
    assert gains is None and fill == "constant"
    assert mats.reshape(3, 6).tolist() == [[1.0, 0.0, 83.0, 0.0, 1.0, 83.0]] * 3
    assert ds.transforms(3)[0].data_ptr() == mats.data_ptr() == ds.transforms(2)[0].data_ptr() and ds.transforms(2)[0].numel() == 12
    assert ds.transforms(5)[0].reshape(5, 6).tolist() == [[1.0, 0.0, 83.0, 0.0, 1.0, 83.0]] * 5


# ---------------------------------------------------------------------------------------------------------------------------------
def test_lua_side_parses_and_binds_the_entry():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    fg = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    lua_parser.parse(fg)
    for probe in ("function M.photoDataset(photos, windowH, windowW, s, draw, fill)", "function M.photoResult(photos, windowH, windowW, coarseScale, fineScale, draw, fill)",
                  "C.fg_warp_faces(ctx,", "function Photos:gatherFields(picks, fields, cs, n, outLayout, augment)", "function M.Dataset(images)",
                  "function M.augmentedResult("):
        assert probe in fg, probe
    assert "int fg_warp_faces(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx, " \
           "const float* mats, const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff, " \
           "int out_layout, int fill);" in fg
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"
