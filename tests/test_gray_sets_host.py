"""CPU-only: grayscale from resident byte sets -- fg_warp_images_u8_y, fg_warp_c2f_u8_y, fg_warp_faces_u8_y (include/facegen_hip.h)
and gray=True of runtime.DeviceDataset / PhotoDataset, dataset_c2f.toResultAugmented / toResultPhotos and the ops -- in a
planning-only context (FG_DEVICE_NONE): the numpy restatement of the luma Y and the facts the device tests rest on, the declarations
and the bindings, every refusal of the fp32 siblings at c = 1 repeated with the _u8_y name and without a launch, the limits in pixels,
one launch per call with the sibling's kernel name, grid, block and LDS bytes at c = 1, the gray= rules, and the Lua side as far as
parsing goes.

A case runs through the fp32 entry with c = 1 and through the _u8_y entry, one after the other, in one child process: what the test
holds against the _u8_y call is the fp32 call's own return code, message and launch line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_augment_host import LAUNCH_RE, FG_ERR_INVALID, FG_ERR_UNSUPPORTED
from test_u8_sets_host import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fg_warp_images", "fg_warp_c2f", "fg_warp_faces")
KERNEL = dict(fg_warp_images="warp_images_kernel", fg_warp_c2f="warp_c2f_kernel", fg_warp_faces="warp_faces_kernel")
K_R, K_G, K_B = np.float32(0.299), np.float32(0.587), np.float32(0.114)


def luma(r, g, b):
    """Y of the header: ((0.299f * p(r)) + (0.587f * p(g))) + (0.114f * p(b)), every float32 operation rounded on its own"""
    pr, pg, pb = decode(r), decode(g), decode(b)
    return ((K_R * pr) + (K_G * pg)) + (K_B * pb)


def luma_set(b_nchw):
    """[N][3][H][W] bytes -> [N][1][H][W] float32 luma"""
    b_nchw = np.asarray(b_nchw)
    assert b_nchw.dtype == np.uint8 and b_nchw.ndim == 4 and b_nchw.shape[1] == 3
    y = luma(b_nchw[:, 0], b_nchw[:, 1], b_nchw[:, 2])
    assert y.dtype == np.float32
    return np.ascontiguousarray(y[:, None])


def test_the_numpy_restatement_of_the_luma():
    """the constants' bits, white and the maximum over all 256^3 triples, the once-rounded double evaluation (another float
    somewhere: random bytes tell a fused or reordered decode from the contract), and the gray triples"""
    from face_generator_amd import _lib
    from face_generator_amd.runtime import LUMA
    assert tuple(np.float32(k) for k in LUMA) == (K_R, K_G, K_B)            # what storage="f32", gray=True converts with
    hdr = open(_lib.HEADER).read()
    src = open(os.path.join(ROOT, "face_generator_amd", "csrc", "image.hip")).read()
    for k, text, bits in ((K_R, "0x1.322d0ep-2", 0x3e991687), (K_G, "0x1.2c8b44p-1", 0x3f1645a2), (K_B, "0x1.d2f1aap-4", 0x3de978d5)):
        assert text in hdr and text + "f * wi_pix(" in src, text            # the header's constants are the kernels'
        assert float(k) == float.fromhex(text), (k, text)
        assert int(np.array([k]).view(np.int32)[0]) == bits, (text, hex(int(np.array([k]).view(np.int32)[0])))
    assert luma(np.uint8(255), np.uint8(255), np.uint8(255)) == np.float32(1.0)
    assert luma(np.uint8(0), np.uint8(0), np.uint8(0)) == np.float32(0.0)
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    top, differ = np.float32(0), 0
    for r in range(256):
        rr = np.full_like(g, r)
        y = luma(rr, g, b)
        assert y.dtype == np.float32
        top = max(top, y.max())
        d = [np.float64(k) * decode(v).astype(np.float64) for k, v in ((K_R, rr), (K_G, g), (K_B, b))]      # the same floats, exact products
        once = (d[0] + d[1] + d[2]).astype(np.float32)
        differ += int((once != y).sum())
    assert top == np.float32(1.0)
    print("the once-rounded double evaluation is another float for %d of %d triples (%.1f %%)" % (differ, 256 ** 3, 100.0 * differ / 256 ** 3))
    assert differ > 0                       # (30.2 % of the triples)
    v = np.arange(256, dtype=np.uint8)
    assert int((luma(v, v, v) == decode(v)).sum()) == 191


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def test_header_binding_and_cdef_declare_the_three_entries_with_one_signature(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    hdr = open(_lib.HEADER).read()
    lua = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    want = dict(
        fg_warp_images="fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_layout, const int* idx, const float* mats, "
                       "const float* gains, int n, float* out, int ho, int wo, int fill",
        fg_warp_c2f="fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_layout, const int* idx, const float* mats, "
                    "const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int fill",
        fg_warp_faces="fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_layout, const int* idx, const float* mats, "
                      "const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff, int fill")
    for e in ENTRIES:
        y = e + "_u8_y"
        assert y in decls and hasattr(plan_ctx.lib, y), y
        names = [a for a in decls[e][2] if a not in ("c", "out_layout")]    # the sibling's arguments: three channels in, one out
        assert decls[y][2] == names, (y, decls[y][2])
        keep = [k for k, a in enumerate(decls[e][2]) if a not in ("c", "out_layout")]
        assert decls[y][0] == decls[e][0] and decls[y][1] == [decls[e][1][k] for k in keep]
        assert list(getattr(plan_ctx.lib, y).argtypes) == [getattr(plan_ctx.lib, e).argtypes[k] for k in keep]
        flat = re.sub(r"\s+", " ", hdr)
        assert "int %s(%s);" % (y, want[e]) in flat, y                      # the header, the line breaks apart
        assert "int %s(%s);" % (y, want[e]) in lua, y                       # the cdef: the same text
    doc = hdr[hdr.index("grayscale from a resident byte set"):hdr.index("int fg_warp_images_u8_y")]
    for word in ("Y(r, g, b) = ((0.299f * p(r)) + (0.587f * p(g))) + (0.114f * p(b))", "rounded on its own", "0x1.322d0ep-2", "0x1.2c8b44p-1",
                 "0x1.d2f1aap-4", "image.rgb2y", "parity\n *   unpinned by the reference", "191 of\n *      the 256", "bit for bit", "c = 1", "0x7fc00000",
                 "hs * ws <= 16384", "s * s <= 16384", "2^31 bytes", "FG_ERR_UNSUPPORTED", "one byte is enough", "Nothing outside set[0 .. 3 * n_set * hs * ws)",
                 "16-byte aligned", "P % 16 == 0", "4-byte aligned", "P % 4 == 0", "byte loads otherwise", "No load reaches over", "one launch", "no scratch"):
        assert word in doc, word
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"


# ---------------------------------------------------------------------------------------------------------------------------------
# every case through the fp32 sibling at c = 1 and through the _u8_y entry
# ---------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: None if t is None else t.data_ptr())
n = 4
SF, SB = torch.zeros(4 * 128 * 130 + 4), torch.zeros(3 * 4 * 128 * 130 + 20, dtype=torch.uint8)
I, M, G = torch.zeros(n, dtype=torch.int32), torch.zeros(6 * n), torch.ones(n)
F, C, D = (torch.zeros(n * 128 * 128 + 4) for _ in range(3))
ORDER = dict(
    fg_warp_images=["set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "out", "ho", "wo", "out_layout", "fill"],
    fg_warp_c2f=["set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "s", "cs", "fine", "coarse", "diff", "out_layout", "fill"],
    fg_warp_faces=["set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "hw", "ww", "s", "cs", "fine", "coarse", "diff",
                   "out_layout", "fill"])
GOOD = dict(
    fg_warp_images=dict(n_set=4, c=1, hs=40, ws=40, set_layout=1, idx=I, mats=M, gains=G, n=n, out=F, ho=32, wo=32, out_layout=1, fill=0),
    fg_warp_c2f=dict(n_set=4, c=1, hs=40, ws=40, set_layout=1, idx=I, mats=M, gains=G, n=n, s=32, cs=16, fine=F, coarse=C, diff=D, out_layout=1, fill=0),
    fg_warp_faces=dict(n_set=4, c=1, hs=30, ws=40, set_layout=1, idx=I, mats=M, gains=G, n=n, hw=6, ww=8, s=4, cs=2, fine=F, coarse=C, diff=D,
                       out_layout=1, fill=0))
def cases(entry):
    good = GOOD[entry]
    yield "good", {}
    for k in ("set", "idx"):
        yield "null-" + k, {k: None}
    outs = [k for k in ("out", "fine", "coarse", "diff") if k in good]
    yield "null-outputs", {k: None for k in outs}
    for k in ("n_set", "hs", "ws", "ho", "wo", "hw", "ww", "s", "cs"):
        if k in good:
            for v in (0, -1):
                if not (entry == "fg_warp_faces" and k == "cs" and v == 0):
                    yield "%%s=%%d" %% (k, v), {k: v}
    yield "n=-1", dict(n=-1)
    for k in ("set_layout", "fill"):
        for v in (-1, 2):
            yield "%%s=%%d" %% (k, v), {k: v}
    yield "n=0", dict(n=0)
    yield "no-gains", dict(gains=None)
    for sl in (0, 1):
        for off in (0, 1, 4):
            yield "lay-%%d-%%d" %% (sl, off), dict(set_layout=sl, off=off)
    if entry == "fg_warp_images":
        yield "no-mats-sizes", dict(mats=None)
        yield "no-mats", dict(mats=None, ho=40, wo=40)
        yield "above", dict(hs=4, ws=4097, ho=4, wo=4)
        yield "above-huge", dict(hs=1 << 30, ws=1 << 30)
        yield "at-limit", dict(hs=128, ws=128)
        yield "below-limit-129x127", dict(hs=129, ws=127)
        yield "above-129x128", dict(hs=129, ws=128)
        yield "above-128x129", dict(hs=128, ws=129)
        yield "above-3-channel-limit", dict(hs=100, ws=90)
        yield "out-2^31", dict(ho=1 << 16, wo=1 << 15)
    if entry == "fg_warp_c2f":
        yield "cs>s", dict(cs=33)
        yield "no-mats-sizes", dict(mats=None)
        yield "no-mats", dict(mats=None, hs=32, ws=32)
        yield "above", dict(hs=4, ws=4097)
        yield "fine-above", dict(s=129, cs=32)
        yield "at-limit", dict(hs=128, ws=128, s=128, cs=64)
        yield "below-limit-129x127", dict(hs=129, ws=127)
        yield "above-129x128", dict(hs=129, ws=128)
        yield "above-128x129", dict(hs=128, ws=129)
        yield "big-64", dict(hs=128, ws=128, s=64, cs=32)
        for name, kw in (("only-coarse", dict(fine=None, diff=None)), ("diff-coarse", dict(fine=None)), ("only-fine", dict(coarse=None, diff=None))):
            yield name, kw
    if entry == "fg_warp_faces":
        yield "cs>s", dict(cs=5)
        yield "cs0-coarse", dict(cs=0, diff=None)
        yield "cs0-diff", dict(cs=0, coarse=None)
        yield "cs0-no-fine", dict(cs=0, fine=None, coarse=None, diff=None)
        yield "cs0", dict(cs=0, coarse=None, diff=None)
        yield "no-mats-sizes", dict(mats=None)
        yield "no-mats", dict(mats=None, hw=30, ww=40)
        yield "photo-2^31", dict(hs=1 << 16, ws=1 << 15)
        yield "photo-bytes-2^31", dict(hs=1 << 15, ws=1 << 15)
        yield "photo-bytes-below", dict(hs=1 << 15, ws=21845)
        yield "window-250", dict(hs=250, ws=250, hw=250, ww=250, s=64, cs=32)
        yield "just-above", dict(hw=1, ww=35297, s=64, cs=32)
        yield "just-fits", dict(hw=1, ww=35296, s=64, cs=32)
        yield "lfw-64", dict(hs=250, ws=250, hw=84, ww=84, s=64, cs=32)
        yield "lfw-32", dict(hs=250, ws=250, hw=84, ww=84, s=32, cs=16)
        for name, kw in (("only-coarse", dict(fine=None, diff=None)), ("diff-coarse", dict(fine=None)), ("only-fine", dict(coarse=None, diff=None))):
            yield name, kw
for entry in ORDER:
    order_y = [k for k in ORDER[entry] if k not in ("c", "out_layout")]
    for tag, kw in cases(entry):
        for storage, fn, S, order in (("f32", entry, SF, ORDER[entry]), ("u8y", entry + "_u8_y", SB, order_y)):
            a = dict(GOOD[entry], set=S)
            a.update(kw)
            off = a.pop("off", 0)
            if a["set"] is not None:
                a["set"] = S[off:]
            for k in ("set", "idx", "mats", "gains", "out", "fine", "coarse", "diff"):
                if k in a:
                    a[k] = P(a[k])
            sys.stderr.write("fg-mark %%s|%%s|%%s\n" %% (entry, tag, storage)); sys.stderr.flush()
            rc = getattr(lib, fn)(ctx.h, *[a[k] for k in order])
            print("%%s|%%s|%%s\t%%d\t%%s" %% (entry, tag, storage, rc, lib.fg_last_error(ctx.h).decode() if rc else ""))
    for storage, fn, order in (("f32", entry, ORDER[entry]), ("u8y", entry + "_u8_y", order_y)):
        sys.stderr.write("fg-mark %%s|null-ctx|%%s\n" %% (entry, storage)); sys.stderr.flush()
        rc = getattr(lib, fn)(None, *[None if k in ("set", "idx", "mats", "gains", "out", "fine", "coarse", "diff") else 1 for k in order])
        print("%%s|null-ctx|%%s\t%%d\t%%s" %% (entry, storage, rc, lib.fg_last_error(None).decode()))
sys.stderr.write("fg-mark end|end|end\n")
"""


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    launches, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = tuple(l.split(" ", 1)[1].split("|"))
            launches[cur] = []
        elif cur is not None and l.startswith("fg-launch"):
            m = LAUNCH_RE.match(l)
            assert m, l
            launches[cur].append((m.group(1),) + tuple(int(v) for v in m.groups()[1:]) + (l,))
    rcs = {}
    for l in r.stdout.splitlines():
        key, rc, msg = l.split("\t")
        assert tuple(key.split("|")) not in rcs, key
        rcs[tuple(key.split("|"))] = (int(rc), msg)
    return launches, rcs


INVALID = {"null-set", "null-idx", "null-outputs", "n=-1", "cs>s", "no-mats-sizes", "cs0-coarse", "cs0-diff", "cs0-no-fine", "photo-2^31", "out-2^31",
           "null-ctx"} | {"%s=%d" % (k, v) for k in ("n_set", "hs", "ws", "ho", "wo", "hw", "ww", "s", "cs", "set_layout", "fill") for v in (0, -1, 2)}
UNSUPPORTED = {"above", "above-huge", "fine-above", "window-250", "just-above", "above-129x128", "above-128x129"}
OWN = {"photo-bytes-2^31"}                  # refused by the _u8_y entry alone: three bytes per pixel


def test_every_refusal_of_the_siblings_is_repeated_with_the_u8_y_name_and_launches_nothing(child):
    launches, rcs = child
    seen = {e: set() for e in ENTRIES}
    for (entry, tag, storage), (rc, msg) in rcs.items():
        if storage != "u8y" or tag in OWN:
            continue
        rc32, msg32 = rcs[entry, tag, "f32"]
        assert rc == rc32, (entry, tag, rc, rc32, msg)
        if tag in INVALID or tag in UNSUPPORTED:
            seen[entry].add(tag)
            assert rc == (FG_ERR_INVALID if tag in INVALID else FG_ERR_UNSUPPORTED), (entry, tag, rc, msg)
            assert entry + "_u8_y" in msg and entry + "_u8_y" not in msg32, (entry, tag, msg, msg32)
            assert msg == msg32.replace(entry, entry + "_u8_y"), (entry, tag, msg, msg32)     # the sibling's message at c = 1, the name apart
            assert launches[entry, tag, "u8y"] == [] and launches[entry, tag, "f32"] == [], (entry, tag)
        else:
            assert rc == 0, (entry, tag, rc, msg)
    common = {"null-set", "null-idx", "null-outputs", "null-ctx", "n=-1", "n_set=0", "hs=0", "ws=-1", "set_layout=2", "set_layout=-1", "fill=2", "fill=-1",
              "no-mats-sizes"}
    assert common | {"ho=0", "wo=-1", "above", "above-huge", "out-2^31", "above-129x128", "above-128x129"} <= seen["fg_warp_images"]
    assert common | {"s=0", "cs=0", "cs>s", "above", "fine-above", "above-129x128", "above-128x129"} <= seen["fg_warp_c2f"]
    assert common | {"hw=0", "ww=-1", "s=-1", "cs=-1", "cs>s", "cs0-coarse", "cs0-diff", "cs0-no-fine", "photo-2^31", "window-250", "just-above"} \
        <= seen["fg_warp_faces"]
    assert "cs = 0 takes fine alone" in rcs["fg_warp_faces", "cs0-diff", "u8y"][1]


def test_the_limits_are_counted_in_luma_floats(child):
    """hs * ws <= 16384: 128 x 128 is accepted, and so is a source above the 3-channel limit of 73 x 73; 129 x 128 and 128 x 129 are
    FG_ERR_UNSUPPORTED with the size and the limit in the message; 129 x 127 = 16383 pixels is below the limit and accepted.  The
    faces formula is fg_warp_faces' at c = 1, and a photo is 3 * hs * ws bytes below 2^31"""
    launches, rcs = child
    for entry in ("fg_warp_images", "fg_warp_c2f"):
        for tag in ("at-limit", "below-limit-129x127"):
            assert rcs[entry, tag, "u8y"][0] == 0 and len(launches[entry, tag, "u8y"]) == 1, (entry, tag, rcs[entry, tag, "u8y"])
        for tag, size, floats in (("above-129x128", "1 x 129 x 128", "16512"), ("above-128x129", "1 x 128 x 129", "16512"), ("above", "1 x 4 x 4097", "16388")):
            rc, msg = rcs[entry, tag, "u8y"]
            assert rc == FG_ERR_UNSUPPORTED and size in msg and floats in msg and "16384" in msg and entry + "_u8_y" in msg, (entry, tag, msg)
    assert rcs["fg_warp_images", "above-3-channel-limit", "u8y"][0] == 0
    assert launches["fg_warp_images", "above-3-channel-limit", "u8y"][0][5] == 4 * 100 * 90
    rc, msg = rcs["fg_warp_c2f", "fine-above", "u8y"]
    assert rc == FG_ERR_UNSUPPORTED and "1 x 129 x 129" in msg and "16384" in msg
    # the faces formula at c = 1: a window of 35296 floats fits with a face of 64 and its coarse image, 35297 does not
    rc, msg = rcs["fg_warp_faces", "just-above", "u8y"]
    assert rc == FG_ERR_UNSUPPORTED and "1 x 1 x 35297" in msg and "163840" in msg, msg
    assert rcs["fg_warp_faces", "just-fits", "u8y"][0] == 0 and launches["fg_warp_faces", "just-fits", "u8y"][0][5] <= 163840
    rc, msg = rcs["fg_warp_faces", "window-250", "u8y"]
    assert rc == FG_ERR_UNSUPPORTED and "1 x 250 x 250" in msg, msg
    # three bytes per pixel: 2^30 pixels are a photo for the one-channel sibling and 3 * 2^30 bytes for this entry
    assert rcs["fg_warp_faces", "photo-bytes-2^31", "f32"][0] == 0
    rc, msg = rcs["fg_warp_faces", "photo-bytes-2^31", "u8y"]
    assert rc == FG_ERR_INVALID and "fg_warp_faces_u8_y" in msg and "3 x 32768 x 32768" in msg and "2^31 bytes" in msg, msg
    assert launches["fg_warp_faces", "photo-bytes-2^31", "u8y"] == []
    assert rcs["fg_warp_faces", "photo-bytes-below", "u8y"][0] == 0 and 3 * (1 << 15) * 21845 < 2 ** 31 <= 3 * (1 << 15) * 21846


def test_a_call_is_one_launch_of_the_siblings_kernel_grid_block_and_lds_at_one_channel(child):
    launches, rcs = child
    ran = {e: 0 for e in ENTRIES}
    for (entry, tag, storage), (rc, msg) in rcs.items():
        if storage != "u8y" or tag in INVALID or tag in UNSUPPORTED or tag in OWN:
            continue
        got, sib = launches[entry, tag, "u8y"], launches[entry, tag, "f32"]
        if tag == "n=0":
            assert got == [] and sib == [], (entry, got, sib)
            continue
        assert len(got) == 1 and len(sib) == 1, (entry, tag, got, sib)
        assert got[0][0] == sib[0][0] == KERNEL[entry], (entry, tag, got, sib)
        assert got[0][1:6] == sib[0][1:6] and got[0][1:5] == (4, 1, 1, 256), (entry, tag, got, sib)      # grid n, block 256, the LDS at c = 1
        # the fp32 line at one channel as it always was; the luma line: an instance per set layout, the tag as the third literal argument
        assert re.match(r"^fg-launch \(%s<true, true>\) grid=4,1,1 block=256 lds=\d+$" % KERNEL[entry], sib[0][-1]), sib[0][-1]
        m = re.match(r"^fg-launch \(%s<(true|false), true, wi_y8>\) grid=4,1,1 block=256 lds=\d+$" % KERNEL[entry], got[0][-1])
        assert m, got[0][-1]
        layout = int(tag[4]) if tag.startswith("lay-") else 1
        assert m.group(1) == ("true" if layout else "false"), (tag, got[0][-1])
        ran[entry] += 1
    assert min(ran.values()) >= 6 + 6, ran
    assert launches["fg_warp_images", "at-limit", "u8y"][0][5] == 65536 and launches["fg_warp_images", "good", "u8y"][0][5] == 4 * 40 * 40
    assert launches["fg_warp_c2f", "good", "u8y"][0][5] == 4 * (40 * 40 + 32 * 32) + 28 * 48
    assert launches["fg_warp_c2f", "big-64", "u8y"][0][5] == 4 * (128 * 128 + 64 * 64) + 28 * 96 > 65536
    assert launches["fg_warp_c2f", "at-limit", "u8y"][0][5] == 2 * 65536 + 28 * 192
    assert launches["fg_warp_faces", "lfw-64", "u8y"][0][5] == 4 * (84 * 84 + 64 * 64) + 28 * (3 * 64 + 32)
    assert launches["fg_warp_faces", "just-fits", "u8y"][0][5] > 65536


def test_each_luma_instance_above_64_kb_has_its_limit_raised_behind_its_own_key():
    """the luma instances are functions of their own: each launcher raises the limit of the instance it launches, once per context,
    behind a key of that instance; the launchers stand behind the existing ones, which read as they did; no new kernel names"""
    src = open(os.path.join(ROOT, "face_generator_amd", "csrc", "image.hip")).read()

    def launcher(name):
        body = src[src.index("int %s(" % name):]
        return body[:body.index("\n}\n")]
    for name, kernel, macro in (("fg_launch_warp_c2f", "warp_c2f_kernel", "C2F"), ("fg_launch_warp_faces", "warp_faces_kernel", "FACES")):
        y = launcher(name + "_u8_y")
        assert re.search(r"static char attr_key;\s*\\\s*if \(fg_attr_first\(ctx, &attr_key\)\)\s*\\\s*FG_HIP\(ctx, hipFuncSetAttribute\(\(const void\*\)"
                         + re.escape(kernel + "<SN, ON, wi_y8>") + r",\s*hipFuncAttributeMaxDynamicSharedMemorySize", y), y
        assert y.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL((%s<SN, ON, wi_y8>)," % kernel in y, y
        # an expansion per set layout, each in a block of its own: two statics, two keys
        assert "if (set_nchw) { %s_Y(true, true); } else { %s_Y(false, true); }" % (macro, macro) in y, y
        assert "wi_y8" not in launcher(name) and "wi_y8" not in launcher(name + "_u8")
        assert src.index("int %s_u8_y(" % name) > src.index("int %s_u8(" % name) > src.index("int %s(" % name)
    y = launcher("fg_launch_warp_images_u8_y")
    assert "hipLaunchKernelGGL((warp_images_kernel<SN, ON, wi_y8>)," in y and "wi_y8" not in launcher("fg_launch_warp_images")
    for kernel in KERNEL.values():
        assert len(re.findall(r"template <bool SET_NCHW, bool OUT_NCHW, typename PIX = float>\s*__global__ __launch_bounds__\(256\) void %s\(" % kernel, src)) == 1
    assert len(re.findall(r"__global__", src)) == 5


# ---------------------------------------------------------------------------------------------------------------------------------
# gray=
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_gray_rule_of_the_ops(plan_ctx):
    from face_generator_amd import ops
    idx = torch.zeros(2, dtype=torch.int32)
    for layout, shape in (("nchw", (5, 3, 8, 8)), ("nhwc", (5, 8, 8, 3))):
        x = torch.zeros(shape, dtype=torch.uint8)
        for ol, out in (("nhwc", (2, 8, 8, 1)), ("nchw", (2, 1, 8, 8))):
            assert tuple(ops.warp_images(x, idx, set_layout=layout, out_layout=ol, gray=True, ctx=plan_ctx).shape) == out
            assert [tuple(t.shape) for t in ops.warp_c2f(x, idx, 8, 4, set_layout=layout, out_layout=ol, gray=True, ctx=plan_ctx)] == [out] * 3
        assert [tuple(t.shape) for t in ops.warp_faces(x, idx, (8, 8), 4, 2, fields=("diff", "fine"), set_layout=layout, gray=True, ctx=plan_ctx)] \
            == [(2, 4, 4, 1)] * 2
        assert tuple(ops.warp_images(x, idx, set_layout=layout, ctx=plan_ctx).shape) == (2, 8, 8, 3)      # the default: three channels out
    out = plan_ctx.empty(2, 8, 8, 1)
    assert ops.warp_images(torch.zeros(5, 3, 8, 8, dtype=torch.uint8), idx, out=out, gray=True, ctx=plan_ctx).data_ptr() == out.data_ptr()
    with pytest.raises(ValueError, match="out must be"):
        ops.warp_images(torch.zeros(5, 3, 8, 8, dtype=torch.uint8), idx, out=plan_ctx.empty(2, 8, 8, 3), gray=True, ctx=plan_ctx)
    for bad in (torch.zeros(5, 3, 8, 8), torch.zeros(5, 1, 8, 8, dtype=torch.uint8), torch.zeros(5, 4, 8, 8, dtype=torch.uint8),
                torch.zeros(5, 8, 8, 3, dtype=torch.uint8)):                # floats; one and four channels; pixel-major handed over as planes
        for call in (lambda: ops.warp_images(bad, idx, gray=True, ctx=plan_ctx), lambda: ops.warp_c2f(bad, idx, 8, 4, gray=True, ctx=plan_ctx),
                     lambda: ops.warp_faces(bad, idx, (8, 8), 4, gray=True, ctx=plan_ctx)):
            with pytest.raises(ValueError, match="gray=True takes a uint8 set of 3 channels"):
                call()


def test_the_gray_rules_of_the_classes_and_the_to_result_functions(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter, DeviceDataset, PhotoDataset, FgError, is_resident
    rng = np.random.default_rng(4)
    b = rng.integers(0, 256, (5, 3, 12, 12), dtype=np.uint8)
    y = luma_set(b)
    # the default: nothing changes
    ds = DeviceDataset(plan_ctx, b, storage="u8")
    assert ds.gray is False and (ds.c, ds.set_c) == (3, 3) and PhotoDataset(plan_ctx, b, 8, 4).gray is False
    # storage="u8": the R, G, B bytes stay, one channel is handed out
    ds = DeviceDataset(plan_ctx, b, storage="u8", gray=True)
    assert ds.gray and ds.storage == "u8" and ds.images.dtype == torch.uint8 and torch.equal(ds.images, torch.as_tensor(b))
    assert (ds.n, ds.c, ds.set_c, ds.h, ds.w) == (5, 1, 3, 12, 12) and is_resident(ds)
    assert tuple(ds.gather([0, 4, 4]).shape) == (3, 12, 12, 1) and tuple(ds.gather([1], layout="nchw").shape) == (1, 1, 12, 12)
    assert tuple(ds[3].shape) == (1, 12, 12) and ds[3].dtype == torch.float32 and tuple(ds.rows(1, 4).shape) == (3, 1, 12, 12)
    assert tuple(ds.gather([]).shape) == (0, 12, 12, 1)
    out = plan_ctx.empty(2, 12, 12, 1)
    assert ds.gather([0, 1], out=out).data_ptr() == out.data_ptr()
    with pytest.raises(FgError, match="out must be"):
        ds.gather([0, 1], out=plan_ctx.empty(2, 12, 12, 3))
    ds.set_augment(Augmenter((8, 8), seed=1))
    assert tuple(ds.gather([0, 1]).shape) == (2, 8, 8, 1) and tuple(ds.gather([0, 1], augment=False).shape) == (2, 12, 12, 1)
    with pytest.raises(FgError, match="8-bit"):
        DeviceDataset(plan_ctx, b, scale=6, storage="u8", gray=True)       # u8 with scale= stays refused
    # storage="f32": the luma, formed once, each operation rounded on its own; an ordinary one-channel set from then on
    for x in (decode(b), torch.as_tensor(decode(b))):
        ds = DeviceDataset(plan_ctx, x, gray=True)
        assert ds.gray and ds.storage == "f32" and (ds.c, ds.set_c) == (1, 3) and tuple(ds.images.shape) == (5, 1, 12, 12)
        assert torch.equal(ds.images.view(torch.int32), torch.as_tensor(y).view(torch.int32))
        ph = PhotoDataset(plan_ctx, x, 8, 4, gray=True)
        assert (ph.c, ph.set_c) == (1, 3) and torch.equal(ph.photos.view(torch.int32), torch.as_tensor(y).view(torch.int32))
    assert tuple(DeviceDataset(plan_ctx, decode(b), scale=6, gray=True).images.shape) == (5, 1, 6, 6)     # scale= runs on the luma
    big = np.random.default_rng(5).integers(0, 256, (300, 3, 4, 4), dtype=np.uint8)     # more images than one piece of the conversion
    assert torch.equal(DeviceDataset(plan_ctx, decode(big), gray=True).images.view(torch.int32), torch.as_tensor(luma_set(big)).view(torch.int32))
    # three channels in
    for bad in (b[:, :1], b[:, :2], np.concatenate([b, b[:, :1]], 1)):
        for storage in ("u8", "f32"):
            x = bad if storage == "u8" else decode(bad)
            with pytest.raises(FgError, match="DeviceDataset: gray=True.*3 channels"):
                DeviceDataset(plan_ctx, x, storage=storage, gray=True)
            with pytest.raises(FgError, match="PhotoDataset: gray=True.*3 channels"):
                PhotoDataset(plan_ctx, x, 8, 4, storage=storage, gray=True)
            with pytest.raises(FgError, match="3 channels"):
                dataset_c2f.toResultAugmented(x, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx, storage=storage, gray=True)
            with pytest.raises(FgError, match="3 channels"):
                dataset_c2f.toResultPhotos(x, (8, 8), 2, 4, None, ctx=plan_ctx, storage=storage, gray=True)
    ph = PhotoDataset(plan_ctx, b, 8, 4, augment=DeviceAugmenter((8, 8), seed=3), storage="u8", gray=True)
    assert (ph.c, ph.set_c) == (1, 3) and ph.photos.dtype == torch.uint8 and tuple(ph.photos.shape) == (5, 3, 12, 12)
    assert tuple(ph.gather([0, 1]).shape) == (2, 4, 4, 1) and tuple(ph[2].shape) == (1, 4, 4) and tuple(ph.rows(0, 5).shape) == (5, 1, 4, 4)
    assert [tuple(t.shape) for t in ph.gather_fields([1, 2], ("diff", "coarse"), coarse_scale=2, layout="nchw")] == [(2, 1, 4, 4)] * 2
    # the results
    for storage, dtype, x in (("f32", torch.float32, decode(b)), ("u8", torch.uint8, b)):
        res = dataset_c2f.toResultAugmented(x, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx, storage=storage, gray=True)
        assert res.set.gray and res.set.storage == storage and res.set.images.dtype == dtype and (res.set.c, res.set.set_c) == (1, 3)
        assert [tuple(t.shape) for t in res.gather_fields([0, 4], ("fine", "diff"))] == [(2, 8, 8, 1)] * 2
        assert [tuple(t.shape) for t in res.gather_fields([], ("fine", "diff"))] == [(0, 8, 8, 1)] * 2
        assert all(tuple(getattr(res[1], f).shape) == (1, 8, 8) for f in ("fine", "coarse", "diff"))
        res = dataset_c2f.toResultPhotos(x, (8, 8), 2, 4, Augmenter((8, 8), seed=3), ctx=plan_ctx, storage=storage, gray=True)
        assert res.set.gray and res.set.storage == storage and res.set.photos.dtype == dtype and (res.set.c, res.set.set_c) == (1, 3)
        assert [tuple(t.shape) for t in res.gather_fields([0, 4], ("coarse",), layout="nchw")] == [(2, 1, 4, 4)]
    # defaults: no gray
    assert dataset_c2f.toResultAugmented(b, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx, storage="u8").set.c == 3
    # an image above the entry's limit is stored, and refused by the library at the pull, in pixels
    big = DeviceDataset(plan_ctx, np.zeros((2, 3, 128, 129), dtype=np.uint8), storage="u8", gray=True)
    with pytest.raises(FgError, match="fg_warp_images_u8_y.*16512"):
        big.gather([0])
    assert tuple(DeviceDataset(plan_ctx, np.zeros((2, 3, 128, 128), dtype=np.uint8), storage="u8", gray=True).gather([0]).shape) == (1, 128, 128, 1)


def test_the_pulls_of_a_gray_byte_set_are_single_launches_of_the_luma_instances():
    """gather, rows and ds[i] of a gray byte DeviceDataset: the identity launch of fg_warp_images_u8_y; the results: one launch of the
    c2f / faces kernel.  A gray fp32 set launches what a one-channel set launches"""
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from face_generator_amd import dataset_c2f
from face_generator_amd.runtime import get_context, Augmenter, DeviceDataset, PhotoDataset
ctx = get_context(-1)
b = np.zeros((5, 3, 12, 12), dtype=np.uint8)
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
ds = DeviceDataset(ctx, b, storage="u8", gray=True)
mark("gather"); ds.gather([0, 1, 2])
mark("rows"); ds.rows(1, 3)
mark("item"); ds[4]
ds.set_augment(Augmenter((8, 8), seed=1))
mark("warped"); ds.gather([0, 1, 2], layout="nchw")
ph = PhotoDataset(ctx, b, 8, 4, storage="u8", gray=True)
mark("faces"); ph.gather([0, 1, 2])
mark("faces-rows"); ph.rows(0, 2)
mark("faces-item"); ph[1]
res = dataset_c2f.toResultAugmented(b, 4, 8, Augmenter((8, 8), seed=3), ctx=ctx, storage="u8", gray=True)
mark("augmented"); res.gather_fields([0, 1, 2], ("diff", "coarse"))
res = dataset_c2f.toResultPhotos(b, (8, 8), 2, 4, Augmenter((8, 8), seed=3), ctx=ctx, storage="u8", gray=True)
mark("photos"); res.gather_fields([0, 1, 2], ("diff", "coarse"))
for tag, kw, x in (("gray", dict(gray=True), b.astype(np.float32)), ("one", {}, b[:, :1].astype(np.float32))):
    mark(tag + "-make"); f32 = DeviceDataset(ctx, x, **kw)
    mark(tag + "-gather"); f32.gather([0, 1, 2])
    mark(tag + "-rows"); f32.rows(1, 3)
    f32.set_augment(Augmenter((8, 8), seed=1))
    mark(tag + "-warped"); f32.gather([0, 1, 2])
    mark(tag + "-photo-make"); ph = PhotoDataset(ctx, x, 8, 4, **kw)
    mark(tag + "-faces"); ph.gather([0, 1, 2])
    mark(tag + "-result-make"); res = dataset_c2f.toResultAugmented(x, 4, 8, Augmenter((8, 8), seed=3), ctx=ctx, **kw)
    mark(tag + "-augmented"); res.gather_fields([0, 1, 2], ("diff", "coarse"))
mark("end")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FG_LAUNCH_LOG="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, cur = {}, None
    for l in r.stderr.splitlines():
        if l.startswith("fg-mark "):
            cur = l.split()[1]
            sections[cur] = []
        elif cur is not None and l.startswith("fg-launch"):
            sections[cur].append(l)
    lds = 4 * 12 * 12
    for tag, n in (("gather", 3), ("rows", 2), ("item", 1), ("warped", 3)):
        assert sections[tag] == ["fg-launch (warp_images_kernel<true, true, wi_y8>) grid=%d,1,1 block=256 lds=%d" % (n, lds)], (tag, sections[tag])
    for tag, kernel, n in (("faces", "warp_faces_kernel", 3), ("faces-rows", "warp_faces_kernel", 2), ("faces-item", "warp_faces_kernel", 1),
                           ("augmented", "warp_c2f_kernel", 3), ("photos", "warp_faces_kernel", 3)):
        assert len(sections[tag]) == 1 and sections[tag][0].startswith("fg-launch (%s<true, true, wi_y8>) grid=%d,1,1 block=256 lds=" % (kernel, n)), \
            (tag, sections[tag])
    # an fp32 gray set: the conversion is torch's, at construction; from then on what a one-channel set launches, line for line
    for part in ("make", "gather", "rows", "warped", "photo-make", "faces", "result-make", "augmented"):
        assert sections["gray-" + part] == sections["one-" + part], (part, sections["gray-" + part], sections["one-" + part])
        assert not any("wi_y8" in l or "uint8_t" in l for l in sections["gray-" + part])
    assert len(sections["gray-gather"]) == 1 and "warp_" not in sections["gray-gather"][0] and sections["gray-rows"] == []
    assert len(sections["gray-warped"]) == 1 and "(warp_images_kernel<true, true>)" in sections["gray-warped"][0]


# ---------------------------------------------------------------------------------------------------------------------------------
def test_lua_side_parses_and_takes_the_option():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    fg = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    lua_parser.parse(fg)
    for probe in ("function M.u8y(bytes)", "function M.u8(bytes)", "local function residentPixels(images)", "return host, dev, images.gray and 'u8y' or 'u8'",
                  "C.fg_warp_images_u8_y(ctx, self.images.bytes, self.n, self.h, self.w, 1,", "C.fg_warp_c2f_u8_y(ctx, self.images.bytes, self.n, self.h, self.w, 1,",
                  "C.fg_warp_faces_u8_y(ctx, self.photos.bytes, self.n, self.photoH, self.photoW, 1,", "bytes:size(2) == 3",
                  "setmetatable({tensor = bytes, gray = true}, U8)"):
        assert probe in fg, probe
    # FG.u8y is the same tag as FG.u8, so it is accepted wherever FG.u8 is: the four constructors go through residentPixels, straight
    # or through FG.Dataset / FG.photoDataset, and hand out one channel
    for fn, via in (("function M.Dataset(images)", "residentPixels(images)"), ("function M.photoDataset(", "residentPixels(photos)"),
                    ("function M.augmentedResult(", "M.Dataset(fineImages)"), ("function M.photoResult(", "M.photoDataset(photos,")):
        body = fg[fg.index(fn):]
        assert via in body[:body.index("\nend\n")], fn
    for fn in ("function M.Dataset(images)", "function M.photoDataset("):
        body = fg[fg.index(fn):]
        body = body[:body.index("\nend\n")]
        assert "c = storage == 'u8y' and 1 or" in body and "setC = " in body, fn
    # the un-augmented pulls of a byte set, luma or not, are the identity call
    get = fg[fg.index("function Dataset:get(i)"):fg.index("function Dataset:gatherWarped(")]
    assert get.count("self.storage ~= 'f32'") == 2
