"""CPU-only: the resident sets held as 8-bit pixels -- fg_warp_images_u8, fg_warp_c2f_u8, fg_warp_faces_u8 (include/facegen_hip.h)
and storage="u8" of runtime.DeviceDataset / PhotoDataset and dataset_c2f.toResultAugmented / toResultPhotos -- in a planning-only
context (FG_DEVICE_NONE): the declarations and the bindings, every refusal of the fp32 siblings repeated with the _u8 name and without
a launch, one launch per call with the sibling's grid, block and LDS bytes (the two instances above 64 KB included), the fp32 launch
lines left as they were, the storage= rules, and the Lua side as far as parsing goes.

A case runs through the fp32 entry and through its _u8 sibling, one after the other, in one child process: what the test holds
against the _u8 call is the fp32 call's own return code, message and launch line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_augment_host import LAUNCH_RE, FG_ERR_INVALID, FG_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fg_warp_images", "fg_warp_c2f", "fg_warp_faces")
KERNEL = dict(fg_warp_images="warp_images_kernel", fg_warp_c2f="warp_c2f_kernel", fg_warp_faces="warp_faces_kernel")


def decode(b):
    """the value of a byte, as the header states it and as the host loaders compute it"""
    return np.asarray(b).astype(np.float32) / np.float32(255)


def test_the_value_of_a_byte_is_a_true_division():
    """the premise of the decode test on the device: the product with the rounded reciprocal is another float for 126 bytes"""
    b = np.arange(256)
    p = decode(b)
    assert p.dtype == np.float32 and p[0] == 0.0 and p[255] == 1.0 and np.all(np.diff(p) > 0)
    exact = np.array([np.float32(int(v) / 255.0) for v in b], dtype=np.float32)      # the double quotient rounded once more: 24 + 8 bits fit
    assert np.array_equal(p.view(np.int32), exact.view(np.int32))
    assert int((b.astype(np.float32) * (np.float32(1) / np.float32(255)) != p).sum()) == 126


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def test_header_binding_and_cdef_declare_the_three_entries(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    hdr = open(_lib.HEADER).read()
    lua = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    for e in ENTRIES:
        u = e + "_u8"
        assert u in decls and hasattr(plan_ctx.lib, u), u
        assert decls[u][2] == decls[e][2], (u, decls[u][2])                 # the sibling's argument names
        assert decls[u][0] == decls[e][0] and decls[u][1] == decls[e][1]    # ... and, a pointer being a pointer, its ctypes
        assert getattr(plan_ctx.lib, u).argtypes == getattr(plan_ctx.lib, e).argtypes
        assert re.search(r"int %s\(fg_ctx\* ctx, const uint8_t\* set, long long n_set," % u, hdr), u
        assert "int %s(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx," % u in lua, u
    doc = hdr[hdr.index("the three warps on a set held as 8-bit pixels"):hdr.index("int fg_warp_images_u8")]
    for word in ("p(b) = (float)b / 255.0f", "correctly rounded", "126 of the 256", "np.float32(b) / np.float32(255)", "bit for bit", "fp32 sibling",
                 "0x7fc00000", "names\n *   the _u8 entry", "16384", "LDS formula of fg_warp_faces", "one byte is enough", "16-byte aligned",
                 "% 16 == 0", "4-byte aligned", "% 4 == 0", "byte loads otherwise", "no load reaches over", "Nothing outside set[0 .. n_set * c * hs * ws)",
                 "no fg_gather_images for bytes", "one launch", "no scratch"):
        assert word in doc, word
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"


# ---------------------------------------------------------------------------------------------------------------------------------
# every case through both siblings
# ---------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: None if t is None else t.data_ptr())
n = 4
SF, SB = torch.zeros(4 * 64 * 64 + 4), torch.zeros(4 * 64 * 64 + 20, dtype=torch.uint8)
I, M, G = torch.zeros(n, dtype=torch.int32), torch.zeros(6 * n), torch.ones(n)
F, C, D = (torch.zeros(n * 4 * 64 * 64 + 4) for _ in range(3))
ORDER = dict(
    fg_warp_images=["set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "out", "ho", "wo", "out_layout", "fill"],
    fg_warp_c2f=["set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "s", "cs", "fine", "coarse", "diff", "out_layout", "fill"],
    fg_warp_faces=["set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "hw", "ww", "s", "cs", "fine", "coarse", "diff",
                   "out_layout", "fill"])
GOOD = dict(
    fg_warp_images=dict(n_set=7, c=3, hs=40, ws=40, set_layout=1, idx=I, mats=M, gains=G, n=n, out=F, ho=32, wo=32, out_layout=0, fill=0),
    fg_warp_c2f=dict(n_set=7, c=3, hs=40, ws=40, set_layout=1, idx=I, mats=M, gains=G, n=n, s=32, cs=16, fine=F, coarse=C, diff=D, out_layout=0, fill=0),
    fg_warp_faces=dict(n_set=7, c=3, hs=30, ws=40, set_layout=1, idx=I, mats=M, gains=G, n=n, hw=6, ww=8, s=4, cs=2, fine=F, coarse=C, diff=D,
                       out_layout=0, fill=0))
def cases(entry):
    good = GOOD[entry]
    yield "good", {}
    for k in ("set", "idx"):
        yield "null-" + k, {k: None}
    outs = [k for k in ("out", "fine", "coarse", "diff") if k in good]
    yield "null-outputs", {k: None for k in outs}
    for k in ("n_set", "c", "hs", "ws", "ho", "wo", "hw", "ww", "s", "cs"):
        if k in good:
            for v in (0, -1):
                if not (entry == "fg_warp_faces" and k == "cs" and v == 0):
                    yield "%%s=%%d" %% (k, v), {k: v}
    yield "n=-1", dict(n=-1)
    for k in ("set_layout", "out_layout", "fill"):
        for v in (-1, 2):
            yield "%%s=%%d" %% (k, v), {k: v}
    yield "n=0", dict(n=0)
    yield "no-gains", dict(gains=None)
    for sl in (0, 1):
        for ol in (0, 1):
            for off in (0, 1, 4):
                yield "lay-%%d-%%d-%%d" %% (sl, ol, off), dict(set_layout=sl, out_layout=ol, off=off)
    yield "gray", dict(c=1, set_layout=0, out_layout=1)
    if entry == "fg_warp_images":
        yield "no-mats-sizes", dict(mats=None)
        yield "no-mats", dict(mats=None, ho=40, wo=40)
        yield "above", dict(c=1, hs=4, ws=4097, ho=4, wo=4)
        yield "above-huge", dict(c=1 << 30, hs=1 << 30, ws=1 << 30)
        yield "at-limit", dict(c=4, hs=64, ws=64, ho=64, wo=64)
        yield "out-2^31", dict(ho=1 << 15, wo=1 << 15)
    if entry == "fg_warp_c2f":
        yield "cs>s", dict(cs=33)
        yield "no-mats-sizes", dict(mats=None)
        yield "no-mats", dict(mats=None, hs=32, ws=32)
        yield "above", dict(c=1, hs=4, ws=4097)
        yield "fine-above", dict(c=3, s=74, cs=32)
        yield "lfw-64", dict(c=3, hs=64, ws=64, s=64, cs=32)
        yield "at-limit", dict(c=4, hs=64, ws=64, s=64, cs=64)
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
        yield "photo-2^31", dict(c=2, hs=1 << 15, ws=1 << 15)
        yield "window-200", dict(hs=250, ws=250, hw=200, ww=200, s=64, cs=32)
        yield "just-above", dict(c=1, hw=1, ww=35297, s=64, cs=32)
        yield "sum-above", dict(hs=250, ws=250, hw=84, ww=84, s=80, cs=40)
        yield "just-fits", dict(c=1, hw=1, ww=35296, s=64, cs=32)
        yield "lfw-64", dict(hs=250, ws=250, hw=84, ww=84, s=64, cs=32)
        yield "lfw-32", dict(hs=250, ws=250, hw=84, ww=84, s=32, cs=16)
        yield "photo-big", dict(c=1, hs=1 << 15, ws=(1 << 16) - 1)
        for name, kw in (("only-coarse", dict(fine=None, diff=None)), ("diff-coarse", dict(fine=None)), ("only-fine", dict(coarse=None, diff=None))):
            yield name, kw
for entry in ORDER:
    for tag, kw in cases(entry):
        for storage, fn, S in (("f32", entry, SF), ("u8", entry + "_u8", SB)):
            a = dict(GOOD[entry], set=S)
            a.update(kw)
            off = a.pop("off", 0)
            if a["set"] is not None:
                a["set"] = S[off:]
            for k in ("set", "idx", "mats", "gains", "out", "fine", "coarse", "diff"):
                if k in a:
                    a[k] = P(a[k])
            sys.stderr.write("fg-mark %%s|%%s|%%s\n" %% (entry, tag, storage)); sys.stderr.flush()
            rc = getattr(lib, fn)(ctx.h, *[a[k] for k in ORDER[entry]])
            print("%%s|%%s|%%s\t%%d\t%%s" %% (entry, tag, storage, rc, lib.fg_last_error(ctx.h).decode() if rc else ""))
    for storage, fn in (("f32", entry), ("u8", entry + "_u8")):
        sys.stderr.write("fg-mark %%s|null-ctx|%%s\n" %% (entry, storage)); sys.stderr.flush()
        rc = getattr(lib, fn)(None, *[None if k in ("set", "idx", "mats", "gains", "out", "fine", "coarse", "diff") else 1 for k in ORDER[entry]])
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
           "null-ctx"} | {"%s=%d" % (k, v) for k in ("n_set", "c", "hs", "ws", "ho", "wo", "hw", "ww", "s", "cs", "set_layout", "out_layout", "fill")
                          for v in (0, -1, 2)}
UNSUPPORTED = {"above", "above-huge", "fine-above", "window-200", "just-above", "sum-above"}


def test_every_refusal_of_the_siblings_is_repeated_with_the_u8_name_and_launches_nothing(child):
    launches, rcs = child
    seen = {e: set() for e in ENTRIES}
    for (entry, tag, storage), (rc, msg) in rcs.items():
        if storage != "u8":
            continue
        rc32, msg32 = rcs[entry, tag, "f32"]
        assert rc == rc32, (entry, tag, rc, rc32, msg)
        if tag in INVALID or tag in UNSUPPORTED:
            seen[entry].add(tag)
            assert rc == (FG_ERR_INVALID if tag in INVALID else FG_ERR_UNSUPPORTED), (entry, tag, rc, msg)
            assert entry + "_u8" in msg and entry + "_u8" not in msg32, (entry, tag, msg, msg32)
            assert msg == msg32.replace(entry, entry + "_u8"), (entry, tag, msg, msg32)       # the sibling's message, the name apart
            assert launches[entry, tag, "u8"] == [] and launches[entry, tag, "f32"] == [], (entry, tag)
        else:
            assert rc == 0, (entry, tag, rc, msg)
    # the issue's list, per entry: NULL pointers, sizes below 1, a bad layout or fill, mats == NULL with differing sizes, the limits
    common = {"null-set", "null-idx", "null-outputs", "null-ctx", "n=-1", "n_set=0", "c=-1", "hs=0", "ws=-1", "set_layout=2", "out_layout=-1", "fill=2",
              "no-mats-sizes"}
    assert common | {"ho=0", "wo=-1", "above", "above-huge", "out-2^31"} <= seen["fg_warp_images"]
    assert common | {"s=0", "cs=0", "cs>s", "above", "fine-above"} <= seen["fg_warp_c2f"]
    assert common | {"hw=0", "ww=-1", "s=-1", "cs=-1", "cs>s", "cs0-coarse", "cs0-diff", "cs0-no-fine", "photo-2^31", "window-200", "just-above",
                     "sum-above"} <= seen["fg_warp_faces"]
    assert "16384" in rcs["fg_warp_images", "above", "u8"][1] and "16388" in rcs["fg_warp_images", "above", "u8"][1]
    assert "3 x 74 x 74" in rcs["fg_warp_c2f", "fine-above", "u8"][1] and "163840" in rcs["fg_warp_faces", "sum-above", "u8"][1]
    assert "cs = 0 takes fine alone" in rcs["fg_warp_faces", "cs0-diff", "u8"][1]


def test_a_call_is_one_launch_of_the_siblings_kernel_grid_block_and_lds(child):
    launches, rcs = child
    inst = {(1, 1): "<true, true", (1, 0): "<true, false", (0, 1): "<false, true", (0, 0): "<false, false"}
    ran = {e: 0 for e in ENTRIES}
    for (entry, tag, storage), (rc, msg) in rcs.items():
        if storage != "u8" or tag in INVALID or tag in UNSUPPORTED:
            continue
        got, sib = launches[entry, tag, "u8"], launches[entry, tag, "f32"]
        if tag == "n=0":
            assert got == [] and sib == [], (entry, got, sib)
            continue
        assert len(got) == 1 and len(sib) == 1, (entry, tag, got, sib)
        assert got[0][0] == sib[0][0] == KERNEL[entry], (entry, tag, got, sib)
        assert got[0][1:6] == sib[0][1:6] and got[0][1:5] == (4, 1, 1, 256), (entry, tag, got, sib)      # grid, block, LDS bytes
        # the instance text: the fp32 line as it always was, the u8 line with the pixel type as the third literal argument
        m = re.match(r"^fg-launch \(%s<(true|false), (true|false)>\) grid=4,1,1 block=256 lds=\d+$" % KERNEL[entry], sib[0][-1])
        assert m, sib[0][-1]
        assert got[0][-1] == sib[0][-1].replace(">)", ", uint8_t>)"), (got[0][-1], sib[0][-1])
        if tag.startswith("lay-"):
            sl, ol = int(tag[4]), int(tag[6])
            assert inst[sl, ol] + ", uint8_t>" in got[0][-1] and inst[sl, ol] + ">" in sib[0][-1], (tag, got[0][-1])
        if tag == "gray":
            assert "<true, true, uint8_t>" in got[0][-1]                    # one channel: the two layouts are one order
        ran[entry] += 1
    assert min(ran.values()) >= 12 + 3, ran
    # the sizes the LDS of a launch depends on, and the two launches above the 64 KB a kernel gets without an attribute change
    assert launches["fg_warp_images", "at-limit", "u8"][0][5] == 65536 and launches["fg_warp_images", "good", "u8"][0][5] == 4 * 3 * 40 * 40
    assert launches["fg_warp_c2f", "lfw-64", "u8"][0][5] == 2 * 4 * 3 * 64 * 64 + 28 * 96 > 65536
    assert launches["fg_warp_faces", "lfw-64", "u8"][0][5] == 140096
    assert launches["fg_warp_faces", "just-fits", "u8"][0][5] <= 163840 < 65536 * 3


def test_each_u8_instance_above_64_kb_has_its_limit_raised_behind_its_own_key():
    """the byte instances are functions of their own: without a hipFuncSetAttribute of their own they would refuse to launch on the
    device, while a planning-only run is happy.  Each launcher raises the limit of the instance it launches, once per context, and
    the fp32 launchers read as they did"""
    src = open(os.path.join(ROOT, "face_generator_amd", "csrc", "image.hip")).read()

    def launcher(name):
        body = src[src.index("int %s(" % name):]
        return body[:body.index("\n}\n")]
    for name, kernel, macro in (("fg_launch_warp_c2f", "warp_c2f_kernel", "C2F"), ("fg_launch_warp_faces", "warp_faces_kernel", "FACES")):
        f32, u8 = launcher(name), launcher(name + "_u8")
        for body, inst, mac in ((f32, "<SN, ON>", macro), (u8, "<SN, ON, uint8_t>", macro + "_U8")):
            assert re.search(r"static char attr_key;\s*\\\s*if \(fg_attr_first\(ctx, &attr_key\)\)\s*\\\s*FG_HIP\(ctx, hipFuncSetAttribute\(\(const void\*\)"
                             + re.escape(kernel + inst) + r",\s*hipFuncAttributeMaxDynamicSharedMemorySize", body), body
            assert body.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL((%s%s)," % (kernel, inst) in body, body
            assert "FG_BY_LAYOUT(set_nchw, out_nchw, %s)" % mac in body, body
        assert "uint8_t" not in f32
    f32, u8 = launcher("fg_launch_warp_images"), launcher("fg_launch_warp_images_u8")
    assert "hipLaunchKernelGGL((warp_images_kernel<SN, ON>)," in f32 and "uint8_t" not in f32
    assert "hipLaunchKernelGGL((warp_images_kernel<SN, ON, uint8_t>)," in u8
    # no new kernel names: the three kernels gained a defaulted trailing pixel type
    for kernel in KERNEL.values():
        assert len(re.findall(r"template <bool SET_NCHW, bool OUT_NCHW, typename PIX = float>\s*__global__ __launch_bounds__\(256\) void %s\(" % kernel, src)) == 1
    assert len(re.findall(r"__global__", src)) == 5


# ---------------------------------------------------------------------------------------------------------------------------------
# storage=
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ops_take_a_uint8_set_and_still_refuse_every_other_dtype(plan_ctx):
    from face_generator_amd import ops
    idx = torch.zeros(2, dtype=torch.int32)
    for dtype in (torch.float32, torch.uint8):
        x = torch.zeros(3, 2, 8, 8, dtype=dtype)
        assert tuple(ops.warp_images(x, idx, ctx=plan_ctx).shape) == (2, 8, 8, 2)
        assert [tuple(t.shape) for t in ops.warp_c2f(x, idx, 8, 4, ctx=plan_ctx)] == [(2, 8, 8, 2)] * 3
        assert [tuple(t.shape) for t in ops.warp_faces(x, idx, (8, 8), 4, 2, fields=("diff", "fine"), ctx=plan_ctx)] == [(2, 4, 4, 2)] * 2
    for dtype in (torch.float64, torch.int8, torch.int32, torch.float16):
        x = torch.zeros(3, 2, 8, 8, dtype=dtype)
        for call in (lambda: ops.warp_images(x, idx, ctx=plan_ctx), lambda: ops.warp_c2f(x, idx, 8, 4, ctx=plan_ctx),
                     lambda: ops.warp_faces(x, idx, (8, 8), 4, ctx=plan_ctx)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        ops.warp_images(torch.zeros(3, 8, 8, 2, dtype=torch.uint8).permute(0, 3, 1, 2), idx, ctx=plan_ctx)      # not contiguous


def test_storage_rules_of_the_classes_and_the_to_result_functions(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter, DeviceDataset, PhotoDataset, FgError, is_resident
    rng = np.random.default_rng(4)
    b = rng.integers(0, 256, (5, 3, 12, 12), dtype=np.uint8)
    # the default: today's behaviour for every input, uint8 included -- float32 in HBM, a byte's own value
    for x in (b, torch.as_tensor(b), b.astype(np.float32), b.astype(np.float64)):
        ds = DeviceDataset(plan_ctx, x)
        assert ds.storage == "f32" and ds.images.dtype == torch.float32 and torch.equal(ds.images, torch.as_tensor(b).to(torch.float32))
        ph = PhotoDataset(plan_ctx, x, 8, 4)
        assert ph.storage == "f32" and ph.photos.dtype == torch.float32 and torch.equal(ph.photos, torch.as_tensor(b).to(torch.float32))
    assert DeviceDataset(plan_ctx, b.astype(np.float32), scale=6).images.shape == (5, 3, 6, 6)
    # storage="u8": the bytes, kept as bytes
    for x in (b, torch.as_tensor(b)):
        ds = DeviceDataset(plan_ctx, x, storage="u8")
        assert ds.storage == "u8" and ds.images.dtype == torch.uint8 and ds.images.is_contiguous() and torch.equal(ds.images, torch.as_tensor(b))
        assert (ds.n, ds.c, ds.h, ds.w) == (5, 3, 12, 12) and ds.size() == len(ds) == 5 and is_resident(ds)
        assert ds.images.numel() * ds.images.element_size() * 4 == DeviceDataset(plan_ctx, x).images.numel() * 4
        ph = PhotoDataset(plan_ctx, x, 8, 4, storage="u8")
        assert ph.storage == "u8" and ph.photos.dtype == torch.uint8 and torch.equal(ph.photos, torch.as_tensor(b)) and is_resident(ph)
    for bad in (b.astype(np.float32), torch.as_tensor(b).to(torch.float64), b.astype(np.int8), b.astype(np.int32)):
        with pytest.raises(FgError, match="uint8"):
            DeviceDataset(plan_ctx, bad, storage="u8")
        with pytest.raises(FgError, match="uint8"):
            PhotoDataset(plan_ctx, bad, 8, 4, storage="u8")
    with pytest.raises(FgError, match="8-bit"):
        DeviceDataset(plan_ctx, b, scale=6, storage="u8")
    with pytest.raises(FgError, match="8-bit"):
        DeviceDataset(plan_ctx, b, scale=12, storage="u8")                  # even the size the images have
    for cls, make in (("DeviceDataset", lambda s: DeviceDataset(plan_ctx, b, storage=s)), ("PhotoDataset", lambda s: PhotoDataset(plan_ctx, b, 8, 4, storage=s))):
        for s in ("u16", None, "float32"):
            with pytest.raises(FgError, match=cls):
                make(s)
    with pytest.raises(FgError):
        DeviceDataset(plan_ctx, b[0], storage="u8")
    # the protocol on a byte set: shapes and dtypes of what is handed out (planning-only: no values)
    ds = DeviceDataset(plan_ctx, b, storage="u8")
    assert tuple(ds.gather([0, 4, 4]).shape) == (3, 12, 12, 3) and ds.gather([1], layout="nchw").dtype == torch.float32
    assert tuple(ds[3].shape) == (3, 12, 12) and ds[3].dtype == torch.float32
    assert tuple(ds.rows(1, 4).shape) == (3, 3, 12, 12) and ds.rows(1, 4).dtype == torch.float32
    assert tuple(ds.gather([]).shape) == (0, 12, 12, 3)
    out = plan_ctx.empty(2, 12, 12, 3)
    assert ds.gather([0, 1], out=out).data_ptr() == out.data_ptr()
    with pytest.raises(IndexError):
        ds.gather([5])
    with pytest.raises(IndexError):
        ds[5]
    ds.set_augment(Augmenter((8, 8), seed=1))
    assert tuple(ds.gather([0, 1]).shape) == (2, 8, 8, 3) and tuple(ds.gather([0, 1], augment=False).shape) == (2, 12, 12, 3)
    # an image above the entry's limit: stored, and refused by the library at the un-augmented pull, with its message
    big = DeviceDataset(plan_ctx, np.zeros((2, 1, 4, 4097), dtype=np.uint8), storage="u8")
    with pytest.raises(FgError, match="fg_warp_images_u8.*16388"):
        big.gather([0])
    ph = PhotoDataset(plan_ctx, b, 8, 4, augment=DeviceAugmenter((8, 8), seed=3), storage="u8")
    assert tuple(ph.gather([0, 1]).shape) == (2, 4, 4, 3) and tuple(ph[2].shape) == (3, 4, 4) and tuple(ph.rows(0, 5).shape) == (5, 3, 4, 4)
    assert [tuple(t.shape) for t in ph.gather_fields([1, 2], ("diff", "coarse"), coarse_scale=2, layout="nchw")] == [(2, 3, 4, 4)] * 2
    # the results
    for storage, dtype in (("f32", torch.float32), ("u8", torch.uint8)):
        kw = {} if storage == "f32" else dict(storage=storage)
        res = dataset_c2f.toResultAugmented(b, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx, **kw)
        assert isinstance(res, dataset_c2f.AugmentedResult) and res.set.storage == storage and res.set.images.dtype == dtype
        assert [tuple(t.shape) for t in res.gather_fields([0, 4], ("fine", "diff"))] == [(2, 8, 8, 3)] * 2
        assert all(tuple(getattr(res[1], f).shape) == (3, 8, 8) for f in ("fine", "coarse", "diff"))
        res = dataset_c2f.toResultPhotos(b, (8, 8), 2, 4, Augmenter((8, 8), seed=3), ctx=plan_ctx, **kw)
        assert isinstance(res, dataset_c2f.PhotoResult) and res.set.storage == storage and res.set.photos.dtype == dtype
        assert [tuple(t.shape) for t in res.gather_fields([0, 4], ("coarse",), layout="nchw")] == [(2, 3, 4, 4)]
    with pytest.raises(FgError, match="uint8"):
        dataset_c2f.toResultAugmented(b.astype(np.float32), 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx, storage="u8")
    with pytest.raises(FgError, match="uint8"):
        dataset_c2f.toResultPhotos(b.astype(np.float32), (8, 8), 2, 4, None, ctx=plan_ctx, storage="u8")
    # a set handed over as an object keeps its own storage
    ds8 = DeviceDataset(plan_ctx, b, storage="u8")
    assert dataset_c2f.toResultAugmented(ds8, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx).set is ds8
    # toResultResident stores computed coarse and diff fields: fp32 only
    with pytest.raises(FgError, match="bytes"):
        dataset_c2f.toResultResident(ds8, 4, 12, ctx=plan_ctx)
    assert dataset_c2f.toResultResident(DeviceDataset(plan_ctx, b.astype(np.float32)), 4, 12, ctx=plan_ctx).fine.storage == "f32"


def test_the_pulls_of_a_byte_set_are_single_launches_of_the_u8_instances():
    """gather, rows and ds[i] of a byte DeviceDataset: the identity launch of fg_warp_images_u8, no gather kernel; the results: one
    launch of the c2f / faces kernel"""
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from face_generator_amd import dataset_c2f
from face_generator_amd.runtime import get_context, Augmenter, DeviceDataset, PhotoDataset
ctx = get_context(-1)
b = np.zeros((5, 3, 12, 12), dtype=np.uint8)
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
ds = DeviceDataset(ctx, b, storage="u8")
mark("gather"); ds.gather([0, 1, 2])
mark("rows"); ds.rows(1, 3)
mark("item"); ds[4]
ds.set_augment(Augmenter((8, 8), seed=1))
mark("warped"); ds.gather([0, 1, 2], layout="nchw")
ph = PhotoDataset(ctx, b, 8, 4, storage="u8")
mark("faces"); ph.gather([0, 1, 2])
mark("faces-rows"); ph.rows(0, 2)
res = dataset_c2f.toResultAugmented(b, 4, 8, Augmenter((8, 8), seed=3), ctx=ctx, storage="u8")
mark("augmented"); res.gather_fields([0, 1, 2], ("diff", "coarse"))
res = dataset_c2f.toResultPhotos(b, (8, 8), 2, 4, Augmenter((8, 8), seed=3), ctx=ctx, storage="u8")
mark("photos"); res.gather_fields([0, 1, 2], ("diff", "coarse"))
f32 = DeviceDataset(ctx, b)
mark("f32-gather"); f32.gather([0, 1, 2])
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
    lds = 4 * 3 * 12 * 12
    assert sections["gather"] == ["fg-launch (warp_images_kernel<true, false, uint8_t>) grid=3,1,1 block=256 lds=%d" % lds]
    assert sections["rows"] == ["fg-launch (warp_images_kernel<true, true, uint8_t>) grid=2,1,1 block=256 lds=%d" % lds]
    assert sections["item"] == ["fg-launch (warp_images_kernel<true, true, uint8_t>) grid=1,1,1 block=256 lds=%d" % lds]
    assert sections["warped"] == ["fg-launch (warp_images_kernel<true, true, uint8_t>) grid=3,1,1 block=256 lds=%d" % lds]
    for tag, kernel, n in (("faces", "warp_faces_kernel<true, false, uint8_t>", 3), ("faces-rows", "warp_faces_kernel<true, true, uint8_t>", 2),
                           ("augmented", "warp_c2f_kernel<true, false, uint8_t>", 3), ("photos", "warp_faces_kernel<true, false, uint8_t>", 3)):
        assert len(sections[tag]) == 1 and sections[tag][0].startswith("fg-launch (%s) grid=%d,1,1 block=256 lds=" % (kernel, n)), (tag, sections[tag])
    assert len(sections["f32-gather"]) == 1 and "uint8_t" not in sections["f32-gather"][0] and "warp_" not in sections["f32-gather"][0]


# ---------------------------------------------------------------------------------------------------------------------------------
def test_lua_side_parses_and_takes_the_option():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    fg = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    lua_parser.parse(fg)
    for probe in ("function M.u8(bytes)", "local function residentPixels(images)", "C.fg_warp_images_u8(ctx, self.images.bytes,",
                  "C.fg_warp_c2f_u8(ctx, self.images.bytes,", "C.fg_warp_faces_u8(ctx, self.photos.bytes,", "ffi.cast('const uint8_t*', dev.ptr)",
                  "torch.ByteTensor"):
        assert probe in fg, probe
    # the four constructors go through residentPixels, straight or through FG.Dataset / FG.photoDataset
    for fn, via in (("function M.Dataset(images)", "residentPixels(images)"), ("function M.photoDataset(", "residentPixels(photos)"),
                    ("function M.augmentedResult(", "M.Dataset(fineImages)"), ("function M.photoResult(", "M.photoDataset(photos,")):
        body = fg[fg.index(fn):]
        assert via in body[:body.index("\nend\n")], fn
