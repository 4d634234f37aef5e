"""CPU-only: fg_warp_c2f (include/facegen_hip.h) and the coarse-to-fine set augmented per batch (dataset_c2f.AugmentedResult) in a
planning-only context (FG_DEVICE_NONE): the declaration and the export, every refusal with its code and message and without a
launch, the launch list of one call per layout pair and at the LDS limit, the draws of gather_fields, S.rng left alone, the index
picks and the augmenter's state after an epoch of adversarial_c2f.train and approxParzen, the guards of the two constructors, and the
Lua side as far as parsing goes.  The kernel's values are checked on the device by tests/test_gpu_augment_c2f.py."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_augment_host import LAUNCH_RE, FG_ERR_INVALID, FG_ERR_UNSUPPORTED, CountingRandom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "set", "n_set", "c", "hs", "ws", "set_layout", "idx", "mats", "gains", "n", "s", "cs", "fine", "coarse", "diff", "out_layout", "fill"]


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def test_header_declares_and_library_exports_the_entry(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    assert "fg_warp_c2f" in decls and hasattr(plan_ctx.lib, "fg_warp_c2f")
    assert decls["fg_warp_c2f"][2] == ARGS
    hdr = open(_lib.HEADER).read()
    doc = hdr[hdr.index("the coarse-to-fine example under a fresh random transform"):hdr.index("int fg_warp_c2f")]
    for word in ("fg_warp_images", "fg_c2f_coarse_diff", "bit for bit", "image.scale(image.scale(F, cs, cs), s, s)", "0x7fc00000", "NULL", "16384",
                 "FG_ERR_UNSUPPORTED", "FG_ERR_INVALID", "16-byte", "one launch"):
        assert word in doc, word


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: None if t is None else t.data_ptr())
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
n_set, c, hs, ws, s, cs, n = 7, 3, 6, 8, 4, 2, 4
S, I = torch.zeros(4 * 64 * 64 + 4), torch.zeros(n, dtype=torch.int32)
F, C, D = (torch.zeros(n * 4 * 64 * 64 + 4) for _ in range(3))
M, G = torch.zeros(6 * n), torch.ones(n)
good = dict(set=S, n_set=n_set, c=c, hs=hs, ws=ws, set_layout=1, idx=I, mats=M, gains=G, n=n, s=s, cs=cs, fine=F, coarse=C, diff=D,
            out_layout=0, fill=0)
def call(**kw):
    a = dict(good, **kw)
    for k in ("set", "idx", "mats", "gains", "fine", "coarse", "diff"):
        a[k] = P(a[k])
    return lib.fg_warp_c2f(ctx.h, *[a[k] for k in good])
def report(tag, rc):
    print("%%s\t%%d\t%%s" %% (tag, rc, lib.fg_last_error(ctx.h).decode()))
mark("good"); report("good", call())
for k in ("set", "idx"):
    mark("null-" + k); report("null-" + k, call(**{k: None}))
mark("null-outputs"); report("null-outputs", call(fine=None, coarse=None, diff=None))
for k in ("n_set", "c", "hs", "ws", "s", "cs"):
    for v in (0, -1):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("n=-1"); report("n=-1", call(n=-1))
for k in ("set_layout", "out_layout", "fill"):
    for v in (-1, 2):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("cs>s"); report("cs>s", call(cs=s + 1))
mark("no-mats-sizes"); report("no-mats-sizes", call(mats=None))
mark("no-mats-width"); report("no-mats-width", call(mats=None, hs=s))
mark("src-16385"); report("src-16385", call(c=1, hs=5, ws=3277))
mark("src-big"); report("src-big", call(c=3, hs=128, ws=128))
mark("src-huge"); report("src-huge", call(c=1 << 30, hs=1 << 30, ws=1 << 30))
mark("fine-16428"); report("fine-16428", call(c=3, s=74))
mark("fine-huge"); report("fine-huge", call(c=1, hs=4, ws=4, s=1 << 30, cs=1 << 30))
mark("null-ctx"); print("null-ctx\t%%d\t%%s" %% (lib.fg_warp_c2f(None, P(S), n_set, c, hs, ws, 1, P(I), P(M), P(G), n, s, cs, P(F), P(C), P(D), 0, 0),
                                                 lib.fg_last_error(None).decode()))
mark("n=0"); report("n=0", call(n=0))
mark("limit"); report("limit", call(c=4, hs=64, ws=64, s=64, cs=32, n_set=1, set_layout=0, out_layout=1))
mark("limit-equal"); report("limit-equal", call(c=4, hs=64, ws=64, s=64, cs=64, n_set=1))
mark("small-source"); report("small-source", call(c=4, hs=2, ws=2, s=64, cs=64, n_set=1))
mark("no-mats"); report("no-mats", call(mats=None, hs=s, ws=s))
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
    invalid = ["null-set", "null-idx", "null-outputs", "n=-1", "cs>s", "no-mats-sizes", "no-mats-width", "null-ctx"]
    invalid += ["%s=%d" % (k, v) for k in ("n_set", "c", "hs", "ws", "s", "cs") for v in (0, -1)]
    invalid += ["%s=%d" % (k, v) for k in ("set_layout", "out_layout", "fill") for v in (-1, 2)]
    for tag in invalid:
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_INVALID, (tag, rc)
        assert "fg_warp_c2f" in msg, (tag, msg)
        assert sections[tag] == [], (tag, sections[tag])
    for tag, size in (("src-16385", "16385"), ("src-big", "49152"), ("src-huge", ""), ("fine-16428", "16428"), ("fine-huge", "")):
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_UNSUPPORTED and "fg_warp_c2f" in msg and size in msg and "16384" in msg, (tag, rc, msg)
        assert sections[tag] == [], (tag, sections[tag])


def test_an_empty_batch_launches_nothing_and_a_call_is_one_launch_of_the_c2f_kernel(child):
    sections, rcs = child
    assert rcs["n=0"][0][0] == 0 and sections["n=0"] == []
    assert all(rc == 0 for rc, _ in rcs["lay"]) and len(rcs["lay"]) == 16
    for tag in ("good", "no-mats", "no-gains", "limit", "limit-equal", "small-source", "gray", "only-coarse", "diff-coarse", "only-fine"):
        assert rcs[tag][0][0] == 0 and len(sections[tag]) == 1 and sections[tag][0][0] == "warp_c2f_kernel", (tag, rcs[tag], sections[tag])
        assert sections[tag][0][1:5] == (4, 1, 1, 256), sections[tag]       # one block of 256 threads per image: the exact count
    inst = {(1, 1): "<true, true>", (1, 0): "<true, false>", (0, 1): "<false, true>", (0, 0): "<false, false>"}
    for (sl, ol), text in inst.items():
        for off in (0, 1):
            for fill in (0, 1):
                (name, gx, gy, gz, block, lds, line), = sections["lay-%d-%d-%d-%d" % (sl, ol, off, fill)]
                assert name == "warp_c2f_kernel" and text in line, line
                assert (gx, gy, gz, block) == (4, 1, 1, 256), line
                assert lds == (3 * 6 * 8 + 3 * 4 * 4) * 4 + (4 + 2) * 28 + 8, line      # source image, fine image, s + cs plans, to 16 bytes
    assert "<false, true>" in sections["limit"][0][-1]
    assert "<true, true>" in sections["gray"][0][-1]                        # one channel: the two layouts are one order
    # both images at the limit: 128 KB and the plans, within the 160 KB of a compute unit; cs == s and a source smaller than the
    # small image too
    for tag, plans in (("limit", 64 + 32), ("limit-equal", 64 + 64), ("small-source", 64 + 64)):
        assert sections[tag][0][5] == 2 * 65536 + plans * 28, sections[tag]
    assert max(s[0][5] for s in sections.values() if s) <= 163840
    # above the 64 KB a launch gets by default the limit of each instance is raised, once per context
    src = open(os.path.join(ROOT, "face_generator_amd", "csrc", "image.hip")).read()
    launcher = src[src.index("int fg_launch_warp_c2f("):]
    launcher = launcher[:launcher.index("\n}\n")]
    assert re.search(r"fg_attr_first\(ctx, &attr_key\)\)\s*\\?\s*FG_HIP\(ctx, hipFuncSetAttribute\(\(const void\*\)warp_c2f_kernel<SN, ON>, "
                     r"hipFuncAttributeMaxDynamicSharedMemorySize", launcher), launcher
    # one launch site, expanded once per pair of layouts
    assert launcher.count("hipLaunchKernelGGL(") == 1 and "FG_BY_LAYOUT(set_nchw, out_nchw, C2F)" in launcher
    by_layout = src[src.index("#define FG_BY_LAYOUT("):]
    by_layout = by_layout[:by_layout.index("\n//")]
    assert all("LAUNCH(%s, %s);" % p in by_layout for p in (("true", "true"), ("true", "false"), ("false", "true"), ("false", "false"))), by_layout


# ---------------------------------------------------------------------------------------------------------------------------------
# AugmentedResult
# ---------------------------------------------------------------------------------------------------------------------------------
def test_gather_fields_draws_once_per_call_and_leaves_the_loops_rng_alone(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, FgError
    from face_generator_amd.state import S
    S.reset()
    S.rng = random.Random(11)
    before = S.rng.getstate()
    py_state, np_state, torch_state = random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state()
    x = np.random.default_rng(2).uniform(0, 1, (5, 3, 12, 12)).astype(np.float32)
    res = dataset_c2f.toResultAugmented(x, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx)
    assert isinstance(res, dataset_c2f.AugmentedResult) and res.size() == len(res) == 5
    assert res.set.augment is None and tuple(res.set.images.shape) == (5, 3, 12, 12)       # the un-augmented set, stored once
    res.augment.rng = CountingRandom(3)
    per_image = 7                           # flip, zoom, rotation, shear, tx, ty, brightness
    for k, (picks, fields) in enumerate([([0, 4, 4], ("diff", "coarse")), ([1], ("fine",)), ([2, 3, 0, 1], ("fine", "coarse", "diff")), ([3, 3], ("coarse",))]):
        res.augment.rng.calls.clear()
        got = res.gather_fields(picks, fields)
        assert len(res.augment.rng.calls) == per_image * len(picks), (picks, fields)
        assert len(got) == len(fields) and all(tuple(g.shape) == (len(picks), 8, 8, 3) for g in got)
        assert len({g.data_ptr() for g in got}) == len(fields)
    assert tuple(res.gather_fields([1, 2], ("diff",), layout="nchw")[0].shape) == (2, 3, 8, 8)
    assert tuple(res.gather([1, 2, 2], "coarse").shape) == (3, 8, 8, 3)
    res.augment.rng.calls.clear()
    empty = res.gather_fields([], ("diff", "coarse"))
    assert [tuple(t.shape) for t in empty] == [(0, 8, 8, 3)] * 2 and res.augment.rng.calls == []
    ex = res[3]
    assert len(res.augment.rng.calls) == per_image and all(tuple(getattr(ex, f).shape) == (3, 8, 8) for f in ("coarse", "fine", "diff"))
    for bad in ((), ("fine", "fine"), ("sharp",)):
        with pytest.raises(FgError):
            res.gather_fields([0], bad)
    with pytest.raises(IndexError):
        res.gather_fields([5], ("fine",))
    with pytest.raises(IndexError):
        res[5]
    # the draws of four calls are the draws of a twin: 3 + 1 + 4 + 2 transforms, whatever the number of fields
    res2 = dataset_c2f.toResultAugmented(x, 4, 8, Augmenter((8, 8), seed=3), ctx=plan_ctx)
    twin = Augmenter((8, 8), seed=3)
    for picks, fields in (([0, 4, 4], ("diff", "coarse")), ([1], ("fine",)), ([2, 3, 0, 1], ("fine", "coarse", "diff")), ([3, 3], ("coarse",))):
        res2.gather_fields(picks, fields)
        twin.draw(len(picks), (12, 12))
    assert twin.rng.getstate() == res2.augment.rng.getstate()
    from face_generator_amd.runtime import is_resident
    assert is_resident(res)
    assert S.rng.getstate() == before and random.getstate() == py_state
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


def test_the_constructors_guard_the_augmenter_and_to_result_resident_still_refuses(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter, DeviceDataset, FgError
    fine = torch.rand(6, 3, 20, 20)
    with pytest.raises(FgError, match="16"):
        dataset_c2f.toResultAugmented(fine, 8, 16, Augmenter((20, 20)), ctx=plan_ctx)           # out_hw is not the fine scale
    with pytest.raises(FgError):
        dataset_c2f.toResultAugmented(fine, 8, 16, Augmenter((16, 12)), ctx=plan_ctx)
    with pytest.raises(FgError):
        dataset_c2f.toResultAugmented(fine, 8, 16, None, ctx=plan_ctx)
    with pytest.raises(FgError):
        dataset_c2f.toResultAugmented(fine, 17, 16, Augmenter((16, 16)), ctx=plan_ctx)
    with pytest.raises(FgError):
        dataset_c2f.toResultAugmented(DeviceDataset(plan_ctx, fine, augment=Augmenter((16, 16))), 8, 16, Augmenter((16, 16)), ctx=plan_ctx)
    with pytest.raises(ValueError):
        dataset_c2f.toResultAugmented(fine[:, :, :12], 8, 16, Augmenter((16, 16)), ctx=plan_ctx)
    assert dataset_c2f.toResultAugmented(DeviceDataset(plan_ctx, fine), 8, 16, Augmenter((16, 16)), ctx=plan_ctx).size() == 6
    with pytest.raises(FgError, match="augment"):
        dataset_c2f.toResultResident(fine[:, :, 2:-2, 2:-2], 8, 16, ctx=plan_ctx, augment=Augmenter((16, 16)))
    with pytest.raises(FgError, match="toResultAugmented"):
        dataset_c2f.toResultResident(DeviceDataset(plan_ctx, fine[:, :, 2:-2, 2:-2], augment=Augmenter((16, 16))), 8, 16, ctx=plan_ctx)


def _draws_of_c2f(plan_ctx, make_data):
    """tests/test_dataset_host.py _draws_of_c2f with the dataset left to the caller and N_epoch = 20 (batches of 8, 8, 8, 8 and 4)"""
    import test_dataset_host as TD
    from face_generator_amd import models_c2f, adversarial_c2f
    from face_generator_amd.state import S
    Sz, B = 16, 8
    S.reset()
    S.OPT.update(batchSize=B, N_epoch=20, D_iterations=2, G_iterations=1, saveFreq=1000, seed=3, coarseSize=Sz // 2, fineSize=Sz)
    S.IMG_DIMENSIONS = (3, Sz, Sz)
    torch.manual_seed(5)
    S.MODEL_G = models_c2f.create_G((3, Sz, Sz), cuda=True, max_batch=B)
    S.MODEL_D = models_c2f.create_D((3, Sz, Sz), cuda=True, max_batch=B)
    S._trainer = adversarial_c2f.TrainerC2F(plan_ctx, S.MODEL_G, S.MODEL_D, S.OPT)
    S.rng = TD.RecordingRandom(3)
    data = make_data()
    adversarial_c2f.train(data)
    n_train = len(S.rng.log)
    adversarial_c2f.best_dist = -1.0            # no checkpoint from the planning run
    adversarial_c2f.approxParzen(data, 3, 4)
    return list(S.rng.log), n_train, S.rng.getstate()


def test_augmented_and_resident_c2f_train_and_parzen_draw_the_same_indices(plan_ctx):
    """the math.random picks are one stream with and without augmentation; the augmenter ends where a twin ends that drew, per
    iteration, D_iterations x (half + half) transforms for the real pairs and the fake conds and B for G's conds, then one per
    approxParzen sample (coarse and fine of one transform)"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    images = np.random.default_rng(4).uniform(0, 1, (11, 3, 20, 20)).astype(np.float32)
    plain, n_plain, plain_state = _draws_of_c2f(plan_ctx, lambda: dataset_c2f.toResultResident(torch.as_tensor(images[:, :, 2:-2, 2:-2]), 8, 16, ctx=plan_ctx))
    aug = Augmenter((16, 16), seed=9)
    got, n_got, got_state = _draws_of_c2f(plan_ctx, lambda: dataset_c2f.toResultAugmented(images, 8, 16, aug, ctx=plan_ctx))
    assert n_plain == n_got == 4 * (2 * (4 + 4) + 8) + (2 * (2 + 2) + 4)
    assert len(got) == n_got + 3 and got == plain and got_state == plain_state
    twin = Augmenter((16, 16), seed=9)
    for half, B in [(4, 8)] * 4 + [(2, 4)]:
        for _ in range(2):
            twin.draw(half, (20, 20))
            twin.draw(half, (20, 20))
        twin.draw(B, (20, 20))
    state_after_train = twin.rng.getstate()
    twin.draw(3, (20, 20))
    assert twin.rng.getstate() == aug.rng.getstate() != state_after_train


def test_the_loops_pull_fields_of_one_transform_in_one_call(plan_ctx):
    """the real half of a D iteration is one gather_fields(idx, ("diff", "coarse")), the conds of the fake half and of G one-field
    pulls of "coarse"; approxParzen pulls ("coarse", "fine") of its pick once per sample"""
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import Augmenter
    log = []

    class Logging(dataset_c2f.AugmentedResult):
        def gather_fields(self, indices, fields, layout="nhwc"):
            log.append((len(indices), tuple(fields)))
            return super().gather_fields(indices, fields, layout=layout)
    images = np.random.default_rng(4).uniform(0, 1, (11, 3, 16, 16)).astype(np.float32)

    def make():
        from face_generator_amd.runtime import DeviceDataset
        return Logging(DeviceDataset(plan_ctx, images), 8, 16, Augmenter((16, 16)))
    _, n, _ = _draws_of_c2f(plan_ctx, make)
    per_iter = lambda half, B: [(half, ("diff", "coarse")), (half, ("coarse",))] * 2 + [(B, ("coarse",))]
    assert log == per_iter(4, 8) * 4 + per_iter(2, 4) + [(1, ("coarse", "fine"))] * 3


# ---------------------------------------------------------------------------------------------------------------------------------
def test_lua_side_parses_and_binds_the_entry():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    fg = open(os.path.join(ROOT, "lua", "facegen_hip.lua")).read()
    lua_parser.parse(fg)
    for probe in ("function Dataset:gatherWarpedC2F(idx, n, mats, gains, s, cs, fine, coarse, diff, outLayout, fill)", "function M.augmentedResult(",
                  "C.fg_warp_c2f(ctx,", "function M.residentResult(fineImages, coarseScale)",
                  "function Dataset:gatherWarped(idx, n, mats, gains, out, outLayout, fill)"):
        assert probe in fg, probe
    assert "int fg_warp_c2f(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx, " \
           "const float* mats, const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int out_layout, int fill);" in fg
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"
