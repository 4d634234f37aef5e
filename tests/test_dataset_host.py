"""CPU-only: fg_gather_images (include/facegen_hip.h) and the training set resident in HBM (runtime.DeviceDataset,
dataset_c2f.toResultResident) in a planning-only context (FG_DEVICE_NONE): the declaration and the export, every refusal with its
message and without a launch, the launch list of one gather, the dataset protocol, the index draws of the resident epoch loops beside
the host-fed ones, and the Lua side as far as parsing goes.  What the kernels move is checked on the device
(tests/test_gpu_dataset.py)."""
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
LAUNCH_RE = re.compile(r"^fg-launch \(?\s*([A-Za-z_]\w*)[^)]*\)? grid=(\d+),(\d+),(\d+) block=(\d+) lds=(\d+)$")


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def _err(ctx):
    return ctx.lib.fg_last_error(ctx.h).decode()


def test_header_declares_and_library_exports_the_entry(plan_ctx):
    from face_generator_amd import _lib
    decls = _lib.parse_header()
    assert "fg_gather_images" in decls and hasattr(plan_ctx.lib, "fg_gather_images")
    assert decls["fg_gather_images"][2] == ["ctx", "set", "n_set", "c", "h", "w", "set_layout", "idx", "n", "out", "out_layout"]
    hdr = open(_lib.HEADER).read()
    doc = hdr[hdr.index("dataset[i] for a set that lives in HBM"):hdr.index("int fg_gather_images")]
    for word in ("dataset.lua:66-69", "dataset_c2f.lua:65-106", "quiet NaN", "2^31", "FG_ERR_INVALID", "16-byte"):
        assert word in doc, word


# one child process with FG_LAUNCH_LOG: sections of stderr between marks; the return codes and messages come back on stdout
CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
lib, P = ctx.lib, (lambda t: None if t is None else t.data_ptr())
def mark(s):
    sys.stderr.write("fg-mark %%s\n" %% s); sys.stderr.flush()
n_set, c, h, w, n = 7, 3, 4, 6, 4
S, O, I = torch.zeros(n_set * c * h * w + 4), torch.zeros(n * c * h * w + 4), torch.zeros(n, dtype=torch.int32)
good = dict(set=S, n_set=n_set, c=c, h=h, w=w, set_layout=1, idx=I, n=n, out=O, out_layout=0)
def call(**kw):
    a = dict(good, **kw)
    for k in ("set", "idx", "out"):
        a[k] = P(a[k])
    return lib.fg_gather_images(ctx.h, *[a[k] for k in good])
def report(tag, rc):
    print("%%s\t%%d\t%%s" %% (tag, rc, lib.fg_last_error(ctx.h).decode()))
mark("good"); report("good", call())
for k in ("set", "idx", "out"):
    mark("null-" + k); report("null-" + k, call(**{k: None}))
for k in ("n_set", "c", "h", "w"):
    for v in (0, -1):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("n=-1"); report("n=-1", call(n=-1))
for k in ("set_layout", "out_layout"):
    for v in (-1, 2):
        mark("%%s=%%d" %% (k, v)); report("%%s=%%d" %% (k, v), call(**{k: v}))
mark("image-2^31"); report("image-2^31", call(c=1 << 11, h=1 << 10, w=1 << 10))
mark("null-ctx"); print("null-ctx\t%%d\t" %% lib.fg_gather_images(None, P(S), n_set, c, h, w, 1, P(I), n, P(O), 0))
mark("n=0"); report("n=0", call(n=0))
for sl in (0, 1):
    for ol in (0, 1):
        for off in (0, 1):
            mark("lay-%%d-%%d-%%d" %% (sl, ol, off)); report("lay", call(set_layout=sl, out_layout=ol, set=S[off:], out=O[off:]))
mark("gray"); report("gray", call(c=1, set_layout=1, out_layout=0))
mark("onepixel"); report("onepixel", call(h=1, w=1, set_layout=0, out_layout=1))
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


def test_every_invalid_argument_is_refused_with_a_message_and_without_a_launch(child):
    sections, rcs = child
    assert rcs["good"] == [(0, rcs["good"][0][1])]
    bad = ["null-set", "null-idx", "null-out", "n_set=0", "n_set=-1", "c=0", "c=-1", "h=0", "h=-1", "w=0", "w=-1", "n=-1",
           "set_layout=-1", "set_layout=2", "out_layout=-1", "out_layout=2", "image-2^31"]
    for tag in bad:
        (rc, msg), = rcs[tag]
        assert rc == FG_ERR_INVALID, (tag, rc)
        assert "fg_gather_images" in msg, (tag, msg)
        assert sections[tag] == [], (tag, sections[tag])
    assert rcs["null-ctx"][0][0] == FG_ERR_INVALID and sections["null-ctx"] == []


def test_an_empty_gather_launches_nothing_and_a_gather_is_one_launch(child):
    sections, rcs = child
    assert rcs["n=0"][0][0] == 0 and sections["n=0"] == []
    assert len(sections["good"]) == 1
    assert all(rc == 0 for rc, _ in rcs["lay"])
    want = {(1, 0): "nchw_to_nhwc_kernel", (0, 1): "nhwc_to_nchw_kernel", (0, 0): "copy_kernel", (1, 1): "copy_kernel"}
    for (sl, ol), kernel in want.items():
        for off in (0, 1):
            (name, gx, gy, gz, block, lds, line), = sections["lay-%d-%d-%d" % (sl, ol, off)]
            assert name == kernel and block == 256 and gy == gz == 1, line
            assert lds == (0 if sl == ol else 3 * (256 + 8) * 4), line     # a transposing gather: 3 channel rows of the padded LDS tile
            assert gx == 4, line                # 4 images of 24 pixels x 3 channels: one unit of work each
    # an image of 3 x 4 x 6 floats: 16-byte accesses on both sides while the bases are aligned, 4-byte ones off by one float
    assert "<1, true, true>" in sections["lay-1-0-0"][0][-1] and "<1, false, false>" in sections["lay-1-0-1"][0][-1]
    assert "<1, true, true>" in sections["lay-0-1-0"][0][-1] and "<1, false, false>" in sections["lay-0-1-1"][0][-1]
    assert "<1, true>" in sections["lay-0-0-0"][0][-1] and "<1, false>" in sections["lay-1-1-1"][0][-1]
    # one channel, or one pixel: the two layouts are the same order, and the gather is the row copy
    assert [s[0] for s in sections["gray"]] == ["copy_kernel"] and [s[0] for s in sections["onepixel"]] == ["copy_kernel"]


def test_device_dataset_protocol_on_a_planning_context(plan_ctx):
    from face_generator_amd.runtime import DeviceDataset, FgError
    x = np.arange(5 * 3 * 4 * 6, dtype=np.float32).reshape(5, 3, 4, 6)
    for images in (x, torch.tensor(x)):
        ds = DeviceDataset(plan_ctx, images)
        assert ds.size() == len(ds) == 5 and (ds.c, ds.h, ds.w) == (3, 4, 6)
        item = ds[3]
        assert item.shape == (3, 4, 6) and item.device.type == "cpu" and np.array_equal(item.numpy(), x[3])
        assert np.array_equal(ds.rows(1, 3).numpy(), x[1:3])
        assert ds.gather([0, 4, 4]).shape == (3, 4, 6, 3) and ds.gather([1], layout="nchw").shape == (1, 3, 4, 6)
        assert ds.gather(torch.tensor([2, 2], dtype=torch.int32)).shape == (2, 4, 6, 3)
        assert ds.gather([]).shape == (0, 4, 6, 3)
        out = torch.zeros(2 * 72)
        assert ds.gather([1, 2], out=out).data_ptr() == out.data_ptr()
        for wrong in ([5], [-1], [0, 1, 99]):
            with pytest.raises(IndexError):
                ds.gather(wrong)
        with pytest.raises(IndexError):
            ds[5]
        with pytest.raises(FgError):
            ds.gather([0], layout="hwc")
        with pytest.raises(FgError):
            ds.gather([0], out=torch.zeros(7))
    with pytest.raises(FgError):
        DeviceDataset(plan_ctx, np.zeros((3, 4, 6), dtype=np.float32))
    scaled = DeviceDataset(plan_ctx, np.zeros((2, 3, 8, 8), dtype=np.float32), scale=4)
    assert (scaled.size(), scaled.c, scaled.h, scaled.w) == (2, 3, 4, 4)
    same = DeviceDataset(plan_ctx, x[:, :, :, :4], scale=4)
    assert np.array_equal(same[2].numpy(), x[2, :, :, :4])


def test_resident_result_protocol_on_a_planning_context(plan_ctx):
    from face_generator_amd import dataset_c2f
    from face_generator_amd.runtime import DeviceDataset
    fine = torch.rand(6, 3, 16, 16)
    res = dataset_c2f.toResultResident(fine, 8, 16, ctx=plan_ctx)
    assert res.size() == len(res) == 6
    assert all(isinstance(getattr(res, f), DeviceDataset) and getattr(res, f).size() == 6 for f in ("fine", "coarse", "diff"))
    ex = res[4]
    assert isinstance(ex, dataset_c2f.Example) and torch.equal(ex.fine, fine[4]) and ex.coarse.shape == ex.diff.shape == (3, 16, 16)
    assert res.gather([0, 5, 5], "coarse").shape == (3, 16, 16, 3)
    with pytest.raises(ValueError):
        dataset_c2f.toResultResident(fine, 8, 32, ctx=plan_ctx)


class RecordingRandom(random.Random):
    """S.rng with a log of every randrange(n) it answers"""

    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def randrange(self, *a, **k):
        v = super().randrange(*a, **k)
        self.log.append((a, v))
        return v


class ListDataset:
    def __init__(self, items):
        self.items = items

    def size(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _draws_of_adversarial(plan_ctx, resident, gate):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import DeviceDataset
    from face_generator_amd.state import S
    C, B, N = 1, 16, 23
    S.reset()
    adversarial.accs.clear()
    S.OPT.update(batchSize=B, noiseDim=100, N_epoch=51, saveFreq=1000, seed=11, grayscale=True, D_iterations=2)
    S.IMG_DIMENSIONS = (C, 32, 32)
    torch.manual_seed(5)
    S.MODEL_G = nn_utils.activateCuda(models.create_G((C, 32, 32), 100))
    S.MODEL_D = nn_utils.activateCuda(models.create_D((C, 32, 32)))
    S.rng = RecordingRandom(11)
    images = np.random.default_rng(3).uniform(0, 1, (N, C, 32, 32)).astype(np.float32)
    data = DeviceDataset(plan_ctx, images) if resident else ListDataset(list(images))
    adversarial.train(data, 0.6 if gate else 1.01, 3)
    return S.rng.log, S.rng.getstate()


@pytest.mark.parametrize("gate", [False, True])
def test_resident_and_host_fed_adversarial_train_draw_the_same_indices(plan_ctx, gate):
    """N_epoch = 51 (odd) at batch 16: batches of 16 x 5, then 10, then the skip; D_iterations = 2"""
    host, host_state = _draws_of_adversarial(plan_ctx, False, gate)
    res, res_state = _draws_of_adversarial(plan_ctx, True, gate)
    assert len(host) == 2 * (5 * 8 + 5) and host == res and host_state == res_state
    assert all(a == (23,) and 0 <= v < 23 for a, v in host)


def _draws_of_c2f(plan_ctx, resident):
    from face_generator_amd import models_c2f, adversarial_c2f, dataset_c2f
    from face_generator_amd.state import S
    Sz, B = 16, 8
    S.reset()
    S.OPT.update(batchSize=B, N_epoch=15, D_iterations=2, G_iterations=1, saveFreq=1000, seed=3, coarseSize=Sz // 2, fineSize=Sz)
    S.IMG_DIMENSIONS = (3, Sz, Sz)
    torch.manual_seed(5)
    S.MODEL_G = models_c2f.create_G((3, Sz, Sz), cuda=True, max_batch=B)
    S.MODEL_D = models_c2f.create_D((3, Sz, Sz), cuda=True, max_batch=B)
    S._trainer = adversarial_c2f.TrainerC2F(plan_ctx, S.MODEL_G, S.MODEL_D, S.OPT)
    S.rng = RecordingRandom(3)
    fine = torch.tensor(np.random.default_rng(4).uniform(0, 1, (11, 3, Sz, Sz)).astype(np.float32))
    data = (dataset_c2f.toResultResident if resident else dataset_c2f.toResult)(fine, Sz // 2, Sz, ctx=plan_ctx)
    adversarial_c2f.train(data)
    n_train = len(S.rng.log)
    adversarial_c2f.best_dist = -1.0            # no checkpoint from the planning run
    adversarial_c2f.approxParzen(data, 3, 5)
    return S.rng.log, n_train, S.rng.getstate()


def test_resident_and_host_fed_c2f_train_and_parzen_draw_the_same_indices(plan_ctx):
    """N_epoch = 15 (odd) at batch 8: batches of 8, 8, 6 (the last one cut from 7), then the skip at t = 13; per batch and
    D-iteration half picks for the real pair and half for the fake conds, then the batch's picks for G's conds"""
    host, n_host, host_state = _draws_of_c2f(plan_ctx, False)
    res, n_res, res_state = _draws_of_c2f(plan_ctx, True)
    assert n_host == n_res == 2 * (4 + 4) * 2 + 2 * (3 + 3) + (8 + 8 + 6)
    assert len(host) == n_host + 3 and host == res and host_state == res_state


def test_lua_files_parse_and_the_loops_use_the_device_dataset():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lua_parser
    src = {}
    for name in ("facegen_hip", "adversarial_hip", "adversarial_c2f_hip", "sample_hip"):
        src[name] = open(os.path.join(ROOT, "lua", name + ".lua")).read()
        lua_parser.parse(src[name])
    fg = src["facegen_hip"]
    for probe in ("function M.gatherImages(", "function M.Dataset(", "function Dataset:size()", "function Dataset:gather(",
                  "C.fg_gather_images(ctx,", "Dataset.__index = function(self, k)", "function M.residentResult("):
        assert probe in fg, probe
    assert "int fg_gather_images(fg_ctx* ctx, const float* set, long long n_set" in fg      # the generated cdef
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_lua_cdef.py"), "--check"])
    assert r.returncode == 0, "lua/facegen_hip.lua: the cdef block is not what scripts/gen_lua_cdef.py generates"
    assert "FG.isDataset(dataset)" in src["adversarial_hip"] and "dataset:gather(picks)" in src["adversarial_hip"]
    c2f = src["adversarial_c2f_hip"]
    assert "FG.isDataset(trainData.coarse)" in c2f and c2f.count(":gather(") >= 5 and "FG.isDataset(ds.coarse)" in c2f
    assert "FG.Dataset(" in src["sample_hip"] and "FG.gatherImages(" in src["sample_hip"]
    # the host-fed loops are still there, word for word
    assert "for i = 1, half do real[i] = dataset[math.random(dataset:size())] end" in src["adversarial_hip"]
    assert "local ex = trainData[math.random(trainData:size())]" in c2f
