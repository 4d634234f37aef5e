"""CPU-only: an nn.ConcatTable discriminator (models.lua:110-376) compiled to ONE fg_net through the FG_CONCAT_TABLE / FG_BRANCH /
FG_JOIN_TABLE markers of include/facegen_hip.h, in a planning-only context (FG_DEVICE_NONE): parameter order, mask order, refusals,
the launch list of one fused 16-px iteration, and the host-side model builders against oracle nets built here from the layer lists.
(The planning-only context is process-wide: in the suite's default order this module runs after tests/test_abi_host.py, whose
no-GPU checks expect a process that has not created one.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch7_nn as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- oracle twins of the reference's table discriminators, from the layer lists of models.lua -------------------------------------
def _conv(i, o, k, rng, stride=1):
    return O.SpatialConvolution(i, o, k, k, stride, stride, (k - 1) // 2, None, rng)


def _dense(insz, rng):
    return O.Sequential(O.View(insz), O.Linear(insz, 1024, rng), O.PReLU(), O.Dropout(0.5, rng), O.Linear(1024, 1024, rng), O.PReLU())


def _table(branches, joined, rng):
    return O.Sequential(O.ConcatTable(*branches), O.JoinTable(), O.Linear(joined, 1024, rng), O.PReLU(), O.Dropout(0.5, rng),
                        O.Linear(1024, 1, rng), O.Sigmoid())


def oracle_D16(dims, rng):
    """models.lua:110-160"""
    c, h, w = dims
    flat = 64 * h * w // 4
    fine = O.Sequential(_conv(c, 64, 3, rng), O.PReLU(), _conv(64, 64, 3, rng), O.PReLU(), O.SpatialMaxPooling(2, 2),
                        O.SpatialDropout(0.5, rng), O.View(flat), O.Linear(flat, 1024, rng), O.PReLU(), O.Dropout(0.5, rng))
    coarse = O.Sequential(_conv(c, 32, 5, rng), O.PReLU(), _conv(32, 64, 5, rng), O.PReLU(), O.SpatialMaxPooling(2, 2),
                          O.SpatialDropout(0.5, rng), O.View(flat), O.Linear(flat, 1024, rng), O.PReLU(), O.Dropout(0.5, rng))
    return _table([fine, coarse, _dense(c * h * w, rng)], 3072, rng)


def _strided(c, k, ws, flat, nout, dropout, rng):
    mods, i = [], c
    for o, s in ws:
        mods += [_conv(i, o, k, rng, s), O.PReLU()]
        i = o
    mods += [O.SpatialDropout(0.5, rng), O.View(flat), O.Linear(flat, nout, rng), O.PReLU()]
    if dropout:
        mods.append(O.Dropout(0.5, rng))
    return O.Sequential(*mods)


def oracle_D16_b(dims, rng):
    """models.lua:161-216"""
    c, h, w = dims
    ws, flat = [(64, 1), (64, 1), (128, 1), (128, 2)], 128 * h * w // 4
    return _table([_strided(c, 3, ws, flat, 512, True, rng), _strided(c, 5, ws, flat, 512, True, rng), _dense(c * h * w, rng)], 2048, rng)


def oracle_D16_c(dims, rng):
    """models.lua:218-274"""
    c, h, w = dims
    ws, flat = [(64, 1), (64, 1), (128, 1), (128, 2), (512, 2)], 512 * h * w // 16
    return _table([_strided(c, 3, ws, flat, 1024, False, rng), _strided(c, 5, ws, flat, 1024, False, rng), _dense(c * h * w, rng)], 3072, rng)


def oracle_D32(dims, rng):
    """models.lua:322-376"""
    c, h, w = dims
    ff, fc = 64 * h * w // 4, 54 * h * w // 16
    fine = O.Sequential(_conv(c, 64, 3, rng), O.PReLU(), _conv(64, 64, 3, rng), O.PReLU(), O.SpatialMaxPooling(2, 2),
                        O.SpatialDropout(0.5, rng), O.View(ff), O.Linear(ff, 1024, rng), O.PReLU())
    coarse = O.Sequential(_conv(c, 32, 5, rng), O.PReLU(), _conv(32, 32, 5, rng), O.PReLU(), O.SpatialMaxPooling(2, 2),
                          _conv(32, 54, 5, rng), O.PReLU(), _conv(54, 54, 5, rng), O.PReLU(), O.SpatialMaxPooling(2, 2),
                          O.SpatialDropout(0.5, rng), O.View(fc), O.Linear(fc, 1024, rng), O.PReLU(), O.Dropout(0.5, rng),
                          O.Linear(1024, 1024, rng), O.PReLU())
    return _table([fine, coarse, _dense(c * h * w, rng)], 3072, rng)


ORACLES = dict(create_D16_d=lambda d, r: O.create_D16_d(d, r), create_D16=oracle_D16, create_D16_b=oracle_D16_b,
               create_D16_c=oracle_D16_c, create_D32=oracle_D32)
# the nets a device plan is built for (create_D32's 54-channel max-pool has no kernel; it stays a host-side model)
COMPILED = [("create_D16_d", (3, 16, 16)), ("create_D16_d", (1, 16, 16)), ("create_D16", (3, 16, 16)), ("create_D16", (1, 16, 16)),
            ("create_D16_b", (3, 16, 16)), ("create_D16_b", (1, 16, 16)), ("create_D16_c", (3, 16, 16)), ("create_D16_c", (1, 16, 16))]
COUNTS = {("create_D16", (3, 16, 16)): 13467914, ("create_D16", (1, 16, 16)): 12940874, ("create_D16_b", (3, 16, 16)): 13308046,
          ("create_D32", (3, 32, 32)): 28894941}


@pytest.fixture(scope="module")
def plan_ctx():
    from face_generator_amd import build
    from face_generator_amd.runtime import get_context
    build.build(verbose=False)
    return get_context(-1)


def _flat_offsets(onet):
    """{id(module): (weight offset, weight n, bias offset, bias n)} in the oracle's getParameters() order"""
    offs, off = {}, 0
    for (m, pn, gn) in onet.parameters():
        n = getattr(m, pn).size
        e = offs.setdefault(id(m), [-1, 0, -1, 0])
        if pn == "weight":
            e[0], e[1] = off, n
        else:
            e[2], e[3] = off, n
        off += n
    return offs, off


def _flat_modules(onet):
    """the oracle's modules in the order of the flat spec list: marker slots are None"""
    ct = onet.modules[0]
    out = [None]
    for b in ct.modules:
        out.append(None)
        out.extend(b.modules)
    out.append(None)
    return out + list(onet.modules[2:])


@pytest.mark.parametrize("name,dims", COMPILED)
def test_one_plan_follows_the_oracle_parameter_and_mask_order(plan_ctx, name, dims):
    from face_generator_amd import models
    from face_generator_amd.runtime import DeviceNet
    B = 4
    onet = ORACLES[name](dims, np.random.default_rng(5))
    net = getattr(models, name)(dims)
    specs = net.layer_specs()
    assert specs[0] == ("CONCAT_TABLE", len(net.branches)) and [s[0] for s in specs].count("BRANCH") == len(net.branches)
    dn = DeviceNet(plan_ctx, specs, dims, B)
    offs, total = _flat_offsets(onet)
    assert dn.n_params == total
    if (name, dims) in COUNTS:
        assert total == COUNTS[(name, dims)]
    fm = _flat_modules(onet)
    assert len(fm) == len(specs)
    for i, m in enumerate(fm):
        got = dn.param_offsets(i)
        if m is None or id(m) not in offs:
            assert got[1] == 0 and got[3] == 0, (i, got)
        else:
            want = offs[id(m)]
            assert (got[0], got[1]) == (want[0], want[1]), (i, type(m).__name__, got, want)
            if want[3]:
                assert (got[2], got[3]) == (want[2], want[3]), (i, type(m).__name__, got, want)
    # dropout masks: module order across the branches, then the tail; sizes from an oracle forward
    onet.forward(np.zeros((B,) + tuple(dims), np.float32))
    want = []
    for m in O.walk_modules(onet):
        if isinstance(m, O.SpatialDropout):
            want.append(B * m.output.shape[1])
        elif isinstance(m, O.Dropout):
            want.append(m.output.size)
    assert dn.n_masks == len(want)
    assert [dn.mask_shape(i, B)[0] for i in range(dn.n_masks)] == want
    assert (dn.out_c, dn.out_h, dn.out_w) == (1, 1, 1)
    # the markers own no activation
    with pytest.raises(Exception):
        dn.layer_output(0)


def test_create_D32_is_refused_by_name_not_computed(plan_ctx):
    """create_D32 (models.lua:322-376) is a host-side model only: its coarse branch pools a 54-channel map, the max-pool kernels
    read four channels at a time.  fg_net_create names the layer; nothing is built."""
    from face_generator_amd import models, FgError
    D = models.create_D32((3, 32, 32))
    onet = oracle_D32((3, 32, 32), np.random.default_rng(5))
    assert sum(getattr(m, n).numel() for m, n in D.parameter_list()) == onet.getParameters()[0].size == COUNTS[("create_D32", (3, 32, 32))]
    with pytest.raises(FgError, match=r"layer 2[0-9]: MaxPool"):
        D.cuda(plan_ctx, max_batch=4)
    assert D.device_net is None


BAD = {
    "join without a table": [("LINEAR", 768, 8), ("JOIN_TABLE",)],
    "fewer branches than announced": [("CONCAT_TABLE", 3), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("BRANCH",), ("VIEW", 768),
                                      ("LINEAR", 768, 8), ("JOIN_TABLE",), ("LINEAR", 16, 1)],
    "more branches than announced": [("CONCAT_TABLE", 2), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("BRANCH",), ("VIEW", 768),
                                     ("LINEAR", 768, 8), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("JOIN_TABLE",), ("LINEAR", 24, 1)],
    "nested table": [("CONCAT_TABLE", 2), ("BRANCH",), ("CONCAT_TABLE", 2), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("BRANCH",),
                     ("VIEW", 768), ("LINEAR", 768, 8), ("JOIN_TABLE",), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("JOIN_TABLE",)],
    "table behind another layer": [("CONV", 3, 64, 3, 1), ("CONCAT_TABLE", 2), ("BRANCH",), ("VIEW", 64 * 256), ("LINEAR", 64 * 256, 8),
                                   ("BRANCH",), ("VIEW", 64 * 256), ("LINEAR", 64 * 256, 8), ("JOIN_TABLE",), ("LINEAR", 16, 1)],
    "branch ends in a spatial map": [("CONCAT_TABLE", 2), ("BRANCH",), ("CONV", 3, 64, 3, 1), ("PRELU",), ("BRANCH",), ("VIEW", 768),
                                     ("LINEAR", 768, 8), ("JOIN_TABLE",), ("LINEAR", 16, 1)],
    "five branches": [("CONCAT_TABLE", 5)] + [("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8)] * 5 + [("JOIN_TABLE",), ("LINEAR", 40, 1)],
    "table never closed": [("CONCAT_TABLE", 2), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8)],
    "BatchNorm in a branch": [("CONCAT_TABLE", 2), ("BRANCH",), ("CONV", 3, 64, 3, 1), ("BATCHNORM", 64), ("VIEW", 64 * 256),
                              ("LINEAR", 64 * 256, 8), ("BRANCH",), ("VIEW", 768), ("LINEAR", 768, 8), ("JOIN_TABLE",), ("LINEAR", 16, 1)],
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_malformed_tables_are_refused_with_a_message(plan_ctx, what):
    from face_generator_amd.runtime import make_specs
    lib = plan_ctx.lib
    specs = make_specs(BAD[what])
    h = ctypes.c_void_p()
    rc = lib.fg_net_create(plan_ctx.h, specs, len(BAD[what]), 3, 16, 16, ctypes.byref(h))
    assert rc < 0 and not h.value, (what, rc)
    msg = lib.fg_last_error(plan_ctx.h).decode()
    assert "layer" in msg and len(msg) > 20, msg


def test_wellformed_small_tables_plan_and_run(plan_ctx):
    """2, 3 and 4 branches plan, and a dry forward / backward (both flag combinations) walks every stage"""
    from face_generator_amd.runtime import DeviceNet
    for widths in ((8, 8), (4, 12, 8), (4, 12, 8, 128)):
        specs = [("CONCAT_TABLE", len(widths))]
        for wd in widths:
            specs += [("BRANCH",), ("VIEW", 768), ("LINEAR", 768, wd)] + ([("PRELU",), ("DROPOUT", 0, 0, 0, 0, 0.5)] if wd > 4 else [])
        specs += [("JOIN_TABLE",), ("LINEAR", sum(widths), 1), ("SIGMOID",)]
        dn = DeviceNet(plan_ctx, specs, (3, 16, 16), 5)
        assert dn.n_params == sum(768 * wd + wd + (1 if wd > 4 else 0) for wd in widths) + sum(widths) + 1
        assert dn.n_masks == sum(1 for wd in widths if wd > 4)
        x = torch.zeros(5, 16, 16, 3)
        dn.forward(x)
        assert dn.backward(torch.zeros(5, 1), True, True).shape == x.shape
        dn.backward(torch.zeros(5, 1), True, False)


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
from face_generator_amd import models, adversarial
from face_generator_amd.runtime import get_context
ctx = get_context(-1)
B = 8
G = models.create_G((3, 16, 16), 100).cuda(ctx, max_batch=B)
D = models.create_D((3, 16, 16)).cuda(ctx, max_batch=B)
tr = adversarial.Trainer(ctx, G, D, dict(batchSize=B, noiseDim=100))
assert tr.gan is not None
for it in range(2):
    sys.stderr.write("fg-iteration %%d\n" %% it); sys.stderr.flush()
    tr.step_D(torch.zeros(B // 2, 16, 16, 3), None)
    tr.step_G(B)
sys.stderr.write("fg-iteration end\n")
"""


def launch_lines_of_one_16px_iteration():
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stderr.splitlines()
    a, b = lines.index("fg-iteration 1"), lines.index("fg-iteration end")
    return [l for l in lines[a + 1:b] if l.startswith("fg-launch")]


def test_fused_16px_iteration_plans_and_lists_its_launches(plan_ctx):
    """One D-step + one G-step of G16 / D16_d through fg_gan_create in a planning-only child process with FG_LAUNCH_LOG=1: the
    (second, steady-state) iteration lists the join in both D forwards, the split in both D backwards and the sum of the branches'
    input gradients in the G-step.  The count is recorded in profiles/r07_16px_branched.md."""
    lines = launch_lines_of_one_16px_iteration()
    names = [l.split()[1] for l in lines]
    joins = sum("rows_join_split_kernel<4, false>" in l for l in lines)
    splits = sum("rows_join_split_kernel<4, true>" in l for l in lines)
    sums = sum("sum_parts_kernel<4>" in l for l in lines)
    print("launch lines per 16-px iteration (D-step + G-step, B = 8): %d; join %d split %d sum %d" % (len(lines), joins, splits, sums))
    assert (joins, splits, sums) == (2, 2, 1), (joins, splits, sums, names)
    prof = os.path.join(ROOT, "profiles", "r07_16px_branched.md")
    assert "%d launch lines" % len(lines) in open(prof).read()


@pytest.mark.parametrize("name,dims", COMPILED + [("create_D32", (3, 32, 32))])
def test_model_builders_mirror_the_oracle_nets(name, dims):
    from face_generator_amd import models, nn
    net = getattr(models, name)(dims)
    onet = ORACLES[name](dims, np.random.default_rng(5))
    assert [type(m).__name__ for m in net.modules] == [type(m).__name__ for m in onet.modules]
    assert len(net.branches) == len(onet.modules[0].modules)
    for b, ob in zip(net.branches, onet.modules[0].modules):
        assert [type(m).__name__ for m in b.modules] == [type(m).__name__ for m in ob.modules]
        for m, om in zip(b.modules, ob.modules):
            if isinstance(m, nn.SpatialConvolution):
                assert m.spec()[1:5] == (om.weight.shape[1], om.weight.shape[0], om.weight.shape[2], (om.weight.shape[2] - 1) // 2)
                assert (2 if m.spec()[5] == 2 else 1) == om.dh
            if isinstance(m, (nn.Dropout, nn.SpatialDropout)):
                assert m.p == om.p == 0.5
    assert [tuple(getattr(m, n).shape) for m, n in net.parameter_list()] == [tuple(getattr(m, p).shape) for (m, p, g) in onet.parameters()]
    r = repr(net)
    assert r.count("nn.ConcatTable") == 1 and r.count("nn.JoinTable") == 1 and r.count("nn.Sequential") == 1 + len(net.branches)
    assert models.create_D((3, 16, 16)).branches[0].modules[0].weight.shape[0] == 128          # models.lua:98-104 still picks create_D16_d
    assert not hasattr(models.create_D((3, 32, 32)), "branches")


def test_three_branch_state_dict_and_torch7_round_trip(tmp_path):
    from face_generator_amd import models, nn, nn_utils, t7_checkpoint as C
    D = models.create_D16((3, 16, 16))
    G = models.create_G((3, 16, 16), 100)
    sd = nn_utils.state_dict(D)
    assert set(sd["layers"]) == {"branches", "tail"} and len(sd["layers"]["branches"]) == 3
    D2 = models.create_D16((3, 16, 16))
    nn_utils.load_state_dict(D2, sd)
    for (m, n), (m2, n2) in zip(D.parameter_list(), D2.parameter_list()):
        assert torch.equal(getattr(m, n), getattr(m2, n2))
    path = str(tmp_path / "adversarial.net")
    C.save_checkpoint(path, D, G, dict(scale=16, grayscale=False), 3)
    back = C.load_checkpoint(path)
    Db = back["D"]
    assert isinstance(Db, nn.ConcatSequential) and len(Db.branches) == 3
    assert Db.layer_specs() == D.layer_specs()
    for (m, n), (m2, n2) in zip(D.parameter_list(), Db.parameter_list()):
        assert torch.equal(getattr(m, n), getattr(m2, n2))
