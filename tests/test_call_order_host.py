"""Call-order independence, the part that needs no device: tests/call_order.py runs every scenario of tests/CALL_ORDER.md once in a
child process on a planning-only context (get_context(-1)) with FG_LAUNCH_LOG=1.  Asserted here:
* history does not change dispatch: the launch log of every probe on the USED object equals the log of the same probe on its fresh
  twin line for line -- kernel, grid, block, LDS.  The one thing a fresh object does that a used one may not need is the re-pack of its
  weights (pack_jobs_kernel<false>, and in math mode 6 the split of the packed weights into planes right behind it) and, for a gan, the
  one-block fill of its target vectors: such a line of the TWIN's log is passed over where the used object does not launch it at that
  place (align), nothing is ever taken out of the used object's log, and the parameter-moving scenarios assert separately that the used
  object DID re-pack;
* the return codes of the calls that are refused because of what came before them -- among them the backward behind a forward that
  was itself refused (FG_ERR_WORKSPACE, a bad batch, missing masks) or is still paused, which used to run over activations that were
  never computed, and fg_gan_update behind a step that overwrote the gradients it was holding.
What the probes compute is compared on the device (tests/test_gpu_call_order.py)."""
import os
import subprocess
import sys

import pytest

import call_order as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK = "fg-launch pack_jobs_kernel<false>"
SPLIT = "fg-launch split_planes_kernel"
TARGETS = "fg-launch fill_kernel grid=1,1,1 "


@pytest.fixture(scope="module")
def run():
    """-> {(scenario, kind): dict(probes=[(who, tag, [launch lines])], notes=[...], mismatches=[...], rc={name: code}, lines=[...])}"""
    env = dict(os.environ, FG_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "call_order.py"), "host"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stderr.splitlines()
    assert lines and lines[-1] == "fg-co done", lines[-5:]
    out, cur, probe = {}, None, None
    for l in lines:
        if l.startswith("fg-co scenario "):
            _, _, name, kind = l.split()
            cur = out[(name, kind)] = dict(probes=[], mismatches=[], rc={}, lines=[])
        elif l.startswith("fg-co probe end"):
            probe = None
        elif l.startswith("fg-co probe "):
            who, tag = l[len("fg-co probe "):].split(" ", 1)
            probe = (who, tag, [])
            cur["probes"].append(probe)
        elif l.startswith("fg-co mismatch "):
            cur["mismatches"].append(l[len("fg-co mismatch "):])
        elif l.startswith("fg-co rc "):
            code, name = l[len("fg-co rc "):].split(" ", 1)
            cur["rc"][name] = int(code)
        elif l.startswith("fg-launch "):
            if probe is not None:
                probe[2].append(l)
        if cur is not None:
            cur["lines"].append(l)
    return out


def weight_splits(sc):
    """the launches that split the packed weights of this scenario's nets into bf16 planes: the line right behind a re-pack in a twin's log"""
    return {b for who, _, log in sc["probes"] if who == "twin" for a, b in zip(log, log[1:]) if a.startswith(PACK) and b.startswith(SPLIT)}


def once_only(l, splits):
    """what a FRESH object launches once and a used one may not need: the re-pack of its weights, the split of the packed weights into
    planes in its first call in math mode 6 (right behind the re-pack, or at the head of a backward in mode 6 whose forward ran in mode
    0), and a gan's fill of its BCE target vectors (one block, once per batch size)"""
    return "pack" if l.startswith(PACK) else "split" if l in splits else "targets" if l.startswith(TARGETS) else None


def align(used, twin, splits, nets, fills):
    """walks both logs in step.  Nothing is ever taken out of the USED object's log; a line of the twin's is passed over only where the
    used object does not launch it at that place and it is once_only -- at most one re-pack (with its split) per net of the object and
    `fills` target fills per probe.  -> None, or (index in used, index in twin) of the first difference"""
    i, skipped = 0, dict(pack=0, split=0, targets=0)
    for j, l in enumerate(twin):
        if i < len(used) and used[i] == l:
            i += 1
            continue
        kind = once_only(l, splits)
        if kind is None:
            return i, j
        skipped[kind] += 1
    if i < len(used) or skipped["pack"] > nets or skipped["split"] > nets or skipped["targets"] > fills:
        return i, len(twin)
    return None


CASES = [(name, k) for name, _, kinds in CO.NET_SCENARIOS + CO.GAN_SCENARIOS for k in kinds]


@pytest.mark.parametrize("name,kind", CASES)
def test_history_does_not_change_dispatch(run, name, kind):
    sc = run[(name, kind)]
    assert not sc["mismatches"], "\n".join(sc["mismatches"])
    used = [p for p in sc["probes"] if p[0] == "used"]
    twin = [p for p in sc["probes"] if p[0] == "twin"]
    assert used and [p[1] for p in used] == [p[1] for p in twin]
    # a net probe runs one net and no gan; a gan or sampler probe runs two nets, and a fresh gan fills its two target vectors
    nets, fills = (2, 2) if kind in CO.PAIRS and name != "optimizer_moves" else (1, 0)
    splits = weight_splits(sc)
    for (_, tag, a), (_, _, b) in zip(used, twin):
        assert b, "%s: the twin's probe launched nothing" % tag
        d = align(a, b, splits, nets, fills)
        if d is not None:
            i, j = d
            raise AssertionError("%s %s, %s: the used object launches %d kernels, its twin %d; first difference at launch %d / %d:\n  used: %s\n  twin: %s"
                                 % (name, kind, tag, len(a), len(b), i, j, a[i] if i < len(a) else "-", b[j] if j < len(b) else "-"))


@pytest.mark.parametrize("kind", CO.ALL_KINDS)
def test_moved_parameters_are_packed_again(run, kind):
    """behind a host write + fg_net_params_changed and behind fg_net_bind the next forward re-packs the weights, in math 6 the planes too"""
    sc = run[("params_moved", kind)]
    used = [p for p in sc["probes"] if p[0] == "used"]
    assert len(used) == 4
    for who, tag, log in used:
        assert sum(l.startswith(PACK) for l in log) == 1, tag
        i = next(i for i, l in enumerate(log) if l.startswith(PACK))
        assert ("split_planes_kernel" in log[i + 1]) == tag.startswith("math 6"), tag


@pytest.mark.parametrize("pair", ["px32", "c2f"])
def test_optimizer_moves_reach_the_fused_and_the_unfused_update(run, pair):
    """FG_FUSE_ADAM_PACK set: the update of D is ONE launch that packs as well, and the next forward does not pack; cleared, and for
    SGD / Adagrad: the next forward packs"""
    sc = run[("optimizer_moves", pair)]
    upd, cur = {}, None
    for l in sc["lines"]:
        if l.startswith("fg-co update D "):
            cur = upd.setdefault(l[len("fg-co update D "):], [])
        elif l.startswith("fg-co update end"):
            cur = None
        elif cur is not None and l.startswith("fg-launch "):
            cur.append(l)
    assert any("pack_jobs_kernel<true>" in l for l in upd["Adam with FG_FUSE_ADAM_PACK"])
    assert not any("pack_jobs_kernel" in l for l in upd["Adam without FG_FUSE_ADAM_PACK"])
    twins = {tag: log for who, tag, log in sc["probes"] if who == "twin"}
    for who, tag, log in sc["probes"]:
        if who == "used" and ": D alone" in tag:
            assert any(l.startswith(PACK) for l in log) == ("with FG_FUSE_ADAM_PACK" not in tag), tag
            # the planes follow the weights, however those were packed: the launch behind the twin's re-pack, on the used object too
            tw = twins[tag]
            assert tw[0].startswith(PACK), tag
            if tag.startswith("math 6"):
                assert tw[1].startswith(SPLIT) and tw[1] in log[:2], tag
            else:
                assert not any(l.startswith(SPLIT) for l in log + tw), tag


def test_return_codes(run):
    rc = run[("return_codes", "-")]["rc"]
    assert len(rc) >= 36
    bad = []
    for name, code in rc.items():
        want = (0 if name.startswith("FG_OK:") else CO.FG_ERR_WORKSPACE if name.startswith("FG_ERR_WORKSPACE:")
                else CO.FG_PAUSED_SYNC if name.startswith("FG_PAUSED_SYNC:") else CO.FG_ERR_INVALID)
        if code != want:
            bad.append("%s: returned %d, expected %d" % (name, code, want))
    assert not bad, "\n".join(bad)


def test_a_backward_behind_a_refused_forward_is_refused(run):
    """make_plan used to publish the batch of a forward that was then refused for its workspace: a backward at that batch passed every
    guard and ran over activations that were never computed"""
    rc = run[("return_codes", "-")]["rc"]
    for name in ("backward at the batch of a forward refused for its workspace", "backward_range at the batch of a forward refused for its workspace",
                 "backward behind a forward refused for its batch", "backward behind a forward refused for its masks",
                 "fg_net_backward_range continuing a range across a fresh forward"):
        assert rc[name] == CO.FG_ERR_INVALID, name
    assert rc["FG_OK: backward once a forward succeeded"] == 0
    assert not run[("abandoned_pause", "G32")]["mismatches"]           # ... and behind a forward that is still paused


def test_a_refused_forward_abandons_a_paused_pass(run):
    """a forward refused for its workspace has already published the offsets of ITS batch: a pass paused before it (sync-BN) must not be
    resumed over them"""
    rc = run[("return_codes", "-")]["rc"]
    assert rc["FG_PAUSED_SYNC: a forward with sync-BN pauses at the first BatchNorm"] == CO.FG_PAUSED_SYNC
    assert rc["FG_PAUSED_SYNC: a backward with sync-BN pauses at the last BatchNorm"] == CO.FG_PAUSED_SYNC
    assert rc["fg_net_forward_resume behind a refused forward that followed the paused one"] == CO.FG_ERR_INVALID
    assert rc["fg_net_backward_resume behind a refused forward that followed the paused backward"] == CO.FG_ERR_INVALID


def test_the_ledger_accounts_for_every_state_field():
    """tests/CALL_ORDER.md names every member of Stage, fg_net, OptCfg, fg_gan and fg_sampler as `Struct.member` in a table row"""
    import re
    text = open(os.path.join(ROOT, "tests", "CALL_ORDER.md")).read()
    rows = [l for l in text.splitlines() if l.startswith("|")]
    named = set(re.findall(r"`(\w+\.\w+)`", "\n".join(rows)))
    missing, total = [], 0
    for fn, name in CO.STRUCTS:
        fields = CO.struct_fields(fn, name)
        assert len(fields) >= 12, (name, fields)
        total += len(fields)
        missing += ["%s.%s" % (name, f) for f in fields if "%s.%s" % (name, f) not in named]
    assert not missing, "no ledger row for: " + ", ".join(missing)
    known = {"%s.%s" % (n, f) for fn, n in CO.STRUCTS for f in CO.struct_fields(fn, n)}
    assert not named - known, "the ledger names members that no longer exist: " + ", ".join(sorted(named - known))
    # every scenario the ledger names exists
    scen = {n for n, _, _ in CO.NET_SCENARIOS + CO.GAN_SCENARIOS} | {"return_codes"}
    used = set(re.findall(r"\b([a-z]+(?:_[a-z]+)+)\b", "\n".join(l.split("|")[3] for l in rows if l.count("|") >= 5))) & scen
    assert used == scen, "scenarios no ledger row names: " + ", ".join(sorted(scen - used))
