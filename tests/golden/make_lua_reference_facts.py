"""Generate tests/golden/lua_reference_facts.json: what tests/test_lua_binding.py needs to know about the reference's own Lua scripts
(train.lua, models_c2f.lua, ...) to check lua/patches/*.patch and the re-hosted loops against them.

The reference's scripts are not part of this repository, so the tests cannot read them; this script reads a checkout of the reference
once and records, for the patches as they are now:
  * per patch: its sha256, the files it touches, and whether it applies to the untouched reference (patch -p1 --dry-run);
  * per reference script (*.lua, */*.lua): the sha256 before and after all patches, whether both versions parse (tests/lua_parser.py),
    and the free names each version reads / writes;
  * per patched script of PATCHED_PROBES: the offsets of every probe string (or "re:" pattern) in its comment-stripped text.
tests/test_lua_binding.py fails when a patch no longer has the recorded sha256: after changing a patch, run again
    python tests/golden/make_lua_reference_facts.py <reference checkout>
"""
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "lua_reference_facts.json")
sys.path.insert(0, TESTS)
from lua_parser import parse as lua_parse, LuaSyntaxError  # noqa: E402
from test_lua_binding import PATCHED_PROBES, strip_lua_comments  # noqa: E402


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def parse_facts(path):
    try:
        c = lua_parse(open(path).read())
    except LuaSyntaxError:
        return False, [], []
    return True, sorted(c.globals_read), sorted(c.globals_written)


def probe_offsets(text, probe):
    if probe.startswith("re:"):
        return [m.start() for m in re.finditer(probe[3:], text)]
    return [m.start() for m in re.finditer(re.escape(probe), text)]


def main(ref):
    patches = sorted(glob.glob(os.path.join(ROOT, "lua", "patches", "*.patch")))
    scripts = sorted(os.path.relpath(s, ref) for s in glob.glob(os.path.join(ref, "*.lua")) + glob.glob(os.path.join(ref, "*", "*.lua")))
    facts = {"about": "recorded by tests/golden/make_lua_reference_facts.py from a checkout of the reference; read by tests/test_lua_binding.py",
             "patches": {}, "scripts": {}, "probes": {}}
    tmp = tempfile.mkdtemp(prefix="fg_lua_ref_")
    try:
        for rel in scripts:
            os.makedirs(os.path.dirname(os.path.join(tmp, rel)) or tmp, exist_ok=True)
            shutil.copy(os.path.join(ref, rel), os.path.join(tmp, rel))
        for p in patches:
            targets = sorted(set(re.findall(r"^\+\+\+ b/(\S+)", open(p).read(), re.M)))
            r = subprocess.run(["patch", "-p1", "--dry-run", "-d", ref, "-i", p], capture_output=True, text=True)
            facts["patches"][os.path.basename(p)] = {"sha256": sha256(p), "targets": targets, "applies": r.returncode == 0}
        for p in patches:
            subprocess.run(["patch", "-p1", "-s", "-d", tmp, "-i", p], check=True)
        for rel in scripts:
            ok, rd, wr = parse_facts(os.path.join(ref, rel))
            pok, prd, pwr = parse_facts(os.path.join(tmp, rel))
            facts["scripts"][rel] = {"sha256": sha256(os.path.join(ref, rel)), "parses": ok, "globals_read": rd, "globals_written": wr,
                                     "patched_sha256": sha256(os.path.join(tmp, rel)), "patched_parses": pok,
                                     "patched_globals_read": prd, "patched_globals_written": pwr}
        for rel, probes in sorted(PATCHED_PROBES.items()):
            text = strip_lua_comments(open(os.path.join(tmp, rel)).read())
            facts["probes"][rel] = {pr: probe_offsets(text, pr) for pr in probes}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d patches, %d scripts" % (OUT, len(facts["patches"]), len(facts["scripts"])))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/make_lua_reference_facts.py <reference checkout>")
    main(os.path.abspath(sys.argv[1]))
