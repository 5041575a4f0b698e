"""csrc/'s per-subject headers stand alone (host side, no GPU).

Every `__host__ __device__`-only header compiles as a unit of its own, so each includes what it
uses; and tests/native_walk, which needs the walks, builds from tg_walk.h without the map, the
rules or the option loops.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-treasure-game_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST = [HIPCC, "-x", "hip", "--offload-host-only", "-fsyntax-only", "-std=c++17",
        "-Wno-unused-command-line-argument"]

# the per-env core by subject (tg_core.h includes the six), the hash, and the other headers the
# host checks build from
HEADERS = ["tg_state.h", "tg_mt.h", "tg_walk.h", "tg_map.h", "tg_rules.h", "tg_option.h",
           "tg_hash.h", "tg_level.h", "tg_render.h", "tg_render_scaled.h", "tg_policy_mlp.h",
           "tg_srv_word.h"]


def test_each_host_header_compiles_alone(tmp_path):
    procs = []
    for h in HEADERS:
        assert os.path.exists(os.path.join(CSRC, h)), h
        unit = tmp_path / (h[:-2] + "_unit.hip")
        unit.write_text('#include "%s"\n' % os.path.join(CSRC, h))
        procs.append((h, subprocess.Popen(HOST + [str(unit)], stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT, text=True)))
    failed = {}
    for h, p in procs:
        out = p.communicate()[0]
        if p.returncode != 0:
            failed[h] = out[-2000:]
    assert not failed, failed


def test_core_is_the_six_subject_headers():
    text = open(os.path.join(CSRC, "tg_core.h")).read()
    assert re.findall(r'^#include "(\w+\.h)"', text, re.M) == HEADERS[:6]
    code = [l for l in text.splitlines() if l.strip() and not l.startswith(("//", "#"))]
    assert code == [], code


def test_walk_check_builds_without_rules_or_options(tmp_path):
    deps = tmp_path / "walk_check.d"
    src = os.path.join(ROOT, "tests", "native_walk", "walk_check.cpp")
    subprocess.run(HOST + ["-MD", "-MF", str(deps), src], check=True, cwd=os.path.dirname(src))
    used = {os.path.basename(p) for p in deps.read_text().replace("\\\n", " ").split()
            if os.path.basename(p).startswith("tg_")}
    assert "tg_walk.h" in used
    assert not used & {"tg_core.h", "tg_map.h", "tg_rules.h", "tg_option.h"}, used
