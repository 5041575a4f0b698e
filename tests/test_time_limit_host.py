"""The step limit's host side (tg_set_time_limit): decode_episodes with and without the
truncated flag, and tg_stats' layout as a C compiler sees include/tg_amd.h against the ctypes
mirror.  (tests/test_capi.py's export check covers the new symbol by itself.)"""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_rows(recs):
    """(env, ret, len word) -> the 16-B tg_episode rows as int64 [k, 2] (little endian:
    ret in the low half of the second word, len in the high half)"""
    return torch.tensor([[env, (ret & 0xFFFFFFFF) | (ln << 32)] for env, ret, ln in recs],
                        dtype=torch.int64).reshape(len(recs), 2)


def test_decode_episodes_strips_the_flag(tg):
    T = tg._lib.TG_EPISODE_TRUNCATED
    assert T == 1 << 30
    recs = [(0, 5, 7), (3, -4, 7 | T), (2**40 + 1, 0, 1 | T), (9, -2**31, 2**30 - 1),
            (10, 2**31 - 1, (2**30 - 1) | T)]
    rows = raw_rows(recs)
    plain = tg.TreasureGameVec.decode_episodes(rows)
    assert plain.dtype == torch.int64 and tuple(plain.shape) == (5, 3)
    assert plain.tolist() == [[0, 5, 7], [3, -4, 7], [2**40 + 1, 0, 1], [9, -2**31, 2**30 - 1],
                              [10, 2**31 - 1, 2**30 - 1]]
    flagged = tg.TreasureGameVec.decode_episodes(rows, truncated=True)
    assert flagged.dtype == torch.int64 and tuple(flagged.shape) == (5, 4)
    assert torch.equal(flagged[:, :3], plain)
    assert flagged[:, 3].tolist() == [0, 1, 1, 0, 1]
    empty = raw_rows([])
    assert tuple(tg.TreasureGameVec.decode_episodes(empty).shape) == (0, 3)
    assert tuple(tg.TreasureGameVec.decode_episodes(empty, truncated=True).shape) == (0, 4)


def test_done_bits(tg):
    assert (tg.DONE_TERMINATED, tg.DONE_TRUNCATED) == (1, 2)
    assert (tg._lib.TG_DONE_TERMINATED, tg._lib.TG_DONE_TRUNCATED) == (1, 2)


def test_stats_layout_matches_the_header(tg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler (cc / gcc) for the header's layout check")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tg_amd.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %u %u %d\\n", sizeof(tg_stats),\n'
                   "         offsetof(tg_stats, episodes_truncated), TG_DONE_TERMINATED,\n"
                   "         TG_DONE_TRUNCATED, TG_EPISODE_TRUNCATED);\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    size, off, term, trunc, flag = map(int, subprocess.check_output([str(exe)]).split())
    S = tg._lib.Stats
    assert size == ctypes.sizeof(S)
    assert off == S.episodes_truncated.offset
    assert S._fields_[-1][0] == "episodes_truncated"  # appended: earlier offsets unchanged
    assert off + 8 == size
    assert (term, trunc, flag) == (tg._lib.TG_DONE_TERMINATED, tg._lib.TG_DONE_TRUNCATED,
                                   tg._lib.TG_EPISODE_TRUNCATED)
