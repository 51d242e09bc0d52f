"""The dense scans' launch plan (csrc/scan_plan.h) is a pure host function: compile it into a small program of its own
and hold it to the table recorded from the selection logic it replaced (tests/golden/gen_scan_plan_table.py), for every
tile count, dtype, metric, batch size, debug mask and group size in it.  bench.py labels its result with a kernel name
derived from the same inputs, so the selection must not move."""
import os
import runpy
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_plan_table.txt")


def _compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.fail("no host C++ compiler")


def _golden():
    """-> the group lines [(n_rows, override, NRB)], the outcomes {code: text}, the plan lines [(KT, dtype, metric, codes)]."""
    groups, outcomes, plans = [], {}, []
    for line in open(GOLDEN).read().splitlines():
        if line.startswith("#"):
            continue
        if "->" in line:
            n, o, _, nrb = line.split()
            groups.append((int(n), int(o), int(nrb)))
        elif " = " in line:
            code, text = line.split(" = ")
            outcomes[code] = text
        else:
            head, cells = line.split(" : ")
            plans.append(tuple(int(x) for x in head.split()) + ([c.split(",") for c in cells.split()],))
    return groups, outcomes, plans


def test_scan_plan_matches_the_recorded_selection(tmp_path):
    gen = runpy.run_path(os.path.join(ROOT, "tests", "golden", "gen_scan_plan_table.py"))
    KTS, BS, MASKS = gen["KTS"], gen["BS"], gen["MASKS"]
    assert KTS == (4, 8, 24, 32, 156, 160) and BS == (1, 16, 17, 64, 65, 128, 129, 256, 257, 300)
    assert MASKS == (0, 1, 2, 3, 4, 8, 16, 1 | 16)
    groups, outcomes, plans = _golden()
    assert sorted({g[2] for g in groups}) == [1, 4] and len(groups) == 4          # both group sizes, by size and pinned
    assert [p[:3] for p in plans] == [(kt, dt, m) for kt in KTS for dt in (1, 0) for m in (0, 1, 2)]
    # every search of the table as an input line of the program, with the line the table expects back
    inputs, want = [], []
    for n_rows, override, nrb in groups:
        for KT, dtype, metric, cells in plans:
            assert len(cells) == len(BS) and all(len(c) == len(MASKS) for c in cells)
            for B, cell in zip(BS, cells):
                for mask, code in zip(MASKS, cell):
                    head = "%d %d %d %d %d %d %d" % (KT, dtype, metric, n_rows, override, mask, B)
                    inputs.append(head)
                    o = outcomes[code]
                    if o == "none":
                        want.append(head + " | none")
                    else:
                        chunk_q, l2, rest = o.split(" ", 2)
                        want.append("%s | %s %d %s %s" % (head, chunk_q, nrb, l2, rest))
    assert len(inputs) == 4 * 6 * 2 * 3 * 10 * 8
    exe = str(tmp_path / "scan_plan_table")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "scan_plan_table.cpp")], check=True)
    got = subprocess.run([exe], input="\n".join(inputs) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(want)
    wrong = [(w, g) for w, g in zip(want, got) if w != g]
    assert not wrong, wrong[:5]
    # the table holds what it is meant to hold: every kernel, the refusal, a trailing 128-query pass behind a 256-query one
    text = "\n".join(want)
    for needle in (":lds:", ":bigq:", ":qreg:", ":q64:", ":gemm:", "| none", "256:qreg:16 44:bigq:8", "| 256 1 0 ", "| 256 4 0 "):
        assert needle in text, needle


def test_the_table_is_what_its_generator_writes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_scan_plan_table.py")],
                         capture_output=True, text=True, check=True).stdout
    assert out == open(GOLDEN).read()
