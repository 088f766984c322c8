"""CPU: the arithmetic of the context forms' staging layer (csrc/seb_stage.h: Carver, RunOut, run_sections and
runs_upload_bytes) under AddressSanitizer + UndefinedBehaviorSanitizer, as the stand-alone program
tools/sanitize/stage_check.cpp (nothing is loaded into Python; the header's part without HIP compiles alone).  The
program lives in every layout, in a heap buffer of exactly the layout's total, so a section past the total is a
report; its printed table must have, per case, the properties computed here in numpy: every offset a multiple of
16, the sections in order and disjoint, the total at least the sum of the sizes and exactly the sum of the sizes
rounded up to 16 each, and runs_upload_bytes at least where the walk over the runs ends.  Sizes and entry counts
from {0, 1, 15, 16, 17, 4096}; runs with and without deleted, seq and values."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "sanitize", "stage_check.cpp")
SIZES = (0, 1, 15, 16, 17, 4096)


def up16(x):
    return (np.asarray(x, np.uint64) + np.uint64(15)) & ~np.uint64(15)


def check_layout(sizes, offs, total, what):
    """The sections of `sizes` bytes at `offs` in a buffer of `total`."""
    sizes, offs = np.asarray(sizes, np.uint64), np.asarray(offs, np.uint64)
    assert not (offs % 16).any(), (what, "an offset off a 16-byte boundary")
    assert (offs[1:] >= offs[:-1] + sizes[:-1]).all(), (what, "sections out of order or overlapping")
    assert offs[-1] + sizes[-1] <= total, (what, "the last section passes the total")
    assert total >= sizes.sum(), what
    want = np.concatenate([[0], np.cumsum(up16(sizes))])
    assert offs.tolist() == want[:-1].tolist() and total == want[-1], (what, "not the sizes rounded up to 16 each")


def index_bytes(n):  # stage_check.cpp's stand-in for the kernels' index size
    return 13 * n + 5 if n else 0


def test_staging_arithmetic_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "stage_check")
    san = ["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <sanitizer/asan_interface.h>\nint main() { return 0; }\n")
    r = subprocess.run([*san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:  # only a toolchain without the sanitizers skips; the real sources must compile
        pytest.skip(f"sanitizer build unavailable: {r.stderr[-400:]}")
    r = subprocess.run([*san, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "ERROR: " not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    rows = {}
    for line in lines[:-1]:
        head, tail = line.split(" : ")
        kind, *args = head.split()
        rows[(kind,) + tuple(int(x) for x in args)] = [int(x) for x in tail.split()]
    assert lines[-1] == f"ok {len(rows)}" and len(rows) == len(lines) - 1
    # the carver: four sections
    for sizes in itertools.product(SIZES, repeat=4):
        got = rows.pop(("C",) + sizes)
        check_layout(sizes, got[:4], got[4], ("C", sizes))
    # a sorted run's six arrays, with and without sequences
    for kb, vb, n, seq in itertools.product(SIZES, SIZES, SIZES, (0, 1)):
        got = rows.pop(("R", kb, vb, n, seq))
        check_layout([kb, 8 * (n + 1), vb, 8 * (n + 1), n, 8 * n if seq else 0], got[:6], got[6], ("R", kb, vb, n, seq))
    # two host runs (n and 17 entries) as runs_upload walks them
    for n, kb, vb, dele, seq, vals in itertools.product(SIZES, SIZES, SIZES, (0, 1), (0, 1), (0, 1)):
        total, cursor = rows.pop(("U", n, kb, vb, dele, seq, vals))
        need = 0
        for entries, v in ((n, vb), (17, 33)):
            if entries:  # a run of no entries takes nothing
                need += int(up16([kb, 8 * (entries + 1), 8 * (entries + 1), entries if dele else 0, 8 * entries if seq else 0,
                                  v if vals else 0, index_bytes(entries)]).sum())
        assert total >= cursor == need and total % 16 == 0, ("U", n, kb, vb, dele, seq, vals, total, cursor, need)
    assert not rows
