"""CPU: the host half of the block-id step under AddressSanitizer + UndefinedBehaviorSanitizer, as the stand-alone
program tools/sanitize/blockids_check.cpp (nothing is loaded into Python).  The cells, the residency table and every
output sit in exact-size heap buffers, so one element read past an input, or written past an output, is a report;
the program's output must equal blockids_ref's restatement.  The cases of test_blockids.py: the patterns with no
table, every rule with the mixed table (also cut below the slots in use), the SEB_ERR_RANGE retry, the sizes alone,
cells == 0 and the refusals."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import blockids_ref as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tools", "sanitize", "blockids_check.cpp"),
       os.path.join(ROOT, "storage-engines_amd", "csrc", "seb_blockids.cpp")]


def nums(a):
    if a is None:
        return "null"
    return ",".join(str(int(x)) for x in np.asarray(a).reshape(-1)) or "-"


def line(cand, blocks, first=None, count=None, id_base=0, mode="plan", cells=None, slots=None):
    return " ".join([nums(cand), nums(blocks), str(len(cand) if cells is None else cells), nums(first), nums(count),
                     str((0 if first is None else len(first)) if slots is None else slots), str(id_base), str(mode)])


lst = lambda c, t: np.array([] if c == "-" else [int(x) for x in c.split(",")], t)  # noqa: E731


def test_block_ids_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "blockids_check")
    san = ["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <sanitizer/asan_interface.h>\nint main() { return 0; }\n")
    r = subprocess.run([*san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:  # only a toolchain without the sanitizers skips; the real sources must compile
        pytest.skip(f"sanitizer build unavailable: {r.stderr[-400:]}")
    r = subprocess.run([*san, "-o", exe, *SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = []  # (input line, ("A", sizes, bid, uniq_slot, uniq_block) | ("S", sizes) | ("R", rc, sizes or None))

    def add(cand, blocks, first=None, count=None, id_base=0, mode="plan"):
        want = bref.block_ids(cand, blocks, first, count, id_base)
        cases.append((line(cand, blocks, first, count, id_base, mode), ("A",) + want))

    first, count = bref.table_mixed()
    for cells in (1, 63, 65, 257, 1025):
        for name in bref.PATTERNS:
            cand, blocks = bref.pattern(name, cells)
            add(cand, blocks)
            add(cand, blocks, first, count, id_base=cells)
        cand, blocks = bref.pattern("mixed", cells)
        add(cand, blocks, first[:1], count[:1])          # res_slots below the slots in use
        add(cand, blocks, first[:4], count[:4])
    e16, e64 = np.zeros(0, np.uint16), np.zeros(0, np.uint64)
    cases.append((line(e16, e64), ("A", (0, 0, 0, 0, 0), np.zeros(0, np.uint32), e16, e64)))
    cases.append((line(None, None, cells=0), ("A", (0, 0, 0, 0, 0), np.zeros(0, np.uint32), e16, e64)))
    cases.append((line(None, None, cells=0, mode="sizes"), ("S", (0, 0, 0, 0, 0))))
    # the SEB_ERR_RANGE retry, a larger capacity, the sizes alone
    cand, blocks = bref.pattern("7x3", 257)
    want = bref.block_ids(cand, blocks, id_base=5)
    uniq = want[0][3]
    cases.append((line(cand, blocks, id_base=5, mode=uniq - 1), ("R", -4, want[0])))
    cases.append((line(cand, blocks, id_base=5, mode=0), ("R", -4, want[0])))
    cases.append((line(cand, blocks, id_base=5, mode=uniq), ("A",) + want))
    cases.append((line(cand, blocks, id_base=5, mode=uniq + 7), ("A",) + want))
    cases.append((line(cand, blocks, id_base=bref.NO_ID, mode="sizes"), ("S", want[0])))
    # refusals: null inputs, a table without one of its arrays, 2^32 cells, ids past 2^32 - 2
    cases.append((line(None, blocks, cells=257), ("R", -1, None)))
    cases.append((line(cand, None, cells=257), ("R", -1, None)))
    cases.append((line(cand, blocks, first, None, slots=6), ("R", -1, None)))
    cases.append((line(cand, blocks, None, count, slots=6), ("R", -1, None)))
    cases.append((line(None, None, cells=2**32), ("R", -2, None)))
    cases.append((line(cand, blocks, id_base=bref.NO_ID - uniq + 1, mode=uniq), ("R", -5, want[0])))
    top = bref.block_ids(cand, blocks, id_base=bref.NO_ID - uniq)
    cases.append((line(cand, blocks, id_base=bref.NO_ID - uniq, mode=uniq), ("A",) + top))
    inp = "".join(ln + "\n" for ln, _ in cases)
    r = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "ERROR: " not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {len(cases)}"
    refused = 0
    for i, ((_, want), got) in enumerate(zip(cases, lines)):
        f = got.split()
        if want[0] == "R":
            assert int(f[0]) == want[1] and len(f) == 6, (i, got)
            if want[2] is not None:
                assert tuple(int(x) for x in f[1:6]) == want[2], (i, got)
            refused += 1
        else:
            assert f[0] == "0", (i, got)
            assert tuple(int(x) for x in f[1:6]) == want[1], (i, got)
            if want[0] == "S":
                assert len(f) == 6, (i, got)
                continue
            have = (lst(f[6], np.uint32), lst(f[7], np.uint16), lst(f[8], np.uint64))
            bref.assert_same(have, (want[2].reshape(-1), want[3], want[4]), f"case {i}")
    assert refused == 8
