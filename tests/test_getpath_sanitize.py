"""CPU: the host half of the Get path under AddressSanitizer + UndefinedBehaviorSanitizer, as the stand-alone
program tools/sanitize/getpath_check.cpp (nothing is loaded into Python).  Key batches, statuses and every output
sit in exact-size heap buffers, so one byte read past the keys or the statuses, or written past an output, is a
report; the program's output must equal getpath_ref's restatement.  The cases of test_getpath.py: every layout,
the decided fractions, the odd status bytes, empty keys, n == 0, the SEB_ERR_RANGE retry, the refusals, the join's
truth table and its bad rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import getpath_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tools", "sanitize", "getpath_check.cpp"),
       os.path.join(ROOT, "storage-engines_amd", "csrc", "seb_getpath.cpp")]


def hx(a):
    if a is None:
        return "null"
    return bytes(np.asarray(a, np.uint8)).hex() or "-"


def nums(a):
    if a is None:
        return "null"
    return ",".join(str(int(x)) for x in a) or "-"


def compact_line(keys, mem, stride=None, lead=0, caps=None):
    """stride None: a batch with offsets, `lead` bytes in front of the first key (offsets[0] != 0)."""
    if stride is None:
        off = np.cumsum([lead] + [len(k) for k in keys])
        data = b"\xee" * lead + b"".join(keys)
        f = ["C", "0", nums(off), hx(np.frombuffer(data, np.uint8))]
    else:
        f = ["C", str(stride), "null", hx(np.frombuffer(b"".join(keys), np.uint8))]
    f += [hx(mem), "plan" if caps is None else str(caps[0]), "0" if caps is None else str(caps[1])]
    return " ".join(f)


def join_line(mem, row, sst, mem_vloc=None, mem_vlen=None, sst_col=None, sst_vloc=None, sst_vlen=None):
    return " ".join(["J", hx(mem), nums(mem_vloc), nums(mem_vlen), nums(row), hx(sst), nums(sst_col), nums(sst_vloc),
                     nums(sst_vlen)])


unhex = lambda h, t=np.uint8: np.frombuffer(b"" if h == "-" else bytes.fromhex(h), t)  # noqa: E731
lst = lambda c, t: None if c == "null" else np.array([] if c == "-" else [int(x) for x in c.split(",")], t)  # noqa: E731


def test_get_path_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "getpath_check")
    san = ["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <sanitizer/asan_interface.h>\nint main() { return 0; }\n")
    r = subprocess.run([*san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:  # only a toolchain without the sanitizers skips; the real sources must compile
        pytest.skip(f"sanitizer build unavailable: {r.stderr[-400:]}")
    r = subprocess.run([*san, "-o", exe, *SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(17)
    cases = []  # (input line, ("C", sizes, keys, off, row) | ("J", five arrays) | ("R", rc, sizes or None))

    def statuses(n):
        return [np.zeros(n, np.uint8), np.where(np.arange(n) % 2, 1, 2).astype(np.uint8),
                rng.choice(np.array([0, 1, 2], np.uint8), n), rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), n)]

    def add_compact(keys, mem, stride=None, lead=0):
        cases.append((compact_line(keys, mem, stride, lead), ("C",) + pref.compact_arrays(keys, mem, stride)))

    for n in (0, 1, 2, 63, 65, 300):
        for stride in (16, 5, 24):
            keys = [bytes(rng.integers(0, 256, stride, dtype=np.uint8)) for _ in range(n)]
            for mem in statuses(n):
                add_compact(keys, mem, stride)
        for lead in (0, 7):
            keys = [bytes(rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8)) for _ in range(n)]
            for mem in statuses(n):
                add_compact(keys, mem, None, lead)
    add_compact([b""] * 5, np.array([0, 1, 0, 2, 0], np.uint8))           # a batch of empty keys only
    add_compact([b"", b"ab", b"", b"", b"c", b""], np.array([3, 0, 2, 255, 1, 0], np.uint8), lead=3)
    add_compact([b""] * 4, np.array([0, 1, 0, 0], np.uint8), stride=0)     # stride 0: keys of no bytes
    # the SEB_ERR_RANGE retry: a cap one below its size refuses with the sizes, the exact caps succeed
    keys = [bytes(rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8)) for _ in range(50)]
    mem = (np.arange(50) % 3 == 0).astype(np.uint8)
    want = pref.compact_arrays(keys, mem)
    _, m, kbytes = want[0]
    for caps in ((kbytes - 1, m), (kbytes, m - 1), (0, 0)):
        cases.append((compact_line(keys, mem, None, 2, caps), ("R", -4, want[0])))
    cases.append((compact_line(keys, mem, None, 2, (kbytes, m)), ("C",) + want))
    cases.append((compact_line(keys, mem, None, 2, (kbytes + 5, m + 2)), ("C",) + want))
    k16 = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(9)]
    cases.append((compact_line(k16, np.zeros(9, np.uint8), 16, caps=(143, 9)), ("R", -4, (9, 9, 144))))
    # refusals: offsets that decrease name the key; null statuses
    bad = compact_line([b"ab", b"c", b"def"], np.zeros(3, np.uint8)).split()
    bad[2] = "0,2,1,4"
    cases.append((" ".join(bad), ("R", -3, None)))
    # an empty batch with a null status array: valid, n == 0
    cases.append(("C 16 null - null plan 0", ("C", (0, 0, 0), np.zeros(0, np.uint8), None, np.zeros(0, np.uint32))))
    # the join's truth table, with every nullable input and with each left out
    jm, js = (x.reshape(-1).astype(np.uint8) for x in np.meshgrid(np.arange(3), np.arange(3), indexing="ij"))
    _, row = pref.compact([b""] * 9, jm)
    full = dict(mem_vloc=np.arange(1000, 1009, dtype=np.uint64), mem_vlen=np.arange(10, 19, dtype=np.uint32),
                sst_col=np.arange(3, dtype=np.uint16), sst_vloc=np.arange(5000, 5003, dtype=np.uint64),
                sst_vlen=np.arange(70, 73, dtype=np.uint32))
    for drop in (None, *full):
        part = {k: v for k, v in full.items() if k != drop}
        cases.append((join_line(jm, row, js[row], **part), ("J",) + pref.join_rows(jm, row, js[row], **part)))
    cases.append((join_line(jm, row, js[row]), ("J",) + pref.join_rows(jm, row, js[row])))
    # bad rows: unnamed undecided keys; rows outside the batch or naming decided keys
    bm = np.array([0, 1, 0, 2, 3, 0], np.uint8)
    b1 = dict(mem_vloc=np.arange(6, dtype=np.uint64) + 100, mem_vlen=np.arange(6, dtype=np.uint32) + 7,
              sst_col=np.array([1, 2], np.uint16), sst_vloc=np.array([11, 12], np.uint64), sst_vlen=np.array([3, 4], np.uint32))
    r1, s1 = np.array([0, 5], np.uint32), np.array([1, 2], np.uint8)
    cases.append((join_line(bm, r1, s1, **b1), ("J",) + pref.join_rows(bm, r1, s1, **b1)))
    r2, s2 = np.array([1, 3, 6, 2**32 - 1, 2], np.uint32), np.array([2, 1, 1, 1, 1], np.uint8)
    b2 = dict(b1, sst_col=np.arange(5, dtype=np.uint16), sst_vloc=np.arange(5, dtype=np.uint64) + 50,
              sst_vlen=np.arange(5, dtype=np.uint32) + 60)
    cases.append((join_line(bm, r2, s2, **b2), ("J",) + pref.join_rows(bm, r2, s2, **b2)))
    e0, e32 = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    cases.append((join_line(e0, e32, e0), ("J",) + pref.join_rows(e0, e32, e0)))                # n == 0 and m == 0
    cases.append((join_line(bm, e32, e0), ("J",) + pref.join_rows(bm, e32, e0)))                # m == 0
    cases.append(("J null null null 0 01 null null null", ("R", 0, None)))                     # n == 0: the row is ignored
    cases.append((f"J {hx(bm)} null null null - null null null", ("J",) + pref.join_rows(bm, e32, e0)))  # m == 0 needs no row
    inp = "".join(line + "\n" for line, _ in cases)
    r = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "ERROR: " not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {len(cases)}"
    refused = 0
    for i, ((_, want), line) in enumerate(zip(cases, lines)):
        f = line.split()
        if want[0] == "R":
            assert int(f[0]) == want[1], (i, line)
            if want[2] is not None:
                assert tuple(int(x) for x in f[1:4]) == want[2], (i, line)
            refused += want[1] != 0
        elif want[0] == "C":
            assert f[0] == "0", (i, line)
            _, sizes, keys_w, off_w, row_w = want
            assert tuple(int(x) for x in f[1:4]) == sizes, (i, line)
            assert np.array_equal(unhex(f[4]), keys_w), i
            off_g = lst(f[5], np.uint64)
            assert (off_g is None) == (off_w is None), i
            if off_w is not None:
                assert np.array_equal(off_g, off_w), i
            assert np.array_equal(lst(f[6], np.uint32), row_w), i
        else:
            assert f[0] == "0", (i, line)
            got = (unhex(f[1]), unhex(f[2]), lst(f[3], np.uint16), lst(f[4], np.uint64), lst(f[5], np.uint32))
            pref.assert_same(got, want[1:], f"case {i}")
    assert refused == 5
