"""CPU: the host half of the B-tree's range scans under AddressSanitizer + UndefinedBehaviorSanitizer, as the
stand-alone program tools/sanitize/btscan_check.cpp (nothing is loaded into Python, nothing is preloaded).  Every
image, kind, level, the directory, the bounds and every output sit in exact-size heap buffers, so one byte read past
an input or written past an output is a report; the program's output must equal btree_scan_ref's restatement.  Every
shared case with its generated ranges, at a limit of 3 and (up to 400 keys) at no limit; every image the directory
refuses (every corrupt image of btree_ref, the literal deep trees), whose bytes the device tests then run on.  The directory
arithmetic and the cell locate this program runs are seb_btree.h's, the same text the kernels compile."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import btree_ref as bref
import btree_scan_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "storage-engines_amd", "csrc")
SRC = [os.path.join(ROOT, "tools", "sanitize", "btscan_check.cpp"), os.path.join(CSRC, "seb_btscan.cpp"), os.path.join(CSRC, "seb_btree.cpp")]
RULES = {1: "root", 2: "bad", 3: "level", 4: "mixed", 5: "deep", 6: "wide", 7: "twice", 8: "chain", 9: "order"}


def hx(b):
    return bytes(b).hex() or "-"


def fnv(b):
    h = 0xcbf29ce484222325
    for x in bytes(b):
        h = ((h ^ x) * 0x100000001b3) & (2**64 - 1)
    return h


def test_btree_scan_host_half_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "btscan_check")
    san = ["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <sanitizer/asan_interface.h>\nint main() { return 0; }\n")
    r = subprocess.run([*san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:  # only a toolchain without the sanitizers skips; the real sources must compile
        pytest.skip(f"sanitizer build unavailable: {r.stderr[-400:]}")
    r = subprocess.run([*san, "-o", exe, *SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = []
    for name, c in sorted(bref.cases().items()):
        kind, level, _ = bref.check(c.image, c.meta)
        try:
            d = sref.build_dir(c.image, c.meta, kind, level)[0]
        except sref.Refused:
            d = None
        starts, ends = sref.ranges(c, np.random.default_rng(17), d, cap=6)
        for limit in ((0, 3) if len(c.keys) <= 400 else (3,)):  # the large cases' unbounded ranges: the limit only
            cases.append((name, c.image, limit, starts, ends))
    for name, (image, keys) in sorted(bref.corrupt_cases().items()):
        cases.append((name, image, 0, keys[:2], keys[1:3]))
    cases.append(("refused_short", bref.cases()["e_root_split"].image[:4000], 0, [b"a"], [b""]))
    cases.append(("no_ranges", bref.cases()["e_root_split"].image, 0, [], []))
    lines = []
    for i, (name, image, limit, starts, ends) in enumerate(cases):
        path = tmp_path / f"image_{i}.db"
        path.write_bytes(image)
        lines.append(" ".join(["S", str(path), str(limit), str(len(starts)), *[hx(k) for k in starts], *[hx(k) for k in ends]]))
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "ERROR: " not in r.stderr, r.stderr[-3000:]
    out = r.stdout.strip().split("\n")
    assert out[-1] == f"ok {len(cases)}"
    nums = lambda f: [] if f == "-" else [int(x) for x in f.split(",")]  # noqa: E731
    refused = entries = 0
    for (name, image, limit, starts, ends), got in zip(cases, out):
        meta = bref.open_image(image)
        if meta is None:
            assert got == "invalid" and name.startswith("refused"), name
            continue
        kind, level, _ = bref.check(image, meta)
        try:
            d, info = sref.build_dir(image, meta, kind, level)
        except sref.Refused as e:
            f = got.split()
            assert f[0] == "refused" and RULES[int(f[1])] == e.rule and int(f[2]) == e.page, (name, got, str(e))
            refused += 1
            continue
        f = got.split()
        assert nums(f[0]) == [info["leaves"], info["keys"], info["depth"]] and nums(f[1]) == [fnv(d)], name
        want = sref.scan_by_dir(image, meta, d, starts, ends, limit)
        for j, k in enumerate(("range_status", "range_off", "status", "kloc", "klen", "vloc", "vlen", "key_off", "val_off")):
            assert nums(f[2 + j]) == [int(x) for x in want[k]], (name, limit, k)
        assert nums(f[11]) == [fnv(want["keys"])] and nums(f[12]) == [fnv(want["vals"])], name
        entries += len(want["status"])
    literal = sum(1 for c in cases if c[0].endswith("_literal"))
    assert literal >= 2 and refused == len(bref.corrupt_cases()) + literal and entries > 3_000
