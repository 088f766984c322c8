"""Time the memtable write side (seb_dev_wal_frame_*, seb_dev_run_size_delta, seb_dev_runs_fold_*) on the shapes the
engine produces, with keygen.wal_image's layout: 16-byte keys (keygen.key16), 100-byte values, a Delete (no value)
every 16th op.

  apply       a batch of 50,000 ops in random key order (sequences from 2^32 + 1) onto an active memtable of three
              runs of 50,000 entries: frame plan, frame emit (the records and their seal), the seal alone, replay
              plan, replay emit, the new run's index, the size delta
  fold        8 runs of 50,000 entries, a tenth of each run's keys shared by all eight: fold plan, fold emit
  fold_large  8 runs of 250,000 entries, the same mix

Before any timing every output of the device must equal the host half byte for byte (seb_wal_frame_emit,
seb_wal_replay_emit, seb_run_size_delta, seb_runs_fold_emit).  Then, with seb.Timer (no L2-flushing fence),
--warmup + --steps steps per shape, every step timed separately; a step that ends in its own synchronise (the
plans, the index) includes it.  Printed with the times: the DESIGN.md 5.15 model = streams / 4.4 TB/s + gathers /
351 G/s (5.14's measured bisection rate), and the host half on one thread over the same input.  One JSON line
per shape; no pass/fail threshold.

    python tools/apply_bench.py [--out profiles/apply_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd")]

import keygen as kg  # noqa: E402

STREAM_TBS = 4.4   # the 16-B vector stream rate
GATHER_GS = 351.0  # the measured rate of bisections over an L2-resident prefix array
VALUE, DELETE_EVERY = 100, 16
SHAPES = {"apply": (50_000, 3), "fold": (50_000, 8), "fold_large": (250_000, 8)}


def make_run(idx: np.ndarray, seed: int):
    """The run of key16(idx) for sorted, distinct idx: (keys u8, key_off, vals u8, val_off, deleted, seq)."""
    n = idx.size
    rng = np.random.default_rng(seed)
    dele = (np.arange(n) % DELETE_EVERY == DELETE_EVERY - 1).astype(np.uint8)
    voff = np.concatenate([[0], np.cumsum(np.where(dele == 1, 0, VALUE))]).astype(np.uint64)
    vals = rng.integers(0, 256, int(voff[-1]), dtype=np.uint8)
    return (kg.key16(idx).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(16), vals, voff, dele,
            rng.permutation(n).astype(np.uint64) + np.uint64(1))


def make_runs(n: int, count: int):
    """count runs of n entries: a tenth of a run's keys are key16(16 j), shared by every run; the others are its own,
    key16(16 j + r + 1)."""
    shared = n // 10
    j = np.arange(n - shared, dtype=np.int64)
    pool = 16 * np.sort(np.random.default_rng(3).choice(n - shared, shared, replace=False)).astype(np.int64)
    return [make_run(np.sort(np.concatenate([pool, 16 * j + r + 1])), seed=10 + r) for r in range(count)]


def make_ops(n: int):
    """n ops in random key order over the runs' key range: (keys (n, 16) u8, vals u8, val_off, deleted)."""
    rng = np.random.default_rng(4)
    keys = kg.key16(rng.permutation(n).astype(np.int64) * 7)
    voff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(VALUE))  # a Delete carries its value bytes; they are not written
    dele = (np.arange(n) % DELETE_EVERY == DELETE_EVERY - 1).astype(np.uint8)
    return keys, rng.integers(0, 256, n * VALUE, dtype=np.uint8), voff, dele


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def timed(torch, seb, fn, steps, warmup):
    t = [seb.Timer() for _ in range(2)]
    ms = []
    for step in range(warmup + steps):
        t[0].record()
        fn()
        t[1].record()
        torch.cuda.synchronize()
        if step >= warmup:
            ms.append(t[0].elapsed_ms(t[1]))
    return stats(ms)


def to_dev(torch, a):
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def upload_runs(torch, seb, runs):
    druns, dvals, indexes = [], [], []
    for keys, koff, vals, voff, dele, seq in runs:
        run = seb.dev_run(to_dev(torch, keys), to_dev(torch, koff), to_dev(torch, voff), to_dev(torch, dele), to_dev(torch, seq))
        ix = torch.empty(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
        seb.dev_run_index(run, ix)
        druns.append(run), dvals.append(to_dev(torch, vals)), indexes.append(ix)
    return druns, dvals, indexes


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def run_apply(torch, seb, n, count, steps, warmup):
    first_seq = (1 << 32) + 1
    runs = make_runs(n, count)
    keys, vals, voff, dele = make_ops(n)
    druns, _, indexes = upload_runs(torch, seb, runs)
    hruns = [seb.host_run(r[0], r[1], r[3], r[4], r[5]) for r in runs]
    dk = seb.dev_keys(to_dev(torch, keys), n=n, stride=16)
    dvals, dvoff, ddel = to_dev(torch, vals), to_dev(torch, voff), to_dev(torch, dele)
    rec = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    total = seb.dev_wal_frame_plan(dk, dvoff, ddel, rec)
    img = torch.zeros(total, dtype=torch.uint8, device="cuda")
    seb.dev_wal_frame_emit(dk, dvals, dvoff, ddel, first_seq, rec, img)
    ws = torch.zeros(seb.dev_wal_replay_workspace_size(n), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_wal_replay_plan(img, rec, ws)
    _, n_out, kb, vb = sizes[:4]
    out = [torch.zeros(kb, dtype=torch.uint8, device="cuda"), torch.zeros(n_out + 1, dtype=torch.int64, device="cuda"),
           torch.zeros(vb, dtype=torch.uint8, device="cuda"), torch.zeros(n_out + 1, dtype=torch.int64, device="cuda"),
           torch.zeros(n_out, dtype=torch.uint8, device="cuda"), torch.zeros(n_out, dtype=torch.int64, device="cuda")]
    seb.dev_wal_replay_emit(img, rec, sizes, ws, *out)
    fresh = seb.dev_run(out[0], out[1], out[3], out[4], out[5])
    fix = torch.empty(seb.dev_run_index_size(n_out), dtype=torch.uint8, device="cuda")
    delta = torch.zeros(1, dtype=torch.int64, device="cuda")
    seb.dev_run_size_delta(fresh, druns, indexes, delta)
    torch.cuda.synchronize()
    # the host half over the same input, one thread: the check, and the yardstick
    (want_img, want_off), frame_host = host_ms(lambda: seb.wal_frame(keys, vals, voff, dele, first_seq))
    want_run, replay_host = host_ms(lambda: seb.wal_replay_emit(want_img, want_off))
    hfresh = seb.host_run(want_run[0], want_run[1], want_run[3], want_run[4], want_run[5])
    want_delta, delta_host = host_ms(lambda: seb.run_size_delta(hfresh, hruns))
    assert np.array_equal(img.cpu().numpy(), want_img), "the image differs from the host half"
    assert np.array_equal(rec.cpu().numpy().view(np.uint64), want_off), "rec_off differs from the host half"
    assert sizes == want_run[6], "the replay's sizes differ from the host half"
    for o, w, what in zip(out, want_run, ("keys", "key_off", "vals", "val_off", "deleted", "seq")):
        assert np.array_equal(o.cpu().numpy().view(w.dtype), w), f"the run's {what} differs from the host half"
    assert int(delta.cpu().numpy()[0]) == want_delta, "the size delta differs from the host half"
    t = {"frame_plan": timed(torch, seb, lambda: seb.dev_wal_frame_plan(dk, dvoff, ddel, rec), steps, warmup),
         "frame_emit": timed(torch, seb, lambda: seb.dev_wal_frame_emit(dk, dvals, dvoff, ddel, first_seq, rec, img), steps, warmup),
         "seal": timed(torch, seb, lambda: seb.dev_wal_crc(img, rec, seb.WAL_SEAL), steps, warmup),
         "replay_plan": timed(torch, seb, lambda: seb.dev_wal_replay_plan(img, rec, ws), steps, warmup),
         "replay_emit": timed(torch, seb, lambda: seb.dev_wal_replay_emit(img, rec, sizes, ws, *out), steps, warmup),
         "index": timed(torch, seb, lambda: seb.dev_run_index(fresh, fix), steps, warmup),
         "delta": timed(torch, seb, lambda: seb.dev_run_size_delta(fresh, druns, indexes, delta), steps, warmup)}
    levels = int(n).bit_length()
    chunks = (total + 15) // 16
    emit_gathers, delta_gathers = chunks * levels, n_out * count * levels
    emit_bytes = 2 * total
    model = {"frame_emit_ms": round(emit_bytes / (STREAM_TBS * 1e12) * 1e3 + emit_gathers / (GATHER_GS * 1e9) * 1e3, 4),
             "delta_ms": round(delta_gathers / (GATHER_GS * 1e9) * 1e3, 4)}
    whole = sum(t[k]["median_ms"] for k in ("frame_plan", "frame_emit", "replay_plan", "replay_emit", "index", "delta"))
    return {"bench": "apply", "shape": "apply", "ops": n, "runs": [n] * count, "image_bytes": total, "entries_out": n_out,
            "size_delta": want_delta, "steps": steps, "warmup": warmup, **t, "device_sum_ms": round(whole, 4),
            "frame_emit_gathers": emit_gathers, "delta_gathers": delta_gathers, "model": model,
            "host_one_thread_ms": {"frame": frame_host, "replay": replay_host, "delta": delta_host,
                                   "sum": round(frame_host + replay_host + delta_host, 3)}}


def run_fold(torch, seb, name, n, count, steps, warmup):
    runs = make_runs(n, count)
    druns, dvals, indexes = upload_runs(torch, seb, runs)
    total = n * count
    val_bytes = [r[2].size for r in runs]
    ws = torch.zeros(seb.dev_runs_fold_workspace_size(total), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_runs_fold_plan(druns, indexes, val_bytes, ws)
    _, n_out, kb, vb = sizes[:4]
    out = [torch.zeros(kb, dtype=torch.uint8, device="cuda"), torch.zeros(n_out + 1, dtype=torch.int64, device="cuda"),
           torch.zeros(vb, dtype=torch.uint8, device="cuda"), torch.zeros(n_out + 1, dtype=torch.int64, device="cuda"),
           torch.zeros(n_out, dtype=torch.uint8, device="cuda"), torch.zeros(n_out, dtype=torch.int64, device="cuda")]
    seb.dev_runs_fold_emit(druns, indexes, dvals, sizes, ws, *out)
    torch.cuda.synchronize()
    hruns = [seb.host_run(r[0], r[1], r[3], r[4], r[5]) for r in runs]
    want, fold_host = host_ms(lambda: seb.runs_fold(hruns, [r[2] for r in runs]))
    assert sizes == want[6], "the fold's sizes differ from the host half"
    for o, w, what in zip(out, want, ("keys", "key_off", "vals", "val_off", "deleted", "seq")):
        assert np.array_equal(o.cpu().numpy().view(w.dtype), w), f"the folded run's {what} differs from the host half"
    t = {"fold_plan": timed(torch, seb, lambda: seb.dev_runs_fold_plan(druns, indexes, val_bytes, ws), steps, warmup),
         "fold_emit": timed(torch, seb, lambda: seb.dev_runs_fold_emit(druns, indexes, dvals, sizes, ws, *out), steps, warmup)}
    levels = int(n).bit_length()
    gathers = total * (count - 1) * levels
    slot_bytes = 16 * total * 4  # cleared, written, read by the sums and by the emit
    out_bytes = kb + vb + 17 * n_out + 16
    model = {"fold_plan_ms": round(gathers / (GATHER_GS * 1e9) * 1e3 + slot_bytes / (STREAM_TBS * 1e12) * 1e3, 4),
             "fold_emit_ms": round(2 * out_bytes / (STREAM_TBS * 1e12) * 1e3, 4)}
    return {"bench": "apply", "shape": name, "runs": [n] * count, "entries_in": total, "entries_out": n_out,
            "shadowed": sizes[4], "key_bytes": kb, "val_bytes": vb, "steps": steps, "warmup": warmup, **t,
            "plan_gathers": gathers, "model": model,
            "gather_rate_gs": round(gathers / (t["fold_plan"]["median_ms"] * 1e-3) / 1e9, 1),
            "host_one_thread_ms": {"fold": fold_host}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=[*SHAPES, "all"], default="all")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for name in (SHAPES if a.shape == "all" else (a.shape,)):
        n, count = SHAPES[name]
        res = run_apply(torch, seb, n, count, a.steps, a.warmup) if name == "apply" else run_fold(torch, seb, name, n, count,
                                                                                                  a.steps, a.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
