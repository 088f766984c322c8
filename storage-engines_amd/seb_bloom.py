"""Python host binding of libseb_bloom.so (the C ABI in include/seb_bloom.h), via ctypes.

`BloomFilter` mirrors the reference's Go API (lsm/bloom.go) one method per method, so the
parity tests read like the reference's own call sequences:

    NewBloomFilter(expectedKeys, fpr)  lsm/bloom.go:19   -> BloomFilter(n, p)
    (*BloomFilter).Add(key)            lsm/bloom.go:70   -> .add(key)            (deferred, batched)
    (*BloomFilter).MayContain(key)     lsm/bloom.go:82   -> .may_contain(key)
    (*BloomFilter).Encode()            lsm/bloom.go:96   -> .encode()
    DecodeBloomFilter(data)            lsm/bloom.go:105  -> BloomFilter.decode(data)  (None if < 12 B)

Every computation runs in the HIP library on the GPU: if the library is missing, or no gfx950
device is present, the device-resident and batch calls raise SebError.  The one exception is the
drop-in boundary's (SURVEY.md 8(b) error row): the Go API mirror (`BloomFilter`) keeps working on
its host copy when its device path fails, as the Go API has no error returns; `fallback_count()`
counts those uses and the GPU tests and smoke() assert it stays 0.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEB_LIB_PATH") or os.path.join(_HERE, "lib", "libseb_bloom.so")  # override: A/B builds
HEADER = os.path.join(os.path.dirname(_HERE), "include", "seb_bloom.h")

SEB_OK = 0
SEB_BUILD_FRESH = 1
ERRORS = {-1: "SEB_ERR_INVALID", -2: "SEB_ERR_DEVICE", -3: "SEB_ERR_NOMEM", -4: "SEB_ERR_RANGE", -5: "SEB_ERR_SHORT",
          -6: "SEB_ERR_INTERNAL"}


class SebError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class seb_keys(C.Structure):
    _fields_ = [("data", C.c_void_p), ("offsets", C.c_void_p), ("n", C.c_uint64), ("stride", C.c_uint32),
                ("reserved", C.c_uint32)]


class seb_sst_sizes(C.Structure):
    _fields_ = [("num_blocks", C.c_uint64), ("data_bytes", C.c_uint64), ("index_bytes", C.c_uint64),
                ("meta_bytes", C.c_uint64), ("oversize_entries", C.c_uint64)]

    def as_tuple(self):
        return (self.num_blocks, self.data_bytes, self.index_bytes, self.meta_bytes, self.oversize_entries)


class seb_merge_sizes(C.Structure):
    _fields_ = [("entries_in", C.c_uint64), ("entries_out", C.c_uint64), ("key_bytes", C.c_uint64),
                ("val_bytes", C.c_uint64), ("shadowed", C.c_uint64), ("dropped", C.c_uint64)]

    def as_tuple(self):
        return (self.entries_in, self.entries_out, self.key_bytes, self.val_bytes, self.shadowed, self.dropped)


class seb_replay_sizes(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("entries_out", C.c_uint64), ("key_bytes", C.c_uint64),
                ("val_bytes", C.c_uint64), ("overwritten", C.c_uint64), ("tombstones", C.c_uint64),
                ("max_sequence", C.c_uint64), ("memtable_size", C.c_uint64)]

    def as_tuple(self):
        return (self.records_in, self.entries_out, self.key_bytes, self.val_bytes, self.overwritten, self.tombstones,
                self.max_sequence, self.memtable_size)


class seb_fold_sizes(C.Structure):
    _fields_ = [("entries_in", C.c_uint64), ("entries_out", C.c_uint64), ("key_bytes", C.c_uint64),
                ("val_bytes", C.c_uint64), ("shadowed", C.c_uint64), ("tombstones", C.c_uint64),
                ("max_sequence", C.c_uint64), ("memtable_size", C.c_uint64)]

    def as_tuple(self):
        return (self.entries_in, self.entries_out, self.key_bytes, self.val_bytes, self.shadowed, self.tombstones,
                self.max_sequence, self.memtable_size)


class seb_compact_sizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("undecided", C.c_uint64), ("key_bytes", C.c_uint64), ("reserved", C.c_uint64)]

    def as_tuple(self):
        return (self.n, self.undecided, self.key_bytes)


class seb_values_sizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("found", C.c_uint64), ("val_bytes", C.c_uint64), ("reserved", C.c_uint64)]

    def as_tuple(self):
        return (self.n, self.found, self.val_bytes)


class seb_blockids_sizes(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("resident", C.c_uint64), ("misses", C.c_uint64), ("uniq", C.c_uint64),
                ("bad", C.c_uint64), ("reserved", C.c_uint64)]

    def as_tuple(self):
        return (self.cells, self.resident, self.misses, self.uniq, self.bad)


class seb_segcompact_sizes(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("live_in", C.c_uint64), ("distinct", C.c_uint64), ("survivors", C.c_uint64),
                ("tombstoned", C.c_uint64), ("shadowed", C.c_uint64), ("image_bytes", C.c_uint64), ("reserved", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class seb_bt_meta(C.Structure):
    _fields_ = [("root", C.c_uint32), ("header_pages", C.c_uint32), ("free_list", C.c_uint32), ("num_pages", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class seb_bt_stats(C.Structure):
    _fields_ = [("leaves", C.c_uint64), ("internals", C.c_uint64), ("bad", C.c_uint64), ("reach_leaves", C.c_uint64),
                ("reach_internals", C.c_uint64), ("reach_bad", C.c_uint64), ("keys", C.c_uint64), ("depth", C.c_uint32),
                ("uniform", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class seb_bt_dir_info(C.Structure):
    _fields_ = [("leaves", C.c_uint64), ("keys", C.c_uint64), ("depth", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class seb_bt_scan_sizes(C.Structure):
    _fields_ = [("ranges", C.c_uint64), ("entries", C.c_uint64), ("key_bytes", C.c_uint64), ("val_bytes", C.c_uint64)]

    def as_tuple(self):
        return (self.ranges, self.entries, self.key_bytes, self.val_bytes)


class seb_run(C.Structure):
    """A sorted run in the builder's input layout (the memtable lookup): host or device pointers per entry point."""
    _fields_ = [("keys", C.c_void_p), ("key_bytes", C.c_uint64), ("key_off", C.c_void_p), ("val_off", C.c_void_p),
                ("deleted", C.c_void_p), ("seq", C.c_void_p), ("n", C.c_uint64)]


class seb_filter_ref(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("num_bits", C.c_uint64), ("num_hashes", C.c_uint32),
                ("reserved", C.c_uint32)]


_lib = None
_vp = C.c_void_p
_u64 = C.c_uint64
_u32 = C.c_uint32
_i = C.c_int

_SIGS = {
    "seb_params": (_i, [C.c_int64, C.c_double, C.POINTER(_u64), C.POINTER(_u32)]),
    "seb_num_bytes": (_u64, [_u64]),
    "seb_words_bytes": (_u64, [_u64]),
    "seb_abi_version": (_i, []),
    "seb_last_error": (C.c_char_p, []),
    "seb_set_option": (_i, [C.c_char_p, C.c_int64]),
    "seb_get_option": (_i, [C.c_char_p, C.POINTER(C.c_int64)]),
    "seb_dev_build_workspace_size": (_u64, [_u64, _u64, _u32]),
    "seb_dev_build_ws": (_i, [C.POINTER(seb_keys), _vp, _u64, _u32, _vp, _u64, _vp]),
    "seb_device_check": (_i, [_i]),
    "seb_dev_clear": (_i, [_vp, _u64, _vp]),
    "seb_dev_build": (_i, [C.POINTER(seb_keys), _vp, _u64, _u32, _vp]),
    "seb_dev_build_fresh": (_i, [C.POINTER(seb_keys), _vp, _u64, _u32, _vp]),
    "seb_dev_probe": (_i, [C.POINTER(seb_keys), _vp, _u64, _u32, _vp, _vp]),
    "seb_dev_probe_multi": (_i, [C.POINTER(seb_keys), C.POINTER(seb_filter_ref), _u32, _vp, _u32, _vp]),
    "seb_dev_build_many": (_i, [C.POINTER(seb_keys), C.POINTER(_u64), C.POINTER(seb_filter_ref), _u32, _vp]),
    "seb_dev_alloc": (_i, [C.POINTER(_vp), _u64]),
    "seb_dev_free": (_i, [_vp]),
    "seb_host_alloc": (_i, [C.POINTER(_vp), _u64]),
    "seb_host_free": (_i, [_vp]),
    "seb_memcpy_h2d": (_i, [_vp, _vp, _u64, _vp]),
    "seb_memcpy_d2h": (_i, [_vp, _vp, _u64, _vp]),
    "seb_stream_sync": (_i, [_vp]),
    "seb_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "seb_ctx_destroy": (None, [_vp]),
    "seb_build": (_i, [_vp, C.POINTER(seb_keys), _vp, _u64, _u32, _u32]),
    "seb_probe": (_i, [_vp, C.POINTER(seb_keys), _vp, _u64, _u32, _vp]),
    "seb_probe_multi": (_i, [_vp, C.POINTER(seb_keys), C.POINTER(seb_filter_ref), _u32, _vp]),
    "seb_filter_new": (_vp, [C.c_int64, C.c_double]),
    "seb_filter_free": (None, [_vp]),
    "seb_filter_add": (_i, [_vp, _vp, _u64]),
    "seb_filter_add_batch": (_i, [_vp, C.POINTER(seb_keys)]),
    "seb_filter_may_contain": (_i, [_vp, _vp, _u64]),
    "seb_filter_may_contain_batch": (_i, [_vp, C.POINTER(seb_keys), _vp]),
    "seb_filter_encoded_size": (_u64, [_vp]),
    "seb_filter_encode": (_i, [_vp, _vp, _u64]),
    "seb_filter_decode": (_vp, [_vp, _u64]),
    "seb_filter_num_bits": (_u64, [_vp]),
    "seb_filter_num_hashes": (_u32, [_vp]),
    "seb_filter_pending": (_u64, [_vp]),
    "seb_filter_flush": (_i, [_vp]),
    "seb_fallback_count": (_u64, []),
    "seb_multiget_order_fallbacks": (_u64, []),
    "seb_registry_new": (_vp, [_i]),
    "seb_registry_free": (None, [_vp]),
    "seb_registry_put": (_i, [_vp, _u64, _i, _vp, _u64, _vp, _u64, _vp, _u64]),
    "seb_registry_remove": (_i, [_vp, _u64]),
    "seb_registry_slots": (_i, [_vp, C.POINTER(_u64), C.POINTER(C.c_int32), _u32]),
    "seb_registry_multiget": (_i, [_vp, C.POINTER(seb_keys), _vp]),
    "seb_registry_multiget_dev": (_i, [_vp, C.POINTER(seb_keys), _vp, _vp]),
    "seb_registry_max_candidates": (_i, [_vp]),
    "seb_registry_multiget_list": (_i, [_vp, C.POINTER(seb_keys), _vp, _u32]),
    "seb_registry_multiget_list_dev": (_i, [_vp, C.POINTER(seb_keys), _vp, _u32, _vp]),
    "seb_registry_multiget_files": (_i, [_vp, C.POINTER(seb_keys), _vp, _u32, C.POINTER(_u32)]),
    "seb_index_scan": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "seb_registry_put_index": (_i, [_vp, _u64, _vp, _u64]),
    "seb_registry_index_entries": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "seb_registry_locate_dev": (_i, [_vp, C.POINTER(seb_keys), _vp, _u32, _vp, _vp]),
    "seb_registry_locate": (_i, [_vp, C.POINTER(seb_keys), _vp, _u32, _vp]),
    "seb_registry_multiget_blocks": (_i, [_vp, C.POINTER(seb_keys), _vp, _vp, _u32, C.POINTER(_u32)]),
    "seb_block_search": (_i, [_vp, _u64, _vp, _u64, C.POINTER(_u32)]),
    "seb_dev_search_blocks": (_i, [C.POINTER(seb_keys), _vp, _u32, _vp, _vp, _u32, _vp, _vp]),
    "seb_dev_resolve_rows": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    "seb_search_blocks": (_i, [_vp, C.POINTER(seb_keys), _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "seb_blocks_dedup": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "seb_block_ids": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u64, C.POINTER(seb_blockids_sizes)]),
    "seb_dev_block_ids_resident": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _vp]),
    "seb_dev_block_ids_workspace_size": (_u64, [_u64, _u64]),
    "seb_dev_block_ids_plan": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _u64, _vp, _u64, C.POINTER(seb_blockids_sizes), _vp]),
    "seb_dev_block_ids_emit": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _u64, _u32, C.POINTER(seb_blockids_sizes), _vp, _vp,
                                    _vp, _vp, _vp]),
    "seb_sst_plan": (_i, [C.POINTER(seb_keys), _vp, C.POINTER(seb_sst_sizes)]),
    "seb_sst_encode": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(seb_sst_sizes)]),
    "seb_sst_footer": (_i, [_u64, _u64, _u64, _vp]),
    "seb_dev_sst_workspace_size": (_u64, [_u64, _u32]),
    "seb_dev_sst_plan": (_i, [C.POINTER(seb_keys), _vp, C.POINTER(_u64), _u32, _vp, _u64, C.POINTER(seb_sst_sizes), _vp]),
    "seb_dev_sst_encode": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, C.POINTER(_u64), _u32, C.POINTER(seb_sst_sizes), _vp,
                                _u64, _vp, _vp, _vp, _vp, _vp]),
    "seb_sst_build": (_i, [_vp, C.POINTER(seb_keys), _vp, _vp, _vp, C.c_int64, _vp, _u64, C.POINTER(_u64)]),
    "seb_block_entries": (_i, [_vp, _u64, _vp, _u32, C.POINTER(_u32)]),
    "seb_merge_plan": (_i, [_vp, _vp, _vp, _u32, _u32, C.POINTER(seb_merge_sizes)]),
    "seb_merge_emit": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, C.POINTER(seb_merge_sizes)]),
    "seb_dev_merge_count": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "seb_dev_merge_workspace_size": (_u64, [_u64, _u32, _u32]),
    "seb_dev_merge_plan": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u64, C.POINTER(seb_merge_sizes), _vp]),
    "seb_dev_merge_emit": (_i, [_vp, C.POINTER(seb_merge_sizes), _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_merge": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64,
                       C.POINTER(seb_merge_sizes)]),
    "seb_wal_replay_plan": (_i, [_vp, _vp, _u64, C.POINTER(seb_replay_sizes)]),
    "seb_wal_replay_emit": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(seb_replay_sizes)]),
    "seb_dev_wal_replay_workspace_size": (_u64, [_u64]),
    "seb_dev_wal_replay_plan": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(seb_replay_sizes), _vp]),
    "seb_dev_wal_replay_emit": (_i, [_vp, _vp, C.POINTER(seb_replay_sizes), _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_wal_recover": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64,
                             C.POINTER(seb_replay_sizes)]),
    "seb_runs_search": (_i, [C.POINTER(seb_keys), C.POINTER(seb_run), _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_get_join": (_i, [_vp, _vp, _u64, _vp, _vp]),
    "seb_dev_run_index_size": (_u64, [_u64]),
    "seb_dev_run_index": (_i, [C.POINTER(seb_run), _vp, _u64, _vp]),
    "seb_dev_runs_search": (_i, [C.POINTER(seb_keys), C.POINTER(seb_run), C.POINTER(_vp), _u32, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp]),
    "seb_dev_get_join": (_i, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "seb_get_compact": (_i, [C.POINTER(seb_keys), _vp, C.POINTER(seb_compact_sizes), _vp, _u64, _vp, _vp, _u64]),
    "seb_get_join_rows": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_dev_get_compact_workspace_size": (_u64, [_u64]),
    "seb_dev_get_compact_plan": (_i, [C.POINTER(seb_keys), _vp, _vp, _u64, C.POINTER(seb_compact_sizes), _vp]),
    "seb_dev_get_compact_emit": (_i, [C.POINTER(seb_keys), _vp, C.POINTER(seb_compact_sizes), _vp, _vp, _vp, _vp, _vp]),
    "seb_dev_get_join_rows": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_get_values": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_u64), _u32, _vp, _u64,
                            C.POINTER(seb_values_sizes), _vp, _vp, _u64]),
    "seb_dev_get_values_workspace_size": (_u64, [_u64]),
    "seb_dev_get_values_plan": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_u64), _u32, _vp, _u64, _vp,
                                     _u64, C.POINTER(seb_values_sizes), _vp]),
    "seb_dev_get_values_emit": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_u64), _u32, _vp, _u64,
                                     C.POINTER(seb_values_sizes), _vp, _vp, _vp, _vp]),
    "seb_memtable_get": (_i, [_vp, C.POINTER(seb_keys), C.POINTER(seb_run), _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_wal_frame_plan": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, C.POINTER(_u64)]),
    "seb_wal_frame_emit": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, _u64, _vp, _u64]),
    "seb_dev_wal_frame_plan": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, C.POINTER(_u64), _vp]),
    "seb_dev_wal_frame_emit": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "seb_run_size_delta": (_i, [C.POINTER(seb_run), C.POINTER(seb_run), _u32, C.POINTER(C.c_int64)]),
    "seb_dev_run_size_delta": (_i, [C.POINTER(seb_run), C.POINTER(seb_run), C.POINTER(_vp), _u32, _vp, _vp]),
    "seb_runs_fold_plan": (_i, [C.POINTER(seb_run), C.POINTER(_u64), _u32, C.POINTER(seb_fold_sizes)]),
    "seb_runs_fold_emit": (_i, [C.POINTER(seb_run), C.POINTER(_vp), C.POINTER(_u64), _u32, _vp, _vp, _vp, _vp, _vp, _vp,
                                C.POINTER(seb_fold_sizes)]),
    "seb_dev_runs_fold_workspace_size": (_u64, [_u64]),
    "seb_dev_runs_fold_plan": (_i, [C.POINTER(seb_run), C.POINTER(_vp), C.POINTER(_u64), _u32, _vp, _u64,
                                    C.POINTER(seb_fold_sizes), _vp]),
    "seb_dev_runs_fold_emit": (_i, [C.POINTER(seb_run), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), _u32,
                                    C.POINTER(seb_fold_sizes), _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_memtable_apply": (_i, [_vp, C.POINTER(seb_keys), _vp, _vp, _vp, _u64, C.POINTER(seb_run), _u32, _vp, _u64,
                                C.POINTER(_u64), _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(seb_replay_sizes),
                                C.POINTER(C.c_int64), C.POINTER(_u64)]),
    "seb_memtable_fold": (_i, [_vp, C.POINTER(seb_run), C.POINTER(_vp), C.POINTER(_u64), _u32, _vp, _u64, _vp, _vp, _u64,
                               _vp, _vp, _vp, _u64, C.POINTER(seb_fold_sizes)]),
    "seb_workspace_bytes": (_u64, []),
    "seb_dev_or_slices": (_i, [_vp, _u32, _u64, _vp, _vp]),
    "seb_workspace_release": (_i, []),
    "seb_dev_shard_route": (_i, [C.POINTER(seb_keys), _u32, _vp, _vp, _vp]),
    "seb_dev_shard_partition_workspace_size": (_u64, [_u64, _u32]),
    "seb_dev_shard_partition": (_i, [C.POINTER(seb_keys), _u32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "seb_dev_wal_crc": (_i, [_vp, _vp, _u64, _i, _vp, _vp, _vp]),
    "seb_wal_scan": (_i, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "seb_seg_scan": (_i, [_vp, _u64, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "seb_seg_verify": (_i, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "seb_hidx_lookup": (_i, [_vp, _u64, _vp, _vp, _u64, C.POINTER(seb_keys), _i, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "seb_dev_hidx_table_bytes": (_u64, [_u64]),
    "seb_dev_hidx_clear": (_i, [_vp, _u64, _vp]),
    "seb_dev_seg_verify": (_i, [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "seb_dev_hidx_insert": (_i, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp]),
    "seb_dev_hidx_count": (_i, [_vp, _u64, C.POINTER(_u64), C.POINTER(_u64), _vp]),
    "seb_dev_hidx_get": (_i, [_vp, _u64, _vp, _u64, C.POINTER(seb_keys), _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_hidx_recover": (_i, [_vp, C.POINTER(_vp), C.POINTER(_u64), _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp,
                              C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "seb_seg_frame_plan": (_i, [C.POINTER(seb_keys), _vp, _vp, _u64, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "seb_seg_frame_emit": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, _u64, _vp, _u64]),
    "seb_dev_seg_frame_plan": (_i, [C.POINTER(seb_keys), _vp, _vp, _u64, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64),
                                    _vp]),
    "seb_dev_seg_frame_emit": (_i, [C.POINTER(seb_keys), _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "seb_seg_compact": (_i, [_vp, _u64, _vp, _vp, _u64, _u64, _vp, _u64, _vp, _u64, C.POINTER(seb_segcompact_sizes)]),
    "seb_dev_seg_compact_workspace_size": (_u64, [_u64]),
    "seb_dev_seg_compact_plan": (_i, [_vp, _u64, _vp, _vp, _u64, _vp, _u64, C.POINTER(seb_segcompact_sizes), _vp]),
    "seb_dev_seg_compact_emit": (_i, [_vp, _u64, _vp, _u64, _u64, C.POINTER(seb_segcompact_sizes), _vp, _u64, _vp, _vp, _vp]),
    "seb_hidx_logical_size": (_i, [_vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)]),
    "seb_dev_hidx_logical_size": (_i, [_vp, _u64, _vp, _u64, C.POINTER(_u64), _vp]),
    "seb_hidx_compact": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _vp, _u64, _vp, _u64, _vp, _u64,
                              C.POINTER(seb_segcompact_sizes), _vp, _vp, C.POINTER(_u64)]),
    "seb_bt_open": (_i, [_vp, _u64, C.POINTER(seb_bt_meta)]),
    "seb_bt_check": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, _vp, C.POINTER(seb_bt_stats)]),
    "seb_bt_get": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), C.POINTER(seb_keys), _vp, _vp, _vp, _vp, _vp]),
    "seb_dev_bt_check": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, _vp, C.POINTER(seb_bt_stats), _vp]),
    "seb_dev_bt_get": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), C.POINTER(seb_keys), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_bt_load": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, C.POINTER(seb_bt_meta), C.POINTER(seb_bt_stats)]),
    "seb_bt_dir_bytes": (_u64, [_u32]),
    "seb_bt_dir_build": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, _vp, _vp, C.POINTER(seb_bt_dir_info)]),
    "seb_bt_scan": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, C.POINTER(seb_keys), C.POINTER(seb_keys), _u64, _vp, _vp,
                         _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(seb_bt_scan_sizes)]),
    "seb_dev_bt_dir_workspace_size": (_u64, [_u32]),
    "seb_dev_bt_dir_build": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, _vp, _vp, _vp, _u64, C.POINTER(seb_bt_dir_info), _vp]),
    "seb_dev_bt_scan_workspace_size": (_u64, [_u64]),
    "seb_dev_bt_scan_plan": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, C.POINTER(seb_keys), C.POINTER(seb_keys), _u64, _vp,
                                  _vp, _u64, C.POINTER(seb_bt_scan_sizes), _vp]),
    "seb_dev_bt_scan_cells": (_i, [_vp, _u64, C.POINTER(seb_bt_meta), _vp, C.POINTER(seb_bt_scan_sizes), _vp, _u64, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "seb_dev_pack_residues": (_i, [C.POINTER(seb_keys), _u64, _u32, _vp, _vp]),
    "seb_dev_probe_packed": (_i, [_vp, _u64, _vp, _u64, _u32, _vp, _vp]),
    "seb_dev_probe_emit_packed": (_i, [C.POINTER(seb_keys), _vp, _u64, _u32, _vp, _vp, _vp]),
    "seb_dev_probe_multi_packed": (_i, [_vp, _u64, C.POINTER(seb_filter_ref), _u32, _vp, _u32, _vp]),
    "seb_packed6_bytes": (_u64, [_u64]),
    "seb_dev_pack_residues6": (_i, [C.POINTER(seb_keys), _u64, _u32, _vp, _vp]),
    "seb_dev_probe_multi_packed6": (_i, [_vp, _u64, C.POINTER(seb_filter_ref), _u32, _vp, _u32, _vp]),
    "seb_timer_create": (_i, [C.POINTER(_vp)]),
    "seb_timer_record": (_i, [_vp, _vp]),
    "seb_timer_elapsed_ms": (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    "seb_timer_destroy": (_i, [_vp]),
}

WAL_CRC, WAL_SEAL, WAL_VERIFY = 0, 1, 2
NO_BLOCK = 2**64 - 1  # SEB_NO_BLOCK: no index entry <= the key, a padded cell, or a slot without a file
BLOCK_BYTES = 4096    # SEB_BLOCK_BYTES: a block pool slot (readBlock returns at most this many bytes)
NO_BLOCK_ID = 2**32 - 1  # SEB_NO_BLOCK_ID: a cell without a block to search
CELL_NONE, CELL_MISS, CELL_FOUND, CELL_TOMBSTONE, CELL_TRUNC = range(5)
GET_MISS, GET_FOUND, GET_ERROR = range(3)
MEM_NONE, MEM_FOUND, MEM_TOMBSTONE = range(3)  # seb_mem_status
MEM_MAX_RUNS = 8           # SEB_MEM_MAX_RUNS
MEM_NO_ENTRY = 2**32 - 1   # SEB_MEM_NO_ENTRY
BT_PAGE_BYTES, BT_MAX_DEPTH = 4096, 32               # SEB_BT_PAGE_BYTES, SEB_BT_MAX_DEPTH
BT_NO_PAGE, BT_NO_LEVEL = 2**32 - 1, 0xFF            # SEB_BT_NO_PAGE, SEB_BT_NO_LEVEL
BT_PAGE_BAD, BT_PAGE_INTERNAL, BT_PAGE_LEAF = range(3)  # seb_bt_page_kind


def build_library() -> str:
    """Compile libseb_bloom.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")], check=True)
    return LIB_PATH


def lib():
    """Load the HIP library; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SebError(-2, f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback exists)")
        try:  # share torch's HIP runtime when torch is in the process (same SONAME)
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().seb_last_error() or b"").decode()


def check(rc: int) -> int:
    if rc < 0:
        raise SebError(rc, last_error())
    return rc


def params(n: int, p: float) -> tuple[int, int]:
    m, k = _u64(), _u32()
    check(lib().seb_params(n, p, C.byref(m), C.byref(k)))
    return m.value, k.value


def num_bytes(m: int) -> int:
    return lib().seb_num_bytes(m)


def words_bytes(m: int) -> int:
    return lib().seb_words_bytes(m)


def set_option(name: str, value: int) -> None:
    """Tuning knob (build_algo, probe_phases, bucket_min_keys, grid_cap, ...); results never change."""
    check(lib().seb_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_int64()
    check(lib().seb_get_option(name.encode(), C.byref(v)))
    return v.value


class option:
    """Context manager: temporarily set a tuning knob."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)

    def __exit__(self, *exc):
        set_option(self.name, self.old)


def fallback_count() -> int:
    """Go-API-mirror builds / probes that ran on the host copy because the device path failed."""
    return int(lib().seb_fallback_count())


def device_check(device: int = 0) -> None:
    check(lib().seb_device_check(device))


# ------------------------------------------------------------------ key batches (host) ----

class HostKeys:
    """A host key batch: fixed-stride (n, L) uint8 array, or (data, offsets) variable-length."""

    def __init__(self, data: np.ndarray, offsets: np.ndarray | None = None):
        if offsets is None:
            arr = np.ascontiguousarray(data, dtype=np.uint8)
            if arr.ndim != 2:
                raise ValueError("fixed-length keys must be a 2-D (n, L) uint8 array")
            self.n, self.stride = arr.shape
            self.data = arr
            self.offsets = None
        else:
            self.data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
            self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            self.n = self.offsets.shape[0] - 1
            self.stride = 0
        self._s = seb_keys(self.data.ctypes.data if self.data.size else None,
                           self.offsets.ctypes.data if self.offsets is not None else None,
                           self.n, self.stride, 0)

    @property
    def ref(self):
        return C.byref(self._s)


def as_keys(keys) -> HostKeys:
    if isinstance(keys, HostKeys):
        return keys
    if isinstance(keys, tuple):
        return HostKeys(keys[0], keys[1])
    if isinstance(keys, (list,)):
        lens = np.array([len(k) for k in keys], dtype=np.uint64)
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        data = np.frombuffer(b"".join(keys), dtype=np.uint8) if len(keys) else np.zeros(0, np.uint8)
        return HostKeys(data, off)
    return HostKeys(keys)


# ------------------------------------------------------------------ host-buffer API ------

class Ctx:
    """seb_ctx: streams + scratch on one device; host-buffer build / probe (PCIe-inclusive)."""

    def __init__(self, device: int = 0):
        p = _vp()
        check(lib().seb_ctx_create(device, C.byref(p)))
        self._p = p

    def close(self):
        if self._p:
            lib().seb_ctx_destroy(self._p)
            self._p = None

    __del__ = close

    def build(self, keys, m: int, k: int, bits: np.ndarray | None = None) -> np.ndarray:
        kb = as_keys(keys)
        fresh = bits is None
        out = np.zeros(num_bytes(m), dtype=np.uint8) if fresh else bits
        check(lib().seb_build(self._p, kb.ref, out.ctypes.data, m, k, SEB_BUILD_FRESH if fresh else 0))
        return out

    def probe(self, keys, bits: np.ndarray, m: int, k: int) -> np.ndarray:
        kb = as_keys(keys)
        out = np.zeros(max(kb.n, 1), dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        check(lib().seb_probe(self._p, kb.ref, bits.ctypes.data, m, k, out.ctypes.data))
        return out[: kb.n]

    def search_blocks(self, keys, bid: np.ndarray, pool: np.ndarray, blen: np.ndarray, want_cells: bool = False):
        """Host form of the block search: bid is the (n, cap) u32 block ids, pool the blocks in
        4096-byte slots (host bytes), blen their lengths.  Returns (status u8, col u16, vloc u64,
        vlen u32) per key, plus the (n, cap) u32 cell results with want_cells."""
        kb = as_keys(keys)
        bid = np.ascontiguousarray(bid, dtype=np.uint32)
        if bid.ndim != 2 or bid.shape[0] != kb.n:
            raise ValueError("bid must be an (n, cap) array of u32 block ids")
        cap = bid.shape[1]
        pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
        blen = np.ascontiguousarray(blen, dtype=np.uint16)
        nb = blen.size
        if pool.size < nb * BLOCK_BYTES:
            raise ValueError(f"pool holds {pool.size} bytes, {nb} blocks need {nb * BLOCK_BYTES}")
        n1 = max(kb.n, 1)
        status, col = np.zeros(n1, np.uint8), np.zeros(n1, np.uint16)
        vloc, vlen = np.zeros(n1, np.uint64), np.zeros(n1, np.uint32)
        cells = np.zeros((n1, max(cap, 1)), np.uint32)
        src = bid if bid.size else np.zeros(1, np.uint32)
        check(lib().seb_search_blocks(self._p, kb.ref, src.ctypes.data, cap, pool.ctypes.data if nb else None,
                                      blen.ctypes.data if nb else None, nb, status.ctypes.data, col.ctypes.data,
                                      vloc.ctypes.data, vlen.ctypes.data, cells.ctypes.data if want_cells else None))
        out = (status[: kb.n], col[: kb.n], vloc[: kb.n], vlen[: kb.n])
        return out + (cells[: kb.n, :cap],) if want_cells else out

    def sst_build(self, keys, vals, val_off, deleted=None, expected_keys: int | None = None) -> bytes:
        """The complete SSTable file image SSTableBuilder leaves on disk for the run (keys, values
        vals[val_off[i]:val_off[i+1]], deleted bytes): data blocks, index, metadata, the Encode() of
        NewBloomFilter(expected_keys, 0.01) with every key added (default: the entry count), footer."""
        kb = _sst_keys(keys)
        vals, val_off, deleted = _sst_host_args(kb, vals, val_off, deleted)
        expected = kb.n if expected_keys is None else expected_keys
        need = _u64(0)
        out = np.zeros(1, np.uint8)
        while True:
            rc = lib().seb_sst_build(self._p, kb.ref, vals.ctypes.data, val_off.ctypes.data,
                                     deleted.ctypes.data if deleted is not None else None, expected, out.ctypes.data,
                                     out.size, C.byref(need))
            if rc == -4 and need.value > out.size:
                out = np.zeros(need.value, np.uint8)
                continue
            check(rc)
            return out[: need.value].tobytes()

    def merge(self, pool, blen, run_begin, flags: int = 0, caps: tuple[int, int, int] | None = None):
        """The compaction merge from host memory: run r = blocks [run_begin[r], run_begin[r+1]) of the pool
        (4096-byte slots, blen their lengths).  Returns (keys u8, key_off u64, vals u8, val_off u64,
        deleted u8, sizes) of the merged run; caps = (key bytes, value bytes, entries) fixes the output
        capacities instead of retrying with the sizes a too small first call reports."""
        pool, blen, rb, nb, nr = _merge_host_args(pool, blen, run_begin)
        sz = seb_merge_sizes()
        return _retry_with_sizes(lambda *run: lib().seb_merge(
            self._p, pool.ctypes.data if nb else None, blen.ctypes.data if nb else None, nb, rb.ctypes.data if nr else None, nr,
            flags, *run, C.byref(sz)), caps, sz, seq=False)

    def wal_recover(self, image, caps: tuple[int, int, int] | None = None):
        """WAL.ReadAll + recoverFromWAL from host memory: the log image is scanned, verified and replayed.
        Returns (keys u8, key_off u64, vals u8, val_off u64, deleted u8, seq u64, sizes) of the memtable's
        sorted run; caps = (key bytes, value bytes, entries) fixes the output capacities instead of retrying
        with the sizes a too small first call reports.  A record that fails its CRC: SebError (INVALID, "CRC
        mismatch (record R)"); otherwise a truncated tail: SebError (SHORT)."""
        img = _wal_image_arg(image)
        sz = seb_replay_sizes()
        return _retry_with_sizes(lambda *run: lib().seb_wal_recover(self._p, img.ctypes.data if img.size else None, img.size, *run,
                                                                    C.byref(sz)), caps, sz)

    def memtable_get(self, keys, runs):
        """LSM.Get's memtable steps from host memory: `runs` are host_run()s, the active memtable first.
        Returns (status u8, run u8, entry u32, vloc u64, vlen u32, seq u64) per key."""
        kb = as_keys(keys)
        arr = _run_array(runs)
        out = _memget_out(kb.n)
        check(lib().seb_memtable_get(self._p, kb.ref, arr, len(runs), *[o.ctypes.data for o in out]))
        return tuple(o[: kb.n] for o in out)

    def memtable_apply(self, keys, vals, val_off, deleted=None, first_seq: int = 1, runs=(), caps=None):
        """One write batch from host memory (LSM.Put / LSM.Delete per op, in order): ops as wal_frame takes them,
        `runs` the active memtable's existing host_run()s, newest first.  Returns (image u8, run, size_delta,
        sequence) with run = (keys u8, key_off u64, vals u8, val_off u64, deleted u8, seq u64, replay sizes) of the
        batch and sequence = lsm.sequence after it; caps = (image bytes, key bytes, value bytes, entries) fixes the
        capacities instead of retrying with the sizes a too small first call reports."""
        kb, va, vo, de = _ops_host_args(keys, vals, val_off, deleted)
        arr = _run_array(list(runs))
        sz, img_bytes, delta, seq_after = seb_replay_sizes(), _u64(0), C.c_int64(0), _u64(0)
        image, run = _retry_with_sizes(lambda image, ic, *run: lib().seb_memtable_apply(
            self._p, kb.ref, va.ctypes.data, vo.ctypes.data, None if de is None else de.ctypes.data, first_seq, arr, len(runs),
            image, ic, C.byref(img_bytes), *run, C.byref(sz), C.byref(delta), C.byref(seq_after)), caps, sz, image_bytes=img_bytes)
        return image, run, delta.value, seq_after.value

    def memtable_fold(self, runs, vals, caps=None):
        """Fold host_run()s (newest first; vals[r] = run r's value bytes) into the one run GetAllEntries() returns:
        (keys u8, key_off u64, vals u8, val_off u64, deleted u8, seq u64, fold sizes); caps = (key bytes, value
        bytes, entries)."""
        arr, vp, vb, keep = _fold_host_args(runs, vals)
        sz = seb_fold_sizes()
        return _retry_with_sizes(lambda *run: lib().seb_memtable_fold(self._p, arr, vp, vb, len(runs), *run, C.byref(sz)), caps, sz)

    def probe_multi(self, keys, filters: list[tuple[np.ndarray, int, int]]) -> np.ndarray:
        kb = as_keys(keys)
        keep = [np.ascontiguousarray(b, dtype=np.uint8) for b, _, _ in filters]
        refs = (seb_filter_ref * len(filters))(*[seb_filter_ref(b.ctypes.data, m, k, 0)
                                                  for b, (_, m, k) in zip(keep, filters)])
        out = np.zeros(max(kb.n, 1), dtype=np.uint64)
        check(lib().seb_probe_multi(self._p, kb.ref, refs, len(filters), out.ctypes.data))
        return out[: kb.n]


# ------------------------------------------------------------- Go API mirror (handles) ----

class BloomFilter:
    """lsm/bloom.go's BloomFilter, backed by an HBM-resident bit array in libseb_bloom."""

    def __init__(self, expected_keys: int | None = None, fpr: float = 0.01, *, _handle=None):
        if _handle is None:
            _handle = lib().seb_filter_new(expected_keys, fpr)
            if not _handle:
                raise SebError(-4, last_error())
        self._h = _handle

    @classmethod
    def decode(cls, data: bytes):
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        h = lib().seb_filter_decode(buf.ctypes.data, len(data))
        return cls(_handle=h) if h else None

    def close(self):
        if getattr(self, "_h", None):
            lib().seb_filter_free(self._h)
            self._h = None

    __del__ = close

    @property
    def num_bits(self) -> int:
        return lib().seb_filter_num_bits(self._h)

    @property
    def num_hashes(self) -> int:
        return lib().seb_filter_num_hashes(self._h)

    @property
    def pending(self) -> int:
        return lib().seb_filter_pending(self._h)

    def add(self, key: bytes) -> None:
        check(lib().seb_filter_add(self._h, key, len(key)))

    def add_batch(self, keys) -> None:
        kb = as_keys(keys)
        check(lib().seb_filter_add_batch(self._h, kb.ref))

    def may_contain(self, key: bytes) -> bool:
        return bool(check(lib().seb_filter_may_contain(self._h, key, len(key))))

    def may_contain_batch(self, keys) -> np.ndarray:
        kb = as_keys(keys)
        out = np.zeros(max(kb.n, 1), dtype=np.uint8)
        check(lib().seb_filter_may_contain_batch(self._h, kb.ref, out.ctypes.data))
        return out[: kb.n]

    def flush(self) -> None:
        check(lib().seb_filter_flush(self._h))

    def encode(self) -> bytes:
        size = lib().seb_filter_encoded_size(self._h)
        out = np.zeros(size, dtype=np.uint8)
        check(lib().seb_filter_encode(self._h, out.ctypes.data, size))
        return out.tobytes()


# ------------------------------------------- filter registry + batched LSM lookup (§8f) ----

class Registry:
    """Device-resident SSTable filter registry (seb_registry): put the bloom block of each open
    SSTable with its level and key range; multiget() returns, per key, a u64 mask of the slots
    LSM.Get would consult whose filter may contain the key (lsm/lsm.go:168-198)."""

    def __init__(self, device: int = 0):
        self._h = lib().seb_registry_new(device)
        if not self._h:
            raise SebError(-3, "seb_registry_new failed")

    def close(self):
        if getattr(self, "_h", None):
            lib().seb_registry_free(self._h)
            self._h = None

    __del__ = close

    def put(self, file_num: int, level: int, bloom_block: bytes, min_key: bytes, max_key: bytes) -> int:
        return check(lib().seb_registry_put(self._h, file_num, level, bloom_block, len(bloom_block), min_key,
                                            len(min_key), max_key, len(max_key)))

    def remove(self, file_num: int) -> None:
        check(lib().seb_registry_remove(self._h, file_num))

    MAX_FILES = 4096  # kRegMaxFiles (u16 slot ids)

    def slots(self) -> dict[int, tuple[int, int]]:
        cap = self.MAX_FILES
        fn = (_u64 * cap)()
        lv = (C.c_int32 * cap)()
        check(lib().seb_registry_slots(self._h, fn, lv, cap))
        return {s: (fn[s], lv[s]) for s in range(cap) if lv[s] >= 0}

    def max_candidates(self) -> int:
        """Longest Get walk: every L0 file plus one file per non-empty level 1..4."""
        return check(lib().seb_registry_max_candidates(self._h))

    def multiget_list(self, keys, cap: int | None = None) -> np.ndarray:
        """Per key, the slots of the files Get would consult whose filter may contain it, in
        visiting order, padded with 0xFFFF: an (n, cap) u16 array.  Any registry size."""
        kb = as_keys(keys)
        cap = max(self.max_candidates(), 1) if cap is None else cap
        out = np.zeros((max(kb.n, 1), cap), dtype=np.uint16)
        check(lib().seb_registry_multiget_list(self._h, kb.ref, out.ctypes.data, cap))
        return out[: kb.n]

    def multiget_list_dev(self, keys: "seb_keys", out, cap: int, stream=None) -> None:
        check(lib().seb_registry_multiget_list_dev(self._h, C.byref(keys), out.data_ptr(), cap, _stream(stream)))

    def multiget_files(self, keys, cap: int = 1) -> np.ndarray:
        """Per key, the file numbers Get would read whose filter may contain it, in visiting order,
        padded with 2^64-1: an (n, cap) u64 array from one atomic registry call (retried while the
        registry grows between sizing and lookup)."""
        kb = as_keys(keys)
        need = _u32()
        while True:
            out = np.zeros((max(kb.n, 1), cap), dtype=np.uint64)
            rc = lib().seb_registry_multiget_files(self._h, kb.ref, out.ctypes.data, cap, C.byref(need))
            if rc == -4 and need.value > cap:
                cap = need.value
                continue
            check(rc)
            return out[: kb.n]

    def multiget(self, keys) -> np.ndarray:
        kb = as_keys(keys)
        out = np.zeros(max(kb.n, 1), dtype=np.uint64)
        check(lib().seb_registry_multiget(self._h, kb.ref, out.ctypes.data))
        return out[: kb.n]

    def multiget_dev(self, keys: "seb_keys", out, stream=None) -> None:
        check(lib().seb_registry_multiget_dev(self._h, C.byref(keys), out.data_ptr(), _stream(stream)))

    def put_index(self, file_num: int, index_block: bytes) -> None:
        """Attach a registered file's encoded index block (the bytes OpenSSTable hands decodeIndex,
        lsm/sstable.go:105-119)."""
        check(lib().seb_registry_put_index(self._h, file_num, index_block, len(index_block)))

    def index_entries(self, file_num: int) -> int:
        n = _u64()
        check(lib().seb_registry_index_entries(self._h, file_num, C.byref(n)))
        return n.value

    def locate(self, keys, cand: np.ndarray) -> np.ndarray:
        """Per cell of multiget_list's (n, cap) u16 rows, the offset of the data block SSTable.Get
        would read in that file (lsm/sstable.go:210-222), NO_BLOCK for none: an (n, cap) u64 array."""
        kb = as_keys(keys)
        cand = np.ascontiguousarray(cand, dtype=np.uint16)
        if cand.ndim != 2 or cand.shape[0] != kb.n:
            raise ValueError("cand must be an (n, cap) array of u16 slots")
        cap = cand.shape[1]
        src = cand if cand.size else np.zeros(1, np.uint16)
        out = np.zeros((max(kb.n, 1), max(cap, 1)), dtype=np.uint64)
        check(lib().seb_registry_locate(self._h, kb.ref, src.ctypes.data, cap, out.ctypes.data))
        return out[: kb.n, :cap]

    def locate_dev(self, keys: "seb_keys", cand, blocks, cap: int, stream=None) -> None:
        """Device form: cand (n * cap u16) and blocks (n * cap u64) are device tensors; not synchronised."""
        cells = keys.n * cap
        if cand.numel() * cand.element_size() < 2 * cells:
            raise ValueError(f"cand holds {cand.numel() * cand.element_size()} bytes, n * cap u16 cells need {2 * cells}")
        if blocks.numel() * blocks.element_size() < 8 * cells:
            raise ValueError(f"blocks holds {blocks.numel() * blocks.element_size()} bytes, n * cap u64 cells need "
                             f"{8 * cells}")
        check(lib().seb_registry_locate_dev(self._h, C.byref(keys), cand.data_ptr(), cap, blocks.data_ptr(),
                                            _stream(stream)))

    def multiget_blocks(self, keys, cap: int = 1) -> tuple[np.ndarray, np.ndarray]:
        """The read plan: multiget_files' (n, cap) file numbers and, parallel to them, the block
        offset to read in each (NO_BLOCK: none), from one atomic registry call."""
        kb = as_keys(keys)
        need = _u32()
        while True:
            files = np.zeros((max(kb.n, 1), cap), dtype=np.uint64)
            blocks = np.zeros((max(kb.n, 1), cap), dtype=np.uint64)
            rc = lib().seb_registry_multiget_blocks(self._h, kb.ref, files.ctypes.data, blocks.ctypes.data, cap,
                                                    C.byref(need))
            if rc == -4 and need.value > cap:
                cap = need.value
                continue
            check(rc)
            return files[: kb.n], blocks[: kb.n]


# ------------------------------------------------- device-resident API (torch tensors) ----

def workspace_bytes() -> int:
    """Bytes of library-owned scratch (per device and stream) currently held."""
    return int(lib().seb_workspace_bytes())


def workspace_release() -> None:
    """Synchronise the streams that own library scratch and free it."""
    check(lib().seb_workspace_release())


def _stream(stream=None) -> int:
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


class Timer:
    """A HIP timing event without the system-scope completion fence (seb_timer_*): recording it
    between two kernels does not flush L2 the way torch.cuda.Event does."""

    def __init__(self):
        self._e = _vp()
        check(lib().seb_timer_create(C.byref(self._e)))

    def record(self, stream=None) -> None:
        check(lib().seb_timer_record(self._e, _stream(stream)))

    def elapsed_ms(self, end: "Timer") -> float:
        ms = C.c_float()
        check(lib().seb_timer_elapsed_ms(self._e, end._e, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "_e", None) and _lib is not None:
            _lib.seb_timer_destroy(self._e)
            self._e = None


def dev_keys(data, offsets=None, n: int | None = None, stride: int = 16) -> seb_keys:
    """seb_keys over device tensors (uint8 data; optional uint64/int64 offsets of n+1).
    The returned struct keeps the tensors alive (the C struct holds raw device pointers)."""
    if offsets is not None:
        kd = seb_keys(data.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, 0, 0)
    else:
        nn = n if n is not None else data.numel() // stride
        kd = seb_keys(data.data_ptr(), None, nn, stride, 0)
    kd._keep = (data, offsets)
    return kd


def dev_or_slices(slices, num_slices: int, out, stream=None) -> None:
    """out = OR of the num_slices equal slices of `slices` (int32 tensors; the sharded build's
    reduction after the all-to-all)."""
    sw = out.numel()
    if slices.numel() < num_slices * sw:
        raise ValueError("slices holds fewer than num_slices * out.numel() words")
    check(lib().seb_dev_or_slices(slices.data_ptr(), num_slices, sw, out.data_ptr(), _stream(stream)))


def dev_clear(words, m: int, stream=None) -> None:
    check(lib().seb_dev_clear(words.data_ptr(), m, _stream(stream)))


def dev_build(keys: seb_keys, words, m: int, k: int, stream=None) -> None:
    check(lib().seb_dev_build(C.byref(keys), words.data_ptr(), m, k, _stream(stream)))


def dev_build_fresh(keys: seb_keys, words, m: int, k: int, stream=None) -> None:
    """A new filter from the keys: `words` need not be cleared (every word is written)."""
    check(lib().seb_dev_build_fresh(C.byref(keys), words.data_ptr(), m, k, _stream(stream)))


def dev_build_workspace_size(n: int, m: int, k: int) -> int:
    return lib().seb_dev_build_workspace_size(n, m, k)


def dev_build_ws(keys: seb_keys, words, m: int, k: int, ws, stream=None) -> None:
    check(lib().seb_dev_build_ws(C.byref(keys), words.data_ptr(), m, k, ws.data_ptr() if ws is not None else None,
                                 ws.numel() * ws.element_size() if ws is not None else 0, _stream(stream)))


def dev_probe(keys: seb_keys, words, m: int, k: int, out, stream=None) -> None:
    check(lib().seb_dev_probe(C.byref(keys), words.data_ptr(), m, k, out.data_ptr(), _stream(stream)))


def dev_pack_residues(keys: seb_keys, m: int, k: int, packed, stream=None) -> None:
    """8-byte packed residues per key (k == 7, m < 2^29) for a batch shared by same-size filters."""
    check(lib().seb_dev_pack_residues(C.byref(keys), m, k, packed.data_ptr(), _stream(stream)))


def dev_probe_packed(packed, n: int, words, m: int, k: int, out, stream=None) -> None:
    check(lib().seb_dev_probe_packed(packed.data_ptr(), n, words.data_ptr(), m, k, out.data_ptr(), _stream(stream)))


def dev_probe_emit_packed(keys: seb_keys, words, m: int, k: int, out, packed, stream=None) -> None:
    """dev_probe that also writes the batch's packed residues (the broadcast root's probe)."""
    check(lib().seb_dev_probe_emit_packed(C.byref(keys), words.data_ptr(), m, k, out.data_ptr(), packed.data_ptr(),
                                          _stream(stream)))


def dev_probe_multi_packed(packed, n: int, filters: list[tuple[object, int, int]], mask, stream=None) -> None:
    """dev_probe_multi over packed residues (filters of one (m, k); k == 7, m < 2^29)."""
    refs = (seb_filter_ref * len(filters))(*[seb_filter_ref(w.data_ptr(), m, k, 0) for w, m, k in filters])
    check(lib().seb_dev_probe_multi_packed(packed.data_ptr(), n, refs, len(filters), mask.data_ptr(),
                                           mask.element_size(), _stream(stream)))


PACK6_BITS = 21      # narrow packed residues: m < 2^21 (include/seb_bloom.h)
PACK6_BLOCK = 384    # bytes per 64-key block (64 u32 low words + 64 u16 high halves)


def packed6_bytes(n: int) -> int:
    """Bytes of an n-key batch of 6-byte packed residues (whole 64-key blocks)."""
    return -(-n // 64) * PACK6_BLOCK


def pack6_supported(m: int, k: int) -> bool:
    return k == 7 and 0 < m < (1 << PACK6_BITS)


def _check_packed6(packed6, n: int) -> None:
    have = packed6.numel() * packed6.element_size()
    if have < packed6_bytes(n):  # whole 64-key blocks: 6 * n bytes is short unless n % 64 == 0
        raise ValueError(f"packed6 holds {have} bytes, {n} keys need packed6_bytes(n) = {packed6_bytes(n)}")


def dev_pack_residues6(keys: seb_keys, m: int, k: int, packed6, stream=None) -> None:
    """6-byte packed residues per key in 64-key blocks (k == 7, m < 2^21): a quarter fewer bytes
    than dev_pack_residues for the batch a compaction-sized filter set shares."""
    _check_packed6(packed6, keys.n)
    check(lib().seb_dev_pack_residues6(C.byref(keys), m, k, packed6.data_ptr(), _stream(stream)))


def dev_probe_multi_packed6(packed6, n: int, filters: list[tuple[object, int, int]], mask, stream=None) -> None:
    """dev_probe_multi over 6-byte packed residues (filters of one (m, k); k == 7, m < 2^21)."""
    _check_packed6(packed6, n)
    refs = (seb_filter_ref * len(filters))(*[seb_filter_ref(w.data_ptr(), m, k, 0) for w, m, k in filters])
    check(lib().seb_dev_probe_multi_packed6(packed6.data_ptr(), n, refs, len(filters), mask.data_ptr(),
                                            mask.element_size(), _stream(stream)))


def dev_probe_multi(keys: seb_keys, filters: list[tuple[object, int, int]], mask, stream=None) -> None:
    refs = (seb_filter_ref * len(filters))(*[seb_filter_ref(w.data_ptr(), m, k, 0) for w, m, k in filters])
    check(lib().seb_dev_probe_multi(C.byref(keys), refs, len(filters), mask.data_ptr(), mask.element_size(),
                                    _stream(stream)))


def dev_build_many(keys: seb_keys, key_begin: list[int], filters: list[tuple[object, int, int]],
                   stream=None) -> None:
    kbeg = (_u64 * len(key_begin))(*key_begin)
    refs = (seb_filter_ref * len(filters))(*[seb_filter_ref(w.data_ptr(), m, k, 0) for w, m, k in filters])
    check(lib().seb_dev_build_many(C.byref(keys), kbeg, refs, len(filters), _stream(stream)))


def new_words(m: int, device="cuda"):
    """Zeroed device word array for an m-bit filter (torch uint32 view, 16-B padded)."""
    import torch
    return torch.zeros(max(words_bytes(m) // 4, 4), dtype=torch.int32, device=device)


def words_to_bits(words, m: int) -> np.ndarray:
    """First ceil(m/8) bytes of a device word array = the reference's bits slice."""
    return words.cpu().numpy().view(np.uint8)[: (m + 7) // 8].copy()


# ------------------------------------------------ shard routing + WAL checksums (§8(f) row 4)

def _ptr(t):
    return t.data_ptr() if t is not None else None


def dev_shard_route(keys: seb_keys, shard_bits: int, shard=None, hash=None, stream=None) -> None:
    """shard[i] = FNV-1a32(key i) & (2^bits - 1) (hashindex/shard.go:47-52); hash[i] = the hash."""
    check(lib().seb_dev_shard_route(C.byref(keys), shard_bits, _ptr(shard), _ptr(hash), _stream(stream)))


def dev_shard_partition_workspace_size(n: int, shard_bits: int) -> int:
    return lib().seb_dev_shard_partition_workspace_size(n, shard_bits)


def dev_shard_partition(keys: seb_keys, shard_bits: int, perm, shard_begin=None, shard=None, ws=None,
                        stream=None) -> None:
    """Stable partition by shard (hashindex/shard.go:104-122): perm grouped by shard, input order
    inside a shard; shard_begin (2^bits + 1 u64) delimits the groups."""
    import torch
    if ws is None:
        ws = torch.empty(max(dev_shard_partition_workspace_size(keys.n, shard_bits), 1), dtype=torch.uint8,
                         device=perm.device)
    check(lib().seb_dev_shard_partition(C.byref(keys), shard_bits, _ptr(perm), _ptr(shard_begin), _ptr(shard),
                                        ws.data_ptr(), ws.numel(), _stream(stream)))


def dev_wal_crc(data, rec_off, mode: int = WAL_CRC, crc=None, ok=None, stream=None) -> None:
    """CRC32-IEEE of WAL records data[rec_off[i]+4, rec_off[i+1]) (lsm/wal.go:59); SEAL stores it,
    VERIFY sets ok[i] (framing + stored CRC, lsm/wal.go:123-133)."""
    check(lib().seb_dev_wal_crc(data.data_ptr(), rec_off.data_ptr(), rec_off.numel() - 1, mode, _ptr(crc), _ptr(ok),
                                _stream(stream)))


# ------------------------------- batched data-block search (SSTable.Get's last step, lsm/sstable.go:242-290)

def cell_unpack(cell) -> tuple:
    """(status, voff, vlen) of a u32 cell result (status << 28 | voff << 13 | vlen); arrays give arrays."""
    c = np.asarray(cell, dtype=np.uint32) if isinstance(cell, np.ndarray) else int(cell)
    return c >> 28, (c >> 13) & 0x1FFF, c & 0x1FFF


def block_search(block: bytes, key: bytes) -> int:
    """searchBlock's walk on the host for one block image (at most 4096 bytes) and one key: the u32
    cell result.  "block truncated" is the status CELL_TRUNC, not an error."""
    cell = _u32(0)
    check(lib().seb_block_search(bytes(block), len(block), bytes(key), len(key), C.byref(cell)))
    return cell.value


def blocks_dedup(files: np.ndarray, blocks: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """multiget_blocks' parallel (file, block offset) arrays into the read list: (bid, uniq_files,
    uniq_blocks) with each distinct pair once in first-appearance order and bid (u32, the shape of
    `files`) its position per cell, NO_BLOCK_ID where the block is NO_BLOCK."""
    files = np.ascontiguousarray(files, dtype=np.uint64)
    blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
    if files.shape != blocks.shape:
        raise ValueError("files and blocks must have one shape")
    cells = files.size
    bid = np.zeros(max(cells, 1), np.uint32)
    need = _u64(0)
    cap = max(min(cells, 1024), 1)
    while True:
        uf, ub = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        rc = lib().seb_blocks_dedup(files.ctypes.data if cells else None, blocks.ctypes.data if cells else None, cells,
                                    bid.ctypes.data, uf.ctypes.data, ub.ctypes.data, cap, C.byref(need))
        if rc == -4 and need.value > cap:
            cap = need.value
            continue
        check(rc)
        return bid[:cells].reshape(files.shape), uf[: need.value], ub[: need.value]


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def dev_search_blocks(keys: seb_keys, bid, cap: int, pool, blen, cells, num_blocks: int | None = None,
                      stream=None) -> None:
    """Device form: cells[c] (n * cap u32) = the block search of pool block bid[c] (u32) for key
    c // cap; pool holds num_blocks (default: blen.numel()) slots of 4096 bytes, blen (u16) their
    lengths.  Not synchronised."""
    ncell = keys.n * cap
    nb = blen.numel() if num_blocks is None else num_blocks
    if blen.element_size() != 2 or blen.numel() < nb:
        raise ValueError(f"blen holds {blen.numel()} lengths of {blen.element_size()} bytes, {nb} blocks need {nb} u16")
    if _nbytes(bid) < 4 * ncell:
        raise ValueError(f"bid holds {_nbytes(bid)} bytes, n * cap u32 cells need {4 * ncell}")
    if _nbytes(cells) < 4 * ncell:
        raise ValueError(f"cells holds {_nbytes(cells)} bytes, n * cap u32 cells need {4 * ncell}")
    if _nbytes(pool) < BLOCK_BYTES * nb:
        raise ValueError(f"pool holds {_nbytes(pool)} bytes, {nb} blocks need {BLOCK_BYTES * nb}")
    check(lib().seb_dev_search_blocks(C.byref(keys), bid.data_ptr(), cap, pool.data_ptr(), blen.data_ptr(), nb,
                                      cells.data_ptr(), _stream(stream)))


def dev_resolve_rows(cells, bid, n: int, cap: int, status, col=None, vloc=None, vlen=None, stream=None) -> None:
    """Device form of LSM.Get's decision per row of cells: status (n u8), and optionally col (n u16),
    vloc (n u64: the value's byte offset in the pool) and vlen (n u32).  Not synchronised."""
    for name, t, size in (("cells", cells, 4 * n * cap), ("bid", bid, 4 * n * cap), ("status", status, n),
                          ("col", col, 2 * n), ("vloc", vloc, 8 * n), ("vlen", vlen, 4 * n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {n} keys x {cap} cells need {size}")
    check(lib().seb_dev_resolve_rows(cells.data_ptr(), bid.data_ptr(), n, cap, status.data_ptr(), _ptr(col), _ptr(vloc),
                                     _ptr(vlen), _stream(stream)))


def search_blocks(keys, bid: np.ndarray, pool: np.ndarray, blen: np.ndarray, want_cells: bool = False, device: int = 0):
    """Ctx.search_blocks on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.search_blocks(keys, bid, pool, blen, want_cells)
    finally:
        ctx.close()


# ------------------------------- batched SSTable builder (lsm/sstable_builder.go:42-135,185-290)

SST_FOOTER_BYTES = 28
SST_MAGIC = 0x5354424C
SST_TILE = 1024  # kSstTile: entries per tile of the device cut (tests place runs around it)


def _sst_keys(keys) -> HostKeys:
    kb = as_keys(keys)
    if kb.offsets is not None and kb.data.size == 0:  # a run of empty keys still needs a data pointer
        kb = HostKeys(np.zeros(1, np.uint8), kb.offsets)
    return kb


def _sst_host_args(kb: HostKeys, vals, val_off, deleted):
    vals = np.ascontiguousarray(vals, dtype=np.uint8).reshape(-1)
    if vals.size == 0:
        vals = np.zeros(1, np.uint8)
    val_off = np.ascontiguousarray(val_off, dtype=np.uint64)
    if val_off.shape != (kb.n + 1,):
        raise ValueError(f"val_off must hold n + 1 = {kb.n + 1} offsets")
    if deleted is not None:
        deleted = np.ascontiguousarray(deleted, dtype=np.uint8)
        if deleted.shape != (kb.n,):
            raise ValueError(f"deleted must hold n = {kb.n} bytes")
        if kb.n == 0:
            deleted = None
    return vals, val_off, deleted


def sst_plan(keys, val_off) -> tuple[int, int, int, int, int]:
    """The builder's cut on the host: (num_blocks, data_bytes, index_bytes, meta_bytes,
    oversize_entries) of one file."""
    kb = _sst_keys(keys)
    val_off = np.ascontiguousarray(val_off, dtype=np.uint64)
    if val_off.shape != (kb.n + 1,):
        raise ValueError(f"val_off must hold n + 1 = {kb.n + 1} offsets")
    sz = seb_sst_sizes()
    check(lib().seb_sst_plan(kb.ref, val_off.ctypes.data, C.byref(sz)))
    return sz.as_tuple()


def sst_encode(keys, vals, val_off, deleted=None) -> tuple[bytes, bytes, bytes]:
    """The host half: (data section, index block, metadata) of one file, oversized blocks included."""
    kb = _sst_keys(keys)
    vals, val_off, deleted = _sst_host_args(kb, vals, val_off, deleted)
    _, d, x, m, _ = sst_plan(kb, val_off)
    data, index, meta = np.zeros(max(d, 1), np.uint8), np.zeros(x, np.uint8), np.zeros(m, np.uint8)
    check(lib().seb_sst_encode(kb.ref, vals.ctypes.data, val_off.ctypes.data,
                               deleted.ctypes.data if deleted is not None else None, data.ctypes.data, d,
                               index.ctypes.data, x, meta.ctypes.data, m, None))
    return data[:d].tobytes(), index.tobytes(), meta.tobytes()


def sst_footer(index_offset: int, bloom_offset: int, metadata_offset: int) -> bytes:
    out = np.zeros(SST_FOOTER_BYTES, np.uint8)
    check(lib().seb_sst_footer(index_offset, bloom_offset, metadata_offset, out.ctypes.data))
    return out.tobytes()


def dev_sst_workspace_size(n: int, num_files: int) -> int:
    return lib().seb_dev_sst_workspace_size(n, num_files)


def dev_sst_plan(keys: seb_keys, val_off, file_begin: list[int], ws, stream=None) -> list[tuple[int, int, int, int, int]]:
    """Device form: the cut of every file (entries [file_begin[f], file_begin[f+1]) of the batch) into
    the workspace tensor `ws`; synchronises and returns each file's (num_blocks, data_bytes,
    index_bytes, meta_bytes, oversize_entries)."""
    nf = len(file_begin) - 1
    if _nbytes(val_off) < 8 * (keys.n + 1):
        raise ValueError(f"val_off holds {_nbytes(val_off)} bytes, n + 1 u64 offsets need {8 * (keys.n + 1)}")
    want = dev_sst_workspace_size(keys.n, max(nf, 0))
    if _nbytes(ws) < want:
        raise ValueError(f"workspace holds {_nbytes(ws)} bytes, dev_sst_workspace_size gives {want}")
    fb = (_u64 * (nf + 1))(*file_begin)
    sizes = (seb_sst_sizes * max(nf, 1))()
    check(lib().seb_dev_sst_plan(C.byref(keys), val_off.data_ptr(), fb, nf, ws.data_ptr(), _nbytes(ws), sizes,
                                 _stream(stream)))
    return [sizes[f].as_tuple() for f in range(nf)]


def dev_sst_encode(keys: seb_keys, vals, val_off, deleted, file_begin: list[int], sizes, ws, data, index, meta,
                   blen=None, stream=None) -> None:
    """Device form: writes the files' data sections back to back into `data` (block b at b * 4096),
    their true lengths into blen (u16, optional), the index blocks into `index` and the metadata into
    `meta`; `sizes` as dev_sst_plan returned them.  Not synchronised."""
    nf = len(file_begin) - 1
    if len(sizes) != nf:
        raise ValueError("one sizes tuple per file")
    blocks = sum(s[0] for s in sizes)
    for name, t, size in (("data", data, sum(s[1] for s in sizes)), ("index", index, sum(s[2] for s in sizes)),
                          ("meta", meta, sum(s[3] for s in sizes)), ("blen", blen, 2 * blocks),
                          ("val_off", val_off, 8 * (keys.n + 1)), ("deleted", deleted, keys.n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, the plan needs {size}")
    if blen is not None and blen.element_size() != 2:
        raise ValueError("blen must be a 16-bit tensor")
    fb = (_u64 * (nf + 1))(*file_begin)
    cs = (seb_sst_sizes * max(nf, 1))(*[seb_sst_sizes(*s) for s in sizes])
    check(lib().seb_dev_sst_encode(C.byref(keys), _ptr(vals), val_off.data_ptr(), _ptr(deleted), fb, nf, cs,
                                   ws.data_ptr(), _nbytes(ws), data.data_ptr(), _ptr(blen), index.data_ptr(),
                                   meta.data_ptr(), _stream(stream)))


def sst_build(keys, vals, val_off, deleted=None, expected_keys: int | None = None, device: int = 0) -> bytes:
    """Ctx.sst_build on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.sst_build(keys, vals, val_off, deleted, expected_keys)
    finally:
        ctx.close()


# ------------------------------- batched compaction merge (lsm/compaction.go:69-124,226-333)

MERGE_DROP_TOMBSTONES = 1  # SEB_MERGE_DROP_TOMBSTONES: targetLevel == 4
MERGE_MAX_RUNS = 1 << 20   # SEB_MERGE_MAX_RUNS
MERGE_TILE = 1024          # kMergeTile: records per tile of a merge pass, of the survivor scan and of the emit
MAX_BLOCK_ENTRIES = 454    # the most entries a 4096-byte block yields


def block_entries(block: bytes, cap: int = MAX_BLOCK_ENTRIES) -> np.ndarray:
    """loadBlock's walk on the host for one block image (at most 4096 bytes): the offsets (u16) of the
    entries' 9-byte headers.  More than cap entries: SebError (RANGE) whose .count is the number found."""
    off = np.zeros(max(cap, 1), np.uint16)
    count = _u32(0)
    rc = lib().seb_block_entries(bytes(block), len(block), off.ctypes.data, cap, C.byref(count))
    if rc < 0:
        err = SebError(rc, last_error())
        err.count = count.value
        raise err
    return off[: count.value].copy()


def _merge_host_args(pool, blen, run_begin):
    pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
    blen = np.ascontiguousarray(blen, dtype=np.uint16)
    rb = np.ascontiguousarray(run_begin, dtype=np.uint64)
    nb, nr = blen.size, max(rb.size - 1, 0)
    if pool.size < nb * BLOCK_BYTES:
        raise ValueError(f"pool holds {pool.size} bytes, {nb} blocks need {nb * BLOCK_BYTES}")
    if nr and int(rb[-1]) > nb:
        raise ValueError(f"run_begin ends at {int(rb[-1])}, blen holds {nb} blocks")
    return pool, blen, rb, nb, nr


def _run_out(key_bytes: int, val_bytes: int, entries: int, seq: bool = True):
    """A sorted run's output arrays: keys u8, key_off u64, vals u8, val_off u64, deleted u8 and, with seq, seq u64."""
    out = (np.zeros(max(key_bytes, 1), np.uint8), np.zeros(entries + 1, np.uint64), np.zeros(max(val_bytes, 1), np.uint8),
           np.zeros(entries + 1, np.uint64), np.zeros(max(entries, 1), np.uint8))
    return out + (np.zeros(max(entries, 1), np.uint64),) if seq else out


def _run_trim(out, sz, seq: bool = True):
    """_run_out's arrays cut to the sizes, and the sizes."""
    n = sz.entries_out
    run = (out[0][: sz.key_bytes], out[1][: n + 1], out[2][: sz.val_bytes], out[3][: n + 1], out[4][:n])
    return run + ((out[5][:n],) if seq else ()) + (sz.as_tuple(),)


def _retry_with_sizes(call, caps, sz, seq: bool = True, image_bytes=None):
    """A host-buffer form that returns a sorted run, called with output capacities caps = ([image bytes,] key bytes,
    value bytes, entries): call([image, its capacity,] the run's arrays and capacities in the forms' order) -> rc.
    Without caps a call that reports SEB_ERR_RANGE is repeated with the sizes it filled (sz, and image_bytes where the
    form returns an image); any other error is raised with the sizes attached.  Returns the trimmed run[, after the image]."""
    fixed = caps is not None
    caps = tuple(caps) if fixed else (0,) * (3 if image_bytes is None else 4)
    while True:
        kc, vc, ec = caps[-3:]
        out = _run_out(kc, vc, ec, seq)
        p = [a.ctypes.data for a in out]
        image = None if image_bytes is None else np.zeros(max(caps[0], 1), np.uint8)
        rc = call(*(() if image is None else (image.ctypes.data, caps[0])), p[0], kc, p[1], p[2], vc, p[3], *p[4:], ec)
        need = (() if image is None else (image_bytes.value,)) + (sz.key_bytes, sz.val_bytes, sz.entries_out)
        if rc == -4 and not fixed and any(n > c for n, c in zip(need, caps)):
            caps = need
            continue
        if rc < 0:  # SEB_ERR_RANGE fills the sizes: the exception carries them
            err = SebError(rc, last_error())
            err.sizes = sz.as_tuple()
            if image is not None:
                err.image_bytes = image_bytes.value
            raise err
        return _run_trim(out, sz, seq) if image is None else (image[: image_bytes.value], _run_trim(out, sz, seq))


def merge_plan(pool, blen, run_begin, flags: int = 0) -> tuple[int, int, int, int, int, int]:
    """The host half's plan: (entries_in, entries_out, key_bytes, val_bytes, shadowed, dropped) of the merge
    of the pool's runs.  A run that is not strictly increasing: SebError (INVALID) naming run and entry."""
    pool, blen, rb, nb, nr = _merge_host_args(pool, blen, run_begin)
    sz = seb_merge_sizes()
    check(lib().seb_merge_plan(pool.ctypes.data if nb else None, blen.ctypes.data if nb else None,
                               rb.ctypes.data if nr else None, nr, flags, C.byref(sz)))
    return sz.as_tuple()


def merge_emit(pool, blen, run_begin, flags: int = 0, sizes=None):
    """The host half: (keys u8, key_off u64, vals u8, val_off u64, deleted u8, sizes) of the merged run;
    sizes default to merge_plan's."""
    pool, blen, rb, nb, nr = _merge_host_args(pool, blen, run_begin)
    sz = seb_merge_sizes(*(merge_plan(pool, blen, rb, flags) if sizes is None else sizes))
    out = _run_out(sz.key_bytes, sz.val_bytes, sz.entries_out, seq=False)
    check(lib().seb_merge_emit(pool.ctypes.data if nb else None, blen.ctypes.data if nb else None,
                               rb.ctypes.data if nr else None, nr, flags, out[0].ctypes.data, out[1].ctypes.data,
                               out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data, C.byref(sz)))
    return _run_trim(out, sz, seq=False)


def _run_begin(run_begin):
    rb = [int(x) for x in run_begin]
    return rb, max(len(rb) - 1, 0), (_u64 * max(len(rb), 1))(*rb)


def dev_merge_count(pool, blen, run_begin, block_entries, stream=None) -> list[int]:
    """Device form: block_entries (u16 tensor, one per block) = each block's entry count; synchronises and
    returns each run's entry count."""
    rb, nr, crb = _run_begin(run_begin)
    nb = rb[-1] if rb else 0
    for name, t, size in (("pool", pool, BLOCK_BYTES * nb), ("blen", blen, 2 * nb), ("block_entries", block_entries, 2 * nb)):
        if nb and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {nb} blocks need {size}")
    runs = (_u64 * max(nr, 1))()
    check(lib().seb_dev_merge_count(_ptr(pool) if nb else None, _ptr(blen) if nb else None, nb, crb if nr else None, nr,
                                    _ptr(block_entries) if nb else None, runs, _stream(stream)))
    return [runs[r] for r in range(nr)]


def dev_merge_workspace_size(entries: int, num_blocks: int, num_runs: int) -> int:
    return lib().seb_dev_merge_workspace_size(entries, num_blocks, num_runs)


def dev_merge_plan(pool, blen, run_begin, block_entries, ws, flags: int = 0, ws_bytes: int | None = None,
                   stream=None) -> tuple[int, int, int, int, int, int]:
    """Device form: decode, order check, merge and survivor scan into the workspace tensor `ws`
    (dev_merge_workspace_size bytes); synchronises and returns the sizes."""
    rb, nr, crb = _run_begin(run_begin)
    nb = rb[-1] if rb else 0
    sz = seb_merge_sizes()
    check(lib().seb_dev_merge_plan(_ptr(pool) if nb else None, _ptr(blen) if nb else None, nb, crb if nr else None, nr,
                                   _ptr(block_entries) if nb else None, flags, _ptr(ws),
                                   (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes, C.byref(sz),
                                   _stream(stream)))
    return sz.as_tuple()


def dev_merge_emit(pool, sizes, ws, keys, key_off, vals, val_off, deleted, stream=None) -> None:
    """Device form: writes the merged run (sizes as dev_merge_plan returned them): keys / vals (u8), key_off /
    val_off (entries_out + 1 u64 each), deleted (entries_out u8).  Not synchronised."""
    sz = seb_merge_sizes(*sizes)
    for name, t, size in (("keys", keys, sz.key_bytes), ("vals", vals, sz.val_bytes), ("deleted", deleted, sz.entries_out),
                          ("key_off", key_off, 8 * (sz.entries_out + 1)), ("val_off", val_off, 8 * (sz.entries_out + 1))):
        if (t is None and size) or (t is not None and _nbytes(t) < size):
            raise ValueError(f"{name} holds {0 if t is None else _nbytes(t)} bytes, the plan needs {size}")
    check(lib().seb_dev_merge_emit(_ptr(pool), C.byref(sz), _ptr(ws), _nbytes(ws) if ws is not None else 0, _ptr(keys),
                                   _ptr(key_off), _ptr(vals), _ptr(val_off), _ptr(deleted), _stream(stream)))


def merge(pool, blen, run_begin, flags: int = 0, caps=None, device: int = 0):
    """Ctx.merge on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.merge(pool, blen, run_begin, flags, caps)
    finally:
        ctx.close()


# ------------------------------- WAL replay (lsm/lsm.go:273-298 over lsm/memtable.go:34-93,129-137)

def _wal_image_arg(image) -> np.ndarray:
    if isinstance(image, (bytes, bytearray, memoryview)):
        return np.frombuffer(image, np.uint8)
    return np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)


def _replay_host_args(image, rec_off):
    img = _wal_image_arg(image)
    off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    return img, off, max(off.size - 1, 0)


def wal_replay_plan(image, rec_off) -> tuple[int, int, int, int, int, int, int, int]:
    """The host half's plan: (records_in, entries_out, key_bytes, val_bytes, overwritten, tombstones,
    max_sequence, memtable_size) of the replay of records [rec_off[i], rec_off[i+1]) of the image.  A record
    that is not framed, or offsets that decrease: SebError (INVALID) naming the record."""
    img, off, n = _replay_host_args(image, rec_off)
    sz = seb_replay_sizes()
    check(lib().seb_wal_replay_plan(img.ctypes.data if n else None, off.ctypes.data if n else None, n, C.byref(sz)))
    return sz.as_tuple()


def wal_replay_emit(image, rec_off, sizes=None):
    """The host half: (keys u8, key_off u64, vals u8, val_off u64, deleted u8, seq u64, sizes) of the memtable's
    sorted run; sizes default to wal_replay_plan's."""
    img, off, n = _replay_host_args(image, rec_off)
    sz = seb_replay_sizes(*(wal_replay_plan(img, off) if sizes is None else sizes))
    out = _run_out(sz.key_bytes, sz.val_bytes, sz.entries_out)
    check(lib().seb_wal_replay_emit(img.ctypes.data if n else None, off.ctypes.data if n else None, n, out[0].ctypes.data,
                                    out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data,
                                    out[5].ctypes.data, C.byref(sz)))
    return _run_trim(out, sz)


def dev_wal_replay_workspace_size(n: int) -> int:
    return lib().seb_dev_wal_replay_workspace_size(n)


def dev_wal_replay_plan(data, rec_off, ws, ws_bytes: int | None = None, stream=None):
    """Device form: data (u8 tensor or view, any alignment) and rec_off (n + 1 offsets, a 64-bit tensor) on the
    device; checks, decodes and sorts the records and marks the survivors into the workspace tensor `ws`
    (dev_wal_replay_workspace_size bytes); synchronises and returns the sizes."""
    n = max(rec_off.numel() - 1, 0) if rec_off is not None else 0
    sz = seb_replay_sizes()
    check(lib().seb_dev_wal_replay_plan(_ptr(data) if n else None, _ptr(rec_off) if n else None, n, _ptr(ws),
                                        (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                        C.byref(sz), _stream(stream)))
    return sz.as_tuple()


def dev_wal_replay_emit(data, rec_off, sizes, ws, keys, key_off, vals, val_off, deleted, seq=None, stream=None) -> None:
    """Device form: writes the run (sizes as dev_wal_replay_plan returned them): keys / vals (u8), key_off /
    val_off (entries_out + 1 u64 each), deleted (entries_out u8), seq (entries_out u64, optional).  Not
    synchronised."""
    sz = seb_replay_sizes(*sizes)
    for name, t, size in (("keys", keys, sz.key_bytes), ("vals", vals, sz.val_bytes), ("deleted", deleted, sz.entries_out),
                          ("key_off", key_off, 8 * (sz.entries_out + 1)), ("val_off", val_off, 8 * (sz.entries_out + 1)),
                          ("seq", seq, 8 * sz.entries_out if seq is not None else 0)):
        if (t is None and size) or (t is not None and _nbytes(t) < size):
            raise ValueError(f"{name} holds {0 if t is None else _nbytes(t)} bytes, the plan needs {size}")
    if sz.records_in and (rec_off is None or rec_off.numel() < sz.records_in + 1):
        raise ValueError(f"rec_off holds fewer than {sz.records_in + 1} offsets")
    check(lib().seb_dev_wal_replay_emit(_ptr(data), _ptr(rec_off), C.byref(sz), _ptr(ws), _nbytes(ws) if ws is not None else 0,
                                        _ptr(keys), _ptr(key_off), _ptr(vals), _ptr(val_off), _ptr(deleted), _ptr(seq),
                                        _stream(stream)))


def wal_recover(image, caps=None, device: int = 0):
    """Ctx.wal_recover on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.wal_recover(image, caps)
    finally:
        ctx.close()


# ------------------------------- batched memtable lookup (lsm/lsm.go:144-166 over lsm/memtable.go:95-112)

def host_run(keys, key_off, val_off, deleted=None, seq=None) -> seb_run:
    """seb_run over host arrays (numpy; keys may be bytes): n = len(key_off) - 1, key_bytes = len(keys).  No
    array is copied unless its dtype or layout has to change; the struct keeps them alive."""
    kb = _wal_image_arg(keys)
    ko = np.ascontiguousarray(key_off, dtype=np.uint64)
    vo = np.ascontiguousarray(val_off, dtype=np.uint64)
    if ko.size != vo.size:
        raise ValueError("key_off and val_off must hold n + 1 offsets each")
    n = max(ko.size - 1, 0)
    de = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
    sq = None if seq is None else np.ascontiguousarray(seq, dtype=np.uint64)
    for name, a in (("deleted", de), ("seq", sq)):
        if a is not None and a.size < n:
            raise ValueError(f"{name} holds {a.size} entries, the run has {n}")
    r = seb_run(kb.ctypes.data if kb.size else None, kb.size, ko.ctypes.data if ko.size else None,
                vo.ctypes.data if vo.size else None, de.ctypes.data if de is not None and n else None,
                sq.ctypes.data if sq is not None and n else None, n)
    r._keep = (kb, ko, vo, de, sq)
    return r


def dev_run(keys, key_off, val_off, deleted=None, seq=None, n: int | None = None, key_bytes: int | None = None) -> seb_run:
    """seb_run over device tensors (u8 keys and deleted at any alignment; 64-bit key_off, val_off and seq); n
    defaults to key_off.numel() - 1 and key_bytes to the bytes `keys` holds.  The struct keeps the tensors alive."""
    nn = (key_off.numel() - 1 if key_off is not None else 0) if n is None else n
    for name, t, size in (("key_off", key_off, 8 * (nn + 1)), ("val_off", val_off, 8 * (nn + 1)), ("deleted", deleted, nn),
                          ("seq", seq, 8 * nn)):
        if nn and t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {nn} entries need {size}")
    kbytes = (_nbytes(keys) if keys is not None else 0) if key_bytes is None else key_bytes
    r = seb_run(_ptr(keys), kbytes, _ptr(key_off), _ptr(val_off), _ptr(deleted), _ptr(seq), nn)
    r._keep = (keys, key_off, val_off, deleted, seq)
    return r


def _run_array(runs):
    arr = (seb_run * max(len(runs), 1))(*runs)
    arr._keep = list(runs)
    return arr


def _memget_out(n: int):
    n1 = max(n, 1)
    return (np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros(n1, np.uint32), np.zeros(n1, np.uint64),
            np.zeros(n1, np.uint32), np.zeros(n1, np.uint64))


def runs_search(keys, runs):
    """The host half: MemTable.Get of every key over `runs` (host_run()s, the active memtable first), the first
    run that holds the key deciding.  Returns (status u8, run u8, entry u32, vloc u64, vlen u32, seq u64).  A
    run that fails its checks: SebError (INVALID) naming "run R: entry E"."""
    kb = as_keys(keys)
    arr = _run_array(runs)
    out = _memget_out(kb.n)
    check(lib().seb_runs_search(kb.ref, arr, len(runs), *[o.ctypes.data for o in out]))
    return tuple(o[: kb.n] for o in out)


def get_join(mem_status, sst_status):
    """The host half of LSM.Get's decision over both halves: (status u8, source u8)."""
    mem = np.ascontiguousarray(mem_status, dtype=np.uint8)
    sst = np.ascontiguousarray(sst_status, dtype=np.uint8)
    if mem.shape != sst.shape:
        raise ValueError("mem_status and sst_status must have one shape")
    st, src = np.zeros(max(mem.size, 1), np.uint8), np.zeros(max(mem.size, 1), np.uint8)
    check(lib().seb_get_join(mem.ctypes.data, sst.ctypes.data, mem.size, st.ctypes.data, src.ctypes.data))
    return st[: mem.size], src[: mem.size]


def dev_run_index_size(n: int) -> int:
    return lib().seb_dev_run_index_size(n)


def dev_run_index(run: seb_run, index, index_bytes: int | None = None, stream=None) -> None:
    """Device form: checks the run (a dev_run()) and builds its index into the tensor `index`
    (dev_run_index_size(run.n) bytes, 16-byte aligned).  Synchronises; a run that fails: SebError (INVALID)
    naming "entry E"."""
    check(lib().seb_dev_run_index(C.byref(run), _ptr(index), (_nbytes(index) if index is not None else 0)
                                  if index_bytes is None else index_bytes, _stream(stream)))


def dev_runs_search(keys: seb_keys, runs, indexes, status, run=None, entry=None, vloc=None, vlen=None, seq=None,
                    stream=None) -> None:
    """Device form: `runs` are dev_run()s and `indexes` their index tensors (None for an empty run); status (n
    u8) and optionally run (n u8), entry (n u32), vloc (n u64), vlen (n u32), seq (n u64).  Not synchronised."""
    if len(runs) != len(indexes):
        raise ValueError("one index per run")
    n = keys.n
    for name, t, size in (("status", status, n), ("run", run, n), ("entry", entry, 4 * n), ("vloc", vloc, 8 * n),
                          ("vlen", vlen, 4 * n), ("seq", seq, 8 * n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {n} keys need {size}")
    for r, ix in zip(runs, indexes):
        if r.n and ix is not None and _nbytes(ix) < dev_run_index_size(r.n):
            raise ValueError(f"an index holds {_nbytes(ix)} bytes, {r.n} entries need {dev_run_index_size(r.n)}")
    ix = (_vp * max(len(runs), 1))(*[_ptr(t) for t in indexes])
    check(lib().seb_dev_runs_search(C.byref(keys), _run_array(runs), ix, len(runs), _ptr(status), _ptr(run), _ptr(entry),
                                    _ptr(vloc), _ptr(vlen), _ptr(seq), _stream(stream)))


def dev_get_join(mem_status, sst_status, n: int, status, source=None, stream=None) -> None:
    """Device form of LSM.Get's decision over the memtables' status and the SSTables' (dev_resolve_rows'):
    status (n u8, may be sst_status itself) and optionally source (n u8: 0 memtables, 1 SSTables).  Not
    synchronised."""
    for name, t in (("mem_status", mem_status), ("sst_status", sst_status), ("status", status), ("source", source)):
        if t is not None and _nbytes(t) < n:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {n} keys need {n}")
    check(lib().seb_dev_get_join(_ptr(mem_status), _ptr(sst_status), n, _ptr(status), _ptr(source), _stream(stream)))


# ------------------------------- Get path: undecided keys on to the SSTable steps (lsm/lsm.go:144-166)

def _np_ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def get_compact(keys, mem_status, caps: tuple[int, int] | None = None):
    """The host half: the keys `mem_status` leaves undecided (neither MEM_FOUND nor MEM_TOMBSTONE), in batch order.
    Returns (sizes, out_keys u8, out_off u64 or None for a fixed-stride batch, row u32); sizes = (n, undecided,
    key_bytes).  caps = (key_cap, row_cap) sizes the outputs instead of a plan: a cap below its size raises SebError
    (RANGE) with `.sizes` set for the retry."""
    kb = as_keys(keys)
    mem = np.ascontiguousarray(mem_status, dtype=np.uint8)
    if mem.size != kb.n:
        raise ValueError(f"mem_status holds {mem.size} bytes, the batch has {kb.n} keys")
    sz = seb_compact_sizes()
    if caps is None:
        check(lib().seb_get_compact(kb.ref, _np_ptr(mem), C.byref(sz), None, 0, None, None, 0))
        caps = (sz.key_bytes, sz.undecided)
    key_cap, row_cap = caps
    out_keys, row = np.zeros(max(key_cap, 1), np.uint8), np.zeros(max(row_cap, 1), np.uint32)
    out_off = np.zeros(row_cap + 1, np.uint64) if kb.offsets is not None else None
    rc = lib().seb_get_compact(kb.ref, _np_ptr(mem), C.byref(sz), out_keys.ctypes.data, key_cap,
                               out_off.ctypes.data if out_off is not None else None, row.ctypes.data, row_cap)
    if rc < 0:
        err = SebError(rc, last_error())
        err.sizes = sz.as_tuple()
        raise err
    return (sz.as_tuple(), out_keys[: sz.key_bytes], None if out_off is None else out_off[: sz.undecided + 1],
            row[: sz.undecided])


def get_join_rows(mem_status, row, sst_status, mem_vloc=None, mem_vlen=None, sst_col=None, sst_vloc=None, sst_vlen=None):
    """The host half of the row-mapped join: sst_* are indexed by compacted key j and land on batch key row[j].
    Returns (status u8, source u8, col u16, vloc u64, vlen u32), n elements each."""
    mem = np.ascontiguousarray(mem_status, dtype=np.uint8)
    rw = np.ascontiguousarray(row, dtype=np.uint32)
    ss = np.ascontiguousarray(sst_status, dtype=np.uint8)
    opt = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)  # noqa: E731
    mvl, mvn = opt(mem_vloc, np.uint64), opt(mem_vlen, np.uint32)
    sc, svl, svn = opt(sst_col, np.uint16), opt(sst_vloc, np.uint64), opt(sst_vlen, np.uint32)
    n, m = mem.size, rw.size
    for name, a, want in (("sst_status", ss, m), ("mem_vloc", mvl, n), ("mem_vlen", mvn, n), ("sst_col", sc, m),
                          ("sst_vloc", svl, m), ("sst_vlen", svn, m)):
        if a is not None and a.size != want:
            raise ValueError(f"{name} holds {a.size} elements, not {want}")
    n1 = max(n, 1)
    out = (np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros(n1, np.uint16), np.zeros(n1, np.uint64),
           np.zeros(n1, np.uint32))
    check(lib().seb_get_join_rows(_np_ptr(mem), _np_ptr(mvl), _np_ptr(mvn), n, _np_ptr(rw), m, _np_ptr(ss), _np_ptr(sc),
                                  _np_ptr(svl), _np_ptr(svn), *[o.ctypes.data for o in out]))
    return tuple(o[:n] for o in out)


def dev_get_compact_workspace_size(n: int) -> int:
    return lib().seb_dev_get_compact_workspace_size(n)


def dev_get_compact_plan(keys: seb_keys, mem_status, ws, ws_bytes: int | None = None, stream=None) -> seb_compact_sizes:
    """Device form: counts the keys of the device batch `keys` that `mem_status` (n u8) leaves undecided, into the
    workspace tensor `ws` (dev_get_compact_workspace_size(n) bytes, 16-byte aligned).  Synchronises; returns the
    sizes (.n, .undecided, .key_bytes) that dev_get_compact_emit takes."""
    if mem_status is not None and _nbytes(mem_status) < keys.n:
        raise ValueError(f"mem_status holds {_nbytes(mem_status)} bytes, {keys.n} keys need {keys.n}")
    sz = seb_compact_sizes()
    check(lib().seb_dev_get_compact_plan(C.byref(keys), _ptr(mem_status), _ptr(ws), (_nbytes(ws) if ws is not None else 0)
                                         if ws_bytes is None else ws_bytes, C.byref(sz), _stream(stream)))
    return sz


def dev_get_compact_emit(keys: seb_keys, mem_status, sizes: seb_compact_sizes, ws, out_keys, out_off, row, stream=None):
    """Device form: writes the compacted batch into the caller's tensors out_keys (sizes.key_bytes u8, any
    alignment), out_off (sizes.undecided + 1 u64; None for a fixed-stride batch) and row (sizes.undecided u32).
    Returns (dev_keys over the compacted batch, row); not synchronised."""
    m = sizes.undecided
    for name, t, size in (("mem_status", mem_status, keys.n), ("out_keys", out_keys, sizes.key_bytes), ("row", row, 4 * m),
                          ("out_off", out_off, 8 * (m + 1)),
                          ("ws", ws, dev_get_compact_workspace_size(keys.n) if keys.n else 0)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, the plan needs {size}")
    check(lib().seb_dev_get_compact_emit(C.byref(keys), _ptr(mem_status), C.byref(sizes), _ptr(ws), _ptr(out_keys),
                                         _ptr(out_off), _ptr(row), _stream(stream)))
    if keys.offsets:
        ck = seb_keys(_ptr(out_keys), _ptr(out_off), m, 0, 0)
    else:
        ck = seb_keys(_ptr(out_keys), None, m, keys.stride, 0)
    ck._keep = (out_keys, out_off)
    return ck, row


def dev_get_join_rows(mem_status, n: int, row, m: int, sst_status, status, source=None, col=None, vloc=None, vlen=None,
                      mem_vloc=None, mem_vlen=None, sst_col=None, sst_vloc=None, sst_vlen=None, stream=None) -> None:
    """Device form of the row-mapped join: the SSTable steps ran on the m compacted keys (sst_status, and optionally
    sst_col / sst_vloc / sst_vlen, as dev_resolve_rows wrote them) and row (m u32) names each one's batch key.
    Outputs: status (n u8) and optionally source (n u8), col (n u16), vloc (n u64), vlen (n u32).  Not
    synchronised."""
    for name, t, size in (("mem_status", mem_status, n), ("mem_vloc", mem_vloc, 8 * n), ("mem_vlen", mem_vlen, 4 * n),
                          ("row", row, 4 * m), ("sst_status", sst_status, m), ("sst_col", sst_col, 2 * m),
                          ("sst_vloc", sst_vloc, 8 * m), ("sst_vlen", sst_vlen, 4 * m), ("status", status, n),
                          ("source", source, n), ("col", col, 2 * n), ("vloc", vloc, 8 * n), ("vlen", vlen, 4 * n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {n} keys and {m} rows need {size}")
    check(lib().seb_dev_get_join_rows(_ptr(mem_status), _ptr(mem_vloc), _ptr(mem_vlen), n, _ptr(row), m, _ptr(sst_status),
                                      _ptr(sst_col), _ptr(sst_vloc), _ptr(sst_vlen), _ptr(status), _ptr(source), _ptr(col),
                                      _ptr(vloc), _ptr(vlen), _stream(stream)))


# ------------------------------- Get values: the found values into one dense buffer (lsm/sstable.go:276-278)

def get_values(status, source, run, vloc, vlen, vals=(), pool=None, val_cap: int | None = None, val_bytes=None):
    """The host half and the device form's reference: the values of the keys whose status is GET_FOUND, back to back
    in batch order.  source 0 reads vals[run[i]] (the runs' value bytes, u8 arrays; None for a null pointer, whose
    size val_bytes[r] then gives), source 1 reads pool; run may be None with at most one run.  Returns (sizes,
    out_off u64 n + 1, out_vals u8); sizes = (n, found, val_bytes).  val_cap sizes out_vals instead of a plan: below
    the values' bytes it raises SebError (RANGE) with `.sizes` set for the retry.  An invalid found key raises
    SebError (INVALID) naming the lowest one."""
    st = np.ascontiguousarray(status, dtype=np.uint8)
    so = np.ascontiguousarray(source, dtype=np.uint8)
    rn = None if run is None else np.ascontiguousarray(run, dtype=np.uint8)
    vl = np.ascontiguousarray(vloc, dtype=np.uint64)
    vn = np.ascontiguousarray(vlen, dtype=np.uint32)
    n = st.size
    for name, a in (("source", so), ("run", rn), ("vloc", vl), ("vlen", vn)):
        if a is not None and a.size != n:
            raise ValueError(f"{name} holds {a.size} elements, the batch has {n} keys")
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.uint8) for v in vals]
    nr = len(keep)
    vp = (_vp * max(nr, 1))(*[v.ctypes.data if v is not None else None for v in keep])
    vb = (_u64 * max(nr, 1))(*(val_bytes if val_bytes is not None else [0 if v is None else v.size for v in keep]))
    pl = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint8)
    args = (_np_ptr(st), _np_ptr(so), _np_ptr(rn), _np_ptr(vl), _np_ptr(vn), n, vp if nr else None, vb if nr else None, nr,
            pl.ctypes.data if pl is not None else None, pl.size if pl is not None else 0)
    sz = seb_values_sizes()
    if val_cap is None:
        check(lib().seb_get_values(*args, C.byref(sz), None, None, 0))
        val_cap = sz.val_bytes
    out_off, out_vals = np.zeros(n + 1, np.uint64), np.zeros(max(val_cap, 1), np.uint8)
    rc = lib().seb_get_values(*args, C.byref(sz), out_off.ctypes.data, out_vals.ctypes.data, val_cap)
    if rc < 0:
        err = SebError(rc, last_error())
        err.sizes = sz.as_tuple()
        raise err
    return sz.as_tuple(), out_off, out_vals[: sz.val_bytes]


def dev_get_values_workspace_size(n: int) -> int:
    return lib().seb_dev_get_values_workspace_size(n)


def _values_dev_args(status, source, run, vloc, vlen, n, vals, val_bytes, pool, pool_bytes):
    for name, t, size in (("status", status, n), ("source", source, n), ("run", run, n), ("vloc", vloc, 8 * n),
                          ("vlen", vlen, 4 * n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {n} keys need {size}")
    nr = len(vals)
    if val_bytes is None:
        val_bytes = [_nbytes(v) if v is not None else 0 for v in vals]
    vp = (_vp * max(nr, 1))(*[_ptr(v) for v in vals])
    vb = (_u64 * max(nr, 1))(*val_bytes)
    if pool_bytes is None:
        pool_bytes = _nbytes(pool) if pool is not None else 0
    return (_ptr(status), _ptr(source), _ptr(run), _ptr(vloc), _ptr(vlen), n, vp if nr else None, vb if nr else None, nr,
            _ptr(pool), pool_bytes)


def dev_get_values_plan(status, source, run, vloc, vlen, n: int, vals, pool, ws, val_bytes=None, pool_bytes=None,
                        ws_bytes: int | None = None, stream=None) -> seb_values_sizes:
    """Device form: sizes the gather of the found keys' values.  status / source / run (n u8; run None with at most
    one run), vloc (n u64) and vlen (n u32) as dev_get_join_rows and dev_runs_search wrote them; vals = the runs'
    value tensors (val_bytes defaults to their sizes; None for a null pointer), pool = the block pool tensor.  The
    plan goes into the workspace tensor `ws` (dev_get_values_workspace_size(n) bytes, 16-byte aligned).
    Synchronises; returns the sizes (.n, .found, .val_bytes) that dev_get_values_emit takes; an invalid found key
    raises SebError (INVALID) naming the lowest one."""
    args = _values_dev_args(status, source, run, vloc, vlen, n, vals, val_bytes, pool, pool_bytes)
    sz = seb_values_sizes()
    check(lib().seb_dev_get_values_plan(*args, _ptr(ws), (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                        C.byref(sz), _stream(stream)))
    return sz


def dev_get_values_emit(status, source, run, vloc, vlen, n: int, vals, pool, sizes: seb_values_sizes, ws, out_off, out_vals,
                        val_bytes=None, pool_bytes=None, stream=None) -> None:
    """Device form: writes out_off (n + 1 u64) and out_vals (sizes.val_bytes u8, any alignment; None where that is
    0) from the same inputs and workspace as the plan.  Not synchronised."""
    for name, t, size in (("out_off", out_off, 8 * (n + 1) if n else 0), ("out_vals", out_vals, sizes.val_bytes),
                          ("ws", ws, dev_get_values_workspace_size(n) if n else 0)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, the plan needs {size}")
    args = _values_dev_args(status, source, run, vloc, vlen, n, vals, val_bytes, pool, pool_bytes)
    check(lib().seb_dev_get_values_emit(*args, C.byref(sizes), _ptr(ws), _ptr(out_off), _ptr(out_vals), _stream(stream)))


# ------------------------------- block ids: located cells (slot, block offset) into ids of the block pool

def block_ids(cand, blocks, res_first=None, res_count=None, id_base: int = 0, uniq_cap: int | None = None,
              stream=None):
    """The host half and the device forms' reference: cand (u16 slots, 0xFFFF padding) and blocks (u64 offsets,
    NO_BLOCK for none) of one shape, and optionally the residency table (res_first / res_count u32 per slot,
    res_first NO_BLOCK_ID for a file that is not resident).  Returns (sizes, bid u32 in the shape of cand, uniq_slot
    u16, uniq_block u64); sizes = (cells, resident, misses, uniq, bad).  uniq_cap sizes the read list instead of a
    sizes-only call: below `uniq` it raises SebError (RANGE) with `.sizes` set for the retry.  `stream` is accepted
    for symmetry with the device forms and ignored: nothing here touches a device."""
    cand = np.ascontiguousarray(cand, dtype=np.uint16)
    blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
    if cand.shape != blocks.shape:
        raise ValueError("cand and blocks must have one shape")
    rf = None if res_first is None else np.ascontiguousarray(res_first, dtype=np.uint32)
    rc_ = None if res_count is None else np.ascontiguousarray(res_count, dtype=np.uint32)
    if (rf is None) != (rc_ is None) or (rf is not None and rf.size != rc_.size):
        raise ValueError("res_first and res_count must both be given, with one entry per slot")
    slots = 0 if rf is None else rf.size
    cells = cand.size
    sz = seb_blockids_sizes()
    if uniq_cap is None:
        check(lib().seb_block_ids(_np_ptr(cand), _np_ptr(blocks), cells, _np_ptr(rf), _np_ptr(rc_), slots, id_base, None,
                                  None, None, 0, C.byref(sz)))
        uniq_cap = sz.uniq
    bid = np.zeros(max(cells, 1), np.uint32)
    us, ub = np.zeros(max(uniq_cap, 1), np.uint16), np.zeros(max(uniq_cap, 1), np.uint64)
    rc = lib().seb_block_ids(_np_ptr(cand), _np_ptr(blocks), cells, _np_ptr(rf), _np_ptr(rc_), slots, id_base,
                             bid.ctypes.data, us.ctypes.data, ub.ctypes.data, uniq_cap, C.byref(sz))
    if rc < 0:
        err = SebError(rc, last_error())
        err.sizes = sz.as_tuple()
        raise err
    return sz.as_tuple(), bid[:cells].reshape(cand.shape), us[: sz.uniq], ub[: sz.uniq]


def _blockids_check(cells, cand, blocks, res_first, res_count, res_slots, extra=()):
    for name, t, size in (("cand", cand, 2 * cells), ("blocks", blocks, 8 * cells), ("res_first", res_first, 4 * res_slots),
                          ("res_count", res_count, 4 * res_slots)) + tuple(extra):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {cells} cells and {res_slots} slots need {size}")


def dev_block_ids_resident(cand, blocks, cells: int, res_first, res_count, res_slots: int, bid, counts=None,
                           stream=None) -> None:
    """Device form, one kernel: bid[c] (u32) = the pool id of cell c of a resident file (res_first[slot] + offset /
    4096), NO_BLOCK_ID for padding, refused offsets and the cells of files that are not resident.  counts
    (optional, three u64): resident, misses, bad.  Not synchronised."""
    _blockids_check(cells, cand, blocks, res_first, res_count, res_slots, (("bid", bid, 4 * cells), ("counts", counts, 24)))
    check(lib().seb_dev_block_ids_resident(_ptr(cand), _ptr(blocks), cells, _ptr(res_first), _ptr(res_count), res_slots,
                                           _ptr(bid), _ptr(counts), _stream(stream)))


def dev_block_ids_workspace_size(cells: int, max_uniq: int, stream=None) -> int:
    return lib().seb_dev_block_ids_workspace_size(cells, max_uniq)


def dev_block_ids_plan(cand, blocks, cells: int, res_first, res_count, res_slots: int, max_uniq: int, ws,
                       ws_bytes: int | None = None, stream=None) -> seb_blockids_sizes:
    """Device form: classifies the cells and numbers the distinct (slot, offset) pairs of the files that are not
    resident, into the workspace tensor `ws` (dev_block_ids_workspace_size(cells, max_uniq) bytes, 16-byte
    aligned).  Synchronises; returns the sizes that dev_block_ids_emit takes.  More than max_uniq distinct pairs
    raises SebError (RANGE) with `.sizes` set: max_uniq = sizes.misses always suffices."""
    _blockids_check(cells, cand, blocks, res_first, res_count, res_slots)
    sz = seb_blockids_sizes()
    rc = lib().seb_dev_block_ids_plan(_ptr(cand), _ptr(blocks), cells, _ptr(res_first), _ptr(res_count), res_slots, max_uniq,
                                      _ptr(ws), (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                      C.byref(sz), _stream(stream))
    if rc < 0:
        err = SebError(rc, last_error())
        err.sizes = sz
        raise err
    return sz


def dev_block_ids_emit(cand, blocks, cells: int, res_first, res_count, res_slots: int, max_uniq: int, id_base: int,
                       sizes: seb_blockids_sizes, ws, bid, uniq_slot, uniq_block, stream=None) -> None:
    """Device form: bid (cells u32) for every cell, a miss cell's id = id_base + its pair's rank, and the read list
    uniq_slot (sizes.uniq u16) / uniq_block (sizes.uniq u64).  The same inputs, max_uniq and workspace as the plan.
    Not synchronised."""
    _blockids_check(cells, cand, blocks, res_first, res_count, res_slots,
                    (("bid", bid, 4 * cells), ("uniq_slot", uniq_slot, 2 * sizes.uniq), ("uniq_block", uniq_block, 8 * sizes.uniq),
                     ("ws", ws, dev_block_ids_workspace_size(cells, max_uniq) if cells else 0)))
    check(lib().seb_dev_block_ids_emit(_ptr(cand), _ptr(blocks), cells, _ptr(res_first), _ptr(res_count), res_slots, max_uniq,
                                       id_base, C.byref(sizes), _ptr(ws), _ptr(bid), _ptr(uniq_slot), _ptr(uniq_block),
                                       _stream(stream)))


def memtable_get(keys, runs, device: int = 0):
    """Ctx.memtable_get on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.memtable_get(keys, runs)
    finally:
        ctx.close()


# ------------------------------- memtable write side (lsm/lsm.go:97-137, lsm/wal.go:31-65, lsm/memtable.go:34-93)

def _ops_host_args(keys, vals, val_off, deleted):
    kb = as_keys(keys)
    va = _wal_image_arg(vals)
    vo = np.ascontiguousarray(val_off, dtype=np.uint64)
    if vo.size != kb.n + 1:
        raise ValueError(f"val_off holds {vo.size} offsets, {kb.n} ops need {kb.n + 1}")
    de = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
    if de is not None and de.size < kb.n:
        raise ValueError(f"deleted holds {de.size} bytes, the batch has {kb.n} ops")
    return kb, va, vo, de


def wal_frame_plan(keys, val_off, deleted=None) -> tuple[np.ndarray, int]:
    """The host half's plan of a Put / Delete batch: (rec_off u64 of n + 1 boundaries, image bytes).  A key or a
    value of 2^32 bytes or more, or offsets that decrease: SebError (INVALID) naming "op I"."""
    kb = as_keys(keys)
    vo = np.ascontiguousarray(val_off, dtype=np.uint64)
    de = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
    off, total = np.zeros(kb.n + 1, np.uint64), _u64(0)
    check(lib().seb_wal_frame_plan(kb.ref, vo.ctypes.data, None if de is None else de.ctypes.data, off.ctypes.data,
                                   C.byref(total)))
    return off, total.value


def wal_frame(keys, vals, val_off, deleted=None, first_seq: int = 1) -> tuple[np.ndarray, np.ndarray]:
    """The host half: the batch as WAL.Append's sealed records, op i with sequence first_seq + i (a Delete with no
    value and deleted = 1): (image u8, rec_off u64)."""
    kb, va, vo, de = _ops_host_args(keys, vals, val_off, deleted)
    off, total = wal_frame_plan(kb, vo, de)
    image = np.zeros(max(total, 1), np.uint8)
    check(lib().seb_wal_frame_emit(kb.ref, va.ctypes.data, vo.ctypes.data, None if de is None else de.ctypes.data, first_seq,
                                   image.ctypes.data, total))
    return image[:total], off


def dev_wal_frame_plan(keys: seb_keys, val_off, deleted, rec_off, stream=None) -> int:
    """Device form: rec_off (n + 1 u64, a 64-bit tensor) is written; synchronises and returns the image's size."""
    if keys.n and (rec_off is None or _nbytes(rec_off) < 8 * (keys.n + 1)):
        raise ValueError(f"rec_off holds fewer than {keys.n + 1} offsets")
    total = _u64(0)
    check(lib().seb_dev_wal_frame_plan(C.byref(keys), _ptr(val_off), _ptr(deleted), _ptr(rec_off), C.byref(total),
                                       _stream(stream)))
    return total.value


def dev_wal_frame_emit(keys: seb_keys, vals, val_off, deleted, first_seq: int, rec_off, image, image_bytes: int | None = None,
                       stream=None) -> None:
    """Device form: the sealed image into `image` (u8 tensor or view, any alignment); rec_off and image_bytes as
    dev_wal_frame_plan left them.  Not synchronised."""
    total = (_nbytes(image) if image is not None else 0) if image_bytes is None else image_bytes
    if total and _nbytes(image) < total:
        raise ValueError(f"image holds {_nbytes(image)} bytes, the plan needs {total}")
    check(lib().seb_dev_wal_frame_emit(C.byref(keys), _ptr(vals), _ptr(val_off), _ptr(deleted), first_seq, _ptr(rec_off),
                                       _ptr(image), total, _stream(stream)))


def run_size_delta(fresh: seb_run, runs) -> int:
    """The host half: MemTable.size's change when the host_run() `fresh` goes in front of the active memtable's
    `runs` (host_run()s, newest first, at most MEM_MAX_RUNS - 1)."""
    d = C.c_int64(0)
    check(lib().seb_run_size_delta(C.byref(fresh), _run_array(list(runs)), len(runs), C.byref(d)))
    return d.value


def dev_run_size_delta(fresh: seb_run, runs, indexes, delta, stream=None) -> None:
    """Device form: dev_run()s and the existing runs' index tensors; delta: one int64 on the device.  Not synchronised."""
    if len(runs) != len(indexes):
        raise ValueError("one index per run")
    if delta is None or _nbytes(delta) < 8:
        raise ValueError("delta holds fewer than 8 bytes")
    ix = (_vp * max(len(runs), 1))(*[_ptr(t) for t in indexes])
    check(lib().seb_dev_run_size_delta(C.byref(fresh), _run_array(list(runs)), ix, len(runs), _ptr(delta), _stream(stream)))


def _fold_host_args(runs, vals):
    if len(runs) != len(vals):
        raise ValueError("one value array per run")
    keep = [_wal_image_arg(v) for v in vals]
    vp = (_vp * max(len(runs), 1))(*[v.ctypes.data if v.size else None for v in keep])
    vb = (_u64 * max(len(runs), 1))(*[v.size for v in keep])
    return _run_array(list(runs)), vp, vb, keep


def runs_fold_plan(runs, vals) -> tuple[int, int, int, int, int, int, int, int]:
    """The host half's plan: (entries_in, entries_out, key_bytes, val_bytes, shadowed, tombstones, max_sequence,
    memtable_size) of the fold of host_run()s, newest first; vals[r] = run r's value bytes."""
    arr, _, vb, keep = _fold_host_args(runs, vals)
    sz = seb_fold_sizes()
    check(lib().seb_runs_fold_plan(arr, vb, len(runs), C.byref(sz)))
    return sz.as_tuple()


def runs_fold(runs, vals, sizes=None):
    """The host half: (keys u8, key_off u64, vals u8, val_off u64, deleted u8, seq u64, sizes) of the one run the
    runs add up to; sizes default to runs_fold_plan's."""
    arr, vp, vb, keep = _fold_host_args(runs, vals)
    sz = seb_fold_sizes(*(runs_fold_plan(runs, vals) if sizes is None else sizes))
    out = _run_out(sz.key_bytes, sz.val_bytes, sz.entries_out)
    check(lib().seb_runs_fold_emit(arr, vp, vb, len(runs), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                   out[3].ctypes.data, out[4].ctypes.data, out[5].ctypes.data, C.byref(sz)))
    return _run_trim(out, sz)


def dev_runs_fold_workspace_size(entries: int) -> int:
    return lib().seb_dev_runs_fold_workspace_size(entries)


def _fold_dev_args(runs, indexes, vals, val_bytes):
    if len(runs) != len(indexes) or (vals is not None and len(vals) != len(runs)):
        raise ValueError("one index and one value tensor per run")
    ix = (_vp * max(len(runs), 1))(*[_ptr(t) for t in indexes])
    if val_bytes is None:
        val_bytes = [_nbytes(v) if v is not None else 0 for v in vals]
    vb = (_u64 * max(len(runs), 1))(*val_bytes)
    vp = None if vals is None else (_vp * max(len(runs), 1))(*[_ptr(v) for v in vals])
    return _run_array(list(runs)), ix, vp, vb


def dev_runs_fold_plan(runs, indexes, val_bytes, ws, ws_bytes: int | None = None, stream=None):
    """Device form: dev_run()s (newest first), their index tensors and the bytes each run's values hold; ranks every
    entry into the workspace tensor `ws` (dev_runs_fold_workspace_size(total entries) bytes); synchronises and
    returns the sizes."""
    arr, ix, _, vb = _fold_dev_args(runs, indexes, None, list(val_bytes))
    sz = seb_fold_sizes()
    check(lib().seb_dev_runs_fold_plan(arr, ix, vb, len(runs), _ptr(ws),
                                       (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes, C.byref(sz),
                                       _stream(stream)))
    return sz.as_tuple()


def dev_runs_fold_emit(runs, indexes, vals, sizes, ws, keys, key_off, out_vals, val_off, deleted, seq=None, val_bytes=None,
                       stream=None) -> None:
    """Device form: writes the folded run (sizes as dev_runs_fold_plan returned them); vals[r] = run r's value
    tensor.  Not synchronised."""
    sz = seb_fold_sizes(*sizes)
    for name, t, size in (("keys", keys, sz.key_bytes), ("out_vals", out_vals, sz.val_bytes), ("deleted", deleted, sz.entries_out),
                          ("key_off", key_off, 8 * (sz.entries_out + 1)), ("val_off", val_off, 8 * (sz.entries_out + 1)),
                          ("seq", seq, 8 * sz.entries_out if seq is not None else 0)):
        if (t is None and size) or (t is not None and _nbytes(t) < size):
            raise ValueError(f"{name} holds {0 if t is None else _nbytes(t)} bytes, the plan needs {size}")
    arr, ix, vp, vb = _fold_dev_args(runs, indexes, vals, val_bytes)
    check(lib().seb_dev_runs_fold_emit(arr, ix, vp, vb, len(runs), C.byref(sz), _ptr(ws), _nbytes(ws) if ws is not None else 0,
                                       _ptr(keys), _ptr(key_off), _ptr(out_vals), _ptr(val_off), _ptr(deleted), _ptr(seq),
                                       _stream(stream)))


def memtable_apply(keys, vals, val_off, deleted=None, first_seq: int = 1, runs=(), caps=None, device: int = 0):
    """Ctx.memtable_apply on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.memtable_apply(keys, vals, val_off, deleted, first_seq, runs, caps)
    finally:
        ctx.close()


def memtable_fold(runs, vals, caps=None, device: int = 0):
    """Ctx.memtable_fold on a context made for the call."""
    ctx = Ctx(device)
    try:
        return ctx.memtable_fold(runs, vals, caps)
    finally:
        ctx.close()


def index_scan(block: bytes) -> int:
    """decodeIndex's walk (lsm/sstable.go:168-201) on the host: the entry count, or SebError (SHORT:
    too small / truncated; INVALID: keys not non-decreasing)."""
    n = _u64(0)
    check(lib().seb_index_scan(block, len(block), C.byref(n)))
    return n.value


def wal_scan(image: bytes | np.ndarray) -> tuple[np.ndarray, int]:
    """ReadAll's framing walk (lsm/wal.go:98-121) on the host: (offsets[0..n], status)."""
    buf = np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray)) else image
    cap = buf.size // 21 + 2
    off = np.zeros(cap, np.uint64)
    n = _u64(0)
    rc = lib().seb_wal_scan(buf.ctypes.data, buf.size, off.ctypes.data, cap, C.byref(n))
    if rc not in (0, -5):
        check(rc)
    return off[: n.value + 1].copy(), rc


# ------------------------------- hash index, read side: recover() of segment images, Get of a key batch (hashindex/)

SEG_HEADER_BYTES = 20        # SEB_SEG_HEADER_BYTES
HIDX_NO_RECORD = 2**64 - 1   # SEB_HIDX_NO_RECORD


def _bytes_arg(b) -> np.ndarray:
    if isinstance(b, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(b), np.uint8)
    return np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)


def seg_scan(image, base: int = 0, cap: int | None = None) -> tuple[np.ndarray, int]:
    """One segment image's header walk on the host (hashindex/recovery.go:86-112 without the CRC): (the records' pool
    offsets base + file offset, short_tail).  cap: the offsets' capacity (default: always enough)."""
    buf = _bytes_arg(image)
    cap = buf.size // SEG_HEADER_BYTES + 1 if cap is None else cap
    off = np.zeros(max(cap, 1), np.uint64)
    n, tail = _u64(0), _i(0)
    check(lib().seb_seg_scan(_np_ptr(buf), buf.size, base, off.ctypes.data, cap, C.byref(n), C.byref(tail)))
    return off[: n.value].copy(), tail.value


def segs_scan(segments):
    """The layout the hash index calls take, from the segment images oldest first: (pool u8, rec_off u64, seg_first
    u64 S + 1, seg_base u64, seg_bytes u64, short_tail u8)."""
    imgs = [_bytes_arg(s) for s in segments]
    seg_bytes = np.array([a.size for a in imgs], np.uint64)
    seg_base = np.zeros(len(imgs), np.uint64)
    if len(imgs) > 1:
        np.cumsum(seg_bytes[:-1], out=seg_base[1:])
    offs, tails, first = [], [], [0]
    for a, b in zip(imgs, seg_base):
        o, t = seg_scan(a, int(b))
        offs.append(o), tails.append(t), first.append(first[-1] + o.size)
    pool = np.concatenate(imgs) if imgs else np.zeros(0, np.uint8)
    rec_off = np.concatenate(offs) if offs else np.zeros(0, np.uint64)
    return pool, rec_off.astype(np.uint64), np.array(first, np.uint64), seg_base, seg_bytes, np.array(tails, np.uint8)


def seg_verify(pool, rec_off, seg_first, seg_base, seg_bytes):
    """recover()'s CRC pass and cuts on the host: (ok u8 per record, valid u64 and size_after u64 per segment, live u8
    per record)."""
    pool, rec_off = _bytes_arg(pool), np.ascontiguousarray(rec_off, dtype=np.uint64)
    first, base, size = (np.ascontiguousarray(a, dtype=np.uint64) for a in (seg_first, seg_base, seg_bytes))
    n, s = rec_off.size, first.size - 1
    ok, live = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    valid, after = np.zeros(s, np.uint64), np.zeros(s, np.uint64)
    check(lib().seb_seg_verify(_np_ptr(pool), pool.size, _np_ptr(rec_off), n, first.ctypes.data, _np_ptr(base), _np_ptr(size), s,
                               _np_ptr(ok), _np_ptr(valid), _np_ptr(after), _np_ptr(live)))
    return ok, valid, after, live


def hidx_lookup(pool, rec_off, live, keys, verify: bool = True):
    """HashIndex.Get for a key batch on the host, over the live records: (status u8, rec u64, vloc u64, vlen u32,
    distinct).  The reference for dev_hidx_get."""
    pool, rec_off = _bytes_arg(pool), np.ascontiguousarray(rec_off, dtype=np.uint64)
    lv = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
    kb = as_keys(keys)
    n = kb.n
    status, rec = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    vloc, vlen = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    distinct = _u64(0)
    check(lib().seb_hidx_lookup(_np_ptr(pool), pool.size, _np_ptr(rec_off), _np_ptr(lv), rec_off.size, kb.ref, int(bool(verify)),
                                _np_ptr(status), _np_ptr(rec), _np_ptr(vloc), _np_ptr(vlen), C.byref(distinct)))
    return status, rec, vloc, vlen, distinct.value


def dev_hidx_table_bytes(capacity: int) -> int:
    return lib().seb_dev_hidx_table_bytes(capacity)


def dev_hidx_clear(table, capacity: int, stream=None) -> None:
    check(lib().seb_dev_hidx_clear(_ptr(table), capacity, _stream(stream)))


def dev_seg_verify(pool, pool_bytes: int, rec_off, n: int, seg_first, num_segments: int, ok, valid, live=None,
                   stream=None) -> None:
    """Device form of seg_verify: ok (n u8), valid (num_segments u64, device) and live (n u8, optional) from rec_off
    (n u64) and seg_first (num_segments + 1 u64).  Not synchronised."""
    check(lib().seb_dev_seg_verify(_ptr(pool), pool_bytes, _ptr(rec_off), n, _ptr(seg_first), num_segments, _ptr(ok),
                                   _ptr(valid), _ptr(live), _stream(stream)))


def dev_hidx_insert(table, capacity: int, pool, pool_bytes: int, rec_off, live, n: int, stream=None) -> None:
    """The live records (live None: all) into the table.  Not synchronised; dev_hidx_count reports a table that
    filled."""
    check(lib().seb_dev_hidx_insert(_ptr(table), capacity, _ptr(pool), pool_bytes, _ptr(rec_off), _ptr(live), n,
                                    _stream(stream)))


def dev_hidx_count(table, capacity: int, stream=None) -> tuple[int, int]:
    """Synchronises: (distinct keys, bad records skipped); SebError (RANGE) where the table filled."""
    distinct, bad = _u64(0), _u64(0)
    check(lib().seb_dev_hidx_count(_ptr(table), capacity, C.byref(distinct), C.byref(bad), _stream(stream)))
    return distinct.value, bad.value


def dev_hidx_get(table, capacity: int, pool, pool_bytes: int, keys: seb_keys, verify: bool, status, rec=None, vloc=None,
                 vlen=None, source=None, stream=None) -> None:
    """HashIndex.Get for a device key batch: status (u8), rec / vloc (u64), vlen (u32), source (u8), each of keys.n
    elements; all but status optional.  No insert may run concurrently.  Not synchronised."""
    check(lib().seb_dev_hidx_get(_ptr(table), capacity, _ptr(pool), pool_bytes, C.byref(keys), int(bool(verify)), _ptr(status),
                                 _ptr(rec), _ptr(vloc), _ptr(vlen), _ptr(source), _stream(stream)))


# ------------------------------- hash index, write side (hashindex/segment.go:61-125, hashindex.go:92-215, compaction.go)

SEG_NO_LIMIT = 1 << 62  # a rotation limit no segment reaches


def seg_frame_plan(keys, val_off, deleted=None, active_size: int = 0, limit: int = SEG_NO_LIMIT, cut_cap: int | None = None):
    """The host half's plan of a Put / Delete batch for the hash index: (rec_off u64 of n + 1 boundaries, cuts u64,
    image bytes).  cut_cap: the cuts' capacity (default: always enough; below the count: SebError RANGE).  An empty
    key, a key or value of 2^32 bytes or more, keySize + valueSize >= 2^32 or offsets that decrease: SebError
    (INVALID) naming "op I"."""
    kb = as_keys(keys)
    vo = np.ascontiguousarray(val_off, dtype=np.uint64)
    de = None if deleted is None else np.ascontiguousarray(deleted, dtype=np.uint8)
    off, total, ncuts = np.zeros(kb.n + 1, np.uint64), _u64(0), _u64(0)
    cap = kb.n if cut_cap is None else cut_cap
    cut = np.zeros(max(cap, 1), np.uint64)
    check(lib().seb_seg_frame_plan(kb.ref, vo.ctypes.data, _np_ptr(de), active_size, limit, off.ctypes.data, cut.ctypes.data, cap,
                                   C.byref(total), C.byref(ncuts)))
    return off, cut[: ncuts.value].copy(), total.value


def seg_frame(keys, vals, val_off, deleted=None, timestamp: int = 0, active_size: int = 0, limit: int = SEG_NO_LIMIT):
    """The host half: the batch as segment.append's sealed records, every one with `timestamp` (a Delete with no
    value): (image u8, rec_off u64, cuts u64)."""
    kb, va, vo, de = _ops_host_args(keys, vals, val_off, deleted)
    off, cuts, total = seg_frame_plan(kb, vo, de, active_size, limit)
    image = np.zeros(max(total, 1), np.uint8)
    check(lib().seb_seg_frame_emit(kb.ref, va.ctypes.data, vo.ctypes.data, _np_ptr(de), timestamp, image.ctypes.data, total))
    return image[:total], off, cuts


def dev_seg_frame_plan(keys: seb_keys, val_off, deleted, rec_off, active_size: int = 0, limit: int = SEG_NO_LIMIT,
                       cut_cap: int | None = None, stream=None) -> tuple[int, np.ndarray]:
    """Device form: rec_off (n + 1 u64, a 64-bit tensor) is written; synchronises and returns (image bytes, cuts u64 on
    the host)."""
    if keys.n and (rec_off is None or _nbytes(rec_off) < 8 * (keys.n + 1)):
        raise ValueError(f"rec_off holds fewer than {keys.n + 1} offsets")
    total, ncuts = _u64(0), _u64(0)
    cap = keys.n if cut_cap is None else cut_cap
    cut = np.zeros(max(cap, 1), np.uint64)
    check(lib().seb_dev_seg_frame_plan(C.byref(keys), _ptr(val_off), _ptr(deleted), active_size, limit, _ptr(rec_off),
                                       cut.ctypes.data, cap, C.byref(total), C.byref(ncuts), _stream(stream)))
    return total.value, cut[: ncuts.value].copy()


def dev_seg_frame_emit(keys: seb_keys, vals, val_off, deleted, timestamp: int, rec_off, image, image_bytes: int | None = None,
                       stream=None) -> None:
    """Device form: the sealed image into `image` (u8 tensor or view, any alignment); rec_off and image_bytes as
    dev_seg_frame_plan left them.  Not synchronised."""
    total = (_nbytes(image) if image is not None else 0) if image_bytes is None else image_bytes
    if total and image is not None and _nbytes(image) < total:
        raise ValueError(f"image holds {_nbytes(image)} bytes, the plan needs {total}")
    check(lib().seb_dev_seg_frame_emit(C.byref(keys), _ptr(vals), _ptr(val_off), _ptr(deleted), timestamp, _ptr(rec_off),
                                       _ptr(image), total, _stream(stream)))


def seg_compact(pool, rec_off, live, timestamp: int, caps: tuple[int, int] | None = None):
    """compactSegments on the host over the live records (live None: all) of the chosen segments: (image u8,
    out_rec_off u64 of survivors + 1, sizes dict).  caps: (image bytes, offsets) instead of the sizing call's."""
    pool, rec_off = _bytes_arg(pool), np.ascontiguousarray(rec_off, dtype=np.uint64)
    lv = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
    sz = seb_segcompact_sizes()
    if caps is None:
        check(lib().seb_seg_compact(_np_ptr(pool), pool.size, _np_ptr(rec_off), _np_ptr(lv), rec_off.size, timestamp, None, 0, None,
                                    0, C.byref(sz)))
        caps = (sz.image_bytes, sz.survivors + 1)
    image, out = np.zeros(max(caps[0], 1), np.uint8), np.zeros(max(caps[1], 1), np.uint64)
    rc = lib().seb_seg_compact(_np_ptr(pool), pool.size, _np_ptr(rec_off), _np_ptr(lv), rec_off.size, timestamp, image.ctypes.data,
                               caps[0], out.ctypes.data, caps[1], C.byref(sz))
    if rc < 0:
        err = SebError(rc, last_error())
        err.sizes = sz.as_dict()
        raise err
    return image[: sz.image_bytes], out[: sz.survivors + 1], sz.as_dict()


def segs_compact(segments, num_segments: int, timestamp: int):
    """compactSegments of the oldest num_segments segment images on the host, as the reference runs it: scan, verify,
    and a record that fails its CRC in one of them aborts the compaction (SebError INVALID naming segment and record);
    a short tail is dropped silently.  Returns seg_compact's triple."""
    pool, rec_off, first, base, size, _ = segs_scan(list(segments)[:num_segments])
    _, valid, _, live = seg_verify(pool, rec_off, first, base, size)
    for s in range(num_segments):
        if int(valid[s]) < int(first[s + 1]) - int(first[s]):
            raise SebError(-1, f"segs_compact: segment {s}: record {int(valid[s])} fails its CRC: the compaction is aborted")
    return seg_compact(pool, rec_off, live, timestamp)


def hidx_logical_size(pool, rec_off, live=None) -> int:
    """getLogicalSize on the host: keySize + valueSize over the index of the live records, tombstones included."""
    pool, rec_off = _bytes_arg(pool), np.ascontiguousarray(rec_off, dtype=np.uint64)
    lv = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
    out = _u64(0)
    check(lib().seb_hidx_logical_size(_np_ptr(pool), pool.size, _np_ptr(rec_off), _np_ptr(lv), rec_off.size, C.byref(out)))
    return out.value


def dev_seg_compact_workspace_size(num_records: int) -> int:
    return lib().seb_dev_seg_compact_workspace_size(num_records)


def dev_seg_compact_plan(pool, pool_bytes: int, rec_off, live, n: int, ws, ws_bytes: int | None = None,
                         stream=None) -> seb_segcompact_sizes:
    """Device form: the scratch table, the survivors' marks and their scan into `ws`; synchronises and returns the sizes."""
    sz = seb_segcompact_sizes()
    check(lib().seb_dev_seg_compact_plan(_ptr(pool), pool_bytes, _ptr(rec_off), _ptr(live), n, _ptr(ws),
                                         (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes, C.byref(sz),
                                         _stream(stream)))
    return sz


def dev_seg_compact_emit(pool, pool_bytes: int, rec_off, n: int, timestamp: int, sizes: seb_segcompact_sizes, ws, image,
                         out_rec_off, ws_bytes: int | None = None, stream=None) -> None:
    """Device form: the survivors into `image` (any alignment) and their offsets into out_rec_off (survivors + 1 u64).
    Not synchronised."""
    if image is not None and _nbytes(image) < sizes.image_bytes:
        raise ValueError(f"image holds {_nbytes(image)} bytes, the plan needs {sizes.image_bytes}")
    if out_rec_off is None or _nbytes(out_rec_off) < 8 * (sizes.survivors + 1):
        raise ValueError(f"out_rec_off holds fewer than {sizes.survivors + 1} offsets")
    check(lib().seb_dev_seg_compact_emit(_ptr(pool), pool_bytes, _ptr(rec_off), n, timestamp, C.byref(sizes), _ptr(ws),
                                         (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes, _ptr(image),
                                         _ptr(out_rec_off), _stream(stream)))


def dev_hidx_logical_size(table, capacity: int, pool, pool_bytes: int, stream=None) -> int:
    """getLogicalSize over the table; synchronises."""
    out = _u64(0)
    check(lib().seb_dev_hidx_logical_size(_ptr(table), capacity, _ptr(pool), pool_bytes, C.byref(out), _stream(stream)))
    return out.value


def _ctx_hidx_recover(self, segments, dev_pool, dev_table, capacity: int, pool_cap: int | None = None):
    """seb_hidx_recover: the segment images (host, oldest first) into the device pool and table.  Returns a dict:
    valid, size_after, short_tail, cut (per segment), records, live_records, distinct.  SebError (RANGE) carries the
    same dict without `distinct` as `.recovered` where the table filled."""
    imgs = [_bytes_arg(s) for s in segments]
    s = len(imgs)
    ptrs = (_vp * max(s, 1))(*[a.ctypes.data if a.size else None for a in imgs])
    sizes = (_u64 * max(s, 1))(*[a.size for a in imgs])
    valid, after = np.zeros(s, np.uint64), np.zeros(s, np.uint64)
    tail, cut = np.zeros(s, np.uint8), np.zeros(s, np.uint8)
    records, alive, distinct = _u64(0), _u64(0), _u64(0)
    cap = (dev_pool.numel() if dev_pool is not None else 0) if pool_cap is None else pool_cap
    rc = lib().seb_hidx_recover(self._p, ptrs if s else None, sizes if s else None, s, _ptr(dev_pool), cap, _ptr(dev_table),
                                capacity, _np_ptr(valid), _np_ptr(after), _np_ptr(tail), _np_ptr(cut), C.byref(records),
                                C.byref(alive), C.byref(distinct))
    out = dict(valid=valid, size_after=after, short_tail=tail, cut=cut, records=records.value, live_records=alive.value)
    if rc < 0:
        err = SebError(rc, last_error())
        err.recovered = out
        raise err
    out["distinct"] = distinct.value
    return out


Ctx.hidx_recover = _ctx_hidx_recover


def _ctx_hidx_compact(self, dev_pool, pool_bytes: int, seg_base, seg_bytes, num_compact: int, rest_rec_off, rest_live,
                      rest_records: int, timestamp: int, dst_pool, dev_table, capacity: int, new_rec_off,
                      dst_cap: int | None = None):
    """seb_hidx_compact: the oldest num_compact segments of the device pool compacted into the front of dst_pool, the
    others copied behind, the table rebuilt.  Returns a dict: sizes, seg_base, seg_bytes (of the new pool), distinct,
    pool_bytes, records (the entries of new_rec_off).  SebError (RANGE) carries sizes / seg_base / seg_bytes as
    `.compacted` where a capacity is below the need."""
    base, size = (np.ascontiguousarray(a, dtype=np.uint64) for a in (seg_base, seg_bytes))
    s = base.size
    out = s - num_compact + 1
    nbase, nsize = np.zeros(max(out, 1), np.uint64), np.zeros(max(out, 1), np.uint64)
    sz, distinct = seb_segcompact_sizes(), _u64(0)
    cap = (_nbytes(dst_pool) if dst_pool is not None else 0) if dst_cap is None else dst_cap
    rc = lib().seb_hidx_compact(self._p, _ptr(dev_pool), pool_bytes, _np_ptr(base), _np_ptr(size), s, num_compact,
                                _ptr(rest_rec_off), _ptr(rest_live), rest_records, timestamp, _ptr(dst_pool), cap, _ptr(dev_table),
                                capacity, _ptr(new_rec_off), _nbytes(new_rec_off) // 8 if new_rec_off is not None else 0,
                                C.byref(sz), _np_ptr(nbase), _np_ptr(nsize), C.byref(distinct))
    got = dict(sizes=sz.as_dict(), seg_base=nbase[:out], seg_bytes=nsize[:out])
    if rc < 0:
        err = SebError(rc, last_error())
        err.compacted = got
        raise err
    got.update(distinct=distinct.value, pool_bytes=int(nbase[out - 1] + nsize[out - 1]), records=sz.survivors + rest_records)
    return got


Ctx.hidx_compact = _ctx_hidx_compact


class HashIndex:
    """The read side of the reference's hash index on one device: the segment pool and the key table live in device
    memory.  recover(segments) is hashindex's recover(); get_batch(keys) is HashIndex.Get for a batch, ending in the
    values gather (dev_get_values_*) with the segment pool as its pool; insert(tail) takes records appended to the
    active (last) segment."""

    def __init__(self, device: int = 0):
        self._ctx = Ctx(device)
        self.device = device
        self.pool = self.table = None
        self.pool_bytes = self.capacity = self.count = 0
        self.segment_sizes = np.zeros(0, np.uint64)
        self.segment_limit = SEG_NO_LIMIT  # put_batch's rotation limit (SegmentSizeBytes)
        self._seg_bytes = []  # the bytes each segment takes in the pool (a cut segment keeps its image's)
        self._images, self._runs = None, []  # the recovered images and every insert's (rec_off, live, n) device tensors:
                                             # what a rebuild into a larger table needs

    def close(self):
        self._ctx.close()
        self.pool = self.table = None
        self._runs = []

    def recover(self, segments, slack_bytes: int = 0, capacity: int | None = None) -> dict:
        """The segment images (bytes or u8 arrays, oldest first).  slack_bytes: room kept behind the pool for
        insert().  Returns Ctx.hidx_recover's dict; `count` and `segment_sizes` (size_after) are set from it."""
        import torch
        imgs = [_bytes_arg(s) for s in segments]
        total = sum(a.size for a in imgs)
        dev = torch.device("cuda", self.device)
        self.pool = torch.zeros(max(total + slack_bytes, 16), dtype=torch.uint8, device=dev)
        self.pool_bytes = total
        cap = max(total // 64, 16) if capacity is None else capacity
        while True:
            self.capacity = cap
            self.table = torch.empty(dev_hidx_table_bytes(cap), dtype=torch.uint8, device=dev)
            try:
                got = self._ctx.hidx_recover(imgs, self.pool, self.table, cap, pool_cap=self.pool.numel())
                break
            except SebError as e:
                if e.code != -4 or not hasattr(e, "recovered") or e.recovered["live_records"] <= cap:
                    raise
                cap = e.recovered["live_records"]  # cannot fill again
        self.count = got["distinct"]
        self.segment_sizes = got["size_after"].copy()
        self._seg_bytes = [a.size for a in imgs]
        self._images, self._runs = imgs, []  # a rebuild into a larger table scans and verifies them again (_insert_all)
        return got

    def _materialize(self):
        import torch
        if self._images is not None:  # the recovered segments' records, as the device arrays an insert takes
            dev = self.pool.device
            pool, rec_off, first, base, size, _ = segs_scan(self._images)
            live = seg_verify(pool, rec_off, first, base, size)[3]
            self._runs.insert(0, (torch.from_numpy(rec_off.view(np.int64).copy()).to(dev), torch.from_numpy(live.copy()).to(dev),
                                  rec_off.size))
            self._images = None

    def _insert_all(self):
        self._materialize()
        dev_hidx_clear(self.table, self.capacity)
        for rec_off, live, n in self._runs:
            if n:
                dev_hidx_insert(self.table, self.capacity, self.pool, self.pool_bytes, rec_off, live, n)
        return dev_hidx_count(self.table, self.capacity)[0]

    def insert(self, tail) -> int:
        """Records appended to the active segment: `tail` is the bytes written behind it (whole records; a bad one
        cuts the tail there, as recover would).  Returns the number of records that went in."""
        import torch
        buf = _bytes_arg(tail)
        if self.pool is None or self.pool_bytes + buf.size > self.pool.numel():
            raise ValueError("the pool has no room for the tail: recover with slack_bytes")
        dev = self.pool.device
        rec_off, _ = seg_scan(buf, self.pool_bytes)
        n = rec_off.size
        self.pool[self.pool_bytes: self.pool_bytes + buf.size] = torch.from_numpy(buf.copy()).to(dev)
        self.pool_bytes += buf.size
        if self._seg_bytes:
            self._seg_bytes[-1] += buf.size
        if n == 0:
            return 0
        d_off = torch.from_numpy(rec_off.view(np.int64).copy()).to(dev)
        d_first = torch.tensor([0, n], dtype=torch.int64, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        live = torch.empty(n, dtype=torch.uint8, device=dev)
        valid = torch.empty(1, dtype=torch.int64, device=dev)
        dev_seg_verify(self.pool, self.pool_bytes, d_off, n, d_first, 1, ok, valid, live)
        self._runs.append((d_off, live, n))
        dev_hidx_insert(self.table, self.capacity, self.pool, self.pool_bytes, d_off, live, n)
        try:
            self.count = dev_hidx_count(self.table, self.capacity)[0]
        except SebError as e:
            if e.code != -4:
                raise
            self.capacity = max(2 * self.capacity, self.count + n)
            self.table = torch.empty(dev_hidx_table_bytes(self.capacity), dtype=torch.uint8, device=dev)
            self.count = self._insert_all()
        took = int(valid.cpu()[0])
        if len(self.segment_sizes):
            self.segment_sizes[-1] += np.uint64(buf.size if took == n else int(rec_off[took]) - int(rec_off[0]))
        return took

    def get_batch(self, keys, verify: bool = True):
        """HashIndex.Get for a key batch (anything as_keys takes): (status u8, out_off u64 n + 1, out_vals u8): key
        i's value is out_vals[out_off[i]: out_off[i + 1]] where status[i] == GET_FOUND; GET_ERROR is a CRC mismatch."""
        import torch
        kb = as_keys(keys)
        n = kb.n
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8)
        dev = self.pool.device
        data = torch.from_numpy(kb.data.reshape(-1).copy() if kb.data.size else np.zeros(1, np.uint8)).to(dev)
        if kb.offsets is not None:
            dk = dev_keys(data, torch.from_numpy(kb.offsets.view(np.int64).copy()).to(dev))
        else:
            dk = dev_keys(data, n=n, stride=kb.stride)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        source = torch.empty(n, dtype=torch.uint8, device=dev)
        vloc = torch.empty(n, dtype=torch.int64, device=dev)
        vlen = torch.empty(n, dtype=torch.int32, device=dev)
        dev_hidx_get(self.table, self.capacity, self.pool, self.pool_bytes, dk, verify, status, None, vloc, vlen, source)
        ws = torch.empty(dev_get_values_workspace_size(n), dtype=torch.uint8, device=dev)
        sz = dev_get_values_plan(status, source, None, vloc, vlen, n, [], self.pool, ws, pool_bytes=self.pool_bytes)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        out_vals = torch.empty(max(sz.val_bytes, 1), dtype=torch.uint8, device=dev)
        dev_get_values_emit(status, source, None, vloc, vlen, n, [], self.pool, sz, ws, out_off, out_vals if sz.val_bytes else None,
                            pool_bytes=self.pool_bytes)
        torch.cuda.synchronize(dev)
        return status.cpu().numpy(), out_off.cpu().numpy().view(np.uint64), out_vals.cpu().numpy()[: sz.val_bytes]


    # ------------------------------------------------ the write side

    def _count_or_grow(self, added: int) -> None:
        import torch
        try:
            self.count = dev_hidx_count(self.table, self.capacity)[0]
        except SebError as e:
            if e.code != -4:
                raise
            self.capacity = max(2 * self.capacity, self.count + added)
            self.table = torch.empty(dev_hidx_table_bytes(self.capacity), dtype=torch.uint8, device=self.pool.device)
            self.count = self._insert_all()

    def put_batch(self, keys, vals, val_off, deleted=None, timestamp: int = 0):
        """HashIndex.Put / Delete for a batch (ops as seg_frame takes them, host memory): framed and sealed on the device
        straight behind the pool, verified, inserted.  Rotation at `segment_limit`.  Returns (image u8, rec_off u64 of
        n + 1 offsets within the image, cuts u64): the engine appends image[:rec_off[cuts[0]]] to its active file and
        opens a new file at every cut."""
        import torch
        kb, va, vo, de = _ops_host_args(keys, vals, val_off, deleted)
        n = kb.n
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        dev = torch.device("cuda", self.device)
        if self.pool is None:
            self.pool = torch.zeros(16, dtype=torch.uint8, device=dev)
            self.capacity = max(n, 16)
            self.table = torch.zeros(dev_hidx_table_bytes(self.capacity), dtype=torch.uint8, device=dev)
        if not self._seg_bytes:
            self._seg_bytes, self.segment_sizes = [0], np.zeros(1, np.uint64)
        data = torch.from_numpy(kb.data.reshape(-1).copy() if kb.data.size else np.zeros(1, np.uint8)).to(dev)
        if kb.offsets is not None:
            dk = dev_keys(data, torch.from_numpy(kb.offsets.view(np.int64).copy()).to(dev))
        else:
            dk = dev_keys(data, n=n, stride=kb.stride)
        d_vals = torch.from_numpy(va.copy() if va.size else np.zeros(1, np.uint8)).to(dev)
        d_voff = torch.from_numpy(vo.view(np.int64).copy()).to(dev)
        d_del = None if de is None else torch.from_numpy(de.copy()).to(dev)
        d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total, cuts = dev_seg_frame_plan(dk, d_voff, d_del, d_off, int(self._seg_bytes[-1]), self.segment_limit)
        if self.pool_bytes + total > self.pool.numel():
            grown = torch.zeros(max(2 * self.pool.numel(), self.pool_bytes + total), dtype=torch.uint8, device=dev)
            grown[: self.pool_bytes] = self.pool[: self.pool_bytes]
            self.pool = grown
        at = self.pool_bytes
        image = self.pool[at: at + total]
        dev_seg_frame_emit(dk, d_vals, d_voff, d_del, timestamp, d_off, image, total)
        self.pool_bytes += total
        p_off = (d_off[:n] + at).contiguous()
        d_first = torch.tensor([0, n], dtype=torch.int64, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        live = torch.empty(n, dtype=torch.uint8, device=dev)
        valid = torch.empty(1, dtype=torch.int64, device=dev)
        dev_seg_verify(self.pool, self.pool_bytes, p_off, n, d_first, 1, ok, valid, live)
        self._materialize()
        self._runs.append((p_off, live, n))
        dev_hidx_insert(self.table, self.capacity, self.pool, self.pool_bytes, p_off, live, n)
        self._count_or_grow(n)
        rec_off = d_off.cpu().numpy().view(np.uint64)
        edges = [0] + [int(rec_off[int(c)]) for c in cuts] + [total]
        sizes = [edges[i + 1] - edges[i] for i in range(len(edges) - 1)]
        self._seg_bytes[-1] += sizes[0]
        self._seg_bytes += sizes[1:]
        self.segment_sizes = np.concatenate([self.segment_sizes, np.zeros(len(sizes) - 1, np.uint64)])
        self.segment_sizes[len(self.segment_sizes) - len(sizes):] += np.array(sizes, np.uint64)
        return image.cpu().numpy(), rec_off, cuts

    def compact(self, num_segments: int, timestamp: int = 0) -> dict:
        """compactSegments + applyCompaction for the oldest num_segments segments: their live records' survivors
        become one new segment at the front of a new pool, the other segments follow it unchanged, and the table
        is rebuilt from everything (linear probing has no delete).  Every Get answers as before; `count` drops by
        the keys whose latest record was a tombstone in a compacted segment.  Returns the compaction's sizes."""
        import torch
        c = num_segments
        if self.pool is None or not 1 <= c <= len(self._seg_bytes):
            raise ValueError(f"compact({c}) of {len(self._seg_bytes)} segments")
        self._materialize()
        dev = self.pool.device
        edge = int(sum(int(b) for b in self._seg_bytes[:c]))  # where the first segment that stays begins
        runs = [r for r in self._runs if r[2]]
        rec = torch.cat([r[0][: r[2]] for r in runs]) if runs else torch.zeros(0, dtype=torch.int64, device=dev)
        live = torch.cat([r[1][: r[2]] for r in runs]) if runs else torch.zeros(0, dtype=torch.uint8, device=dev)
        n_c = int((rec < edge).sum())  # the runs lie in pool order: the compacted segments' records come first
        head_off, head_live = rec[:n_c].contiguous(), live[:n_c].contiguous()
        ws = torch.empty(max(dev_seg_compact_workspace_size(n_c), 16), dtype=torch.uint8, device=dev)
        sz = dev_seg_compact_plan(self.pool, self.pool_bytes, head_off if n_c else None, head_live if n_c else None, n_c, ws)
        rest = self.pool_bytes - edge
        total = sz.image_bytes + rest
        pool = torch.zeros(max(total + self.pool.numel() - self.pool_bytes, 16), dtype=torch.uint8, device=dev)
        out_off = torch.empty(sz.survivors + 1, dtype=torch.int64, device=dev)
        dev_seg_compact_emit(self.pool, self.pool_bytes, head_off if n_c else None, n_c, timestamp, sz, ws,
                             pool if sz.image_bytes else None, out_off)
        pool[sz.image_bytes: total] = self.pool[edge: self.pool_bytes]
        rest_off = (rec[n_c:] - edge + sz.image_bytes).contiguous()
        ones = torch.ones(sz.survivors, dtype=torch.uint8, device=dev)
        self.pool, self.pool_bytes = pool, total
        self._runs = [(out_off[: sz.survivors].contiguous(), ones, sz.survivors), (rest_off, live[n_c:].contiguous(), rec.numel() - n_c)]
        self._seg_bytes = [sz.image_bytes] + list(self._seg_bytes[c:])
        self.segment_sizes = np.concatenate([np.array([sz.image_bytes], np.uint64), self.segment_sizes[c:]])
        self.count = self._insert_all()
        return sz.as_dict()

    def logical_size(self) -> int:
        """getLogicalSize: keySize + valueSize over the index, tombstoned keys included."""
        return dev_hidx_logical_size(self.table, self.capacity, self.pool, self.pool_bytes)


# ------------------------------- B-tree, read side: a page-file image checked, Get of a key batch (btree/)

def bt_open(image) -> seb_bt_meta:
    """readMetadata (btree/pager.go:142-164) of a page-file image on the host: the seb_bt_meta every other call takes
    (.root, .header_pages, .free_list, .num_pages = min(NumPages, the image's whole pages)).  SebError (INVALID) where
    the reference gives ErrInvalidDatabase."""
    img = _bytes_arg(image)
    meta = seb_bt_meta()
    check(lib().seb_bt_open(_np_ptr(img), img.size, C.byref(meta)))
    return meta


def bt_check(image, meta: seb_bt_meta):
    """The structural pass on the host: (kind u8, level u8, stats dict), one kind and one level per page."""
    img = _bytes_arg(image)
    kind, level = np.zeros(meta.num_pages, np.uint8), np.zeros(meta.num_pages, np.uint8)
    st = seb_bt_stats()
    check(lib().seb_bt_check(_np_ptr(img), img.size, C.byref(meta), _np_ptr(kind), _np_ptr(level), C.byref(st)))
    return kind, level, st.as_dict()


def bt_get(image, meta: seb_bt_meta, keys):
    """BTree.Get for a key batch on the host: (status u8, leaf u32, pos u32, vloc u64, vlen u32).  The reference for
    dev_bt_get."""
    img = _bytes_arg(image)
    kb = as_keys(keys)
    n = kb.n
    status, leaf, pos = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    vloc, vlen = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    check(lib().seb_bt_get(_np_ptr(img), img.size, C.byref(meta), kb.ref, _np_ptr(status), _np_ptr(leaf), _np_ptr(pos),
                           _np_ptr(vloc), _np_ptr(vlen)))
    return status, leaf, pos, vloc, vlen


def dev_bt_check(image, image_bytes: int, meta: seb_bt_meta, kind=None, level=None, stream=None) -> dict:
    """The structural pass on a device image: kind / level (u8 tensors of meta.num_pages, nullable) are filled,
    the stats come back as a dict.  Synchronises."""
    for name, t in (("kind", kind), ("level", level)):
        if t is not None and _nbytes(t) < meta.num_pages:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, the image has {meta.num_pages} pages")
    st = seb_bt_stats()
    check(lib().seb_dev_bt_check(_ptr(image), image_bytes, C.byref(meta), _ptr(kind), _ptr(level), C.byref(st), _stream(stream)))
    return st.as_dict()


def dev_bt_get(image, image_bytes: int, meta: seb_bt_meta, keys: seb_keys, status, leaf=None, pos=None, vloc=None, vlen=None,
               source=None, stream=None) -> None:
    """BTree.Get for a device key batch: status (u8), leaf / pos (u32), vloc (u64), vlen (u32), source (u8), each of
    keys.n elements; all but status nullable.  Not synchronised."""
    n = keys.n
    for name, t, size in (("status", status, n), ("leaf", leaf, 4 * n), ("pos", pos, 4 * n), ("vloc", vloc, 8 * n),
                          ("vlen", vlen, 4 * n), ("source", source, n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {n} keys need {size}")
    check(lib().seb_dev_bt_get(_ptr(image), image_bytes, C.byref(meta), C.byref(keys), _ptr(status), _ptr(leaf), _ptr(pos),
                               _ptr(vloc), _ptr(vlen), _ptr(source), _stream(stream)))


# ------------------------------- B-tree, range scans: the leaf directory, Scan of a batch of ranges (btree/iterator.go)

def bt_dir_bytes(num_pages: int) -> int:
    return lib().seb_bt_dir_bytes(num_pages)


def bt_dir_build(image, meta: seb_bt_meta, kind, level):
    """The leaf directory of a checked image on the host: (dir u8 of bt_dir_bytes(meta.num_pages), info dict with
    leaves, keys, depth).  kind / level: bt_check's arrays.  A refused image raises SebError (INVALID) naming the
    page.  The reference for dev_bt_dir_build: both write the same bytes."""
    img = _bytes_arg(image)
    kd, lv = np.ascontiguousarray(kind, dtype=np.uint8), np.ascontiguousarray(level, dtype=np.uint8)
    if kd.size < meta.num_pages or lv.size < meta.num_pages:
        raise ValueError(f"kind / level hold {kd.size} / {lv.size} bytes, the image has {meta.num_pages} pages")
    d = np.zeros(bt_dir_bytes(meta.num_pages) // 8, np.uint64).view(np.uint8)
    info = seb_bt_dir_info()
    check(lib().seb_bt_dir_build(_np_ptr(img), img.size, C.byref(meta), _np_ptr(kd), _np_ptr(lv), _np_ptr(d), C.byref(info)))
    return d, info.as_dict()


def _bound_keys(keys) -> HostKeys:
    """A batch of bounds: every one may be empty, and a batch without a byte still needs a data pointer."""
    kb = as_keys(keys)
    if kb.offsets is not None and kb.data.size == 0:
        kb = HostKeys(np.zeros(1, np.uint8), kb.offsets)
    return kb


def bt_scan(image, meta: seb_bt_meta, dir, starts, ends, limit: int = 0, caps=None):
    """BTree.Scan for a batch of ranges [start, end) on the host (an empty start: from the first key; an empty end:
    unbounded; limit 0: none).  Returns a dict: range_status (u8), range_off (u64, R + 1), the entries' status, source,
    kloc, klen, vloc, vlen, the dense key_off / keys and val_off / vals, and sizes = (ranges, entries, key_bytes,
    val_bytes).  caps = (entry_cap, key_cap, val_cap) sizes the outputs instead of a sizing call: below the need it
    raises SebError (RANGE) with `.sizes` set for the retry.  The reference for dev_bt_scan_plan / _cells."""
    img = _bytes_arg(image)
    d = np.ascontiguousarray(dir, dtype=np.uint8)
    ks, ke = _bound_keys(starts), _bound_keys(ends)
    R = ks.n
    rs, ro = np.zeros(R, np.uint8), np.zeros(R + 1, np.uint64)
    sz = seb_bt_scan_sizes()
    head = (_np_ptr(img), img.size, C.byref(meta), _np_ptr(d), ks.ref, ke.ref, limit, _np_ptr(rs), _np_ptr(ro))
    if caps is None:
        rc = lib().seb_bt_scan(*head, None, None, None, None, None, None, 0, None, None, 0, None, None, 0, C.byref(sz))
        if rc < 0 and not (rc == -4 and sz.entries < 2**32):
            raise SebError(rc, last_error())
        caps = (sz.entries, sz.key_bytes, sz.val_bytes)
    ec, kc, vc = caps
    st, so = np.zeros(ec, np.uint8), np.zeros(ec, np.uint8)
    kl, vl = np.zeros(ec, np.uint64), np.zeros(ec, np.uint64)
    kn, vn = np.zeros(ec, np.uint32), np.zeros(ec, np.uint32)
    ko, vo = np.zeros(ec + 1, np.uint64), np.zeros(ec + 1, np.uint64)
    kb, vb = np.zeros(max(kc, 1), np.uint8), np.zeros(max(vc, 1), np.uint8)
    rc = lib().seb_bt_scan(*head, _np_ptr(st), _np_ptr(so), _np_ptr(kl), _np_ptr(kn), _np_ptr(vl), _np_ptr(vn), ec, _np_ptr(ko),
                           _np_ptr(kb), kc, _np_ptr(vo), _np_ptr(vb), vc, C.byref(sz))
    if rc < 0:
        err = SebError(rc, last_error())
        err.sizes = sz.as_tuple()
        raise err
    n = sz.entries
    return dict(range_status=rs, range_off=ro, status=st[:n], source=so[:n], kloc=kl[:n], klen=kn[:n], vloc=vl[:n], vlen=vn[:n],
                key_off=ko[: n + 1], keys=kb[: sz.key_bytes], val_off=vo[: n + 1], vals=vb[: sz.val_bytes], sizes=sz.as_tuple())


def dev_bt_dir_workspace_size(num_pages: int) -> int:
    return lib().seb_dev_bt_dir_workspace_size(num_pages)


def dev_bt_dir_build(image, image_bytes: int, meta: seb_bt_meta, kind, level, dir, ws, ws_bytes: int | None = None,
                     stream=None) -> dict:
    """The leaf directory of a checked device image into `dir` (u8 tensor of bt_dir_bytes(meta.num_pages), 8-byte
    aligned); kind / level as dev_bt_check wrote them; ws: dev_bt_dir_workspace_size(meta.num_pages) bytes, 16-byte
    aligned.  Synchronises; returns the info dict; a refused image raises SebError (INVALID) naming the page."""
    for name, t, size in (("kind", kind, meta.num_pages), ("level", level, meta.num_pages), ("dir", dir, bt_dir_bytes(meta.num_pages))):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, {meta.num_pages} pages need {size}")
    info = seb_bt_dir_info()
    check(lib().seb_dev_bt_dir_build(_ptr(image), image_bytes, C.byref(meta), _ptr(kind), _ptr(level), _ptr(dir), _ptr(ws),
                                     (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes, C.byref(info),
                                     _stream(stream)))
    return info.as_dict()


def dev_bt_scan_workspace_size(ranges: int) -> int:
    return lib().seb_dev_bt_scan_workspace_size(ranges)


def dev_bt_scan_plan(image, image_bytes: int, meta: seb_bt_meta, dir, starts: seb_keys, ends: seb_keys, limit: int,
                     range_status, ws, ws_bytes: int | None = None, stream=None) -> seb_bt_scan_sizes:
    """Sizes a batch of ranges (device key batches of equal n): range_status (u8, n) is written, the plan goes into
    `ws` (dev_bt_scan_workspace_size(n) bytes, 8-byte aligned).  Synchronises; returns the sizes (.ranges, .entries)
    that dev_bt_scan_cells takes.  2^32 entries or more: SebError (RANGE)."""
    if range_status is not None and _nbytes(range_status) < starts.n:
        raise ValueError(f"range_status holds {_nbytes(range_status)} bytes, {starts.n} ranges")
    sz = seb_bt_scan_sizes()
    check(lib().seb_dev_bt_scan_plan(_ptr(image), image_bytes, C.byref(meta), _ptr(dir), C.byref(starts), C.byref(ends), limit,
                                     _ptr(range_status), _ptr(ws), (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                     C.byref(sz), _stream(stream)))
    return sz


def dev_bt_scan_cells(image, image_bytes: int, meta: seb_bt_meta, dir, sizes: seb_bt_scan_sizes, ws, range_off, status, source,
                      kloc, klen, vloc, vlen, ws_bytes: int | None = None, stream=None) -> None:
    """Writes range_off (u64, ranges + 1) and per entry status / source (u8), kloc / vloc (u64), klen / vlen (u32) from
    the plan in `ws`: the arrays dev_get_values_* take with the image as pool.  Not synchronised."""
    n = sizes.entries
    for name, t, size in (("range_off", range_off, 8 * (sizes.ranges + 1)), ("status", status, n), ("source", source, n),
                          ("kloc", kloc, 8 * n), ("klen", klen, 4 * n), ("vloc", vloc, 8 * n), ("vlen", vlen, 4 * n)):
        if t is not None and _nbytes(t) < size:
            raise ValueError(f"{name} holds {_nbytes(t)} bytes, the plan needs {size}")
    check(lib().seb_dev_bt_scan_cells(_ptr(image), image_bytes, C.byref(meta), _ptr(dir), C.byref(sizes), _ptr(ws),
                                      (_nbytes(ws) if ws is not None else 0) if ws_bytes is None else ws_bytes, _ptr(range_off),
                                      _ptr(status), _ptr(source), _ptr(kloc), _ptr(klen), _ptr(vloc), _ptr(vlen), _stream(stream)))


def _ctx_bt_load(self, image, dev_image, dev_kind=None, dev_level=None, cap: int | None = None):
    """seb_bt_load: a host image opened, uploaded into dev_image and checked.  Returns (meta, stats dict)."""
    img = _bytes_arg(image)
    meta, st = seb_bt_meta(), seb_bt_stats()
    cap = (_nbytes(dev_image) if dev_image is not None else 0) if cap is None else cap
    check(lib().seb_bt_load(self._p, _np_ptr(img), img.size, _ptr(dev_image), cap, _ptr(dev_kind), _ptr(dev_level),
                            C.byref(meta), C.byref(st)))
    return meta, st.as_dict()


Ctx.bt_load = _ctx_bt_load


class BTreeImage:
    """The read side of the reference's B-tree on one device: the page-file image lives in device memory.
    open(image) is readMetadata + upload + the structural check + the leaf directory; check() runs the check again;
    get_batch(keys) is BTree.Get for a batch, ending in the values gather (dev_get_values_*) with the image as its pool;
    scan_batch(starts, ends) is BTree.Scan for a batch of ranges through the directory, ending in two such gathers.
    An image whose directory is refused still opens: `dir` is None, `dir_error` keeps the message, get_batch works."""

    def __init__(self, device: int = 0):
        self._ctx = Ctx(device)
        self.device = device
        self.image = self.kind = self.level = self.meta = None
        self.dir, self.dir_info, self.dir_error = None, {}, None
        self.image_bytes = 0
        self.stats = {}

    def close(self):
        self._ctx.close()
        self.image = self.kind = self.level = self.dir = None

    def open(self, image) -> dict:
        """The file's bytes (what Sync wrote, any WAL already applied).  Returns the check's stats; `meta`, `kind`
        and `level` (device tensors, one byte per page) are set."""
        import torch
        img = _bytes_arg(image)
        dev = torch.device("cuda", self.device)
        pages = img.size // BT_PAGE_BYTES
        self.image = torch.empty(max(pages * BT_PAGE_BYTES, 16), dtype=torch.uint8, device=dev)
        self.kind = torch.empty(max(pages, 1), dtype=torch.uint8, device=dev)
        self.level = torch.empty(max(pages, 1), dtype=torch.uint8, device=dev)
        self.meta, self.stats = self._ctx.bt_load(img, self.image, self.kind, self.level)
        self.image_bytes = self.meta.num_pages * BT_PAGE_BYTES
        self._build_dir()
        return self.stats

    def _build_dir(self):
        import torch
        dev, pages = self.image.device, self.meta.num_pages
        d = torch.empty(bt_dir_bytes(pages), dtype=torch.uint8, device=dev)
        ws = torch.empty(dev_bt_dir_workspace_size(pages), dtype=torch.uint8, device=dev)
        self.dir, self.dir_info, self.dir_error = None, {}, None
        try:
            self.dir_info = dev_bt_dir_build(self.image, self.image_bytes, self.meta, self.kind, self.level, d, ws)
            self.dir = d
        except SebError as e:
            if e.code != -1:
                raise
            self.dir_error = str(e)

    def check(self) -> dict:
        self.stats = dev_bt_check(self.image, self.image_bytes, self.meta, self.kind, self.level)
        return self.stats

    def _dev_keys(self, keys):
        import torch
        kb = as_keys(keys)
        dev = self.image.device
        data = torch.from_numpy(kb.data.reshape(-1).copy() if kb.data.size else np.zeros(1, np.uint8)).to(dev)
        if kb.offsets is not None:
            return dev_keys(data, torch.from_numpy(kb.offsets.view(np.int64).copy()).to(dev))
        return dev_keys(data, n=kb.n, stride=kb.stride)

    def _gather(self, status, source, loc, length, n):
        import torch
        dev = self.image.device
        ws = torch.empty(dev_get_values_workspace_size(n), dtype=torch.uint8, device=dev)
        sz = dev_get_values_plan(status, source, None, loc, length, n, [], self.image, ws, pool_bytes=self.image_bytes)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        out = torch.empty(max(sz.val_bytes, 1), dtype=torch.uint8, device=dev)
        dev_get_values_emit(status, source, None, loc, length, n, [], self.image, sz, ws, off, out if sz.val_bytes else None,
                            pool_bytes=self.image_bytes)
        return off, out, sz.val_bytes

    def scan_batch(self, starts, ends, limit: int = 0):
        """BTree.Scan for a batch of ranges [start, end) (anything as_keys takes; an empty start: from the first key;
        an empty end: unbounded; limit 0: none): (range_status u8, range_off u64 R + 1, key_off u64, keys u8, val_off
        u64, vals u8).  Range r's entries are [range_off[r], range_off[r + 1]); entry e's key is keys[key_off[e]:
        key_off[e + 1]], its value vals[val_off[e]: val_off[e + 1]].  range_status[r] == GET_ERROR: a bound's walk met a
        page the image does not hold whole.  Raises SebError where the image's directory was refused."""
        import torch
        if self.dir is None:
            raise SebError(-1, self.dir_error or "BTreeImage.scan_batch: no image is open")
        ks, ke = self._dev_keys(starts), self._dev_keys(ends)
        R = ks.n
        dev = self.image.device
        zero = np.zeros(1, np.uint64)
        if R == 0:
            return np.zeros(0, np.uint8), zero, zero.copy(), np.zeros(0, np.uint8), zero.copy(), np.zeros(0, np.uint8)
        rs = torch.empty(R, dtype=torch.uint8, device=dev)
        ws = torch.empty(dev_bt_scan_workspace_size(R), dtype=torch.uint8, device=dev)
        sz = dev_bt_scan_plan(self.image, self.image_bytes, self.meta, self.dir, ks, ke, limit, rs, ws)
        n = sz.entries
        ro = torch.empty(R + 1, dtype=torch.int64, device=dev)
        st, so = torch.empty(max(n, 1), dtype=torch.uint8, device=dev), torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        kl, vl = torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        kn, vn = torch.empty(max(n, 1), dtype=torch.int32, device=dev), torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        dev_bt_scan_cells(self.image, self.image_bytes, self.meta, self.dir, sz, ws, ro, st, so, kl, kn, vl, vn)
        if n == 0:
            torch.cuda.synchronize(dev)
            return (rs.cpu().numpy(), ro.cpu().numpy().view(np.uint64), zero, np.zeros(0, np.uint8), zero.copy(),
                    np.zeros(0, np.uint8))
        ko, kb, kbytes = self._gather(st, so, kl, kn, n)
        vo, vb, vbytes = self._gather(st, so, vl, vn, n)
        torch.cuda.synchronize(dev)
        return (rs.cpu().numpy(), ro.cpu().numpy().view(np.uint64), ko.cpu().numpy().view(np.uint64), kb.cpu().numpy()[:kbytes],
                vo.cpu().numpy().view(np.uint64), vb.cpu().numpy()[:vbytes])

    def get_batch(self, keys):
        """BTree.Get for a key batch (anything as_keys takes): (status u8, out_off u64 n + 1, out_vals u8): key i's
        value is out_vals[out_off[i]: out_off[i + 1]] where status[i] == GET_FOUND; GET_ERROR is an empty key or a
        walk that met a page or a cell the image does not hold whole."""
        import torch
        kb = as_keys(keys)
        n = kb.n
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8)
        dev = self.image.device
        data = torch.from_numpy(kb.data.reshape(-1).copy() if kb.data.size else np.zeros(1, np.uint8)).to(dev)
        if kb.offsets is not None:
            dk = dev_keys(data, torch.from_numpy(kb.offsets.view(np.int64).copy()).to(dev))
        else:
            dk = dev_keys(data, n=n, stride=kb.stride)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        source = torch.empty(n, dtype=torch.uint8, device=dev)
        vloc = torch.empty(n, dtype=torch.int64, device=dev)
        vlen = torch.empty(n, dtype=torch.int32, device=dev)
        dev_bt_get(self.image, self.image_bytes, self.meta, dk, status, None, None, vloc, vlen, source)
        ws = torch.empty(dev_get_values_workspace_size(n), dtype=torch.uint8, device=dev)
        sz = dev_get_values_plan(status, source, None, vloc, vlen, n, [], self.image, ws, pool_bytes=self.image_bytes)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        out_vals = torch.empty(max(sz.val_bytes, 1), dtype=torch.uint8, device=dev)
        dev_get_values_emit(status, source, None, vloc, vlen, n, [], self.image, sz, ws, out_off, out_vals if sz.val_bytes else None,
                            pool_bytes=self.image_bytes)
        torch.cuda.synchronize(dev)
        return status.cpu().numpy(), out_off.cpu().numpy().view(np.uint64), out_vals.cpu().numpy()[: sz.val_bytes]
