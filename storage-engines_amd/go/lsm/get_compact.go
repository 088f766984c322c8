// The step between a GetBatch's memtable lookup and its SSTable steps, over the Get path group of libseb_bloom
// (include/seb_bloom.h): LSM.Get returns at the first memtable that holds the key (lsm/lsm.go:144-166) and reads
// no filter, index or block for it, so only the keys the memtables leave undecided go on.
//
//	compact  the undecided keys of a batch, in batch order, as a dense batch plus row[j] = the batch index of
//	         compacted key j (seb_get_compact on host memory; seb_dev_get_compact_plan / _emit on device memory)
//	join     the SSTables' answers for the compacted keys put back on their batch rows, the memtables' answers on
//	         the others (seb_get_join_rows; seb_dev_get_join_rows)
//
// The call order of a GetBatch that keeps its batch on the device: seb_dev_runs_search, CompactPlan, CompactEmit,
// FilterRegistry's MultiGet list, locate, block search and resolve on the m compacted keys, JoinRows.
//
// No departure from the reference: per key the answer is seb_dev_get_join's over the whole batch.
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_getpath.py, tests/test_gpu_getpath.py).
package lsm

/*
#include <stdint.h>
#include <stdlib.h>
#include "seb_bloom.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// CompactSizes is seb_compact_sizes: what a plan returns and an emit takes.
type CompactSizes struct {
	N, Undecided, KeyBytes uint64
}

// GetAnswer is LSM.Get's answer for one key of a batch after the join.
type GetAnswer struct {
	Status uint8  // SEB_GET_MISS, SEB_GET_FOUND or SEB_GET_ERROR
	Source uint8  // 0: the memtables decided; 1: the SSTables' answer stands
	Col    uint16 // the deciding file's column of the key's candidate row, 0xFFFF for none
	VLoc   uint64 // the value's place: in its run's value bytes (Source 0) or in the block pool (Source 1)
	VLen   uint32
}

func u32Ptr(s []uint32) *C.uint32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&s[0]))
}

// compactUndecided is the host half: the keys whose memtable status is neither found nor tombstone, in batch
// order, packed like packKeys packs a batch, and each one's index in `keys`.
func compactUndecided(keys []string, memStatus []byte) (data []byte, offs []uint64, row []uint32, err error) {
	if len(memStatus) != len(keys) {
		return nil, nil, nil, fmt.Errorf("failed to compact keys: %d statuses for %d keys", len(memStatus), len(keys))
	}
	in, inOffs := packKeys(keys)
	kb := C.seb_keys{data: bytesPtr(in), offsets: u64Ptr(inOffs), n: C.uint64_t(len(keys))}
	var sz C.seb_compact_sizes
	if C.seb_get_compact(&kb, bytesPtr(memStatus), &sz, nil, 0, nil, nil, 0) != 0 { // the plan: sizes only
		return nil, nil, nil, fmt.Errorf("failed to compact keys: %s", C.GoString(C.seb_last_error()))
	}
	data = make([]byte, sz.key_bytes)
	offs = make([]uint64, sz.undecided+1)
	row = make([]uint32, sz.undecided)
	if C.seb_get_compact(&kb, bytesPtr(memStatus), &sz, bytesPtr(data), sz.key_bytes, u64Ptr(offs), u32Ptr(row),
		sz.undecided) != 0 {
		return nil, nil, nil, fmt.Errorf("failed to compact keys: %s", C.GoString(C.seb_last_error()))
	}
	return data, offs, row, nil
}

// joinRows is the host half of the row-mapped join: mem* are per batch key (getBatchMemtables' answers), sst* per
// compacted key (FilterRegistry.SearchBlocks' answers for the keys compactUndecided returned).
func joinRows(memStatus []byte, memVLoc []uint64, memVLen []uint32, row []uint32, sstStatus []byte, sstCol []uint16,
	sstVLoc []uint64, sstVLen []uint32) ([]GetAnswer, error) {
	n := len(memStatus)
	out := make([]GetAnswer, n)
	if n == 0 {
		return out, nil
	}
	status, source := make([]byte, n), make([]byte, n)
	col := make([]uint16, n)
	vloc := make([]uint64, n)
	vlen := make([]uint32, n)
	var colIn *C.uint16_t
	if len(sstCol) != 0 {
		colIn = (*C.uint16_t)(unsafe.Pointer(&sstCol[0]))
	}
	rc := C.seb_get_join_rows(bytesPtr(memStatus), u64Ptr(memVLoc), u32Ptr(memVLen), C.uint64_t(n), u32Ptr(row),
		C.uint64_t(len(row)), bytesPtr(sstStatus), colIn, u64Ptr(sstVLoc), u32Ptr(sstVLen), bytesPtr(status),
		bytesPtr(source), (*C.uint16_t)(unsafe.Pointer(&col[0])), u64Ptr(vloc), u32Ptr(vlen))
	if rc != 0 {
		return nil, fmt.Errorf("failed to join the SSTables' answers: %s", C.GoString(C.seb_last_error()))
	}
	for i := range out {
		out[i] = GetAnswer{Status: status[i], Source: source[i], Col: col[i], VLoc: vloc[i], VLen: vlen[i]}
	}
	return out, nil
}

// The device form: every pointer below is device memory the caller owns (an engine that keeps its batches in
// HBM), `stream` its HIP stream.

// DevCompactWorkspaceSize is the workspace a plan of n keys needs (16-byte aligned device memory).
func DevCompactWorkspaceSize(n uint64) uint64 {
	return uint64(C.seb_dev_get_compact_workspace_size(C.uint64_t(n)))
}

// DevCompactPlan counts the undecided keys of the device batch kb; it synchronises the stream.
func DevCompactPlan(kb *C.seb_keys, memStatus unsafe.Pointer, workspace unsafe.Pointer, workspaceBytes uint64,
	stream unsafe.Pointer) (CompactSizes, error) {
	var sz C.seb_compact_sizes
	if C.seb_dev_get_compact_plan(kb, (*C.uint8_t)(memStatus), workspace, C.uint64_t(workspaceBytes), &sz, stream) != 0 {
		return CompactSizes{}, fmt.Errorf("failed to plan the compaction: %s", C.GoString(C.seb_last_error()))
	}
	return CompactSizes{N: uint64(sz.n), Undecided: uint64(sz.undecided), KeyBytes: uint64(sz.key_bytes)}, nil
}

// DevCompactEmit writes outKeys[0, KeyBytes), outOff[0, Undecided] (nil for a fixed-stride batch) and
// row[0, Undecided); not synchronised.  The compacted batch is {outKeys, outOff, Undecided, kb.stride}.
func DevCompactEmit(kb *C.seb_keys, memStatus unsafe.Pointer, sizes CompactSizes, workspace, outKeys, outOff, row,
	stream unsafe.Pointer) (C.seb_keys, error) {
	sz := C.seb_compact_sizes{n: C.uint64_t(sizes.N), undecided: C.uint64_t(sizes.Undecided),
		key_bytes: C.uint64_t(sizes.KeyBytes)}
	if C.seb_dev_get_compact_emit(kb, (*C.uint8_t)(memStatus), &sz, workspace, (*C.uint8_t)(outKeys),
		(*C.uint64_t)(outOff), (*C.uint32_t)(row), stream) != 0 {
		return C.seb_keys{}, fmt.Errorf("failed to compact keys: %s", C.GoString(C.seb_last_error()))
	}
	out := C.seb_keys{data: (*C.uint8_t)(outKeys), n: C.uint64_t(sizes.Undecided)}
	if kb.offsets != nil {
		out.offsets = (*C.uint64_t)(outOff)
	} else {
		out.stride = kb.stride
	}
	return out, nil
}

// DevJoinRows is seb_dev_get_join_rows: sst* as seb_dev_resolve_rows wrote them for the m compacted keys; source,
// col, vloc and vlen may be nil, and so may memVLoc, memVLen, sstCol, sstVLoc and sstVLen.  Not synchronised.
func DevJoinRows(memStatus, memVLoc, memVLen unsafe.Pointer, n uint64, row unsafe.Pointer, m uint64, sstStatus, sstCol,
	sstVLoc, sstVLen, status, source, col, vloc, vlen, stream unsafe.Pointer) error {
	rc := C.seb_dev_get_join_rows((*C.uint8_t)(memStatus), (*C.uint64_t)(memVLoc), (*C.uint32_t)(memVLen), C.uint64_t(n),
		(*C.uint32_t)(row), C.uint64_t(m), (*C.uint8_t)(sstStatus), (*C.uint16_t)(sstCol), (*C.uint64_t)(sstVLoc),
		(*C.uint32_t)(sstVLen), (*C.uint8_t)(status), (*C.uint8_t)(source), (*C.uint16_t)(col), (*C.uint64_t)(vloc),
		(*C.uint32_t)(vlen), stream)
	if rc != 0 {
		return fmt.Errorf("failed to join the SSTables' answers: %s", C.GoString(C.seb_last_error()))
	}
	return nil
}
