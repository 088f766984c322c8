// The memtable steps of a GetBatch over the batched memtable lookup of libseb_bloom (include/seb_bloom.h, the
// memtable lookup group): what LSM.Get does at lsm/lsm.go:144-166, for a whole key batch in one call.
//
//	runs     the active memtable's entries, then the immutable one's if there is one, each packed into the
//	         builder's input layout under its read lock (what GetAllEntries hands to a flush)
//	lookup   one seb_memtable_get call: MemTable.Get of every key in every run, the first run that holds a key
//	         deciding
//	answer   per key: found with the value, a tombstone (LSM.Get returns "not found" and reads no SSTable), or
//	         undecided; only the undecided keys go on to FilterRegistry's MultiGet and SearchBlocks
//
// No departure from the reference: a key's answer is the one LSM.Get gives when nothing is written between
// the calls.  A tombstone in a memtable ends the Get, unlike one inside an SSTable (FilterRegistry.SearchBlocks).
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_memget.py, tests/test_gpu_memget.py).
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

// MemGetStatus is a key's answer from the memtables.
type MemGetStatus uint8

const (
	MemNone      MemGetStatus = C.SEB_MEM_NONE      // in neither memtable: the SSTables decide
	MemFound     MemGetStatus = C.SEB_MEM_FOUND     // Value is the answer
	MemTombstone MemGetStatus = C.SEB_MEM_TOMBSTONE // deleted: "not found", and no SSTable is read
)

// MemGetResult is MemTable.Get's answer for one key of a batch.
type MemGetResult struct {
	Status   MemGetStatus
	Value    []byte
	Sequence uint64
}

// packedRun keeps a memtable's entries in the builder's input layout alive across the C call.
type packedRun struct {
	keys, deleted   []byte
	keyOff, valOff  []uint64
	seq             []uint64
	values          [][]byte
}

func packMemTable(m *MemTable) *packedRun {
	m.mu.RLock()
	defer m.mu.RUnlock()
	n := len(m.entries)
	p := &packedRun{deleted: make([]byte, n), keyOff: make([]uint64, n+1), valOff: make([]uint64, n+1),
		seq: make([]uint64, n), values: make([][]byte, n)}
	for i, e := range m.entries {
		p.keys = append(p.keys, e.Key...)
		p.keyOff[i+1] = uint64(len(p.keys))
		p.valOff[i+1] = p.valOff[i] + uint64(len(e.Value))
		if e.Deleted {
			p.deleted[i] = 1
		}
		p.seq[i] = e.Sequence
		p.values[i] = e.Value
	}
	return p
}

// getBatchMemtables answers every key from the active memtable, then the immutable one.  The caller joins the
// result with the SSTables' answer for the keys whose Status is MemNone.
func (lsm *LSM) getBatchMemtables(keys []string) ([]MemGetResult, error) {
	out := make([]MemGetResult, len(keys))
	if len(keys) == 0 {
		return out, nil
	}
	lsm.mu.RLock()
	packed := []*packedRun{packMemTable(lsm.activeMemtable)}
	if lsm.immutableMemtable != nil {
		packed = append(packed, packMemTable(lsm.immutableMemtable))
	}
	lsm.mu.RUnlock()

	// the run structs hold Go pointers, so they live in C memory for the call
	runs := (*[C.SEB_MEM_MAX_RUNS]C.seb_run)(C.calloc(C.SEB_MEM_MAX_RUNS, C.size_t(unsafe.Sizeof(C.seb_run{}))))
	defer C.free(unsafe.Pointer(runs))
	for r, p := range packed {
		runs[r] = C.seb_run{keys: bytesPtr(p.keys), key_bytes: C.uint64_t(len(p.keys)), key_off: u64Ptr(p.keyOff),
			val_off: u64Ptr(p.valOff), deleted: bytesPtr(p.deleted), seq: u64Ptr(p.seq), n: C.uint64_t(len(p.seq))}
	}

	data, offs := packKeys(keys)
	kb := C.seb_keys{data: bytesPtr(data), offsets: u64Ptr(offs), n: C.uint64_t(len(keys))}
	status, run := make([]byte, len(keys)), make([]byte, len(keys))
	entry := make([]uint32, len(keys))
	seq := make([]uint64, len(keys))

	var ctx *C.seb_ctx
	if C.seb_ctx_create(C.int(0), &ctx) != 0 {
		return nil, fmt.Errorf("failed to look up memtables: %s", C.GoString(C.seb_last_error()))
	}
	defer C.seb_ctx_destroy(ctx)
	rc := C.seb_memtable_get(ctx, &kb, &runs[0], C.uint32_t(len(packed)), bytesPtr(status), bytesPtr(run),
		(*C.uint32_t)(unsafe.Pointer(&entry[0])), nil, nil, u64Ptr(seq))
	if rc != 0 {
		return nil, fmt.Errorf("failed to look up memtables: %s", C.GoString(C.seb_last_error()))
	}
	for i := range keys {
		out[i].Status = MemGetStatus(status[i])
		out[i].Sequence = seq[i]
		if out[i].Status == MemFound {
			out[i].Value = packed[run[i]].values[entry[i]]
		}
	}
	return out, nil
}
