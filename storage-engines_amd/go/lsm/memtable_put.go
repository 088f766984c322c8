// PutBatch over the memtable write side of libseb_bloom (include/seb_bloom.h, the memtable write side group): what
// LSM.Put / LSM.Delete do at lsm/lsm.go:97-137, 203-235 for a whole batch of one writer in one call.
//
//	sequences  op i gets lsm.sequence + 1 + i, as atomic.AddUint64 would hand them out in order
//	log        one seb_memtable_apply call frames the ops as WAL.Append's records and seals them; the image is the
//	           batch's one Write to the log file
//	memtable   the call also returns the batch's sorted run (what MemTable.Put / Delete of these ops alone would
//	           leave) and MemTable.size's change against the active memtable's runs; the run goes in front of them
//	freeze     the reference tests IsFull() after every op and freezes only when no flush is pending, so the size
//	           at which it freezes is no invariant; here the caller's test runs once per batch, on the size after it
//
// No departure from the reference for one writer: the log bytes are Append's, and the runs fold (seb_memtable_fold,
// newest first) into the memtable the ops would have built one by one.  Concurrent writers are serialised by
// lsm.mu, as PutBatch holds it for the batch.
//
// It assumes three additions to the engine: LSM.activeRuns and LSM.activeSize (the active memtable as runs, newest
// first, and its MemTable.size) and WAL.WriteImage (one Write of framed records).
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_memwrite.py, tests/test_gpu_memwrite.py).
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

// BatchOp is one Put (Delete false) or Delete (Value ignored) of a batch.
type BatchOp struct {
	Key    string
	Value  []byte
	Delete bool
}

// memRun is one sorted run of the active memtable in the builder's input layout, newest first in lsm.activeRuns.
type memRun struct {
	keys, vals, deleted []byte
	keyOff, valOff, seq []uint64
}

// PutBatch applies ops in order: the log first (wal.go:31-65), then the memtable.  It returns MemTable.size
// after the batch; the caller freezes the memtable when that passes its limit and no flush is pending.
func (lsm *LSM) PutBatch(ops []BatchOp) (int64, error) {
	if len(ops) == 0 {
		return lsm.activeSize, nil
	}
	lsm.mu.Lock()
	defer lsm.mu.Unlock()
	if len(lsm.activeRuns) >= C.SEB_MEM_MAX_RUNS-1 {
		if err := lsm.foldActiveRuns(); err != nil {
			return 0, err
		}
	}

	keys := make([]string, len(ops))
	valOff := make([]uint64, len(ops)+1)
	deleted := make([]byte, len(ops))
	var vals []byte
	for i, op := range ops {
		keys[i] = op.Key
		if op.Delete {
			deleted[i] = 1
		} else {
			vals = append(vals, op.Value...)
		}
		valOff[i+1] = uint64(len(vals))
	}
	data, offs := packKeys(keys)
	kb := C.seb_keys{data: bytesPtr(data), offsets: u64Ptr(offs), n: C.uint64_t(len(ops))}

	// the run structs hold Go pointers, so they live in C memory for the call
	runs := (*[C.SEB_MEM_MAX_RUNS]C.seb_run)(C.calloc(C.SEB_MEM_MAX_RUNS, C.size_t(unsafe.Sizeof(C.seb_run{}))))
	defer C.free(unsafe.Pointer(runs))
	for r, p := range lsm.activeRuns {
		runs[r] = C.seb_run{keys: bytesPtr(p.keys), key_bytes: C.uint64_t(len(p.keys)), key_off: u64Ptr(p.keyOff),
			val_off: u64Ptr(p.valOff), deleted: bytesPtr(p.deleted), seq: u64Ptr(p.seq), n: C.uint64_t(len(p.seq))}
	}

	var ctx *C.seb_ctx
	if C.seb_ctx_create(C.int(0), &ctx) != 0 {
		return 0, fmt.Errorf("failed to apply batch: %s", C.GoString(C.seb_last_error()))
	}
	defer C.seb_ctx_destroy(ctx)

	// upper bounds of every output: a record is 21 bytes and its key and value; a run holds at most every op
	n := len(ops)
	image := make([]byte, 21*n+len(data)+len(vals))
	run := &memRun{keys: make([]byte, len(data)+1), vals: make([]byte, len(vals)+1), deleted: make([]byte, n),
		keyOff: make([]uint64, n+1), valOff: make([]uint64, n+1), seq: make([]uint64, n)}
	var imageBytes, sequence C.uint64_t
	var delta C.int64_t
	var sizes C.seb_replay_sizes
	rc := C.seb_memtable_apply(ctx, &kb, bytesPtr(vals), u64Ptr(valOff), bytesPtr(deleted), C.uint64_t(lsm.sequence+1),
		&runs[0], C.uint32_t(len(lsm.activeRuns)), bytesPtr(image), C.uint64_t(len(image)), &imageBytes,
		bytesPtr(run.keys), C.uint64_t(len(data)), u64Ptr(run.keyOff), bytesPtr(run.vals), C.uint64_t(len(vals)),
		u64Ptr(run.valOff), bytesPtr(run.deleted), u64Ptr(run.seq), C.uint64_t(n), &sizes, &delta, &sequence)
	if rc != 0 {
		return 0, fmt.Errorf("failed to apply batch: %s", C.GoString(C.seb_last_error()))
	}
	if err := lsm.wal.WriteImage(image[:imageBytes]); err != nil { // the batch's one Write (wal.go:59-62)
		return 0, fmt.Errorf("failed to write WAL: %w", err)
	}
	out := int(sizes.entries_out)
	run.keys, run.vals = run.keys[:sizes.key_bytes], run.vals[:sizes.val_bytes]
	run.keyOff, run.valOff, run.deleted, run.seq = run.keyOff[:out+1], run.valOff[:out+1], run.deleted[:out], run.seq[:out]
	lsm.activeRuns = append([]*memRun{run}, lsm.activeRuns...)
	lsm.activeSize += int64(delta)
	lsm.sequence = uint64(sequence)
	return lsm.activeSize, nil
}

// foldActiveRuns folds the active memtable's runs into one: GetAllEntries() of the memtable they add up to.
func (lsm *LSM) foldActiveRuns() error {
	runs := (*[C.SEB_MEM_MAX_RUNS]C.seb_run)(C.calloc(C.SEB_MEM_MAX_RUNS, C.size_t(unsafe.Sizeof(C.seb_run{}))))
	defer C.free(unsafe.Pointer(runs))
	vals := (*[C.SEB_MEM_MAX_RUNS]*C.uint8_t)(C.calloc(C.SEB_MEM_MAX_RUNS, C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(vals))
	valBytes := make([]uint64, len(lsm.activeRuns))
	var keyCap, valCap, entryCap uint64
	for r, p := range lsm.activeRuns {
		runs[r] = C.seb_run{keys: bytesPtr(p.keys), key_bytes: C.uint64_t(len(p.keys)), key_off: u64Ptr(p.keyOff),
			val_off: u64Ptr(p.valOff), deleted: bytesPtr(p.deleted), seq: u64Ptr(p.seq), n: C.uint64_t(len(p.seq))}
		vals[r] = bytesPtr(p.vals)
		valBytes[r] = uint64(len(p.vals))
		keyCap, valCap, entryCap = keyCap+uint64(len(p.keys)), valCap+uint64(len(p.vals)), entryCap+uint64(len(p.seq))
	}
	var ctx *C.seb_ctx
	if C.seb_ctx_create(C.int(0), &ctx) != 0 {
		return fmt.Errorf("failed to fold memtable runs: %s", C.GoString(C.seb_last_error()))
	}
	defer C.seb_ctx_destroy(ctx)
	out := &memRun{keys: make([]byte, keyCap+1), vals: make([]byte, valCap+1), deleted: make([]byte, entryCap+1),
		keyOff: make([]uint64, entryCap+1), valOff: make([]uint64, entryCap+1), seq: make([]uint64, entryCap+1)}
	var sizes C.seb_fold_sizes
	rc := C.seb_memtable_fold(ctx, &runs[0], &vals[0], u64Ptr(valBytes), C.uint32_t(len(lsm.activeRuns)), bytesPtr(out.keys),
		C.uint64_t(keyCap), u64Ptr(out.keyOff), bytesPtr(out.vals), C.uint64_t(valCap), u64Ptr(out.valOff),
		bytesPtr(out.deleted), u64Ptr(out.seq), C.uint64_t(entryCap), &sizes)
	if rc != 0 {
		return fmt.Errorf("failed to fold memtable runs: %s", C.GoString(C.seb_last_error()))
	}
	n := int(sizes.entries_out)
	out.keys, out.vals = out.keys[:sizes.key_bytes], out.vals[:sizes.val_bytes]
	out.keyOff, out.valOff, out.deleted, out.seq = out.keyOff[:n+1], out.valOff[:n+1], out.deleted[:n], out.seq[:n]
	lsm.activeRuns = []*memRun{out}
	lsm.activeSize = int64(sizes.memtable_size)
	return nil
}
