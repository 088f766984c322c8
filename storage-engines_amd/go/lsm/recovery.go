// recoverFromWAL over the batched WAL replay of libseb_bloom (include/seb_bloom.h, the WAL replay group): the
// same signature as the reference's lsm/lsm.go:273, so NewLSM calls it unchanged.
//
//	read     the log file's bytes in one piece (what WAL.ReadAll reads record by record)
//	recover  one seb_wal_recover call: ReadAll's framing walk and CRC check, then every record through
//	         MemTable.Put / MemTable.Delete at once: one entry per key from its last record, in key order
//	install  the sorted run becomes the active memtable's entries, with the size Put and Delete would have
//	         left and the highest sequence of the log
//
// No departure from the reference: the entries, their order, lsm.sequence and MemTable.size are what the
// record-by-record replay leaves.  Errors come in ReadAll's order (a record that fails its CRC before a
// truncated tail), with the library's text wrapped as ReadAll's callers see it.
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_replay.py, tests/test_gpu_replay.py).
package lsm

/*
#include <stdint.h>
#include "seb_bloom.h"
*/
import "C"

import (
	"fmt"
	"log"
	"os"
)

// recoverFromWAL replays the write-ahead log into the active memtable on the device.
func (lsm *LSM) recoverFromWAL() error {
	image, err := os.ReadFile(lsm.wal.path)
	if err != nil {
		return fmt.Errorf("failed to read WAL header: %w", err)
	}
	if len(image) == 0 {
		return nil
	}

	var ctx *C.seb_ctx
	if C.seb_ctx_create(C.int(0), &ctx) != 0 {
		return fmt.Errorf("failed to recover from WAL: %s", C.GoString(C.seb_last_error()))
	}
	defer C.seb_ctx_destroy(ctx)

	var sizes C.seb_replay_sizes
	keys, vals, deleted := make([]byte, 1), make([]byte, 1), make([]byte, 1)
	keyOff, valOff, seq := make([]uint64, 1), make([]uint64, 1), make([]uint64, 1)
	for {
		rc := C.seb_wal_recover(ctx, bytesPtr(image), C.uint64_t(len(image)), bytesPtr(keys), C.uint64_t(len(keys)),
			u64Ptr(keyOff), bytesPtr(vals), C.uint64_t(len(vals)), u64Ptr(valOff), bytesPtr(deleted), u64Ptr(seq),
			C.uint64_t(len(deleted)), &sizes)
		if rc == C.SEB_ERR_RANGE { // the retry contract: *sizes holds what the outputs need
			keys = make([]byte, uint64(sizes.key_bytes)+1)
			vals = make([]byte, uint64(sizes.val_bytes)+1)
			deleted = make([]byte, uint64(sizes.entries_out)+1)
			seq = make([]uint64, uint64(sizes.entries_out)+1)
			keyOff = make([]uint64, uint64(sizes.entries_out)+2)
			valOff = make([]uint64, uint64(sizes.entries_out)+2)
			continue
		}
		if rc != 0 {
			return fmt.Errorf("%s", C.GoString(C.seb_last_error()))
		}
		break
	}
	if sizes.records_in == 0 {
		return nil
	}

	log.Printf("Recovering %d entries from WAL", uint64(sizes.records_in))

	n := int(sizes.entries_out)
	entries := make([]MemTableEntry, n, n+1024)
	for i := 0; i < n; i++ {
		e := MemTableEntry{Key: string(keys[keyOff[i]:keyOff[i+1]]), Sequence: seq[i], Deleted: deleted[i] == 1}
		if !e.Deleted { // Delete stores Value nil; Put keeps a slice, empty or not
			e.Value = make([]byte, valOff[i+1]-valOff[i])
			copy(e.Value, vals[valOff[i]:valOff[i+1]])
		}
		entries[i] = e
	}
	mt := lsm.activeMemtable
	mt.mu.Lock()
	mt.entries = entries
	mt.size = int(sizes.memtable_size)
	mt.mu.Unlock()
	if uint64(sizes.max_sequence) > lsm.sequence {
		lsm.sequence = uint64(sizes.max_sequence)
	}
	return nil
}
