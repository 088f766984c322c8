// mergeFiles over the batched compaction merge of libseb_bloom (include/seb_bloom.h, the compaction merge
// group): the same signature as the reference's lsm/compaction.go:226, so CompactL0ToL1 and CompactLnToLn1
// (:155-223) call it unchanged.
//
//	read     every input file's data blocks (sst.readBlock per index entry) into one block pool, file i =
//	         run i, in the order the caller passes the files (allFiles: the upper level first)
//	merge    one seb_merge call: loadBlock's decode, the k-way merge by key, one entry per key, tombstones
//	         dropped when targetLevel == 4
//	build    the merged run in files of 100,000 entries through SSTableBuilder (one seb_sst_build each)
//
// One departure from the reference, stated in seb_bloom.h: of several entries with one key the reference
// keeps whichever container/heap's array order leaves for last; here the entry of the lowest-numbered run,
// i.e. of the file that comes first in `sstables`, survives.  Everything else is the reference's output.
// Every input file must be strictly increasing (anything a flush or an earlier merge wrote is); the library
// refuses a file that is not, where the reference would merge it in a heap-dependent order.
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_merge.py, tests/test_gpu_merge.py).
package lsm

/*
#include <stdint.h>
#include "seb_bloom.h"
*/
import "C"

import (
	"fmt"
	"path/filepath"
	"unsafe"
)

const mergeBlockBytes = 4096
const maxEntriesPerFile = 100000

func u64Ptr(v []uint64) *C.uint64_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&v[0]))
}

// mergeFiles performs the k-way merge of the input SSTables on the device and writes the output files.
func mergeFiles(dataDir string, sstables []*SSTable, targetLevel int, nextFileNum *uint64) ([]*SSTable, error) {
	var pool []byte
	var blen []uint16
	runBegin := make([]uint64, 1, len(sstables)+1)
	for _, sst := range sstables {
		for _, ie := range sst.index {
			block, err := sst.readBlock(ie.BlockOffset)
			if err != nil {
				return nil, err
			}
			slot := make([]byte, mergeBlockBytes)
			copy(slot, block)
			pool = append(pool, slot...)
			blen = append(blen, uint16(len(block)))
		}
		runBegin = append(runBegin, uint64(len(blen)))
	}

	var ctx *C.seb_ctx
	if C.seb_ctx_create(C.int(0), &ctx) != 0 {
		return nil, fmt.Errorf("failed to merge sstables: %s", C.GoString(C.seb_last_error()))
	}
	defer C.seb_ctx_destroy(ctx)
	flags := C.uint32_t(0)
	if targetLevel == 4 {
		flags = C.SEB_MERGE_DROP_TOMBSTONES
	}
	var blenPtr *C.uint16_t
	if len(blen) > 0 {
		blenPtr = (*C.uint16_t)(unsafe.Pointer(&blen[0]))
	}
	var sizes C.seb_merge_sizes
	keys, vals, deleted := make([]byte, 1), make([]byte, 1), make([]byte, 1)
	keyOff, valOff := make([]uint64, 1), make([]uint64, 1)
	for {
		rc := C.seb_merge(ctx, bytesPtr(pool), blenPtr, C.uint32_t(len(blen)), u64Ptr(runBegin), C.uint32_t(len(sstables)),
			flags, bytesPtr(keys), C.uint64_t(len(keys)), u64Ptr(keyOff), bytesPtr(vals), C.uint64_t(len(vals)),
			u64Ptr(valOff), bytesPtr(deleted), C.uint64_t(len(deleted)), &sizes)
		if rc == C.SEB_ERR_RANGE { // the retry contract: *sizes holds what the outputs need
			keys = make([]byte, uint64(sizes.key_bytes)+1)
			vals = make([]byte, uint64(sizes.val_bytes)+1)
			deleted = make([]byte, uint64(sizes.entries_out)+1)
			keyOff = make([]uint64, uint64(sizes.entries_out)+2)
			valOff = make([]uint64, uint64(sizes.entries_out)+2)
			continue
		}
		if rc != 0 {
			return nil, fmt.Errorf("failed to merge sstables: %s", C.GoString(C.seb_last_error()))
		}
		break
	}

	var out []*SSTable
	n := int(sizes.entries_out)
	for first := 0; first < n; first += maxEntriesPerFile {
		last := first + maxEntriesPerFile
		if last > n {
			last = n
		}
		fileNum := *nextFileNum
		*nextFileNum++
		path := filepath.Join(dataDir, fmt.Sprintf("L%d-%06d.sst", targetLevel, fileNum))
		builder, err := NewSSTableBuilder(path, maxEntriesPerFile)
		if err != nil {
			return nil, err
		}
		for i := first; i < last; i++ {
			key := string(keys[keyOff[i]:keyOff[i+1]])
			if err := builder.Add(key, vals[valOff[i]:valOff[i+1]], deleted[i] == 1); err != nil {
				builder.Abort()
				return nil, err
			}
		}
		if err := builder.Finish(); err != nil {
			return nil, err
		}
		sst, err := OpenSSTable(path, targetLevel, fileNum)
		if err != nil {
			return nil, err
		}
		out = append(out, sst)
	}
	return out, nil
}
