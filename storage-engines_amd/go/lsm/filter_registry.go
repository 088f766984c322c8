// Filter registry + batched Get filter step (SURVEY.md §8(f) rows 1-2) — additive API beside the
// drop-in bloom.go.  The reference's callers do not use it; a batched MultiGet would:
//
//	OpenSSTable (lsm/sstable.go:121-129)        -> reg.Put(fileNum, level, bloomBlock, minKey, maxKey)
//	compaction removes inputs (compaction.go:335-343) -> reg.Remove(fileNum)
//	LSM.Get's walk + MayContain (lsm/lsm.go:168-198) -> reg.Candidates(keys)
//	OpenSSTable reads indexData (lsm/sstable.go:105-119)   -> reg.PutIndex(fileNum, indexData)
//	SSTable.Get's index bisection (lsm/sstable.go:210-222) -> reg.MultiGetBlocks(keys)
//	readBlock (lsm/sstable.go:225-239) stays with the caller: it reads every BlockRead once
//	searchBlock + Get's decision (sstable.go:242-290, lsm.go:174-197) -> reg.SearchBlocks(keys, reads, blocks)
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is
// tested through the Python binding (tests/test_gpu_parity.py, test_registry_*).
package lsm

/*
#include <stdint.h>
#include <stdlib.h>
#include "seb_bloom.h"
*/
import "C"

import (
	"runtime"
	"sync"
	"sync/atomic"
	"unsafe"
)

// FilterRegistry holds the bloom filters of the open SSTables in HBM (one per LSM instance).
type FilterRegistry struct {
	h       *C.seb_registry
	capHint atomic.Uint32 // row width of the last Candidates call (the C side re-checks it)
	device  int
	ctxMu   sync.Mutex
	ctx     *C.seb_ctx // SearchBlocks' streams and staging buffers, made on first use
}

func regPanic(op string) {
	panic("lsm: FilterRegistry." + op + ": " + C.GoString(C.seb_last_error()))
}

// NewFilterRegistry creates an empty registry on GPU `device`.
func NewFilterRegistry(device int) *FilterRegistry {
	h := C.seb_registry_new(C.int(device))
	if h == nil {
		regPanic("New")
	}
	r := &FilterRegistry{h: h, device: device}
	runtime.SetFinalizer(r, func(r *FilterRegistry) {
		if r.ctx != nil {
			C.seb_ctx_destroy(r.ctx)
		}
		C.seb_registry_free(r.h)
	})
	return r
}

func bytesPtr(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

// Put registers an SSTable's bloom block (its Encode() bytes) with the file's level and key
// range; levels 1..4 are kept by MinKey as lsm/levels.go:45-63 keeps them.  Returns the slot.
func (r *FilterRegistry) Put(fileNum uint64, level int, bloomBlock []byte, minKey, maxKey string) int {
	mn, mx := []byte(minKey), []byte(maxKey)
	rc := C.seb_registry_put(r.h, C.uint64_t(fileNum), C.int(level), bytesPtr(bloomBlock), C.uint64_t(len(bloomBlock)),
		bytesPtr(mn), C.uint64_t(len(mn)), bytesPtr(mx), C.uint64_t(len(mx)))
	if rc < 0 {
		regPanic("Put")
	}
	runtime.KeepAlive(bloomBlock)
	return int(rc)
}

// Remove frees a file's filter (compaction deleted the file).
func (r *FilterRegistry) Remove(fileNum uint64) {
	if C.seb_registry_remove(r.h, C.uint64_t(fileNum)) != 0 {
		regPanic("Remove")
	}
}

// Candidates returns, per key, the file numbers Get would read for it — every L0 file and the
// covering file of each level 1..4 whose bloom filter may contain the key — in Get's visiting
// order.  One GPU launch for the whole batch, any number of registered files.
func (r *FilterRegistry) Candidates(keys []string) [][]uint64 {
	out := make([][]uint64, len(keys))
	if len(keys) == 0 {
		return out
	}
	data, offs := packKeys(keys)
	// the seb_keys struct holds Go pointers: it lives in C memory and what it points to is pinned
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&data[0])
	pin.Pin(&offs[0])
	ks := (*C.seb_keys)(C.malloc(C.size_t(unsafe.Sizeof(C.seb_keys{}))))
	defer C.free(unsafe.Pointer(ks))
	*ks = C.seb_keys{data: (*C.uint8_t)(unsafe.Pointer(&data[0])), offsets: (*C.uint64_t)(unsafe.Pointer(&offs[0])),
		n: C.uint64_t(len(keys))}
	// One C call sizes the rows, runs the lookup and maps slots to file numbers under the
	// registry's lock, so a concurrent flush (Put) or compaction (Remove + Put reusing the slot)
	// cannot overflow a row or make a slot name the wrong file.  SEB_ERR_RANGE: the registry
	// grew since the last call; retry with the width it reports.
	capRow := C.uint32_t(r.capHint.Load())
	if capRow == 0 {
		capRow = 1
	}
	var files []uint64
	for {
		files = make([]uint64, len(keys)*int(capRow))
		var need C.uint32_t
		rc := C.seb_registry_multiget_files(r.h, ks, (*C.uint64_t)(unsafe.Pointer(&files[0])), capRow, &need)
		if rc == C.int(C.SEB_ERR_RANGE) && need > capRow {
			capRow = need
			continue
		}
		if rc != 0 {
			regPanic("Candidates")
		}
		r.capHint.Store(uint32(capRow))
		break
	}
	runtime.KeepAlive(data)
	runtime.KeepAlive(offs)
	w := int(capRow)
	for i := range keys {
		for _, f := range files[i*w : (i+1)*w] {
			if f == ^uint64(0) {
				break
			}
			out[i] = append(out[i], f)
		}
	}
	return out
}

// PutIndex attaches a registered file's encoded index block: the indexData OpenSSTable hands to
// decodeIndex (lsm/sstable.go:105-119).  It is kept in HBM beside the file's filter and freed by Remove.
func (r *FilterRegistry) PutIndex(fileNum uint64, indexData []byte) {
	if C.seb_registry_put_index(r.h, C.uint64_t(fileNum), bytesPtr(indexData), C.uint64_t(len(indexData))) != 0 {
		regPanic("PutIndex")
	}
	runtime.KeepAlive(indexData)
}

// BlockRead is one read of a MultiGet's plan: readBlock(Offset) in SSTable File.
type BlockRead struct {
	File   uint64
	Offset uint64
}

// MultiGetBlocks is Candidates plus SSTable.Get's index step (lsm/sstable.go:210-222): per key, in
// Get's visiting order, the files whose filter may contain it and the offset of the one data block
// to read in each.  A candidate file whose first index key sorts after the key is left out, as Get
// returns "not found" for it without a read.  Every registered file needs PutIndex first.
func (r *FilterRegistry) MultiGetBlocks(keys []string) [][]BlockRead {
	out := make([][]BlockRead, len(keys))
	if len(keys) == 0 {
		return out
	}
	data, offs := packKeys(keys)
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&data[0])
	pin.Pin(&offs[0])
	ks := (*C.seb_keys)(C.malloc(C.size_t(unsafe.Sizeof(C.seb_keys{}))))
	defer C.free(unsafe.Pointer(ks))
	*ks = C.seb_keys{data: (*C.uint8_t)(unsafe.Pointer(&data[0])), offsets: (*C.uint64_t)(unsafe.Pointer(&offs[0])),
		n: C.uint64_t(len(keys))}
	capRow := C.uint32_t(r.capHint.Load())
	if capRow == 0 {
		capRow = 1
	}
	var files, blocks []uint64
	for { // SEB_ERR_RANGE: the registry grew since the last call; retry with the width it reports
		files = make([]uint64, len(keys)*int(capRow))
		blocks = make([]uint64, len(keys)*int(capRow))
		var need C.uint32_t
		rc := C.seb_registry_multiget_blocks(r.h, ks, (*C.uint64_t)(unsafe.Pointer(&files[0])),
			(*C.uint64_t)(unsafe.Pointer(&blocks[0])), capRow, &need)
		if rc == C.int(C.SEB_ERR_RANGE) && need > capRow {
			capRow = need
			continue
		}
		if rc != 0 {
			regPanic("MultiGetBlocks")
		}
		r.capHint.Store(uint32(capRow))
		break
	}
	runtime.KeepAlive(data)
	runtime.KeepAlive(offs)
	w := int(capRow)
	for i := range keys {
		for j := i * w; j < (i+1)*w && files[j] != ^uint64(0); j++ {
			if blocks[j] != ^uint64(0) { // SEB_NO_BLOCK: blockIdx == 0, nothing to read
				out[i] = append(out[i], BlockRead{File: files[j], Offset: blocks[j]})
			}
		}
	}
	return out
}

// GetResult is LSM.Get's answer over the SSTables for one key of a SearchBlocks batch.
type GetResult struct {
	Found bool   // a file holds a live entry for the key
	Err   bool   // the deciding block is truncated: searchBlock's "block truncated"
	Read  int    // index into the key's reads of the block that decided, -1 for none
	Value []byte // the value (a copy), nil unless Found
}

// SearchBlocks finishes the batch MultiGetBlocks began.  reads[i] is MultiGetBlocks' answer for keys[i];
// blocks maps every distinct BlockRead to the bytes readBlock returned for it (at most 4096; the caller
// does the file reads, each block once).  Per key it walks each block as searchBlock does
// (lsm/sstable.go:242-290) and decides as LSM.Get does (lsm/lsm.go:174-197): the first file in visiting
// order that finds the key or fails ends the walk.  A tombstone inside an SSTable does NOT end it
// (sst.Get returns found == false, sstable.go:273-275), so an older file's value is returned, exactly
// as the reference does.  One H2D copy, two launches and one D2H copy for the whole batch.
func (r *FilterRegistry) SearchBlocks(keys []string, reads [][]BlockRead, blocks map[BlockRead][]byte) []GetResult {
	out := make([]GetResult, len(keys))
	if len(keys) == 0 {
		return out
	}
	if len(reads) != len(keys) {
		panic("lsm: FilterRegistry.SearchBlocks: len(reads) != len(keys)")
	}
	w := 1
	for _, row := range reads {
		if len(row) > w {
			w = len(row)
		}
	}
	// the block pool: each distinct block once, in first-appearance order, in 4096-byte slots
	ids := make(map[BlockRead]uint32)
	var pool []byte
	var blen []uint16
	bid := make([]uint32, len(keys)*w)
	for i := range bid {
		bid[i] = ^uint32(0) // SEB_NO_BLOCK_ID
	}
	for i, row := range reads {
		for j, rd := range row {
			id, ok := ids[rd]
			if !ok {
				b, have := blocks[rd]
				if !have || len(b) > 4096 {
					panic("lsm: FilterRegistry.SearchBlocks: a read's block is missing or longer than 4096 bytes")
				}
				id = uint32(len(blen))
				ids[rd] = id
				slot := make([]byte, 4096)
				copy(slot, b)
				pool = append(pool, slot...)
				blen = append(blen, uint16(len(b)))
			}
			bid[i*w+j] = id
		}
	}
	data, offs := packKeys(keys)
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&data[0])
	pin.Pin(&offs[0])
	ks := (*C.seb_keys)(C.malloc(C.size_t(unsafe.Sizeof(C.seb_keys{}))))
	defer C.free(unsafe.Pointer(ks))
	*ks = C.seb_keys{data: (*C.uint8_t)(unsafe.Pointer(&data[0])), offsets: (*C.uint64_t)(unsafe.Pointer(&offs[0])),
		n: C.uint64_t(len(keys))}
	status := make([]uint8, len(keys))
	col := make([]uint16, len(keys))
	vloc := make([]uint64, len(keys))
	vlen := make([]uint32, len(keys))
	var poolPtr *C.uint8_t
	var blenPtr *C.uint16_t
	if len(blen) > 0 {
		poolPtr = (*C.uint8_t)(unsafe.Pointer(&pool[0]))
		blenPtr = (*C.uint16_t)(unsafe.Pointer(&blen[0]))
	}
	r.ctxMu.Lock()
	if r.ctx == nil && C.seb_ctx_create(C.int(r.device), &r.ctx) != 0 {
		r.ctxMu.Unlock()
		regPanic("SearchBlocks")
	}
	rc := C.seb_search_blocks(r.ctx, ks, (*C.uint32_t)(unsafe.Pointer(&bid[0])), C.uint32_t(w), poolPtr, blenPtr,
		C.uint32_t(len(blen)), (*C.uint8_t)(unsafe.Pointer(&status[0])), (*C.uint16_t)(unsafe.Pointer(&col[0])),
		(*C.uint64_t)(unsafe.Pointer(&vloc[0])), (*C.uint32_t)(unsafe.Pointer(&vlen[0])), nil)
	r.ctxMu.Unlock()
	if rc != 0 {
		regPanic("SearchBlocks")
	}
	runtime.KeepAlive(data)
	runtime.KeepAlive(offs)
	for i := range keys {
		out[i].Read = -1
		if col[i] != 0xFFFF {
			out[i].Read = int(col[i])
		}
		switch status[i] {
		case C.SEB_GET_FOUND:
			out[i].Found = true
			out[i].Value = append([]byte{}, pool[vloc[i]:vloc[i]+uint64(vlen[i])]...)
		case C.SEB_GET_ERROR:
			out[i].Err = true
		}
	}
	return out
}

// packKeys lays keys out as one byte buffer + len(keys)+1 offsets (the seb_keys var-length form).
func packKeys(keys []string) ([]byte, []uint64) {
	total := 0
	for _, k := range keys {
		total += len(k)
	}
	data := make([]byte, total+1)
	offs := make([]uint64, len(keys)+1)
	pos := 0
	for i, k := range keys {
		offs[i] = uint64(pos)
		pos += copy(data[pos:], k)
	}
	offs[len(keys)] = uint64(pos)
	return data, offs
}
