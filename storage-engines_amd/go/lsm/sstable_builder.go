// Drop-in SSTableBuilder over the batched builder of libseb_bloom (include/seb_bloom.h, the SSTable
// builder group): the same constructor and methods as the reference's lsm/sstable_builder.go, so
// flushMemTable (lsm/lsm.go) and the compaction writer (lsm/compaction.go:253-300) compile unchanged.
//
//	NewSSTableBuilder(path, expectedKeys)  creates the file, as the reference does
//	Add(key, value, deleted)               buffers the entry (key bytes, value bytes, offsets, one byte)
//	Finish()                               one seb_sst_build call: data blocks, index, metadata, the filter's
//	                                       Encode() and the footer as one image, byte-identical to what the
//	                                       reference writes; then one Write, Sync and Close
//	Abort()                                closes and removes the file
//
// The reference's Add can fail only through flushBlock's file writes; here Add never touches the file,
// so write errors surface from Finish.  A file with an entry of more than 4,092 bytes is encoded by the
// library's host half (the device never writes a block longer than 4096 bytes); the image is the same.
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is
// tested through the Python binding (tests/test_sst_build.py, tests/test_gpu_sst_build.py).
package lsm

/*
#include <stdint.h>
#include <stdlib.h>
#include "seb_bloom.h"
*/
import "C"

import (
	"fmt"
	"os"
	"runtime"
	"unsafe"
)

// SSTableBuilder constructs a new SSTable from sorted entries.
type SSTableBuilder struct {
	file         *os.File
	path         string
	expectedKeys int
	keys         []byte
	keyOff       []uint64
	vals         []byte
	valOff       []uint64
	deleted      []byte
}

// NewSSTableBuilder creates a new SSTable builder.
func NewSSTableBuilder(path string, expectedKeys int) (*SSTableBuilder, error) {
	file, err := os.Create(path)
	if err != nil {
		return nil, fmt.Errorf("failed to create sstable: %w", err)
	}
	return &SSTableBuilder{file: file, path: path, expectedKeys: expectedKeys, keyOff: []uint64{0}, valOff: []uint64{0}}, nil
}

// Add adds a key-value pair to the SSTable.  MUST be called in sorted key order!
func (b *SSTableBuilder) Add(key string, value []byte, deleted bool) error {
	if b.expectedKeys == 0 {
		panic("runtime error: integer divide by zero") // the reference's bloomFilter.Add on a 0-bit filter
	}
	b.keys = append(b.keys, key...)
	b.keyOff = append(b.keyOff, uint64(len(b.keys)))
	b.vals = append(b.vals, value...)
	b.valOff = append(b.valOff, uint64(len(b.vals)))
	d := byte(0)
	if deleted {
		d = 1
	}
	b.deleted = append(b.deleted, d)
	return nil
}

// Finish builds the file image in one library call and writes it.
func (b *SSTableBuilder) Finish() error {
	n := len(b.deleted)
	var ctx *C.seb_ctx
	if C.seb_ctx_create(C.int(0), &ctx) != 0 {
		return fmt.Errorf("failed to build sstable: %s", C.GoString(C.seb_last_error()))
	}
	defer C.seb_ctx_destroy(ctx)
	// the seb_keys struct holds Go pointers: it lives in C memory and what it points to is pinned
	var pin runtime.Pinner
	defer pin.Unpin()
	ks := (*C.seb_keys)(C.malloc(C.size_t(unsafe.Sizeof(C.seb_keys{}))))
	defer C.free(unsafe.Pointer(ks))
	*ks = C.seb_keys{n: C.uint64_t(n)}
	pin.Pin(&b.keyOff[0])
	ks.offsets = (*C.uint64_t)(unsafe.Pointer(&b.keyOff[0]))
	if len(b.keys) > 0 {
		pin.Pin(&b.keys[0])
		ks.data = (*C.uint8_t)(unsafe.Pointer(&b.keys[0]))
	} else if n > 0 {
		pad := []byte{0} // a run of empty keys still needs a data pointer
		pin.Pin(&pad[0])
		ks.data = (*C.uint8_t)(unsafe.Pointer(&pad[0]))
	}
	valOff := (*C.uint64_t)(unsafe.Pointer(&b.valOff[0]))
	var need C.uint64_t
	image := make([]byte, 1)
	for {
		rc := C.seb_sst_build(ctx, ks, bytesPtr(b.vals), valOff, bytesPtr(b.deleted), C.int64_t(b.expectedKeys),
			bytesPtr(image), C.uint64_t(len(image)), &need)
		if rc == C.SEB_ERR_RANGE && uint64(need) > uint64(len(image)) {
			image = make([]byte, uint64(need)) // the retry contract: *need is the image's size
			continue
		}
		if rc != 0 {
			return fmt.Errorf("failed to build sstable: %s", C.GoString(C.seb_last_error()))
		}
		break
	}
	runtime.KeepAlive(b)
	if _, err := b.file.Write(image[:need]); err != nil {
		return fmt.Errorf("failed to write sstable: %w", err)
	}
	if err := b.file.Sync(); err != nil {
		return fmt.Errorf("failed to sync sstable: %w", err)
	}
	return b.file.Close()
}

// Abort closes and deletes the SSTable file.
func (b *SSTableBuilder) Abort() error {
	b.file.Close()
	return os.Remove(b.path)
}
