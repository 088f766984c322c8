// The B-tree's read side, over the "B-tree, read side" group of libseb_bloom (include/seb_bloom.h): what readMetadata
// (btree/pager.go:142-164) makes of a page file, a structural check of every page, and what Get
// (btree/btree.go:232-280) answers from the pages, for a key batch.
//
//	Open      readMetadata of a page-file image on the host (seb_bt_open): root, the header's NumPages, the free list and
//	          NumPages = the pages the image really holds, the bound every later page access is held to
//	Load      open + upload + check of a host image through a context (seb_bt_load)
//	DevCheck  the structural pass on a device image (seb_dev_bt_check): kind and level per page, the counts; synchronises
//	DevGet    status / leaf / pos / vloc / vlen / source for a device key batch (seb_dev_bt_get); (status, vloc, vlen) are
//	          the arrays the LSM Get path ends in, so lsm.DevValuesPlan / DevValuesEmit gather the values from them with
//	          the image as their pool
//	GetHost   the whole answer on the host, for a caller without a GPU (seb_bt_check, seb_bt_get)
//	Scan      BTree.Scan(startKey, endKey) on the host through the leaf directory of the "B-tree, range scans" group
//	          (seb_bt_check, seb_bt_dir_build, seb_bt_scan): the range's keys and values, dense, in key order
//	DevDirBuild / DevScanPlan / DevScanCells  the device forms (seb_dev_bt_dir_build, seb_dev_bt_scan_plan,
//	          seb_dev_bt_scan_cells); the entry arrays then go to lsm.DevValuesPlan / DevValuesEmit twice, keys and values
//
// A miss carries the leaf reached and searchCell's insertion point, which is where Iterator.seek starts.  GetError is
// an empty key, a page id outside the image, and the stated departures from the reference: a page type that is
// neither 1 nor 2, a touched cell that does not parse, a walk of more than MaxDepth pages (a cycle).
//
// The reference's splitInternal (btree/split.go:141-164) misplaces two child pointers, so trees of depth >= 3 lose
// keys to the reference's own Get; these calls follow the image and answer what that walk answers on the same bytes.
//
// Scan departs from btree/iterator.go where include/seb_bloom.h says so: an empty start begins at the tree's first key
// (the reference's descent by CellAt(0).Child skips the leftmost subtree), an empty leaf inside the chain is passed
// over, and an image whose leaf directory is refused (the reference's own depth >= 3 trees among them) is an error.
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested through
// the Python binding (tests/test_btree.py, tests/test_btree_sanitize.py, tests/test_gpu_btree.py, tests/test_btree_scan.py,
// tests/test_btree_scan_sanitize.py, tests/test_gpu_btree_scan.py).
package btree

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

// Get statuses (seb_get_status).
const (
	GetMiss  = 0
	GetFound = 1
	GetError = 2
)

// Page kinds (seb_bt_page_kind) and limits.
const (
	PageBad      = 0
	PageInternal = 1
	PageLeaf     = 2
	PageBytes    = 4096
	MaxDepth     = 32
	NoPage       = ^uint32(0) // leaf for an empty key
	NoLevel      = 0xFF       // level of a page the root does not reach
)

// Meta is readMetadata's result; NumPages = min(HeaderPages, len(image) / 4096).
type Meta struct {
	Root, HeaderPages, FreeList, NumPages uint32
}

// Stats is what the check counts.
type Stats struct {
	Leaves, Internals, Bad                uint64 // pages [1, NumPages) by kind
	ReachLeaves, ReachInternals, ReachBad uint64 // those the root reaches
	Keys                                  uint64 // cells on reachable good leaves
	Depth                                 uint32
	Uniform                               bool // every reachable good leaf sits at one level
}

// Answer is one key's result on the host.
type Answer struct {
	Status    byte
	Leaf, Pos uint32
	VLoc      uint64
	VLen      uint32
}

// DevKeys is a key batch in device memory, in the layouts seb_dev_shard_route takes.
type DevKeys struct {
	Data, Offsets unsafe.Pointer // Offsets nil: fixed-length keys of Stride bytes
	N             uint64
	Stride        uint32
}

func bytesPtr(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

func lastError(what string) error {
	return fmt.Errorf("%s: %s", what, C.GoString(C.seb_last_error()))
}

func (m Meta) c() C.seb_bt_meta {
	return C.seb_bt_meta{root: C.uint32_t(m.Root), header_pages: C.uint32_t(m.HeaderPages), free_list: C.uint32_t(m.FreeList),
		num_pages: C.uint32_t(m.NumPages)}
}

func metaOf(m C.seb_bt_meta) Meta {
	return Meta{Root: uint32(m.root), HeaderPages: uint32(m.header_pages), FreeList: uint32(m.free_list), NumPages: uint32(m.num_pages)}
}

func statsOf(s C.seb_bt_stats) Stats {
	return Stats{Leaves: uint64(s.leaves), Internals: uint64(s.internals), Bad: uint64(s.bad), ReachLeaves: uint64(s.reach_leaves),
		ReachInternals: uint64(s.reach_internals), ReachBad: uint64(s.reach_bad), Keys: uint64(s.keys), Depth: uint32(s.depth),
		Uniform: s.uniform != 0}
}

// Open is readMetadata: an error where the reference gives ErrInvalidDatabase.
func Open(image []byte) (Meta, error) {
	var m C.seb_bt_meta
	if C.seb_bt_open(bytesPtr(image), C.uint64_t(len(image)), &m) != 0 {
		return Meta{}, lastError("failed to open the page file")
	}
	return metaOf(m), nil
}

// Load opens a host image, uploads its pages into devImage (device memory of capBytes) and checks them; devKind and
// devLevel (device memory, one byte per page) may be nil.  ctx is a seb_ctx.
func Load(ctx unsafe.Pointer, image []byte, devImage unsafe.Pointer, capBytes uint64, devKind, devLevel unsafe.Pointer) (Meta, Stats, error) {
	var m C.seb_bt_meta
	var s C.seb_bt_stats
	if C.seb_bt_load((*C.seb_ctx)(ctx), bytesPtr(image), C.uint64_t(len(image)), (*C.uint8_t)(devImage), C.uint64_t(capBytes),
		(*C.uint8_t)(devKind), (*C.uint8_t)(devLevel), &m, &s) != 0 {
		return metaOf(m), Stats{}, lastError("failed to load the page file")
	}
	return metaOf(m), statsOf(s), nil
}

// DevCheck runs the structural pass on a device image; it synchronises `stream`.  kind and level may be nil.
func DevCheck(image unsafe.Pointer, imageBytes uint64, meta Meta, kind, level, stream unsafe.Pointer) (Stats, error) {
	m := meta.c()
	var s C.seb_bt_stats
	if C.seb_dev_bt_check((*C.uint8_t)(image), C.uint64_t(imageBytes), &m, (*C.uint8_t)(kind), (*C.uint8_t)(level), &s, stream) != 0 {
		return Stats{}, lastError("failed to check the page file")
	}
	return statsOf(s), nil
}

// DevGet enqueues Get for a device key batch on `stream`; not synchronised.  status is required; leaf, pos, vloc, vlen
// and source may be nil.  The image must not change while it runs.
func DevGet(image unsafe.Pointer, imageBytes uint64, meta Meta, keys DevKeys, status, leaf, pos, vloc, vlen, source,
	stream unsafe.Pointer) error {
	m := meta.c()
	kb := C.seb_keys{data: (*C.uint8_t)(keys.Data), offsets: (*C.uint64_t)(keys.Offsets), n: C.uint64_t(keys.N), stride: C.uint32_t(keys.Stride)}
	if C.seb_dev_bt_get((*C.uint8_t)(image), C.uint64_t(imageBytes), &m, &kb, (*C.uint8_t)(status), (*C.uint32_t)(leaf),
		(*C.uint32_t)(pos), (*C.uint64_t)(vloc), (*C.uint32_t)(vlen), (*C.uint8_t)(source), stream) != 0 {
		return lastError("failed to get from the B-tree")
	}
	return nil
}

// GetHost checks a host image and answers a key batch from it (keyData, keyOff: n + 1 offsets), without a GPU.
func GetHost(image []byte, keyData []byte, keyOff []uint64) ([]Answer, Meta, Stats, error) {
	meta, err := Open(image)
	if err != nil {
		return nil, meta, Stats{}, err
	}
	m := meta.c()
	var s C.seb_bt_stats
	if C.seb_bt_check(bytesPtr(image), C.uint64_t(len(image)), &m, nil, nil, &s) != 0 {
		return nil, meta, Stats{}, lastError("failed to check the page file")
	}
	n := len(keyOff) - 1
	if n < 0 {
		n = 0
	}
	status := make([]byte, n+1)
	leaf, pos, vlen := make([]uint32, n+1), make([]uint32, n+1), make([]uint32, n+1)
	vloc := make([]uint64, n+1)
	var off *C.uint64_t
	if len(keyOff) > 0 {
		off = (*C.uint64_t)(unsafe.Pointer(&keyOff[0]))
	}
	kb := C.seb_keys{data: bytesPtr(keyData), offsets: off, n: C.uint64_t(n)}
	if C.seb_bt_get(bytesPtr(image), C.uint64_t(len(image)), &m, &kb, bytesPtr(status), (*C.uint32_t)(unsafe.Pointer(&leaf[0])),
		(*C.uint32_t)(unsafe.Pointer(&pos[0])), (*C.uint64_t)(unsafe.Pointer(&vloc[0])), (*C.uint32_t)(unsafe.Pointer(&vlen[0]))) != 0 {
		return nil, meta, Stats{}, lastError("failed to get from the B-tree")
	}
	out := make([]Answer, n)
	for i := range out {
		out[i] = Answer{Status: status[i], Leaf: leaf[i], Pos: pos[i], VLoc: vloc[i], VLen: vlen[i]}
	}
	return out, meta, statsOf(s), nil
}

// Entry is one key-value pair of a scan.
type Entry struct {
	Key, Value []byte
}

// DirInfo is what a leaf directory holds: the listed leaves, the tree's keys and its levels.
type DirInfo struct {
	Leaves, Keys uint64
	Depth        uint32
}

// DirBytes is the size of an image's leaf directory.
func DirBytes(numPages uint32) uint64 { return uint64(C.seb_bt_dir_bytes(C.uint32_t(numPages))) }

// Scan is BTree.Scan(startKey, endKey) for one range [startKey, endKey) of a host image, without a GPU: at most limit
// entries (0: all) in key order.  An empty startKey starts at the first key.  endKey nil is unbounded; a non-nil empty
// endKey yields nothing, as in the reference, and is answered here without a call.
func Scan(image []byte, startKey, endKey []byte, limit uint64) ([]Entry, error) {
	if endKey != nil && len(endKey) == 0 {
		return nil, nil
	}
	meta, err := Open(image)
	if err != nil {
		return nil, err
	}
	m := meta.c()
	np := int(meta.NumPages)
	kind, level := make([]byte, np+1), make([]byte, np+1)
	if C.seb_bt_check(bytesPtr(image), C.uint64_t(len(image)), &m, bytesPtr(kind), bytesPtr(level), nil) != 0 {
		return nil, lastError("failed to check the page file")
	}
	dir := make([]uint64, DirBytes(meta.NumPages)/8+1) // 8-byte aligned
	dirPtr := (*C.uint8_t)(unsafe.Pointer(&dir[0]))
	var info C.seb_bt_dir_info
	if C.seb_bt_dir_build(bytesPtr(image), C.uint64_t(len(image)), &m, bytesPtr(kind), bytesPtr(level), dirPtr, &info) != 0 {
		return nil, lastError("failed to build the leaf directory")
	}
	one := []byte{0}
	bound := func(k []byte, off *[2]uint64) C.seb_keys {
		off[1] = uint64(len(k))
		data := bytesPtr(k)
		if len(k) == 0 {
			data = bytesPtr(one)
		}
		return C.seb_keys{data: data, offsets: (*C.uint64_t)(unsafe.Pointer(&off[0])), n: 1}
	}
	var so, eo [2]uint64
	ks, ke := bound(startKey, &so), bound(endKey, &eo)
	var rangeStatus [1]byte
	var rangeOff [2]uint64
	var sz C.seb_bt_scan_sizes
	rs, ro := (*C.uint8_t)(unsafe.Pointer(&rangeStatus[0])), (*C.uint64_t)(unsafe.Pointer(&rangeOff[0]))
	// the sizing call: no entry outputs, caps of 0; SEB_ERR_RANGE with the sizes filled is its expected answer
	C.seb_bt_scan(bytesPtr(image), C.uint64_t(len(image)), &m, dirPtr, &ks, &ke, C.uint64_t(limit), rs, ro, nil, nil, nil, nil, nil, nil,
		0, nil, nil, 0, nil, nil, 0, &sz)
	if rangeStatus[0] != 0 {
		return nil, fmt.Errorf("failed to seek: the walk met a page the image does not hold whole")
	}
	n := int(sz.entries)
	if n == 0 {
		return nil, nil
	}
	status, source := make([]byte, n), make([]byte, n)
	kloc, vloc, keyOff, valOff := make([]uint64, n), make([]uint64, n), make([]uint64, n+1), make([]uint64, n+1)
	klen, vlen := make([]uint32, n), make([]uint32, n)
	keys, vals := make([]byte, int(sz.key_bytes)+1), make([]byte, int(sz.val_bytes)+1)
	u64 := func(p []uint64) *C.uint64_t { return (*C.uint64_t)(unsafe.Pointer(&p[0])) }
	u32 := func(p []uint32) *C.uint32_t { return (*C.uint32_t)(unsafe.Pointer(&p[0])) }
	if C.seb_bt_scan(bytesPtr(image), C.uint64_t(len(image)), &m, dirPtr, &ks, &ke, C.uint64_t(limit), rs, ro, bytesPtr(status),
		bytesPtr(source), u64(kloc), u32(klen), u64(vloc), u32(vlen), C.uint64_t(n), u64(keyOff), bytesPtr(keys), sz.key_bytes,
		u64(valOff), bytesPtr(vals), sz.val_bytes, &sz) != 0 {
		return nil, lastError("failed to scan the B-tree")
	}
	out := make([]Entry, n)
	for i := range out {
		out[i] = Entry{Key: keys[keyOff[i]:keyOff[i+1]], Value: vals[valOff[i]:valOff[i+1]]}
	}
	return out, nil
}

// DevDirBuild builds the leaf directory of a checked device image into dir (device memory of DirBytes(meta.NumPages),
// 8-byte aligned); kind and level as DevCheck wrote them; workspace: device memory of
// seb_dev_bt_dir_workspace_size(meta.NumPages) bytes, 16-byte aligned.  It synchronises `stream`.
func DevDirBuild(image unsafe.Pointer, imageBytes uint64, meta Meta, kind, level, dir, workspace unsafe.Pointer, workspaceBytes uint64,
	stream unsafe.Pointer) (DirInfo, error) {
	m := meta.c()
	var info C.seb_bt_dir_info
	if C.seb_dev_bt_dir_build((*C.uint8_t)(image), C.uint64_t(imageBytes), &m, (*C.uint8_t)(kind), (*C.uint8_t)(level), (*C.uint8_t)(dir),
		workspace, C.uint64_t(workspaceBytes), &info, stream) != 0 {
		return DirInfo{}, lastError("failed to build the leaf directory")
	}
	return DirInfo{Leaves: uint64(info.leaves), Keys: uint64(info.keys), Depth: uint32(info.depth)}, nil
}

func (k DevKeys) c() C.seb_keys {
	return C.seb_keys{data: (*C.uint8_t)(k.Data), offsets: (*C.uint64_t)(k.Offsets), n: C.uint64_t(k.N), stride: C.uint32_t(k.Stride)}
}

// DevScanPlan sizes a batch of ranges (starts.N == ends.N; an empty bound: from the first key / unbounded); it writes
// rangeStatus (one byte per range), keeps the plan in workspace (seb_dev_bt_scan_workspace_size(starts.N) bytes) and
// synchronises `stream`.  It returns the entry count that DevScanCells takes.
func DevScanPlan(image unsafe.Pointer, imageBytes uint64, meta Meta, dir unsafe.Pointer, starts, ends DevKeys, limit uint64,
	rangeStatus, workspace unsafe.Pointer, workspaceBytes uint64, stream unsafe.Pointer) (uint64, error) {
	m := meta.c()
	ks, ke := starts.c(), ends.c()
	var sz C.seb_bt_scan_sizes
	if C.seb_dev_bt_scan_plan((*C.uint8_t)(image), C.uint64_t(imageBytes), &m, (*C.uint8_t)(dir), &ks, &ke, C.uint64_t(limit),
		(*C.uint8_t)(rangeStatus), workspace, C.uint64_t(workspaceBytes), &sz, stream) != 0 {
		return uint64(sz.entries), lastError("failed to plan the scan")
	}
	return uint64(sz.entries), nil
}

// DevScanCells enqueues the scan's outputs on `stream` (not synchronised): rangeOff (ranges + 1 u64) and per entry
// status / source (u8), kloc / vloc (u64), klen / vlen (u32): what lsm.DevValuesPlan / DevValuesEmit take with the image
// as their pool, once over (kloc, klen) for the keys and once over (vloc, vlen) for the values.
func DevScanCells(image unsafe.Pointer, imageBytes uint64, meta Meta, dir unsafe.Pointer, ranges, entries uint64, workspace unsafe.Pointer,
	workspaceBytes uint64, rangeOff, status, source, kloc, klen, vloc, vlen, stream unsafe.Pointer) error {
	m := meta.c()
	sz := C.seb_bt_scan_sizes{ranges: C.uint64_t(ranges), entries: C.uint64_t(entries)}
	if C.seb_dev_bt_scan_cells((*C.uint8_t)(image), C.uint64_t(imageBytes), &m, (*C.uint8_t)(dir), &sz, workspace, C.uint64_t(workspaceBytes),
		(*C.uint64_t)(rangeOff), (*C.uint8_t)(status), (*C.uint8_t)(source), (*C.uint64_t)(kloc), (*C.uint32_t)(klen), (*C.uint64_t)(vloc),
		(*C.uint32_t)(vlen), stream) != 0 {
		return lastError("failed to scan the B-tree")
	}
	return nil
}
