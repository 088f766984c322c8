// The hash index, over the hash index groups of libseb_bloom (include/seb_bloom.h): what
// recover() (hashindex/recovery.go) makes of the segment files, and what Get (hashindex/hashindex.go:217-260 ->
// segment.read) answers from them, for a key batch.
//
//	Recover   the segment files (oldest first) into a device pool and a device key table: scan on the host, upload,
//	          CRC pass with the cuts, insert (seb_hidx_recover); per segment the valid records, the size after
//	          recovery, whether it was cut and whether it ends in a short tail; the key count, tombstones included
//	LookupHost the whole answer on the host, for a caller without a GPU (seb_seg_scan, seb_seg_verify, seb_hidx_lookup)
//	DevGet    status / rec / vloc / vlen / source for a device key batch (seb_dev_hidx_get); the three arrays the LSM
//	          Get path ends in, so lsm.DevValuesPlan / DevValuesEmit gather the values from them with the segment
//	          pool as their pool
//	DevInsert records appended to the active segment into the same table (seb_dev_seg_verify, seb_dev_hidx_insert,
//	          seb_dev_hidx_count)
//
//	Frame     a Put / Delete batch as segment.append's sealed records in device memory, with the rotation's cuts
//	          (seb_dev_seg_frame_plan, seb_dev_seg_frame_emit); FrameHost is the same on the host
//	Compact   compactSegments + applyCompaction for the oldest c segments of a device pool (seb_hidx_compact): the
//	          survivors in log order at the front of a new pool, the other segments behind, the table rebuilt
//	LogicalSize getLogicalSize over the table (seb_dev_hidx_logical_size)
//
// One stated departure: a header with keySize + valueSize >= 2^32 counts as a CRC failure and cuts its segment; the
// reference adds the two as uint32 and then fails the CRC or panics on the slice.
//
// NAMING THE COMPACTED FILE.  The reference names the compacted segment with the current time, so its id is above
// every segment it did not compact, and after a restart its own recover() replays the compacted (older) records over
// newer ones.  The table Compact leaves equals the live index after applyCompaction: the compacted image lies at the
// LOWEST pool offsets, so newer segments still win.  An engine that wants recover() to rebuild that same index must
// name the compacted file so that it sorts BEFORE the segments it did not compact (the id of the newest compacted
// segment, say).
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested through
// the Python binding (tests/test_hashindex.py, tests/test_gpu_hashindex.py, tests/test_hashwrite.py,
// tests/test_gpu_hashwrite.py).
package hashindex

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
	GetError = 2 // the record's CRC does not match
)

// NoRecord is rec for a key that is not found.
const NoRecord = ^uint64(0)

func bytesPtr(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

func u64Ptr(v []uint64) *C.uint64_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&v[0]))
}

func lastError(what string) error {
	return fmt.Errorf("%s: %s", what, C.GoString(C.seb_last_error()))
}

// TableBytes is the device memory a table of `capacity` keys needs (16-byte aligned).
func TableBytes(capacity uint64) uint64 { return uint64(C.seb_dev_hidx_table_bytes(C.uint64_t(capacity))) }

// Recovered is what recover() leaves per segment, and the index's size.
type Recovered struct {
	Valid, SizeAfter []uint64
	ShortTail, Cut   []bool
	Records          uint64 // scanned
	LiveRecords      uint64 // the sum of Valid
	Keys             uint64 // distinct keys, tombstones included (HashIndex.Count after recovery)
}

// ErrTableFull is returned with Recovered filled (but for Keys): retry with capacity = LiveRecords.
var ErrTableFull = fmt.Errorf("the key table filled")

// Recover runs recover() for the segment files (host bytes, oldest first) on ctx (a seb_ctx): devPool (device
// memory of poolCap bytes, at least the files' total) receives them back to back, devTable (TableBytes(capacity)
// bytes of device memory) the index.
func Recover(ctx unsafe.Pointer, segments [][]byte, devPool unsafe.Pointer, poolCap uint64, devTable unsafe.Pointer, capacity uint64) (*Recovered, error) {
	s := len(segments)
	// the images' pointers live in C memory for the call (cgo forbids Go pointers to Go pointers)
	ptrs := (**C.uint8_t)(C.calloc(C.size_t(s+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(ptrs))
	pv := unsafe.Slice(ptrs, s+1)
	sizes := make([]uint64, s+1)
	for i, seg := range segments {
		pv[i], sizes[i] = bytesPtr(seg), uint64(len(seg))
	}
	r := &Recovered{Valid: make([]uint64, s), SizeAfter: make([]uint64, s), ShortTail: make([]bool, s), Cut: make([]bool, s)}
	tail, cut := make([]byte, s+1), make([]byte, s+1)
	var records, live, keys C.uint64_t
	rc := C.seb_hidx_recover((*C.seb_ctx)(ctx), ptrs, u64Ptr(sizes), C.uint64_t(s), (*C.uint8_t)(devPool), C.uint64_t(poolCap),
		devTable, C.uint64_t(capacity), u64Ptr(r.Valid), u64Ptr(r.SizeAfter), bytesPtr(tail), bytesPtr(cut), &records, &live, &keys)
	for i := 0; i < s; i++ {
		r.ShortTail[i], r.Cut[i] = tail[i] != 0, cut[i] != 0
	}
	r.Records, r.LiveRecords, r.Keys = uint64(records), uint64(live), uint64(keys)
	if rc == C.SEB_ERR_RANGE && r.LiveRecords > capacity {
		return r, ErrTableFull
	}
	if rc != 0 {
		return nil, lastError("failed to recover the hash index")
	}
	return r, nil
}

// Answer is one key's Get: Status, the record's pool offset, and where its value lies in the pool.
type Answer struct {
	Status byte
	Rec    uint64
	VLoc   uint64
	VLen   uint32
}

// LookupHost is recover() and Get on the host: the segments are scanned and verified, the index is a map built
// inside the call.  keys in the variable-length layout: key i = keyData[keyOff[i]:keyOff[i+1]].
func LookupHost(segments [][]byte, keyData []byte, keyOff []uint64, verify bool) ([]Answer, *Recovered, error) {
	s := len(segments)
	var pool []byte
	var recOff []uint64
	first, base, size := make([]uint64, s+1), make([]uint64, s+1), make([]uint64, s+1)
	r := &Recovered{Valid: make([]uint64, s), SizeAfter: make([]uint64, s), ShortTail: make([]bool, s), Cut: make([]bool, s)}
	for i, seg := range segments {
		off := make([]uint64, len(seg)/int(C.SEB_SEG_HEADER_BYTES)+1)
		var n C.uint64_t
		var tail C.int
		if C.seb_seg_scan(bytesPtr(seg), C.uint64_t(len(seg)), C.uint64_t(len(pool)), u64Ptr(off), C.uint64_t(len(off)), &n, &tail) != 0 {
			return nil, nil, lastError("failed to scan a segment")
		}
		first[i], base[i], size[i] = uint64(len(recOff)), uint64(len(pool)), uint64(len(seg))
		r.ShortTail[i] = tail != 0
		recOff = append(recOff, off[:n]...)
		pool = append(pool, seg...)
	}
	first[s] = uint64(len(recOff))
	live := make([]byte, len(recOff)+1)
	if C.seb_seg_verify(bytesPtr(pool), C.uint64_t(len(pool)), u64Ptr(recOff), C.uint64_t(len(recOff)), u64Ptr(first), u64Ptr(base),
		u64Ptr(size), C.uint64_t(s), nil, u64Ptr(r.Valid), u64Ptr(r.SizeAfter), bytesPtr(live)) != 0 {
		return nil, nil, lastError("failed to verify the segments")
	}
	for i := 0; i < s; i++ {
		r.Cut[i] = r.Valid[i] < first[i+1]-first[i]
		r.ShortTail[i] = r.ShortTail[i] && !r.Cut[i]
		r.LiveRecords += r.Valid[i]
	}
	r.Records = uint64(len(recOff))
	n := len(keyOff) - 1
	if n < 0 {
		n = 0
	}
	status := make([]byte, n+1)
	rec, vloc := make([]uint64, n+1), make([]uint64, n+1)
	vlen := make([]uint32, n+1)
	kb := C.seb_keys{data: bytesPtr(keyData), offsets: u64Ptr(keyOff), n: C.uint64_t(n)}
	v := C.int(0)
	if verify {
		v = 1
	}
	var keys C.uint64_t
	if C.seb_hidx_lookup(bytesPtr(pool), C.uint64_t(len(pool)), u64Ptr(recOff), bytesPtr(live), C.uint64_t(len(recOff)), &kb, v,
		bytesPtr(status), u64Ptr(rec), u64Ptr(vloc), (*C.uint32_t)(unsafe.Pointer(&vlen[0])), &keys) != 0 {
		return nil, nil, lastError("failed to look the keys up")
	}
	r.Keys = uint64(keys)
	out := make([]Answer, n)
	for i := range out {
		out[i] = Answer{Status: status[i], Rec: rec[i], VLoc: vloc[i], VLen: vlen[i]}
	}
	return out, r, nil
}

// DevKeys is a key batch in device memory, in the layouts seb_dev_shard_route takes.
type DevKeys struct {
	Data, Offsets unsafe.Pointer // Offsets nil: fixed-length keys of Stride bytes
	N             uint64
	Stride        uint32
}

// DevGet enqueues Get for a device key batch on `stream`; not synchronised.  status is required; rec, vloc, vlen and
// source may be nil.  No DevInsert may run concurrently on the same table.
func DevGet(table unsafe.Pointer, capacity uint64, pool unsafe.Pointer, poolBytes uint64, keys DevKeys, verify bool,
	status, rec, vloc, vlen, source, stream unsafe.Pointer) error {
	kb := C.seb_keys{data: (*C.uint8_t)(keys.Data), offsets: (*C.uint64_t)(keys.Offsets), n: C.uint64_t(keys.N), stride: C.uint32_t(keys.Stride)}
	v := C.int(0)
	if verify {
		v = 1
	}
	if C.seb_dev_hidx_get(table, C.uint64_t(capacity), (*C.uint8_t)(pool), C.uint64_t(poolBytes), &kb, v, (*C.uint8_t)(status),
		(*C.uint64_t)(rec), (*C.uint64_t)(vloc), (*C.uint32_t)(vlen), (*C.uint8_t)(source), stream) != 0 {
		return lastError("failed to get from the hash index")
	}
	return nil
}

// DevInsert verifies n appended records (recOff: their pool offsets in device memory, all of one segment; ok, live:
// n device bytes each; valid: one device u64) and inserts the live ones; it synchronises and returns the key count.
// The pool must already hold the records' bytes.  ErrTableFull: clear a larger table and insert everything again.
func DevInsert(table unsafe.Pointer, capacity uint64, pool unsafe.Pointer, poolBytes uint64, recOff unsafe.Pointer, n uint64,
	segFirst, ok, live, valid, stream unsafe.Pointer) (uint64, error) {
	if C.seb_dev_seg_verify((*C.uint8_t)(pool), C.uint64_t(poolBytes), (*C.uint64_t)(recOff), C.uint64_t(n), (*C.uint64_t)(segFirst), 1,
		(*C.uint8_t)(ok), (*C.uint64_t)(valid), (*C.uint8_t)(live), stream) != 0 {
		return 0, lastError("failed to verify the appended records")
	}
	if C.seb_dev_hidx_insert(table, C.uint64_t(capacity), (*C.uint8_t)(pool), C.uint64_t(poolBytes), (*C.uint64_t)(recOff),
		(*C.uint8_t)(live), C.uint64_t(n), stream) != 0 {
		return 0, lastError("failed to insert into the hash index")
	}
	var keys C.uint64_t
	switch C.seb_dev_hidx_count(table, C.uint64_t(capacity), &keys, nil, stream) {
	case 0:
		return uint64(keys), nil
	case C.SEB_ERR_RANGE:
		return 0, ErrTableFull
	}
	return 0, lastError("failed to count the hash index")
}

// DevClear empties a table; not synchronised.
func DevClear(table unsafe.Pointer, capacity uint64, stream unsafe.Pointer) error {
	if C.seb_dev_hidx_clear(table, C.uint64_t(capacity), stream) != 0 {
		return lastError("failed to clear the hash index")
	}
	return nil
}

// Ops is a Put / Delete batch in device memory: keys in DevKeys' layouts, op i's value = Vals[ValOff[i]:ValOff[i+1]]
// (ValOff: n + 1 u64, ValOff[0] may be != 0), Deleted (nil: none) one byte per op; a Delete's value bytes are ignored.
type Ops struct {
	Keys                  DevKeys
	Vals, ValOff, Deleted unsafe.Pointer
}

// Framed is what a frame plan returns: the image's size and, for rotation at `limit` behind activeSize bytes of the
// active segment, the first op of each new segment.  Ops [0, Cuts[0]) stay in the active one; the engine splits the
// image at recOff[Cuts[k]].
type Framed struct {
	ImageBytes uint64
	Cuts       []uint64
}

// ErrCuts is returned with Framed.Cuts sized to the need where cutCap was too small.
var ErrCuts = fmt.Errorf("more cuts than cutCap")

// FramePlan sizes the batch: recOff (n + 1 device u64) is written, the call synchronises.  An empty key, a key or a
// value of 2^32 bytes or more, keySize + valueSize >= 2^32 and offsets that decrease are refused, naming the op.
func FramePlan(ops Ops, activeSize, limit uint64, recOff unsafe.Pointer, cutCap uint64, stream unsafe.Pointer) (*Framed, error) {
	kb := C.seb_keys{data: (*C.uint8_t)(ops.Keys.Data), offsets: (*C.uint64_t)(ops.Keys.Offsets), n: C.uint64_t(ops.Keys.N),
		stride: C.uint32_t(ops.Keys.Stride)}
	cuts := make([]uint64, cutCap+1)
	var total, ncuts C.uint64_t
	rc := C.seb_dev_seg_frame_plan(&kb, (*C.uint64_t)(ops.ValOff), (*C.uint8_t)(ops.Deleted), C.uint64_t(activeSize), C.uint64_t(limit),
		(*C.uint64_t)(recOff), u64Ptr(cuts), C.uint64_t(cutCap), &total, &ncuts, stream)
	if rc == C.SEB_ERR_RANGE {
		return &Framed{Cuts: make([]uint64, uint64(ncuts))}, ErrCuts
	}
	if rc != 0 {
		return nil, lastError("failed to plan the segment frame")
	}
	return &Framed{ImageBytes: uint64(total), Cuts: cuts[:ncuts]}, nil
}

// Frame writes the sealed records (every one with `timestamp`, the reference's time.Now().Unix()) into image
// (ImageBytes bytes of device memory, any alignment: the pool behind its last byte, say); not synchronised.
func Frame(ops Ops, timestamp uint64, recOff, image unsafe.Pointer, imageBytes uint64, stream unsafe.Pointer) error {
	kb := C.seb_keys{data: (*C.uint8_t)(ops.Keys.Data), offsets: (*C.uint64_t)(ops.Keys.Offsets), n: C.uint64_t(ops.Keys.N),
		stride: C.uint32_t(ops.Keys.Stride)}
	if C.seb_dev_seg_frame_emit(&kb, (*C.uint8_t)(ops.Vals), (*C.uint64_t)(ops.ValOff), (*C.uint8_t)(ops.Deleted), C.uint64_t(timestamp),
		(*C.uint64_t)(recOff), (*C.uint8_t)(image), C.uint64_t(imageBytes), stream) != 0 {
		return lastError("failed to frame the batch")
	}
	return nil
}

// FrameHost is the same on the host: key i = keyData[keyOff[i]:keyOff[i+1]], value i = vals[valOff[i]:valOff[i+1]].
// It returns the sealed image, the records' boundaries and the cuts.
func FrameHost(keyData []byte, keyOff []uint64, vals []byte, valOff []uint64, deleted []byte, timestamp, activeSize, limit uint64) ([]byte, []uint64, []uint64, error) {
	n := len(keyOff) - 1
	if n < 0 {
		n = 0
	}
	kb := C.seb_keys{data: bytesPtr(keyData), offsets: u64Ptr(keyOff), n: C.uint64_t(n)}
	recOff, cuts := make([]uint64, n+1), make([]uint64, n+1)
	var total, ncuts C.uint64_t
	if C.seb_seg_frame_plan(&kb, u64Ptr(valOff), bytesPtr(deleted), C.uint64_t(activeSize), C.uint64_t(limit), u64Ptr(recOff), u64Ptr(cuts),
		C.uint64_t(n), &total, &ncuts) != 0 {
		return nil, nil, nil, lastError("failed to plan the segment frame")
	}
	image := make([]byte, uint64(total))
	if C.seb_seg_frame_emit(&kb, bytesPtr(vals), u64Ptr(valOff), bytesPtr(deleted), C.uint64_t(timestamp), bytesPtr(image), total) != 0 {
		return nil, nil, nil, lastError("failed to frame the batch")
	}
	return image, recOff, cuts[:ncuts], nil
}

// Compacted is what a compaction leaves: its counters, the new pool's segments, and the key count.
type Compacted struct {
	RecordsIn, LiveIn, Distinct, Survivors, Tombstoned, Shadowed, ImageBytes uint64
	SegBase, SegBytes                                                        []uint64 // the new image first
	Keys                                                                     uint64
}

// ErrCapacity is returned with Compacted's sizes and segments filled where dstCap or newRecCap is below the need
// (ImageBytes + the bytes of the segments that stay; Survivors + restRecords + 1).
var ErrCapacity = fmt.Errorf("a capacity is below the compaction's sizes")

// Compact runs compactSegments + applyCompaction on ctx for the oldest c of the segments that devPool holds back to
// back (segBase / segBytes, oldest first).  A bad record in one of the c segments aborts, as the reference does.  The
// segments that stay come with their live records' offsets (restRecOff, restLive: device memory).  dstPool receives
// the new image and those segments, newRecOff (device u64) every record's offset in it, devTable the rebuilt index.
// See "naming the compacted file" above.
func Compact(ctx unsafe.Pointer, devPool unsafe.Pointer, poolBytes uint64, segBase, segBytes []uint64, c uint64,
	restRecOff, restLive unsafe.Pointer, restRecords, timestamp uint64, dstPool unsafe.Pointer, dstCap uint64,
	devTable unsafe.Pointer, capacity uint64, newRecOff unsafe.Pointer, newRecCap uint64) (*Compacted, error) {
	s := uint64(len(segBase))
	out := &Compacted{SegBase: make([]uint64, s+1), SegBytes: make([]uint64, s+1)}
	var sz C.seb_segcompact_sizes
	var keys C.uint64_t
	rc := C.seb_hidx_compact((*C.seb_ctx)(ctx), (*C.uint8_t)(devPool), C.uint64_t(poolBytes), u64Ptr(segBase), u64Ptr(segBytes),
		C.uint64_t(s), C.uint64_t(c), (*C.uint64_t)(restRecOff), (*C.uint8_t)(restLive), C.uint64_t(restRecords), C.uint64_t(timestamp),
		(*C.uint8_t)(dstPool), C.uint64_t(dstCap), devTable, C.uint64_t(capacity), (*C.uint64_t)(newRecOff), C.uint64_t(newRecCap), &sz,
		u64Ptr(out.SegBase), u64Ptr(out.SegBytes), &keys)
	out.RecordsIn, out.LiveIn, out.Distinct, out.Survivors = uint64(sz.records_in), uint64(sz.live_in), uint64(sz.distinct), uint64(sz.survivors)
	out.Tombstoned, out.Shadowed, out.ImageBytes, out.Keys = uint64(sz.tombstoned), uint64(sz.shadowed), uint64(sz.image_bytes), uint64(keys)
	if c >= 1 && c <= s {
		out.SegBase, out.SegBytes = out.SegBase[:s-c+1], out.SegBytes[:s-c+1]
	}
	if rc == C.SEB_ERR_RANGE {
		return out, ErrCapacity
	}
	if rc != 0 {
		return nil, lastError("failed to compact the hash index")
	}
	return out, nil
}

// LogicalSize is getLogicalSize (hashindex.go:360-385): keySize + valueSize over the table's entries, tombstoned keys
// included; the denominator of the space-amplification trigger.  It synchronises.
func LogicalSize(table unsafe.Pointer, capacity uint64, pool unsafe.Pointer, poolBytes uint64, stream unsafe.Pointer) (uint64, error) {
	var v C.uint64_t
	if C.seb_dev_hidx_logical_size(table, C.uint64_t(capacity), (*C.uint8_t)(pool), C.uint64_t(poolBytes), &v, stream) != 0 {
		return 0, lastError("failed to take the logical size")
	}
	return uint64(v), nil
}
