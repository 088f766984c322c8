// The last step of a GetBatch, over the Get values group of libseb_bloom (include/seb_bloom.h): LSM.Get returns the
// value, a copy of the block's bytes (lsm/sstable.go:276-278) or the memtable entry's Value (lsm/lsm.go:146-152,
// 157-163, 175-180).  The join (get_compact.go) ends with a place per key; this step copies the found keys' values
// back to back into one buffer, in batch order, with an offset array.
//
//	values  outOff[0..n] and outVals[0, outOff[n]): key i's value is outVals[outOff[i]:outOff[i+1]], empty for a key
//	        that is not found (seb_get_values on host memory; seb_dev_get_values_plan / _emit on device memory)
//
// The call order of a GetBatch that keeps its batch on the device and ends in bytes: seb_dev_runs_search (with its
// run output), CompactPlan, CompactEmit, FilterRegistry's MultiGet list, locate, block ids, block search and
// resolve on the m compacted keys, JoinRows, ValuesPlan, ValuesEmit, then one seb_memcpy_d2h of outOff and one of
// outVals.
//
// One stated refusal: a found key whose value does not lie inside the source it names fails the whole batch
// ("key K"); skipping it would be a Get that returns the wrong bytes.
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_values.py, tests/test_gpu_values.py).
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

// ValuesSizes is seb_values_sizes: what a plan returns and an emit takes.
type ValuesSizes struct {
	N, Found, ValBytes uint64
}

// gatherValues is the host half: answers as joinRows returned them, run[i] the deciding run of a key the
// memtables decided (nil with at most one run), runVals the runs' value bytes and pool the block pool.  The value
// of key i is vals[off[i]:off[i+1]].
func gatherValues(answers []GetAnswer, run []byte, runVals [][]byte, pool []byte) (off []uint64, vals []byte, err error) {
	n := len(answers)
	status, source := make([]byte, n), make([]byte, n)
	vloc := make([]uint64, n)
	vlen := make([]uint32, n)
	for i, a := range answers {
		status[i], source[i], vloc[i], vlen[i] = a.Status, a.Source, a.VLoc, a.VLen
	}
	// the runs' pointers live in C memory for the call (cgo forbids Go pointers to Go pointers)
	ptrs := (**C.uint8_t)(C.calloc(C.size_t(len(runVals)+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(ptrs))
	pv := unsafe.Slice(ptrs, len(runVals)+1)
	sizes := make([]uint64, len(runVals)+1)
	for r, v := range runVals {
		pv[r], sizes[r] = bytesPtr(v), uint64(len(v))
	}
	call := func(sz *C.seb_values_sizes, off []uint64, vals []byte) C.int {
		return C.seb_get_values(bytesPtr(status), bytesPtr(source), bytesPtr(run), u64Ptr(vloc), u32Ptr(vlen), C.uint64_t(n),
			ptrs, u64Ptr(sizes), C.uint32_t(len(runVals)), bytesPtr(pool), C.uint64_t(len(pool)), sz, u64Ptr(off), bytesPtr(vals),
			C.uint64_t(len(vals)))
	}
	var sz C.seb_values_sizes
	if call(&sz, nil, nil) != 0 { // the plan: sizes only
		return nil, nil, fmt.Errorf("failed to gather values: %s", C.GoString(C.seb_last_error()))
	}
	off = make([]uint64, n+1)
	vals = make([]byte, sz.val_bytes)
	if call(&sz, off, vals) != 0 {
		return nil, nil, fmt.Errorf("failed to gather values: %s", C.GoString(C.seb_last_error()))
	}
	return off, vals, nil
}

// The device form: every array below is device memory the caller owns, `stream` its HIP stream; runVals and
// runBytes are host slices of device pointers and sizes, one per run.

// DevValuesWorkspaceSize is the workspace a plan of n keys needs (16-byte aligned device memory).
func DevValuesWorkspaceSize(n uint64) uint64 {
	return uint64(C.seb_dev_get_values_workspace_size(C.uint64_t(n)))
}

// DevValuesInputs are the arrays seb_dev_get_join_rows and seb_dev_runs_search left on the device, and the sources.
type DevValuesInputs struct {
	Status, Source, Run, VLoc, VLen unsafe.Pointer
	N                               uint64
	RunVals                         []unsafe.Pointer
	RunBytes                        []uint64
	Pool                            unsafe.Pointer
	PoolBytes                       uint64
}

func (in *DevValuesInputs) runs() (**C.uint8_t, func()) {
	ptrs := (**C.uint8_t)(C.calloc(C.size_t(len(in.RunVals)+1), C.size_t(unsafe.Sizeof(uintptr(0)))))
	pv := unsafe.Slice(ptrs, len(in.RunVals)+1)
	for r, p := range in.RunVals {
		pv[r] = (*C.uint8_t)(p)
	}
	return ptrs, func() { C.free(unsafe.Pointer(ptrs)) }
}

// DevValuesPlan sizes the gather; it synchronises the stream.  An invalid found key is an error naming it.
func DevValuesPlan(in *DevValuesInputs, workspace unsafe.Pointer, workspaceBytes uint64, stream unsafe.Pointer) (ValuesSizes, error) {
	ptrs, free := in.runs()
	defer free()
	var sz C.seb_values_sizes
	rc := C.seb_dev_get_values_plan((*C.uint8_t)(in.Status), (*C.uint8_t)(in.Source), (*C.uint8_t)(in.Run),
		(*C.uint64_t)(in.VLoc), (*C.uint32_t)(in.VLen), C.uint64_t(in.N), ptrs, u64Ptr(in.RunBytes),
		C.uint32_t(len(in.RunVals)), (*C.uint8_t)(in.Pool), C.uint64_t(in.PoolBytes), workspace, C.uint64_t(workspaceBytes),
		&sz, stream)
	if rc != 0 {
		return ValuesSizes{}, fmt.Errorf("failed to plan the values' gather: %s", C.GoString(C.seb_last_error()))
	}
	return ValuesSizes{N: uint64(sz.n), Found: uint64(sz.found), ValBytes: uint64(sz.val_bytes)}, nil
}

// DevValuesEmit writes outOff[0, N] and outVals[0, ValBytes); not synchronised.  The same inputs and workspace as
// the plan.
func DevValuesEmit(in *DevValuesInputs, sizes ValuesSizes, workspace, outOff, outVals, stream unsafe.Pointer) error {
	ptrs, free := in.runs()
	defer free()
	sz := C.seb_values_sizes{n: C.uint64_t(sizes.N), found: C.uint64_t(sizes.Found), val_bytes: C.uint64_t(sizes.ValBytes)}
	rc := C.seb_dev_get_values_emit((*C.uint8_t)(in.Status), (*C.uint8_t)(in.Source), (*C.uint8_t)(in.Run),
		(*C.uint64_t)(in.VLoc), (*C.uint32_t)(in.VLen), C.uint64_t(in.N), ptrs, u64Ptr(in.RunBytes),
		C.uint32_t(len(in.RunVals)), (*C.uint8_t)(in.Pool), C.uint64_t(in.PoolBytes), &sz, workspace, (*C.uint64_t)(outOff),
		(*C.uint8_t)(outVals), stream)
	if rc != 0 {
		return fmt.Errorf("failed to gather values: %s", C.GoString(C.seb_last_error()))
	}
	return nil
}
