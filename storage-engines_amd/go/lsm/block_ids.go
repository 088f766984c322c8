// The step between a GetBatch's block locate and its block search, over the block-id group of libseb_bloom
// (include/seb_bloom.h): a located cell (registry slot, block offset) becomes an id of the caller's block pool.
//
//	resident  a file whose data section lies in the pool as blocks first .. first + count - 1 is mapped by
//	          arithmetic (DevBlockIDsResident: one kernel, the whole step for a tree that is all resident)
//	miss      the other cells' distinct (slot, offset) pairs are numbered in order of first appearance; the pair of
//	          rank r is entry r of the read list, and the caller reads that block into pool block idBase + r
//	          (blockIDs on host memory; DevBlockIDsPlan / DevBlockIDsEmit on device memory)
//
// The call order of a GetBatch that keeps its batch on the device: FilterRegistry's MultiGet list, locate,
// DevBlockIDsPlan, DevBlockIDsEmit, the reads of the list's blocks, block search, resolve.
//
// No departure from the reference: readBlock is asked for exactly the (file, offset) pairs SSTable.Get would read,
// each once.  Offsets of 2^48 and more are refused (no file is 256 TiB).
//
// Not compiled in this repository's pipeline (no Go toolchain in the image); the C ABI it calls is tested
// through the Python binding (tests/test_blockids.py, tests/test_gpu_blockids.py).
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

// NoBlockID is SEB_NO_BLOCK_ID: a cell without a block to search, and a slot of the residency table whose file is
// not resident.
const NoBlockID = ^uint32(0)

// BlockIDSizes is seb_blockids_sizes: what a plan returns and an emit takes.
type BlockIDSizes struct {
	Cells, Resident, Misses, Uniq, Bad uint64
}

// Residency says where the resident files' data sections lie in the pool: First[slot] is the file's first pool
// block (NoBlockID: not resident), Count[slot] its number of blocks.  Slots past len(First) are not resident.
type Residency struct {
	First, Count []uint32
}

// BlockRead is one entry of the read list: block Offset of the file in registry slot Slot.
type BlockRead struct {
	Slot   uint16
	Offset uint64
}

func u16Ptr(s []uint16) *C.uint16_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint16_t)(unsafe.Pointer(&s[0]))
}

func blockIDSizes(sz *C.seb_blockids_sizes) BlockIDSizes {
	return BlockIDSizes{Cells: uint64(sz.cells), Resident: uint64(sz.resident), Misses: uint64(sz.misses),
		Uniq: uint64(sz.uniq), Bad: uint64(sz.bad)}
}

// blockIDs is the host half: cand and blocks as the MultiGet list and the locate wrote them, one element per
// cell.  It returns each cell's pool id and the read list; read r belongs in pool block idBase + r.
func blockIDs(cand []uint16, blocks []uint64, res Residency, idBase uint32) (bid []uint32, reads []BlockRead,
	sizes BlockIDSizes, err error) {
	if len(cand) != len(blocks) || len(res.First) != len(res.Count) {
		return nil, nil, BlockIDSizes{}, fmt.Errorf("failed to map block ids: %d slots for %d offsets, %d firsts for %d counts",
			len(cand), len(blocks), len(res.First), len(res.Count))
	}
	cells, slots := C.uint64_t(len(cand)), C.uint32_t(len(res.First))
	var sz C.seb_blockids_sizes
	if C.seb_block_ids(u16Ptr(cand), u64Ptr(blocks), cells, u32Ptr(res.First), u32Ptr(res.Count), slots,
		C.uint32_t(idBase), nil, nil, nil, 0, &sz) != 0 { // the sizes alone
		return nil, nil, BlockIDSizes{}, fmt.Errorf("failed to map block ids: %s", C.GoString(C.seb_last_error()))
	}
	bid = make([]uint32, len(cand))
	uniqSlot := make([]uint16, sz.uniq)
	uniqBlock := make([]uint64, sz.uniq)
	if C.seb_block_ids(u16Ptr(cand), u64Ptr(blocks), cells, u32Ptr(res.First), u32Ptr(res.Count), slots,
		C.uint32_t(idBase), u32Ptr(bid), u16Ptr(uniqSlot), u64Ptr(uniqBlock), sz.uniq, &sz) != 0 {
		return nil, nil, BlockIDSizes{}, fmt.Errorf("failed to map block ids: %s", C.GoString(C.seb_last_error()))
	}
	reads = make([]BlockRead, len(uniqSlot))
	for r := range reads {
		reads[r] = BlockRead{Slot: uniqSlot[r], Offset: uniqBlock[r]}
	}
	return bid, reads, blockIDSizes(&sz), nil
}

// The device form: every pointer below is device memory the caller owns, `stream` its HIP stream.  resFirst and
// resCount hold resSlots u32 each (nil with resSlots 0: no file is resident).

// DevBlockIDsResident maps the cells of resident files and leaves NoBlockID in the others; counts (nil, or three
// u64: resident, misses, bad) tells the caller whether a miss path is needed at all.  Not synchronised.
func DevBlockIDsResident(cand, blocks unsafe.Pointer, cells uint64, resFirst, resCount unsafe.Pointer, resSlots uint32,
	bid, counts, stream unsafe.Pointer) error {
	if C.seb_dev_block_ids_resident((*C.uint16_t)(cand), (*C.uint64_t)(blocks), C.uint64_t(cells), (*C.uint32_t)(resFirst),
		(*C.uint32_t)(resCount), C.uint32_t(resSlots), (*C.uint32_t)(bid), (*C.uint64_t)(counts), stream) != 0 {
		return fmt.Errorf("failed to map block ids: %s", C.GoString(C.seb_last_error()))
	}
	return nil
}

// DevBlockIDsWorkspaceSize is the workspace a plan of `cells` cells with at most maxUniq distinct miss pairs needs
// (16-byte aligned device memory).
func DevBlockIDsWorkspaceSize(cells, maxUniq uint64) uint64 {
	return uint64(C.seb_dev_block_ids_workspace_size(C.uint64_t(cells), C.uint64_t(maxUniq)))
}

// ErrBlockIDsRange reports more than maxUniq distinct miss pairs: plan again with maxUniq = Sizes.Misses.
type ErrBlockIDsRange struct {
	Sizes BlockIDSizes
}

func (e *ErrBlockIDsRange) Error() string {
	return fmt.Sprintf("more than the %d distinct blocks the plan allowed for; %d cells miss", e.Sizes.Uniq-1, e.Sizes.Misses)
}

// DevBlockIDsPlan classifies the cells and numbers the distinct miss pairs; it synchronises the stream.  maxUniq:
// the number of blocks in the files that are not resident is a good bound, `cells` always suffices.
func DevBlockIDsPlan(cand, blocks unsafe.Pointer, cells uint64, resFirst, resCount unsafe.Pointer, resSlots uint32,
	maxUniq uint64, workspace unsafe.Pointer, workspaceBytes uint64, stream unsafe.Pointer) (BlockIDSizes, error) {
	var sz C.seb_blockids_sizes
	rc := C.seb_dev_block_ids_plan((*C.uint16_t)(cand), (*C.uint64_t)(blocks), C.uint64_t(cells), (*C.uint32_t)(resFirst),
		(*C.uint32_t)(resCount), C.uint32_t(resSlots), C.uint64_t(maxUniq), workspace, C.uint64_t(workspaceBytes), &sz, stream)
	if rc == C.SEB_ERR_RANGE {
		return blockIDSizes(&sz), &ErrBlockIDsRange{Sizes: blockIDSizes(&sz)}
	}
	if rc != 0 {
		return BlockIDSizes{}, fmt.Errorf("failed to plan the block ids: %s", C.GoString(C.seb_last_error()))
	}
	return blockIDSizes(&sz), nil
}

// DevBlockIDsEmit writes bid[0, Cells), uniqSlot[0, Uniq) (u16) and uniqBlock[0, Uniq) (u64); the same cells,
// residency table, maxUniq and workspace as the plan.  Not synchronised.
func DevBlockIDsEmit(cand, blocks unsafe.Pointer, cells uint64, resFirst, resCount unsafe.Pointer, resSlots uint32,
	maxUniq uint64, idBase uint32, sizes BlockIDSizes, workspace, bid, uniqSlot, uniqBlock, stream unsafe.Pointer) error {
	sz := C.seb_blockids_sizes{cells: C.uint64_t(sizes.Cells), resident: C.uint64_t(sizes.Resident),
		misses: C.uint64_t(sizes.Misses), uniq: C.uint64_t(sizes.Uniq), bad: C.uint64_t(sizes.Bad)}
	if C.seb_dev_block_ids_emit((*C.uint16_t)(cand), (*C.uint64_t)(blocks), C.uint64_t(cells), (*C.uint32_t)(resFirst),
		(*C.uint32_t)(resCount), C.uint32_t(resSlots), C.uint64_t(maxUniq), C.uint32_t(idBase), &sz, workspace,
		(*C.uint32_t)(bid), (*C.uint16_t)(uniqSlot), (*C.uint64_t)(uniqBlock), stream) != 0 {
		return fmt.Errorf("failed to emit the block ids: %s", C.GoString(C.seb_last_error()))
	}
	return nil
}
