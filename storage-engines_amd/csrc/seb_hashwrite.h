// seb_hashwrite.h — the host-only code of seb_hashwrite.cpp (no HIP dependency): the host half of the hash index's
// write side: a Put / Delete batch framed as segment.append's records with the rotation's cuts,
// compactSegments for a prefix of the segments, and getLogicalSize.
#pragma once
#include <cstdint>

#include "seb_hashindex.h"

namespace seb {

struct SegCompactSizes {  // seb_segcompact_sizes
    uint64_t records_in, live_in;   // the records given, and those with live[r] != 0
    uint64_t distinct, survivors;   // keys among the live records; records written
    uint64_t tombstoned, shadowed;  // keys whose winning record has no value; live records that lost to a later one
    uint64_t image_bytes, reserved;
};

// rec_off[0..n] (nullable), cut[0..*ncuts) (nullable: the cuts are only counted), *image_bytes and *ncuts (nullable)
// for a batch appended behind active_size bytes of the active segment with rotation at `limit`.  0; -1 a null
// argument; -2 / -3 op *bad_op's key / value offsets decrease or span 2^32 bytes or more; -4 2^32 ops or more; -6
// op *bad_op's key is empty; -7 its keySize + valueSize is 2^32 or more; -8 cut_cap is below *ncuts (which is set);
// -9 limit is 0.  No byte of keys, vals or deleted is read before every op's offsets passed (deleted is read for
// the value's size).
int seg_frame_plan(const KeysView &keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                   uint64_t limit, uint64_t *rec_off, uint64_t *cut, uint64_t cut_cap, uint64_t *image_bytes,
                   uint64_t *ncuts, uint64_t *bad_op);
// The sealed image into image[0, image_bytes): every record carries `timestamp`.  seg_frame_plan's codes; -5
// image_bytes is not the plan's.
int seg_frame_emit(const KeysView &keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                   uint64_t timestamp, uint8_t *image, uint64_t image_bytes, uint64_t *bad_op);

// compactSegments over the live records (live nullable: all) of the chosen segments, rec_off in scan order: per key
// the record at the greatest offset wins, a winner with valueSize > 0 survives, the survivors go to image in record
// order with `timestamp` and a fresh CRC, out_rec_off[0..survivors] = their offsets in the image.  image and
// out_rec_off null: the sizes only.  0; -1 a null argument; -2 pool_bytes >= 2^47; -3 out of memory; -4 live record
// *bad lies outside the pool or breaks the 2^32 rule; -5 image_cap or rec_cap is below a size (*sizes is set).
int seg_compact(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live, uint64_t n,
                uint64_t timestamp, uint8_t *image, uint64_t image_cap, uint64_t *out_rec_off, uint64_t rec_cap,
                SegCompactSizes *sizes, uint64_t *bad);

// getLogicalSize: the sum over the index (tombstoned keys included) of keySize + valueSize of the winning record.
// 0; -1; -2; -3 as above; a record outside the pool takes no part (hidx_lookup's rule).
int hidx_logical_size(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live, uint64_t n,
                      uint64_t *logical);

}  // namespace seb
