// ewk_snapshot.h -- launch interface of the stream-snapshot kernels (ewk_snapshot.hip; internal).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ewk_gate.h"

namespace ewk {

// One launch packs the streams ids[0..n) into records, or unpacks records into them: record i,
// at rec + i * record_bytes, is stream ids[i].  The engine-side arrays are addressed by stream;
// those an engine does not have are nullptr (pack writes zeros for them, unpack skips them).
struct SnapArgs {
    const int32_t* ids;        // [n] streams
    const int32_t* pending;    // [n] carry samples per listed stream (pack; nullptr: 0)
    int32_t n;
    int32_t n_blocks;
    unsigned char* rec;        // [n][record_bytes], 16-byte aligned
    int64_t record_bytes;
    int64_t off[8];            // section offsets (ewk_snapshot_layout::section, EWK_SNAP_*)
    int64_t sec_bytes[8];      // ... and sizes
    unsigned char* ring;       // [n_streams][row_bytes]
    int64_t row_bytes;         // sring_len * sample size
    GateStream* st;
    double* block_rms;         // [n_streams][n_blocks]
    double* sorted_rms;        // [n_streams][2][n_blocks]
    LsnState* lsn_st;          // nullptr or [n_streams][kLsnStates]
    const int32_t* lsn_count;  // nullptr or [n_streams] (pack: rows past the count are zero)
    float* hist;               // nullptr or [n_streams][H]
    int32_t H;
    int32_t compact;           // sring_len < ring_len: block RMSs are kept from the first write
    uint8_t* fresh;            // nullptr or [n_streams]
    int32_t fresh_all;         // pack without flags: the engine-wide flag
    int32_t es;                // bytes per ring sample
    unsigned char* carry;      // nullptr or [n_streams][in_block] samples of the ring's type
    int32_t in_block;
    int32_t pad0;
};
hipError_t launch_snapshot_pack(const SnapArgs& a, hipStream_t s);
hipError_t launch_snapshot_unpack(const SnapArgs& a, hipStream_t s);

}  // namespace ewk
