// ewk_g711.h -- the G.711 decode (ITU-T G.711: PCMU mu-law, PCMA A-law), one definition for the
// host (ewk_g711_table) and the device (ewk_resample.hip, ewk_chunks.hip, ewk_level3.hip).  A host
// compiler builds it alone.  Branch-free integer arithmetic on the code byte, no table in memory:
// every code is a 16-bit integer v, and v / 32768 is exact in float32.
//   mu-law: u = ~b & 0xFF, t = (((u & 0xF) << 3) + 0x84) << ((u >> 4) & 7),
//           v = (u & 0x80) ? 0x84 - t : t - 0x84            (-32124 .. 32124; 0x7F and 0xFF are 0)
//   A-law:  a = b ^ 0x55, e = (a >> 4) & 7, m = a & 0xF,
//           t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1),
//           v = (a & 0x80) ? t : -t                         (-32256 .. 32256; smallest magnitude 8)
// Both equal CPython's audioop.ulaw2lin / alaw2lin at width 2 on all 256 codes.
#pragma once

#include <stdint.h>

#ifndef __HIPCC__
#define EWK_G711_HD inline
#else
#include <hip/hip_runtime.h>
#define EWK_G711_HD __host__ __device__ __forceinline__
#endif

namespace ewk {

constexpr int kG711Ulaw = 0, kG711Alaw = 1;   // EWK_G711_ULAW, EWK_G711_ALAW (include/ewk.h)

EWK_G711_HD int32_t g711_ulaw(uint32_t b) {
    const uint32_t u = ~b & 0xFFu;
    const int32_t t = (int32_t)((((u & 0xFu) << 3) + 0x84u) << ((u >> 4) & 7u));
    return (u & 0x80u) ? 0x84 - t : t - 0x84;
}

EWK_G711_HD int32_t g711_alaw(uint32_t b) {
    const uint32_t a = (b ^ 0x55u) & 0xFFu;
    const uint32_t e = (a >> 4) & 7u, m = a & 0xFu;
    // e == 0: (m << 4) + 8; else ((m << 4) + 0x108) << (e - 1)
    const int32_t t = (int32_t)(((m << 4) + (e ? 0x108u : 8u)) << (e ? e - 1u : 0u));
    return (a & 0x80u) ? t : -t;
}

// the 16-bit value of code b under `law` (kG711Ulaw or kG711Alaw)
EWK_G711_HD int32_t g711_decode(uint32_t b, int32_t law) { return law == kG711Alaw ? g711_alaw(b) : g711_ulaw(b); }

// ... and the float sample, by the expression every PCM16 decode of the engine uses
EWK_G711_HD float g711_sample(uint32_t b, int32_t law) { return (float)g711_decode(b, law) * (1.0f / 32768.0f); }

}  // namespace ewk
