// mbx_compand.h -- one linear PCM sample (int16) -> its G.711 byte, mu-law or A-law, stated ONCE for the host loop
// (mbx_pcm_compand_host, mbx_pcm8.hip) and for the kernel that compands on the device (pcm_compand_kernel, mbx_pcm8.hip).
// Host-visible: nothing here needs a device compile.  No table and no search through the segment end points: the segment of a
// magnitude is the place of its leading one, one find-first-bit instruction on the device.
// The bytes are those of the classic linear2ulaw on the 14-bit value and linear2alaw on the 13-bit value (ITU-T G.711; CPython's
// audioop.lin2ulaw / lin2alaw give the same 65,536 bytes each).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MBX_COMPAND_FN __host__ __device__ inline
#else
#define MBX_COMPAND_FN inline
#endif

namespace mbx {

constexpr int kLawUlaw = 0, kLawAlaw = 1;   // MBX_LAW_ULAW, MBX_LAW_ALAW (include/mbx_pcm8.h)

MBX_COMPAND_FN int compand_log2(uint32_t m) { return 31 - __builtin_clz(m); }   // floor(log2 m), m > 0

// mu-law: the 14-bit magnitude clipped at 8159 and biased by 33 lies in 33..8192; segment 0..7 and four mantissa bits below the
// leading one, the one value 8192 (segment "8") is the top code.  The byte is the code inverted, sign in bit 7.
MBX_COMPAND_FN uint8_t pcm16_to_ulaw(int16_t x) {
    const int v = x >> 2;
    const bool neg = v < 0;
    const int a = neg ? -v : v;
    const uint32_t m = (uint32_t)(a > 8159 ? 8159 : a) + 33u;
    const int seg = compand_log2(m) - 5;
    const uint32_t code = seg == 8 ? 0x7Fu : ((uint32_t)seg << 4) | ((m >> (seg + 1)) & 15u);
    return (uint8_t)(code ^ (neg ? 0x7Fu : 0xFFu));
}

// A-law: the 13-bit value, a negative one as its one's complement, 0..4095; magnitudes below 32 share segment 0 and the shift of
// segment 1 (m | 16 has its leading one at bit 4 there, and where m has it elsewhere).  The byte is the code with the even bits
// inverted, sign in bit 7.
MBX_COMPAND_FN uint8_t pcm16_to_alaw(int16_t x) {
    const int v = x >> 3;
    const bool neg = v < 0;
    const uint32_t m = (uint32_t)(neg ? -v - 1 : v);
    const int seg = compand_log2(m | 16u) - 4;
    const uint32_t code = ((uint32_t)seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15u);
    return (uint8_t)(code ^ (neg ? 0x55u : 0xD5u));
}

MBX_COMPAND_FN uint8_t pcm16_compand(int law, int16_t x) { return law == kLawAlaw ? pcm16_to_alaw(x) : pcm16_to_ulaw(x); }

}  // namespace mbx
