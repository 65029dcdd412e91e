// mbx_keystream_words.h -- a keystream row (include/mbx_keystream.h: MBX_KEYSTREAM_ROW_BYTES bytes per frame, parameter bit i in bit
// 7 - (i & 7) of byte i >> 3) -> the three words that are XORed onto w[0..2] of the frame's parameter record, stated ONCE for the host
// function (mbx_keystream_apply_host, mbx_api.hip) and for the kernels that apply a row on the device (mbx_keystream.hip).
// Host-visible: nothing here needs a device compile (tests/keystream_check.cpp holds it to a bit-by-bit loop under a sanitizer).
//
// Parameter bit i of a record is bit 31 - (i % 32) of w[i / 32] (mbx_unpack_records), so word j is bytes 4j .. 4j + 3 of the row read
// big-endian: one byte swap of the dword as a little-endian machine loads it, then the bits at and beyond nbits masked off.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MBX_KEYSTREAM_FN __host__ __device__ inline
#else
#define MBX_KEYSTREAM_FN inline
#endif

namespace mbx {

constexpr int kKeystreamRowBytes = 12;   // MBX_KEYSTREAM_ROW_BYTES

struct KeystreamWords {
    uint32_t x, y, z;   // onto w[0], w[1], w[2]; w[3] (error counts and flags) has no keystream
};

// parameter bits of a record of `codec` (MBX_CODEC_*): imbe_d[88] for the IMBE codecs -- a 7100x4400 record leaves its front end in
// 7200x4400 order --, ambe_d[49] for the AMBE ones; 0: no such codec
MBX_KEYSTREAM_FN int keystream_nbits(int codec) {
    return (codec == 0 || codec == 2) ? 88 : ((codec == 1 || codec == 3) ? 49 : 0);
}

// which bits of word j (0..2) are parameter bits when the record holds nbits of them
MBX_KEYSTREAM_FN uint32_t keystream_word_mask(int nbits, int j) {
    const int kept = nbits - 32 * j;
    return kept <= 0 ? 0u : (kept >= 32 ? 0xffffffffu : 0xffffffffu << (32 - kept));
}

// d0, d1, d2: the row's three dwords as a little-endian load gives them (byte 0 of the row in the low byte of d0)
MBX_KEYSTREAM_FN KeystreamWords keystream_words(uint32_t d0, uint32_t d1, uint32_t d2, int nbits) {
    KeystreamWords k;
    k.x = __builtin_bswap32(d0) & keystream_word_mask(nbits, 0);
    k.y = __builtin_bswap32(d1) & keystream_word_mask(nbits, 1);
    k.z = __builtin_bswap32(d2) & keystream_word_mask(nbits, 2);
    return k;
}

// the same from the row's bytes, wherever they sit (the host function; the kernels load dwords from their 4-byte aligned rows)
MBX_KEYSTREAM_FN KeystreamWords keystream_words_of_row(const uint8_t* row, int nbits) {
    uint32_t d[3];
    for (int j = 0; j < 3; ++j) {
        d[j] = (uint32_t)row[4 * j] | ((uint32_t)row[4 * j + 1] << 8) | ((uint32_t)row[4 * j + 2] << 16) | ((uint32_t)row[4 * j + 3] << 24);
    }
    return keystream_words(d[0], d[1], d[2], nbits);
}

}  // namespace mbx
