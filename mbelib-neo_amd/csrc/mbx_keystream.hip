// mbx_keystream.hip -- keystream input (include/mbx_keystream.h): a caller's keystream row XORed onto the parameter bits of a frame
// between FEC and parameter decode, where the reference's callers apply it between mbe_decodeImbe7200x4400Frame /
// mbe_decodeAmbe3600x2450Frame and mbe_processImbe4400Dataf / mbe_processAmbe2450Dataf (ref src/imbe/imbe7200x4400.c:935-948,
// src/ambe/ambe3600x2450.c:684-714: the one-call forms are those two calls back to back).
//
// Three kernels, nothing of their own but the XOR: the stage alone on records that are there (keystream_apply_kernel), and the hard
// and the soft front of a KEYED batch step, which run the per-frame functions of mbx_fec_frame.h / the searches of mbx_fec_soft.h
// exactly as the unkeyed fronts do and XOR the row's words (mbx_keystream_words.h) onto x, y, z of the record before its one store.
// w (error counts and flags: the reference's *result context) has no keystream.  A row is 12 bytes, 4-byte aligned: three dword
// loads per frame, one byte swap per word.  The expand launch and the stream stage behind a keyed front are the unkeyed step's.
#include "mbx_device.h"
#include "mbx_fec_soft.h"
#include "mbx_kernels.h"
#include "mbx_keystream_words.h"

namespace mbx {

// the words of row i (rows of kKeystreamRowBytes, 4-byte aligned) for a record of nbits parameter bits
__device__ __forceinline__ KeystreamWords keystream_row(const uint8_t* __restrict__ keystream, size_t i, int nbits) {
    const uint32_t* const d = reinterpret_cast<const uint32_t*>(keystream + i * (size_t)kKeystreamRowBytes);
    return keystream_words(d[0], d[1], d[2], nbits);
}

// records in place, one thread per record: w[0..2] ^= the row's words; w[3] is neither read nor written
__global__ void __launch_bounds__(256)
keystream_apply_kernel(int nbits, mbx_param_record* __restrict__ records, size_t n, const uint8_t* __restrict__ keystream) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    const KeystreamWords k = keystream_row(keystream, i, nbits);
    uint32_t* const w = records[i].w;
    const uint32_t x = w[0] ^ k.x, y = w[1] ^ k.y, z = w[2] ^ k.z;
    w[0] = x;
    w[1] = y;
    w[2] = z;
}

// The hard front of a keyed step, one thread per frame: frames `stride` bytes apart (a codec's own frame size, or the 18-byte rows of
// a mixed step), the codec uniform (`codec`) or per row (row_codec, non-NULL in a mixed step: mixed_row_codec_kernel).  Each frame
// takes the front end CodecShape::front names for its codec, as in fec_mixed_kernel.  A byte that names no codec: no record is
// written and the keystream row is not read.
__global__ void __launch_bounds__(256)
fec_keyed_kernel(const uint8_t* __restrict__ frames, size_t n, int stride, int codec, const uint8_t* __restrict__ row_codec,
                 const uint8_t* __restrict__ keystream, mbx_param_record* __restrict__ out, DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    const int c = row_codec ? (int)row_codec[i] : codec;
    const uint8_t* const f = frames + i * (size_t)stride;
    uint4 rec;
    switch (c) {
    case MBX_CODEC_IMBE7200X4400:
        rec = fec_imbe7200x4400_frame(tabs.t, f);
        break;
    case MBX_CODEC_IMBE7100X4400:
        rec = fec_imbe7100x4400_frame(tabs.t, f);
        break;
    case MBX_CODEC_AMBE3600X2450:
    case MBX_CODEC_AMBE3600X2400:
        rec = fec_ambe3600x2450_frame(tabs.t, f);
        break;
    default:
        return;
    }
    const KeystreamWords k = keystream_row(keystream, i, keystream_nbits(c));
    rec.x ^= k.x;
    rec.y ^= k.y;
    rec.z ^= k.z;
    *reinterpret_cast<uint4*>(&out[i]) = rec;
}

// The soft front of a keyed step, one wave per frame: frames `cells` cells apart (a codec's own cell array, or the 184-cell rows of
// a mixed step), the codec wave-uniform as in soft_front_mixed_kernel -- a scalar branch into the searches of the three soft fronts,
// on one SoftScratch.  Lane 0 XORs and stores.  A byte that names no codec: no record is written, the keystream row is not read.
__global__ void __launch_bounds__(64, 8)
soft_front_keyed_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, int cells, int codec, const uint8_t* __restrict__ row_codec,
                        const uint8_t* __restrict__ keystream, mbx_param_record* __restrict__ records, DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const mbe_soft_bit* const row = soft + i * (size_t)cells;
    const int c = row_codec ? __builtin_amdgcn_readfirstlane((int)row_codec[i]) : codec;   // (one row per wave: uniform)
    uint4 rec;
    switch (c) {
    case MBX_CODEC_IMBE7200X4400:
        rec = soft_record_imbe7200x4400(S, row, tabs, lane);
        break;
    case MBX_CODEC_IMBE7100X4400:
        rec = soft_record_imbe7100x4400(S, row, tabs, lane);
        break;
    case MBX_CODEC_AMBE3600X2450:
    case MBX_CODEC_AMBE3600X2400:
        rec = soft_record_ambe3600(S, row, tabs, lane);
        break;
    default:
        return;
    }
    if (lane == 0) {
        const KeystreamWords k = keystream_row(keystream, i, keystream_nbits(c));
        rec.x ^= k.x;
        rec.y ^= k.y;
        rec.z ^= k.z;
        *reinterpret_cast<uint4*>(&records[i]) = rec;
    }
}

}  // namespace mbx
