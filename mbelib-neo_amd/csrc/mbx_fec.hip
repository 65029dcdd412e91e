// mbx_fec.hip -- FEC stage: wire frames -> parameter records.  One thread per frame; frames
// are independent here (no stream state), so the grid is simply ceil(n / 256) workgroups.
//
// Replaces (ref = arancormonk/mbelib-neo v2.0.0):
//   IMBE  src/imbe/imbe7200x4400.c:424-443 (C0 Golay), :636-673 (PR demodulation),
//         :469-515 (3x Golay + 3x Hamming + raw row), :709-744 (frame decode + status)
//   AMBE  src/ambe/ambe_common.c:22-46 (C0 Golay + overall parity), :75-100 (demodulation),
//         :127-157 (Golay on C1, raw C2/C3); src/ambe/ambe3600x2450.c:649-682
//   ECC   src/ecc/ecc.c:221-301 (Golay(23,12) by syndrome table), :366-408 (Hamming(15,11))
// Further down: the IMBE 7100x4400 front end (its own C0 / seed / Hamming mapping / bit order) and the soft-decision
// front end (one wavefront per frame, exhaustive maximum-likelihood decode of every block).
// Integer work only: results are bit-exact.
#include "mbx_device.h"
#include "mbx_fec_frame.h"
#include "mbx_fec_soft.h"
#include "mbx_kernels.h"
#include "mbx_llr_cell.h"

namespace mbx {

__global__ void __launch_bounds__(256)
fec_imbe7200x4400_kernel(const uint8_t* __restrict__ frames, size_t n, mbx_param_record* __restrict__ out,
                         DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    *reinterpret_cast<uint4*>(&out[i]) = fec_imbe7200x4400_frame(tabs.t, frames + i * MBX_IMBE_FRAME_BYTES);
}

__global__ void __launch_bounds__(256)
fec_ambe3600x2450_kernel(const uint8_t* __restrict__ frames, size_t n, mbx_param_record* __restrict__ out,
                         DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    *reinterpret_cast<uint4*>(&out[i]) = fec_ambe3600x2450_frame(tabs.t, frames + i * MBX_AMBE_FRAME_BYTES);   // 9-byte frames: byte loads
}

// ------------------------------------------------------------------------------------------
// IMBE 7100x4400 front end: rows of 19, 24, 23, 23, 15, 15, 23 cells.
//   ref src/imbe/imbe7100x4400.c:100-122 (C0: Golay shortened to 18 cells), :292-334 (demodulation, 7-bit
//       seed), :153-212 (Golay on C1..C3, Hamming with the 7100 bit mapping on C4/C5, raw C6),
//       :381-438 (mbe_convertImbe7100to7200: a permutation of the 88 bits that depends on K(b0)),
//       :440-479 (frame decode); src/ecc/ecc.c:422-464 (mbe_7100x4400hamming1511)
// The record holds the 88 bits AFTER the conversion, i.e. in 7200x4400 order: the stream stage is the
// 7200x4400 one.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
fec_imbe7100x4400_kernel(const uint8_t* __restrict__ frames, size_t n, mbx_param_record* __restrict__ out,
                         DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    *reinterpret_cast<uint4*>(&out[i]) = fec_imbe7100x4400_frame(tabs.t, frames + i * MBX_IMBE7100_FRAME_BYTES);
}

// The front of a MIXED hard-decision step (mbx_process_batch_mixed): rows of MBX_IMBE_FRAME_BYTES whatever the codec (an AMBE frame
// in the first nine bytes), the codec of row i in row_codec[i] (mixed_row_codec_kernel).  Each row takes the front end
// CodecShape::front names for its codec -- the per-frame functions of the three kernels above, nothing of its own -- so a
// 7100x4400 row leaves as a 7200x4400 record and a D-STAR row takes the 3600x2450 front.  Rows of one stream are neighbours:
// lanes diverge only where a wave straddles a stream boundary.  A byte that names no codec: no record is written.
__global__ void __launch_bounds__(256)
fec_mixed_kernel(const uint8_t* __restrict__ frames, size_t n, const uint8_t* __restrict__ row_codec, mbx_param_record* __restrict__ out,
                 DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint8_t* const f = frames + i * MBX_IMBE_FRAME_BYTES;
    switch (row_codec[i]) {
    case MBX_CODEC_IMBE7200X4400:
        *reinterpret_cast<uint4*>(&out[i]) = fec_imbe7200x4400_frame(tabs.t, f);
        break;
    case MBX_CODEC_IMBE7100X4400:
        *reinterpret_cast<uint4*>(&out[i]) = fec_imbe7100x4400_frame(tabs.t, f);
        break;
    case MBX_CODEC_AMBE3600X2450:
    case MBX_CODEC_AMBE3600X2400:
        *reinterpret_cast<uint4*>(&out[i]) = fec_ambe3600x2450_frame(tabs.t, f);
        break;
    default:
        break;
    }
}

// float -> int16 (a21): ref src/core/mbelib.c:1148-1177.  One thread per sample.
__device__ __forceinline__ int16_t float_to_pcm16(float x) {
    const float top = 32767.0f * 0.95f;
    const uint32_t bits = __float_as_uint(x);
    const uint32_t mag = bits & 0x7FFFFFFFu;
    float v;
    if (mag > 0x7F800000u) {
        v = 0.0f;
    } else if (mag == 0x7F800000u) {
        v = (bits & 0x80000000u) ? -top : top;
    } else {
        v = 7.0f * x;
        v = (v > top) ? top : ((v < -top) ? -top : v);
    }
    return (int16_t)(int)v;   // C cast: truncate toward zero
}

// Host -> device staging of a batch's wire frames by the GPU itself: `src` is PINNED host memory, read over PCIe in 16-byte
// pieces (every line once), `dst` device memory.  Used by the sessions instead of a DMA copy: a host-to-device DMA of batch
// k + 1 queues behind the device-to-host DMA of batch k's PCM on the copy engine, which serialises the next batch's kernels
// behind that transfer (measured: 0.257 ms of kernels + 0.379 ms of PCM per 65,536 frames back to back instead of
// overlapped); 1.2 MB read by a kernel on the compute stream costs 40 us and leaves the engine to the PCM.
__global__ void __launch_bounds__(256)
stage_in_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t bytes) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n16 = bytes >> 4;
    if (i < n16) {
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else if (i == n16) {
        for (size_t b = n16 << 4; b < bytes; ++b) {
            dst[b] = src[b];
        }
    }
}

// LLRs -> soft cells (mbx_soft_from_llr; the conversion: mbx_llr_cell.h).  A workgroup takes chunks of kLlrChunk LLRs, grid-stride: the
// chunk goes to LDS as it comes, with dword loads from the first aligned dword on and single pieces at the edges (an aligned dword
// of the source is an aligned dword of LDS), then a lane owns the two cells of one aligned output dword, reads their LLRs from LDS
// and stores the pair -- a single cell where the dword is not wholly inside the chunk.  A chunk is a whole number of dwords on
// both sides, so every chunk has the alignment phases of the first.
template <int kLlrBytes>
__global__ void __launch_bounds__(256)
soft_from_llr_kernel(const uint8_t* __restrict__ llr, size_t count, mbe_soft_bit* __restrict__ soft) {
    static_assert(kLlrBytes == 1 || kLlrBytes == 2, "int8 or int16");
    __shared__ uint32_t stage[kLlrChunk * kLlrBytes / 4 + 1];   // (+ one dword for the phase)
    uint8_t* in8 = reinterpret_cast<uint8_t*>(stage);
    const int tid = (int)threadIdx.x;
    const int head = (int)(reinterpret_cast<uintptr_t>(llr) & 3u);   // byte i of a chunk sits at in8[head + i]
    const int lead = (4 - head) & 3;                                 // bytes in front of the first aligned dword
    uint16_t* out = reinterpret_cast<uint16_t*>(soft);
    const int a = (int)((reinterpret_cast<uintptr_t>(out) >> 1) & 1u);
    for (size_t first = (size_t)blockIdx.x * kLlrChunk; first < count; first += (size_t)gridDim.x * kLlrChunk) {
        const int here = (int)(count - first < (size_t)kLlrChunk ? count - first : (size_t)kLlrChunk);
        const int nbytes = here * kLlrBytes;
        const uint8_t* src = llr + first * kLlrBytes;
        const int edge = lead < nbytes ? lead : nbytes;
        const int ndw = (nbytes - edge) >> 2;
        const int tail = edge + 4 * ndw;   // the bytes behind the last whole dword: fewer than four
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + edge);   // (aligned wherever ndw > 0: then edge == lead)
        uint32_t* d32 = reinterpret_cast<uint32_t*>(in8 + head + edge);
        for (int m = tid; m < ndw; m += 256) {
            d32[m] = s32[m];
        }
        // the edges in pieces of one LLR (an int16 array is 2-aligned: its edges are whole LLRs)
        if (tid * kLlrBytes < edge) {
            if constexpr (kLlrBytes == 2) {
                *reinterpret_cast<uint16_t*>(in8 + head + 2 * tid) = *reinterpret_cast<const uint16_t*>(src + 2 * tid);
            } else {
                in8[head + tid] = src[tid];
            }
        } else if (tid >= 4 && (tid - 4) * kLlrBytes < nbytes - tail) {
            const int at = tail + (tid - 4) * kLlrBytes;
            if constexpr (kLlrBytes == 2) {
                *reinterpret_cast<uint16_t*>(in8 + head + at) = *reinterpret_cast<const uint16_t*>(src + at);
            } else {
                in8[head + at] = src[at];
            }
        }
        __syncthreads();
        const auto cell = [&](int i) -> uint32_t {
            if constexpr (kLlrBytes == 2) {
                return soft_cell_from_llr(*reinterpret_cast<const int16_t*>(in8 + head + 2 * i));
            } else {
                return soft_cell_from_llr(*reinterpret_cast<const int8_t*>(in8 + head + i));
            }
        };
        uint16_t* o = out + first;
        const int pairs = (here + 1 + a) >> 1;
        for (int p = tid; p < pairs; p += 256) {
            const int c0 = 2 * p - a, c1 = c0 + 1;
            if (c0 >= 0 && c1 < here) {
                *reinterpret_cast<uint32_t*>(o + c0) = cell(c0) | (cell(c1) << 16);
            } else if (c0 >= 0) {
                o[c0] = (uint16_t)cell(c0);
            } else if (c1 < here) {
                o[c1] = (uint16_t)cell(c1);
            }
        }
        __syncthreads();   // the next chunk overwrites the stage
    }
}
template __global__ void soft_from_llr_kernel<1>(const uint8_t*, size_t, mbe_soft_bit*);
template __global__ void soft_from_llr_kernel<2>(const uint8_t*, size_t, mbe_soft_bit*);

__global__ void __launch_bounds__(256)
floattoshort_kernel(const float* __restrict__ in, int16_t* __restrict__ out, size_t nsamples) {
    // two samples per thread so every lane stores a full dword
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i + 1 < nsamples) {
        const float2 v = *reinterpret_cast<const float2*>(in + i);
        const uint32_t lo = (uint16_t)float_to_pcm16(v.x), hi = (uint16_t)float_to_pcm16(v.y);
        *reinterpret_cast<uint32_t*>(out + i) = lo | (hi << 16);
    } else if (i < nsamples) {
        out[i] = float_to_pcm16(in[i]);
    }
}


// What a host tallies from the mbe_process_result of every frame (ref include/mbelib-neo/mbelib.h:154-166: the flag bits and
// the three error counts), for a whole batch on the device: 20 bytes read per frame, one set of atomics per workgroup.
// Integer sums only: the histogram of a batch does not depend on the launch geometry.
__global__ void __launch_bounds__(256)
result_histogram_kernel(const mbe_process_result* __restrict__ results, size_t n, unsigned long long* __restrict__ hist) {
    unsigned v[kResultHistWords];
#pragma unroll
    for (int k = 0; k < kResultHistWords; ++k) {
        v[k] = 0u;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const mbe_process_result r = results[i];
        v[0] += 1u;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            v[1 + b] += (r.flags >> b) & 1u;
        }
        v[9] += (unsigned)r.c0_errors;
        v[10] += (unsigned)r.protected_errors;
        v[11] += (unsigned)r.c4_errors;
        v[12] += (unsigned)r.total_errors;
        v[13] += r.total_errors > 0 ? 1u : 0u;
    }
    __shared__ unsigned part[4][kResultHistWords];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < kResultHistWords; ++k) {   // (a thread holds at most n / (grid x 256) + 1 frames: the 32-bit partial sums cannot wrap
        unsigned s = v[k];                          //  for the grid mbx_result_histogram launches)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s += (unsigned)__shfl_xor((int)s, d, 64);
        }
        if (lane == 0) {
            part[wave][k] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < kResultHistWords) {
        const unsigned long long s = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (s != 0ULL) {
            atomicAdd(&hist[threadIdx.x], s);
        }
    }
}


// ------------------------------------------------------------------------------------------
// The sub-stages of the frame decode as the reference exposes them one by one (in-place helpers of the classic
// ecc -> demodulate -> ecc call sequence), batched: one thread per frame, packed frames in, packed frames out.
//   stage 1  C0 ECC        mbe_eccImbe7200x4400C0 src/imbe/imbe7200x4400.c:424-443, mbe_eccAmbe3600C0_common
//                          src/ambe/ambe_common.c:22-46, mbe_eccImbe7100x4400C0 src/imbe/imbe7100x4400.c:100-122
//   stage 2  demodulation  mbe_demodulateImbe7200x4400Data :636-673, mbe_demodulateAmbe3600Data_common :75-100,
//                          mbe_demodulateImbe7100x4400Data :292-334  (seed = the C0 data bits AS THEY ARE in the frame)
//   stage 4  data ECC      mbe_eccImbe7200x4400Data :469-515,563-578, mbe_eccAmbe3600Data_common :127-157,
//                          mbe_eccImbe7100x4400Data :153-212 (bits in 7100 order: no conversion here)
//   stage 8  mbe_convertImbe7100to7200 src/imbe/imbe7100x4400.c:381-438 on a record (frames = records in, out = records)
// out record: parameter bits of stage 4 / 8; w[3] = corrected-error count of the stage (bits 0..7), C4 errors (16..23).
// These are slices of the frame kernels above, kept apart from them so that the hot kernels stay as they are.
// ------------------------------------------------------------------------------------------
struct BitWriter160 {
    uint32_t w[5] = {0, 0, 0, 0, 0};
    int      n = 0;
    __device__ void push(uint32_t value, int width) {   // `width` bits, first = MSB of the field
        for (int j = width - 1; j >= 0; --j, ++n) {
            w[n >> 5] |= ((value >> j) & 1u) << (31 - (n & 31));
        }
    }
    __device__ void store(uint8_t* p, int nbytes) const {
        for (int b = 0; b < nbytes; ++b) {
            p[b] = (uint8_t)(w[b >> 2] >> (24 - 8 * (b & 3)));
        }
    }
};

__device__ void convert_7100_to_7200(const mbx_tables* T, const Bits88& d, Bits88& t) {
    const int b0 = (int)(((d.hi >> 56) & 0x7eull) << 1) | (d.get(86) << 1) | d.get(87);   // bits 1..6, 86, 87
    const int K = (b0 < 208) ? (int)T->imbe_K[b0] : 12;
    t.put(87, d.get(0));
    t.put(48 + K, d.get(42));
    t.put(49 + K, d.get(43));
    for (int q = 0; q < K; ++q) {
        t.put(48 + q, d.get(44 + q));
    }
    int j = 0, k = 1;
    while (j < 87) {
        t.put(j, d.get(k));
        if (++j == 48) {
            j += K + 2;
        }
        if (++k == 42) {
            k += K + 2;
        }
    }
}

__global__ void __launch_bounds__(256)
fec_stage_kernel(int codec, int stage, const uint8_t* __restrict__ frames, size_t n, uint8_t* __restrict__ frames_out,
                 mbx_param_record* __restrict__ out, DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    const mbx_tables* T = tabs.t;
    if (stage == 8) {   // records in, records out
        const uint4 r = reinterpret_cast<const uint4*>(frames)[i];
        Bits88 d, t;
        d.hi = ((uint64_t)r.x << 32) | r.y;
        d.lo = (uint64_t)r.z << 32;
        convert_7100_to_7200(T, d, t);
        reinterpret_cast<uint4*>(out)[i] = make_uint4((uint32_t)(t.hi >> 32), (uint32_t)t.hi, (uint32_t)(t.lo >> 32), 0u);
        return;
    }
    const bool ambe = codec == MBX_CODEC_AMBE3600X2450 || codec == MBX_CODEC_AMBE3600X2400;
    const int fbytes = ambe ? MBX_AMBE_FRAME_BYTES : MBX_IMBE_FRAME_BYTES;
    const uint8_t* f = frames + i * (size_t)fbytes;
    BitReader br;
    for (int k = 0; k < 5; ++k) {
        br.w[k] = 0;
    }
    for (int b = 0; b < fbytes; ++b) {
        br.w[b >> 2] |= (uint32_t)f[b] << (24 - 8 * (b & 3));
    }
    int errs = 0, c4 = 0;
    RecordWriter rw;
    BitWriter160 bw;
    uint32_t w;
    if (codec == MBX_CODEC_IMBE7200X4400) {
        const int width[8] = {23, 23, 23, 23, 15, 15, 15, 7};
        uint32_t row[8];
        for (int r = 0, pos = 0; r < 8; pos += width[r], ++r) {
            row[r] = br.take(pos, width[r]);
        }
        if (stage == 1) {
            errs = golay2312(T, row[0], row[0]);
        } else if (stage == 2) {
            PrSequence pr(row[0] >> 11);
            for (int r = 1; r < 7; ++r) {
                row[r] ^= pr.mask_for(width[r]);
            }
        } else {
            rw.push(row[0], 23, 12);
            for (int r = 1; r < 4; ++r) {
                errs += golay2312(T, row[r], w);
                rw.push(w, 23, 12);
            }
            for (int r = 4; r < 7; ++r) {
                const int e = hamming1511(T, row[r], w);
                errs += e;
                c4 = (r == 4) ? e : c4;
                rw.push(w, 15, 11);
            }
            rw.push(row[7], 7, 7);
        }
        for (int r = 0; r < 8; ++r) {
            bw.push(row[r], width[r]);
        }
    } else if (codec == MBX_CODEC_IMBE7100X4400) {
        const int width[7] = {19, 24, 23, 23, 15, 15, 23};
        uint32_t row[7];
        for (int r = 0, pos = 0; r < 7; pos += width[r], ++r) {
            row[r] = br.take(pos, width[r]);
        }
        if (stage == 1) {   // cells 1..18 are the code word's low 18 positions, the five missing ones are zeros
            errs = golay2312(T, (row[0] >> 1) & 0x3ffffu, w);
            row[0] = ((w & 0x3ffffu) << 1) | (row[0] & 1u);
        } else if (stage == 2) {
            PrSequence pr((row[0] >> 12) & 0x7fu);
            for (int r = 1; r < 6; ++r) {
                row[r] ^= pr.mask_for(width[r]);
            }
        } else {
            rw.push(row[0] >> 12, 7, 7);
            errs += golay2312(T, row[1] >> 1, w);
            rw.push(w, 23, 12);
            errs += golay2312(T, row[2], w);
            rw.push(w, 23, 12);
            errs += golay2312(T, row[3], w);
            rw.push(w, 23, 12);
            c4 = hamming1511_7100(T, row[4], w);
            errs += c4;
            rw.push(w, 15, 11);
            errs += hamming1511_7100(T, row[5], w);
            rw.push(w, 15, 11);
            rw.push(row[6], 23, 23);
        }
        for (int r = 0; r < 7; ++r) {
            bw.push(row[r], width[r]);
        }
    } else {
        uint32_t row0 = br.take(0, 24), row1 = br.take(24, 23), row2 = br.take(47, 11), row3 = br.take(58, 14);
        if (stage == 1) {
            errs = golay2312(T, row0 >> 1, w);
            row0 = (w << 1) | (row0 & 1u);
            if (errs == 0 && (__popc(row0) & 1)) {
                row0 ^= 1u;
                errs = 1;
            }
        } else if (stage == 2) {
            PrSequence pr((row0 >> 12) & 0xfffu);
            row1 ^= pr.mask_for(23);
        } else {
            rw.push(row0, 24, 12);
            errs = golay2312(T, row1, w);
            rw.push(w, 23, 12);
            rw.push(row2, 11, 11);
            rw.push(row3, 14, 14);
        }
        bw.push(row0, 24);
        bw.push(row1, 23);
        bw.push(row2, 11);
        bw.push(row3, 14);
    }
    if (frames_out) {
        bw.store(frames_out + i * (size_t)fbytes, fbytes);
    }
    if (out) {
        reinterpret_cast<uint4*>(out)[i] = make_uint4((uint32_t)(rw.hi >> 32), (uint32_t)rw.hi, (uint32_t)(rw.lo >> 32),
                                                      (uint32_t)errs | ((uint32_t)c4 << 16));
    }
}

// ------------------------------------------------------------------------------------------
// Cell arrays -> wire frames on the device: hosts that hold their bursts as the reference's
// char arrays (imbe_fr[8][23] / ambe_fr[4][24] / imbe_fr[7][24], one char per bit) can upload them as they are; this
// kernel validates every cell like the reference does (mbe_validate_bits, src/internal/mbe_result.h:18-29: the WHOLE
// array, unused cells included) and packs the rows in wire order (row r, cells width[r]-1 .. 0).
// One workgroup of 256 threads takes 32 frames: the cells are staged through LDS with coalesced 4-byte loads, then one
// thread per output byte gathers its eight cells.  status[i] = 0 or MBE_STATUS_INVALID_BITS (the frame is then packed
// from the low bit of each cell and must be ignored by the caller, like the reference's "nothing is written").
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
pack_cells_kernel(int codec, const char* __restrict__ cells, size_t n, uint8_t* __restrict__ packed, int32_t* __restrict__ status) {
    constexpr int kFrames = 32;
    __shared__ uint32_t stage[kFrames * 184 / 4];
    __shared__ int bad[kFrames];
    const bool ambe = codec == MBX_CODEC_AMBE3600X2450 || codec == MBX_CODEC_AMBE3600X2400;
    const int ncell = codec == MBX_CODEC_IMBE7200X4400 ? 184 : (ambe ? 96 : 168);
    const int stride = codec == MBX_CODEC_IMBE7200X4400 ? 23 : 24;
    const int fbytes = ambe ? MBX_AMBE_FRAME_BYTES : MBX_IMBE_FRAME_BYTES;
    const int rows = codec == MBX_CODEC_IMBE7200X4400 ? 8 : (ambe ? 4 : 7);
    const int w0[8] = {23, 23, 23, 23, 15, 15, 15, 7}, w1[8] = {24, 23, 11, 14, 0, 0, 0, 0}, w2[8] = {19, 24, 23, 23, 15, 15, 23, 0};
    const size_t first = (size_t)blockIdx.x * kFrames;
    const int here = (int)((n - first) < (size_t)kFrames ? (n - first) : (size_t)kFrames);
    if (threadIdx.x < kFrames) {
        bad[threadIdx.x] = 0;
    }
    __syncthreads();
    const int words = here * ncell / 4;   // ncell is a multiple of 4 for all three shapes
    const uint32_t* src = reinterpret_cast<const uint32_t*>(cells + first * (size_t)ncell);
    for (int i = (int)threadIdx.x; i < words; i += 256) {
        const uint32_t v = src[i];
        stage[i] = v;
        if (v & 0xfefefefeu) {   // a cell outside {0, 1}
            bad[(i * 4) / ncell] = 1;   // the four cells of a word may straddle two frames: mark both
            bad[(i * 4 + 3) / ncell] = 1;
        }
    }
    __syncthreads();
    const char* c = reinterpret_cast<const char*>(stage);
    for (int o = (int)threadIdx.x; o < here * fbytes; o += 256) {
        const int f = o / fbytes, b = o % fbytes;
        uint32_t byte = 0;
        for (int k = 0; k < 8; ++k) {
            int pos = 8 * b + k, r = 0;   // wire position -> (row, cell)
            for (; r < rows; ++r) {
                const int w = codec == MBX_CODEC_IMBE7200X4400 ? w0[r] : (ambe ? w1[r] : w2[r]);
                if (pos < w) {
                    byte |= (uint32_t)(c[f * ncell + r * stride + (w - 1 - pos)] & 1) << (7 - k);
                    break;
                }
                pos -= w;
            }
        }
        packed[(first + (size_t)f) * (size_t)fbytes + (size_t)b] = (uint8_t)byte;
    }
    if ((int)threadIdx.x < here && status) {
        status[first + threadIdx.x] = bad[threadIdx.x] ? MBE_STATUS_INVALID_BITS : 0;
    }
}

// Code-word level ECC (the public per-word helpers, batched): kind 0 = Golay(23,12), 1 = Hamming(15,11),
// 2 = Hamming(15,11) with the IMBE 7100x4400 bit mapping (mbe_7100x4400hamming1511, src/ecc/ecc.c:422-464).
//   ref mbe_golay2312 / mbe_checkGolayBlock src/ecc/ecc.c:221-301, mbe_hamming1511 src/ecc/ecc.c:366-408
__global__ void __launch_bounds__(256)
ecc_words_kernel(int kind, const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out, int32_t* __restrict__ errs,
                 DeviceTables tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    uint32_t fixed;
    const int e = (kind == 0)   ? golay2312(tabs.t, in[i] & 0x7fffffu, fixed)
                  : (kind == 1) ? hamming1511(tabs.t, in[i] & 0x7fffu, fixed)
                                : hamming1511_7100(tabs.t, in[i] & 0x7fffu, fixed);
    out[i] = fixed;
    if (errs) {
        errs[i] = e;
    }
}


// ------------------------------------------------------------------------------------------
// Soft-decision front end, FEC only (mbx_fec_soft): one wavefront per frame, the search and the three
// frame forms in mbx_fec_soft.h -- shared with the soft front kernels of the batch paths (mbx_soft_front.hip).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64, 8)
fec_imbe7200x4400_soft_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, mbx_param_record* __restrict__ out,
                              DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const uint4 rec = soft_record_imbe7200x4400(S, soft + i * MBX_IMBE_SOFT_BITS, tabs, lane);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&out[i]) = rec;
    }
}

__global__ void __launch_bounds__(64, 8)
fec_ambe3600x2450_soft_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, mbx_param_record* __restrict__ out,
                              DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const uint4 rec = soft_record_ambe3600(S, soft + i * MBX_AMBE_SOFT_BITS, tabs, lane);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&out[i]) = rec;
    }
}

__global__ void __launch_bounds__(64, 8)
fec_imbe7100x4400_soft_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, mbx_param_record* __restrict__ out,
                              DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const uint4 rec = soft_record_imbe7100x4400(S, soft + i * MBX_IMBE7100_SOFT_BITS, tabs, lane);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&out[i]) = rec;
    }
}

// Code-word level soft ECC, batched: kind 0 = Golay (23 soft bits per block), 1 = Hamming (15), 2 = Hamming
// with the IMBE 7100x4400 bit mapping (mbe_7100x4400hamming1511Soft).
// out = corrected word in the cell order of the hard helpers, errs = the reference's return value.
__global__ void __launch_bounds__(64, 8)
ecc_soft_words_kernel(int kind, const mbe_soft_bit* __restrict__ in, size_t n, uint32_t* __restrict__ out, int32_t* __restrict__ errs,
                      DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const int width = (kind == 0) ? 23 : 15;
    load_soft_cells(S, in + i * (size_t)width, width, lane);
    SoftLane L;
    golay_lane_patterns(tabs, lane, L);
    if (kind == 2) {
        hamming_lane_patterns<true>(tabs, lane, L);
    } else {
        hamming_lane_patterns<false>(tabs, lane, L);
    }
    int rel, diffs;
    const uint32_t hard = soft_block(S, tabs, 0, width, 0, 0u, lane, rel);
    const uint32_t w = (kind == 0)   ? golay_soft_wave(tabs, L, hard, 0, S, lane, diffs)
                       : (kind == 1) ? hamming_soft_wave<false>(tabs, L, hard, 0, S, lane, diffs)
                                     : hamming_soft_wave<true>(tabs, L, hard, 0, S, lane, diffs);
    if (lane == 0) {
        out[i] = w;
        if (errs) {
            errs[i] = diffs;
        }
    }
}

}  // namespace mbx
