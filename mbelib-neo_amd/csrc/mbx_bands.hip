// mbx_bands.hip -- band records (include/mbx_bands.h): the int16 rows a step wrote against a caller's bank of K probes -> K records per
// row, { int32 re; int32 im } or uint32 (re^2 + im^2) >> 31, in one launch BEHIND the step.  The arithmetic, the bound and the refusals
// are mbx_bands_plan.h, host-only and shared with the host definition below and with tests/bands_check.cpp.
//
// pcm_bands_kernel<form>.  The lane map is the one pcm_levels_kernel measured its way to (mbx_levels.hip): 16 LANES PER ROW of TEN
// SAMPLES each, 4 rows per 64-lane wave, 16 rows per workgroup; a lane's five dwords of its row are one 16-byte and one 4-byte load at
// its 20-byte offset and stay in registers while the probes pass by.
//   The bank, at most 20,480 B, comes into LDS once per workgroup in 16-byte pieces, and the workgroup then walks the 16-row groups
// blockIdx.x, blockIdx.x + gridDim.x, ... (at most kBandsMaxGrid workgroups: with a group per workgroup 1,048,576 rows would fetch the
// bank 65,536 times, four times the bytes of the rows themselves).  The rows of the next group are requested before the probes of this
// one are summed.
//   In LDS and on the device a probe is 80 PAIRS { dword i of c, dword i of s } (bands_interleave, mbx_bands_plan.h: made once, by
// mbx_band_bank_create), so that a lane fetches both vectors' taps of two samples as one 8-byte word and every probe of a round lies
// at a constant offset from one address (a first build with c and s apart read five ds_read2_b32 per probe and spent 72 vector adds
// per round on their addresses, where this one reads two ds_read2_b64 and a ds_read_b64 and spends 27; by the LDS table some 18
// LDS cycles per probe and wave either way, beside some 100 cycles of vector issue on each of the four SIMDs that share the LDS: the
// kernel is bound by vector issue, as pcm_levels_kernel is).  Lane j of every row reads pairs 5 j .. 5 j + 4 of probe k.
// Per instruction that is 16 distinct 8-byte words at a stride of 10 dwords: banks (a / 4) mod 64 = 10 j mod 64 = 0, 10, 20, 30, 40, 50,
// 60, 6, 16, 26, 36, 46, 56, 2, 12, 22 and the odd bank behind each, all different (and mod 32, as ds_read2_b64 counts them over 16
// contiguous lanes: 0, 10, 20, 30, 8, 18, 28, 6, 16, 26, 4, 14, 24, 2, 12, 22, sixteen different even banks); the other row groups
// read the SAME addresses, which broadcast.  No conflict, no padding.
//   The sums are v_dot2_i32_i16, ten per probe and lane, exact because every partial sum is inside int32 under the bank's bound.  The
// two row reductions per probe are the four DPP xor steps of pcm_levels_kernel (quad_perm, quad_perm, row_half_mirror, row_mirror): no
// LDS, no ds_bpermute.  Afterwards every lane of the row holds the totals; lane j KEEPS those of probe j (and of probe 16 + j in a
// second round), so the records of a row leave as contiguous 8- or 4-byte stores from up to 16 lanes, not as K stores from lane 0.
// The power form is two 64-bit multiply-adds and a shift, in the lane that stores.  Rows beyond nrows load nothing and store nothing,
// and still walk the reductions, so that no lane reads a lane that has left.  No atomics, no scratch.
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include <mbx_bands.h>
#include "mbx_bands_plan.h"

namespace mbx {

static_assert(sizeof(mbx_band_record) == 8 && offsetof(mbx_band_record, re) == 0 && offsetof(mbx_band_record, im) == 4, "a complex record is re, then im");
static_assert(kBandsMaxProbes * kBandsProbeBytes == 20480 && kBandsProbeBytes % 16 == 0, "the bank in LDS, in 16-byte pieces");

// A lane's share of a row: ten samples, five dwords at the lane's 20-byte offset (4-byte aligned, no more)
struct alignas(4) BandShare {
    uint32_t w[kBandsSamples / 2];
};

// a value of the lane `lane ^ m` of the 16 lanes of a row, m = 1, 2, 4, 8 (level_row_xor of mbx_levels.hip: the 16 lanes of a row are a
// DPP row, and once the lanes that differ in the lower bits hold equal values the mirrors reach a lane that holds what lane ^ m holds)
template <int kXor>
__device__ __forceinline__ int32_t band_row_xor(int32_t v) {
    constexpr int kCtrl = kXor == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : kXor == 2 ? 0x4E /* quad_perm [2,3,0,1] */
                        : kXor == 4 ? 0x141 /* row_half_mirror */ : 0x140 /* row_mirror */;
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, 0xF, 0xF, false);
}
__device__ __forceinline__ int32_t band_row_total(int32_t v) {   // (wrapping adds of parts whose every partial sum is inside int32)
    v += band_row_xor<1>(v);   // (lowest bit first: the mirrors need the lanes below them level)
    v += band_row_xor<2>(v);
    v += band_row_xor<4>(v);
    v += band_row_xor<8>(v);
    return v;
}

__device__ __forceinline__ BandShare band_share_of(const int16_t* __restrict__ pcm16, size_t row, int j, bool live) {
    BandShare mine = {};
    if (live) {
        mine = *reinterpret_cast<const BandShare*>(pcm16 + row * 160u + (size_t)(j * kBandsSamples));
    }
    return mine;
}

// bank: K probes of 80 pairs { c, s } of dwords, as bands_interleave lays them out (16-byte aligned); pcm16: nrows rows (16-byte aligned); out: nrows * K records of kForm (16-byte aligned)
template <int kForm>
__global__ void __launch_bounds__(kBandsBlock)
pcm_bands_kernel(const uint32_t* __restrict__ bank, int K, const int16_t* __restrict__ pcm16, size_t nrows, void* __restrict__ out) {
    __shared__ uint4 lds[kBandsMaxProbes * kBandsProbeWords / 4];
    const int tid = (int)threadIdx.x;
    const int j = tid % kBandsLanes, local = tid / kBandsLanes;
    const size_t groups = (nrows + kBandsBlockRows - 1) / kBandsBlockRows;
    size_t group = blockIdx.x;
    BandShare mine = band_share_of(pcm16, group * kBandsBlockRows + (size_t)local, j, group * kBandsBlockRows + (size_t)local < nrows);
    for (int piece = tid; piece < K * (kBandsProbeWords / 4); piece += kBandsBlock) {
        lds[piece] = reinterpret_cast<const uint4*>(bank)[piece];
    }
    __syncthreads();
    const uint2* const mine_of_bank = reinterpret_cast<const uint2*>(lds) + j * (kBandsSamples / 2);
    for (; group < groups; group += gridDim.x) {   // (uniform over the workgroup: every lane walks every reduction)
        const size_t row = group * kBandsBlockRows + (size_t)local;
        const bool   live = row < nrows;
        const size_t next_row = row + (size_t)gridDim.x * kBandsBlockRows;
        const BandShare ahead = band_share_of(pcm16, next_row, j, next_row < nrows);   // (beyond the last group next_row >= nrows)
        for (int first = 0; first < K; first += kBandsLanes) {   // a round: the probes first .. first + 15, lane j keeps first + j
            const uint2* const round = mine_of_bank + first * (kBandsProbeWords / 2);
            int32_t keep_re = 0, keep_im = 0;
#pragma unroll
            for (int kk = 0; kk < kBandsLanes; ++kk) {
                if (first + kk < K) {   // (uniform)
                    int32_t re = 0, im = 0;
#pragma unroll
                    for (int i = 0; i < kBandsSamples / 2; ++i) {
                        const uint2 cs = round[kk * (kBandsProbeWords / 2) + i];
                        re = bands_dot2(mine.w[i], cs.x, re);
                        im = bands_dot2(mine.w[i], cs.y, im);
                    }
                    re = band_row_total(re);
                    im = band_row_total(im);
                    keep_re = j == kk ? re : keep_re;
                    keep_im = j == kk ? im : keep_im;
                }
            }
            if (live && first + j < K) {
                const size_t at = row * (size_t)K + (size_t)(first + j);
                if (kForm == kBandsComplex) {
                    reinterpret_cast<int2*>(out)[at] = int2{keep_re, keep_im};
                } else {
                    reinterpret_cast<uint32_t*>(out)[at] = bands_power(keep_re, keep_im);
                }
            }
        }
        mine = ahead;
    }
}
template __global__ void pcm_bands_kernel<kBandsComplex>(const uint32_t*, int, const int16_t*, size_t, void*);
template __global__ void pcm_bands_kernel<kBandsPower>(const uint32_t*, int, const int16_t*, size_t, void*);

}  // namespace mbx

namespace {

int refuse(const char* who, mbx::BandsRefusal why) {
    return why == mbx::kBandsAlign ? mbx::misaligned(who, "mbx_bands.h") : mbx::refuse(who, mbx::bands_refusal_text(why));
}

// a bank as the caller gives it: the pointers, K and the bound, the vector that broke it by name
int bank_refused(const char* who, bool have_place, const int16_t* probes, int K) {
    int      probe = 0;
    char     which = 'c';
    uint32_t sum = 0;
    const mbx::BandsRefusal why = mbx::bands_bank_refused(have_place, probes, K, &probe, &which, &sum);
    if (why == mbx::kBandsBound) {
        char text[120];
        mbx::bands_bound_text(text, sizeof(text), probe, which, sum);
        return mbx::refuse(who, text);
    }
    return why == mbx::kBandsOk ? 0 : refuse(who, why);
}

}  // namespace

extern "C" {

static_assert(MBX_BANDS_MAX_PROBES == mbx::kBandsMaxProbes && MBX_BANDS_VECTOR_BOUND == mbx::kBandsVectorBound && MBX_BANDS_COMPLEX == mbx::kBandsComplex
                  && MBX_BANDS_POWER == mbx::kBandsPower,
              "one set of limits, in the public header and in mbx_bands_plan.h");

int mbx_band_bank_create(mbx_band_bank** out, const int16_t* probes, int K) {
    const char* const who = "mbx_band_bank_create";
    if (out) {
        *out = nullptr;
    }
    int rc = bank_refused(who, out != nullptr, probes, K);
    if (rc < 0) {
        return rc;
    }
    int dev = -1;
    rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_band_bank* b = new (std::nothrow) mbx_band_bank();
    if (!b) {
        return mbx::refuse(who, "out of memory");
    }
    b->device = dev;
    b->K = K;
    std::vector<uint32_t> image((size_t)K * mbx::kBandsProbeWords);
    for (int k = 0; k < K; ++k) {
        mbx::bands_interleave(probes + (size_t)k * 2u * mbx::kBandsVector, image.data() + (size_t)k * mbx::kBandsProbeWords);
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->d_probes), mbx::bands_bank_bytes(K));
    if (e == hipSuccess) {   // (a blocking copy from pageable memory: the image may go when the call returns)
        e = hipMemcpy(b->d_probes, image.data(), mbx::bands_bank_bytes(K), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {   // (the copy is on the null stream, and the launches that read the bank may be on a non-blocking one)
        e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipFree(b->d_probes);
        delete b;
        return mbx::hip_failed("", "mbx_band_bank_create: the probes", e);
    }
    *out = b;
    return 0;
}

int mbx_band_bank_destroy(mbx_band_bank* b) {
    if (b) {
        (void)hipFree(b->d_probes);
        (void)hipGetLastError();
        delete b;
    }
    return 0;
}

int mbx_band_bank_probes(const mbx_band_bank* b) { return b ? b->K : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_pcm_bands_host(const int16_t* probes, int K, int form, const int16_t* pcm16, size_t nrows, void* out) {
    const char* const who = "mbx_pcm_bands_host";
    if (!pcm16 || !out) {
        return refuse(who, mbx::kBandsPointers);
    }
    const int rc = bank_refused(who, true, probes, K);
    if (rc < 0) {
        return rc;
    }
    const mbx::BandsRefusal why = mbx::bands_shape_refused(K, form, nrows);
    if (why != mbx::kBandsOk) {
        return refuse(who, why);
    }
    for (size_t r = 0; r < nrows; ++r) {
        for (int k = 0; k < K; ++k) {
            const int16_t* const c = probes + (size_t)k * 2u * mbx::kBandsVector;
            const int32_t re = mbx::bands_sum(pcm16 + r * 160u, c), im = mbx::bands_sum(pcm16 + r * 160u, c + mbx::kBandsVector);
            const size_t at = r * (size_t)K + (size_t)k;
            if (form == mbx::kBandsComplex) {
                static_cast<mbx_band_record*>(out)[at] = mbx_band_record{re, im};
            } else {
                static_cast<uint32_t*>(out)[at] = mbx::bands_power(re, im);
            }
        }
    }
    return 0;
}

int mbx_pcm_bands(const mbx_band_bank* b, int form, const int16_t* d_pcm16, size_t nrows, void* d_out, void* stream) {
    const char* const who = "mbx_pcm_bands";
    const mbx::BandsRefusal why = mbx::bands_launch_refused(b ? b->K : 0, form, d_pcm16, nrows, d_out);
    if (why != mbx::kBandsOk) {
        return refuse(who, why);
    }
    if (nrows == 0) {
        return 0;
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    if (b->device != dev) {
        return mbx::refuse(who, "a bank of another device than the current one");
    }
    const dim3 grid(mbx::bands_grid(nrows)), block(mbx::kBandsBlock);
    if (form == mbx::kBandsComplex) {
        hipLaunchKernelGGL(mbx::pcm_bands_kernel<mbx::kBandsComplex>, grid, block, 0, (hipStream_t)stream, b->d_probes, b->K, d_pcm16, nrows, d_out);
    } else {
        hipLaunchKernelGGL(mbx::pcm_bands_kernel<mbx::kBandsPower>, grid, block, 0, (hipStream_t)stream, b->d_probes, b->K, d_pcm16, nrows, d_out);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "pcm_bands_kernel", e);
}

}  // extern "C"
