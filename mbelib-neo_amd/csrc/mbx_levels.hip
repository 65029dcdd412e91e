// mbx_levels.hip -- levels out and the gated mix-down (include/mbx_levels.h): the int16 rows a step wrote -> one 16-byte level record
// per row (energy, peak, clipped), and talkgroup buses that sum only the inputs a gate CHOOSES by those records, in one launch for the
// levels and one or two for the buses, BEHIND the step.  The arithmetic is mbx_levels.h, shared with the host definitions below; the
// checks are mbx_levels_plan.h, host-only; the plan, its tables, the way from its handle to a launch and the prelude of the host
// definition are those of mbx_mixdown.hip (mbx_mixdown_plan.h), and a lane's bus, add, walk, long tail and store are
// mbx_mixdown_lanes.h, shared with the kernels there and in mbx_hold.hip.
//
// pcm_levels_kernel.  A row is 320 B, and its level is a reduction over the lanes that share it.  The partition: 16 LANES PER ROW of
// TEN SAMPLES each, 4 rows per 64-lane wave.  Why: the kernel is bound by vector issue, not by bytes (a first build with lane j on the
// 16-byte piece j and lanes 0 .. 3 on piece 16 + j as well issued both pieces' work in every wave for a quarter of its lanes: 193
// vector instructions and 16 ds_bpermute per wave, 94 us per 1,048,576 rows where the compand launch took 90; EXPERIMENTS "Levels and
// gated mix-down"), so the work has to be level across the lanes and short.  16 lanes are a DPP row, so the four xor steps of the
// reduction are v_mov_b32_dpp / v_add_u32_dpp (quad_perm, quad_perm, row_half_mirror, row_mirror) and touch no LDS crossbar; ten samples
// are five dwords, the same for every lane, loaded as one 16-byte and one 4-byte load at the lane's 20-byte offset (4-byte aligned,
// which a global load may be), a wave reading 1,280 contiguous bytes; and two samples of a dword are handled at once by the packed
// 16-bit instructions and one dot product.  Against "20 lanes of 8 samples, 3 rows per wave": aligned 16-byte loads, but 4 idle
// lanes in 64, a reduction over 20 lanes that no DPP or xor pattern covers, and a division by 3 in the address.  Lane 0 of the row
// stores the record as one 16-byte store.  No LDS, no atomics.  Rows beyond nrows load nothing and store nothing, and still walk the
// reduction, so that no lane reads a lane that has left.
//
// mixdown_gated_kernel (short buses): the lane map of mixdown_kernel.  A lane first walks its bus's inputs reading only the level
// records (16 B, the same address across the 20 lanes of a bus, which straddle waves and cannot shuffle: each selects for itself) and
// keeps the 8 largest keys in registers by an unrolled insertion; the N-th is the threshold.  Then the sum, four inputs at a time as
// mixdown_sum has it, with the row load of every input below the threshold skipped.
// mixdown_gated_long_kernel: one workgroup of 256 per bus.  With loudest_n = 0 the 12-slice pass of mixdown_long_kernel, closed inputs
// skipped.  With loudest_n = N: the lanes stride over the inputs, at most 16 keys each in registers; N rounds of a workgroup-wide
// maximum "largest key below the previous round's" (a wave reduction, then 4 words through LDS) name the N chosen inputs to every
// lane, the position of each in the low bits of its key; the first 20 lanes sum those at most 8 rows.  No slice pass.
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include "mbx_levels.h"    // the arithmetic: the private header of this directory
#include <mbx_levels.h>    // the public header of the same name: include/, first on the include path
#include <mbx_limit.h>     // (mbx_mixdown_gated_sums and its host twin are declared there)
#include "mbx_levels_plan.h"
#include "mbx_mixdown_lanes.h"

namespace mbx {

static_assert(sizeof(mbx_row_level) == 16 && alignof(mbx_row_level) == 8 && offsetof(mbx_row_level, energy) == 0 && offsetof(mbx_row_level, peak) == 8
                  && offsetof(mbx_row_level, clipped) == 10 && offsetof(mbx_row_level, zero) == 12,
              "a level record is 16 bytes: energy at 0, peak at 8, clipped at 10");
static_assert(sizeof(mbx_row_level) == kLevelBytes, "mbx_levels_plan.h counts the bytes of d_levels with it");

// A lane's share of a row in pcm_levels_kernel: ten samples, five dwords at the lane's 20-byte offset (4-byte aligned, no more)
struct alignas(4) LevelShare {
    uint32_t w[kLevelSamples / 2];
};
typedef unsigned short level_u16x2 __attribute__((ext_vector_type(2)));
typedef short          level_i16x2 __attribute__((ext_vector_type(2)));

// Two samples of one dword into a lane's part of the level, BOTH HALVES AT ONCE with the packed 16-bit instructions; the values are
// those of level_add_sample (mbx_levels.h), which stays the definition:
//   s = x >> 15 (0 or -1), t = x ^ s = the one's-complement magnitude, 0 .. 32767; |x| = t - s as uint16, 32768 for -32768;
//   x is 32767 or -32768 iff t == 32767 iff bit 15 of t + 1 is set;  x^2 + y^2 <= 2^31 is one unsigned dot product.
struct LevelPart {
    uint64_t    energy = 0;
    level_u16x2 peak = {0, 0};   // of the low and of the high samples, apart until the end
    uint32_t    clipped = 0;
};
__device__ __forceinline__ void level_add_pair(LevelPart& l, uint32_t w) {
    const level_i16x2 x = __builtin_bit_cast(level_i16x2, w);
    const level_i16x2 s = x >> (level_i16x2){15, 15};
    const level_u16x2 t = __builtin_bit_cast(level_u16x2, (level_i16x2)(x ^ s));
    const level_u16x2 a = t - __builtin_bit_cast(level_u16x2, s);
    l.peak = __builtin_elementwise_max(l.peak, a);
    l.energy += (uint64_t)__builtin_amdgcn_udot2(a, a, 0u, false);
    const level_u16x2 c = (t + (level_u16x2){1, 1}) >> (level_u16x2){15, 15};
    l.clipped = __builtin_amdgcn_udot2(c, (level_u16x2){1, 1}, l.clipped, false);
}

// a value of the lane `lane ^ m` of the 16 lanes of a row, m = 1, 2, 4, 8: the 16 lanes of a row are a DPP row, and once the lanes
// that differ in the lower bits hold equal values, the mirrors of 8 and of 16 lanes reach a lane that holds what lane ^ m holds
template <int kXor>
__device__ __forceinline__ uint32_t level_row_xor(uint32_t v) {
    constexpr int kCtrl = kXor == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : kXor == 2 ? 0x4E /* quad_perm [2,3,0,1] */
                        : kXor == 4 ? 0x141 /* row_half_mirror */ : 0x140 /* row_mirror */;
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}
template <int kXor>
__device__ __forceinline__ void level_merge_row(uint32_t& lo, uint32_t& hi, level_u16x2& peak, uint32_t& clipped) {
    const uint64_t e = ((uint64_t)lo | ((uint64_t)hi << 32)) + ((uint64_t)level_row_xor<kXor>(lo) | ((uint64_t)level_row_xor<kXor>(hi) << 32));
    lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
    peak = __builtin_elementwise_max(peak, __builtin_bit_cast(level_u16x2, level_row_xor<kXor>(__builtin_bit_cast(uint32_t, peak))));
    clipped += level_row_xor<kXor>(clipped);
}

// pcm16: nrows rows (16-byte aligned); levels: nrows records
__global__ void __launch_bounds__(kLevelsBlock)
pcm_levels_kernel(const int16_t* __restrict__ pcm16, size_t nrows, mbx_row_level* __restrict__ levels) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t row = g / kLevelLanes;
    const int j = (int)(g % kLevelLanes);
    const bool live = row < nrows;
    LevelPart l;
    if (live) {
        const LevelShare mine = *reinterpret_cast<const LevelShare*>(pcm16 + row * 160u + (size_t)(j * kLevelSamples));
#pragma unroll
        for (int i = 0; i < kLevelSamples / 2; ++i) {
            level_add_pair(l, mine.w[i]);
        }
    }
    uint32_t lo = (uint32_t)l.energy, hi = (uint32_t)(l.energy >> 32);   // (a lane's part is at most 10 * 2^30: the halves travel apart)
    level_merge_row<1>(lo, hi, l.peak, l.clipped);   // (lowest bit first: the mirrors need the lanes below them level)
    level_merge_row<2>(lo, hi, l.peak, l.clipped);
    level_merge_row<4>(lo, hi, l.peak, l.clipped);
    level_merge_row<8>(lo, hi, l.peak, l.clipped);
    if (live && j == 0) {
        const uint32_t peak = l.peak.x > l.peak.y ? l.peak.x : l.peak.y;
        *reinterpret_cast<uint4*>(levels + row) = uint4{lo, hi, peak | (l.clipped << 16), 0u};
    }
}

// the key of the input `in` at position k of its bus, from its row's record: one 16-byte load
__device__ __forceinline__ uint64_t gate_key_of(const mbx_row_level* __restrict__ levels, const MixdownInput in, int32_t k, uint32_t open_peak) {
    const uint4 v = *reinterpret_cast<const uint4*>(levels + in.row);
    return gate_key((uint64_t)v.x | ((uint64_t)v.y << 32), v.z & 0xFFFFu, k, open_peak);
}

// mixdown_sum (mbx_mixdown_lanes.h) under a gate: the same batches of four, the key of every input from its record, and the row load
// of an input whose key is below the threshold skipped.  (threshold >= 1, and the filler of a short batch has the key 0.)
template <int kStep>
__device__ __forceinline__ void mixdown_gated_sum(const int16_t* __restrict__ pcm16, const mbx_row_level* __restrict__ levels,
                                                  const MixdownInput* __restrict__ input, int32_t first, int32_t count, int piece, uint32_t open_peak,
                                                  uint64_t threshold, int32_t acc[kMixdownPiece]) {
    constexpr int kBatch = 4;
    for (int32_t i = first; i < count; i += kBatch * kStep) {
        MixdownInput in[kBatch];
        bool chosen[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int32_t k = i + j * kStep;
            in[j] = input[k < count ? k : i];
            chosen[j] = (k < count ? gate_key_of(levels, in[j], k, open_peak) : 0u) >= threshold;
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            if (chosen[j]) {
                mixdown_add_input(pcm16, in[j], piece, acc);
            }
        }
    }
}

// the arguments of mixdown_kernel, the records of the rows and the gate
template <int kOut>
__global__ void __launch_bounds__(256)
mixdown_gated_kernel(const int16_t* __restrict__ pcm16, const mbx_row_level* __restrict__ levels, const int32_t* __restrict__ bus_offset,
                     const int32_t* __restrict__ short_bus, const MixdownInput* __restrict__ input, int n_short, uint32_t open_peak, int loudest_n,
                     void* __restrict__ out) {
    const auto [slot, piece] = mixdown_short_slot();
    if (slot >= (size_t)n_short) {
        return;
    }
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, short_bus, slot);
    uint64_t top[kGateMaxLoudest] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t k = 0; loudest_n > 0 && k < count; ++k) {   // (a plan may make any bus short: correct for every count up to 4,096)
        gate_insert(top, gate_key_of(levels, input[lo + k], k, open_peak));
    }
    const uint64_t threshold = gate_threshold_of(top, loudest_n);
    int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
    mixdown_gated_sum<1>(pcm16, levels, input + lo, 0, count, piece, open_peak, threshold, acc);
    mixdown_store<kOut>(out, bus, piece, acc);
}
template __global__ void mixdown_gated_kernel<kMixdownPcm16>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, int, uint32_t, int, void*);
template __global__ void mixdown_gated_kernel<kMixdownUlaw>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, int, uint32_t, int, void*);
template __global__ void mixdown_gated_kernel<kMixdownAlaw>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, int, uint32_t, int, void*);
template __global__ void mixdown_gated_kernel<kMixdownSums>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, int, uint32_t, int, void*);

// one workgroup per long bus: long_bus[blockIdx.x] is its bus
template <int kOut>
__global__ void __launch_bounds__(256)
mixdown_gated_long_kernel(const int16_t* __restrict__ pcm16, const mbx_row_level* __restrict__ levels, const int32_t* __restrict__ bus_offset,
                          const int32_t* __restrict__ long_bus, const MixdownInput* __restrict__ input, uint32_t open_peak, int loudest_n,
                          void* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) MixdownPart part;
    __shared__ uint64_t wave_max[kGateWaves];
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, long_bus, blockIdx.x);
    const int tid = (int)threadIdx.x;
    if (loudest_n == 0) {   // every open input: mixdown_long_kernel's slice pass, closed inputs skipped
        const int slice = tid / kMixdownPieces, piece = tid - slice * kMixdownPieces;
        if (slice < kMixdownSlices) {
            int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
            mixdown_gated_sum<kMixdownSlices>(pcm16, levels, input + lo, slice, count, piece, open_peak, 1u, acc);
            mixdown_part_put(part, slice, piece, acc);
        }
        __syncthreads();
        if (tid < kMixdownPieces) {
            int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < kMixdownSlices; ++j) {
                mixdown_part_add(part, j, tid, acc);
            }
            mixdown_store<kOut>(out, bus, tid, acc);
        }
        return;
    }
    // the keys of inputs tid, tid + 256, ...: at most 16, in registers
    uint64_t key[kGateKeysPerLane];
#pragma unroll
    for (int j = 0; j < kGateKeysPerLane; ++j) {
        const int32_t k = tid + j * kMixdownBlock;
        key[j] = k < count ? gate_key_of(levels, input[lo + k], k, open_peak) : 0u;
    }
    // N rounds: the largest key below the previous round's winner.  Keys are unique within a bus, so a round names one input; a round
    // that finds 0 has run out of open inputs, and so have all behind it.  Every lane reads the same winner, so `more` is uniform and
    // the barriers below are reached by all 256 lanes or by none.  (hold_long_kernel has the same rounds: mbx_mixdown_lanes.h says why.)
    uint64_t chosen[kGateMaxLoudest] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t below = ~(uint64_t)0;
    bool more = true;
#pragma unroll
    for (int r = 0; r < kGateMaxLoudest; ++r) {
        if (r < loudest_n && more) {
            uint64_t m = 0;
#pragma unroll
            for (int j = 0; j < kGateKeysPerLane; ++j) {
                m = (key[j] < below && key[j] > m) ? key[j] : m;
            }
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) {
                const uint64_t o = (uint64_t)__shfl_xor((uint32_t)m, x, 64) | ((uint64_t)__shfl_xor((uint32_t)(m >> 32), x, 64) << 32);
                m = o > m ? o : m;
            }
            if ((tid & 63) == 0) {
                wave_max[tid >> 6] = m;
            }
            __syncthreads();
            m = wave_max[0];
#pragma unroll
            for (int w = 1; w < kGateWaves; ++w) {
                m = wave_max[w] > m ? wave_max[w] : m;
            }
            __syncthreads();   // (the next round writes wave_max again)
            chosen[r] = m;
            below = m;
            more = m != 0;
        }
    }
    if (tid < kMixdownPieces) {   // at most 8 rows: the loads in flight together, no slice pass
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
        MixdownInput in[kGateMaxLoudest];
#pragma unroll
        for (int r = 0; r < kGateMaxLoudest; ++r) {
            in[r] = chosen[r] ? input[lo + gate_key_position(chosen[r])] : MixdownInput{0, 0};
        }
#pragma unroll
        for (int r = 0; r < kGateMaxLoudest; ++r) {
            if (chosen[r]) {
                mixdown_add_input(pcm16, in[r], tid, acc);
            }
        }
        mixdown_store<kOut>(out, bus, tid, acc);
    }
}
template __global__ void mixdown_gated_long_kernel<kMixdownPcm16>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, uint32_t, int, void*);
template __global__ void mixdown_gated_long_kernel<kMixdownUlaw>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, uint32_t, int, void*);
template __global__ void mixdown_gated_long_kernel<kMixdownAlaw>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, uint32_t, int, void*);
template __global__ void mixdown_gated_long_kernel<kMixdownSums>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, uint32_t, int, void*);

}  // namespace mbx

namespace {

using mbx::refuse;

int refuse(const char* who, mbx::LevelsRefusal why, mbx::MixdownRefusal mix = mbx::kMixdownOk) {
    if (why == mbx::kLevelsAlign || (why == mbx::kGateMixdown && mix == mbx::kMixdownAlign)) {
        return mbx::misaligned(who, "mbx_levels.h");
    }
    return refuse(who, why == mbx::kGateMixdown ? mbx::mixdown_refusal_text(mix) : mbx::levels_refusal_text(why));
}

// mbx_mixdown_gated_host and its sums twin: `out_kind` is the caller's form, or kMixdownSums
int gated_host(const char* who, int out_kind, const mbx_mixdown_gate* gate, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
               const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, void* out) {
    const mbx::LevelsRefusal bad_gate = mbx::gate_refused(gate != nullptr, gate ? gate->open_peak : 0u, gate ? gate->loudest_n : 0u);
    if (bad_gate != mbx::kLevelsOk) {
        return refuse(who, bad_gate);
    }
    mbx::MixdownPlan plan;
    if (const char* const why = mbx::mixdown_host_out_refused(out_kind, n_buses, bus_offset, src_row, pcm16, nrows, out, &plan)) {
        return refuse(who, why);
    }
    std::vector<uint64_t> keys;
    for (int b = 0; b < n_buses; ++b) {
        const int32_t lo = bus_offset[b], count = bus_offset[b + 1] - lo;
        keys.resize((size_t)count);
        for (int32_t k = 0; k < count; ++k) {   // (the levels of the rows as they are, before the gain)
            const mbx::Level l = mbx::level_of_row(pcm16 + (size_t)src_row[lo + k] * 160u);
            keys[(size_t)k] = mbx::gate_key(l.energy, l.peak, k, gate->open_peak);
        }
        const uint64_t threshold = mbx::gate_threshold(keys.data(), count, gate->loudest_n);
        int32_t acc[160] = {0};
        for (int32_t k = 0; k < count; ++k) {
            const int16_t* const x = pcm16 + (size_t)src_row[lo + k] * 160u;
            // THE definition: an input that is not chosen has the gain 0
            const int16_t g = keys[(size_t)k] >= threshold ? (gain_q12 ? gain_q12[lo + k] : (int16_t)mbx::kMixdownUnity) : (int16_t)0;
            for (int n = 0; n < 160; ++n) {
                acc[n] += mbx::mixdown_term(x[n], g);
            }
        }
        mbx::mixdown_put_row(out_kind, acc, b, out);
    }
    return 0;
}

// mbx_mixdown_gated and its sums twin, down ONE launch path: `out` is the caller's form (mixdown_out_of_form), or kMixdownSums
int gated_launch(const char* who, const mbx_mixdown_plan* plan, const mbx_mixdown_gate* gate, int out, const int16_t* d_pcm16, size_t nrows,
                 const mbx_row_level* d_levels, void* d_out, void* stream) {
    mbx::MixdownRefusal mix = mbx::kMixdownOk;
    const mbx::LevelsRefusal why = mbx::gated_launch_refused(plan ? &plan->plan : nullptr, gate != nullptr, gate ? gate->open_peak : 0u,
                                                             gate ? gate->loudest_n : 0u, out, d_pcm16, nrows, d_levels, d_out, &mix,
                                                             out == mbx::kMixdownSums);
    if (why != mbx::kLevelsOk) {
        return refuse(who, why, mix);
    }
    mbx::MixdownTables t;
    const int rc = mbx::mixdown_tables(who, plan, &t);
    if (rc < 0) {
        return rc;
    }
    const mbx::MixdownPlan& p = plan->plan;
    const uint32_t open_peak = gate->open_peak;
    const int loudest_n = gate->loudest_n;
    mbx::mixdown_by_out(out, [&](auto k) {
        if (p.short_grid) {
            hipLaunchKernelGGL(mbx::mixdown_gated_kernel<k()>, dim3(p.short_grid), dim3(mbx::kMixdownBlock), 0, (hipStream_t)stream, d_pcm16, d_levels,
                               t.bus_offset, t.short_bus, t.input, p.n_short, open_peak, loudest_n, d_out);
        }
        if (p.long_grid) {
            hipLaunchKernelGGL(mbx::mixdown_gated_long_kernel<k()>, dim3(p.long_grid), dim3(mbx::kMixdownBlock), 0, (hipStream_t)stream, d_pcm16,
                               d_levels, t.bus_offset, t.long_bus, t.input, open_peak, loudest_n, d_out);
        }
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mixdown_gated_kernel", e);
}

}  // namespace

extern "C" {

static_assert(MBX_GATE_MAX_LOUDEST == mbx::kGateMaxLoudest, "one limit, in the public header and in mbx_levels.h");

int mbx_pcm_levels_host(const int16_t* pcm16, size_t nrows, mbx_row_level* out) {
    if (!pcm16 || !out) {
        return refuse("mbx_pcm_levels_host", "pcm16 and out are needed");
    }
    for (size_t r = 0; r < nrows; ++r) {
        const mbx::Level l = mbx::level_of_row(pcm16 + r * 160u);
        out[r] = mbx_row_level{l.energy, (uint16_t)l.peak, (uint16_t)l.clipped, 0u};
    }
    return 0;
}

int mbx_pcm_levels(const int16_t* d_pcm16, size_t nrows, mbx_row_level* d_levels, void* stream) {
    const char* const who = "mbx_pcm_levels";
    const mbx::LevelsRefusal why = mbx::levels_launch_refused(d_pcm16, nrows, d_levels);
    if (why != mbx::kLevelsOk) {
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
    hipLaunchKernelGGL(mbx::pcm_levels_kernel, dim3(mbx::levels_grid(nrows)), dim3(mbx::kLevelsBlock), 0, (hipStream_t)stream, d_pcm16, nrows, d_levels);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "pcm_levels_kernel", e);
}

int mbx_mixdown_gated_host(int form, const mbx_mixdown_gate* gate, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                           const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, void* out) {
    return gated_host("mbx_mixdown_gated_host", mbx::mixdown_out_of_form(form), gate, n_buses, bus_offset, src_row, gain_q12, pcm16, nrows, out);
}

int mbx_mixdown_gated_sums_host(const mbx_mixdown_gate* gate, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                                const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, int32_t* out) {
    return gated_host("mbx_mixdown_gated_sums_host", mbx::kMixdownSums, gate, n_buses, bus_offset, src_row, gain_q12, pcm16, nrows, out);
}

int mbx_mixdown_gated(const mbx_mixdown_plan* plan, const mbx_mixdown_gate* gate, int form, const int16_t* d_pcm16, size_t nrows,
                      const mbx_row_level* d_levels, void* d_out, void* stream) {
    return gated_launch("mbx_mixdown_gated", plan, gate, mbx::mixdown_out_of_form(form), d_pcm16, nrows, d_levels, d_out, stream);
}

int mbx_mixdown_gated_sums(const mbx_mixdown_plan* plan, const mbx_mixdown_gate* gate, const int16_t* d_pcm16, size_t nrows,
                           const mbx_row_level* d_levels, int32_t* d_out, void* stream) {
    return gated_launch("mbx_mixdown_gated_sums", plan, gate, mbx::kMixdownSums, d_pcm16, nrows, d_levels, d_out, stream);
}

}  // extern "C"
