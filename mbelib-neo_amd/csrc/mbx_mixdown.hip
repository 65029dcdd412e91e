// mbx_mixdown.hip -- mix-down out (include/mbx_mixdown.h): the int16 rows a step wrote -> talkgroup BUSES, each the saturated sum of
// its input rows times their Q12 gains, as int16 or G.711 bytes, in one or two launches BEHIND the step.  The arithmetic is
// mbx_mixdown.h, shared with the host definition below; the checks, the split and the tables are mbx_mixdown_plan.h, host-only, and so
// is what this unit shares with mbx_levels.hip and mbx_hold.hip on the host: the way from the plan handle to a launch (the device
// check, the tables, the dispatch over the forms) and the prelude and the row store of the three host definitions.  What a lane does
// -- its bus, one input's piece, the walk, the tail of a long bus, the store -- is mbx_mixdown_lanes.h, shared with the same two.
//
// Both kernels share one piece shape: a lane owns a PIECE of 8 samples of one bus, loads 16 B per input and stores 16 B (int16) or
// 8 B (bytes) once; 20 adjacent lanes read one 320-byte row contiguously; the sums are eight int32 per lane.  The clamp and the
// compand happen once, after the sum.  The sum is one of integers that cannot overflow (mbx_mixdown.h), so how it is split over
// lanes, slices and LDS does not show in the bits.
//   short buses  mixdown_kernel: flat lanes, lane = slot * 20 + piece, each loops over its bus's inputs; no LDS; waves diverge only
//                by trip count.  Talkgroups of 2 .. 32 members.
//   long buses   mixdown_long_kernel: one workgroup of 256 per bus, 240 lanes = 12 input slices x 20 pieces, slice j takes inputs
//                j, j + 12, ...; the partial sums go through LDS (12 x 160 int32) and the first 20 lanes reduce and store.  Without
//                it one lane would run 4,096 dependent trips on an all-call bus.
// Both write in the caller's bus order: short_bus[] and long_bus[] of the plan's tables name the bus of a slot / a workgroup.
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include "mbx_mixdown.h"    // the arithmetic: the private header of this directory
#include <mbx_mixdown.h>    // the public header of the same name: include/, first on the include path
#include <mbx_limit.h>      // (mbx_mixdown_sums and its host twin are declared there)
#include "mbx_mixdown_plan.h"
#include "mbx_mixdown_lanes.h"   // a lane's bus, add, walk, tail and store, shared with mbx_levels.hip and mbx_hold.hip

namespace mbx {

// pcm16: the step's rows (16-byte aligned); bus_offset[n_buses + 1], short_bus[n_short], input[]: the plan's tables; out: the bus rows
template <int kOut>
__global__ void __launch_bounds__(256)
mixdown_kernel(const int16_t* __restrict__ pcm16, const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ short_bus,
               const MixdownInput* __restrict__ input, int n_short, void* __restrict__ out) {
    const auto [slot, piece] = mixdown_short_slot();
    if (slot >= (size_t)n_short) {
        return;
    }
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, short_bus, slot);
    int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
    mixdown_sum<1>(pcm16, input + lo, 0, count, piece, acc);
    mixdown_store<kOut>(out, bus, piece, acc);
}
template __global__ void mixdown_kernel<kMixdownPcm16>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);
template __global__ void mixdown_kernel<kMixdownUlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);
template __global__ void mixdown_kernel<kMixdownAlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);
template __global__ void mixdown_kernel<kMixdownSums>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);

// one workgroup per long bus: long_bus[blockIdx.x] is its bus
template <int kOut>
__global__ void __launch_bounds__(256)
mixdown_long_kernel(const int16_t* __restrict__ pcm16, const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ long_bus,
                    const MixdownInput* __restrict__ input, void* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) MixdownPart part;
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, long_bus, blockIdx.x);
    const int slice = (int)threadIdx.x / kMixdownPieces, piece = (int)threadIdx.x - slice * kMixdownPieces;
    if (slice < kMixdownSlices) {   // (lanes 240 .. 255 only keep the barrier company)
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
        mixdown_sum<kMixdownSlices>(pcm16, input + lo, slice, count, piece, acc);
        mixdown_part_put(part, slice, piece, acc);
    }
    __syncthreads();
    if (threadIdx.x < kMixdownPieces) {
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kMixdownSlices; ++j) {
            mixdown_part_add(part, j, (int)threadIdx.x, acc);
        }
        mixdown_store<kOut>(out, bus, (int)threadIdx.x, acc);
    }
}
template __global__ void mixdown_long_kernel<kMixdownPcm16>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);
template __global__ void mixdown_long_kernel<kMixdownUlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);
template __global__ void mixdown_long_kernel<kMixdownAlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);
template __global__ void mixdown_long_kernel<kMixdownSums>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);

}  // namespace mbx

// ---- the plan (host) ---------------------------------------------------------------------------------------------------------------
// (struct mbx_mixdown_plan, the handle, and mixdown_tables, its way to a launch: mbx_mixdown_plan.h -- mbx_levels.hip and mbx_hold.hip
// launch from it too)
namespace mbx {
int mixdown_plan_device(const mbx_mixdown_plan* plan) { return plan ? plan->device : -1; }
}  // namespace mbx

namespace {

int refuse(const char* who, mbx::MixdownRefusal why) { return mbx::refuse(who, mbx::mixdown_refusal_text(why)); }

// mbx_mixdown_host and its sums twin: `out_kind` is the caller's form, or kMixdownSums
int mixdown_host(const char* who, int out_kind, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12,
                 const int16_t* pcm16, size_t nrows, void* out) {
    mbx::MixdownPlan plan;
    if (const char* const why = mbx::mixdown_host_out_refused(out_kind, n_buses, bus_offset, src_row, pcm16, nrows, out, &plan)) {
        return mbx::refuse(who, why);
    }
    for (int b = 0; b < n_buses; ++b) {
        int32_t acc[160] = {0};
        for (int32_t k = bus_offset[b]; k < bus_offset[b + 1]; ++k) {
            const int16_t* const x = pcm16 + (size_t)src_row[k] * 160u;
            const int16_t g = gain_q12 ? gain_q12[k] : (int16_t)mbx::kMixdownUnity;
            for (int n = 0; n < 160; ++n) {
                acc[n] += mbx::mixdown_term(x[n], g);
            }
        }
        mbx::mixdown_put_row(out_kind, acc, b, out);
    }
    return 0;
}

// mbx_mixdown and its sums twin, down ONE launch path: `out` is the caller's form (mixdown_out_of_form), or kMixdownSums
int mixdown_launch(const char* who, const mbx_mixdown_plan* plan, int out, const int16_t* d_pcm16, size_t nrows, void* d_out, void* stream) {
    const mbx::MixdownRefusal why = mbx::mixdown_out_refused(plan ? &plan->plan : nullptr, out, d_pcm16, nrows, d_out);
    if (why != mbx::kMixdownOk) {
        return why == mbx::kMixdownAlign ? mbx::misaligned(who, "mbx_mixdown.h") : refuse(who, why);
    }
    mbx::MixdownTables t;
    const int rc = mbx::mixdown_tables(who, plan, &t);
    if (rc < 0) {
        return rc;
    }
    const mbx::MixdownPlan& p = plan->plan;
    mbx::mixdown_by_out(out, [&](auto k) {
        if (p.short_grid) {
            hipLaunchKernelGGL(mbx::mixdown_kernel<k()>, dim3(p.short_grid), dim3(mbx::kMixdownBlock), 0, (hipStream_t)stream, d_pcm16, t.bus_offset,
                               t.short_bus, t.input, p.n_short, d_out);
        }
        if (p.long_grid) {
            hipLaunchKernelGGL(mbx::mixdown_long_kernel<k()>, dim3(p.long_grid), dim3(mbx::kMixdownBlock), 0, (hipStream_t)stream, d_pcm16, t.bus_offset,
                               t.long_bus, t.input, d_out);
        }
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mixdown_kernel", e);
}

}  // namespace

extern "C" {

static_assert(MBX_MIXDOWN_PCM16 == mbx::kMixdownPcm16 && MBX_MIXDOWN_ULAW == mbx::kMixdownUlaw && MBX_MIXDOWN_ALAW == mbx::kMixdownAlaw
                  && MBX_MIXDOWN_UNITY == mbx::kMixdownUnity && MBX_MIXDOWN_MAX_INPUTS == mbx::kMixdownMaxInputs,
              "one numbering of the forms and one set of limits, in the public header and in mbx_mixdown.h");
static_assert(sizeof(mbx::MixdownInput) == 8 && alignof(mbx::MixdownInput) == 8, "an input is one 8-byte load");

// every refusal first, then the device
int mbx_mixdown_plan_create_split(mbx_mixdown_plan** out, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12,
                                  int long_above) {
    const char* const who = "mbx_mixdown_plan_create";
    if (!out) {
        return refuse(who, mbx::kMixdownNoHandle);
    }
    *out = nullptr;
    mbx::MixdownPlan plan;
    const mbx::MixdownRefusal why = mbx::plan_mixdown(n_buses, bus_offset, src_row, long_above, &plan);
    if (why != mbx::kMixdownOk) {
        return refuse(who, why);
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_mixdown_plan* p = new (std::nothrow) mbx_mixdown_plan();
    if (!p) {
        mbx_set_error_text("mbx_mixdown_plan_create: out of memory");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    p->plan = plan;
    p->device = dev;
    std::vector<int32_t> words(plan.words);
    mbx::fill_mixdown_tables(plan, bus_offset, src_row, gain_q12, words.data());
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_words), words.size() * sizeof(int32_t));
    if (e == hipSuccess) {
        e = hipMemcpy(p->d_words, words.data(), words.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)hipFree(p->d_words);
        delete p;
        return mbx::hip_failed("", "mbx_mixdown_plan_create: upload of the tables", e);
    }
    *out = p;
    return 0;
}

int mbx_mixdown_plan_create(mbx_mixdown_plan** out, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12) {
    return mbx_mixdown_plan_create_split(out, n_buses, bus_offset, src_row, gain_q12, 0);
}

int mbx_mixdown_plan_destroy(mbx_mixdown_plan* plan) {
    if (plan) {
        (void)hipFree(plan->d_words);
        (void)hipGetLastError();
        delete plan;
    }
    return 0;
}

int mbx_mixdown_plan_buses(const mbx_mixdown_plan* plan) { return plan ? plan->plan.n_buses : MBE_STATUS_INVALID_ARGUMENT; }
int mbx_mixdown_plan_rows(const mbx_mixdown_plan* plan) { return plan ? plan->plan.rows_needed : MBE_STATUS_INVALID_ARGUMENT; }
int mbx_mixdown_plan_long_buses(const mbx_mixdown_plan* plan) { return plan ? plan->plan.n_long : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_mixdown_host(int form, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12, const int16_t* pcm16,
                     size_t nrows, void* out) {
    return mixdown_host("mbx_mixdown_host", mbx::mixdown_out_of_form(form), n_buses, bus_offset, src_row, gain_q12, pcm16, nrows, out);
}

int mbx_mixdown_sums_host(int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12, const int16_t* pcm16, size_t nrows,
                          int32_t* out) {
    return mixdown_host("mbx_mixdown_sums_host", mbx::kMixdownSums, n_buses, bus_offset, src_row, gain_q12, pcm16, nrows, out);
}

int mbx_mixdown(const mbx_mixdown_plan* plan, int form, const int16_t* d_pcm16, size_t nrows, void* d_out, void* stream) {
    return mixdown_launch("mbx_mixdown", plan, mbx::mixdown_out_of_form(form), d_pcm16, nrows, d_out, stream);
}

int mbx_mixdown_sums(const mbx_mixdown_plan* plan, const int16_t* d_pcm16, size_t nrows, int32_t* d_out, void* stream) {
    return mixdown_launch("mbx_mixdown_sums", plan, mbx::kMixdownSums, d_pcm16, nrows, d_out, stream);
}

}  // extern "C"
