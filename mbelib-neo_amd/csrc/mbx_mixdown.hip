// mbx_mixdown.hip -- mix-down out (include/mbx_mixdown.h): the int16 rows a step wrote -> talkgroup BUSES, each the saturated sum of
// its input rows times their Q12 gains, as int16 or G.711 bytes, in one or two launches BEHIND the step.  The arithmetic is
// mbx_mixdown.h, shared with the host definition below; the checks, the split and the tables are mbx_mixdown_plan.h, host-only.
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
#include "mbx_mixdown_plan.h"
#include "mbx_mixdown_lanes.h"   // the lane's add, walk and store, shared with mbx_levels.hip

namespace mbx {

// pcm16: the step's rows (16-byte aligned); bus_offset[n_buses + 1], short_bus[n_short], input[]: the plan's tables; out: the bus rows
template <int kOut>
__global__ void __launch_bounds__(256)
mixdown_kernel(const int16_t* __restrict__ pcm16, const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ short_bus,
               const MixdownInput* __restrict__ input, int n_short, void* __restrict__ out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t slot = g / kMixdownPieces;
    if (slot >= (size_t)n_short) {
        return;
    }
    const int piece = (int)(g - slot * kMixdownPieces);
    const int bus = short_bus[slot];
    const int32_t lo = bus_offset[bus], count = bus_offset[bus + 1] - lo;
    int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
    mixdown_sum<1>(pcm16, input + lo, 0, count, piece, acc);
    mixdown_store<kOut>(out, bus, piece, acc);
}
template __global__ void mixdown_kernel<kMixdownPcm16>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);
template __global__ void mixdown_kernel<kMixdownUlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);
template __global__ void mixdown_kernel<kMixdownAlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);

// one workgroup per long bus: long_bus[blockIdx.x] is its bus
template <int kOut>
__global__ void __launch_bounds__(256)
mixdown_long_kernel(const int16_t* __restrict__ pcm16, const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ long_bus,
                    const MixdownInput* __restrict__ input, void* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int32_t part[kMixdownSlices][160];
    const int bus = long_bus[blockIdx.x];
    const int32_t lo = bus_offset[bus], count = bus_offset[bus + 1] - lo;
    const int slice = (int)threadIdx.x / kMixdownPieces, piece = (int)threadIdx.x - slice * kMixdownPieces;
    if (slice < kMixdownSlices) {   // (lanes 240 .. 255 only keep the barrier company)
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
        mixdown_sum<kMixdownSlices>(pcm16, input + lo, slice, count, piece, acc);
        int4* const to = reinterpret_cast<int4*>(&part[slice][piece * kMixdownPiece]);
        to[0] = int4{acc[0], acc[1], acc[2], acc[3]};
        to[1] = int4{acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
    if (threadIdx.x < kMixdownPieces) {
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kMixdownSlices; ++j) {
            const int4* const from = reinterpret_cast<const int4*>(&part[j][(int)threadIdx.x * kMixdownPiece]);
            const int4 a = from[0], b = from[1];
            acc[0] += a.x, acc[1] += a.y, acc[2] += a.z, acc[3] += a.w, acc[4] += b.x, acc[5] += b.y, acc[6] += b.z, acc[7] += b.w;
        }
        mixdown_store<kOut>(out, bus, (int)threadIdx.x, acc);
    }
}
template __global__ void mixdown_long_kernel<kMixdownPcm16>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);
template __global__ void mixdown_long_kernel<kMixdownUlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);
template __global__ void mixdown_long_kernel<kMixdownAlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);

}  // namespace mbx

// ---- the plan (host) ---------------------------------------------------------------------------------------------------------------
// (struct mbx_mixdown_plan, the handle: mbx_mixdown_plan.h -- mbx_levels.hip launches from it too)
namespace mbx {
int mixdown_plan_device(const mbx_mixdown_plan* plan) { return plan ? plan->device : -1; }
}  // namespace mbx

namespace {

int refuse(const char* who, mbx::MixdownRefusal why) {
    char text[200];
    snprintf(text, sizeof(text), "%s: %s", who, mbx::mixdown_refusal_text(why));
    mbx_set_error_text(text);
    return MBE_STATUS_INVALID_ARGUMENT;
}

// the current device, after mbx_init() for it
int ready_device(int* dev) {
    const hipError_t e = hipGetDevice(dev);
    if (e != hipSuccess) {
        return mbx::hip_failed("", "hipGetDevice", e);
    }
    if (!mbx_device_ready(*dev)) {
        mbx_set_error_text("mbx_init() has not been called for the current device");
        return MBX_ENOTINIT;
    }
    return 0;
}

template <int kOut>
void launch(const mbx_mixdown_plan* p, const int16_t* d_pcm16, void* d_out, hipStream_t strm) {
    const mbx::MixdownPlan& plan = p->plan;
    const mbx::MixdownInput* const input = reinterpret_cast<const mbx::MixdownInput*>(p->d_words + plan.at_inputs);
    if (plan.short_grid) {
        hipLaunchKernelGGL(mbx::mixdown_kernel<kOut>, dim3(plan.short_grid), dim3(mbx::kMixdownBlock), 0, strm, d_pcm16, p->d_words,
                           p->d_words + plan.at_short, input, plan.n_short, d_out);
    }
    if (plan.long_grid) {
        hipLaunchKernelGGL(mbx::mixdown_long_kernel<kOut>, dim3(plan.long_grid), dim3(mbx::kMixdownBlock), 0, strm, d_pcm16, p->d_words,
                           p->d_words + plan.at_long, input, d_out);
    }
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
    const int rc = ready_device(&dev);
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
    const char* const who = "mbx_mixdown_host";
    if (!mbx::mixdown_form_ok(form)) {
        return refuse(who, mbx::kMixdownForm);
    }
    mbx::MixdownPlan plan;
    const mbx::MixdownRefusal why = mbx::plan_mixdown(n_buses, bus_offset, src_row, 0, &plan);
    if (why != mbx::kMixdownOk) {
        return refuse(who, why);
    }
    if (!out || (!pcm16 && plan.rows_needed > 0)) {
        mbx_set_error_text("mbx_mixdown_host: pcm16 and out are needed");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (nrows < (size_t)plan.rows_needed) {
        return refuse(who, mbx::kMixdownRows);
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
        for (int n = 0; n < 160; ++n) {
            if (form == MBX_MIXDOWN_PCM16) {
                static_cast<int16_t*>(out)[(size_t)b * 160u + n] = mbx::mixdown_clamp(acc[n]);
            } else {
                static_cast<uint8_t*>(out)[(size_t)b * 160u + n] = mbx::mixdown_byte(form, acc[n]);
            }
        }
    }
    return 0;
}

int mbx_mixdown(const mbx_mixdown_plan* plan, int form, const int16_t* d_pcm16, size_t nrows, void* d_out, void* stream) {
    const char* const who = "mbx_mixdown";
    const mbx::MixdownRefusal why = mbx::mixdown_launch_refused(plan ? &plan->plan : nullptr, form, d_pcm16, nrows, d_out);
    if (why != mbx::kMixdownOk) {
        return why == mbx::kMixdownAlign ? mbx::misaligned(who, "mbx_mixdown.h") : refuse(who, why);
    }
    int dev = -1;
    const int rc = ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    if (dev != plan->device) {
        char text[160];
        snprintf(text, sizeof(text), "%s: the plan was made on device %d, the current device is %d", who, plan->device, dev);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const hipStream_t strm = (hipStream_t)stream;
    if (form == MBX_MIXDOWN_PCM16) {
        launch<mbx::kMixdownPcm16>(plan, d_pcm16, d_out, strm);
    } else if (form == MBX_MIXDOWN_ULAW) {
        launch<mbx::kMixdownUlaw>(plan, d_pcm16, d_out, strm);
    } else {
        launch<mbx::kMixdownAlaw>(plan, d_pcm16, d_out, strm);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mixdown_kernel", e);
}

}  // extern "C"
