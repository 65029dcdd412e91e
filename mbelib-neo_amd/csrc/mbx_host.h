// mbx_host.h -- what the host units of libmbx_hip.so (mbx_api.hip, mbx_session.hip, mbx_burst.hip, mbx_collective.hip, mbx_pcm8.hip,
// mbx_mixdown.hip, mbx_levels.hip, mbx_hold.hip, mbx_agc.hip, mbx_limit.hip, mbx_bands.hip, mbx_vote.hip) share to refuse a call: the per-thread text behind mbx_last_error(), the "who: why"
// refusal, the failed-HIP-call text, the alignment refusal, the current device after mbx_init().  Host-only and private; the inlines
// have internal linkage, nothing here is exported.  Only what at least two units use belongs here.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>

#include "mbx.h"

void mbx_set_error_text(const char* text);   // mbx_api.hip: sets the calling thread's mbx_last_error()

struct mbx_mixdown_plan;
struct mbx_vote_plan;
struct mbx_vote_record;

namespace mbx {

int mixdown_plan_device(const mbx_mixdown_plan* plan);   // mbx_mixdown.hip: the device a plan's tables are on (-1: no plan)

// mbx_vote.hip: the two launches of include/mbx_vote.h, for its own entry points and for the voted steps of mbx_api.hip (the caller has
// made the refusals, T > 0, and has the plan's device current)
int vote_select_launch(const mbx_vote_plan* plan, int T, const mbx_param_record* d_cand, const uint8_t* d_present, mbx_param_record* d_records,
                       mbx_vote_record* d_votes, void* stream);
int vote_combine_launch(const mbx_vote_plan* plan, int row_cells, int T, const mbe_soft_bit* d_cand, const uint8_t* d_present, mbe_soft_bit* d_soft,
                        mbx_vote_record* d_votes, void* stream);

static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// an argument is refused: "<who>: <why>", MBE_STATUS_INVALID_ARGUMENT
static inline int refuse(const char* who, const char* why) {
    char text[240];
    snprintf(text, sizeof(text), "%s: %s", who, why);
    mbx_set_error_text(text);
    return MBE_STATUS_INVALID_ARGUMENT;
}

// a HIP call failed: "<prefix><what>: <HIP's text>", MBX_ENODEVICE
static inline int hip_failed(const char* prefix, const char* what, hipError_t e) {
    char text[256];
    snprintf(text, sizeof(text), "%s%s: %s", prefix, what, hipGetErrorString(e));
    mbx_set_error_text(text);
    return MBX_ENODEVICE;
}

// a pointer below the alignment its kind has in `header`'s Alignment table: refused before anything is launched
static inline int misaligned(const char* who, const char* header) {
    char text[200];
    snprintf(text, sizeof(text), "%s: a pointer is below the alignment of its kind (include/%s, Alignment)", who, header);
    mbx_set_error_text(text);
    return MBE_STATUS_INVALID_ARGUMENT;
}

// the current device, after mbx_init() for it
static inline int ready_device(int* dev) {
    const hipError_t e = hipGetDevice(dev);
    if (e != hipSuccess) {
        return hip_failed("", "hipGetDevice", e);
    }
    if (!mbx_device_ready(*dev)) {
        mbx_set_error_text("mbx_init() has not been called for the current device");
        return MBX_ENOTINIT;
    }
    return 0;
}

}  // namespace mbx
