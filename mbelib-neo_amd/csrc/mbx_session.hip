// mbx_session.hip -- the fan-in path of libmbx_hip.so: a session keeps the model state of S streams RESIDENT on the
// device and takes batches of wire frames from HOST memory, returning PCM to HOST memory (include/mbx.h, "sessions").
//
// What crosses PCIe per 20 ms frame is the wire frame in (18 B / 9 B) and the PCM out (320 B int16, + 20 B when the
// mbe_process_result is asked for; 160 B where the host takes G.711 bytes, include/mbx_pcm8.h: one compand launch behind the step;
// a few bus rows in place of them all where the host takes talkgroup buses, include/mbx_mixdown.h: the mix-down launches behind the step;
// 16 B where it takes level records, include/mbx_levels.h: the levels launch behind the step, in front of a gated mix-down)
// -- not the 15.6 KB of state the per-call conveniences (mbx_process_batch_host) move.
//
// Pipeline: kDepth slots of device buffers, two HIP streams.  Batch k uses slot k % kDepth:
//     compute stream   stage-in kernel (frames(k) read from pinned host memory), FEC + stream kernels -> event comp(k)
//     copy-out stream  wait comp(k); D2H PCM / results (DMA)                                          -> event done(k)
// Batches run in submission order (the state of batch k+1 depends on batch k); kernels(k+1) overlap D2H(k).  The frames
// are NOT brought in by a DMA copy: on this stack a host-to-device copy of batch k+1 queues behind the device-to-host copy
// of batch k on the copy engine, which put the next batch's kernels behind that transfer (65,536 frames: 0.257 ms of
// kernels + 0.379 ms of PCM back to back = 103 M frames/s; overlapped the PCM transfer alone bounds the rate).
// The host blocks only when it is kDepth batches ahead of the device.
// Host buffers that are pinned (mbx_host_alloc / hipHostMalloc / hipHostRegister) are DMA targets as they are; pageable
// buffers are staged through pinned memory owned by the slot (one extra host memcpy each way).
//
// Host code only; every number is computed by the kernels of mbx_fec.hip / mbx_stream.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "mbx.h"
#include "mbx_burst.h"
#include "mbx_burst_groups.h"
#include "mbx_codec.h"
#include "mbx_gather.h"
#include "mbx_host.h"
#include "mbx_keystream.h"
#include <mbx_levels.h>    // (the public headers of these two names: include/ is first on the include path)
#include "mbx_levels_plan.h"   // (what a gate is refused for)
#include <mbx_hold.h>      // (the held gate: the public header)
#include "mbx_hold_plan.h"     // (what a hold is refused for, and the plan a state is tied to)
#include <mbx_mixdown.h>   // (the public header: include/ is first on the include path; "mbx_mixdown.h" would be this directory's)
#include "mbx_pcm8.h"

namespace {

constexpr int kDepth = 3;

#define S_TRY(expr)                        \
    do {                                   \
        hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) {            \
            return mbx::hip_failed("session: ", #expr, e_);       \
        }                                  \
    } while (0)

bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // an ordinary (pageable) pointer: not an error for us
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

struct CopyOut {   // a staged output still to be handed to the caller's pageable buffer
    void*       dst = nullptr;
    const void* src = nullptr;
    size_t      bytes = 0;
};

struct Slot {
    uint8_t*            d_frames = nullptr;
    mbe_soft_bit*       d_soft = nullptr;   // soft frames, allocated (as h_soft) by the slot's first soft submit
    mbx_param_record*   d_records = nullptr;
    int16_t*            d_pcm16 = nullptr;
    float*              d_pcmf = nullptr;
    mbe_process_result* d_results = nullptr;
    uint8_t*            d_pcm8 = nullptr;   // companded bytes (include/mbx_pcm8.h): a session created with MBX_SESSION_PCM8
    uint8_t*            d_mix = nullptr;    // bus rows (include/mbx_mixdown.h), max_frames of 320 B: a session created with MBX_SESSION_MIXDOWN
    mbx_row_level*      d_levels = nullptr; // level records (include/mbx_levels.h), max_frames of them: a session created with MBX_SESSION_LEVELS
    int32_t*            d_index = nullptr;
    void*               d_workspace = nullptr;
    uint8_t*            d_bursts = nullptr;   // bursts (hard or soft), grown by the burst submits that need more
    size_t              bursts_cap = 0;
    uint8_t*            d_keystream = nullptr;   // keystream rows (include/mbx_keystream.h), allocated (as h_keystream) by the slot's first keyed submit
    // pinned staging, allocated on first need
    uint8_t*            h_in = nullptr;
    uint8_t*            h_soft = nullptr;
    uint8_t*            h_bursts = nullptr;   // ... and their pinned staging
    size_t              h_bursts_cap = 0;
    uint8_t*            h_keystream = nullptr;
    int32_t*            h_index = nullptr;
    int16_t*            h_pcm16 = nullptr;
    float*              h_pcmf = nullptr;
    uint8_t*            h_pcm8 = nullptr;
    uint8_t*            h_mix = nullptr;
    mbx_row_level*      h_levels = nullptr;
    mbe_process_result* h_results = nullptr;
    mbx_param_record*   h_records = nullptr;
    hipEvent_t          comp = nullptr, done = nullptr;
    bool                busy = false;
    CopyOut             out[7];
    int                 nout = 0;
};

}  // namespace

struct mbx_session {
    int      device = -1;
    int      codec = 0;
    int      streams = 0;
    size_t   max_frames = 0;
    unsigned outputs = 0;
    size_t   frame_bytes = 0;
    size_t   soft_bytes = 0;      // one frame of mbe_soft_bit cells in the reference's shape
    mbe_parms*      d_state = nullptr;   // [streams][3]
    mbx_stream_rng* d_rng = nullptr;     // [streams]
    uint32_t*       d_resident = nullptr;   // [streams]: prev_mp_enhanced of the stream is elided (mbx_process_batch_resident, include/mbx.h)
    hipStream_t s_comp = nullptr, s_out = nullptr;
    Slot     slot[kDepth];
    unsigned long long submitted = 0;
    std::vector<uint8_t> seen;   // submit_indexed: one mark per stream, to refuse an index that names a stream twice
    std::vector<uint8_t> stream_codec;   // a MIXED session (mbx_session_create_mixed): the codec of every stream; empty: all of `codec`
    bool mixed() const { return !stream_codec.empty(); }
};

namespace {

int finish_slot(Slot& sl) {   // wait for the slot's batch and hand staged outputs over
    if (!sl.busy) {
        return 0;
    }
    S_TRY(hipEventSynchronize(sl.done));
    for (int i = 0; i < sl.nout; ++i) {
        memcpy(sl.out[i].dst, sl.out[i].src, sl.out[i].bytes);
    }
    sl.nout = 0;
    sl.busy = false;
    return 0;
}

template <class U>
int pinned(U*& p, size_t count) {
    if (!p) {
        S_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(U), hipHostMallocDefault));
    }
    return 0;
}

struct DeviceGuard {   // a session is bound to the device it was created on, whatever the caller's current device is
    int before = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&before);
        if (before != dev) {
            (void)hipSetDevice(dev);
        } else {
            before = -1;
        }
    }
    ~DeviceGuard() {
        if (before >= 0) {
            (void)hipSetDevice(before);
        }
    }
};

void default_parms(mbe_parms& p) {   // ref mbe_initMbeParms, src/core/mbelib.c:367-410 (defaults only)
    memset(&p, 0, sizeof(p));
    p.w0 = (float)((4.0 * 3.14159265358979323846) / (134.0 + 39.5));
    p.L = (int)(0.9254 * (int)((3.14159265358979323846 / p.w0) + 0.25));
    p.K = 12;
    for (int l = 0; l <= 56; ++l) {
        p.Ml[l] = 1.0f;
    }
    p.localEnergy = 75000.0f;
    p.amplitudeThreshold = 20480;
    p.mutingThreshold = MBE_MUTING_THRESHOLD_IMBE;
    p.noiseSeed = -1.0f;
}

// mbx_session_next_pcm8: where the NEXT submit of a session also delivers its PCM as companded bytes (include/mbx_pcm8.h).  The
// attachment lasts for one submit call, whether that call queues or refuses, so every public submit takes it as its first act --
// by the session's ADDRESS, out of a table beside the sessions: a submit refuses some arguments before it looks at its session, and
// must not dereference a pointer it has not checked to use the attachment up.
// mbx_session_next_mixdown (include/mbx_mixdown.h) attaches the buses of a plan in the same way, in the same record: one submit uses both up.
struct NextOut {
    uint8_t* dst = nullptr;   // host memory, rows * 160 bytes; nullptr: nothing attached
    int      law = 0;         // MBX_LAW_*
    void*                   buses = nullptr;   // host memory, the plan's buses * 160 samples of `form`; nullptr: nothing attached
    const mbx_mixdown_plan* plan = nullptr;
    int                     form = 0;          // MBX_MIXDOWN_*
    bool                    gated = false;     // the buses under `gate` (mbx_session_next_mixdown_gated, include/mbx_levels.h): the same slot, whichever call came last
    mbx_mixdown_gate        gate = {0, 0};
    mbx_gate_state*         held = nullptr;    // the buses under `hold` with this state (mbx_session_next_mixdown_held, include/mbx_hold.h): the same slot again
    mbx_mixdown_hold        hold = {0, 0, 0, 0, 0};
    mbx_row_level*          levels = nullptr;  // host memory, one record per row (mbx_session_next_levels); nullptr: nothing attached
    bool wants_levels() const { return levels || (buses && (gated || held)); }
};
std::mutex g_next_mu;
std::unordered_map<const mbx_session*, NextOut> g_next;

NextOut take_next(const mbx_session* s) {
    std::lock_guard<std::mutex> lock(g_next_mu);
    NextOut out;
    const auto it = g_next.find(s);
    if (it != g_next.end()) {
        out = it->second;
        g_next.erase(it);
    }
    return out;
}

bool range_ok(const mbx_session* s, int first, int count) {
    return s && first >= 0 && count >= 0 && (long long)first + count <= s->streams;
}

// a submit of BURSTS (include/mbx_burst.h): `frames` holds n bursts of `bytes` bytes each, T is the schedule's frames per burst
struct BurstIn {
    const mbx_burst_schedule* sched;
    size_t                    stride;   // hard bursts: the caller's burst_stride
    size_t                    bytes;    // one burst in the input: burst_stride, or mbx_burst_schedule_soft_bytes()
};

// `soft`: frames are mbe_soft_bit cells (soft_bytes per frame) instead of wire frames (frame_bytes)
int enqueue(mbx_session* s, Slot& sl, int n, int T, const int32_t* index, const void* frames, bool soft, int16_t* pcm16, float* pcmf,
            mbe_process_result* results, mbx_param_record* records, const BurstIn* burst, const uint8_t* keystream, const NextOut& next);

int copy_out(mbx_session* s, Slot& sl, size_t nf, int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records, const NextOut& next);

// behind the step of a submit of nf frames that has a destination attached: the slot's int16 rows -> its bytes, on the compute stream
int compand_step(mbx_session* s, Slot& sl, size_t nf, const NextOut& next) {
    return next.dst ? mbx_pcm_compand(next.law, sl.d_pcm16, nf, sl.d_pcm8, s->s_comp) : 0;
}

// ... the level records of those rows, once per submit, for the caller or for the gate of its buses or both
int levels_step(mbx_session* s, Slot& sl, size_t nf, const NextOut& next) {
    return next.wants_levels() ? mbx_pcm_levels(sl.d_pcm16, nf, sl.d_levels, s->s_comp) : 0;
}

// ... and the plan's buses of those rows, nf of them: one or two more launches on the compute stream
int mixdown_step(mbx_session* s, Slot& sl, size_t nf, const NextOut& next) {
    if (next.buses && next.held) {
        return mbx_mixdown_held(next.plan, &next.hold, next.held, next.form, sl.d_pcm16, nf, sl.d_levels, sl.d_mix, s->s_comp);
    }
    if (next.buses && next.gated) {
        return mbx_mixdown_gated(next.plan, &next.gate, next.form, sl.d_pcm16, nf, sl.d_levels, sl.d_mix, s->s_comp);
    }
    return next.buses ? mbx_mixdown(next.plan, next.form, sl.d_pcm16, nf, sl.d_mix, s->s_comp) : 0;
}

// a submit of `rows` rows with buses attached: every row the plan names must be among them, or nothing is queued
int refuse_rows_short_of_the_plan(const NextOut& next, size_t rows) {
    if (next.buses && rows < (size_t)mbx_mixdown_plan_rows(next.plan)) {
        char text[200];
        snprintf(text, sizeof(text), "session: the submit has %zu rows, the mix-down plan attached to it needs %d (mbx_session_next_mixdown)", rows,
                 mbx_mixdown_plan_rows(next.plan));
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return 0;
}

// a mixed session takes burst groups only
int refuse_mixed(const mbx_session* s, const char* who) {
    if (s && s->mixed()) {
        char text[160];
        snprintf(text, sizeof(text), "%s: a mixed session takes burst groups only (mbx_session_submit_burst_groups)", who);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return 0;
}

int submit(const NextOut& next, mbx_session* s, int n, int T, const int32_t* index, const void* frames, bool soft, int16_t* pcm16, float* pcmf,
           mbe_process_result* results, mbx_param_record* records, const BurstIn* burst = nullptr, const uint8_t* keystream = nullptr) {
    if (refuse_mixed(s, "mbx_session_submit") < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!s || !frames || n < 0 || T < 0 || n > s->streams || (size_t)n * (size_t)T > s->max_frames) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if ((pcm16 && !(s->outputs & MBX_SESSION_PCM16)) || (pcmf && !(s->outputs & MBX_SESSION_PCMF))
        || (results && !(s->outputs & MBX_SESSION_RESULTS))) {
        return MBE_STATUS_INVALID_ARGUMENT;   // an output the session was not created for
    }
    if (refuse_rows_short_of_the_plan(next, (size_t)n * (size_t)T) < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (n == 0 || T == 0) {
        return 0;
    }
    if (burst && mbx::burst_shape(burst->sched).llr()) {
        // every LLR is a valid one: nothing to check
    } else if (burst) {   // bursts of a form that can be invalid: a bit byte > 1, a dibit > 3, a soft hard decision > 1 (mbx_burst_validate)
        const int rc = mbx_burst_validate(burst->sched, frames, burst->stride, (size_t)n, soft ? 1 : 0);
        if (rc < 0) {
            return rc;
        }
    } else if (soft) {   // a hard decision > 1 is refused before anything is queued (ref mbe_validate_soft_bits, src/internal/mbe_result.h:31-42)
        const int rc = mbx_validate_soft_bits(static_cast<const mbe_soft_bit*>(frames), (size_t)n * (size_t)T * (s->soft_bytes / sizeof(mbe_soft_bit)));
        if (rc < 0) {
            return rc;
        }
    }
    if (index) {   // every row must name its own stream: two rows on one stream would race on its state
        s->seen.assign((size_t)s->streams, 0);
        for (int i = 0; i < n; ++i) {
            if (index[i] < 0 || index[i] >= s->streams || s->seen[(size_t)index[i]]) {
                mbx_set_error_text("session: stream index out of range or listed twice");
                return MBE_STATUS_INVALID_ARGUMENT;
            }
            s->seen[(size_t)index[i]] = 1;
        }
    }
    DeviceGuard guard(s->device);
    Slot& sl = s->slot[s->submitted % kDepth];
    int rc = finish_slot(sl);   // the batch that used this slot kDepth submissions ago
    if (rc < 0) {
        return rc;
    }
    // From here on work is queued on the three streams against this slot's buffers.  If anything fails halfway the slot is
    // NOT marked busy, so before the error goes back the streams are drained: the next submit may reuse the slot at once.
    rc = enqueue(s, sl, n, T, index, frames, soft, pcm16, pcmf, results, records, burst, keystream, next);
    if (rc < 0) {
        (void)hipStreamSynchronize(s->s_comp);
        (void)hipStreamSynchronize(s->s_out);
        (void)hipGetLastError();
        sl.nout = 0;
        return rc;
    }
    sl.busy = true;
    ++s->submitted;
    return 0;
}

int enqueue(mbx_session* s, Slot& sl, int n, int T, const int32_t* index, const void* frames, bool soft, int16_t* pcm16, float* pcmf,
            mbe_process_result* results, mbx_param_record* records, const BurstIn* burst, const uint8_t* keystream, const NextOut& next) {
    int rc = 0;
    const size_t nf = (size_t)n * (size_t)T;
    // ---- in ----
    // Soft frames are 368 / 336 / 192 B each against 18 / 9: their device buffer and their pinned staging belong to the slot's
    // first soft submit, so a session that never sees one pays for neither.  Bursts likewise: their buffers belong to the burst
    // submits and grow with them (the slot's earlier batch is finished: nothing reads the old ones).
    const size_t in_bytes = soft ? s->soft_bytes : s->frame_bytes;
    const size_t in_total = burst ? (size_t)n * burst->bytes : nf * in_bytes;
    uint8_t*& stage = burst ? sl.h_bursts : (soft ? sl.h_soft : sl.h_in);
    if (burst && sl.bursts_cap < in_total) {
        (void)hipFree(sl.d_bursts);
        sl.d_bursts = nullptr;
        sl.bursts_cap = 0;
        S_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_bursts), in_total));
        sl.bursts_cap = in_total;
    }
    if (!burst && soft && !sl.d_soft) {
        S_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_soft), s->max_frames * s->soft_bytes));
    }
    const uint8_t* src = static_cast<const uint8_t*>(frames);
    // The frames (and the stream index) are fetched by a kernel on the COMPUTE stream, not by a DMA copy: see stage_in_kernel
    // (mbx_fec.hip).  A pinned buffer that is not 16-byte aligned goes through the slot's own pinned staging like a pageable one.
    if (!is_pinned(frames) || (reinterpret_cast<uintptr_t>(src) & 15u)) {
        if (burst) {
            if (sl.h_bursts_cap < in_total) {
                (void)hipHostFree(sl.h_bursts);
                sl.h_bursts = nullptr;
                sl.h_bursts_cap = 0;
                S_TRY(hipHostMalloc(reinterpret_cast<void**>(&sl.h_bursts), in_total, hipHostMallocDefault));
                sl.h_bursts_cap = in_total;
            }
        } else {
            rc = pinned(stage, s->max_frames * in_bytes);
            if (rc < 0) {
                return rc;
            }
        }
        memcpy(stage, frames, in_total);
        src = stage;
    }
    const void* dev_view = src;   // what the GPU dereferences: the same address for hipHostMalloc memory, possibly another one for
    void* mapped = nullptr;       // memory the host registered itself (hipHostRegister)
    if (hipHostGetDevicePointer(&mapped, const_cast<uint8_t*>(src), 0) == hipSuccess && mapped) {
        dev_view = mapped;
    } else {
        (void)hipGetLastError();
    }
    void* const d_in = burst ? static_cast<void*>(sl.d_bursts) : (soft ? static_cast<void*>(sl.d_soft) : static_cast<void*>(sl.d_frames));
    rc = mbx_stage_in(d_in, dev_view, in_total, s->s_comp);
    if (rc < 0) {
        return rc;
    }
    if (index) {
        rc = pinned(sl.h_index, (size_t)s->streams);   // always staged: 4 B per stream, and the caller may reuse its array at once
        if (rc < 0) {
            return rc;
        }
        memcpy(sl.h_index, index, (size_t)n * sizeof(int32_t));
        rc = mbx_stage_in(sl.d_index, sl.h_index, (size_t)n * sizeof(int32_t), s->s_comp);
        if (rc < 0) {
            return rc;
        }
    }
    if (keystream) {   // the keystream rows take the road the frames take: pinned 16-byte aligned rows in place, others staged
        const size_t ks_total = nf * (size_t)MBX_KEYSTREAM_ROW_BYTES;
        if (!sl.d_keystream) {
            S_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_keystream), s->max_frames * (size_t)MBX_KEYSTREAM_ROW_BYTES));
        }
        const uint8_t* ks = keystream;
        if (!is_pinned(keystream) || (reinterpret_cast<uintptr_t>(ks) & 15u)) {
            rc = pinned(sl.h_keystream, s->max_frames * (size_t)MBX_KEYSTREAM_ROW_BYTES);
            if (rc < 0) {
                return rc;
            }
            memcpy(sl.h_keystream, keystream, ks_total);
            ks = sl.h_keystream;
        }
        const void* ks_view = ks;
        void* ks_mapped = nullptr;
        if (hipHostGetDevicePointer(&ks_mapped, const_cast<uint8_t*>(ks), 0) == hipSuccess && ks_mapped) {
            ks_view = ks_mapped;
        } else {
            (void)hipGetLastError();
        }
        rc = mbx_stage_in(sl.d_keystream, ks_view, ks_total, s->s_comp);
        if (rc < 0) {
            return rc;
        }
    }
    // ---- compute ----
    int16_t* d16 = pcm16 || next.dst || next.buses || next.levels ? sl.d_pcm16 : nullptr;   // (the compand, the levels and the mix-down behind the step read the int16 rows)
    float*   dfl = pcmf ? sl.d_pcmf : nullptr;
    mbe_process_result* dres = results ? sl.d_results : nullptr;
    if (keystream) {   // the keyed call takes every form: hard or soft, index or none, resident words or plain triplets
        rc = mbx_process_batch_keyed(s->codec, n, T, index ? sl.d_index : nullptr, soft ? nullptr : sl.d_frames, soft ? sl.d_soft : nullptr,
                                     sl.d_keystream, s->d_state, s->d_resident, s->d_rng, d16, dfl, dres, sl.d_records, s->s_comp);
    } else if (burst && soft) {   // the gather in front of the step the frames submits run: resident words or plain triplets, index or none
        rc = mbx_process_bursts_soft(burst->sched, n, index ? sl.d_index : nullptr, reinterpret_cast<const mbe_soft_bit*>(sl.d_bursts), s->d_state,
                                     s->d_resident, s->d_rng, d16, dfl, dres, sl.d_records, s->s_comp);
    } else if (burst) {
        rc = mbx_process_bursts(burst->sched, n, index ? sl.d_index : nullptr, sl.d_bursts, burst->stride, s->d_state, s->d_resident, s->d_rng, d16,
                                dfl, dres, sl.d_records, s->s_comp);
    } else if (soft) {   // the soft twin of the resident launcher takes every form: index or none, resident words or plain triplets
        rc = mbx_process_batch_soft_resident(s->codec, n, T, index ? sl.d_index : nullptr, sl.d_soft, s->d_state, s->d_resident, s->d_rng,
                                             d16, dfl, dres, sl.d_records, s->s_comp);
    } else if (s->d_resident) {   // the session owns the state between submits: the resident form (no prev_mp_enhanced traffic, lazy prev_mp)
        rc = mbx_process_batch_resident(s->codec, n, T, index ? sl.d_index : nullptr, sl.d_frames, s->d_state, s->d_resident, s->d_rng,
                                        d16, dfl, dres, sl.d_records, s->s_comp);
    } else if (index) {
        rc = mbx_process_batch_indexed(s->codec, n, T, sl.d_index, sl.d_frames, s->d_state, s->d_rng, d16, dfl, dres, sl.d_records,
                                       s->s_comp);
    } else {
        rc = mbx_process_batch_ws(s->codec, n, T, sl.d_frames, s->d_state, s->d_rng, d16, dfl, dres, sl.d_records, sl.d_workspace,
                                  mbx_workspace_bytes(s->max_frames), s->s_comp);
    }
    if (rc < 0 || (rc = compand_step(s, sl, nf, next)) < 0 || (rc = levels_step(s, sl, nf, next)) < 0 || (rc = mixdown_step(s, sl, nf, next)) < 0) {
        return rc;
    }
    return copy_out(s, sl, nf, pcm16, pcmf, results, records, next);
}

// ---- out ----: behind the compute stream's launches of a submit of nf frames, the outputs to the caller (or to the slot's staging)
int copy_out(mbx_session* s, Slot& sl, size_t nf, int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records, const NextOut& next) {
    int rc = 0;
    S_TRY(hipEventRecord(sl.comp, s->s_comp));
    S_TRY(hipStreamWaitEvent(s->s_out, sl.comp, 0));
    sl.nout = 0;
    // per_frame elements of *stage per row (the staging, made on first need, holds most_per_frame); rows: nf, but the buses of a mix-down
    // plan (at most max_frames of them)
    auto out = [&](void* user, const void* dev, auto*& stage, size_t per_frame, size_t rows, size_t most_per_frame) -> int {
        if (!user) {
            return 0;
        }
        const size_t bytes = rows * per_frame * sizeof(*stage);
        void* dst = user;
        if (!is_pinned(user)) {
            int r = pinned(stage, s->max_frames * most_per_frame);
            if (r < 0) {
                return r;
            }
            dst = stage;
            sl.out[sl.nout++] = CopyOut{user, stage, bytes};
        }
        hipError_t e = hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, s->s_out);
        return e == hipSuccess ? 0 : mbx::hip_failed("session: ", "hipMemcpyAsync (device to host)", e);
    };
    const size_t buses = next.buses ? (size_t)mbx_mixdown_plan_buses(next.plan) : 0;
    if ((rc = out(pcm16, sl.d_pcm16, sl.h_pcm16, 160, nf, 160)) < 0 || (rc = out(pcmf, sl.d_pcmf, sl.h_pcmf, 160, nf, 160)) < 0
        || (rc = out(results, sl.d_results, sl.h_results, 1, nf, 1)) < 0 || (rc = out(records, sl.d_records, sl.h_records, 1, nf, 1)) < 0
        || (rc = out(next.dst, sl.d_pcm8, sl.h_pcm8, 160, nf, 160)) < 0
        || (rc = out(next.buses, sl.d_mix, sl.h_mix, next.form == MBX_MIXDOWN_PCM16 ? 320 : 160, buses, 320)) < 0
        || (rc = out(next.levels, sl.d_levels, sl.h_levels, 1, nf, 1)) < 0) {
        return rc;
    }
    S_TRY(hipEventRecord(sl.done, s->s_out));
    return 0;
}

}  // namespace

extern "C" {

void* mbx_host_alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void mbx_host_free(void* p) {
    if (p) {
        (void)hipHostFree(p);
    }
}

// (stream_codec: a mixed session -- `codec` is then none (-1), and the slot buffers are sized for mixed rows)
static int create_session(mbx_session** out, int codec, const uint8_t* stream_codec, int streams, size_t max_frames_per_submit, unsigned outputs) {
    const mbx::CodecShape* shape = mbx::codec_shape(codec);
    if (!out || streams <= 0 || max_frames_per_submit == 0 || (!shape && !stream_codec)
        || (outputs & ~(MBX_SESSION_PCM16 | MBX_SESSION_PCMF | MBX_SESSION_RESULTS | MBX_SESSION_PCM8 | MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS)) != 0u) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    for (int i = 0; stream_codec && i < streams; ++i) {
        if (!mbx::codec_shape(stream_codec[i])) {
            mbx_set_error_text("mbx_session_create_mixed: a stream_codec byte is not one of MBX_CODEC_*");
            return MBE_STATUS_INVALID_ARGUMENT;
        }
    }
    int dev = -1;
    S_TRY(hipGetDevice(&dev));
    if (!mbx_device_ready(dev)) {
        mbx_set_error_text("mbx_session_create: mbx_init() has not been called for the current device");
        return MBX_ENOTINIT;
    }
    mbx_session* s = new (std::nothrow) mbx_session();
    if (!s) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    s->device = dev;
    s->codec = codec;
    s->streams = streams;
    s->max_frames = max_frames_per_submit;
    s->outputs = outputs ? outputs : MBX_SESSION_PCM16;
    s->frame_bytes = stream_codec ? (size_t)MBX_MIXED_ROW_BYTES : (size_t)shape->frame_bytes;
    s->soft_bytes = sizeof(mbe_soft_bit) * (stream_codec ? (size_t)MBX_MIXED_ROW_CELLS : (size_t)shape->cells);
    if (stream_codec) {
        s->stream_codec.assign(stream_codec, stream_codec + streams);
    }
    *out = s;
    auto bail = [&](int rc) {
        mbx_session_destroy(s);
        *out = nullptr;
        return rc;
    };
#define C_TRY(expr)                          \
    do {                                     \
        hipError_t e_ = (expr);              \
        if (e_ != hipSuccess) {              \
            return bail(mbx::hip_failed("session: ", #expr, e_));   \
        }                                    \
    } while (0)
    C_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_state), (size_t)streams * 3 * sizeof(mbe_parms)));
    C_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_rng), (size_t)streams * sizeof(mbx_stream_rng)));
    if (!getenv("MBX_SESSION_ABI_STATE")) {   // (development switch: keep the ABI triplets whole after every submit, for A/B timing)
        C_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_resident), (size_t)streams * sizeof(uint32_t)));
        C_TRY(hipMemset(s->d_resident, 0, (size_t)streams * sizeof(uint32_t)));
    }
    C_TRY(hipStreamCreateWithFlags(&s->s_comp, hipStreamNonBlocking));
    C_TRY(hipStreamCreateWithFlags(&s->s_out, hipStreamNonBlocking));
    const size_t mf = s->max_frames;
    for (Slot& sl : s->slot) {
        C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_frames), mf * s->frame_bytes));
        C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_records), mf * sizeof(mbx_param_record)));
        C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_index), (size_t)streams * sizeof(int32_t)));
        if (!s->d_resident) {   // (the resident entry point uses the workspace the launcher keeps for the compute stream, reserved below)
            C_TRY(hipMalloc(&sl.d_workspace, mbx_workspace_bytes(mf)));
        }
        if (s->outputs & (MBX_SESSION_PCM16 | MBX_SESSION_PCM8 | MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS)) {   // (the step writes int16; the compand, the mix-down and the levels read it)
            C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_pcm16), mf * 160 * sizeof(int16_t)));
        }
        if (s->outputs & MBX_SESSION_PCM8) {
            C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_pcm8), mf * 160));
        }
        if (s->outputs & MBX_SESSION_MIXDOWN) {
            C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_mix), mf * 160 * sizeof(int16_t)));
        }
        if (s->outputs & MBX_SESSION_LEVELS) {
            C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_levels), mf * sizeof(mbx_row_level)));
        }
        if (s->outputs & MBX_SESSION_PCMF) {
            C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_pcmf), mf * 160 * sizeof(float)));
        }
        if (s->outputs & MBX_SESSION_RESULTS) {
            C_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_results), mf * sizeof(mbe_process_result)));
        }
        C_TRY(hipEventCreateWithFlags(&sl.comp, hipEventDisableTiming));
        // (a blocking wait -- hipEventBlockingSync -- was measured here and costs more than it saves: the wake-up latency of every
        // submit that has to wait is exposed, 155 -> 113 M frames/s with two session threads, 117 -> 78 M with four)
        C_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
#undef C_TRY
    // the indexed launches size the compute stream's own workspace once, here, not in the first submit
    int rc = mbx_reserve_stream(s->s_comp, mf);
    if (rc < 0) {
        return bail(rc);
    }
    rc = mbx_session_reset(s, 0, streams);
    return rc < 0 ? bail(rc) : 0;
}

int mbx_session_create(mbx_session** out, int codec, int streams, size_t max_frames_per_submit, unsigned outputs) {
    return create_session(out, codec, nullptr, streams, max_frames_per_submit, outputs);
}

int mbx_session_create_mixed(mbx_session** out, int streams, const uint8_t* stream_codec, size_t max_frames_per_submit, unsigned outputs) {
    if (!stream_codec) {
        mbx_set_error_text("mbx_session_create_mixed: stream_codec is NULL");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return create_session(out, -1, stream_codec, streams, max_frames_per_submit, outputs);
}

int mbx_session_destroy(mbx_session* s) {
    if (!s) {
        return 0;
    }
    (void)take_next(s);   // (an attachment no submit used)
    DeviceGuard guard(s->device);
    if (s->s_comp) {
        (void)hipStreamSynchronize(s->s_comp);
        (void)mbx_release_stream(s->s_comp);
    }
    if (s->s_out) {
        (void)hipStreamSynchronize(s->s_out);
    }
    for (Slot& sl : s->slot) {
        (void)hipFree(sl.d_frames);
        (void)hipFree(sl.d_soft);
        (void)hipFree(sl.d_records);
        (void)hipFree(sl.d_pcm16);
        (void)hipFree(sl.d_pcmf);
        (void)hipFree(sl.d_results);
        (void)hipFree(sl.d_pcm8);
        (void)hipFree(sl.d_mix);
        (void)hipFree(sl.d_levels);
        (void)hipFree(sl.d_index);
        (void)hipFree(sl.d_workspace);
        (void)hipFree(sl.d_bursts);
        (void)hipFree(sl.d_keystream);
        (void)hipHostFree(sl.h_keystream);
        (void)hipHostFree(sl.h_bursts);
        (void)hipHostFree(sl.h_in);
        (void)hipHostFree(sl.h_soft);
        (void)hipHostFree(sl.h_index);
        (void)hipHostFree(sl.h_pcm16);
        (void)hipHostFree(sl.h_pcmf);
        (void)hipHostFree(sl.h_pcm8);
        (void)hipHostFree(sl.h_mix);
        (void)hipHostFree(sl.h_levels);
        (void)hipHostFree(sl.h_results);
        (void)hipHostFree(sl.h_records);
        if (sl.comp) {
            (void)hipEventDestroy(sl.comp);
        }
        if (sl.done) {
            (void)hipEventDestroy(sl.done);
        }
    }
    (void)hipFree(s->d_state);
    (void)hipFree(s->d_resident);
    (void)hipFree(s->d_rng);
    if (s->s_comp) {
        (void)hipStreamDestroy(s->s_comp);
    }
    if (s->s_out) {
        (void)hipStreamDestroy(s->s_out);
    }
    (void)hipGetLastError();
    delete s;
    return 0;
}

int mbx_session_streams(const mbx_session* s) { return s ? s->streams : 0; }

int mbx_session_wait(mbx_session* s) {
    if (!s) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    DeviceGuard guard(s->device);
    for (int i = 0; i < kDepth; ++i) {   // oldest first: staged outputs are handed over in submission order
        int rc = finish_slot(s->slot[(s->submitted + i) % kDepth]);
        if (rc < 0) {
            return rc;
        }
    }
    return 0;
}

int mbx_session_set_state(mbx_session* s, int first, int count, const mbe_parms* state, const mbx_stream_rng* rng) {
    if (!range_ok(s, first, count) || (!state && !rng)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = mbx_session_wait(s);
    if (rc < 0) {
        return rc;
    }
    DeviceGuard guard(s->device);
    S_TRY(hipStreamSynchronize(s->s_comp));   // (a submit that failed halfway leaves no busy slot to wait on)
    if (state) {
        S_TRY(hipMemcpy(s->d_state + 3 * (size_t)first, state, (size_t)count * 3 * sizeof(mbe_parms), hipMemcpyHostToDevice));
        if (s->d_resident) {   // the caller's triplets are whole: nothing is elided any more
            // On the compute stream, not the null stream: s_comp is non-blocking, so a null-stream memset is not ordered in front of the
            // next submit's launches (the workspace flags of mbx_api.hip, same reasoning).  By the API's contract; no race was observed.
            S_TRY(hipMemsetAsync(s->d_resident + first, 0, (size_t)count * sizeof(uint32_t), s->s_comp));
        }
    }
    if (rng) {
        S_TRY(hipMemcpy(s->d_rng + first, rng, (size_t)count * sizeof(mbx_stream_rng), hipMemcpyHostToDevice));
    }
    return 0;
}

int mbx_session_get_state(mbx_session* s, int first, int count, mbe_parms* state, mbx_stream_rng* rng) {
    if (!range_ok(s, first, count) || (!state && !rng)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = mbx_session_wait(s);
    if (rc < 0) {
        return rc;
    }
    DeviceGuard guard(s->device);
    S_TRY(hipStreamSynchronize(s->s_comp));
    if (state) {
        if (s->d_resident) {   // write the elided prev_mp_enhanced structs out: the triplets leave in their ABI form
            rc = mbx_resident_materialize(count, nullptr, s->d_state + 3 * (size_t)first, s->d_resident + first, s->s_comp);
            if (rc < 0) {
                return rc;
            }
            S_TRY(hipStreamSynchronize(s->s_comp));
        }
        S_TRY(hipMemcpy(state, s->d_state + 3 * (size_t)first, (size_t)count * 3 * sizeof(mbe_parms), hipMemcpyDeviceToHost));
    }
    if (rng) {
        S_TRY(hipMemcpy(rng, s->d_rng + first, (size_t)count * sizeof(mbx_stream_rng), hipMemcpyDeviceToHost));
    }
    return 0;
}

int mbx_session_reset(mbx_session* s, int first, int count) {
    if (!range_ok(s, first, count)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (count == 0) {
        return 0;
    }
    mbe_parms p;
    default_parms(p);
    std::vector<mbe_parms> st((size_t)count * 3, p);
    std::vector<mbx_stream_rng> rg((size_t)count);
    for (auto& r : rg) {
        mbx_rng_default(&r);
    }
    return mbx_session_set_state(s, first, count, st.data(), rg.data());
}

int mbx_session_seed(mbx_session* s, int first, int count, const uint32_t* seeds) {
    if (!range_ok(s, first, count) || !seeds) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (count == 0) {   // (as reset: an empty vector's data() is NULL, which set_state refuses)
        return 0;
    }
    std::vector<mbx_stream_rng> rg((size_t)count);
    for (int i = 0; i < count; ++i) {
        mbx_rng_default(&rg[(size_t)i]);
        mbx_rng_seed(&rg[(size_t)i], seeds[i]);
    }
    return mbx_session_set_state(s, first, count, nullptr, rg.data());
}

int mbx_session_submit(mbx_session* s, int T, const uint8_t* frames, int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    return submit(take_next(s), s, s ? s->streams : 0, T, nullptr, frames, false, pcm16, pcmf, results, nullptr);
}

int mbx_session_submit_indexed(mbx_session* s, int n, int T, const int32_t* stream_index, const uint8_t* frames, int16_t* pcm16,
                               float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    const NextOut next = take_next(s);
    if (!stream_index) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return submit(next, s, n, T, stream_index, frames, false, pcm16, pcmf, results, records);
}

int mbx_session_submit_soft(mbx_session* s, int T, const mbe_soft_bit* soft, int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    return submit(take_next(s), s, s ? s->streams : 0, T, nullptr, soft, true, pcm16, pcmf, results, nullptr);
}

int mbx_session_submit_soft_indexed(mbx_session* s, int n, int T, const int32_t* stream_index, const mbe_soft_bit* soft, int16_t* pcm16,
                                    float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    const NextOut next = take_next(s);
    if (!stream_index) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return submit(next, s, n, T, stream_index, soft, true, pcm16, pcmf, results, records);
}

// ---- companded bytes out (include/mbx_pcm8.h): the destination of the next submit ----------------------------------------------------
int mbx_session_next_pcm8(mbx_session* s, int law, uint8_t* pcm8) {
    if (!s) {
        mbx_set_error_text("mbx_session_next_pcm8: no session");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!pcm8) {
        std::lock_guard<std::mutex> lock(g_next_mu);
        const auto it = g_next.find(s);
        if (it != g_next.end()) {
            it->second.dst = nullptr;   // (buses attached beside it stay)
        }
        return 0;
    }
    if (!(s->outputs & MBX_SESSION_PCM8)) {
        mbx_set_error_text("mbx_session_next_pcm8: the session was created without MBX_SESSION_PCM8");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (law != MBX_LAW_ULAW && law != MBX_LAW_ALAW) {
        mbx_set_error_text("mbx_session_next_pcm8: law is MBX_LAW_ULAW or MBX_LAW_ALAW");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    std::lock_guard<std::mutex> lock(g_next_mu);
    NextOut& next = g_next[s];
    next.dst = pcm8;
    next.law = law;
    return 0;
}

// ---- mix-down out (include/mbx_mixdown.h): the buses of the next submit -----------------------------------------------------------------
// (gate: the gated call of include/mbx_levels.h, which shares the buses slot of the record; nullptr: mbx_session_next_mixdown itself.
// held: the held call of include/mbx_hold.h, the same slot again, with its hold and its state)
static int next_mixdown(const char* who, mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_gate* gate, bool gated, void* out,
                        bool held = false, const mbx_mixdown_hold* hold = nullptr, mbx_gate_state* state = nullptr) {
    const auto refused = [who](const char* why) {
        char text[200];
        snprintf(text, sizeof(text), "%s: %s", who, why);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    };
    if (!s) {
        return refused("no session");
    }
    if (!out) {
        std::lock_guard<std::mutex> lock(g_next_mu);
        const auto it = g_next.find(s);
        if (it != g_next.end()) {
            it->second.buses = nullptr;   // (bytes attached beside it stay)
        }
        return 0;
    }
    if (!(s->outputs & MBX_SESSION_MIXDOWN)) {
        return refused("the session was created without MBX_SESSION_MIXDOWN");
    }
    if ((gated || held) && !(s->outputs & MBX_SESSION_LEVELS)) {
        return refused("the session was created without MBX_SESSION_LEVELS");
    }
    if (!plan) {
        return refused("no plan");
    }
    if (gated) {
        const mbx::LevelsRefusal why = mbx::gate_refused(gate != nullptr, gate ? gate->open_peak : 0u, gate ? gate->loudest_n : 0u);
        if (why != mbx::kLevelsOk) {
            return refused(mbx::levels_refusal_text(why));
        }
    }
    if (held) {
        mbx::HoldRefusal why = mbx::hold_refused(hold != nullptr, hold ? hold->open_peak : 0u, hold ? hold->close_peak : 0u, hold ? hold->loudest_n : 0u,
                                                 hold ? hold->ramp_log2 : 0u);
        if (why == mbx::kHoldOk) {
            why = mbx::hold_state_refused(state != nullptr, state ? state->plan : nullptr, plan);
        }
        if (why != mbx::kHoldOk) {
            return refused(mbx::hold_refusal_text(why));
        }
    }
    if (form != MBX_MIXDOWN_PCM16 && form != MBX_MIXDOWN_ULAW && form != MBX_MIXDOWN_ALAW) {
        return refused("form is MBX_MIXDOWN_PCM16, MBX_MIXDOWN_ULAW or MBX_MIXDOWN_ALAW");
    }
    if ((size_t)mbx_mixdown_plan_buses(plan) > s->max_frames) {
        return refused("the plan has more buses than max_frames_per_submit");
    }
    if (mbx::mixdown_plan_device(plan) != s->device) {
        return refused("a plan of another device than the session");
    }
    std::lock_guard<std::mutex> lock(g_next_mu);
    NextOut& next = g_next[s];
    next.buses = out;
    next.plan = plan;
    next.form = form;
    next.gated = gated;
    next.gate = gated ? *gate : mbx_mixdown_gate{0, 0};
    next.held = held ? state : nullptr;
    next.hold = held ? *hold : mbx_mixdown_hold{0, 0, 0, 0, 0};
    return 0;
}

int mbx_session_next_mixdown(mbx_session* s, const mbx_mixdown_plan* plan, int form, void* out) {
    return next_mixdown("mbx_session_next_mixdown", s, plan, form, nullptr, false, out);
}

// ---- levels out and the gated mix-down (include/mbx_levels.h): the records and the gated buses of the next submit ------------------------
int mbx_session_next_mixdown_gated(mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_gate* gate, void* out) {
    return next_mixdown("mbx_session_next_mixdown_gated", s, plan, form, gate, true, out);
}

// ---- the held gate (include/mbx_hold.h): the buses of the next submit under a hold, the caller's state advanced by one frame ------------
int mbx_session_next_mixdown_held(mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_hold* hold, mbx_gate_state* state, void* out) {
    return next_mixdown("mbx_session_next_mixdown_held", s, plan, form, nullptr, false, out, true, hold, state);
}

int mbx_session_next_levels(mbx_session* s, mbx_row_level* out) {
    if (!s) {
        mbx_set_error_text("mbx_session_next_levels: no session");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!out) {
        std::lock_guard<std::mutex> lock(g_next_mu);
        const auto it = g_next.find(s);
        if (it != g_next.end()) {
            it->second.levels = nullptr;   // (bytes and buses attached beside it stay)
        }
        return 0;
    }
    if (!(s->outputs & MBX_SESSION_LEVELS)) {
        mbx_set_error_text("mbx_session_next_levels: the session was created without MBX_SESSION_LEVELS");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    std::lock_guard<std::mutex> lock(g_next_mu);
    g_next[s].levels = out;
    return 0;
}

// ---- keyed submits (include/mbx_keystream.h): a frames submit of either kind with a keystream row per frame ---------------------------
int mbx_session_submit_keyed(mbx_session* s, int n, int T, const int32_t* stream_index, const uint8_t* frames, const mbe_soft_bit* soft,
                             const uint8_t* keystream, int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    const NextOut next = take_next(s);
    if (refuse_mixed(s, "mbx_session_submit_keyed") < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!s || (frames != nullptr) == (soft != nullptr) || (!stream_index && n != s->streams)) {
        mbx_set_error_text("mbx_session_submit_keyed: a session, exactly one of frames and soft, and without an index n = the session's stream count");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return submit(next, s, n, T, stream_index, soft ? static_cast<const void*>(soft) : frames, soft != nullptr, pcm16, pcmf, results, records, nullptr, keystream);
}

// ---- burst submits (include/mbx_burst.h) ---------------------------------------------------------------------------------------------
static int submit_bursts(const char* who, mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index, const void* bursts,
                         size_t burst_stride, bool soft, int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    const NextOut next = take_next(s);
    char text[160];
    if (!s || !sched || !bursts || n < 0 || refuse_mixed(s, who) < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const mbx::BurstShape sh = mbx::burst_shape(sched);
    if (sh.codec != s->codec || sh.device != s->device) {
        snprintf(text, sizeof(text), "%s: the schedule is of another codec or device than the session", who);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!soft && sh.llr()) {
        snprintf(text, sizeof(text), "%s: an LLR schedule has soft bursts only", who);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!soft && burst_stride < sh.bytes) {
        snprintf(text, sizeof(text), "%s: burst_stride is below mbx_burst_schedule_bytes()", who);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if ((!stream_index && n != s->streams) || (size_t)n * (size_t)sh.frames > s->max_frames) {
        snprintf(text, sizeof(text), "%s: without an index n is the session's stream count; n * frames_per_burst <= max_frames_per_submit", who);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const BurstIn in{sched, burst_stride, soft ? mbx_burst_schedule_soft_bytes(sched) : burst_stride};
    return submit(next, s, n, sh.frames, stream_index, bursts, soft, pcm16, pcmf, results, nullptr, &in);
}

int mbx_session_submit_bursts(mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index, const uint8_t* bursts,
                              size_t burst_stride, int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    return submit_bursts("mbx_session_submit_bursts", s, sched, n, stream_index, bursts, burst_stride, false, pcm16, pcmf, results);
}

int mbx_session_submit_bursts_soft(mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index, const mbe_soft_bit* soft,
                                   int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    return submit_bursts("mbx_session_submit_bursts_soft", s, sched, n, stream_index, soft, 0, true, pcm16, pcmf, results);
}

// ---- burst groups (include/mbx_burst_groups.h) --------------------------------------------------------------------------------------
// The groups' bursts into the slot's burst buffer, each group at a 16-byte aligned offset (pinned 16-byte aligned buffers read in
// place, others through the slot's pinned staging at the same offsets), their indices into the slot's index words, then
// mbx_process_burst_groups on the compute stream with the groups rewritten to those device addresses, and the outputs out.
static int enqueue_groups(mbx_session* s, Slot& sl, const mbx_burst_group* groups, int n_groups, bool soft, const mbx::GroupPlan& gp,
                          int16_t* pcm16, float* pcmf, mbe_process_result* results, const NextOut& next) {
    size_t at[MBX_BURST_MAX_GROUPS], bytes[MBX_BURST_MAX_GROUPS], total = 0;
    bool staged = false, indexed = false;
    for (int i = 0; i < n_groups; ++i) {
        const size_t per = soft ? mbx_burst_schedule_soft_bytes(groups[i].sched) : groups[i].burst_stride;
        at[i] = total;
        // (of the last hard burst only the schedule's bytes are there to read, not its whole stride)
        bytes[i] = gp.place[i].bursts ? ((size_t)gp.place[i].bursts - 1) * per + (soft ? per : mbx_burst_schedule_bytes(groups[i].sched)) : 0;
        total = (total + bytes[i] + 15) & ~(size_t)15;
        if (bytes[i] && (!is_pinned(groups[i].bursts) || (reinterpret_cast<uintptr_t>(groups[i].bursts) & 15u))) {
            staged = true;
        }
        indexed = indexed || (gp.place[i].bursts && groups[i].stream_index);
    }
    if (sl.bursts_cap < total) {
        (void)hipFree(sl.d_bursts);
        sl.d_bursts = nullptr;
        sl.bursts_cap = 0;
        S_TRY(hipMalloc(reinterpret_cast<void**>(&sl.d_bursts), total));
        sl.bursts_cap = total;
    }
    if (staged && sl.h_bursts_cap < total) {
        (void)hipHostFree(sl.h_bursts);
        sl.h_bursts = nullptr;
        sl.h_bursts_cap = 0;
        S_TRY(hipHostMalloc(reinterpret_cast<void**>(&sl.h_bursts), total, hipHostMallocDefault));
        sl.h_bursts_cap = total;
    }
    int rc = 0;
    if (indexed) {
        rc = pinned(sl.h_index, (size_t)s->streams);
        if (rc < 0) {
            return rc;
        }
    }
    mbx_burst_group dev[MBX_BURST_MAX_GROUPS];
    for (int i = 0; i < n_groups; ++i) {
        dev[i] = groups[i];
        dev[i].bursts = sl.d_bursts + at[i];
        dev[i].stream_index = nullptr;
        if (!bytes[i]) {
            continue;
        }
        const uint8_t* src = static_cast<const uint8_t*>(groups[i].bursts);
        if (!is_pinned(src) || (reinterpret_cast<uintptr_t>(src) & 15u)) {
            memcpy(sl.h_bursts + at[i], src, bytes[i]);
            src = sl.h_bursts + at[i];
        }
        const void* dev_view = src;
        void* mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, const_cast<uint8_t*>(src), 0) == hipSuccess && mapped) {
            dev_view = mapped;
        } else {
            (void)hipGetLastError();
        }
        rc = mbx_stage_in(sl.d_bursts + at[i], dev_view, bytes[i], s->s_comp);
        if (rc < 0) {
            return rc;
        }
        if (groups[i].stream_index) {   // (the groups name every stream once: their indices fit the slot's `streams` words, at their stream rows)
            memcpy(sl.h_index + gp.place[i].first_stream, groups[i].stream_index, (size_t)groups[i].n_streams * sizeof(int32_t));
            dev[i].stream_index = sl.d_index + gp.place[i].first_stream;
        }
    }
    if (indexed) {
        rc = mbx_stage_in(sl.d_index, sl.h_index, (size_t)gp.total_streams * sizeof(int32_t), s->s_comp);
        if (rc < 0) {
            return rc;
        }
    }
    rc = mbx_process_burst_groups(dev, n_groups, soft ? 1 : 0, s->d_state, s->d_resident, s->d_rng, pcm16 || next.dst || next.buses || next.levels ? sl.d_pcm16 : nullptr,
                                  pcmf ? sl.d_pcmf : nullptr, results ? sl.d_results : nullptr, sl.d_records, s->s_comp);
    if (rc < 0 || (rc = compand_step(s, sl, (size_t)gp.total_rows, next)) < 0 || (rc = levels_step(s, sl, (size_t)gp.total_rows, next)) < 0
        || (rc = mixdown_step(s, sl, (size_t)gp.total_rows, next)) < 0) {
        return rc;
    }
    return copy_out(s, sl, (size_t)gp.total_rows, pcm16, pcmf, results, nullptr, next);
}

int mbx_session_submit_burst_groups(mbx_session* s, const mbx_burst_group* groups, int n_groups, int soft_in, int16_t* pcm16, float* pcmf,
                                    mbe_process_result* results) {
    const char* const who = "mbx_session_submit_burst_groups";
    const NextOut next = take_next(s);
    const bool soft = soft_in != 0;
    char text[200];
    const auto refused = [&](const char* why) {
        snprintf(text, sizeof(text), "%s: %s", who, why);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    };
    if (!s) {
        return refused("no session");
    }
    mbx::GroupShape shapes[MBX_BURST_MAX_GROUPS];
    mbx::GroupPlan gp;
    int rc = mbx::burst_groups_plan(who, groups, n_groups, soft, shapes, &gp);
    if (rc < 0) {
        return rc;
    }
    if ((pcm16 && !(s->outputs & MBX_SESSION_PCM16)) || (pcmf && !(s->outputs & MBX_SESSION_PCMF)) || (results && !(s->outputs & MBX_SESSION_RESULTS))) {
        return refused("an output the session was not created for");
    }
    if ((size_t)gp.total_rows > s->max_frames) {
        return refused("more frames than max_frames_per_submit");
    }
    if (refuse_rows_short_of_the_plan(next, (size_t)gp.total_rows) < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    // every group's schedule is of the codec of every stream the group names; slots in range, none named twice across the groups
    s->seen.assign((size_t)s->streams, 0);
    for (int i = 0; i < n_groups; ++i) {
        const mbx_burst_group& g = groups[i];
        const mbx::BurstShape sh = mbx::burst_shape(g.sched);
        if (sh.device != s->device) {
            return refused("a schedule of another device than the session");
        }
        for (int j = 0; j < g.n_streams; ++j) {
            const long long slot = g.stream_index ? (long long)g.stream_index[j] : (long long)g.first_slot + j;
            if (slot < 0 || slot >= s->streams || s->seen[(size_t)slot]) {
                return refused("stream index out of range or listed twice");
            }
            s->seen[(size_t)slot] = 1;
            if ((s->mixed() ? (int)s->stream_codec[(size_t)slot] : s->codec) != sh.codec) {
                return refused("a schedule of another codec than a stream its group names");
            }
        }
    }
    for (int i = 0; i < n_groups; ++i) {   // bursts of a form that can be invalid (mbx_burst_validate)
        if (gp.place[i].bursts && !mbx::burst_shape(groups[i].sched).llr()) {
            rc = mbx_burst_validate(groups[i].sched, groups[i].bursts, groups[i].burst_stride, (size_t)gp.place[i].bursts, soft ? 1 : 0);
            if (rc < 0) {
                return rc;
            }
        }
    }
    if (gp.total_rows == 0) {
        return 0;
    }
    DeviceGuard guard(s->device);
    Slot& sl = s->slot[s->submitted % kDepth];
    rc = finish_slot(sl);
    if (rc < 0) {
        return rc;
    }
    rc = enqueue_groups(s, sl, groups, n_groups, soft, gp, pcm16, pcmf, results, next);
    if (rc < 0) {   // (as submit: drain, so that the next submit may reuse the slot at once)
        (void)hipStreamSynchronize(s->s_comp);
        (void)hipStreamSynchronize(s->s_out);
        (void)hipGetLastError();
        sl.nout = 0;
        return rc;
    }
    sl.busy = true;
    ++s->submitted;
    return 0;
}

}  // extern "C"
