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
// Host code only; every number is computed by the kernels of mbx_fec.hip / mbx_stream.hip, and every decision that is integers
// alone -- what a submit is refused for, which buffers a session owns, where a group's bursts lie -- is made in mbx_session_plan.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "mbx.h"
#include <mbx_agc.h>       // (levelled rows: the public header)
#include "mbx_agc_plan.h"      // (what an agc is refused for, and the device and the size of a state)
#include <mbx_filter.h>    // (filtered rows: the public header)
#include "mbx_filter_plan.h"   // (what a filter is refused for, and the device and the size of a state)
#include <mbx_limit.h>     // (limited buses: the public header)
#include "mbx_limit_plan.h"    // (what a limit is refused for, and the device, the size and the scratch of a state)
#include <mbx_resample.h>  // (wide rows: the public header)
#include "mbx_resample_plan.h" // (what a resampler is refused for, and the device and the size of a state)
#include <mbx_bands.h>     // (band records: the public header)
#include "mbx_bands_plan.h"    // (the forms, and the device and the probes of a bank)
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
#include "mbx_session_plan.h"

namespace {

constexpr int kDepth = 3;
static_assert(mbx::kMaxBurstGroups == MBX_BURST_MAX_GROUPS, "mbx_session_plan.h lays out as many groups as a call may have");

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

struct CopyOut { void* dst; const void* src; size_t bytes; };   // a staged output still to be handed to the caller's pageable buffer

// A buffer of a slot, on the device or pinned on the host: made by the first need() and made anew by one that asks for more (the
// slot's earlier batch is finished: nothing reads the old one).  A need() of the size it has is free.
template <bool kHost>
struct Grown {
    uint8_t* p = nullptr;
    size_t   cap = 0;
    int need(size_t bytes) {
        if (cap >= bytes) {
            return 0;
        }
        release();
        S_TRY(kHost ? hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault) : hipMalloc(reinterpret_cast<void**>(&p), bytes));
        cap = bytes;
        return 0;
    }
    void release() {
        if (p) {
            (void)(kHost ? hipHostFree(p) : hipFree(p));
        }
        p = nullptr;
        cap = 0;
    }
};
struct Pair { Grown<false> d; Grown<true> h; };   // a device buffer and its pinned staging, the staging made on first need

// The inputs of a slot.  Wire frames and the index words are made with the session.  Soft frames are 368 / 336 / 192 B each against
// 18 / 9: their device buffer and their staging belong to the slot's first soft submit, so a session that never sees one pays for
// neither; the keystream rows (include/mbx_keystream.h) likewise to its first keyed submit.  Bursts (hard or soft) belong to the burst
// submits and grow with them.
enum In { kInFrames = 0, kInSoft, kInBursts, kInKeystream, kInIndex, kInCount };

struct Slot {
    Pair       in[kInCount];
    Pair       out[mbx::kOutCount];   // (mbx_session_plan.h: which of them a session owns, and their sizes)
    void*      d_workspace = nullptr;
    hipEvent_t comp = nullptr, done = nullptr;
    bool       busy = false;
    // the buses of a submit resampled (mbx_session_next_resample, include/mbx_resample.h): made by the slot's first resampled submit,
    // and made anew by one that needs more, so a session that never sees one pays for neither the buffer nor its staging
    Pair       wide;
    // the band records of a submit (mbx_session_next_bands, include/mbx_bands.h): made by the slot's first submit with a bank, for
    // max_frames_per_submit rows of that bank and form, and made anew by a bank that needs more
    Pair       bands;
    CopyOut    staged[mbx::kOutCount + 2];   // (the outputs of the table, the wide buses and the band records)
    int        nout = 0;
    template <class U> U* din(int which) { return reinterpret_cast<U*>(in[which].d.p); }
    template <class U> U* dout(int which) { return reinterpret_cast<U*>(out[which].d.p); }
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
        memcpy(sl.staged[i].dst, sl.staged[i].src, sl.staged[i].bytes);
    }
    sl.nout = 0;
    sl.busy = false;
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
enum MixKind { kMixPlain = 0, kMixGated, kMixHeld };
struct NextOut {
    void*    dst = nullptr;   // host memory, rows * 160 bytes; nullptr: nothing attached
    int      law = 0;         // MBX_LAW_*
    void*                   buses = nullptr;   // host memory, the plan's buses * 160 samples of `form`; nullptr: nothing attached
    const mbx_mixdown_plan* plan = nullptr;
    int                     form = 0;          // MBX_MIXDOWN_*
    // the buses as they are, under `gate` (mbx_session_next_mixdown_gated, include/mbx_levels.h) or under `hold` with the caller's
    // `state` (mbx_session_next_mixdown_held, include/mbx_hold.h): the same slot, whichever call came last
    MixKind                 kind = kMixPlain;
    mbx_mixdown_gate        gate = {0, 0};
    mbx_mixdown_hold        hold = {0, 0, 0, 0, 0};
    mbx_gate_state*         state = nullptr;
    void*                   levels = nullptr;  // host memory, one mbx_row_level per row (mbx_session_next_levels); nullptr: nothing attached
    // the slot's int16 rows levelled in place under `agc` with the caller's `agc_state` (mbx_session_next_agc, include/mbx_agc.h), in
    // front of every other launch behind the step; nullptr: nothing attached
    void*                   agc_state = nullptr;
    mbx_agc                 agc = {0, 0, 0, 0, 0, 0, 0, 0};
    // the slot's int16 rows filtered in place under `filter` with the caller's `filter_state` (mbx_session_next_filter,
    // include/mbx_filter.h), in front of the AGC and so of every launch behind the step; nullptr: nothing attached
    void*                   filter_state = nullptr;
    mbx_filter              filter = {};
    // the buses limited under `limit` with the caller's `limit_state` (mbx_session_next_limit, include/mbx_limit.h): their sums into the
    // state's scratch, then the limiter into the slot's bus buffer in `form`; nullptr: nothing attached
    void*                   limit_state = nullptr;
    mbx_limit               limit = {0, 0, 0, 0, {0, 0, 0}};
    // the buses resampled under `resample` with the caller's `resample_state` into `wide` (mbx_session_next_resample,
    // include/mbx_resample.h): one launch behind the bus launches, from the slot's bus buffer into the slot's wide buffer; nullptr:
    // nothing attached
    void*                   resample_state = nullptr;
    void*                   wide = nullptr;    // host memory, the plan's buses * 160 * L int16
    mbx_resample            resample = {};
    // the records of the slot's int16 rows against `bank` in `band_form` (mbx_session_next_bands, include/mbx_bands.h): one launch
    // beside the levels launch, into the slot's band buffer; nullptr: nothing attached
    void*                   bands = nullptr;   // host memory, rows * K records
    const mbx_band_bank*    bank = nullptr;
    int                     band_form = 0;     // MBX_BANDS_*
    bool wants_levels() const { return levels || (buses && kind != kMixPlain); }
    // the step is handed the slot's int16 rows: for the caller, or for the compand, the levels and the mix-down behind the step; an
    // attached AGC or filter advances its state whether or not anybody takes the rows
    bool wants_pcm16(const void* callers) const { return callers || dst || buses || levels || agc_state || filter_state || bands; }
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

// One attach call: a NULL destination clears `field` of what is attached and leaves the rest; else `why` (the call's own checks, which
// may look at the session) names a refusal or nullptr, and `set` stores into the record.
template <class Why, class Set>
int next_attach(const char* who, const mbx_session* s, const void* out, void* NextOut::*field, Why why, Set set) {
    if (!s) {
        return mbx::refuse(who, "no session");
    }
    if (out) {
        if (const char* text = why()) {
            return mbx::refuse(who, text);
        }
    }
    std::lock_guard<std::mutex> lock(g_next_mu);
    if (out) {
        set(g_next[s]);
    } else if (const auto it = g_next.find(s); it != g_next.end()) {
        it->second.*field = nullptr;
    }
    return 0;
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

// One submit, as its public entry point fills it in.  A group submit uses the kind, the outputs and the attachment.
struct Submit {
    int            n = 0, T = 0;       // n streams of T frames each
    const int32_t* index = nullptr;
    const void*    frames = nullptr;   // wire frames (frame_bytes each); soft: mbe_soft_bit cells (soft_bytes per frame); burst: bursts
    bool           soft = false;
    const BurstIn* burst = nullptr;
    const uint8_t* keystream = nullptr;
    void*          user[mbx::kOutCount] = {};   // where each output goes: the caller's four, and the three of `next`
    NextOut        next;                         // taken for this call
    Submit(const NextOut& nx, int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records) : next(nx) {
        user[mbx::kOutPcm16] = pcm16, user[mbx::kOutPcmf] = pcmf, user[mbx::kOutResults] = results, user[mbx::kOutRecords] = records;
        user[mbx::kOutPcm8] = nx.dst, user[mbx::kOutMix] = nx.buses, user[mbx::kOutLevels] = nx.levels;
    }
    Submit& rows(int n_, int T_, const int32_t* index_, const void* frames_, bool soft_) {
        n = n_, T = T_, index = index_, frames = frames_, soft = soft_;
        return *this;
    }
};

// what the plan header holds a submit to (s may be NULL: then nothing of it is looked at)
mbx::SessionShape shape_of(const mbx_session* s, const Submit& c) {
    mbx::SessionShape sh;
    sh.session = s != nullptr;
    if (s) {
        sh.mixed = s->mixed(), sh.streams = s->streams, sh.max_frames = s->max_frames, sh.flags = s->outputs;
    }
    sh.requested = mbx::requested_outputs(c.user[mbx::kOutPcm16], c.user[mbx::kOutPcmf], c.user[mbx::kOutResults]);
    sh.plan_rows = c.next.buses ? mbx_mixdown_plan_rows(c.next.plan) : 0;   // (every row the plan names must be among the submit's)
    return sh;
}

// what mbx_session_plan.h says of a submit goes back: nothing to do is 0; a refusal with "<who>: <its text>", or with no text where it has none
int refused(const char* who, mbx::SessionRefusal why, const Submit& c, size_t rows) {
    const char* const text = mbx::session_refusal_text(why);
    if (why == mbx::kSessionRowsShort) {
        char numbers[200];
        snprintf(numbers, sizeof(numbers), text, rows, mbx_mixdown_plan_rows(c.next.plan));
        return mbx::refuse("session", numbers);
    }
    return why == mbx::kSessionNothing ? 0 : (text[0] ? mbx::refuse(who, text) : MBE_STATUS_INVALID_ARGUMENT);
}

// Host bytes to a device address.  They are fetched by a kernel on the COMPUTE stream, not by a DMA copy: see stage_in_kernel
// (mbx_fec.hip).  Pinned 16-byte aligned bytes are read in place; others -- pageable, or pinned and not aligned -- go through the
// buffer's pinned staging (`room` bytes of it, made here on first need) at the offset `at` they have on the device.
int carry_in(mbx_session* s, Pair& buf, size_t at, const void* host, size_t bytes, size_t room) {
    const uint8_t* src = static_cast<const uint8_t*>(host);
    if (!is_pinned(src) || !mbx::aligned_to(src, 16)) {
        if (const int rc = buf.h.need(room); rc < 0) {
            return rc;
        }
        memcpy(buf.h.p + at, src, bytes);
        src = buf.h.p + at;
    }
    const void* dev_view = src;   // what the GPU dereferences: the same address for hipHostMalloc memory, possibly another one for
    void* mapped = nullptr;       // memory the host registered itself (hipHostRegister)
    if (hipHostGetDevicePointer(&mapped, const_cast<uint8_t*>(src), 0) == hipSuccess && mapped) {
        dev_view = mapped;
    } else {
        (void)hipGetLastError();
    }
    return mbx_stage_in(buf.d.p + at, dev_view, bytes, s->s_comp);
}

// ---- out ----: behind the compute stream's launches of a submit of nf frames, the outputs to the caller (or to the slot's staging,
// made on the output's first pageable destination)
int copy_out(mbx_session* s, Slot& sl, const Submit& c, size_t nf) {
    S_TRY(hipEventRecord(sl.comp, s->s_comp));
    S_TRY(hipStreamWaitEvent(s->s_out, sl.comp, 0));
    sl.nout = 0;
    const size_t buses = c.next.buses ? (size_t)mbx_mixdown_plan_buses(c.next.plan) : 0;
    for (int k = 0; k < mbx::kOutCount; ++k) {
        if (!c.user[k]) {
            continue;
        }
        const size_t bytes = mbx::out_bytes(k, nf, buses, c.next.form);
        void* dst = c.user[k];
        if (!is_pinned(dst)) {
            if (const int rc = sl.out[k].h.need(mbx::out_capacity(k, s->max_frames)); rc < 0) {
                return rc;
            }
            dst = sl.out[k].h.p;
            sl.staged[sl.nout++] = CopyOut{c.user[k], dst, bytes};
        }
        const hipError_t e = hipMemcpyAsync(dst, sl.out[k].d.p, bytes, hipMemcpyDeviceToHost, s->s_out);
        if (e != hipSuccess) {
            return mbx::hip_failed("session: ", "hipMemcpyAsync (device to host)", e);
        }
    }
    if (c.next.resample_state && buses > 0) {   // the wide buses, on the road every output takes: a pinned destination in place, a pageable one staged
        const size_t bytes = mbx::wide_bytes(buses, c.next.resample.L);
        void* dst = c.next.wide;
        if (!is_pinned(dst)) {
            if (const int rc = sl.wide.h.need(bytes); rc < 0) {
                return rc;
            }
            dst = sl.wide.h.p;
            sl.staged[sl.nout++] = CopyOut{c.next.wide, dst, bytes};
        }
        const hipError_t e = hipMemcpyAsync(dst, sl.wide.d.p, bytes, hipMemcpyDeviceToHost, s->s_out);
        if (e != hipSuccess) {
            return mbx::hip_failed("session: ", "hipMemcpyAsync (device to host)", e);
        }
    }
    if (c.next.bands) {   // the band records, on the same road
        const size_t bytes = mbx::band_bytes(nf, c.next.bank->K, c.next.band_form);
        void* dst = c.next.bands;
        if (!is_pinned(dst)) {
            if (const int rc = sl.bands.h.need(mbx::band_bytes(s->max_frames, c.next.bank->K, c.next.band_form)); rc < 0) {
                return rc;
            }
            dst = sl.bands.h.p;
            sl.staged[sl.nout++] = CopyOut{c.next.bands, dst, bytes};
        }
        const hipError_t e = hipMemcpyAsync(dst, sl.bands.d.p, bytes, hipMemcpyDeviceToHost, s->s_out);
        if (e != hipSuccess) {
            return mbx::hip_failed("session: ", "hipMemcpyAsync (device to host)", e);
        }
    }
    S_TRY(hipEventRecord(sl.done, s->s_out));
    return 0;
}

// a limiter attached to a submit (mbx_session_next_limit): what the submit refuses of it, before anything is queued -- no buses to
// limit, or a plan of more buses than the state has records and scratch for; nullptr: nothing
const char* limit_refused_text(const NextOut& next) {
    if (!next.limit_state) {
        return nullptr;
    }
    if (!next.buses) {
        return "a limiter is attached (mbx_session_next_limit) and no buses are";
    }
    return mbx_mixdown_plan_buses(next.plan) > static_cast<const mbx_limit_state*>(next.limit_state)->buses
               ? "the plan has more buses than the limiter's state (mbx_limit_state_buses)"
               : nullptr;
}

// a resampler attached to a submit (mbx_session_next_resample): what the submit refuses of it, before anything is queued -- no buses to
// resample, buses that are not int16, a plan of more buses than the state has records, or a state of another device; nullptr: nothing
const char* resample_refused_text(const mbx_session* s, const NextOut& next) {
    if (!next.resample_state) {
        return nullptr;
    }
    if (!next.buses) {
        return "a resampler is attached (mbx_session_next_resample) and no buses are";
    }
    if (next.form != MBX_MIXDOWN_PCM16) {
        return "a resampler is attached (mbx_session_next_resample) and the buses are not MBX_MIXDOWN_PCM16";
    }
    const mbx_resample_state* const st = static_cast<const mbx_resample_state*>(next.resample_state);
    if (mbx_mixdown_plan_buses(next.plan) > st->streams) {
        return "the plan has more buses than the resampler's state (mbx_resample_state_streams)";
    }
    return st->device != s->device ? "a resampler's state of another device than the session" : nullptr;
}

// Behind the step of a submit of nf frames, on the compute stream: FIRST the slot's int16 rows filtered in place where a filter is
// attached, THEN levelled in place where an AGC is (the records of the submit's streams: its index on the device, or 0 .. n-1); then those rows -> companded bytes where a
// destination is attached; their level records, once per submit, for the caller or for the gate of its buses or both; beside them the band records of those
// rows where a bank is attached, into the slot's band buffer; the plan's buses of those rows
// (one or two more launches) -- under an attached limiter their sums into the limiter's scratch and the limited rows from there, one
// launch more; the buses resampled into the slot's wide buffer where a resampler is attached, one launch behind them; then the outputs out.
int behind_step(mbx_session* s, Slot& sl, const Submit& c, size_t nf) {
    const NextOut& next = c.next;
    int16_t* const d16 = sl.dout<int16_t>(mbx::kOutPcm16);
    mbx_row_level* const dlev = sl.dout<mbx_row_level>(mbx::kOutLevels);
    uint8_t* const dmix = sl.dout<uint8_t>(mbx::kOutMix);
    int rc = 0;
    const int32_t* const dindex = c.index ? sl.din<int32_t>(kInIndex) : nullptr;
    if (next.filter_state
        && (rc = mbx_pcm_filter(&next.filter, static_cast<mbx_filter_state*>(next.filter_state), dindex, c.n, c.T, d16, d16, s->s_comp)) < 0) {
        return rc;
    }
    if (next.agc_state
        && (rc = mbx_pcm_agc(&next.agc, static_cast<mbx_agc_state*>(next.agc_state), dindex, c.n, c.T, d16, d16, s->s_comp)) < 0) {
        return rc;
    }
    if ((next.dst && (rc = mbx_pcm_compand(next.law, d16, nf, sl.dout<uint8_t>(mbx::kOutPcm8), s->s_comp)) < 0)
        || (next.wants_levels() && (rc = mbx_pcm_levels(d16, nf, dlev, s->s_comp)) < 0)) {
        return rc;
    }
    if (next.bands
        && ((rc = sl.bands.d.need(mbx::band_bytes(s->max_frames, next.bank->K, next.band_form))) < 0
            || (rc = mbx_pcm_bands(next.bank, next.band_form, d16, nf, sl.bands.d.p, s->s_comp)) < 0)) {
        return rc;
    }
    if (next.buses && next.limit_state) {
        mbx_limit_state* const lim = static_cast<mbx_limit_state*>(next.limit_state);
        int32_t* const dsums = mbx_limit_state_sums(lim);
        rc = next.kind == kMixHeld    ? mbx_mixdown_held_sums(next.plan, &next.hold, next.state, d16, nf, dlev, dsums, s->s_comp)
             : next.kind == kMixGated ? mbx_mixdown_gated_sums(next.plan, &next.gate, d16, nf, dlev, dsums, s->s_comp)
                                      : mbx_mixdown_sums(next.plan, d16, nf, dsums, s->s_comp);
        if (rc >= 0) {
            rc = mbx_bus_limit(&next.limit, lim, mbx_mixdown_plan_buses(next.plan), 1, dsums, next.form, dmix, s->s_comp);
        }
    } else if (next.buses && next.kind == kMixHeld) {
        rc = mbx_mixdown_held(next.plan, &next.hold, next.state, next.form, d16, nf, dlev, dmix, s->s_comp);
    } else if (next.buses && next.kind == kMixGated) {
        rc = mbx_mixdown_gated(next.plan, &next.gate, next.form, d16, nf, dlev, dmix, s->s_comp);
    } else if (next.buses) {
        rc = mbx_mixdown(next.plan, next.form, d16, nf, dmix, s->s_comp);
    }
    if (rc >= 0 && next.resample_state) {   // (resample_refused_text: there are buses, and they are int16)
        const int buses = mbx_mixdown_plan_buses(next.plan);
        if (buses > 0 && (rc = sl.wide.d.need(mbx::wide_bytes((size_t)buses, next.resample.L))) >= 0) {
            rc = mbx_pcm_resample(&next.resample, static_cast<mbx_resample_state*>(next.resample_state), nullptr, buses, 1, reinterpret_cast<const int16_t*>(dmix),
                                  reinterpret_cast<int16_t*>(sl.wide.d.p), s->s_comp);
        }
    }
    return rc < 0 ? rc : copy_out(s, sl, c, nf);
}

// The slot of the next batch, with the batch that used it kDepth submissions ago finished, and `enqueue` run on it.  From there on
// work is queued on the two streams against this slot's buffers.  If anything fails halfway the slot is NOT marked busy, so before
// the error goes back the streams are drained: the next submit may reuse the slot at once.
template <class Enqueue>
int on_next_slot(mbx_session* s, Enqueue enqueue) {
    DeviceGuard guard(s->device);
    Slot& sl = s->slot[s->submitted % kDepth];
    int rc = finish_slot(sl);
    if (rc < 0) {
        return rc;
    }
    rc = enqueue(sl);
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

int enqueue(mbx_session* s, Slot& sl, const Submit& c) {
    const int      n = c.n, T = c.T;
    const bool     soft = c.soft;
    const BurstIn* burst = c.burst;
    const size_t   nf = (size_t)n * (size_t)T;
    // ---- in ----: the frames or bursts, the stream index, the keystream rows
    const size_t in_bytes = soft ? s->soft_bytes : s->frame_bytes;
    const size_t in_total = burst ? (size_t)n * burst->bytes : nf * in_bytes;
    const size_t in_room = burst ? in_total : s->max_frames * in_bytes;
    Pair& in = sl.in[burst ? kInBursts : (soft ? kInSoft : kInFrames)];
    int rc = 0;
    if ((rc = in.d.need(in_room)) < 0 || (rc = carry_in(s, in, 0, c.frames, in_total, in_room)) < 0) {
        return rc;
    }
    int32_t* const d_index = c.index ? sl.din<int32_t>(kInIndex) : nullptr;
    if (c.index) {   // always staged: 4 B per stream, and the caller may reuse its array at once
        Grown<true>& h_index = sl.in[kInIndex].h;
        if ((rc = h_index.need((size_t)s->streams * sizeof(int32_t))) < 0) {
            return rc;
        }
        memcpy(h_index.p, c.index, (size_t)n * sizeof(int32_t));
        if ((rc = mbx_stage_in(d_index, h_index.p, (size_t)n * sizeof(int32_t), s->s_comp)) < 0) {
            return rc;
        }
    }
    if (c.keystream) {   // the keystream rows take the road the frames take
        const size_t ks_room = s->max_frames * (size_t)MBX_KEYSTREAM_ROW_BYTES;
        Pair& ks = sl.in[kInKeystream];
        if ((rc = ks.d.need(ks_room)) < 0 || (rc = carry_in(s, ks, 0, c.keystream, nf * (size_t)MBX_KEYSTREAM_ROW_BYTES, ks_room)) < 0) {
            return rc;
        }
    }
    // ---- compute ----
    int16_t* d16 = c.next.wants_pcm16(c.user[mbx::kOutPcm16]) ? sl.dout<int16_t>(mbx::kOutPcm16) : nullptr;
    float*   dfl = c.user[mbx::kOutPcmf] ? sl.dout<float>(mbx::kOutPcmf) : nullptr;
    mbe_process_result* dres = c.user[mbx::kOutResults] ? sl.dout<mbe_process_result>(mbx::kOutResults) : nullptr;
    mbx_param_record* const drec = sl.dout<mbx_param_record>(mbx::kOutRecords);
    uint8_t* const      d_frames = sl.din<uint8_t>(kInFrames);
    mbe_soft_bit* const d_soft = sl.din<mbe_soft_bit>(kInSoft);
    if (c.keystream) {   // the keyed call takes every form: hard or soft, index or none, resident words or plain triplets
        rc = mbx_process_batch_keyed(s->codec, n, T, d_index, soft ? nullptr : d_frames, soft ? d_soft : nullptr, sl.din<uint8_t>(kInKeystream),
                                     s->d_state, s->d_resident, s->d_rng, d16, dfl, dres, drec, s->s_comp);
    } else if (burst && soft) {   // the gather in front of the step the frames submits run: resident words or plain triplets, index or none
        rc = mbx_process_bursts_soft(burst->sched, n, d_index, sl.din<mbe_soft_bit>(kInBursts), s->d_state, s->d_resident, s->d_rng, d16, dfl, dres,
                                     drec, s->s_comp);
    } else if (burst) {
        rc = mbx_process_bursts(burst->sched, n, d_index, sl.din<uint8_t>(kInBursts), burst->stride, s->d_state, s->d_resident, s->d_rng, d16, dfl,
                                dres, drec, s->s_comp);
    } else if (soft) {   // the soft twin of the resident launcher takes every form: index or none, resident words or plain triplets
        rc = mbx_process_batch_soft_resident(s->codec, n, T, d_index, d_soft, s->d_state, s->d_resident, s->d_rng, d16, dfl, dres, drec, s->s_comp);
    } else if (s->d_resident) {   // the session owns the state between submits: the resident form (no prev_mp_enhanced traffic, lazy prev_mp)
        rc = mbx_process_batch_resident(s->codec, n, T, d_index, d_frames, s->d_state, s->d_resident, s->d_rng, d16, dfl, dres, drec, s->s_comp);
    } else if (c.index) {
        rc = mbx_process_batch_indexed(s->codec, n, T, d_index, d_frames, s->d_state, s->d_rng, d16, dfl, dres, drec, s->s_comp);
    } else {
        rc = mbx_process_batch_ws(s->codec, n, T, d_frames, s->d_state, s->d_rng, d16, dfl, dres, drec, sl.d_workspace,
                                  mbx_workspace_bytes(s->max_frames), s->s_comp);
    }
    return rc < 0 ? rc : behind_step(s, sl, c, nf);
}

int submit(mbx_session* s, const Submit& c) {
    const mbx::SessionRefusal why = mbx::frames_submit_refused(shape_of(s, c), c.frames != nullptr, c.n, c.T);
    if (why != mbx::kSessionOk) {
        return refused("mbx_session_submit", why, c, (size_t)c.n * (size_t)c.T);
    }
    if (const char* const text = limit_refused_text(c.next)) {
        return mbx::refuse("mbx_session_submit", text);
    }
    if (const char* const text = resample_refused_text(s, c.next)) {
        return mbx::refuse("mbx_session_submit", text);
    }
    int rc = 0;
    if (c.burst) {   // bursts of a form that can be invalid: a bit byte > 1, a dibit > 3, a soft hard decision > 1 (mbx_burst_validate); every LLR is a valid one
        rc = mbx::burst_shape(c.burst->sched).llr() ? 0 : mbx_burst_validate(c.burst->sched, c.frames, c.burst->stride, (size_t)c.n, c.soft ? 1 : 0);
    } else if (c.soft) {   // a hard decision > 1 is refused before anything is queued (ref mbe_validate_soft_bits, src/internal/mbe_result.h:31-42)
        rc = mbx_validate_soft_bits(static_cast<const mbe_soft_bit*>(c.frames), (size_t)c.n * (size_t)c.T * (s->soft_bytes / sizeof(mbe_soft_bit)));
    }
    if (rc < 0) {
        return rc;
    }
    if (c.index) {
        s->seen.assign((size_t)s->streams, 0);
        if (mbx::mark_streams(s->seen.data(), s->streams, c.index, c.n) != mbx::kSessionOk) {
            return refused("session", mbx::kSessionIndex, c, 0);
        }
    }
    return on_next_slot(s, [&](Slot& sl) { return enqueue(s, sl, c); });
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

// the device side of a new session whose sizes are set: state, streams, the slots' buffers and events, the streams' state at its defaults
static int session_buffers(mbx_session* s) {
    const size_t streams = (size_t)s->streams, mf = s->max_frames;
    S_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_state), streams * 3 * sizeof(mbe_parms)));
    S_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_rng), streams * sizeof(mbx_stream_rng)));
    if (!getenv("MBX_SESSION_ABI_STATE")) {   // (development switch: keep the ABI triplets whole after every submit, for A/B timing)
        S_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_resident), streams * sizeof(uint32_t)));
        S_TRY(hipMemset(s->d_resident, 0, streams * sizeof(uint32_t)));
    }
    S_TRY(hipStreamCreateWithFlags(&s->s_comp, hipStreamNonBlocking));
    S_TRY(hipStreamCreateWithFlags(&s->s_out, hipStreamNonBlocking));
    int rc = 0;
    for (Slot& sl : s->slot) {
        if ((rc = sl.in[kInFrames].d.need(mf * s->frame_bytes)) < 0 || (rc = sl.in[kInIndex].d.need(streams * sizeof(int32_t))) < 0) {
            return rc;
        }
        if (!s->d_resident) {   // (the resident entry point uses the workspace the launcher keeps for the compute stream, reserved below)
            S_TRY(hipMalloc(&sl.d_workspace, mbx_workspace_bytes(mf)));
        }
        for (int k = 0; k < mbx::kOutCount; ++k) {
            if (mbx::out_owned(k, s->outputs) && (rc = sl.out[k].d.need(mbx::out_capacity(k, mf))) < 0) {
                return rc;
            }
        }
        S_TRY(hipEventCreateWithFlags(&sl.comp, hipEventDisableTiming));
        // (a blocking wait -- hipEventBlockingSync -- was measured here and costs more than it saves: the wake-up latency of every
        // submit that has to wait is exposed, 155 -> 113 M frames/s with two session threads, 117 -> 78 M with four)
        S_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    // the indexed launches size the compute stream's own workspace once, here, not in the first submit
    rc = mbx_reserve_stream(s->s_comp, mf);
    return rc < 0 ? rc : mbx_session_reset(s, 0, s->streams);
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
            return mbx::refuse("mbx_session_create_mixed", "a stream_codec byte is not one of MBX_CODEC_*");
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
    const int rc = session_buffers(s);
    if (rc < 0) {
        mbx_session_destroy(s);
        *out = nullptr;
    }
    return rc;
}

int mbx_session_create(mbx_session** out, int codec, int streams, size_t max_frames_per_submit, unsigned outputs) {
    return create_session(out, codec, nullptr, streams, max_frames_per_submit, outputs);
}

int mbx_session_create_mixed(mbx_session** out, int streams, const uint8_t* stream_codec, size_t max_frames_per_submit, unsigned outputs) {
    if (!stream_codec) {
        return mbx::refuse("mbx_session_create_mixed", "stream_codec is NULL");
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
        for (Pair& b : sl.in) {
            b.d.release(), b.h.release();
        }
        for (Pair& b : sl.out) {
            b.d.release(), b.h.release();
        }
        sl.wide.d.release(), sl.wide.h.release();
        sl.bands.d.release(), sl.bands.h.release();
        (void)hipFree(sl.d_workspace);
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
    return submit(s, Submit(take_next(s), pcm16, pcmf, results, nullptr).rows(s ? s->streams : 0, T, nullptr, frames, false));
}

int mbx_session_submit_indexed(mbx_session* s, int n, int T, const int32_t* stream_index, const uint8_t* frames, int16_t* pcm16,
                               float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    Submit c(take_next(s), pcm16, pcmf, results, records);
    return stream_index ? submit(s, c.rows(n, T, stream_index, frames, false)) : MBE_STATUS_INVALID_ARGUMENT;
}

int mbx_session_submit_soft(mbx_session* s, int T, const mbe_soft_bit* soft, int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    return submit(s, Submit(take_next(s), pcm16, pcmf, results, nullptr).rows(s ? s->streams : 0, T, nullptr, soft, true));
}

int mbx_session_submit_soft_indexed(mbx_session* s, int n, int T, const int32_t* stream_index, const mbe_soft_bit* soft, int16_t* pcm16,
                                    float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    Submit c(take_next(s), pcm16, pcmf, results, records);
    return stream_index ? submit(s, c.rows(n, T, stream_index, soft, true)) : MBE_STATUS_INVALID_ARGUMENT;
}

// ---- companded bytes out (include/mbx_pcm8.h): the destination of the next submit ----------------------------------------------------
int mbx_session_next_pcm8(mbx_session* s, int law, uint8_t* pcm8) {
    const auto why = [&]() -> const char* {
        if (!(s->outputs & MBX_SESSION_PCM8)) {
            return "the session was created without MBX_SESSION_PCM8";
        }
        return law != MBX_LAW_ULAW && law != MBX_LAW_ALAW ? "law is MBX_LAW_ULAW or MBX_LAW_ALAW" : nullptr;
    };
    return next_attach("mbx_session_next_pcm8", s, pcm8, &NextOut::dst, why, [&](NextOut& next) { next.dst = pcm8, next.law = law; });
}

// ---- mix-down out (include/mbx_mixdown.h): the buses of the next submit -----------------------------------------------------------------
// how the buses are attached: as they are (mbx_session_next_mixdown), under a gate (the gated call of include/mbx_levels.h) or under a
// hold with the caller's state (the held call of include/mbx_hold.h).  The three share the buses of the record.
struct MixHow {
    MixKind                 kind;
    const mbx_mixdown_gate* gate;
    const mbx_mixdown_hold* hold;
    mbx_gate_state*         state;
};
static int next_mixdown(const char* who, mbx_session* s, const mbx_mixdown_plan* plan, int form, void* out, const MixHow& how) {
    const auto why = [&]() -> const char* {
        if (!(s->outputs & MBX_SESSION_MIXDOWN)) {
            return "the session was created without MBX_SESSION_MIXDOWN";
        }
        if (how.kind != kMixPlain && !(s->outputs & MBX_SESSION_LEVELS)) {
            return "the session was created without MBX_SESSION_LEVELS";
        }
        if (!plan) {
            return "no plan";
        }
        if (how.kind == kMixGated) {
            const mbx_mixdown_gate* gate = how.gate;
            const mbx::LevelsRefusal bad = mbx::gate_refused(gate != nullptr, gate ? gate->open_peak : 0u, gate ? gate->loudest_n : 0u);
            if (bad != mbx::kLevelsOk) {
                return mbx::levels_refusal_text(bad);
            }
        }
        if (how.kind == kMixHeld) {
            const mbx_mixdown_hold* hold = how.hold;
            mbx::HoldRefusal bad = mbx::hold_refused(hold != nullptr, hold ? hold->open_peak : 0u, hold ? hold->close_peak : 0u, hold ? hold->loudest_n : 0u,
                                                     hold ? hold->ramp_log2 : 0u);
            if (bad == mbx::kHoldOk) {
                bad = mbx::hold_state_refused(how.state != nullptr, how.state ? how.state->plan : nullptr, plan);
            }
            if (bad != mbx::kHoldOk) {
                return mbx::hold_refusal_text(bad);
            }
        }
        if (form != MBX_MIXDOWN_PCM16 && form != MBX_MIXDOWN_ULAW && form != MBX_MIXDOWN_ALAW) {
            return "form is MBX_MIXDOWN_PCM16, MBX_MIXDOWN_ULAW or MBX_MIXDOWN_ALAW";
        }
        if ((size_t)mbx_mixdown_plan_buses(plan) > s->max_frames) {
            return "the plan has more buses than max_frames_per_submit";
        }
        return mbx::mixdown_plan_device(plan) != s->device ? "a plan of another device than the session" : nullptr;
    };
    return next_attach(who, s, out, &NextOut::buses, why, [&](NextOut& next) {
        next.buses = out, next.plan = plan, next.form = form, next.kind = how.kind;
        next.gate = how.kind == kMixGated ? *how.gate : mbx_mixdown_gate{0, 0};
        next.hold = how.kind == kMixHeld ? *how.hold : mbx_mixdown_hold{0, 0, 0, 0, 0};
        next.state = how.kind == kMixHeld ? how.state : nullptr;
    });
}

int mbx_session_next_mixdown(mbx_session* s, const mbx_mixdown_plan* plan, int form, void* out) {
    return next_mixdown("mbx_session_next_mixdown", s, plan, form, out, MixHow{kMixPlain, nullptr, nullptr, nullptr});
}

// ---- levels out and the gated mix-down (include/mbx_levels.h): the records and the gated buses of the next submit ------------------------
int mbx_session_next_mixdown_gated(mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_gate* gate, void* out) {
    return next_mixdown("mbx_session_next_mixdown_gated", s, plan, form, out, MixHow{kMixGated, gate, nullptr, nullptr});
}

// ---- the held gate (include/mbx_hold.h): the buses of the next submit under a hold, the caller's state advanced by one frame ------------
int mbx_session_next_mixdown_held(mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_hold* hold, mbx_gate_state* state, void* out) {
    return next_mixdown("mbx_session_next_mixdown_held", s, plan, form, out, MixHow{kMixHeld, nullptr, hold, state});
}

// ---- levelled rows (include/mbx_agc.h): the int16 rows of the next submit under an AGC, the caller's state advanced by its frames ------
int mbx_session_next_agc(mbx_session* s, const mbx_agc* agc, mbx_agc_state* state) {
    const auto why = [&]() -> const char* {
        const mbx::AgcRefusal bad = mbx::agc_refused(agc != nullptr, agc ? agc->target_peak : 0u, agc ? agc->floor_peak : 0u, agc ? agc->min_gain_q10 : 0u,
                                                     agc ? agc->max_gain_q10 : 0u, agc ? agc->ramp_log2 : 0u, agc ? agc->zero : 0u);
        if (bad != mbx::kAgcOk) {
            return mbx::agc_refusal_text(bad);
        }
        if (!mbx::out_owned(mbx::kOutPcm16, s->outputs)) {
            return "the session was created without an output that has int16 rows";
        }
        if (state->streams < s->streams) {
            return "the state holds fewer records than the session has streams";
        }
        return state->device != s->device ? "a state of another device than the session" : nullptr;
    };
    return next_attach("mbx_session_next_agc", s, state, &NextOut::agc_state, why, [&](NextOut& next) { next.agc_state = state, next.agc = *agc; });
}

// ---- filtered rows (include/mbx_filter.h): the int16 rows of the next submit through a cascade, the caller's state advanced by its frames
int mbx_session_next_filter(mbx_session* s, const mbx_filter* filter, mbx_filter_state* state) {
    const auto why = [&]() -> const char* {
        const mbx::FilterRefusal bad = mbx::filter_refused(filter != nullptr, filter ? filter->sections : 0u,
                                                           filter ? (unsigned)(filter->zero[0] | filter->zero[1] | filter->zero[2]) : 0u,
                                                           filter ? &filter->sec[0].b0 : nullptr);
        if (bad != mbx::kFilterOk) {
            return mbx::filter_refusal_text(bad);
        }
        if (!mbx::out_owned(mbx::kOutPcm16, s->outputs)) {
            return "the session was created without an output that has int16 rows";
        }
        if (state->streams < s->streams) {
            return "the state holds fewer records than the session has streams";
        }
        return state->device != s->device ? "a state of another device than the session" : nullptr;
    };
    return next_attach("mbx_session_next_filter", s, state, &NextOut::filter_state, why, [&](NextOut& next) { next.filter_state = state, next.filter = *filter; });
}

// ---- limited buses (include/mbx_limit.h): the buses of the next submit under a limiter, the caller's state advanced by one frame ------
int mbx_session_next_limit(mbx_session* s, const mbx_limit* limit, mbx_limit_state* state) {
    const auto why = [&]() -> const char* {
        const mbx::LimitRefusal bad = mbx::limit_refused(limit != nullptr, limit ? limit->ceiling : 0u, limit ? limit->ramp_log2 : 0u,
                                                         limit ? (unsigned)(limit->zero[0] | limit->zero[1] | limit->zero[2]) : 0u);
        if (bad != mbx::kLimitOk) {
            return mbx::limit_refusal_text(bad);
        }
        return state->device != s->device ? "a state of another device than the session" : nullptr;
    };
    return next_attach("mbx_session_next_limit", s, state, &NextOut::limit_state, why, [&](NextOut& next) { next.limit_state = state, next.limit = *limit; });
}

// ---- wide rows (include/mbx_resample.h): the buses of the next submit resampled as well, the caller's state advanced by one frame ------
int mbx_session_next_resample(mbx_session* s, const mbx_resample* rs, mbx_resample_state* state, int16_t* out) {
    const auto why = [&]() -> const char* {
        const mbx::ResampleRefusal bad = mbx::resample_refused(rs != nullptr, rs ? rs->L : 0u, rs ? rs->K : 0u, rs ? (unsigned)(rs->zero[0] | rs->zero[1]) : 0u,
                                                               rs ? rs->taps : nullptr);
        if (bad != mbx::kResampleOk) {
            return mbx::resample_refusal_text(bad);
        }
        if (!out) {
            return "no place for the wide buses";
        }
        return state->device != s->device ? "a state of another device than the session" : nullptr;
    };
    return next_attach("mbx_session_next_resample", s, state, &NextOut::resample_state, why,
                       [&](NextOut& next) { next.resample_state = state, next.resample = *rs, next.wide = out; });
}

// ---- band records (include/mbx_bands.h): the records of the next submit's int16 rows against a caller's bank ----------------------------
int mbx_session_next_bands(mbx_session* s, const mbx_band_bank* b, int form, void* out) {
    const auto why = [&]() -> const char* {
        if (!b) {
            return "no bank";
        }
        if (!mbx::bands_form_ok(form)) {
            return mbx::bands_refusal_text(mbx::kBandsForm);
        }
        if (!mbx::out_owned(mbx::kOutPcm16, s->outputs)) {
            return "the session was created without an output that has int16 rows";
        }
        return b->device != s->device ? "a bank of another device than the session" : nullptr;
    };
    return next_attach("mbx_session_next_bands", s, out, &NextOut::bands, why, [&](NextOut& next) { next.bands = out, next.bank = b, next.band_form = form; });
}

int mbx_session_next_levels(mbx_session* s, mbx_row_level* out) {
    const auto why = [&]() -> const char* { return s->outputs & MBX_SESSION_LEVELS ? nullptr : "the session was created without MBX_SESSION_LEVELS"; };
    return next_attach("mbx_session_next_levels", s, out, &NextOut::levels, why, [&](NextOut& next) { next.levels = out; });
}

// ---- keyed submits (include/mbx_keystream.h): a frames submit of either kind with a keystream row per frame ---------------------------
int mbx_session_submit_keyed(mbx_session* s, int n, int T, const int32_t* stream_index, const uint8_t* frames, const mbe_soft_bit* soft,
                             const uint8_t* keystream, int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    const char* const who = "mbx_session_submit_keyed";
    Submit c(take_next(s), pcm16, pcmf, results, records);
    if (s && s->mixed()) {
        return refused(who, mbx::kSessionMixed, c, 0);
    }
    if (!s || (frames != nullptr) == (soft != nullptr) || (!stream_index && n != s->streams)) {
        return mbx::refuse(who, "a session, exactly one of frames and soft, and without an index n = the session's stream count");
    }
    c.keystream = keystream;
    return submit(s, c.rows(n, T, stream_index, soft ? static_cast<const void*>(soft) : frames, soft != nullptr));
}

// ---- burst submits (include/mbx_burst.h) ---------------------------------------------------------------------------------------------
// (bursts: hard bursts of burst_stride bytes each, or soft ones of the schedule's own size)
static int submit_bursts(const char* who, mbx_session* s, const mbx_burst_schedule* sched, Submit& c, size_t burst_stride) {
    const mbx::BurstShape sh = sched ? mbx::burst_shape(sched) : mbx::BurstShape{};
    mbx::BurstsShape b;
    b.sched = sched != nullptr, b.bursts = c.frames != nullptr, b.soft = c.soft, b.llr = sched && sh.llr(), b.indexed = c.index != nullptr;
    b.n = c.n, b.frames = sh.frames, b.codec = sh.codec, b.device = sh.device, b.stride = burst_stride, b.sched_bytes = sh.bytes;
    b.session_codec = s ? s->codec : 0, b.session_device = s ? s->device : 0;
    const mbx::SessionRefusal why = mbx::bursts_submit_refused(shape_of(s, c), b);
    if (why != mbx::kSessionOk) {
        return refused(who, why, c, 0);
    }
    const BurstIn in{sched, burst_stride, c.soft ? mbx_burst_schedule_soft_bytes(sched) : burst_stride};
    c.T = sh.frames, c.burst = &in;
    return submit(s, c);
}

int mbx_session_submit_bursts(mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index, const uint8_t* bursts,
                              size_t burst_stride, int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    Submit c(take_next(s), pcm16, pcmf, results, nullptr);
    return submit_bursts("mbx_session_submit_bursts", s, sched, c.rows(n, 0, stream_index, bursts, false), burst_stride);
}

int mbx_session_submit_bursts_soft(mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index, const mbe_soft_bit* soft,
                                   int16_t* pcm16, float* pcmf, mbe_process_result* results) {
    Submit c(take_next(s), pcm16, pcmf, results, nullptr);
    return submit_bursts("mbx_session_submit_bursts_soft", s, sched, c.rows(n, 0, stream_index, soft, true), 0);
}

// ---- burst groups (include/mbx_burst_groups.h) --------------------------------------------------------------------------------------
// The groups' bursts into the slot's burst buffer, each group at a 16-byte aligned offset (pinned 16-byte aligned buffers read in
// place, others through the slot's pinned staging at the same offsets), their indices into the slot's index words, then
// mbx_process_burst_groups on the compute stream with the groups rewritten to those device addresses, and the outputs out.
static int enqueue_groups(mbx_session* s, Slot& sl, const Submit& c, const mbx_burst_group* groups, const mbx::GroupPlan& gp) {
    mbx::GroupIn in[MBX_BURST_MAX_GROUPS];
    for (int i = 0; i < gp.n_groups; ++i) {
        const mbx_burst_group& g = groups[i];
        in[i].bursts = gp.place[i].bursts;
        in[i].per = c.soft ? mbx_burst_schedule_soft_bytes(g.sched) : g.burst_stride;
        in[i].sched_bytes = c.soft ? 0 : mbx_burst_schedule_bytes(g.sched);
        in[i].in_place = in[i].bursts && is_pinned(g.bursts) && mbx::aligned_to(g.bursts, 16);   // (of a group without bursts the pointer is not looked at)
        in[i].has_index = g.stream_index != nullptr;
    }
    const mbx::GroupBytes lay = mbx::group_bytes(in, gp.n_groups, c.soft);
    Pair&          bursts = sl.in[kInBursts];
    Grown<true>&   h_index = sl.in[kInIndex].h;
    int32_t* const d_index = sl.din<int32_t>(kInIndex);
    int rc = 0;
    if ((rc = bursts.d.need(lay.total)) < 0 || (lay.staged && (rc = bursts.h.need(lay.total)) < 0)
        || (lay.indexed && (rc = h_index.need((size_t)s->streams * sizeof(int32_t))) < 0)) {
        return rc;
    }
    mbx_burst_group dev[MBX_BURST_MAX_GROUPS];
    for (int i = 0; i < gp.n_groups; ++i) {
        dev[i] = groups[i];
        dev[i].bursts = bursts.d.p + lay.at[i];
        dev[i].stream_index = nullptr;
        if (!lay.bytes[i]) {
            continue;
        }
        if ((rc = carry_in(s, bursts, lay.at[i], groups[i].bursts, lay.bytes[i], lay.total)) < 0) {
            return rc;
        }
        if (groups[i].stream_index) {   // (the groups name every stream once: their indices fit the slot's `streams` words, at their stream rows)
            memcpy(reinterpret_cast<int32_t*>(h_index.p) + gp.place[i].first_stream, groups[i].stream_index, (size_t)groups[i].n_streams * sizeof(int32_t));
            dev[i].stream_index = d_index + gp.place[i].first_stream;
        }
    }
    if (lay.indexed && (rc = mbx_stage_in(d_index, h_index.p, (size_t)gp.total_streams * sizeof(int32_t), s->s_comp)) < 0) {
        return rc;
    }
    rc = mbx_process_burst_groups(dev, gp.n_groups, c.soft ? 1 : 0, s->d_state, s->d_resident, s->d_rng,
                                  c.next.wants_pcm16(c.user[mbx::kOutPcm16]) ? sl.dout<int16_t>(mbx::kOutPcm16) : nullptr,
                                  c.user[mbx::kOutPcmf] ? sl.dout<float>(mbx::kOutPcmf) : nullptr,
                                  c.user[mbx::kOutResults] ? sl.dout<mbe_process_result>(mbx::kOutResults) : nullptr,
                                  sl.dout<mbx_param_record>(mbx::kOutRecords), s->s_comp);
    return rc < 0 ? rc : behind_step(s, sl, c, (size_t)gp.total_rows);
}

int mbx_session_submit_burst_groups(mbx_session* s, const mbx_burst_group* groups, int n_groups, int soft_in, int16_t* pcm16, float* pcmf,
                                    mbe_process_result* results) {
    const char* const who = "mbx_session_submit_burst_groups";
    Submit c(take_next(s), pcm16, pcmf, results, nullptr);
    c.soft = soft_in != 0;
    if (!s) {
        return refused(who, mbx::kSessionNoSession, c, 0);
    }
    if (c.next.filter_state) {   // (the groups have different frame counts: one launch of mbx_pcm_filter has one T)
        return mbx::refuse(who, "a filter is attached (mbx_session_next_filter): burst groups take none");
    }
    if (c.next.agc_state) {   // (the groups have different frame counts: one launch of mbx_pcm_agc has one T)
        return mbx::refuse(who, "an AGC is attached (mbx_session_next_agc): burst groups take none");
    }
    if (const char* const text = limit_refused_text(c.next)) {   // (a limiter they may take: buses have no T)
        return mbx::refuse(who, text);
    }
    if (const char* const text = resample_refused_text(s, c.next)) {   // (and a resampler, for the same reason)
        return mbx::refuse(who, text);
    }
    mbx::GroupShape shapes[MBX_BURST_MAX_GROUPS];
    mbx::GroupPlan gp;
    int rc = mbx::burst_groups_plan(who, groups, n_groups, c.soft, shapes, &gp);
    if (rc < 0) {
        return rc;
    }
    // the session's sizes; then every group's schedule is of the session's device and of the codec of every stream the group names,
    // slots in range, none named twice across the groups
    mbx::SessionRefusal why = mbx::groups_submit_refused(shape_of(s, c), gp.total_rows);
    s->seen.assign((size_t)s->streams, 0);
    for (int i = 0; i < n_groups && why == mbx::kSessionOk; ++i) {
        const mbx_burst_group& g = groups[i];
        const mbx::BurstShape sh = mbx::burst_shape(g.sched);
        why = sh.device != s->device ? mbx::kGroupsDevice
                                     : mbx::mark_group(s->seen.data(), s->streams, g.stream_index, g.first_slot, g.n_streams,
                                                       s->mixed() ? s->stream_codec.data() : nullptr, s->codec, sh.codec);
    }
    if (why != mbx::kSessionOk) {
        return refused(who, why, c, (size_t)gp.total_rows);
    }
    for (int i = 0; i < n_groups; ++i) {   // bursts of a form that can be invalid (mbx_burst_validate)
        if (gp.place[i].bursts && !mbx::burst_shape(groups[i].sched).llr()) {
            rc = mbx_burst_validate(groups[i].sched, groups[i].bursts, groups[i].burst_stride, (size_t)gp.place[i].bursts, c.soft ? 1 : 0);
            if (rc < 0) {
                return rc;
            }
        }
    }
    if (gp.total_rows == 0) {
        return 0;
    }
    return on_next_slot(s, [&](Slot& sl) { return enqueue_groups(s, sl, c, groups, gp); });
}

}  // extern "C"
