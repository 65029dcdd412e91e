// mbx_session_plan.h -- what a session (mbx_session.hip) decides with integers alone: which buffers a set of session flags owns and how
// many bytes of each go out, what a submit is refused for and in which order, whether an index names every stream once, and where the
// bursts of a group submit lie in the slot's burst buffer.
// Integer work on the host alone: no HIP, no locks, no globals -- so that a CPU program can check it under a sanitizer
// (tests/session_plan_check.cpp), in the manner of mbx_group_plan.h.  Private to mbx_session.hip; nothing here is exported.
#pragma once

#include <cstddef>
#include <cstdint>

#include <mbx.h>           // (the public headers: the session flags and the records the outputs are made of)
#include <mbx_bands.h>
#include <mbx_levels.h>
#include <mbx_mixdown.h>
#include <mbx_pcm8.h>

#include "mbx_group_plan.h"

namespace mbx {

// ---- the outputs of a slot ------------------------------------------------------------------------------------------------------------
enum SessionOut { kOutPcm16 = 0, kOutPcmf, kOutResults, kOutRecords, kOutPcm8, kOutMix, kOutLevels, kOutCount };
struct OutFacts {
    unsigned owners;      // the session flags that make a slot own the device buffer; 0: every session
    size_t   row_bytes;   // bytes per row, of the device buffer and of its pinned staging: max_frames rows each
};
// (the step writes int16; the compand, the mix-down and the levels read it.  A bus row in the staging is 320 B whatever its form.)
constexpr OutFacts kOutFacts[kOutCount] = {
    {MBX_SESSION_PCM16 | MBX_SESSION_PCM8 | MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS, 160 * sizeof(int16_t)},
    {MBX_SESSION_PCMF, 160 * sizeof(float)},
    {MBX_SESSION_RESULTS, sizeof(mbe_process_result)},
    {0u, sizeof(mbx_param_record)},
    {MBX_SESSION_PCM8, 160},
    {MBX_SESSION_MIXDOWN, 160 * sizeof(int16_t)},
    {MBX_SESSION_LEVELS, sizeof(mbx_row_level)},
};
static inline bool out_owned(int which, unsigned flags) { return kOutFacts[which].owners == 0u || (flags & kOutFacts[which].owners) != 0u; }
static inline size_t out_capacity(int which, size_t max_frames) { return max_frames * kOutFacts[which].row_bytes; }
// what goes to the caller of a submit of nf rows: nf rows of everything but the mix, of which the plan's buses go, 320 or 160 B by form
static inline size_t out_bytes(int which, size_t nf, size_t buses, int mix_form) {
    if (which == kOutMix) {
        return buses * (mix_form == MBX_MIXDOWN_PCM16 ? 320u : 160u);
    }
    return nf * kOutFacts[which].row_bytes;
}
// the wide buses of a submit (mbx_session_next_resample, include/mbx_resample.h) are no entry of the table: their buffer belongs to the
// slot's first resampled submit and is sized by that submit -- `buses` rows of 160 * L int16, on the device and in the pinned staging
static inline size_t wide_bytes(size_t buses, unsigned L) { return buses * 160u * (size_t)L * sizeof(int16_t); }
// the band records of a submit (mbx_session_next_bands, include/mbx_bands.h) are no entry of the table either: their buffer belongs to
// the slot's first submit with a bank, is sized by max_frames_per_submit rows of that bank and form -- band_bytes(max_frames, K, form),
// on the device and in the pinned staging -- and is made anew when a later bank needs more; band_bytes(nf, K, form) of it go out
static inline size_t band_bytes(size_t nf, int K, int form) { return nf * (size_t)K * (form == MBX_BANDS_COMPLEX ? sizeof(mbx_band_record) : sizeof(uint32_t)); }
// the outputs a caller may name in a submit, as the session flags they need
static inline unsigned requested_outputs(bool pcm16, bool pcmf, bool results) {
    return (pcm16 ? MBX_SESSION_PCM16 : 0u) | (pcmf ? MBX_SESSION_PCMF : 0u) | (results ? MBX_SESSION_RESULTS : 0u);
}

// ---- what a submit is refused for -----------------------------------------------------------------------------------------------------
enum SessionRefusal {
    kSessionOk = 0,
    kSessionNothing,          // accepted with nothing to do: the call returns 0 and queues nothing
    kSessionArguments,        // a NULL, negative or oversized argument of a frames or bursts submit: no text
    kSessionOutput,           // a frames submit names an output the session was not created for: no text
    kSessionRowsShort,        // (the text is a format: the rows of the submit, %zu, and of the plan, %d)
    kSessionMixed, kSessionNoSession, kSessionIndex,                     // ... and the refusals with a text: of every submit,
    kBurstsSchedule, kBurstsLlrHard, kBurstsStride, kBurstsCount,        // of a bursts submit,
    kGroupsOutput, kGroupsTooManyFrames, kGroupsDevice, kGroupsCodec,    // of a group submit
};
// "<who>: <text>"; an empty text: the refusal sets none
static inline const char* session_refusal_text(SessionRefusal r) {
    switch (r) {
    case kSessionMixed: return "a mixed session takes burst groups only (mbx_session_submit_burst_groups)";
    case kSessionRowsShort: return "the submit has %zu rows, the mix-down plan attached to it needs %d (mbx_session_next_mixdown)";
    case kSessionNoSession: return "no session";
    case kSessionIndex: return "stream index out of range or listed twice";
    case kBurstsSchedule: return "the schedule is of another codec or device than the session";
    case kBurstsLlrHard: return "an LLR schedule has soft bursts only";
    case kBurstsStride: return "burst_stride is below mbx_burst_schedule_bytes()";
    case kBurstsCount: return "without an index n is the session's stream count; n * frames_per_burst <= max_frames_per_submit";
    case kGroupsOutput: return "an output the session was not created for";
    case kGroupsTooManyFrames: return "more frames than max_frames_per_submit";
    case kGroupsDevice: return "a schedule of another device than the session";
    case kGroupsCodec: return "a schedule of another codec than a stream its group names";
    default: return "";
    }
}

// what every submit is held to once its rows are known: the session's sizes and flags, the outputs the caller names
// (requested_outputs), and the rows the mix-down plan attached to the call needs (0: none attached)
struct SessionShape {
    bool     session = false, mixed = false;
    int      streams = 0;
    size_t   max_frames = 0;
    unsigned flags = 0, requested = 0;
    int      plan_rows = 0;
};

// a frames submit (and what a keyed or a bursts submit has become): n streams of T frames from `input`
static inline SessionRefusal frames_submit_refused(const SessionShape& s, bool input, int n, int T) {
    if (s.session && s.mixed) {
        return kSessionMixed;
    }
    if (!s.session || !input || n < 0 || T < 0 || n > s.streams || (size_t)n * (size_t)T > s.max_frames) {
        return kSessionArguments;
    }
    if ((s.requested & ~s.flags) != 0u) {
        return kSessionOutput;
    }
    if ((size_t)n * (size_t)T < (size_t)s.plan_rows) {
        return kSessionRowsShort;
    }
    return n == 0 || T == 0 ? kSessionNothing : kSessionOk;
}

// a bursts submit, in front of the frames submit it becomes: the schedule's facts are looked at only where there is a schedule
struct BurstsShape {
    bool   sched = false, bursts = false, soft = false, llr = false, indexed = false;
    int    n = 0, frames = 0;                     // bursts, and the schedule's frames per burst
    int    codec = 0, device = 0;                 // of the schedule
    int    session_codec = 0, session_device = 0;
    size_t stride = 0, sched_bytes = 0;           // the caller's burst_stride and the schedule's smallest
};
static inline SessionRefusal bursts_submit_refused(const SessionShape& s, const BurstsShape& b) {
    if (!s.session || !b.sched || !b.bursts || b.n < 0) {
        return kSessionArguments;
    }
    if (s.mixed) {
        return kSessionMixed;
    }
    if (b.codec != b.session_codec || b.device != b.session_device) {
        return kBurstsSchedule;
    }
    if (!b.soft && b.llr) {
        return kBurstsLlrHard;
    }
    if (!b.soft && b.stride < b.sched_bytes) {
        return kBurstsStride;
    }
    if ((!b.indexed && b.n != s.streams) || (size_t)b.n * (size_t)b.frames > s.max_frames) {
        return kBurstsCount;
    }
    return kSessionOk;
}

// a group submit whose groups are placed (mbx_group_plan.h), in front of the walk over its streams
static inline SessionRefusal groups_submit_refused(const SessionShape& s, int32_t total_rows) {
    if ((s.requested & ~s.flags) != 0u) {
        return kGroupsOutput;
    }
    if ((size_t)total_rows > s.max_frames) {
        return kGroupsTooManyFrames;
    }
    return (size_t)total_rows < (size_t)s.plan_rows ? kSessionRowsShort : kSessionOk;
}

// ---- every row names its own stream: two rows on one stream would race on its state ---------------------------------------------------
// `seen`: one byte per stream, zero before the first walk of a call; a walk marks the streams it accepts.
// One group: its streams by `index` or, without one, first_slot + j; its schedule's codec is that of every stream it names
// (stream_codec: the codec of every stream of a mixed session; nullptr: all of session_codec)
static inline SessionRefusal mark_group(uint8_t* seen, int streams, const int32_t* index, int first_slot, int n, const uint8_t* stream_codec,
                                        int session_codec, int sched_codec) {
    for (int j = 0; j < n; ++j) {
        const long long slot = index ? (long long)index[j] : (long long)first_slot + j;
        if (slot < 0 || slot >= streams || seen[(size_t)slot]) {
            return kSessionIndex;
        }
        seen[(size_t)slot] = 1;
        if ((stream_codec ? (int)stream_codec[(size_t)slot] : session_codec) != sched_codec) {
            return kGroupsCodec;
        }
    }
    return kSessionOk;
}
// ... and the plain form: the n rows of an indexed frames submit, which ask nothing of a codec
static inline SessionRefusal mark_streams(uint8_t* seen, int streams, const int32_t* index, int n) {
    return mark_group(seen, streams, index, 0, n, nullptr, 0, 0);
}

// ---- where the bursts of a group submit lie ---------------------------------------------------------------------------------------------
// Each group at a 16-byte aligned offset of the slot's burst buffer, and of its pinned staging.  Of the last hard burst only the
// schedule's bytes are there to read, not its whole stride; a group without bursts has no bytes and is never read.
struct GroupIn {
    uint32_t bursts = 0;         // n_streams * bursts_per_stream (GroupPlace)
    size_t   per = 0;            // one burst in the input: the caller's burst_stride, or the schedule's soft bytes
    size_t   sched_bytes = 0;    // hard: the schedule's smallest burst_stride
    bool     in_place = false;   // the bursts are pinned and 16-byte aligned: read where they are
    bool     has_index = false;
};
struct GroupBytes {
    size_t at[kMaxBurstGroups] = {}, bytes[kMaxBurstGroups] = {}, total = 0;
    bool   staged = false;    // a group goes through the pinned staging
    bool   indexed = false;   // a group with bursts names its streams by an index
};
static inline GroupBytes group_bytes(const GroupIn* g, int n_groups, bool soft) {
    GroupBytes out;
    for (int i = 0; i < n_groups; ++i) {
        out.at[i] = out.total;
        out.bytes[i] = g[i].bursts ? ((size_t)g[i].bursts - 1) * g[i].per + (soft ? g[i].per : g[i].sched_bytes) : 0;
        out.total = (out.total + out.bytes[i] + 15) & ~(size_t)15;
        out.staged = out.staged || (out.bytes[i] && !g[i].in_place);
        out.indexed = out.indexed || (g[i].bursts && g[i].has_index);
    }
    return out;
}

}  // namespace mbx
