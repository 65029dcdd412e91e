// session_plan_check.cpp -- mbelib-neo_amd/csrc/mbx_session_plan.h held, on the CPU, to the formulas it took over from mbx_session.hip
// and to the properties of the layout, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_session_plan_host.py.
// A program of its own: nothing of the library is linked.
//   * the output table against the allocation ladder, the staging sizes and the copy-out sizes as the session unit had them written
//     out, for every subset of the six session flags;
//   * the refusals of a frames, a bursts and a group submit against the if-chains the unit had, in their order, over n, T, streams and
//     max_frames around their bounds, every subset of the flags against every subset of the outputs a caller can name, and the texts;
//   * the stream-index walks against the loops the unit had, on a `seen` array of exactly `streams` heap bytes;
//   * the byte layout of a group submit against the loop the unit had -- every (bursts 0..3, stride at / above / far above the
//     schedule's bytes, pinned x aligned, index or none) per group for 0..3 groups, every one of them at every place of 4..8 groups,
//     hard and soft -- and to its properties: offsets 16-byte aligned, regions disjoint and inside the total, the schedule's bytes of
//     the last hard burst, nothing of a group without bursts, the index words of the groups tiling [0, total_streams).
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "mbx_session_plan.h"

namespace {

using namespace mbx;

unsigned long long g_cases = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

// ---- the output table ---------------------------------------------------------------------------------------------------------------------
void outputs() {
    const size_t mf = 7;
    for (unsigned flags = 0; flags < 64; ++flags) {
        // the ladder of create_session: d_records always; the others by flag
        const bool owned[kOutCount] = {
            (flags & (MBX_SESSION_PCM16 | MBX_SESSION_PCM8 | MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS)) != 0,
            (flags & MBX_SESSION_PCMF) != 0,
            (flags & MBX_SESSION_RESULTS) != 0,
            true,
            (flags & MBX_SESSION_PCM8) != 0,
            (flags & MBX_SESSION_MIXDOWN) != 0,
            (flags & MBX_SESSION_LEVELS) != 0,
        };
        for (int k = 0; k < kOutCount; ++k) {
            CHECK(out_owned(k, flags) == owned[k]);
        }
        ++g_cases;
    }
    // ... with these sizes, on the device and in the staging (max_frames rows of the output's widest row)
    const size_t capacity[kOutCount] = {mf * 160 * sizeof(int16_t), mf * 160 * sizeof(float), mf * sizeof(mbe_process_result), mf * sizeof(mbx_param_record),
                                        mf * 160, mf * 160 * sizeof(int16_t), mf * sizeof(mbx_row_level)};
    for (int k = 0; k < kOutCount; ++k) {
        CHECK(out_capacity(k, mf) == capacity[k]);
    }
    // what copy_out moved: rows * per_frame * sizeof(element); the mix: the plan's buses of 320 or 160 bytes by form
    for (size_t nf = 0; nf <= mf; ++nf) {
        for (size_t buses = 0; buses <= mf; ++buses) {
            for (int form : {MBX_MIXDOWN_PCM16, MBX_MIXDOWN_ULAW, MBX_MIXDOWN_ALAW}) {
                const size_t bytes[kOutCount] = {nf * 160 * sizeof(int16_t), nf * 160 * sizeof(float), nf * 1 * sizeof(mbe_process_result),
                                                 nf * 1 * sizeof(mbx_param_record), nf * 160 * sizeof(uint8_t),
                                                 buses * (form == MBX_MIXDOWN_PCM16 ? 320 : 160) * sizeof(uint8_t), nf * 1 * sizeof(mbx_row_level)};
                for (int k = 0; k < kOutCount; ++k) {
                    CHECK(out_bytes(k, nf, buses, form) == bytes[k]);
                    CHECK(bytes[k] <= capacity[k]);   // (what goes out fits the buffers it goes through)
                }
                ++g_cases;
            }
        }
    }
}

// ---- the refusals ---------------------------------------------------------------------------------------------------------------------------
// (the if-chain of submit(), with the enum in place of its returns)
SessionRefusal frames_as_written(bool session, bool mixed, bool frames, int n, int T, int streams, size_t max_frames, unsigned outputs, bool pcm16,
                                 bool pcmf, bool results, bool buses, int plan_rows) {
    if (session && mixed) {
        return kSessionMixed;
    }
    if (!session || !frames || n < 0 || T < 0 || n > streams || (size_t)n * (size_t)T > max_frames) {
        return kSessionArguments;
    }
    if ((pcm16 && !(outputs & MBX_SESSION_PCM16)) || (pcmf && !(outputs & MBX_SESSION_PCMF)) || (results && !(outputs & MBX_SESSION_RESULTS))) {
        return kSessionOutput;
    }
    if (buses && (size_t)n * (size_t)T < (size_t)plan_rows) {
        return kSessionRowsShort;
    }
    if (n == 0 || T == 0) {
        return kSessionNothing;
    }
    return kSessionOk;
}

void frames_submits() {
    for (int session = 0; session < 2; ++session) {
        for (int mixed = 0; mixed < 2; ++mixed) {
            for (int frames = 0; frames < 2; ++frames) {
                for (int streams : {1, 4}) {
                    for (int n : {-1, 0, 1, streams - 1, streams, streams + 1}) {
                        for (int T : {-1, 0, 1, 2, 3}) {
                            for (size_t max_frames : {(size_t)1, (size_t)4, (size_t)8, (size_t)12}) {
                                for (int plan_rows : {0, 1, 5, 9}) {   // (0: no buses attached)
                                    for (unsigned flags = 0; flags < 64; ++flags) {
                                        for (unsigned want = 0; want < 8; ++want) {
                                            SessionShape s;
                                            s.session = session, s.mixed = mixed, s.streams = streams, s.max_frames = max_frames, s.flags = flags;
                                            s.requested = requested_outputs(want & 1, want & 2, want & 4);
                                            s.plan_rows = plan_rows;
                                            CHECK(frames_submit_refused(s, frames, n, T) ==
                                                  frames_as_written(session, mixed, frames, n, T, streams, max_frames, flags, want & 1, want & 2, want & 4,
                                                                    plan_rows != 0, plan_rows));
                                            ++g_cases;
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    CHECK(requested_outputs(true, false, false) == MBX_SESSION_PCM16 && requested_outputs(false, true, false) == MBX_SESSION_PCMF &&
          requested_outputs(false, false, true) == MBX_SESSION_RESULTS && requested_outputs(false, false, false) == 0u);
}

// (the if-chain of submit_bursts())
SessionRefusal bursts_as_written(bool session, bool sched, bool bursts, int n, bool mixed, int codec, int device, int s_codec, int s_device, bool soft,
                                 bool llr, size_t stride, size_t bytes, bool index, int streams, int frames, size_t max_frames) {
    if (!session || !sched || !bursts || n < 0) {
        return kSessionArguments;
    }
    if (mixed) {
        return kSessionMixed;
    }
    if (codec != s_codec || device != s_device) {
        return kBurstsSchedule;
    }
    if (!soft && llr) {
        return kBurstsLlrHard;
    }
    if (!soft && stride < bytes) {
        return kBurstsStride;
    }
    if ((!index && n != streams) || (size_t)n * (size_t)frames > max_frames) {
        return kBurstsCount;
    }
    return kSessionOk;
}

void bursts_submits() {
    const int streams = 4;
    for (unsigned bits = 0; bits < 512; ++bits) {   // session, sched, bursts, mixed, soft, llr, index, the schedule's codec and device the session's or not
        for (int n : {-1, 0, streams - 1, streams, streams + 1}) {
            for (size_t stride : {(size_t)36, (size_t)37, (size_t)38}) {
                for (int frames : {1, 3}) {
                    for (size_t max_frames : {(size_t)3, (size_t)4, (size_t)11, (size_t)12}) {
                        SessionShape s;
                        BurstsShape b;
                        s.session = bits & 1, s.mixed = bits & 8, s.streams = streams, s.max_frames = max_frames;
                        b.sched = bits & 2, b.bursts = bits & 4, b.soft = bits & 16, b.llr = bits & 32, b.indexed = bits & 64;
                        b.n = n, b.frames = frames, b.codec = bits & 128 ? 1 : 0, b.device = bits & 256 ? 2 : 0;
                        b.stride = stride, b.sched_bytes = 37;
                        CHECK(bursts_submit_refused(s, b) == bursts_as_written(s.session, b.sched, b.bursts, n, s.mixed, b.codec, b.device, 0, 0, b.soft, b.llr,
                                                                               stride, 37, b.indexed, streams, frames, max_frames));
                        ++g_cases;
                    }
                }
            }
        }
    }
}

void groups_submits() {
    for (unsigned flags = 0; flags < 64; ++flags) {
        for (unsigned want = 0; want < 8; ++want) {
            for (size_t max_frames : {(size_t)1, (size_t)5}) {
                for (int32_t total_rows : {0, 1, 4, 5, 6, 0x7fffffff}) {
                    for (int plan_rows : {0, 1, 5, 6}) {
                        SessionShape s;
                        s.session = true, s.max_frames = max_frames, s.flags = flags, s.plan_rows = plan_rows;
                        s.requested = requested_outputs(want & 1, want & 2, want & 4);
                        // (the if-chain of mbx_session_submit_burst_groups, between the groups' own plan and the walk over the streams)
                        SessionRefusal as_written = kSessionOk;
                        if (((want & 1) && !(flags & MBX_SESSION_PCM16)) || ((want & 2) && !(flags & MBX_SESSION_PCMF)) ||
                            ((want & 4) && !(flags & MBX_SESSION_RESULTS))) {
                            as_written = kGroupsOutput;
                        } else if ((size_t)total_rows > max_frames) {
                            as_written = kGroupsTooManyFrames;
                        } else if (plan_rows != 0 && (size_t)total_rows < (size_t)plan_rows) {
                            as_written = kSessionRowsShort;
                        }
                        CHECK(groups_submit_refused(s, total_rows) == as_written);
                        ++g_cases;
                    }
                }
            }
        }
    }
}

void texts() {
    // byte for byte what the session unit set, behind "<who>: "; the three without a text set none
    const struct {
        SessionRefusal r;
        const char*    text;
    } all[] = {
        {kSessionOk, ""},
        {kSessionNothing, ""},
        {kSessionArguments, ""},
        {kSessionOutput, ""},
        {kSessionMixed, "a mixed session takes burst groups only (mbx_session_submit_burst_groups)"},
        {kSessionRowsShort, "the submit has %zu rows, the mix-down plan attached to it needs %d (mbx_session_next_mixdown)"},
        {kSessionNoSession, "no session"},
        {kSessionIndex, "stream index out of range or listed twice"},
        {kBurstsSchedule, "the schedule is of another codec or device than the session"},
        {kBurstsLlrHard, "an LLR schedule has soft bursts only"},
        {kBurstsStride, "burst_stride is below mbx_burst_schedule_bytes()"},
        {kBurstsCount, "without an index n is the session's stream count; n * frames_per_burst <= max_frames_per_submit"},
        {kGroupsOutput, "an output the session was not created for"},
        {kGroupsTooManyFrames, "more frames than max_frames_per_submit"},
        {kGroupsDevice, "a schedule of another device than the session"},
        {kGroupsCodec, "a schedule of another codec than a stream its group names"},
    };
    CHECK(sizeof(all) / sizeof(all[0]) == (size_t)kGroupsCodec + 1);
    for (const auto& a : all) {
        CHECK(strcmp(session_refusal_text(a.r), a.text) == 0);
        ++g_cases;
    }
}

// ---- the stream-index walks -------------------------------------------------------------------------------------------------------------------
// `seen` on the heap, exactly `streams` bytes: a mark outside it is the sanitizer's to report
struct Seen {
    uint8_t* p;
    int      streams;
    explicit Seen(int n) : p(static_cast<uint8_t*>(calloc((size_t)n, 1))), streams(n) { CHECK(p != nullptr); }
    ~Seen() { free(p); }
    void clear() { memset(p, 0, (size_t)streams); }
};

// (the loop of submit())
bool plain_as_written(uint8_t* seen, int streams, const int32_t* index, int n) {
    for (int i = 0; i < n; ++i) {
        if (index[i] < 0 || index[i] >= streams || seen[(size_t)index[i]]) {
            return false;
        }
        seen[(size_t)index[i]] = 1;
    }
    return true;
}
// (the inner loop of mbx_session_submit_burst_groups; mixed: the codec of every stream, else the session's)
SessionRefusal group_as_written(uint8_t* seen, int streams, const int32_t* index, int first_slot, int n, bool mixed, const uint8_t* stream_codec, int codec,
                                int sched_codec) {
    for (int j = 0; j < n; ++j) {
        const long long slot = index ? (long long)index[j] : (long long)first_slot + j;
        if (slot < 0 || slot >= streams || seen[(size_t)slot]) {
            return kSessionIndex;
        }
        seen[(size_t)slot] = 1;
        if ((mixed ? (int)stream_codec[(size_t)slot] : codec) != sched_codec) {
            return kGroupsCodec;
        }
    }
    return kSessionOk;
}

void walks() {
    for (int streams = 1; streams <= 4; ++streams) {
        Seen a(streams), b(streams);
        const uint8_t codecs[4] = {1, 3, 1, 0};
        for (int n = 0; n <= 4; ++n) {
            // every index of n words over -1 .. streams, and two far values
            const int32_t values[8] = {-1, 0, 1, 2, 3, 4, INT_MIN, INT_MAX};
            const int     nv = streams + 2 <= 6 ? streams + 2 : 6;
            int           digit[4] = {0, 0, 0, 0};
            for (;;) {
                int32_t index[4];
                bool    in_range = true, twice = false;
                for (int i = 0; i < n; ++i) {
                    index[i] = digit[i] < nv ? values[digit[i]] : values[6 + digit[i] - nv];
                    in_range = in_range && index[i] >= 0 && index[i] < streams;
                    for (int k = 0; k < i; ++k) {
                        twice = twice || index[k] == index[i];
                    }
                }
                a.clear(), b.clear();
                const SessionRefusal got = mark_streams(a.p, streams, index, n);
                CHECK((got == kSessionOk) == plain_as_written(b.p, streams, index, n) && (got == kSessionOk || got == kSessionIndex));
                CHECK((got == kSessionOk) == (in_range && !twice));   // refused: exactly a slot out of range or named twice
                CHECK(memcmp(a.p, b.p, (size_t)streams) == 0);
                ++g_cases;
                // the same words as a group's index, on a single-codec and on a mixed session
                for (int mixed = 0; mixed < 2; ++mixed) {
                    for (int sched_codec : {0, 1}) {
                        a.clear(), b.clear();
                        const SessionRefusal g = mark_group(a.p, streams, index, 99, n, mixed ? codecs : nullptr, 1, sched_codec);
                        CHECK(g == group_as_written(b.p, streams, index, 99, n, mixed, codecs, 1, sched_codec));
                        CHECK(memcmp(a.p, b.p, (size_t)streams) == 0 && (in_range && !twice ? g != kSessionIndex : true));
                        ++g_cases;
                    }
                }
                int at = 0;
                while (at < n && ++digit[at] == nv + 2) {
                    digit[at++] = 0;
                }
                if (at == n) {
                    break;
                }
            }
            // a group named by its first slot: a run of n slots from every start around the pool, and from the ends of int
            for (int first : {-2, -1, 0, 1, 2, 3, 4, 5, INT_MAX - 1, INT_MAX, INT_MIN}) {
                for (int mixed = 0; mixed < 2; ++mixed) {
                    for (int taken = -1; taken < streams; ++taken) {   // a slot an earlier group of the call took, or none
                        a.clear(), b.clear();
                        if (taken >= 0) {
                            a.p[taken] = b.p[taken] = 1;
                        }
                        const SessionRefusal g = mark_group(a.p, streams, nullptr, first, n, mixed ? codecs : nullptr, 1, 1);
                        CHECK(g == group_as_written(b.p, streams, nullptr, first, n, mixed, codecs, 1, 1));
                        const bool fits = n == 0 || (first >= 0 && (long long)first + n <= streams && !(taken >= first && taken < first + n));
                        CHECK((g != kSessionIndex) == fits || (g == kGroupsCodec && mixed));   // (a codec refusal ends the walk before a later bad slot)
                        CHECK(memcmp(a.p, b.p, (size_t)streams) == 0);
                        ++g_cases;
                    }
                }
            }
        }
    }
}

// ---- the byte layout of a group submit --------------------------------------------------------------------------------------------------------
const size_t kSchedBytes[kMaxBurstGroups] = {37, 48, 1, 160, 16, 9, 333, 64};   // the schedule of the group at each place: its smallest hard stride
const size_t kSoftBytes[kMaxBurstGroups] = {2 * 290, 312, 2, 1280, 128, 72, 2664, 512};   // ... and one soft burst of it

struct GroupCase {   // one group of a call, as the session unit saw it
    uint32_t bursts;
    size_t   stride;
    bool     pinned, aligned, index;
};
// every (bursts, stride, pinned, aligned, index) of one group: 4 * 3 * 2 * 2 * 2 = 96
const int kCombos = 96;
GroupCase combo(int c, size_t sched_bytes) {
    GroupCase g;
    g.bursts = (uint32_t)(c % 4), c /= 4;
    g.stride = sched_bytes + (c % 3 == 0 ? 0 : (c % 3 == 1 ? 1 : 4096)), c /= 3;
    g.pinned = c & 1, g.aligned = c & 2, g.index = c & 4;
    return g;
}

void check_layout(const GroupCase* g, int n, bool soft) {
    // the loop of enqueue_groups, as it was written
    size_t at[kMaxBurstGroups], bytes[kMaxBurstGroups], total = 0;
    bool   staged = false, indexed = false;
    for (int i = 0; i < n; ++i) {
        const size_t per = soft ? kSoftBytes[i] : g[i].stride;
        at[i] = total;
        bytes[i] = g[i].bursts ? ((size_t)g[i].bursts - 1) * per + (soft ? per : kSchedBytes[i]) : 0;
        total = (total + bytes[i] + 15) & ~(size_t)15;
        if (bytes[i] && (!g[i].pinned || !g[i].aligned)) {
            staged = true;
        }
        indexed = indexed || (g[i].bursts && g[i].index);
    }
    GroupIn    in[kMaxBurstGroups];
    GroupShape shapes[kMaxBurstGroups];
    for (int i = 0; i < n; ++i) {
        in[i].bursts = g[i].bursts, in[i].per = soft ? kSoftBytes[i] : g[i].stride, in[i].sched_bytes = soft ? 0 : kSchedBytes[i];
        in[i].in_place = g[i].bursts && g[i].pinned && g[i].aligned, in[i].has_index = g[i].index;
        shapes[i].n_streams = (int)g[i].bursts, shapes[i].bursts_per_stream = 1;
    }
    const GroupBytes lay = group_bytes(in, n, soft);
    CHECK(lay.total == total && lay.staged == staged && lay.indexed == indexed);
    GroupPlan plan;
    CHECK(plan_groups(shapes, n, &plan) == kGroupsOk);
    size_t  end = 0;
    int32_t stream = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(lay.at[i] == at[i] && lay.bytes[i] == bytes[i]);
        CHECK(lay.at[i] % 16 == 0 && lay.at[i] >= end && lay.at[i] + lay.bytes[i] <= lay.total);   // aligned, behind the group before it, inside the total
        end = lay.at[i] + lay.bytes[i];
        if (!g[i].bursts) {
            CHECK(lay.bytes[i] == 0);   // nothing of it is read, whatever its pointer is
        } else if (soft) {
            CHECK(lay.bytes[i] == (size_t)g[i].bursts * kSoftBytes[i]);
        } else {   // of the last hard burst the schedule's bytes, not its stride
            CHECK(lay.bytes[i] == ((size_t)g[i].bursts - 1) * g[i].stride + kSchedBytes[i] && lay.bytes[i] <= (size_t)g[i].bursts * g[i].stride);
        }
        // the index words of the groups tile [0, total_streams): group i has n_streams words from its first stream row
        CHECK(plan.place[i].first_stream == stream && plan.place[i].bursts == g[i].bursts);
        stream += shapes[i].n_streams;
    }
    CHECK(plan.total_streams == stream && lay.total % 16 == 0 && lay.total < end + 16);
    ++g_cases;
}

void layouts() {
    GroupCase g[kMaxBurstGroups];
    for (int soft = 0; soft < 2; ++soft) {
        check_layout(g, 0, soft != 0);
        for (int a = 0; a < kCombos; ++a) {
            g[0] = combo(a, kSchedBytes[0]);
            check_layout(g, 1, soft != 0);
            for (int b = 0; b < kCombos; ++b) {
                g[1] = combo(b, kSchedBytes[1]);
                check_layout(g, 2, soft != 0);
                for (int c = 0; c < kCombos; ++c) {
                    g[2] = combo(c, kSchedBytes[2]);
                    check_layout(g, 3, soft != 0);
                }
            }
        }
        // 4 .. 8 groups: every combination at every place, the other places walking through the combinations beside it
        for (int n = 4; n <= kMaxBurstGroups; ++n) {
            for (int place = 0; place < n; ++place) {
                for (int c = 0; c < kCombos; ++c) {
                    for (int i = 0; i < n; ++i) {
                        g[i] = combo(i == place ? c : (c * 7 + i * 29 + n) % kCombos, kSchedBytes[i]);
                    }
                    check_layout(g, n, soft != 0);
                }
            }
        }
    }
}

}  // namespace

int main() {
    outputs();
    frames_submits();
    bursts_submits();
    groups_submits();
    texts();
    walks();
    layouts();
    printf("session_plan_check: %llu cases ok\n", g_cases);
    return 0;
}
