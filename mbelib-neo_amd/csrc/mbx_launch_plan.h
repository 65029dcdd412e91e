// mbx_launch_plan.h -- what a batch step launches, decided in ONE function: plan_step.  The launchers of mbx_api.hip make their own
// argument checks, say what they know of the step in a StepShape, plan once, grow the workspace to the plan's size and issue the plan;
// mbx_uses_expand_launch, mbx_launch_slices, mbx_batch_kernel_name and mbx_stream_kernel_name answer from the same function.
// Integer work on the host alone: no HIP, no locks, no globals, the environment read in one function -- so that a CPU program can
// check it under a sanitizer (tests/launch_plan_check.cpp holds it to the answers of the code it replaced and to its properties).
// What it needs from the device headers comes as plain numbers (DeviceFacts, filled by the launcher).  Private to mbx_api.hip; nothing
// here is exported.  The tables of kernel pointers stay in mbx_api.hip: a plan names its kernel by index.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdlib>

#include "mbx_codec.h"

namespace mbx {

// ---- the launch switches (development, A/B timing), read once per process by the launcher ---------------------------------------
struct LaunchSwitches {
    int  lds_min_frames = 4;      // MBX_LDS_MIN_FRAMES: frames per stream from which the LDS-resident instances are used
    bool res1 = true;             // MBX_NO_RES1 (by presence): resident one-frame launches through the *_res1 instances
    bool lds_resident = true;     // MBX_NO_LDS_RESIDENT (by presence)
    int  slice = -1;              // MBX_SLICE: 0 switches sliced launches off, n > 0 sets the slice length in frames; -1: the launcher's own rule
    int  slice_groups = 3;        // MBX_SLICE_GROUPS: groups of streams of a sliced launch, 2..4
    bool slice_own = true;        // MBX_SLICE_OWN=0: every group on an internal stream, none on the caller's
    bool ragged_order = true;     // MBX_RAGGED_ORDER=0: no order kernel, grid order (A/B timing and the byte test)
    int  fuse_one = 2;            // MBX_FUSE_ONE: the one-launch forms of a T = 1 step, see plan_step
    int  front_lead = INT_MAX;    // MBX_FRONT_LEAD: by how many chunks of eight streams a front block runs ahead of its stream blocks
};
// THE place the switches are read.  (MBX_NO_REVERSE and MBX_DISABLE_TONES are not plan inputs: they start atomics of mbx_api.hip.)
static inline LaunchSwitches read_launch_switches() {
    LaunchSwitches s;
    if (const char* e = getenv("MBX_LDS_MIN_FRAMES")) {
        const int n = atoi(e);
        s.lds_min_frames = (n >= 1 && n <= 1 << 20) ? n : 4;   // anything else (0, negative, not a number) is ignored
    }
    s.res1 = getenv("MBX_NO_RES1") == nullptr;
    s.lds_resident = getenv("MBX_NO_LDS_RESIDENT") == nullptr;
    if (const char* e = getenv("MBX_SLICE")) {
        s.slice = atoi(e);
    }
    if (const char* e = getenv("MBX_SLICE_GROUPS")) {
        const int v = atoi(e);
        s.slice_groups = v < 2 ? 2 : (v > 4 ? 4 : v);
    }
    if (const char* e = getenv("MBX_SLICE_OWN")) {
        s.slice_own = e[0] != '0';
    }
    if (const char* e = getenv("MBX_RAGGED_ORDER")) {
        s.ragged_order = e[0] != '0';
    }
    if (const char* e = getenv("MBX_FUSE_ONE")) {
        s.fuse_one = (e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 2;
    }
    if (const char* e = getenv("MBX_FRONT_LEAD")) {
        const int v = atoi(e);
        s.front_lead = v < 0 ? 0 : v;
    }
    return s;
}

// ---- what the launcher knows of a codec beyond its shape (mbx_codec.h), without the kernels (kCodecKernels, mbx_api.hip) ----------
// rows of kInstances (mbx_api.hip) by their first entry; a row's columns: IMBE 7200x4400 | AMBE 3600x2450 | AMBE 3600x2400 (the two
// fused rows: IMBE 7200x4400 | IMBE 7100x4400, the only codecs with a front end of their own inside the stream's wave)
enum Row { kPlain = 0, kOne = 3, kLds = 6, kRes = 9, kRes1 = 12, kSlice = 15, kOneLaunch = 18, kOneLaunchRes = 21, kOneFused = 24, kRes1Fused = 26 };
constexpr int kInstanceCount = kRes1Fused + 2;
struct CodecLaunch {
    int column;         // of the stream stage in the three-column rows of kInstances (and of kRagged); -1: no stream stage of its own
    int fused_column;   // the IMBE codecs -- a front end inside the stream's wave, a stream kernel that expands a record itself --:
                        // their column in the two fused rows; -1: an AMBE codec
};
constexpr CodecLaunch kCodecLaunch[4] = {{0, 0}, {1, -1}, {-1, 1}, {2, -1}};   // indexed by MBX_CODEC_*
static inline bool imbe_codec(int codec) { return codec_shape(codec) && kCodecLaunch[codec].fused_column >= 0; }
// the codec whose stream stage a codec's frames end in (a codec that is none of the four is rejected before any launch; the names'
// functions answer for it as for AMBE 3600x2450, as they always have)
static inline int stream_codec_of(int codec) {
    const CodecShape* sh = codec_shape(codec);
    return sh ? sh->stream : MBX_CODEC_AMBE3600X2450;
}

// the device headers' figures, as numbers
struct DeviceFacts {
    int    simds;            // 4 per CU; 0: no device context (a prediction then knows no wave slots: nothing is sliced)
    int    imbe_lds_waves;   // resident waves per SIMD of the kernel a long launch takes: MBX_IMBE_LDS_WAVES_PER_SIMD ...
    int    ambe_lds_waves;   // ... MBX_AMBE_LDS_WAVES_PER_SIMD (the kernels' own launch bounds: mbx_device.h)
    size_t row_bytes;        // sizeof(FrameParams)
};

// ---- a step as its caller knows it ---------------------------------------------------------------------------------------------
//   kRecords: the records are there;  kFrames: packed hard frames, a FEC launch in front -- or the whole T = 1 step as ONE launch;
//   kSoft: soft cells, a soft front launch (one wave per frame) in front.  Codec 2 records come out in 7200x4400 order; codec 3 frames
//   take the AMBE front end and are expanded by the 3600x2400 rules.
enum InputKind { kRecords, kFrames, kSoft };
//   A VOTED step (include/mbx_vote.h): `kind` is the form of the CANDIDATES, `candidates` rows of T of them for the S voted streams.
//   kSelectVote: the front launch over candidates * T frames, the select launch, the stream stage of S * T records;  kCombineVote
//   (kSoft only): the combine launch, the soft front over S * T frames, the stream stage.
enum VoteKind { kNoVote, kSelectVote, kCombineVote };
struct StepShape {
    int       codec = 0, S = 0, T = 0;   // T: unused by a ragged step; codec: unused by a mixed one
    size_t    total = 0;                 // rows of a ragged step
    InputKind kind = kRecords;
    bool      rows_given = false;        // the FrameParams rows are there already (mbx_stream_expanded*; the two name predictions assume them)
    bool      resident = false;          // the launch carries DeviceTables::resident
    bool      ragged = false, mixed = false;   // (mixed: ragged with a codec per stream)
    bool      aligned = false;           // wire frames 4-byte aligned (the IMBE front ends load dwords)
    bool      own_workspace = false;     // the rows may go through the stream slot's own workspace and flag words
    bool      slices_allowed = false;    // the launch may be issued slice by slice on the slot's side streams
    bool      capturing = false;         // the stream is being captured into a graph
    bool      keyed = false;             // a keystream row per frame is XORed onto the record by the front launch (mbx_keystream.hip)
    VoteKind  vote = kNoVote;            // a voted step, with ...
    int       candidates = 0;            // ... this many candidate rows (C) and ...
    int       row_cells = 0;             // ... soft candidates of this many cells a frame
};

// ---- ... and everything the launcher then does without asking again -----------------------------------------------------------------
enum StepForm {
    kNoLaunch,        // no such codec: refused before any launch (the other fields answer as for AMBE 3600x2450, for the names' functions)
    kOneLaunchStep,   // the whole T = 1 step as one launch, rows handed over through the slot's workspace and flag words
    kFusedOneStep,    // ... with the front end in the stream's own wave: no rows
    kStagedStep,      // (front launch,) (expand launch,) stream kernel -- plain or slice by slice
    kRaggedStep,      // front launch, expand, (order,) one ragged stream kernel
    kMixedStep,       // row codecs, mixed front launch, mixed expand, (order,) one mixed stream kernel
};
enum FrontLaunch { kNoFront, kFecFront, kSoftFront };
struct StepPlan {
    StepForm    form = kNoLaunch;
    int         instance = 0;           // index into kInstances (Row + column); a ragged step: into kRagged, state form * 3 + column; a mixed one: into kMixed
    FrontLaunch front = kNoFront;
    bool        expand = false;         // an expand launch writes the rows
    bool        rows = false;           // the stream kernel reads rows (expanded or given) instead of expanding records itself
    int         slice_frames = 0;       // > 0: issued in slices of so many frames ...
    int         slice_groups = 0;       // ... over so many groups of streams, ...
    bool        slice_own = false;      // ... group 0 on the caller's stream
    bool        order = false;          // the ragged order kernel runs
    int         front_lead = 0;         // one-launch kernels with a lead argument
    size_t      workspace_frames = 0;   // what the step needs of the workspace its rows go to, in rows, with ...
    size_t      order_offset = 0;       // ... the order words of a ragged step (S of them) and ...
    size_t      codec_offset = 0;       // ... the codec bytes of a mixed one (one per row) behind the rows, at these rows
    bool        outside_capture_only = false;   // needs the slot's flag words or side streams: ask whether the stream is being captured, plan again if so
    VoteKind    vote = kNoVote;         // a voted step: the vote launch behind (select) or in front of (combine) the front launch, which runs over ...
    size_t      front_frames = 0;       // ... so many frames, and ...
    size_t      vote_offset = 0;        // ... the candidates' records (select) or the combined cells (combine) behind the rows, at this row
};

constexpr int kSmallBatchFrames = 256;

// ---- sliced launches (mbx_stream.hip, *_stream_kernel_lds_slice) ------------------------------------------------------------------
// A launch of S streams x T frames is S workgroups of equal length; when S does not fill the device's resident wave slots evenly
// the last round runs part-empty -- BASELINE configs[4]'s shard, 8,192 AMBE+2 streams on 5,120 slots, is 1.6 rounds: the second
// holds 3,072 waves.  Frames of a stream are sequential, but nothing says they must be ONE launch's: the streams are split into
// THREE groups and the frames into slices of 16, and the slices of each group are issued in order on an internal HIP stream of its
// own (forked from and joined to the caller's stream with events).  Measured, 8,192 x 128 AMBE+2, interleaved A/B on one box: plain
// 2.609 ms; two groups 2.518; three 2.481 (-4.7 %); FOUR 3.185 (+22 %: with the caller's stream that is five streams on HIP's four
// hardware queues, and two groups then share one); slices of 8 / 16 / 32 frames with two groups: 2.512 / 2.524 / 2.585.  A slice IS a launch of 16 frames per stream (state in from HBM,
// state out: results bit-identical by construction); the streams' kernels share the device, so the slots one group's slice
// leaves empty are taken by another group's next one (ideal: work / slots = 2.29 ms for that shape instead of ceil(S / slots) rounds).
// Kernel boundaries do the ordering: no in-kernel waiting, no assumption about dispatch.  (Built first as ONE grid of K x S
// workgroups that waited for their stream's previous slice on a progress word: the agent-scope release / acquire pair every slice
// then needs -- an L2 write-back with the PCM of 5,120 waves dirty in it -- made 8,192 x 128 in eight slices 34 % SLOWER.)
// Group 0 runs on the caller's stream itself -- its kernels are queued before the stream waits for the other groups --, so g
// groups occupy g hardware queues, not g + 1, and one group needs no hand-over at all: 2.51 -> 2.42 ms on 8,192 x 128 AMBE+2
// (interleaved A/B; four groups are +26 % either way).
// frames per slice for a launch of S streams x T frames on `slots` resident waves, or 0: the plain launch
static inline int slice_length(int forced, int S, int T, int slots) {
    if (forced == 0 || slots <= 0 || S < 2) {
        return 0;
    }
    const int Tc = forced > 0 ? ((forced + 7) & ~7) : 16;   // multiples of eight: the AMBE bodies expand eight frames at a time
    if (T < 2 * Tc) {
        return 0;
    }
    if (forced > 0) {
        return Tc;
    }
    if (S <= slots) {   // every stream has a slot of its own: nothing to balance
        return 0;
    }
    const double ideal = (double)S / (double)slots;
    const double plain = (double)((S + slots - 1) / slots);
    return (plain >= 1.06 * ideal) ? Tc : 0;   // what the part-empty last round costs must be worth the extra launches
}

// THE decision.
static inline StepPlan plan_step(const StepShape& q, const LaunchSwitches& sw, const DeviceFacts& dev) {
    const CodecShape* sh = codec_shape(q.codec);
    const bool imbe = imbe_codec(q.codec);
    const bool imbe7100 = sh && sh->stream != q.codec;   // own front end, then the 7200x4400 column
    const CodecLaunch& k = kCodecLaunch[stream_codec_of(q.codec)];
    const int col = k.column;
    const int slots = (k.fused_column >= 0 ? dev.imbe_lds_waves : dev.ambe_lds_waves) * dev.simds;   // resident waves of a long launch
    StepPlan p;
    p.front = q.kind == kFrames ? kFecFront : (q.kind == kSoft ? kSoftFront : kNoFront);
    p.front_lead = sw.front_lead;

    if (q.vote != kNoVote) {
        // A voted step: behind the vote its stream stage is that of the RECORDS step of the same S x T -- the expand launch where
        // that has one, its instance -- on the caller's stream alone: never sliced (side streams and events), never a one-launch
        // form (those start from the wire frames of the streams themselves), so it can be captured as it is.  What the vote hands on
        // sits behind the rows of the stream stage in the same workspace: candidates * T records of 16 bytes, or S * T rows of cells.
        StepShape r = q;
        r.vote = kNoVote;
        r.kind = kRecords;
        r.slices_allowed = false;
        r.ragged = r.mixed = r.keyed = false;   // (no such voted steps)
        StepPlan v = plan_step(r, sw, dev);
        const bool combine = q.vote == kCombineVote;
        const size_t st = (size_t)q.S * (size_t)q.T, ct = (size_t)q.candidates * (size_t)q.T;
        const size_t bytes = combine ? st * (size_t)q.row_cells * 2u : ct * 16u;
        v.form = (v.form == kNoLaunch || (combine && q.kind != kSoft) || q.kind == kRecords) ? kNoLaunch : kStagedStep;
        v.front = p.front;
        v.vote = q.vote;
        v.front_frames = combine ? st : ct;
        v.vote_offset = v.workspace_frames;
        v.workspace_frames += dev.row_bytes ? (bytes + dev.row_bytes - 1) / dev.row_bytes : 0;
        return v;
    }
    const bool known = sh || q.mixed;   // (a mixed step brings its codecs: q.codec is not looked at)

    if (q.ragged || q.mixed) {
        // A ragged step: front launch over all rows, expansion, (order,) one ragged stream kernel -- a linear chain on the caller's
        // stream, no one-launch form, never sliced, one kernel per codec column and state form whatever the counts are.  The mixed
        // kernels hold the LDS and the registers of the largest body, an AMBE one.
        // Workgroups are dispatched in grid order; with more streams than resident wave slots the launch ends when the last-dispatched
        // long stream does, so the streams are taken longest first: ragged_order_kernel, in front of the stream kernel on the same
        // stream, writes the order.  With S within the slots every stream starts at once and no order is made.
        p.form = !known ? kNoLaunch : (q.mixed ? kMixedStep : kRaggedStep);
        p.instance = q.mixed ? (q.resident ? 1 : 0) : (q.resident ? 3 : 0) + col;
        p.expand = p.rows = true;
        p.order = sw.ragged_order && q.S > (q.mixed ? dev.ambe_lds_waves * dev.simds : slots);
        // The workspace holds the rows and, behind them, S order words; a mixed step keeps one codec byte per row behind those.
        const size_t order_frames = ((size_t)q.S + 63) / 64;
        const size_t codec_frames = q.mixed ? (q.total + dev.row_bytes - 1) / dev.row_bytes : 0;
        p.order_offset = q.total;
        p.codec_offset = q.total + order_frames;
        p.workspace_frames = q.total + order_frames + codec_frames;
        return p;
    }

    // With several frames per stream prev_mp / prev_mp_enhanced stay in LDS for the whole launch (the *_lds instances,
    // four waves per SIMD) instead of being parked in their HBM slots every frame: mbx_stream.hip, ParkedState.
    const bool lds = q.T >= sw.lds_min_frames && sw.lds_resident;

    // The whole T = 1 step as ONE launch (mbx_stream.hip), for the calls that have the wire frames; the records-based entry points
    // keep the expand + stream pair.  Two forms:
    //   2 (default, 7200x4400 and the AMBE codecs): *_one_launch_kernel -- front blocks (FEC + expansion of eight frames per wave) and
    //     stream blocks in one grid, rows handed over through the stream's workspace (mbx_front_imbe.h);
    //   1 (7100x4400; 7200x4400 with MBX_FUSE_ONE=1): imbe_stream_kernel_one_fused -- the front end in the stream's own wave.
    // MBX_FUSE_ONE=0 switches both off.  MBX_FRONT_LEAD, measured (65,536 x 1, interleaved A/B, one box): lead 0 / 128 / 512: 0.37 /
    // 0.36 / 0.35 ms (stream blocks start before their rows exist and wait); 1024 / 2048 / 4096: 0.2245 / 0.2245 / 0.2230; all first
    // (the default): 0.2229 -- and with the front blocks at a raised wave priority 0.2259 / 0.2253 against 0.2194: what a front block
    // costs is the wave SLOT it holds for the ~10 us of its table-read chain, not its instructions, and slots are what an interleaved
    // front block takes away from stream blocks that could use them.
    // A KEYED step takes neither form, as with MBX_FUSE_ONE=0: the stream blocks of both re-run the front end from the wire frame (the
    // fall-back path; the in-wave form always), so a keyed instance would have to reach into the stream bodies.  It takes the staged
    // launches, whose front launch is the keyed one.
    if (q.kind == kFrames && q.T == 1 && q.S > kSmallBatchFrames && sw.fuse_one != 0 && !q.keyed) {
        // AMBE, 9-byte frames: byte loads, any alignment; no in-wave form: without a workspace the staged kernels.  IMBE: dword loads.
        const bool takes_frames = sh && (!imbe || q.aligned);
        if (takes_frames && sw.fuse_one == 2 && !imbe7100 && q.own_workspace) {
            // A launch that is being CAPTURED into a graph would be replayed with the same epoch, and a replay would find the flags of
            // the replay before it: captured launches take the staged kernels.
            if (!q.capturing) {
                p.form = kOneLaunchStep;
                p.instance = (q.resident ? kOneLaunchRes : kOneLaunch) + col;
                p.workspace_frames = (size_t)q.S;
                p.outside_capture_only = true;
                return p;
            }
        } else if (takes_frames && imbe) {
            p.form = kFusedOneStep;
            p.instance = (q.resident ? kRes1Fused : kOneFused) + kCodecLaunch[q.codec].fused_column;
            return p;
        }
    }

    p.form = known ? kStagedStep : kNoLaunch;
    // IMBE with several frames per stream: the stream kernel expands the records itself, which saves the workspace round
    // trip and a launch (+4 % at T = 16).  With ONE frame per stream the whole-job rate is the same either way (measured
    // 0.296 vs 0.292 ms per 65,536 frames): the table look-ups of the expansion are a latency chain a one-frame wave cannot
    // hide, and the 8-lanes-per-frame expand kernel costs as much as it saves -- there the expansion stays a separate
    // launch, which keeps the dominant kernel to the stream stage proper.
    // ... except for small batches (the synchronous per-frame API is S = T = 1): there a launch less is worth more than the
    // last few per cent of kernel efficiency, and the IMBE stream kernel expands the record itself.
    // AMBE codecs: the LDS-resident instances (T >= 4) expand eight frames of their stream at a time into LDS rows;
    // the HBM-slot instances read rows from the workspace.
    p.expand = !q.rows_given && (imbe ? q.T == 1 && q.S > kSmallBatchFrames : !lds);
    p.rows = q.rows_given || p.expand;
    p.workspace_frames = p.expand ? (size_t)q.S * (size_t)q.T : 0;
    // Sliced: long launches on the slot's own side streams, never resident state, never under capture.
    if (q.slices_allowed && q.own_workspace && lds && !q.resident && !q.capturing) {
        p.slice_frames = slice_length(sw.slice, q.S, q.T, slots);
    }
    if (p.slice_frames > 0) {
        p.instance = kSlice + col;
        p.slice_groups = sw.slice_groups;
        p.slice_own = sw.slice_own;
        p.outside_capture_only = true;
    } else if (q.resident) {   // understood by the *_res / *_res1 instances only, whatever T is and whatever MBX_NO_LDS_RESIDENT says
        // (IMBE's one-frame instance expands a record itself; the AMBE ones read rows, and without rows the looped instance serves T = 1)
        const bool one = q.T == 1 && sw.res1 && (imbe || p.rows);
        p.instance = (one ? kRes1 : kRes) + col;
    } else {
        // (Long AMBE+2 launches used to need a second, register-padded instance to even out their rounds of waves -- config 5's
        // shard is 8 waves per SIMD on 6 slots: 6 + 2.  The LDS-resident instance runs 16 waves per CU: 2 x 16, and
        // 8,192 streams x T = 128 went from 3.51 ms to 3.15 ms.)
        p.instance = (lds ? kLds : (q.T == 1 ? kOne : kPlain)) + col;
    }
    return p;
}

}  // namespace mbx
