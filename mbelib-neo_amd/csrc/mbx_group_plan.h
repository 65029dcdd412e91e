// mbx_group_plan.h -- where the burst groups of one call (include/mbx_burst_groups.h) sit: in the grid of the ONE gather launch that
// covers them all, in the rows of the mixed step behind it, and in the stream's workspace.  From the groups' shapes to first workgroup,
// first frame row and first stream row per group, the totals, the dynamic LDS of the launch (the largest group's) and the workspace
// layout, with the size and overflow refusals.
// Integer work on the host alone: no HIP, no locks, no globals -- so that a CPU program can check it under a sanitizer
// (tests/group_plan_check.cpp), in the manner of mbx_launch_plan.h and mbe_flush_plan.h.  Private to the launcher (mbx_api.hip) and the
// sessions (mbx_session.hip); nothing here is exported.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mbx {

constexpr int kMaxBurstGroups = 8;   // MBX_BURST_MAX_GROUPS

// what the plan needs of one group: the caller's counts and, of its schedule, what the gather of that schedule launches with
struct GroupShape {
    int      codec = 0;               // MBX_CODEC_* of the schedule: the codec of every stream of the group
    int      form = 0;                // MBX_BURST_FORM_* (carried, not looked at: the plan is the same for every form)
    int      frames = 1;              // frames per burst, F >= 1
    int      n_streams = 0;           // >= 0
    int      bursts_per_stream = 1;   // >= 1
    int      bursts_per_wg = 1;       // bursts a workgroup of this schedule's gather takes: 64 (hard), the schedule's own (soft)
    unsigned lds = 0;                 // dynamic LDS of this schedule's gather
};

// ... and where the group then is
struct GroupPlace {
    uint32_t first_wg = 0, wgs = 0;    // workgroups first_wg .. first_wg + wgs - 1 of the grid
    int32_t  first_row = 0, rows = 0;  // frame rows of the step (and of every output)
    int32_t  first_stream = 0;         // stream rows of the step: n_streams of them
    uint32_t bursts = 0;               // n_streams * bursts_per_stream
};

enum GroupRefusal {
    kGroupsOk = 0,
    kGroupCount,          // n_groups outside 0 .. kMaxBurstGroups
    kGroupNegative,       // a negative n_streams
    kGroupBurstsPer,      // bursts_per_stream < 1
    kGroupTooManyFrames,  // more than 2^31-1 frames in total (offsets are int32_t)
};
static inline const char* group_refusal_text(GroupRefusal r) {
    switch (r) {
    case kGroupCount: return "n_groups must be 0 .. MBX_BURST_MAX_GROUPS";
    case kGroupNegative: return "a negative n_streams";
    case kGroupBurstsPer: return "bursts_per_stream must be at least 1";
    case kGroupTooManyFrames: return "more than 2^31-1 frames in one call";
    default: return "";
    }
}

struct GroupPlan {
    GroupPlace place[kMaxBurstGroups];
    int        n_groups = 0;
    uint32_t   grid = 0;            // workgroups of the gather launch
    int32_t    total_rows = 0;      // frame rows of the step
    int32_t    total_streams = 0;   // stream rows of the step
    unsigned   lds = 0;             // dynamic LDS of the gather launch: the largest of the groups that have a workgroup
};

// THE placement.  Groups without streams take no workgroup, no row and no stream row: their first values are the next group's.
static inline GroupRefusal plan_groups(const GroupShape* g, int n_groups, GroupPlan* out) {
    *out = GroupPlan();
    if (n_groups < 0 || n_groups > kMaxBurstGroups) {
        return kGroupCount;
    }
    out->n_groups = n_groups;
    uint64_t wg = 0, row = 0, stream = 0;
    for (int i = 0; i < n_groups; ++i) {
        if (g[i].n_streams < 0) {
            return kGroupNegative;
        }
        if (g[i].bursts_per_stream < 1) {
            return kGroupBurstsPer;
        }
        // (n_streams, bursts_per_stream < 2^31 and frames <= 18: no product below leaves 64 bits)
        const uint64_t bursts = (uint64_t)g[i].n_streams * (uint64_t)g[i].bursts_per_stream;
        if (bursts > 0x7fffffffu) {
            return kGroupTooManyFrames;
        }
        const uint64_t rows = bursts * (uint64_t)(g[i].frames < 1 ? 1 : g[i].frames);
        if (row + rows > 0x7fffffffu) {
            return kGroupTooManyFrames;
        }
        const uint64_t per = (uint64_t)(g[i].bursts_per_wg < 1 ? 1 : g[i].bursts_per_wg);
        GroupPlace& p = out->place[i];
        p.first_wg = (uint32_t)wg;
        p.wgs = (uint32_t)((bursts + per - 1) / per);
        p.first_row = (int32_t)row;
        p.rows = (int32_t)rows;
        p.first_stream = (int32_t)stream;
        p.bursts = (uint32_t)bursts;
        if (p.wgs && g[i].lds > out->lds) {
            out->lds = g[i].lds;
        }
        wg += p.wgs, row += rows, stream += (uint64_t)g[i].n_streams;   // (streams <= bursts <= rows, workgroups <= bursts: all below 2^31)
    }
    out->grid = (uint32_t)wg;
    out->total_rows = (int32_t)row;
    out->total_streams = (int32_t)stream;
    return kGroupsOk;
}

// The workspace of a call, in bytes from the workspace's (256-byte aligned) start:
//   step rows (what the mixed step's own plan asks for: step_frames workspace frames of frame_unit bytes)
//   | gathered rows, 256-byte aligned: total_rows of row_bytes (MBX_MIXED_ROW_BYTES, or MBX_MIXED_ROW_CELLS cells)
//   | layout words, 4-byte aligned: frame_offset[S + 1] and stream_index[S] (int32_t), then stream_codec[S] (bytes)
struct GroupWorkspace {
    size_t gathered = 0, frame_offset = 0, stream_index = 0, stream_codec = 0, end = 0;   // byte offsets
    size_t frames = 0;   // the whole of it in workspace frames: what mbx_reserve_stream is given
};
static inline GroupWorkspace group_workspace(const GroupPlan& p, size_t step_frames, size_t frame_unit, size_t row_bytes) {
    GroupWorkspace w;
    const size_t S = (size_t)p.total_streams;
    w.gathered = (step_frames * frame_unit + 255) & ~(size_t)255;
    w.frame_offset = (w.gathered + (size_t)p.total_rows * row_bytes + 3) & ~(size_t)3;
    w.stream_index = w.frame_offset + (S + 1) * sizeof(int32_t);
    w.stream_codec = w.stream_index + S * sizeof(int32_t);
    w.end = w.stream_codec + S;
    w.frames = frame_unit ? (w.end + frame_unit - 1) / frame_unit : 0;
    return w;
}

}  // namespace mbx
