// mbx_gather.h -- what the launcher (mbx_api.hip) and the sessions (mbx_session.hip) need of a burst schedule (mbx_burst.hip).
// Host-only and private; the public interfaces are include/mbx_burst.h and include/mbx_burst_groups.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mbx_burst.h"
#include "mbx_burst_groups.h"
#include "mbx_group_plan.h"

namespace mbx {

// what a schedule is, as far as its users look: the folded tables stay inside mbx_burst.hip
struct BurstShape {
    int    codec, frames, bits, device;
    size_t bytes;          // the smallest burst_stride of a hard burst in the schedule's form (mbx_burst_schedule_bytes); an LLR form: 0
    size_t frame_bytes;    // one gathered wire frame
    size_t cells;          // one gathered cell array (mbe_soft_bit cells)
    int    form;           // MBX_BURST_FORM_*
    size_t soft_cells;     // cells of one soft burst in the schedule's form (mbx_burst_schedule_soft_cells)
    size_t soft_bytes;     // bytes of one soft burst in the schedule's form (mbx_burst_schedule_soft_bytes)
    // an LLR schedule is soft-only: the hard calls refuse it; its soft bursts are aligned to one LLR (2 | 1), not to a cell
    bool   llr() const { return form == MBX_BURST_FORM_LLR16 || form == MBX_BURST_FORM_LLR8; }
    size_t soft_align() const { return form == MBX_BURST_FORM_LLR8 ? 1 : 2; }
};
BurstShape burst_shape(const mbx_burst_schedule* sched);   // sched != nullptr

// The gather launch alone, arguments already checked by the caller (pointers, alignment, strides, current device == the schedule's):
// n bursts -> n * frames rows at `out`, `row` bytes (hard) or cells (soft) apart.  Returns 0, or MBX_ENODEVICE with the text set.
int burst_gather(const mbx_burst_schedule* sched, bool soft, const void* d_in, size_t burst_stride, size_t n, void* d_out, size_t row,
                 void* stream);

// ---- burst groups (include/mbx_burst_groups.h) ----
// what the placement of a group (mbx_group_plan.h) needs of its schedule's gather: bursts per workgroup and dynamic LDS
int      burst_gather_per_workgroup(const mbx_burst_schedule* sched, bool soft);
unsigned burst_gather_lds(const mbx_burst_schedule* sched, bool soft);
// The host checks of a call's groups, every one before a device is asked for, and their placement: 0, or MBE_STATUS_INVALID_ARGUMENT
// with "<who>: <reason>" in mbx_last_error().  NULL groups / schedule / bursts (of a group that has streams), n_groups outside
// 0 .. 8, counts, a hard call with an LLR schedule, a hard burst_stride below the schedule's bytes, a bursts or index pointer below
// its alignment, more than 2^31-1 frames.  `shapes` (8 entries) receives what the plan was made from.
int burst_groups_plan(const char* who, const mbx_burst_group* groups, int n_groups, bool soft, GroupShape* shapes, GroupPlan* plan);
// one group of the ONE gather launch over all groups: the caller's arguments and the group's place (GroupPlace)
struct GroupGather {
    const mbx_burst_schedule* sched;
    const void*    d_in;
    size_t         burst_stride;        // hard
    uint32_t       bursts;              // n_streams * bursts_per_stream, > 0
    int            bursts_per_stream;
    const int32_t* d_index;             // pool slots of the group's streams, or nullptr: first_slot + j
    int            first_slot;
    uint32_t       first_wg;
    int32_t        first_row, first_stream;
};
// what the launch writes besides the rows: the layout words of the mixed step (frame_offset[S + 1], stream_index[S], stream_codec[S])
struct GroupLayout {
    int      S, total;
    int32_t* d_frame_offset;
    int32_t* d_stream_index;
    uint8_t* d_stream_codec;
};
// The launch, arguments already checked by the caller: `count` groups (1 .. 8, each with bursts) in grid order -> rows of
// MBX_MIXED_ROW_BYTES bytes / MBX_MIXED_ROW_CELLS cells at d_rows.  Returns 0, or MBX_ENODEVICE with the text set.
int burst_gather_groups(const GroupGather* groups, int count, bool soft, unsigned grid, unsigned lds, const GroupLayout& layout, void* d_rows,
                        void* stream);

}  // namespace mbx
