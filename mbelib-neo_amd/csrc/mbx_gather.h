// mbx_gather.h -- what the launcher (mbx_api.hip) and the sessions (mbx_session.hip) need of a burst schedule (mbx_burst.hip).
// Host-only and private; the public interface is include/mbx_burst.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mbx_burst.h"

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

}  // namespace mbx
