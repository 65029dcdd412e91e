// mbx_soft_front.hip -- the front of a SOFT-DECISION batch step (mbx_process_batch_soft and its resident / indexed / workspace
// forms, soft session submits, soft queue mode): one wave takes one frame of mbe_soft_bit cells, runs the maximum-likelihood
// search of its protected blocks (mbx_fec_soft.h) and writes the 16-byte parameter record.  The stream stage follows as for
// records from anywhere else: the expand launch where it reads rows, then the instance chosen for the shape.
//
// FEC ONLY, by measurement.  These kernels were built to expand the record in the searching wave as well (lanes 0..7 running the
// bodies of mbx_expand_imbe.h / mbx_expand_ambe.h on the record in registers, the row written straight to the workspace: two
// launches per step instead of three), with and without the expansion's table values requested right after C0.  Same occupancy,
// bit-identical output, and slower on one box in interleaved A/B: IMBE +2.6 % / +4.3 % with the early requests, AMBE+2 +12 %
// (EXPERIMENTS.md "Soft front"; the fused form is profiles/r07/soft_front_fused.patch, the log profiles/r07/soft_step_ab.log).
// So the record crosses HBM and the 8-frames-per-wave expand launch does the expansion.  Codec 3 (D-STAR) frames are AMBE cells:
// in this form their front is soft_front_ambe_kernel (the fused form had a fourth kernel with the 3600x2400 expansion).
//
// ref: src/imbe/imbe7200x4400.c:746-778 (mbe_processImbe7200x4400SoftFrame), src/imbe/imbe7100x4400.c:481-525,
//      src/ambe/ambe3600x2450.c:684-714
#include "mbx_device.h"
#include "mbx_fec_soft.h"
#include "mbx_kernels.h"

namespace mbx {

__global__ void __launch_bounds__(64, 8)
soft_front_imbe_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, mbx_param_record* __restrict__ records, DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const uint4 rec = soft_record_imbe7200x4400(S, soft + i * MBX_IMBE_SOFT_BITS, tabs, lane);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&records[i]) = rec;
    }
}

// 7100x4400 cells in, the record in 7200x4400 order out: the stream stage runs as IMBE 7200x4400
__global__ void __launch_bounds__(64, 8)
soft_front_imbe7100_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, mbx_param_record* __restrict__ records, DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const uint4 rec = soft_record_imbe7100x4400(S, soft + i * MBX_IMBE7100_SOFT_BITS, tabs, lane);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&records[i]) = rec;
    }
}

// AMBE+2 3600x2450 and AMBE 3600x2400 (the same cells and the same search; the expansion that follows differs)
__global__ void __launch_bounds__(64, 8)
soft_front_ambe_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, mbx_param_record* __restrict__ records, DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const uint4 rec = soft_record_ambe3600(S, soft + i * MBX_AMBE_SOFT_BITS, tabs, lane);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&records[i]) = rec;
    }
}

// The front of a MIXED soft step (mbx_process_batch_soft_mixed): rows of MBX_IMBE_SOFT_BITS cells whatever the codec (a codec's own
// cell array at the front of its row), the codec of row i in row_codec[i].  One wave per row, so the codec is wave-uniform: a scalar
// branch into the search of the three kernels above, on one SoftScratch.  A byte that names no codec: no record is written.
__global__ void __launch_bounds__(64, 8)
soft_front_mixed_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, const uint8_t* __restrict__ row_codec,
                        mbx_param_record* __restrict__ records, DeviceTables tabs) {
    __shared__ SoftScratch S;
    const size_t i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const int lane = lane_id();
    const mbe_soft_bit* const row = soft + i * MBX_IMBE_SOFT_BITS;
    uint4 rec;
    switch (__builtin_amdgcn_readfirstlane((int)row_codec[i])) {   // (one row per wave: uniform)
    case MBX_CODEC_IMBE7200X4400:
        rec = soft_record_imbe7200x4400(S, row, tabs, lane);
        break;
    case MBX_CODEC_IMBE7100X4400:
        rec = soft_record_imbe7100x4400(S, row, tabs, lane);
        break;
    case MBX_CODEC_AMBE3600X2450:
    case MBX_CODEC_AMBE3600X2400:
        rec = soft_record_ambe3600(S, row, tabs, lane);
        break;
    default:
        return;
    }
    if (lane == 0) {
        *reinterpret_cast<uint4*>(&records[i]) = rec;
    }
}

}  // namespace mbx
