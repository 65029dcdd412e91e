// mbx_llr_cell.h -- a signed log-likelihood ratio (LLR) of one received bit -> the soft cell of that bit, stated ONCE for the host loop
// (mbx_soft_bits_from_llr, mbx_api.hip) and for the kernels that convert on the device (burst_gather_soft_kernel's LLR instances,
// mbx_burst.hip; soft_from_llr_kernel, mbx_fec.hip).  Host-visible: nothing here needs a device compile.
// ref: mbe_softBitFromLlr / mbe_softBitsFromLlr, src/core/mbelib.c:125-158.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MBX_LLR_FN __host__ __device__ inline
#else
#define MBX_LLR_FN inline
#endif

namespace mbx {

// The cell as its 16-bit piece, bit | reliability << 8 (mbe_soft_bit is {bit, reliability}, one byte each): bit = (v > 0),
// reliability = min(|v|, 255).  `v` is the LLR widened to int -- an int8 LLR is the int16 LLR of the same value -- so the
// magnitude of -32768 is 32768 and saturates like every other: {0, 255}; 0 gives {0, 0}.
MBX_LLR_FN uint32_t soft_cell_from_llr(int v) {
    const int mag = v < 0 ? -v : v;
    return (v > 0 ? 1u : 0u) | ((uint32_t)(mag > 255 ? 255 : mag) << 8);
}

}  // namespace mbx
