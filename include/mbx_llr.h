/*
 * mbx_llr.h -- soft input as log-likelihood ratios (LLRs) that are NOT bursts, for the MI355X batch launcher (libmbx_hip.so).
 *
 * A soft demodulator emits one signed LLR per received bit.  Bursts of LLRs are converted inside their gather and need no call of
 * their own (mbx_burst_schedule_create_llr, mbx_burst.h); a host converts with mbx_soft_bits_from_llr (mbx.h).  This is the same
 * conversion on the device, for callers that hold frame-shaped LLR arrays ([8][23] | [4][24] | [7][24]: the shapes of the
 * reference's soft frames) in device memory and then call the soft frames calls of mbx.h.
 *
 * Conventions are those of mbx.h: d_ pointers are DEVICE pointers, `stream` is a hipStream_t passed as void*, the launcher is
 * asynchronous on `stream`, never synchronises, and returns 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in
 * mbx_last_error().
 *
 * The conversion, for an LLR v widened to int: bit = (v > 0), reliability = min(|v|, 255); so -32768 gives {0, 255} and 0 gives
 * {0, 0}.  An int8 LLR is the int16 LLR of the same value.
 *
 * Alignment, in the style of the table in mbx.h:
 *   kind        bytes  which pointers
 *   llr         2 | 1  d_llr: llr_bytes; fetched in dwords from the first 4-aligned byte on, single LLRs at the edges
 *   soft        2      d_soft: stored in dwords, single cells at the edges
 * Sizes are exact: nothing is read or written outside the count elements.
 */
#ifndef MBX_LLR_H
#define MBX_LLR_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ref: mbe_softBitsFromLlr  include/mbelib-neo/mbelib.h:224, src/core/mbelib.c:125-158.
 * count LLRs of llr_bytes bytes each (2: int16_t, 1: int8_t) -> count cells, the bytes mbx_soft_bits_from_llr gives on the host.
 * One launch; count = 0 launches nothing.  A NULL pointer or another llr_bytes: MBE_STATUS_INVALID_ARGUMENT, as is a pointer below
 * its alignment (before anything is launched). */
int mbx_soft_from_llr(const void* d_llr, int llr_bytes, size_t count, mbe_soft_bit* d_soft, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MBX_LLR_H */
