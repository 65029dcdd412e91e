/*
 * mbx_mixdown.h -- mix-down out of the MI355X batch launcher (libmbx_hip.so): talkgroup BUSES summed on the device, as int16 or G.711.
 *
 * A step delivers int16 [rows][160], one row per channel, but nobody listens to or stores channels one at a time: a dispatch console
 * hears a select and an unselect bus, a logging recorder stores one track per talkgroup, a conference bridge or an RTP gateway forwards
 * one summed stream per group.  A host that wants buses took every row across PCIe (320 B per frame, 160 B as G.711) and summed them in
 * a per-sample loop of its own.  Here one or two launches BEHIND the step sum the step's rows into buses on the device, a gain per
 * input, and a session delivers the buses alone.  No step, plan or kernel in front of it changes: the launches read what the step
 * wrote.  ("Mixed" means mixed-codec elsewhere in these headers; this is MIX-DOWN, and its outputs are BUSES.)
 *
 * Conventions are those of mbx.h: `stream` is a hipStream_t passed as void*, launchers are asynchronous on `stream`, never
 * synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error().
 *
 * The buses, in CSR form.  Bus b has the inputs k = bus_offset[b] .. bus_offset[b + 1] - 1; input k is the row src_row[k] of the
 * step's int16 [rows][160] and the gain gain_q12[k]: int16 in Q12, MBX_MIXDOWN_UNITY (4096) is 1.0, the range -8.0 .. +7.9998, a
 * negative gain inverts polarity; a NULL gain_q12 is unity everywhere.  A row may feed any number of buses and may occur more than
 * once in one bus.  A bus has at most MBX_MIXDOWN_MAX_INPUTS (4096) inputs; a bus with none is silence.
 *
 * The arithmetic, exact and in integers.  For sample n of bus b
 *     term_k = (x[src_row[k]][n] * gain_q12[k] + 2048) >> 12     an int32 product, an arithmetic (floor) shift
 *     acc    = the sum of term_k over the bus                    int32: |acc| <= 4096 * (2^18 + 1) < 2^31, it cannot overflow
 *     y      = clamp(acc, -32768, 32767)                         hard saturation, once, after the sum
 * and the output is y as int16 (MBX_MIXDOWN_PCM16) or the G.711 byte of y exactly as mbx_pcm8.h defines it (MBX_MIXDOWN_ULAW: silence
 * is 0xFF; MBX_MIXDOWN_ALAW: silence is 0xD5).  A sum of integers does not depend on its order, so the device's bits are those of
 * mbx_mixdown_host and of mbelib-neo_amd/mixdown.py (mix), whatever the split over lanes.  No limiter, no AGC, no gain ramps, no
 * resampling (a gate that fades its inputs in and out is in mbx_hold.h).
 *
 * Alignment, in the style of the table in mbx.h (kinds not named here keep their row there):
 *   kind        bytes  which pointers
 *   mix rows    16     d_pcm16 of mbx_mixdown: a lane loads 16 bytes (8 samples) of a row at once
 *   bus pcm16   16     d_out of mbx_mixdown with MBX_MIXDOWN_PCM16: a lane stores 16 bytes at once
 *   bus bytes   8      d_out of mbx_mixdown with MBX_MIXDOWN_ULAW / _ALAW: a lane stores 8 bytes at once
 * The host arrays of mbx_mixdown_host, of the plan calls and the `out` of mbx_session_next_mixdown may sit anywhere their element type
 * allows.  Sizes are exact: rows below mbx_mixdown_plan_rows() are read, n_buses * 160 samples are written, nothing in front of them
 * or behind them.  d_pcm16 (all nrows rows of it) and d_out must not overlap.  A pointer below its alignment is refused with
 * MBE_STATUS_INVALID_ARGUMENT before a device is asked for and before anything is launched.
 */
#ifndef MBX_MIXDOWN_PUBLIC_H
#define MBX_MIXDOWN_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_MIXDOWN_PCM16 0
#define MBX_MIXDOWN_ULAW  1
#define MBX_MIXDOWN_ALAW  2
#define MBX_MIXDOWN_UNITY      4096
#define MBX_MIXDOWN_MAX_INPUTS 4096
#define MBX_SESSION_MIXDOWN    16u   /* outputs bit of mbx_session_create[_mixed]: the session can deliver buses */

struct mbx_session;
typedef struct mbx_mixdown_plan mbx_mixdown_plan;   /* immutable once made, like a burst schedule */

/* A plan: the buses checked on the host -- every refusal comes before a device is asked for --, then their tables uploaded to the
 * calling thread's CURRENT device (after mbx_init for it); a plan used while another device is current is refused, as a burst
 * schedule is.  The arrays are copied: the caller's may go once the call returns.  Buses with more inputs than the library's default
 * split take the long form of the kernel (one workgroup per bus), the others the short form (one lane per 8 samples); the bits do
 * not depend on it.
 * MBE_STATUS_INVALID_ARGUMENT, the text naming the call: no `out`; n_buses < 1; a NULL bus_offset, or a NULL src_row while a bus
 * has an input; bus_offset[0] != 0; a bus_offset that decreases; a bus of more than MBX_MIXDOWN_MAX_INPUTS inputs; a src_row that is
 * negative or 2^31 - 1.  (The total number of inputs fits int32 by the type of bus_offset.) */
int mbx_mixdown_plan_create(mbx_mixdown_plan** out, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                            const int16_t* gain_q12);
/* The same with the split stated: buses with MORE than long_above inputs take the long form; 0: the library's default; any value from
 * MBX_MIXDOWN_MAX_INPUTS up: every bus takes the short form.  A negative long_above is refused. */
int mbx_mixdown_plan_create_split(mbx_mixdown_plan** out, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                                  const int16_t* gain_q12, int long_above);
/* NULL allowed.  The caller keeps a plan until every launch and every session submit that uses it has completed. */
int mbx_mixdown_plan_destroy(mbx_mixdown_plan* plan);
int mbx_mixdown_plan_buses(const mbx_mixdown_plan* plan);        /* n_buses */
int mbx_mixdown_plan_rows(const mbx_mixdown_plan* plan);         /* rows needed: 1 + the largest src_row, 0 where no bus has an input */
int mbx_mixdown_plan_long_buses(const mbx_mixdown_plan* plan);   /* how many buses take the long form */

/* Host only, no device: the definition, for hosts and tests.  pcm16 is nrows rows of 160 samples of HOST memory, out n_buses * 160
 * samples of `form` (int16_t, or bytes).  The refusals of mbx_mixdown_plan_create, and: a form that is none of the three, a NULL
 * pcm16 (where a bus has an input) or out, nrows below the rows needed. */
int mbx_mixdown_host(int form, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12,
                     const int16_t* pcm16, size_t nrows, void* out);

/* One or two launches behind any step on the same stream (one per kernel form the plan has buses for): the rows of d_pcm16 the plan
 * names -> mbx_mixdown_plan_buses() * 160 samples of `form` in d_out, in the plan's bus order.  Plain launches on the caller's stream:
 * they may be captured.  nrows is the number of rows d_pcm16 holds.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a form that is none of MBX_MIXDOWN_*; a NULL plan, d_pcm16 or d_out; a
 * pointer below its alignment (Alignment); nrows < mbx_mixdown_plan_rows(), so that no launch can read outside d_pcm16; arrays that
 * overlap.  Then: a plan made on another device than the current one. */
int mbx_mixdown(const mbx_mixdown_plan* plan, int form, const int16_t* d_pcm16, size_t nrows, void* d_out, void* stream);

/* Sessions (mbx.h) created with MBX_SESSION_MIXDOWN among their outputs hold, per slot, a device buffer and pinned staging for
 * max_frames_per_submit bus rows.  The NEXT submit of this session, of whatever form -- frames, indexed, soft, soft indexed, keyed,
 * bursts, soft bursts, burst groups --, also delivers mbx_mixdown_plan_buses() * 160 samples of `form` to out (HOST memory: a pinned
 * buffer is written in place, a pageable one through the slot's pinned staging), valid after mbx_session_wait like every output.  The
 * plan's src_row counts in the row order of that submit's pcm16.  The submit's own pcm16 / pcmf / results are delivered as without
 * it, and its pcm16 may be NULL: the session keeps the int16 rows on the device either way, and then only the buses cross PCIe.  A
 * submit with fewer rows than mbx_mixdown_plan_rows() is refused with MBE_STATUS_INVALID_ARGUMENT and nothing is queued; a submit of
 * no rows queues nothing and delivers nothing.  The attachment behaves exactly like mbx_session_next_pcm8 (mbx_pcm8.h), and the two
 * may be attached to one submit: the submit uses it up whether it queues or refuses; reset, seed, get_state and set_state leave it;
 * a NULL out clears it and returns 0.  The plan must outlive the submit's completion.
 * MBE_STATUS_INVALID_ARGUMENT: no session, a session made without MBX_SESSION_MIXDOWN, no plan, a form that is none of MBX_MIXDOWN_*,
 * a plan with more buses than max_frames_per_submit, a plan made on another device than the session's. */
int mbx_session_next_mixdown(struct mbx_session* s, const mbx_mixdown_plan* plan, int form, void* out);

#ifdef __cplusplus
}
#endif

#endif /* MBX_MIXDOWN_PUBLIC_H */
