/*
 * mbx_levels.h -- levels out and the gated mix-down of the MI355X batch launcher (libmbx_hip.so): the peak and the energy of every row
 * a step wrote, measured on the device, and talkgroup buses that sum only the inputs that are OPEN, or only the N LOUDEST of those.
 *
 * A console's activity and clip lights, a recorder's VOX, a gateway's silence suppression and a monitor's "which of 65,536 channels is
 * talking" all need one level per row; a host got it only by taking every row back, 320 B per frame.  A level record is 16 B.  And a
 * bus of mbx_mixdown.h sums everything it is given: right for a talkgroup of four, wrong for an unselect or an all-call bus of hundreds
 * of inputs, which adds up every idle channel's comfort noise and hits the rails as soon as a few talkers overlap.  Bridges and consoles
 * mix the inputs that are open (a level gate), usually only the N loudest of them, N = 3 the classic figure.  Both decisions are exact
 * in integers.  They are stateless per frame: no hang time, no hysteresis, no ramps (the gate that has all three is in mbx_hold.h).
 *
 * Conventions are those of mbx_mixdown.h: `stream` is a hipStream_t passed as void*, launchers are asynchronous on `stream`, never
 * synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every refusal comes before a
 * device is asked for.
 *
 * The level of a row of 160 int16 samples x[n]:
 *     energy  = the sum of x[n]^2                    <= 160 * 2^30 < 2^38
 *     peak    = the largest |x[n]|, taken in int32   0 .. 32768 (|-32768| is 32768)
 *     clipped = how many x[n] are 32767 or -32768    0 .. 160
 *
 * The gate.  An input of a bus is OPEN iff the peak of its row >= open_peak (0: every input is open).  With loudest_n = 0 every open
 * input is summed; with loudest_n = N (1 .. MBX_GATE_MAX_LOUDEST) only the N loudest open inputs of the bus are.  Loudest is decided per
 * bus: input k beats input j if the energy of its row is larger, and at equal energy the smaller k wins, k being the position in the
 * plan's input arrays -- so a row that is in a bus twice ranks its earlier occurrence first.  Levels are of the rows as decoded, before
 * the gain, and an input with gain 0 still competes.  A bus with fewer than N open inputs sums them all; a bus with none is silence
 * (0, 0xFF or 0xD5 by form).
 * The gated bus is, by definition, the bus of mbx_mixdown.h with the gain of every input that is not chosen set to 0: a term at gain 0
 * is (x * 0 + 2048) >> 12 = 0, so "left out" and "gain 0" give the same bits, and the order of the sum does not matter.  A gate {0, 0}
 * gives the bytes of mbx_mixdown.  The device's bits are those of mbx_mixdown_gated_host and of mbelib-neo_amd/levels.py (mix_gated).
 *
 * Alignment, in the style of the table in mbx_mixdown.h (kinds not named here keep their row there):
 *   kind        bytes  which pointers
 *   level rows  16     d_pcm16 of mbx_pcm_levels and of mbx_mixdown_gated: a lane loads 16 bytes (8 samples) of a row at once
 *   levels      16     d_levels of mbx_pcm_levels and of mbx_mixdown_gated: a record is one 16-byte store and one 16-byte load
 *   bus pcm16   16     d_out of mbx_mixdown_gated with MBX_MIXDOWN_PCM16: a lane stores 16 bytes at once
 *   bus bytes   8      d_out of mbx_mixdown_gated with MBX_MIXDOWN_ULAW / _ALAW: a lane stores 8 bytes at once
 * The host arrays of the *_host calls and the `out` of the session calls may sit anywhere their element type allows.  Sizes are exact:
 * nrows records are written by mbx_pcm_levels, nothing in front of them or behind them.  d_levels must overlap neither d_pcm16 nor
 * d_out.  A pointer below its alignment is refused with MBE_STATUS_INVALID_ARGUMENT before a device is asked for.
 */
#ifndef MBX_LEVELS_PUBLIC_H
#define MBX_LEVELS_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_mixdown.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_GATE_MAX_LOUDEST 8
#define MBX_SESSION_LEVELS   32u   /* outputs bit of mbx_session_create[_mixed]: the session can deliver level records */

typedef struct mbx_row_level {
    uint64_t energy;    /* sum of x[n]^2 over the 160 samples: <= 160 * 2^30 < 2^38 */
    uint16_t peak;      /* max |x[n]|: 0 .. 32768 (|-32768| is 32768) */
    uint16_t clipped;   /* how many samples are 32767 or -32768: 0 .. 160 */
    uint32_t zero;      /* 0 */
} mbx_row_level;

typedef struct mbx_mixdown_gate {
    uint16_t open_peak;   /* an input is OPEN iff the peak of its row >= open_peak; 0: every input is open */
    uint16_t loudest_n;   /* 0: every open input is summed; 1 .. MBX_GATE_MAX_LOUDEST: only the N loudest open inputs */
} mbx_mixdown_gate;

/* One launch behind any step on the same stream: the nrows rows of d_pcm16 -> nrows records in d_levels.  A plain launch on the
 * caller's stream: it may be captured.  nrows == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL d_pcm16 or d_levels; a pointer below its alignment (Alignment);
 * arrays that overlap; more than 2^31 - 1 rows. */
int mbx_pcm_levels(const int16_t* d_pcm16, size_t nrows, mbx_row_level* d_levels, void* stream);

/* Host only, no device: the definition.  pcm16 is nrows rows of 160 samples of HOST memory, out nrows records.  A NULL pcm16 or out is
 * refused (nrows == 0 with both given returns 0). */
int mbx_pcm_levels_host(const int16_t* pcm16, size_t nrows, mbx_row_level* out);

/* One or two launches behind mbx_pcm_levels on the same stream (one per kernel form the plan has buses for): the buses of `plan`
 * under `gate`, in the plan's bus order, as mbx_mixdown delivers them.  d_levels holds nrows records, those of d_pcm16: the caller runs
 * mbx_pcm_levels first on the same stream.  It takes no workspace; the plan stays immutable and usable from several streams at once.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL gate (an ungated caller has mbx_mixdown); loudest_n above
 * MBX_GATE_MAX_LOUDEST; open_peak above 32768; a NULL d_levels; a pointer below its alignment (Alignment); everything mbx_mixdown
 * refuses (form, NULL pointers, nrows below the plan's rows, d_pcm16 and d_out overlapping); d_levels overlapping d_pcm16 or d_out.
 * Then: a plan made on another device than the current one. */
int mbx_mixdown_gated(const mbx_mixdown_plan* plan, const mbx_mixdown_gate* gate, int form, const int16_t* d_pcm16, size_t nrows,
                      const mbx_row_level* d_levels, void* d_out, void* stream);

/* Host only, no device: the definition.  The arguments of mbx_mixdown_host and a gate; it computes the levels itself.  The refusals of
 * mbx_mixdown_host and those of the gate. */
int mbx_mixdown_gated_host(int form, const mbx_mixdown_gate* gate, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                           const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, void* out);

/* Sessions (mbx.h) created with MBX_SESSION_LEVELS among their outputs hold, per slot, max_frames_per_submit records on the device and
 * in pinned staging.  The NEXT submit of this session, of whatever form, also delivers one record per row of the submit to out (HOST
 * memory), in the row order of its pcm16, valid after mbx_session_wait.  The submit's pcm16 may be NULL: the session keeps the int16
 * rows on the device either way, and then only the records cross PCIe.  The attachment behaves exactly like mbx_session_next_mixdown:
 * it lasts one submit and is used up whether that queues or refuses; reset, seed, get_state and set_state leave it; a NULL out
 * clears it and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: no session, a session made without MBX_SESSION_LEVELS. */
int mbx_session_next_levels(struct mbx_session* s, mbx_row_level* out);

/* mbx_session_next_mixdown with a gate: the session needs MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS.  It shares the buses slot of the
 * attachment with mbx_session_next_mixdown: whichever was called last holds.  The levels launch runs once per submit, behind the step
 * and in front of the gated mix-down, whether or not mbx_session_next_levels is attached beside it.
 * MBE_STATUS_INVALID_ARGUMENT: what mbx_session_next_mixdown refuses, a session made without either bit, a NULL gate, loudest_n above
 * MBX_GATE_MAX_LOUDEST, open_peak above 32768. */
int mbx_session_next_mixdown_gated(struct mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_gate* gate, void* out);

#ifdef __cplusplus
}
#endif

#endif /* MBX_LEVELS_PUBLIC_H */
