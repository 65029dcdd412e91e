/*
 * mbx_hold.h -- the held gate of the MI355X batch launcher (libmbx_hip.so): mbx_mixdown_gated (mbx_levels.h) with MEMORY.  The gate of
 * mbx_levels.h is stateless per frame: it switches an input on and off at 20 ms frame edges with a step of full amplitude (a click),
 * drops a talker in every frame whose peak dips below the threshold (between words, in an unvoiced consonant, in a repeat frame), and
 * may swap the membership of "the 3 loudest" every frame.  A bridge or a console holds a gate open for a HANG TIME, closes it at a
 * lower level than it opens it (HYSTERESIS), and FADES inputs in and out.  This header does that on the device, behind the step:
 * one 4-byte state record per input of a plan, kept on the device between calls, exact in integers -- the device's bits are those of
 * mbx_mixdown_held_host and of mbelib-neo_amd/hold.py (step).
 *
 * Conventions are those of mbx_levels.h: `stream` is a hipStream_t passed as void*, launchers are asynchronous on `stream`, never
 * synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every refusal comes before a
 * device is asked for.
 *
 * DECISION.  Once per call, for input k of a bus, from the peak p and the energy of its row's mbx_row_level and its previous state
 * (open', hang', on'):
 *     if   p >= open_peak || (open' && p >= close_peak)   open = 1, hang = hang_frames
 *     elif open' && hang' > 0                             open = 1, hang = hang' - 1
 *     else                                                open = 0, hang = 0
 * RANKING is that of mbx_levels.h with "open" as just decided: the key is the energy of THIS frame, at equal energy the smaller k
 * wins; a closed input has no key, and a held input competes with the energy it has now (there is no incumbency).  on = open when
 * loudest_n == 0; otherwise on = open and among the loudest_n largest keys of its bus.  The new state is {hang, open, on}.
 * WEIGHT.  The per-sample weight q(n) of an input, n = 0 .. 159, R = 1 << ramp_log2:
 *     on' && on              R                        steady
 *     !on' && on             min(n + 1, R)            rising: the fade-in starts in the frame that opens the gate -- no look-ahead, no delay
 *     on' && !on             R - min(n + 1, R)        falling
 *     !on' && !on            0                        off
 * SUM.
 *     term   = (x * gain_q12 + 2048) >> 12               as in mbx_mixdown.h
 *     ramped = (term * q(n) + (R >> 1)) >> ramp_log2     an arithmetic shift; |term * q| <= (2^18 + 1) * 2^7 < 2^26
 *     acc    = the sum of the ramped; y = clamp(acc, -32768, 32767); int16 or the G.711 byte, as in mbx_mixdown.h
 * q = R gives ramped == term exactly ((term * R + R / 2) >> ramp_log2 = term, R / 2 < R) and q = 0 gives 0, so an input at steady
 * state contributes the bits it contributes to mbx_mixdown.  |ramped| <= |term| + 1 <= 2^18 + 2, and 4,096 * (2^18 + 2) < 2^31: the
 * int32 accumulator of a full bus cannot overflow.  The sum is over integers: its order does not matter.
 *
 * Two identities follow:
 *   a hold {t, t, 0, n, 0} on zeroed state gives, in every frame, the bytes of mbx_mixdown_gated under {t, n};
 *   any hold with open_peak = 0 and loudest_n = 0 gives, from the second frame on, the bytes of mbx_mixdown -- from the first frame on
 *   if ramp_log2 = 0.
 * Also: close_peak = 0 latches an input open once it has opened.  A row that occurs twice in a bus has two states.  The hold may
 * change from call to call; a smaller loudest_n, or a hold with loudest_n > 0 after one with 0, can make any number of inputs fall at
 * once, and every one of them is faded out.  Ramps are at most 128 samples and never cross a frame.
 *
 * Alignment and overlap are those of mbx_mixdown_gated (mbx_levels.h, Alignment): d_pcm16 16, d_levels 16, d_out 16 as int16 and 8 as
 * bytes; d_levels overlaps neither d_pcm16 nor d_out.  The state object owns its device memory.
 *
 * ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME: mbx_mixdown_held reads and writes the state on `stream`; calls with the same
 * state on two streams, or mbx_gate_state_get / _set / _reset on another stream than the one its launches are queued on, are the
 * caller's to order.  The call is replay-safe: nothing about the state is decided on the host, so a captured graph that holds one
 * mbx_mixdown_held and is replayed three times advances the state three frames.
 */
#ifndef MBX_HOLD_PUBLIC_H
#define MBX_HOLD_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_levels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_HOLD_MAX_RAMP_LOG2 7

typedef struct mbx_mixdown_hold {
    uint16_t open_peak;    /* a closed input opens when the peak of its row >= open_peak (0 .. 32768) */
    uint16_t close_peak;   /* an open input stays open while peak >= close_peak; must be <= open_peak */
    uint16_t hang_frames;  /* frames an open input is held after its peak fell below close_peak */
    uint8_t  loudest_n;    /* 0: every open input; 1 .. MBX_GATE_MAX_LOUDEST */
    uint8_t  ramp_log2;    /* fades take R = 1 << ramp_log2 samples, 0 .. 7 (1 .. 128 samples; 0: a step) */
} mbx_mixdown_hold;

typedef struct mbx_gate_input_state { uint16_t hang_left; uint8_t open; uint8_t on; } mbx_gate_input_state;  /* all zero: closed */

typedef struct mbx_gate_state mbx_gate_state;

/* An opaque object on the plan's device, which must be the current one: one state record per input of the plan, zeroed, and the
 * per-input workspace the launches need (5 bytes per input in all).  A state is tied to the plan it was made for: the plan must
 * outlive it, and mbx_mixdown_held refuses it beside another plan.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL out or plan.  Then: a plan of another device than the current. */
int mbx_gate_state_create(mbx_gate_state** out, const mbx_mixdown_plan* plan);
int mbx_gate_state_destroy(mbx_gate_state* st);                 /* NULL allowed */
int mbx_gate_state_inputs(const mbx_gate_state* st);            /* records it holds: the inputs of its plan; NULL: MBE_STATUS_INVALID_ARGUMENT */
/* every record to zero (closed), asynchronously on `stream` */
int mbx_gate_state_reset(mbx_gate_state* st, void* stream);
/* the records to / from HOST memory, mbx_gate_state_inputs() of them in the order of the plan's input arrays; both synchronise
 * `stream`.  A console reads its talker lights from get: `on` says who is on the bus.  set refuses (MBE_STATUS_INVALID_ARGUMENT,
 * nothing written) records whose open or on is not 0 or 1, or that are on without open. */
int mbx_gate_state_get(const mbx_gate_state* st, mbx_gate_input_state* host, void* stream);
int mbx_gate_state_set(mbx_gate_state* st, const mbx_gate_input_state* host, void* stream);

/* Two or three launches behind mbx_pcm_levels on the same stream, as mbx_mixdown_gated: the buses of `plan` under `hold`, and `state`
 * advanced by one frame.  Asynchronous; never synchronises; may be captured.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL hold or state; close_peak > open_peak; open_peak > 32768;
 * loudest_n > MBX_GATE_MAX_LOUDEST; ramp_log2 > 7; a state of another plan; everything mbx_mixdown_gated refuses. */
int mbx_mixdown_held(const mbx_mixdown_plan* plan, const mbx_mixdown_hold* hold, mbx_gate_state* state, int form, const int16_t* d_pcm16,
                     size_t nrows, const mbx_row_level* d_levels, void* d_out, void* stream);

/* Host only, no device: the definition.  The arguments of mbx_mixdown_gated_host with a hold; `state` is in and out, one record per
 * input (bus_offset[n_buses] of them); it computes the levels itself.  The refusals of mbx_mixdown_gated_host, those of the hold, a
 * NULL state while a bus has an input, and a bad state record (see mbx_gate_state_set). */
int mbx_mixdown_held_host(int form, const mbx_mixdown_hold* hold, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                          const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, mbx_gate_input_state* state, void* out);

/* mbx_session_next_mixdown_gated with a held gate: the session needs MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS; the state object
 * brings its own memory.  It shares the buses slot of the attachment with mbx_session_next_mixdown[_gated]: whichever was called last
 * holds.  It lasts one submit; a submit that refuses uses the attachment up and leaves the state as it was.  The session's compute
 * stream is in order, so a state advances in submit order; mbx_gate_state_get / _set / _reset on a state with submits in flight are the
 * caller's to order, with mbx_session_wait first.  The levels launch runs once per submit.  A NULL out clears the slot and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: what mbx_session_next_mixdown_gated refuses, with the hold's refusals in place of the gate's; a NULL
 * state; a state of another plan. */
int mbx_session_next_mixdown_held(struct mbx_session* s, const mbx_mixdown_plan* plan, int form, const mbx_mixdown_hold* hold,
                                  mbx_gate_state* state, void* out);

#ifdef __cplusplus
}
#endif

#endif /* MBX_HOLD_PUBLIC_H */
