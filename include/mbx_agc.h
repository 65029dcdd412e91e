/*
 * mbx_agc.h -- levelled rows of the MI355X batch launcher (libmbx_hip.so): a per-stream automatic gain control (AGC) over the int16
 * rows a step wrote, on the device, BEHIND the step and in front of every other output launch.  Radios on one talkgroup differ by
 * 20 dB and more, and the decoder's int16 scale is fixed (mbe_floattoshort): a host that plays, records or mixes decoded frames
 * runs a gain over them first.  This header does that where the rows are: one 4-byte state record per stream, kept on the device
 * between calls, one launch per call, exact in integers -- the device's bits are those of mbx_pcm_agc_host and of
 * mbelib-neo_amd/agc.py (step).  The launches of mbx_pcm8.h, mbx_levels.h, mbx_mixdown.h and mbx_hold.h then run on the levelled
 * rows unchanged.
 *
 * Conventions are those of mbx_levels.h: `stream` is a hipStream_t passed as void*, the launcher is asynchronous on `stream`, never
 * synchronises, and returns 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every refusal of an
 * argument comes before a device is asked for.
 *
 * GAINS are Q10: unity is 1024, a gain lies in 1 .. 32768 (x 1/1024 .. x 32).
 *
 * DEFINITION.  Per row of 160 samples, p = the largest |x[n]| taken in int32 (0 .. 32768: the peak of mbx_levels.h); the state in
 * front of the row is (g0, env0):
 *     if p < floor_peak:                                        FROZEN: pauses and comfort noise do not pump the gain
 *         g1 = g0, env = env0
 *     else:
 *         env  = max(p, env0 - ((env0 * release_q8 + 255) >> 8))        rises at once, decays by release/256 per frame, reaches 0
 *         want = clamp((target_peak << 10) / env, min_gain, max_gain)   an unsigned integer division; env >= p >= floor_peak >= 1
 *         g1   = want                                          if want <= g0     (falls at once)
 *              = min(want, g0 + ((g0 * rise_q8 + 255) >> 8))   otherwise         (rises by at most rise/256 of itself per frame)
 *     R = 1 << ramp_log2
 *     g(n) = g0 + (((g1 - g0) * min(n + 1, R)) >> ramp_log2)    an arithmetic shift; g(n) = g1 for n >= R - 1
 *     y[n] = clamp((x[n] * g(n) + 512) >> 10, -32768, 32767)    an arithmetic shift
 *     the new state: (g1, env)
 * BOUNDS.  Everything fits int32 / uint32: |x * g| <= 2^15 * 2^15 = 2^30, so |x * g + 512| < 2^31; |(g1 - g0) * R| < 2^15 * 2^7 =
 * 2^22; env0 * release_q8 + 255 <= 2^15 * 255 + 255 < 2^24; g0 * rise_q8 + 255 < 2^24; target_peak << 10 < 2^25.  g(n) lies between
 * g0 and g1, so it is a gain.
 * There is NO LOOK-AHEAD: a frame that makes the gain fall may clip in its first R samples, and that is part of the definition.
 * The ramp is at most 128 samples and never crosses a frame.
 *
 * Three identities follow:
 *   min_gain_q10 = max_gain_q10 = 1024 on a fresh state returns the input bit for bit ((x * 1024 + 512) >> 10 = x);
 *   min_gain_q10 = max_gain_q10 = G on a state at gain G is the static gain (x * G + 512) >> 10, clamped;
 *   rise_q8 = 0 never raises a gain.
 *
 * LAYOUT.  Rows are stream-major as everywhere in mbx.h: row i * T + t is frame t of entry i, and entry i uses the record
 * d_stream[i] (NULL: record i).  The T frames of an entry are processed in order inside the ONE launch of a call, the gain carried
 * from frame to frame, the record written once at the end.  An entry whose d_stream names a record outside 0 .. streams - 1 is
 * PASSED THROUGH: its rows reach d_out bit for bit and no record is touched (the device cannot refuse, and must not index beyond
 * the state).  An entry listed TWICE in one launch is the caller's to avoid: two entries would race on one record.
 *
 * Alignment: d_in and d_out 16, as d_pcm16 in the table of mbx_levels.h.  d_out == d_in is allowed (a lane reads all its samples of a
 * row before it stores any); any other overlap of the two arrays is refused.
 *
 * ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME: mbx_pcm_agc reads and writes the state on `stream`; calls with the same state
 * on two streams, or mbx_agc_state_get / _set / _reset on another stream than the one its launches are queued on, are the caller's
 * to order.  The call is replay-safe: nothing about the state is decided on the host, so a captured graph that holds one mbx_pcm_agc
 * and is replayed three times advances the state three frames.
 */
#ifndef MBX_AGC_PUBLIC_H
#define MBX_AGC_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx.h"
#include "mbx_hold.h"   /* MBX_HOLD_MAX_RAMP_LOG2: the ramps are those of the held gate */

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_AGC_UNITY_Q10 1024
#define MBX_AGC_MAX_GAIN_Q10 32768
#define MBX_AGC_MAX_RAMP_LOG2 MBX_HOLD_MAX_RAMP_LOG2

typedef struct mbx_agc {
    uint16_t target_peak;    /* where the envelope is brought to: 1 .. 32767 */
    uint16_t floor_peak;     /* a row whose peak is below it freezes the state: 1 .. 32768 */
    uint16_t min_gain_q10;   /* 1 .. 32768, at most max_gain_q10 */
    uint16_t max_gain_q10;   /* 1 .. 32768 */
    uint8_t  release_q8;     /* the envelope decays by release_q8 / 256 of itself per frame: 0 .. 255 (0: it never decays) */
    uint8_t  rise_q8;        /* the gain rises by at most rise_q8 / 256 of itself per frame: 0 .. 255 (0: it never rises) */
    uint8_t  ramp_log2;      /* the gain moves over R = 1 << ramp_log2 samples: 0 .. MBX_AGC_MAX_RAMP_LOG2 (0: a step) */
    uint8_t  zero;           /* must be 0 */
} mbx_agc;

typedef struct mbx_agc_record { uint16_t gain_q10; uint16_t env; } mbx_agc_record;   /* fresh or reset: {1024, 0} */

typedef struct mbx_agc_state mbx_agc_state;

/* An opaque object on the current device: `streams` records, every one {1024, 0}.  The state object owns its device memory.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL out; streams < 0. */
int mbx_agc_state_create(mbx_agc_state** out, int streams);
int mbx_agc_state_destroy(mbx_agc_state* st);                 /* NULL allowed */
int mbx_agc_state_streams(const mbx_agc_state* st);           /* records it holds; NULL: MBE_STATUS_INVALID_ARGUMENT */
/* records first .. first + count - 1 to {1024, 0}, asynchronously on `stream`: a channel that starts a new call.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL state; a range outside the records. */
int mbx_agc_state_reset(mbx_agc_state* st, int first, int count, void* stream);
/* `count` records from `first` to / from HOST memory; both synchronise `stream`.  set refuses (MBE_STATUS_INVALID_ARGUMENT, nothing
 * written) a record whose gain_q10 is 0 or above 32768 or whose env is above 32768; both refuse a NULL state, a range outside the
 * records, and a NULL host with count > 0. */
int mbx_agc_state_get(const mbx_agc_state* st, int first, int count, mbx_agc_record* host, void* stream);
int mbx_agc_state_set(mbx_agc_state* st, int first, int count, const mbx_agc_record* host, void* stream);

/* One launch behind a step on the same stream: the n * T rows of d_in levelled into d_out, and the records of the n entries advanced
 * by T frames.  Asynchronous; never synchronises; may be captured.  n == 0 or T == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL agc, state, d_in or d_out; a field of agc out of its range;
 * min_gain_q10 > max_gain_q10; zero != 0; a negative n or T; n * T above 2^31 - 1; a pointer below its alignment; d_out overlapping
 * d_in without being equal to it.  Then: a state of another device than the current one. */
int mbx_pcm_agc(const mbx_agc* agc, mbx_agc_state* state, const int32_t* d_stream /* n entries, NULL: 0 .. n-1 */, int n, int T,
                const int16_t* d_in, int16_t* d_out, void* stream);

/* Host only, no device: the definition.  `state` is in and out, `streams` records; stream_index as d_stream, in host memory (an
 * entry outside 0 .. streams - 1 is passed through as on the device).  The refusals of mbx_pcm_agc that do not need a device, without
 * the alignment; a negative streams; a state record mbx_agc_state_set would refuse. */
int mbx_pcm_agc_host(const mbx_agc* agc, mbx_agc_record* state, int streams, const int32_t* stream_index, int n, int T,
                     const int16_t* in, int16_t* out);

/* The NEXT submit of a session levels its int16 rows under `agc` with the caller's `state`, in place in the session's own rows, as
 * the FIRST launch behind the step: every int16-derived output of that submit is then of the levelled rows -- the caller's pcm16,
 * mbx_session_next_pcm8, mbx_session_next_levels and every mbx_session_next_mixdown*.  pcmf, results and records are untouched.  The
 * state advances even when the submit takes no int16-derived output.  A frames, soft or keyed submit without an index uses records
 * 0 .. n-1; an indexed or a bursts submit uses its stream index, on the device.  mbx_session_submit_burst_groups REFUSES a submit with
 * an AGC attached (its groups have different frame counts), and a mixed session takes only groups.
 * The attachment lasts one submit and is used up whether the submit queues or refuses; a submit that refuses leaves the state as it
 * was.  The session's compute stream is in order, so a state advances in submit order; mbx_agc_state_get / _set / _reset on a state
 * with submits in flight are the caller's to order, with mbx_session_wait first.  A NULL state clears the attachment and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL session or agc; what mbx_pcm_agc refuses of agc; a session created without an output that has
 * int16 rows (MBX_SESSION_PCM16, _PCM8, _MIXDOWN or _LEVELS); a state of fewer records than mbx_session_streams(), or of another
 * device than the session. */
int mbx_session_next_agc(struct mbx_session* s, const mbx_agc* agc, mbx_agc_state* state);

#ifdef __cplusplus
}
#endif

#endif /* MBX_AGC_PUBLIC_H */
