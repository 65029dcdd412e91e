/*
 * mbx_filter.h -- filtered rows of the MI355X batch launcher (libmbx_hip.so): a per-stream cascade of 1 .. 4 second-order sections
 * (biquads) over the int16 rows a step wrote, on the device, BEHIND the step and IN FRONT OF the gain of mbx_agc.h.  The synthesiser
 * leaves low-frequency thump and DC steps at frame repeats, mutes and erasures; every host that plays or records decoded frames
 * high-passes them before its gain, and often notches or band-limits them as well.  This header does that where the rows are: one
 * 32-byte state record per stream, kept on the device between calls, one launch per call, exact in integers -- the device's bits are
 * those of mbx_pcm_filter_host and of mbelib-neo_amd/filters.py (step).  The launches of mbx_agc.h, mbx_pcm8.h, mbx_levels.h,
 * mbx_mixdown.h, mbx_hold.h and mbx_resample.h then run on the filtered rows unchanged.
 *
 * Conventions are those of mbx_agc.h: `stream` is a hipStream_t passed as void*, the launcher is asynchronous on `stream`, never
 * synchronises, and returns 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every refusal of an
 * argument comes before a device is asked for.
 *
 * COEFFICIENTS are Q14 int16: unity is 16384, a coefficient lies in -2 .. just under 2.  The transfer function of a section is
 *     (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2).
 * The library ships no designer, as it ships none for the taps of mbx_resample.h: mbelib-neo_amd/filters.py has highpass, lowpass,
 * notch and peaking.
 *
 * DEFINITION.  Per sample, section s computes from its input x[n], its own y1, y2 and the fraction e it saved (direct form I with
 * fraction saving):
 *     ff  = b0 * x[n] + b1 * x1 + b2 * x2                  int32
 *     fb  = a1 * y1 + a2 * y2                              int32
 *     acc = ff - fb + e                                    34 bits signed
 *     q   = acc >> 14                                      an arithmetic shift: it floors
 *     e   = acc - (q << 14)                                0 .. 16383: the fraction is carried into the next sample, not dropped
 *     y[n] = clamp(q, -32768, 32767)
 *     x2 = x1, x1 = x[n];  y2 = y1, y1 = y[n]
 * The input of section s + 1 is y of section s, so its x1, x2 ARE section s's y1, y2, and the record holds them once.
 * BOUNDS.  A filter is refused unless every section has |b0| + |b1| + |b2| <= 65535 and |a1| + |a2| <= 65535.  Then
 * |ff| <= 32768 * 65535 < 2^31 and |fb| <= 32768 * 65535 < 2^31: each partial sum is an int32 built from 16 x 16-bit products (a
 * 24-bit multiply-add is enough, no 64-bit multiply is needed).  Only the combination is wider: |acc| <= 2 * 32768 * 65535 + 16383
 * < 2^33 fits 34 bits signed, |q| < 2^19, so acc >> 14 is one funnel shift of a 64-bit add.  STABILITY IS THE CALLER'S: the clamp
 * bounds every value whatever the coefficients.  ZERO-INPUT LIMIT CYCLES of a few LSB exist for some sections (a 4th-order
 * low-pass at 3.4 kHz idles at +-1 behind a burst): they are part of the definition.
 *
 * Four identities follow:
 *   {16384, 0, 0 | 0, 0} returns the input bit for bit;
 *   {0, 16384, 0 | 0, 0} and {0, 0, 16384 | 0, 0} are delays of one and of two samples, across frames and calls: 2 S samples through S
 *   sections of the second;
 *   {8192, 0, 0 | 0, 0} on a constant 1 gives 0, 1, 0, 1 ...: the fraction is saved;
 *   {16384, 0, 0 | -16384, 0} is an integrator that runs into the rail and stays there.
 *
 * LAYOUT.  Rows are stream-major as everywhere in mbx.h: row i * T + t is frame t of entry i, and entry i uses the record
 * d_stream[i] (NULL: record i).  The T frames of an entry are processed in order inside the ONE launch of a call, the record written
 * once behind the last row.  A launch under S sections leaves the y1, y2, e of sections >= S of a record as they were.  An entry
 * whose d_stream names a record outside 0 .. streams - 1 RUNS OVER A ZERO RECORD and stores none (the device cannot refuse, and must
 * not index beyond the state; a filter has no unity to fall back on: this is the rule of mbx_resample.h, not the pass-through of
 * mbx_agc.h).  An entry listed TWICE in one launch is the caller's to avoid: two entries would race on one record.
 *
 * Alignment: d_in and d_out 16, as d_pcm16 in the table of mbx_levels.h.  d_out == d_in is allowed (the rows of a frame are read in
 * full before any of them is stored); any other overlap of the two arrays is refused.
 *
 * ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME: mbx_pcm_filter reads and writes the state on `stream`; calls with the same
 * state on two streams, or mbx_filter_state_get / _set / _reset on another stream than the one its launches are queued on, are the
 * caller's to order.  The call is replay-safe: the filter travels BY VALUE in the kernel arguments and nothing about the state is
 * decided on the host, so a captured graph that holds one mbx_pcm_filter and is replayed three times advances the state three frames,
 * under the coefficients of the capture.
 */
#ifndef MBX_FILTER_PUBLIC_H
#define MBX_FILTER_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_FILTER_MAX_SECTIONS 4
#define MBX_FILTER_UNITY_Q14 16384
#define MBX_FILTER_COEFF_BOUND 65535   /* |b0| + |b1| + |b2| and |a1| + |a2| of a section, at most */

typedef struct mbx_filter_section { int16_t b0, b1, b2, a1, a2; } mbx_filter_section;

typedef struct mbx_filter {
    uint8_t            sections;   /* 1 .. MBX_FILTER_MAX_SECTIONS */
    uint8_t            zero[3];    /* must be 0 */
    mbx_filter_section sec[MBX_FILTER_MAX_SECTIONS];   /* sections beyond `sections` are ignored but must be zero */
} mbx_filter;                      /* 44 bytes */

typedef struct mbx_filter_record {
    int16_t x1, x2;                /* the last two inputs of section 0 */
    struct { int16_t y1, y2; uint16_t e; /* 0 .. 16383 */ } sec[MBX_FILTER_MAX_SECTIONS];
    uint16_t zero[2];              /* must be 0 */
} mbx_filter_record;               /* 32 bytes; fresh or reset: all zero */

typedef struct mbx_filter_state mbx_filter_state;

/* An opaque object on the current device: `streams` records, every one zero.  The state object owns its device memory.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL out; streams < 0. */
int mbx_filter_state_create(mbx_filter_state** out, int streams);
int mbx_filter_state_destroy(mbx_filter_state* st);                 /* NULL allowed */
int mbx_filter_state_streams(const mbx_filter_state* st);           /* records it holds; NULL: MBE_STATUS_INVALID_ARGUMENT */
/* records first .. first + count - 1 to zero, asynchronously on `stream`: a channel that starts a new call.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL state; a range outside the records. */
int mbx_filter_state_reset(mbx_filter_state* st, int first, int count, void* stream);
/* `count` records from `first` to / from HOST memory; both synchronise `stream`.  set refuses (MBE_STATUS_INVALID_ARGUMENT, nothing
 * written) a record with an e above 16383 or a non-zero pad; both refuse a NULL state, a range outside the records, and a NULL host
 * with count > 0. */
int mbx_filter_state_get(const mbx_filter_state* st, int first, int count, mbx_filter_record* host, void* stream);
int mbx_filter_state_set(mbx_filter_state* st, int first, int count, const mbx_filter_record* host, void* stream);

/* One launch behind a step on the same stream: the n * T rows of d_in filtered into d_out, and the records of the n entries advanced
 * by T frames.  Asynchronous; never synchronises; may be captured.  n == 0 or T == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL filter, state, d_in or d_out; sections outside 1 .. 4; a zero byte
 * that is not 0; a section over a bound; a non-zero coefficient beyond `sections`; a negative n or T; n * T above 2^31 - 1; a pointer
 * below its alignment; d_out overlapping d_in without being equal to it.  Then: a state of another device than the current one. */
int mbx_pcm_filter(const mbx_filter* filter, mbx_filter_state* state, const int32_t* d_stream /* n entries, NULL: 0 .. n-1 */, int n, int T,
                   const int16_t* d_in, int16_t* d_out, void* stream);

/* Host only, no device: the definition.  `state` is in and out, `streams` records; stream_index as d_stream, in host memory (an
 * entry outside 0 .. streams - 1 runs over a zero record as on the device).  The refusals of mbx_pcm_filter that do not need a device,
 * without the alignment; a negative streams; a state record mbx_filter_state_set would refuse. */
int mbx_pcm_filter_host(const mbx_filter* filter, mbx_filter_record* state, int streams, const int32_t* stream_index, int n, int T,
                        const int16_t* in, int16_t* out);

/* The NEXT submit of a session filters its int16 rows under `filter` with the caller's `state`, in place in the session's own rows, as
 * the FIRST launch behind the step, IN FRONT OF an AGC attached with mbx_session_next_agc: every int16-derived output of that submit
 * is then of the filtered (and then levelled) rows -- the caller's pcm16, mbx_session_next_pcm8, mbx_session_next_levels and every
 * mbx_session_next_mixdown*.  pcmf, results and records are untouched.  The state advances even when the submit takes no
 * int16-derived output.  A frames, soft or keyed submit without an index uses records 0 .. n-1; an indexed or a bursts submit uses its
 * stream index, on the device.  mbx_session_submit_burst_groups REFUSES a submit with a filter attached (its groups have different
 * frame counts), and a mixed session takes only groups.
 * The attachment lasts one submit and is used up whether the submit queues or refuses; a submit that refuses leaves the state as it
 * was.  The session's compute stream is in order, so a state advances in submit order; mbx_filter_state_get / _set / _reset on a state
 * with submits in flight are the caller's to order, with mbx_session_wait first.  A NULL state clears the attachment and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL session or filter; what mbx_pcm_filter refuses of filter; a session created without an output
 * that has int16 rows (MBX_SESSION_PCM16, _PCM8, _MIXDOWN or _LEVELS); a state of fewer records than mbx_session_streams(), or of
 * another device than the session. */
int mbx_session_next_filter(struct mbx_session* s, const mbx_filter* filter, mbx_filter_state* state);

#ifdef __cplusplus
}
#endif

#endif /* MBX_FILTER_PUBLIC_H */
