/*
 * mbx_resample.h -- wide rows of the MI355X batch launcher (libmbx_hip.so): the 8 kHz int16 rows a step wrote, or the bus rows the
 * mix-down and the limiter wrote, UPSAMPLED to 16, 24, 32 or 48 kHz on the device by a polyphase FIR interpolator with the caller's
 * taps.  Nothing a host feeds -- a sound card, a wide-band RTP payload, a recorder -- runs at 8 kHz, and a host that takes the rows
 * back upsamples them in a per-sample loop.  This header does that where the rows are: one 64-byte history record per row kept on the
 * device between calls, one launch per call, exact in integers -- the device's bits are those of mbx_pcm_resample_host and of
 * mbelib-neo_amd/resample.py (step).  The library ships NO filter designer and owns no tables, as it owns no interleave schedule: the
 * taps are the caller's (resample.py has design(), the one convenience a host needs).
 *
 * Conventions are those of mbx_limit.h: `stream` is a hipStream_t passed as void*, the launcher is asynchronous on `stream`, never
 * synchronises, and returns 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every refusal of an
 * argument comes before a device is asked for.
 *
 * TAPS are Q14: unity is 16384.  The prototype filter h[0 .. K*L-1] runs at the OUTPUT rate; phase p of it is h[p], h[p + L], ...,
 * h[p + (K-1)*L], K taps.
 *
 * THE RECORD of a row is the LAST 32 INPUT SAMPLES of that row, oldest first.  It does not depend on K: a caller may change the filter
 * between calls, and the result is still defined.  Every int16 value is a valid record, so mbx_resample_state_set refuses no record.
 *
 * DEFINITION.  Per input row x[0 .. 159], the record in front of it is hist[0 .. 31]:
 *     x_ext[m] = hist[32 + m]  for m = -32 .. -1
 *     x_ext[m] = x[m]          for m = 0 .. 159
 *     for n = 0 .. 159, p = 0 .. L-1:
 *         acc      = sum over k = 0 .. K-1 of  taps[p + k*L] * x_ext[n - k]          int32
 *         y[n*L+p] = clamp((acc + 8192) >> 14, -32768, 32767)                        an arithmetic shift
 *     the new record: x_ext[128 .. 159]
 * The output row is 160 * L int16.  The filter is causal: its group delay is (K*L - 1) / 2 output samples, and NO FRAME OF LATENCY is
 * added.
 *
 * BOUND.  A filter is refused unless every phase has  sum over k of |taps[p + k*L]| <= 65535.  Then |acc| <= 65535 * 32768 =
 * 2,147,450,880, every partial sum of acc lies inside that too, and acc + 8192 <= 2,147,459,072 < 2^31: everything fits int32.
 * A FINAL CLAMP IS NEEDED: interpolation overshoots -- between two full-scale samples a band-limited curve passes beyond them -- and a
 * phase may have a gain above unity.
 *
 * Four identities follow:
 *   HOLD.      taps[p] = 16384 for every p and everything else 0: y[n*L+p] == x[n] bit for bit;
 *   DELAY.     taps[p + (K-1)*L] = 16384 and everything else 0: y[n*L+p] == x_ext[n - (K-1)] -- this reads the history across frames
 *              and across calls;
 *   BATCHING.  one call with T = 3 is three calls with T = 1: frame t > 0 of an entry takes its history from the tail of row t - 1 of
 *              the INPUT;
 *   DC.        every phase sums to exactly 16384: a constant row over a constant history of the same value is that constant.
 *
 * LAYOUT.  Rows are stream-major as everywhere in mbx.h: input row i * T + t is frame t of entry i, output row i * T + t its 160 * L
 * samples, and entry i uses the record d_stream[i] (NULL: record i).  An entry whose d_stream names a record outside 0 .. streams - 1 is
 * resampled over a ZERO HISTORY and stores no record (the device cannot refuse, and must not index beyond the state).  An entry listed
 * TWICE in one launch is the caller's to avoid: two entries would race on one record.
 *
 * Alignment: d_in and d_out 16, as d_pcm16 in the table of mbx_levels.h.  ANY overlap of d_out with d_in is refused: the sizes differ,
 * so there is no in-place form.
 *
 * ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME: mbx_pcm_resample reads and writes the state on `stream`; calls with the same
 * state on two streams, or mbx_resample_state_get / _set / _reset on another stream than the one its launches are queued on, are the
 * caller's to order.  The call is replay-safe: the filter travels by value with the launch and nothing about the state is decided on
 * the host, so a captured graph that holds one mbx_pcm_resample and is replayed three times advances the state three frames.
 */
#ifndef MBX_RESAMPLE_PUBLIC_H
#define MBX_RESAMPLE_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_RESAMPLE_MAX_TAPS 192          /* 32 taps per phase x 6 phases */
#define MBX_RESAMPLE_UNITY_Q14 16384
#define MBX_RESAMPLE_HISTORY 32

typedef struct mbx_resample {
    uint8_t L;            /* output samples per input sample: 2, 3, 4 or 6 (16, 24, 32, 48 kHz) */
    uint8_t K;            /* taps per phase: even, 2 .. 32 */
    uint8_t zero[2];      /* must be 0 */
    int16_t taps[MBX_RESAMPLE_MAX_TAPS];   /* Q14 prototype filter h[0 .. K*L-1]; taps beyond K*L must be 0 */
} mbx_resample;

typedef struct mbx_resample_record { int16_t hist[MBX_RESAMPLE_HISTORY]; } mbx_resample_record;   /* fresh or reset: zeros */

typedef struct mbx_resample_state mbx_resample_state;

/* An opaque object on the current device: `streams` records of 64 bytes, every one zeros.  The state object owns its device memory.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL out; streams < 0. */
int mbx_resample_state_create(mbx_resample_state** out, int streams);
int mbx_resample_state_destroy(mbx_resample_state* st);            /* NULL allowed */
int mbx_resample_state_streams(const mbx_resample_state* st);      /* records it holds; NULL: MBE_STATUS_INVALID_ARGUMENT */
/* records first .. first + count - 1 to zeros, asynchronously on `stream`: a channel that starts a new call.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL state; a range outside the records. */
int mbx_resample_state_reset(mbx_resample_state* st, int first, int count, void* stream);
/* `count` records from `first` to / from HOST memory; both synchronise `stream`.  Every record is valid: set refuses none.  Both refuse
 * (MBE_STATUS_INVALID_ARGUMENT) a NULL state, a range outside the records, and a NULL host with count > 0. */
int mbx_resample_state_get(const mbx_resample_state* st, int first, int count, mbx_resample_record* host, void* stream);
int mbx_resample_state_set(mbx_resample_state* st, int first, int count, const mbx_resample_record* host, void* stream);

/* ONE launch behind a step or a bus launch on the same stream: the n * T rows of d_in resampled into the n * T rows of 160 * L samples
 * of d_out, and the records of the n entries advanced by T frames.  Asynchronous; never synchronises; may be captured.  n == 0 or
 * T == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL rs, state, d_in or d_out; L that is none of 2, 3, 4, 6; K odd or
 * outside 2 .. 32; a zero byte != 0; a nonzero tap beyond K * L; a phase over the bound; a negative n or T; n * T * 160 * L above
 * 2^31 - 1; a pointer below its alignment; d_out overlapping d_in.  Then: a state of another device than the current one. */
int mbx_pcm_resample(const mbx_resample* rs, mbx_resample_state* state, const int32_t* d_stream /* n entries, NULL: 0 .. n-1 */, int n, int T,
                     const int16_t* d_in, int16_t* d_out, void* stream);

/* Host only, no device: the definition.  `records` is in and out, `streams` of them; stream_index as d_stream, in host memory (an
 * entry outside 0 .. streams - 1 runs over a zero history and stores no record, as on the device).  The refusals of mbx_pcm_resample
 * that do not need a device, without the alignment; a negative streams; NULL records with streams > 0. */
int mbx_pcm_resample_host(const mbx_resample* rs, mbx_resample_record* records, int streams, const int32_t* stream_index, int n, int T,
                          const int16_t* in, int16_t* out);

/* The NEXT submit of a session delivers its BUSES resampled as well: the bus buffer of the slot -- behind mbx_session_next_mixdown,
 * _gated or _held, and behind the limiter of mbx_session_next_limit where one is attached -- takes one more launch on the session's
 * compute stream, mbx_pcm_resample (T = 1, record b for bus b) into a buffer of the slot that is made by the first resampled submit,
 * and `out` (host memory, the plan's buses * 160 * L int16; pinned memory is written in place, pageable memory through the slot's
 * staging) is delivered beside the caller's own buses.  No outputs bit is needed.  The per-stream ROWS of a session are not resampled
 * here: mbx_pcm_resample with d_stream serves them.
 * The submit REFUSES, before anything is queued and with the attachment used up, when a resampler is attached and no buses are, when
 * the buses are in another form than MBX_MIXDOWN_PCM16, when the plan has more buses than the state has records, or when the state is
 * of another device than the session.  mbx_session_submit_burst_groups may take it: buses have no T.
 * The attachment lasts one submit and is used up whether the submit queues or refuses; a submit that refuses leaves the state as it
 * was.  The session's compute stream is in order, so a state advances in submit order; mbx_resample_state_get / _set / _reset on a
 * state with submits in flight are the caller's to order, with mbx_session_wait first.  A NULL state clears the attachment and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL session, rs or out; what mbx_pcm_resample refuses of rs; a state of another device than the
 * session. */
int mbx_session_next_resample(struct mbx_session* s, const mbx_resample* rs, mbx_resample_state* state, int16_t* out);

#ifdef __cplusplus
}
#endif

#endif /* MBX_RESAMPLE_PUBLIC_H */
