/*
 * mbx_limit.h -- limited buses of the MI355X batch launcher (libmbx_hip.so): a look-ahead peak limiter BEHIND the mix-down sums, on the
 * device.  mbx_mixdown.h ends a bus in y = clamp(acc, -32768, 32767): hard saturation of the sum.  Three talkers the AGC of mbx_agc.h
 * brought to 8000 each sum to 24,000, an all-call bus hits the rails, and a saturated bus crackles.  This header has two halves: the
 * bus launches of mbx_mixdown.h, mbx_levels.h and mbx_hold.h with an int32 SUMS output (the sum in front of the clamp), and ONE launch
 * that turns sums into limited int16 / mu-law / A-law bus rows, with one 4-byte state record per bus kept on the device between calls,
 * exact in integers -- the device's bits are those of mbx_bus_limit_host and of mbelib-neo_amd/limit.py (step).
 *
 * Conventions are those of mbx_agc.h: `stream` is a hipStream_t passed as void*, the launchers are asynchronous on `stream`, never
 * synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every refusal of an argument
 * comes before a device is asked for.
 *
 * GAINS are Q15: unity is 32768, a gain lies in 1 .. 32768.  The limiter only attenuates.
 *
 * DEFINITION.  Per bus row s[0 .. 159] (int32), the record in front of it is (g0, h0): a gain and a hold counter.
 *     M      = 1 << 22                                   the limiter's range: 128 x full scale
 *     s'[n]  = clamp(s[n], -M, M);   a[n] = |s'[n]|;   P = max a[n]
 *     need   = 32768                      if P <= ceiling
 *            = (ceiling << 15) / P        otherwise      an unsigned division; >= 8, because ceiling >= 1024 and P <= 2^22
 *     thr0   = (ceiling << 15) / g0                      a[n] * g0 > ceiling << 15  <=>  a[n] > thr0, without the wide product
 *     n*     = the first n with a[n] > thr0, else 160
 *     ATTACK (n* < 160, which is exactly need < g0):
 *         g1 = need;  h1 = hold_frames
 *         g(n) = g1 + (((g0 - g1) * clamp(n* - n, 0, R)) >> ramp_log2)          R = 1 << ramp_log2
 *                g0 until R samples in front of n*, g1 from n* on; a ramp the frame start cuts short begins with a step
 *     otherwise:
 *         h0 > 0:  g1 = g0, h1 = h0 - 1
 *         else:    g1 = min(need, g0 + (((32768 - g0) * release_q8 + 255) >> 8)), h1 = 0
 *         g(n) = g0 + (((g1 - g0) * min(n + 1, R)) >> ramp_log2)                the ramp of mbx_agc.h
 *     y[n] = (s'[n] * g(n) + 16384) >> 15                                        an arithmetic shift; the new record is (g1, h1)
 * The output is y as int16 (MBX_MIXDOWN_PCM16) or the G.711 byte of y exactly as mbx_pcm8.h defines it (MBX_MIXDOWN_ULAW, _ALAW).
 * The limiter sees its whole frame before it writes a sample: this is LOOK-AHEAD INSIDE THE FRAME, at no added latency.  The gain is
 * down before the first sample that needs it.
 *
 * BOUNDS.  |s'[n] * g(n)| <= ceiling << 15 < 2^30 for every sample: before n*, a[n] <= thr0 and g(n) <= g0, so a[n] * g(n) <=
 * thr0 * g0 <= ceiling << 15; from n* on g(n) = g1 <= need, and P * need <= ceiling << 15; without an attack g(n) <= max(g0, g1) <= need.
 * Hence |y[n]| <= ceiling ALWAYS: there is NO FINAL CLAMP, and none is needed.  (g0 - g1) * R <= 2^15 * 2^7 = 2^22; the release term
 * (32768 - g0) * release_q8 + 255 < 2^24.  Everything fits int32 / uint32.
 *
 * Three identities follow:
 *   ceiling = 32767 on a fresh state over sums inside -32767 .. 32767 returns them bit for bit: mbx_mixdown's PCM16 row;
 *   release_q8 = 0 never raises a gain;
 *   one call with T = 3 is three calls with T = 1.
 *
 * LAYOUT.  Row i * T + t is frame t of bus i and uses record i.  The T frames of a bus are processed in order inside the ONE launch of
 * a call, the gain carried from frame to frame, the record written once at the end.
 *
 * Alignment: d_sums 16; d_out 16 as int16 and 8 as bytes (the table of mbx_mixdown.h); the int32 d_out of the sums launches 16.  The
 * rows out of mbx_bus_limit must not overlap the sums in.
 *
 * ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME: mbx_bus_limit reads and writes the state on `stream`; calls with the same state
 * on two streams, or mbx_limit_state_get / _set / _reset on another stream than the one its launches are queued on, are the caller's
 * to order.  So is the scratch of the state (mbx_limit_state_sums).  The call is replay-safe: nothing about the state is decided on the
 * host, so a captured graph that holds one mbx_bus_limit and is replayed three times advances the state three frames.
 */
#ifndef MBX_LIMIT_PUBLIC_H
#define MBX_LIMIT_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx.h"
#include "mbx_hold.h"   /* the held gate, and MBX_HOLD_MAX_RAMP_LOG2: the ramps are those of the held gate (brings mbx_levels.h, mbx_mixdown.h) */

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_LIMIT_UNITY_Q15 32768
#define MBX_LIMIT_MIN_CEILING 1024
#define MBX_LIMIT_MAX_CEILING 32767
#define MBX_LIMIT_RANGE_LOG2 22
#define MBX_LIMIT_MAX_RAMP_LOG2 MBX_HOLD_MAX_RAMP_LOG2

typedef struct mbx_limit {
    uint16_t ceiling;       /* the level the output never exceeds: 1024 .. 32767 */
    uint8_t  release_q8;    /* share of the distance to unity regained per frame: 0 .. 255 (0: the gain never rises) */
    uint8_t  hold_frames;   /* frames the gain stays put behind the last attack: 0 .. 255 */
    uint8_t  ramp_log2;     /* the gain moves over R = 1 << ramp_log2 samples: 0 .. MBX_LIMIT_MAX_RAMP_LOG2 (0: a step) */
    uint8_t  zero[3];       /* must be 0 */
} mbx_limit;

typedef struct mbx_limit_record { uint16_t gain_q15; uint16_t hold_left; } mbx_limit_record;   /* fresh or reset: {32768, 0} */

typedef struct mbx_limit_state mbx_limit_state;

/* An opaque object on the current device: `buses` records, every one {32768, 0}, and a scratch of buses * 160 int32, 16-byte aligned
 * (mbx_limit_state_sums), for the sums between their launch and mbx_bus_limit.  The state object owns its device memory.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL out; buses < 0. */
int mbx_limit_state_create(mbx_limit_state** out, int buses);
int mbx_limit_state_destroy(mbx_limit_state* st);                /* NULL allowed */
int mbx_limit_state_buses(const mbx_limit_state* st);            /* records it holds; NULL: MBE_STATUS_INVALID_ARGUMENT */
/* records first .. first + count - 1 to {32768, 0}, asynchronously on `stream`.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL state; a range outside the records. */
int mbx_limit_state_reset(mbx_limit_state* st, int first, int count, void* stream);
/* `count` records from `first` to / from HOST memory; both synchronise `stream`.  set refuses (MBE_STATUS_INVALID_ARGUMENT, nothing
 * written) a record whose gain_q15 is 0 or above 32768 or whose hold_left is above 255; both refuse a NULL state, a range outside the
 * records, and a NULL host with count > 0. */
int mbx_limit_state_get(const mbx_limit_state* st, int first, int count, mbx_limit_record* host, void* stream);
int mbx_limit_state_set(mbx_limit_state* st, int first, int count, const mbx_limit_record* host, void* stream);
/* the device scratch: buses * 160 int32, 16-byte aligned; NULL for a NULL state.  Sessions use it, and callers may. */
int32_t* mbx_limit_state_sums(const mbx_limit_state* st);

/* ONE launch: the n * T rows of d_sums limited into d_out in `form` (MBX_MIXDOWN_PCM16: int16; _ULAW, _ALAW: bytes), and the records
 * 0 .. n - 1 advanced by T frames.  Asynchronous; never synchronises; may be captured.  n == 0 or T == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL limit, state, d_sums or d_out; a field of the limit out of its
 * range; a zero byte != 0; a negative n or T; n * T above 2^31 - 1; a form that is none of the three; a pointer below its alignment;
 * d_out overlapping d_sums; n above the buses of the state.  Then: a state of another device than the current one. */
int mbx_bus_limit(const mbx_limit* limit, mbx_limit_state* state, int n, int T, const int32_t* d_sums, int form, void* d_out, void* stream);

/* Host only, no device: the definition.  `records` is in and out, n of them.  The refusals of mbx_bus_limit that do not need a device,
 * without the alignment; NULL records with n > 0; a record mbx_limit_state_set would refuse. */
int mbx_bus_limit_host(const mbx_limit* limit, mbx_limit_record* records, int n, int T, const int32_t* sums, int form, void* out);

/* The SUMS launches: the arguments of their parents (mbx_mixdown, mbx_mixdown_gated, mbx_mixdown_held) without `form`; d_out is int32
 * [buses][160], 16-byte aligned.  They run the parent's launches and selection with the same arithmetic and store acc where the parent
 * stores clamp(acc): clamp(sums) IS the parent's PCM16 row.  They refuse what their parents refuse, the form apart.  The _host twins do
 * the same in host memory.  (The public `form` of the parents stays what it is: 3 is refused.) */
int mbx_mixdown_sums(const mbx_mixdown_plan* plan, const int16_t* d_pcm16, size_t nrows, int32_t* d_out, void* stream);
int mbx_mixdown_sums_host(int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12, const int16_t* pcm16,
                          size_t nrows, int32_t* out);
int mbx_mixdown_gated_sums(const mbx_mixdown_plan* plan, const mbx_mixdown_gate* gate, const int16_t* d_pcm16, size_t nrows,
                           const mbx_row_level* d_levels, int32_t* d_out, void* stream);
int mbx_mixdown_gated_sums_host(const mbx_mixdown_gate* gate, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                                const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, int32_t* out);
int mbx_mixdown_held_sums(const mbx_mixdown_plan* plan, const mbx_mixdown_hold* hold, mbx_gate_state* state, const int16_t* d_pcm16,
                          size_t nrows, const mbx_row_level* d_levels, int32_t* d_out, void* stream);
int mbx_mixdown_held_sums_host(const mbx_mixdown_hold* hold, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                               const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, mbx_gate_input_state* state, int32_t* out);

/* The NEXT submit of a session limits its buses under `limit` with the caller's `state`: the buses attached by
 * mbx_session_next_mixdown, _gated or _held take their sums launch into mbx_limit_state_sums(state), then mbx_bus_limit (T = 1) into
 * the session's bus buffer in the attached form, all on the session's compute stream.  The state brings its memory: no outputs bit
 * is needed.  The submit REFUSES, before anything is queued and with the attachment used up, when a limiter is attached and no buses
 * are, or when the plan has more buses than the state.  mbx_session_submit_burst_groups may take it: buses have no T.
 * The attachment lasts one submit and is used up whether the submit queues or refuses; a submit that refuses leaves the state as it
 * was.  The session's compute stream is in order, so a state advances in submit order; mbx_limit_state_get / _set / _reset on a state
 * with submits in flight are the caller's to order, with mbx_session_wait first.  A NULL state clears the attachment and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL session or limit; what mbx_bus_limit refuses of the limit; a state of another device than the
 * session. */
int mbx_session_next_limit(struct mbx_session* s, const mbx_limit* limit, mbx_limit_state* state);

#ifdef __cplusplus
}
#endif

#endif /* MBX_LIMIT_PUBLIC_H */
