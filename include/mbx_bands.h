/*
 * mbx_bands.h -- band records out of the MI355X batch launcher (libmbx_hip.so): the int16 rows a step wrote correlated against a
 * caller's bank of probes on the device, K small records per row instead of the row.
 *
 * A level record (mbx_levels.h) says how loud a row is and nothing of where in the band its energy sits.  A host that detects in-band
 * signalling in the decoded audio (DTMF, alert and paging tones, a 1 kHz test tone, a talk-permit beep), that drives a VOX which tells
 * speech from hum, or that draws a coarse spectrum per channel runs a Goertzel or correlator loop over every frame of every row, and so
 * takes every row back, 320 B per frame.  A bank of eight power records is 32 B.  The caller brings the probes, as it brings interleave
 * schedules, FIR taps and biquad coefficients: the library owns no table and ships no designer (mbelib-neo_amd/bands.py has tone()
 * and dtmf()).  Everything is exact in integers.
 *
 * Conventions are those of mbx_levels.h: `stream` is a hipStream_t passed as void*, the launcher is asynchronous on `stream`, never
 * synchronises, may be captured, and returns 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error(); every
 * refusal of an argument comes before a device is asked for.
 *
 * A bank is K probes, 1 <= K <= MBX_BANDS_MAX_PROBES.  A probe is two vectors of 160 int16, c[n] and s[n]; the caller folds its window
 * and its scale into them.  In memory: K x { c[160], s[160] }, 640 bytes a probe.
 *
 * The bound.  A bank is refused unless every vector has sum |v[n]| <= 65535 (MBX_BANDS_VECTOR_BOUND) -- the phase bound of
 * mbx_resample.h, for the same reason: |sum x[n] v[n]| <= 32768 * 65535 = 2,147,450,880 < 2^31, and every partial sum, in any order
 * and over any partition, lies inside that too.  So the sums below are exact in int32, whatever the lanes of a kernel do.
 *
 * Per row x[0 .. 159] and probe k:
 *     re = sum x[n] * c_k[n]        int32, exact
 *     im = sum x[n] * s_k[n]        int32, exact
 *     MBX_BANDS_COMPLEX:  record = { int32 re; int32 im }                                      8 B per probe
 *     MBX_BANDS_POWER:    record = uint32 ((uint64) re * re + (uint64) im * im) >> 31          4 B per probe
 * The power form: re^2 + im^2 <= 2 * 2,147,450,880^2 < 2^63, and shifted right by 31 it is at most 4,294,836,225 < 2^32, so nothing
 * saturates and nothing is clamped.
 *
 * Layout.  Row r owns the K records at out + r * K * record_bytes, in the bank's probe order; nothing in front of them or behind them.
 *
 * The stage is stateless per row, as the levels are: no window spans two frames.  A caller that wants a 40 ms window combines the
 * COMPLEX records of two frames on the host, the second rotated by the probe's phase advance over 160 samples.
 *
 * Identities:
 *   IMPULSE  c_k = 16384 * delta[n - m], s_k = 0 gives re = 16384 * x[m], im = 0.
 *   LEVELS   a probe pair cannot give the energy of a row (sum x^2 is no linear form of x): this is no replacement for mbx_pcm_levels.
 *   ZERO     a probe of zeros gives zeros in both forms.
 *   LINEAR   the COMPLEX records are additive over two rows whose sum does not clip: records(x + y) = records(x) + records(y).
 *
 * Alignment, in the style of the table in mbx_mixdown.h (kinds not named here keep their row there):
 *   kind          bytes  which pointers
 *   band rows     16     d_pcm16 of mbx_pcm_bands: a lane loads 16 bytes (8 samples) of a row at once
 *   band records  16     d_out of mbx_pcm_bands: the records of a row leave as contiguous 8- or 4-byte stores from the row's lanes
 * The host arrays of mbx_band_bank_create and of mbx_pcm_bands_host and the `out` of the session call may sit anywhere their element
 * type allows.  Sizes are exact.  d_out must not overlap d_pcm16.
 */
#ifndef MBX_BANDS_PUBLIC_H
#define MBX_BANDS_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_BANDS_MAX_PROBES   32
#define MBX_BANDS_VECTOR_BOUND 65535   /* the largest sum of |v[n]| a vector of a probe may have */
#define MBX_BANDS_COMPLEX      0       /* { int32 re; int32 im } per probe */
#define MBX_BANDS_POWER        1       /* uint32 (re^2 + im^2) >> 31 per probe */

struct mbx_session;

typedef struct mbx_band_record {   /* MBX_BANDS_COMPLEX */
    int32_t re;
    int32_t im;
} mbx_band_record;

/* opaque, immutable, on the current device; usable from several streams at once.  It lives in device memory and is never written
 * after creation, so a captured launch replays correctly. */
typedef struct mbx_band_bank mbx_band_bank;

/* probes: K x { c[160], s[160] } in HOST memory; copied before the call returns.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for: a NULL out or probes; K outside 1 .. MBX_BANDS_MAX_PROBES; a vector over
 * the bound -- the text names the probe and whether it was c or s. */
int mbx_band_bank_create(mbx_band_bank** out, const int16_t* probes, int K);
int mbx_band_bank_destroy(mbx_band_bank* b);   /* NULL allowed */
int mbx_band_bank_probes(const mbx_band_bank* b);   /* K; MBE_STATUS_INVALID_ARGUMENT for NULL */

/* One launch behind any step on the same stream: the nrows rows of d_pcm16 -> nrows * K records of `form` in d_out.  nrows == 0
 * launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for and in this order: a NULL b, d_pcm16 or d_out; an unknown form;
 * nrows * K * record_bytes above 2^31 - 1; d_pcm16 or d_out below 16-byte alignment (Alignment); d_out overlapping d_pcm16.
 * Then: a bank made on another device than the current one. */
int mbx_pcm_bands(const mbx_band_bank* b, int form, const int16_t* d_pcm16, size_t nrows, void* d_out, void* stream);

/* Host only, no device: the definition.  probes as mbx_band_bank_create takes them, pcm16 nrows rows of 160 samples of HOST memory.
 * The refusals of mbx_band_bank_create and of mbx_pcm_bands that concern it, in this order: NULLs, K, the bound, the form, the size. */
int mbx_pcm_bands_host(const int16_t* probes, int K, int form, const int16_t* pcm16, size_t nrows, void* out);

/* Sessions (mbx.h) created with an output that has int16 rows (MBX_SESSION_PCM16, _PCM8, _MIXDOWN or _LEVELS): the NEXT submit of this
 * session, of whatever form, also delivers the K records of `form` of every row of the submit to out (HOST memory), in the row order
 * of its pcm16, valid after mbx_session_wait.  The records are of the rows as every other int16-derived output sees them: behind an
 * attached filter and AGC.  The submit's pcm16 may be NULL: then only the records cross PCIe.  The slot's device buffer and pinned
 * staging are made by the slot's first submit with a bank, sized by max_frames_per_submit * K * record_bytes, and made anew when a
 * later bank needs more.  The attachment behaves exactly like mbx_session_next_levels: it lasts one submit and is used up whether that
 * queues or refuses; reset, seed, get_state and set_state leave it; a NULL out clears it and returns 0.  The bank must outlive the
 * submit's wait.
 * MBE_STATUS_INVALID_ARGUMENT: no session; no bank; an unknown form; a session made without an output that has int16 rows; a bank of
 * another device than the session. */
int mbx_session_next_bands(struct mbx_session* s, const mbx_band_bank* b, int form, void* out);

#ifdef __cplusplus
}
#endif

#endif /* MBX_BANDS_PUBLIC_H */
