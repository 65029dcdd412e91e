/*
 * mbx_pcm8.h -- companded PCM out of the MI355X batch launcher (libmbx_hip.so): G.711 mu-law and A-law bytes, converted on the device.
 *
 * Recorders, consoles and RTP gateways store and forward 8 kHz voice as G.711, one byte per sample.  A step delivers int16
 * [rows][160]; a host that wants bytes took 320 B per frame across PCIe and companded them in a per-sample loop of its own.  Here one
 * launch BEHIND the step turns the step's int16 rows into bytes on the device, and a session delivers 160 B per frame.  No step, plan
 * or kernel in front of it changes: the launch reads what the step wrote.
 *
 * Conventions are those of mbx.h: `stream` is a hipStream_t passed as void*, launchers are asynchronous on `stream`, never
 * synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error().
 *
 * The bytes.  mu-law is the classic linear2ulaw on the 14-bit value x >> 2 (magnitude clipped at 8159, bias 33, the code inverted),
 * A-law the classic linear2alaw on the 13-bit value x >> 3 (even bits inverted), both of ITU-T G.711 and bit for bit what CPython's
 * audioop.lin2ulaw / lin2alaw return for 2-byte samples.  mu-law uses 255 of the 256 codes (0x7F is never produced: zero is 0xFF),
 * A-law all 256.  mbelib-neo_amd/pcm8.py holds the same definition in numpy and the two expansion tables.  The library has no
 * expander, no gain, no resampling and no mixing.
 *
 * Alignment, in the style of the table in mbx.h (kinds not named here keep their row there):
 *   kind        bytes  which pointers
 *   pcm8        1      d_pcm8 of mbx_pcm_compand; the host arrays of mbx_pcm_compand_host and the pcm8 of
 *                      mbx_session_next_pcm8 may sit anywhere as well
 * d_pcm16 keeps its row in mbx.h (2).  Sizes are exact: nframes * 160 samples are read and nframes * 160 bytes written, nothing in
 * front of them or behind them.  Where the two addresses allow it -- some sample of the row starts a 16-byte piece of d_pcm16 and
 * an 8-byte piece of d_pcm8 at once, as in every pair of allocations -- a lane moves 16 B in and 8 B out; otherwise the 8-byte
 * stores stay and the samples are loaded one by one.  The at most 7 samples in front of the first piece and behind the last go
 * through as single samples.  Which of the two serves a launch is decided on the host from the two addresses.  The arrays must not
 * overlap.  A pointer below its alignment is refused with MBE_STATUS_INVALID_ARGUMENT before anything is launched.
 */
#ifndef MBX_PCM8_H
#define MBX_PCM8_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_LAW_ULAW 0
#define MBX_LAW_ALAW 1
#define MBX_SESSION_PCM8 8u   /* outputs bit of mbx_session_create[_mixed]: the session can deliver companded bytes */

struct mbx_session;

/* Host only, no device: what the kernel does, for hosts and tests.  nsamples samples of HOST memory -> nsamples bytes.
 * MBE_STATUS_INVALID_ARGUMENT: NULL pcm16 or pcm8, a law that is none of MBX_LAW_*. */
int mbx_pcm_compand_host(int law, const int16_t* pcm16, size_t nsamples, uint8_t* pcm8);

/* One launch behind any step on the same stream: nframes * 160 samples of d_pcm16 -> nframes * 160 bytes of d_pcm8, in the row order
 * of d_pcm16.  A plain launch on the caller's stream: it may be captured.  nframes == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT: a NULL pointer, a law that is none of MBX_LAW_*, an odd d_pcm16 (Alignment). */
int mbx_pcm_compand(int law, const int16_t* d_pcm16, size_t nframes, uint8_t* d_pcm8, void* stream);

/* Sessions (mbx.h) created with MBX_SESSION_PCM8 among their outputs: the NEXT submit of this session, of whatever form -- frames,
 * indexed, soft, soft indexed, keyed, bursts, soft bursts, burst groups --, also delivers its PCM as companded bytes, rows * 160 of
 * them to pcm8 (HOST memory: a pinned buffer is written in place, a pageable one through the slot's pinned staging), in the row
 * order of that submit's pcm16 and valid after mbx_session_wait like every output.  The submit's own pcm16 / pcmf / results are
 * delivered as without it, and its pcm16 may be NULL: the session keeps the int16 rows on the device either way.  The submit uses
 * the attachment up whether it queues or refuses; reset, seed, get_state and set_state leave it.  A NULL pcm8 clears it and returns
 * 0.  MBE_STATUS_INVALID_ARGUMENT: no session, a session made without MBX_SESSION_PCM8, a law that is none of MBX_LAW_*. */
int mbx_session_next_pcm8(struct mbx_session* s, int law, uint8_t* pcm8);

#ifdef __cplusplus
}
#endif

#endif /* MBX_PCM8_H */
