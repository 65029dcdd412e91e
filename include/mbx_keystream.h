/*
 * mbx_keystream.h -- keystream input of the MI355X batch launcher (libmbx_hip.so): encrypted channels on the batched paths.
 *
 * A host that serves encrypted traffic (P25 ADP/DES/AES, DMR and NXDN RC4/AES/"basic privacy") uses the reference's split API: it
 * runs mbe_decodeImbe7200x4400Frame / mbe_decodeAmbe3600x2450Frame (FEC: the parameter bits in imbe_d[88] / ambe_d[49], the error
 * context in *result), XORs its cipher's keystream onto imbe_d / ambe_d itself, and calls mbe_processImbe4400Dataf /
 * mbe_processAmbe2450Dataf with the same result (ref include/mbelib-neo/mbelib.h:352,429,505,564; the one-call form is those two
 * calls back to back, ref src/imbe/imbe7200x4400.c:935-948).  Here the caller brings the keystream and the library applies it on the
 * device at that same place, between FEC and parameter decode, on every batched path that has a record stage.  The library owns no
 * cipher and no key schedule, as it owns no interleave table.
 *
 * Conventions are those of mbx.h: `stream` is a hipStream_t passed as void*, launchers are asynchronous on `stream`, never
 * synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error().
 *
 * The keystream row.  One row of MBX_KEYSTREAM_ROW_BYTES bytes per frame, whatever the codec (one row size, as in a mixed batch).
 * Row r belongs to batch row r: stream-major s * T + t in the uniform calls, the row numbering of d_frame_offset in the ragged and
 * mixed ones.  Parameter bit i is XORed with bit 7 - (i & 7) of byte i >> 3 of the row -- the MSB-first order in which the
 * reference's callers consume RC4 / OFB keystream octets --, where parameter bit i is imbe_d[i] / ambe_d[i] as mbx_unpack_records
 * shows it: bit 31 - (i % 32) of w[i / 32] of the frame's mbx_param_record.  nbits is 88 for codecs 0 and 2 and 49 for codecs 1 and
 * 3.  A 7100x4400 row is keyed in the 7200x4400 order in which its record leaves the front end (the order of the bits after
 * mbe_convertImbe7100to7200, which is the order mbe_processImbe4400Dataf reads).  Bits of the row at and beyond nbits are ignored,
 * whatever they hold.  w[3] is never touched: it carries the error counts and flags, the reference's *result context.  An all-zero
 * row leaves its frame clear, so clear and encrypted channels share a batch.  The d_records output of a keyed call holds the bits
 * AFTER the keystream: what was decoded.
 *
 * Launches.  A keyed step is the unkeyed staged step of the same shape with its front launch replaced: the expand launch and the
 * stream-stage instance, ragged, mixed and sliced launches included, are unchanged, and mbx_last_kernel_name(stream) reports that
 * instance.  The one-launch and in-wave forms of a T = 1 step (mbx.h) have no keyed instances: a keyed T = 1 step takes the staged
 * launches, as the unkeyed step does with MBX_FUSE_ONE=0.  Workspace needs are those of the unkeyed staged step of the same shape
 * (mbx_reserve_stream(stream, S * T), or the total of a ragged step plus its order and codec words as in mbx.h).  The keyed calls are
 * not meant for stream capture.
 *
 * Alignment, in the style of the table in mbx.h (kinds not named here keep their row there):
 *   kind        bytes  which pointers
 *   keystream   4      d_keystream of every call below (a row is loaded as three dwords); the host rows of
 *                      mbx_keystream_apply_host and mbx_session_submit_keyed may sit anywhere
 * Sizes are exact: MBX_KEYSTREAM_ROW_BYTES * rows bytes are read, nothing behind them; a row whose frame has no codec (a mixed
 * step's stream_codec byte that names none) is not read.  A pointer below its alignment is refused with
 * MBE_STATUS_INVALID_ARGUMENT before anything is launched.
 */
#ifndef MBX_KEYSTREAM_H
#define MBX_KEYSTREAM_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_KEYSTREAM_ROW_BYTES 12

struct mbx_session;

/* Host only, no device: what the kernels do, for hosts and tests.  records[i].w[0..2] ^= row i, n rows of HOST memory.  Stands in
 * for the caller's own XOR loop over imbe_d / ambe_d between its two reference calls.  MBE_STATUS_INVALID_ARGUMENT: NULL records or
 * keystream, a codec that is none of MBX_CODEC_*. */
int mbx_keystream_apply_host(int codec, mbx_param_record* records, size_t n, const uint8_t* keystream);

/* The stage alone, for the staged callers: between mbx_fec_* / mbx_fec_soft and mbx_process_records (or mbx_expand_records), in
 * place on n device records -- the XOR of the reference's callers between mbe_decode*Frame and mbe_process*Dataf
 * (ref src/imbe/imbe7200x4400.c:935-948).  A 7100x4400 caller passes codec 2 or 0: both are 88 bits. */
int mbx_apply_keystream(int codec, mbx_param_record* d_records, size_t n, const uint8_t* d_keystream, void* stream);

/* S x T, every uniform form in one call: exactly one of d_frames (wire frames, as mbx_process_batch) / d_soft (soft cells, as
 * mbx_process_batch_soft); d_stream_index NULL = identity (else as mbx_process_batch_indexed); d_resident NULL = ABI triplets (else
 * as mbx_process_batch_resident).  d_keystream: S * T rows; NULL: the unkeyed call of the same form, launch for launch, the
 * one-launch forms included.  Stands in for mbe_decode*Frame, the caller's XOR and mbe_process*Dataf per frame
 * (ref include/mbelib-neo/mbelib.h:352,429,505,564).  d_pcm16, d_pcmf and d_results may each be NULL.  Both or neither of d_frames /
 * d_soft: MBE_STATUS_INVALID_ARGUMENT. */
int mbx_process_batch_keyed(int codec, int S, int T, const int32_t* d_stream_index, const uint8_t* d_frames, const mbe_soft_bit* d_soft,
                            const uint8_t* d_keystream, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                            int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream);

/* Ragged (as mbx_process_batch_ragged / _soft_ragged); d_stream_codec non-NULL = mixed (as mbx_process_batch_mixed / _soft_mixed:
 * `codec` is then unused, rows of MBX_MIXED_ROW_BYTES / MBX_MIXED_ROW_CELLS).  d_keystream: total_frames rows, or NULL: the unkeyed
 * call.  A stream whose codec byte names no codec keeps every byte of its state and outputs, and its keystream rows are not read.
 * The same reference calls as above, per frame of every stream. */
int mbx_process_batch_ragged_keyed(int codec, const uint8_t* d_stream_codec, int S, const int32_t* d_frame_offset, size_t total_frames,
                                   const int32_t* d_stream_index, const uint8_t* d_frames, const mbe_soft_bit* d_soft,
                                   const uint8_t* d_keystream, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                                   int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream);

/* Sessions (mbx.h): mbx_session_submit_indexed / _soft_indexed with a keystream.  n x T frames of HOST memory, exactly one of frames
 * / soft; stream_index NULL: n is the session's stream count; keystream: n * T rows of HOST memory, staged like the frames (pinned
 * 16-byte aligned buffers are read in place, others go through the slot's pinned staging), or NULL: the unkeyed submit.  Keyed and
 * unkeyed submits, hard and soft, may alternate on one session.  A session made by mbx_session_create_mixed refuses the call, as
 * it refuses every frames submit.  The same reference calls as above. */
int mbx_session_submit_keyed(struct mbx_session* s, int n, int T, const int32_t* stream_index, const uint8_t* frames, const mbe_soft_bit* soft,
                             const uint8_t* keystream, int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records);

#ifdef __cplusplus
}
#endif

#endif /* MBX_KEYSTREAM_H */
