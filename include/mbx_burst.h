/*
 * mbx_burst.h -- burst input of the MI355X batch launcher (libmbx_hip.so): a caller's de-interleave schedule applied on the device.
 *
 * include/mbx.h starts at the packed wire frame.  A host receives air-interface BURSTS: a P25 phase 1 LDU carries 9 IMBE frames of
 * one stream, a DMR voice burst 3 AMBE+2 frames, NXDN 4, D-STAR 1, their channel bits interleaved with each other and with sync
 * words, status symbols and slow data.  The reference leaves that step to its callers (ref include/mbelib-neo/mbelib.h:352,429,505,564:
 * mbe_process*Frame[f] take the filled imbe_fr / ambe_fr arrays), and so did this library: a per-bit loop on the host, per frame.
 * Here the caller brings its schedule ONCE -- which received bit goes to which cell of which frame's array: the tables it already
 * has -- and the library applies it on the device to every burst: "S bursts" is "S streams x T = F frames", stream-major.  No
 * air-interface table of any standard is written down in this library.
 *
 * Conventions are those of mbx.h: d_ pointers are DEVICE pointers, `stream` is a hipStream_t passed as void*, launchers are
 * asynchronous on `stream`, never synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in
 * mbx_last_error().
 *
 * Burst formats.  The FORM of a schedule (MBX_BURST_FORM_*, below) says how a receiver holds its bursts; src_bit always counts
 * received BITS, in every form.
 *   hard   burst_stride bytes per burst, burst b at d_bursts + b * burst_stride; burst_stride >= mbx_burst_schedule_bytes(), any
 *          value; of a burst exactly mbx_burst_schedule_bytes() bytes are read, never the bytes or bits behind bit burst_bits - 1
 *            PACKED  received bit j at byte j >> 3, mask 0x80 >> (j & 7) (MSB first, as everywhere in this library)
 *            BITS    received bit j is bit 0 of byte j
 *            DIBITS  received bits 2d and 2d + 1 are bits 1 and 0 of byte d (the first bit of a symbol is the upper one)
 *   soft   mbx_burst_schedule_soft_bytes() bytes per burst in received order, dense: burst b at byte b * soft_bytes of d_soft
 *            PACKED, BITS  one mbe_soft_bit per received bit
 *            DIBITS        one {dibit, reliability} pair per dibit: field `bit` carries the dibit, both bits take the reliability
 *            LLR16         one signed 16-bit log-likelihood ratio per received bit, what a soft demodulator emits
 *            LLR8          one signed 8-bit LLR per received bit: a reliability of its own for every bit in ONE byte per bit
 *          An LLR v becomes the cell {bit = v > 0, reliability = min(|v|, 255)} inside the gather (|v| taken in int: -32768 gives
 *          255, 0 gives {0, 0}; an int8 LLR is the int16 LLR of the same value) -- the conversion of mbx_soft_bits_from_llr (mbx.h),
 *          ref mbe_softBitFromLlr src/core/mbelib.c:125-158 -- then an inverted bit has its hard decision flipped like any other.
 *          LLR schedules (mbx_burst_schedule_create_llr) are soft-only: the soft calls take their bursts through the d_soft / soft
 *          pointer, as a cast; the hard calls refuse them.  (LLRs that are not bursts: mbx_soft_from_llr, mbx_llr.h.)
 * The device never validates: of a BITS byte `& 1` is used, of a DIBITS byte or dibit cell `& 3`, and a soft hard decision goes
 * on as it came (as for soft frames, mbx.h).  Input on the device is the caller's to check; mbx_burst_validate is the host check,
 * and the session submits call it.
 *
 * Alignment, in the style of the table in mbx.h (kinds not named here keep their row of that table):
 *   kind        bytes  which pointers
 *   bursts      1      d_bursts: with d_bursts and burst_stride both multiples of 4 the bursts are fetched in dwords, otherwise byte by byte
 *   softbursts  2      d_soft of the burst calls: one (bit | dibit, reliability) pair is one 16-bit piece; fetched in dwords from the first 4-aligned pair on
 *   llr16       2      d_soft of the burst calls with an LLR16 schedule: one LLR is one 16-bit piece; fetched like softbursts
 *   llr8        1      d_soft of the burst calls with an LLR8 schedule: fetched in dwords from the first 4-aligned byte on, single bytes at the edges
 *   frames      1      d_frames of mbx_deinterleave, for every codec: dwords where they are whole and aligned, single bytes at the edges
 *   soft        2      d_cells of mbx_deinterleave_soft
 * Sizes are exact: nothing is read behind the last burst's burst_stride bytes (mbx_burst_schedule_bytes() of them are read) or
 * outside the n * soft_bytes bytes of soft bursts, nothing is written outside the rows each call names.  A launcher that is handed
 * a pointer below its alignment returns MBE_STATUS_INVALID_ARGUMENT before anything is launched, the call named in mbx_last_error().
 */
#ifndef MBX_BURST_H
#define MBX_BURST_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_BURST_MAX_FRAMES 18   /* frames of one stream in one burst (a P25 LDU: 9) */
#define MBX_BURST_MAX_BITS   4096 /* received bits of one burst (a P25 LDU: 1,728) */
#define MBX_MIXED_ROW_BYTES  18   /* the row of mbx_process_batch_mixed ... */
#define MBX_MIXED_ROW_CELLS  184  /* ... and of mbx_process_batch_soft_mixed */

struct mbx_session; /* mbx.h */

/* ---- the schedule ---------------------------------------------------------------------------------------------------------- */

/* A de-interleave schedule, immutable once made: any number of host threads and streams may use one at the same time. */
typedef struct mbx_burst_schedule mbx_burst_schedule;

/* Replaces the caller-side loop in front of mbe_processImbe7200x4400Frame[f] / mbe_processAmbe3600x2450Frame[f] /
 * mbe_processImbe7100x4400Frame[f] / mbe_processAmbe2400Dstar... (ref include/mbelib-neo/mbelib.h:429,505,564,352) that fills
 * imbe_fr / ambe_fr from the received bits, for every frame of a burst at once.
 * For frame k of the burst (k < frames_per_burst, in time order) and its i-th channel bit (i < n; n = 144, 72, 142, 72 for codecs
 * 0..3): received bit src_bit[k*n + i] of the burst goes to cell [cell_row[k*n + i]][cell_col[k*n + i]] of that frame's array.
 * The three arrays hold frames_per_burst * n ints each.  Burst bits no entry names (sync, status symbols, slow data) are ignored.
 * Checked on the host before a device is asked for -- MBE_STATUS_INVALID_ARGUMENT, the reason in mbx_last_error():
 *   codec is one of MBX_CODEC_*;  1 <= frames_per_burst <= MBX_BURST_MAX_FRAMES;  frames_per_burst * n <= burst_bits <= MBX_BURST_MAX_BITS;
 *   the cells of each frame are a bijection onto the codec's wire cells (the rule of mbx_wire_permutation);
 *   every src_bit is in [0, burst_bits) and no burst bit is named twice.
 * Then the schedule is folded into the tables the kernels read and uploaded to the calling thread's CURRENT device (which must
 * have been mbx_init()ed: MBX_ENODEVICE / MBX_ENOTINIT otherwise, as for every launcher); a schedule used while another device is
 * current is refused.  Synchronous (one small upload). */
int mbx_burst_schedule_create(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                              const int* cell_row, const int* cell_col);

/* How a receiver holds its bursts.  A 4-level FSK / C4FM demodulator emits one symbol per sample point, so the callers of the
 * reference keep one byte per dibit (or per bit), and one reliability per symbol: those bursts are taken as they are. */
#define MBX_BURST_FORM_PACKED 0 /* 8 received bits per byte, MSB first; soft: one mbe_soft_bit per bit */
#define MBX_BURST_FORM_BITS   1 /* one byte per received bit, the bit in bit 0; soft: one mbe_soft_bit per bit (as PACKED) */
#define MBX_BURST_FORM_DIBITS 2 /* one byte per dibit: received bit 2d = (byte >> 1) & 1, bit 2d + 1 = byte & 1; soft: one
                                   {dibit, reliability} pair per dibit in an mbe_soft_bit-sized cell */
/* mbx_burst_schedule_create with the form of the bursts and a fixed descrambling sequence: invert (HOST memory, burst_bits bytes of
 * 0 / 1, or NULL for none) says which received bits arrive inverted.  A hard bit is flipped; of a soft bit the hard decision is
 * flipped and the reliability kept.  Bits no entry names stay ignored, frame bits that pad the last byte (codec 2) stay 0 and
 * cells that are not on the wire stay {0, 0} whatever the sequence says.  Only a sequence that is a property of the burst POSITION
 * can be stated: one that depends on the data is the caller's.  mbx_burst_schedule_create(...) is this call with
 * MBX_BURST_FORM_PACKED and NULL.  Refused like the rest, before a device is asked for: a form that is none of the three, the
 * dibit form with an odd burst_bits, an invert byte above 1. */
int mbx_burst_schedule_create_form(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                                   const int* cell_row, const int* cell_col, int form, const uint8_t* invert);
/* Soft bursts as LLRs, one per received bit (the format table at the top). */
#define MBX_BURST_FORM_LLR16 16 /* int16_t per received bit */
#define MBX_BURST_FORM_LLR8  8  /* int8_t per received bit */
/* mbx_burst_schedule_create_form for a schedule whose soft bursts are LLRs of llr_bytes bytes each (2: int16, MBX_BURST_FORM_LLR16;
 * 1: int8, MBX_BURST_FORM_LLR8).  The same checks in the same order with the same texts, every one before a device is asked for;
 * in the place of the form check: llr_bytes is neither 1 nor 2.  Any burst_bits will do (nothing is shared between two bits).
 * The schedule is SOFT-ONLY: mbx_deinterleave, mbx_process_bursts and mbx_session_submit_bursts refuse it
 * (MBE_STATUS_INVALID_ARGUMENT, the call named in mbx_last_error(), nothing launched or staged), as does the hard form of
 * mbx_burst_validate.  (mbx_burst_schedule_create_form goes on refusing every form but its three.) */
int mbx_burst_schedule_create_llr(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                                  const int* cell_row, const int* cell_col, int llr_bytes /* 2: int16, 1: int8 */, const uint8_t* invert);
/* frees the device tables (the caller must have no launch in flight that uses the schedule); NULL is allowed */
int mbx_burst_schedule_destroy(mbx_burst_schedule* sched);
int mbx_burst_schedule_codec(const mbx_burst_schedule* sched);            /* MBX_CODEC_*, or MBE_STATUS_INVALID_ARGUMENT for NULL */
int mbx_burst_schedule_frames(const mbx_burst_schedule* sched);           /* frames_per_burst */
int mbx_burst_schedule_bits(const mbx_burst_schedule* sched);             /* burst_bits */
int mbx_burst_schedule_form(const mbx_burst_schedule* sched);             /* MBX_BURST_FORM_*, or MBE_STATUS_INVALID_ARGUMENT for NULL */
/* the smallest burst_stride of this schedule's hard bursts: ceil(burst_bits / 8) (PACKED), burst_bits (BITS), burst_bits / 2 (DIBITS);
 * 0 for an LLR schedule (it has no hard bursts) and for NULL */
size_t mbx_burst_schedule_bytes(const mbx_burst_schedule* sched);
/* mbe_soft_bit-sized cells of one soft burst: burst_bits, or burst_bits / 2 in the dibit form; 0 for NULL.  LLR16: burst_bits (an
 * int16 is the size of a cell).  LLR8: 0 -- an int8 burst need not be a whole number of cells; size buffers with
 * mbx_burst_schedule_soft_bytes(), in every form. */
size_t mbx_burst_schedule_soft_cells(const mbx_burst_schedule* sched);
/* bytes of one soft burst: 2 * soft_cells (PACKED, BITS, DIBITS), burst_bits * llr_bytes (LLR16, LLR8); 0 for NULL */
size_t mbx_burst_schedule_soft_bytes(const mbx_burst_schedule* sched);
/* The host check of n bursts in HOST memory (soft != 0: soft bursts, burst_stride is not looked at): 0, MBE_STATUS_INVALID_ARGUMENT
 * (NULL, a burst_stride below mbx_burst_schedule_bytes()), or MBE_STATUS_INVALID_BITS for a BITS byte above 1, a DIBITS byte or a
 * dibit cell above 3, a hard decision of a per-bit soft cell above 1.  Only the bytes and cells a gather would read are looked at:
 * not the padding of the stride.  Every LLR is valid: soft bursts of an LLR schedule give 0 (bursts != NULL), hard validation of one
 * MBE_STATUS_INVALID_ARGUMENT.  No device is needed. */
int mbx_burst_validate(const mbx_burst_schedule* sched, const void* bursts, size_t burst_stride, size_t n, int soft);

/* ---- the gather alone ------------------------------------------------------------------------------------------------------ */

/* n hard bursts -> n * frames_per_burst packed wire frames, burst after burst: frame k of burst b is row b * frames_per_burst + k,
 * at d_frames + row * frame_stride.  The same bytes as the caller-side scatter into imbe_fr / ambe_fr followed by
 * mbx_pack_imbe7200x4400 / mbx_pack_ambe3600x2450 / mbx_pack_imbe7100x4400 (mbx.h): frame bits that pad the last byte (codec 2) are 0.
 * frame_stride = the codec's frame size (18 | 9), or MBX_MIXED_ROW_BYTES for an AMBE codec: then bytes 0..8 of each row are
 * written and bytes 9..17 keep what they hold -- the rows of mbx_process_batch_mixed.  A host with traffic of several air
 * interfaces calls this once per schedule into disjoint row ranges of one array and then makes ONE mixed launch.
 * One launch; n = 0 launches nothing. */
int mbx_deinterleave(const mbx_burst_schedule* sched, const uint8_t* d_bursts, size_t burst_stride, size_t n, uint8_t* d_frames,
                     size_t frame_stride, void* stream);
/* n soft bursts -> n * frames_per_burst cell arrays in the reference's shapes (mbe_soft_bit [8][23] | [4][24] | [7][24]: what
 * mbe_processImbe7200x4400FrameSoft and its kin take, ref include/mbelib-neo/mbelib.h), row b * frames_per_burst + k at
 * d_cells + row * row_cells cells.  row_cells = the codec's cells (184 | 96 | 168 | 96) or MBX_MIXED_ROW_CELLS (the rows of
 * mbx_process_batch_soft_mixed).  EVERY cell of a row is written: cells that are not on the wire, and the cells of a mixed row
 * behind the codec's array, get {0, 0}. */
/* (an LLR schedule: d_soft is the int16_t / int8_t array, cast) */
int mbx_deinterleave_soft(const mbx_burst_schedule* sched, const mbe_soft_bit* d_soft, size_t n, mbe_soft_bit* d_cells,
                          size_t row_cells, void* stream);

/* ---- burst launches -------------------------------------------------------------------------------------------------------- */

/* The gather, then the batch step of (codec, S streams, T = frames_per_burst) exactly as the frames calls of mbx.h run it: burst
 * row s carries the next frames_per_burst frames of pool slot d_stream_index[s] (NULL: slot s).  With d_resident what
 * mbx_process_batch_resident runs (mbx_process_bursts_soft: mbx_process_batch_soft_resident); with d_resident == NULL the ABI
 * triplets are whole after the launch: what mbx_process_batch_indexed / mbx_process_batch (soft: mbx_process_batch_soft_resident
 * without the words) run.  PCM, results, records, state, RNG state and elision words are byte-identical to those calls on the
 * frames the host would have built, and mbx_last_kernel_name(stream) reports the same stream-stage instance.
 * Replaces, for S streams at once, the caller's de-interleave loop AND the mbe_process*Frame[f] / mbe_process*FrameSoft calls behind
 * it (ref include/mbelib-neo/mbelib.h:352,429,505,564).
 * The gather is ONE launch on `stream` in front of that step and adds no internal stream, event or host synchronisation to it.  The
 * gathered frames live in the stream's workspace behind the step's own rows: mbx_burst_workspace_frames(sched, S, soft) is what
 * mbx_reserve_stream(stream, .) must have been given for the call to allocate nothing.
 * d_pcm16, d_pcmf and d_results may each be NULL (outputs: S * frames_per_burst rows, stream-major); S = 0 returns 0 and launches nothing. */
int mbx_process_bursts(const mbx_burst_schedule* sched, int S, const int32_t* d_stream_index, const uint8_t* d_bursts,
                       size_t burst_stride, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16,
                       float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream);
int mbx_process_bursts_soft(const mbx_burst_schedule* sched, int S, const int32_t* d_stream_index, const mbe_soft_bit* d_soft,
                            mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf,
                            mbe_process_result* d_results, mbx_param_record* d_records, void* stream);
/* workspace frames (the unit of mbx_reserve_stream / mbx_reserve) a burst launch of S bursts needs; 0 for a NULL schedule or S < 0 */
size_t mbx_burst_workspace_frames(const mbx_burst_schedule* sched, int S, int soft);

/* ---- sessions -------------------------------------------------------------------------------------------------------------- */

/* mbx_session_submit[_indexed] / mbx_session_submit_soft[_indexed] (mbx.h) fed with bursts in HOST memory: n bursts, burst i for
 * stream stream_index[i] (NULL: n must be the session's stream count, burst i for stream i), T = frames_per_burst,
 * n * frames_per_burst <= max_frames_per_submit, the schedule's codec the session's (MBE_STATUS_INVALID_ARGUMENT otherwise).  The
 * bursts take the road frames take -- pinned buffers are read in place, pageable ones staged, fetched on the compute stream --
 * then the burst launch above.  Outputs: n * frames_per_burst rows each, as for the frames submits.  Bursts of every form that
 * can be invalid (LLR bursts cannot) are checked with mbx_burst_validate first, as soft frames are (MBE_STATUS_INVALID_BITS, nothing queued: state, RNG
 * state and outputs keep their bytes).  The first burst submit of a session grows the compute stream's workspace once. */
int mbx_session_submit_bursts(struct mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index,
                              const uint8_t* bursts, size_t burst_stride, int16_t* pcm16, float* pcmf, mbe_process_result* results);
int mbx_session_submit_bursts_soft(struct mbx_session* s, const mbx_burst_schedule* sched, int n, const int32_t* stream_index,
                                   const mbe_soft_bit* soft, int16_t* pcm16, float* pcmf, mbe_process_result* results);

#ifdef __cplusplus
}
#endif

#endif /* MBX_BURST_H */
