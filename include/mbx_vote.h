/*
 * mbx_vote.h -- voted streams of the MI355X batch launcher (libmbx_hip.so): several receivers' copies of a frame picked or combined
 * on the device, in front of the stream stage.
 *
 * Every other input form of this library has one receiver per decoded stream.  A P25 or DMR talkgroup is heard by several receiver
 * sites at once; a voter decides every 20 ms which site's copy of the frame goes to the vocoder, and receivers with soft demodulators
 * combine the copies bit by bit before the FEC.  A host that decodes every site as a stream of its own and votes on the PCM pays C
 * stream stages where S are needed and votes too late (each site's stream has its own prediction memory and has drifted on its own
 * errors); one that takes the FEC records back every tick and uploads the winners has a synchronous round trip in every tick.  Here
 * the caller brings the GROUPING once -- which candidate rows belong to which voted stream -- and one launch between the front and
 * the stream stage votes.  The library owns two rules, stated below in integers, and no policy beyond them: no weights, no memory of
 * the last winner, no time alignment.
 *
 * Conventions are those of mbx.h: d_ pointers are DEVICE pointers, `stream` is a hipStream_t passed as void*, launchers are
 * asynchronous on `stream`, never synchronise, may be captured, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason
 * in mbx_last_error(); every refusal of an argument comes before a device is asked for.
 *
 * The plan.  cand_offset holds S + 1 ascending int32 offsets, cand_offset[0] = 0 and C = cand_offset[S]: voted stream s owns the
 * candidate rows cand_offset[s] .. cand_offset[s + 1] - 1 of the candidate batch, 1 .. MBX_VOTE_MAX_CANDIDATES of them.  Candidate j
 * of a group is row cand_offset[s] + j; j is the index INSIDE the group that the vote records speak of.
 *
 * Layout.  A candidate batch is C rows of T frames, frame t of candidate row c at c * T + t: the stream-major layout of
 * mbx_process_batch with candidates where the streams are.  d_present is optional: C * T bytes in the same order, non-zero meaning
 * that this site delivered this frame; NULL means that every frame is there.  The voted arrays (records, cells, PCM, results, vote
 * records) are S rows of T, frame t of voted stream s at s * T + t.
 *
 * Select: fewest errors, on records -- so one launch serves hard and soft input.  For voted frame (s, t), over the candidates j of the
 * group that are present, with c0 = w[3] & 0xFF and protected = (w[3] >> 8) & 0xFF exactly as mbx_unpack_records reads them:
 *     key_j    = (c0 + protected) << 16  |  c0 << 8  |  j            (below 2^32; no two candidates share one)
 *     winner   = the j of the smallest key; runner-up = the j of the second smallest
 *     record   = the winner's 16 bytes, unchanged
 *     vote     = { winner, number present, min(255, c0 + protected) of the winner, the same of the runner-up or 0xFF if there is none,
 *                  agree: bit j = candidate j is present and its w[0], w[1], w[2] equal the winner's }
 * A tie on the total is broken by the smaller c0, a tie on both by the lower index.  If NO candidate is present the voted record is
 * candidate 0's as it stands -- what a host with nothing better would feed the reference: the bits of a frame that never came are
 * whatever the receiver left there, and the stream stage decides on their error counts as it does for any frame -- and the vote is
 * { MBX_VOTE_NONE, 0, 0xFF, 0xFF, 0 }.
 *
 * Combine: soft input only, on cells, in front of the soft front.  For cell i of voted frame (s, t), over the present candidates:
 *     v_j      = bit_j ? + reliability_j : - reliability_j          (any non-zero bit byte counts as one)
 *     V        = sum v_j                                            (exact: |V| <= 32 * 255 = 8160)
 *     cell     = { V > 0 ? 1 : V < 0 ? 0 : the bit byte of the lowest-index present candidate,  min(|V|, 255) }
 *     vote     = { MBX_VOTE_COMBINED, number present, 0xFF, 0xFF, agree: bit j = candidate j is present }
 * EVERY cell of the row is combined, the cells no channel bit lands in too.  If no candidate is present the combined row is candidate
 * 0's cells as they stand and the vote is { MBX_VOTE_NONE, 0, 0xFF, 0xFF, 0 }.  The device never validates cells (as for soft frames,
 * mbx.h).
 *
 * Identities:
 *   ONE       a group of one candidate that is present: select returns its record, combine returns its cells byte for byte (cells whose
 *             bit byte is 0 or 1: V = +-reliability, and at reliability 0 the bit byte itself).
 *   SOLE      a group in which one candidate is present equals that candidate, whatever the absent ones hold.
 *   SAME      n present candidates with equal cells {b, r} combine to {b, min(255, n r)}; with equal records, select takes the lowest index
 *             and agree is the mask of the present.
 *   ORDER     combine does not depend on the order of the candidates except through the tie V = 0; select depends on it only through
 *             the index in the key.
 *
 * Alignment, in the style of the table in mbx.h (kinds not named here keep their row there):
 *   kind           bytes  which pointers
 *   cand records   16     d_cand_records and d_records of mbx_vote_select: a record is loaded and stored as one 16-byte piece
 *   cand cells     16     d_cand_soft and d_soft of mbx_vote_combine, d_cand_soft of the voted soft step: a lane loads and stores eight
 *                         cells at once (every row length, 368, 336 or 192 bytes, is a multiple of 16)
 *   present        1      d_present
 *   vote records   8      d_votes: one 8-byte store per voted frame
 *   cand frames    2 | 1  d_cand_frames of the voted hard step: kind `frames` of mbx.h
 * cand_offset of mbx_vote_plan_create and every array of the host definitions are HOST memory and may sit anywhere their element type
 * allows.  Sizes are exact.  No output may overlap an input or another output.
 *
 * Workspace.  A voted step keeps the candidates' records (select) or the combined cells (combine) in the workspace of `stream`,
 * behind the rows of its stream stage.  A caller who captures a voted step into a graph reserves
 * mbx_reserve_stream(stream, mbx_vote_workspace_frames(plan, codec, mode, T)) first: at most S * T rows for the stream stage plus
 * ceil(C * T * 16 / mbx_workspace_bytes(1)) rows (select) or ceil(S * T * row_cells * 2 / mbx_workspace_bytes(1)) rows (combine).
 */
#ifndef MBX_VOTE_PUBLIC_H
#define MBX_VOTE_PUBLIC_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_VOTE_MAX_CANDIDATES 32
#define MBX_VOTE_NONE           0xFF   /* winner: no candidate was present */
#define MBX_VOTE_COMBINED       0xFE   /* winner: the frame is a combination (mbx_vote_combine) */
#define MBX_VOTE_SELECT         0      /* mode of the voted soft step: soft front over C * T frames, then select */
#define MBX_VOTE_COMBINE        1      /* ... combine first, then the soft front over S * T frames */

typedef struct mbx_vote_record {
    uint8_t  winner;   /* index INSIDE the group; MBX_VOTE_NONE (0xFF): no candidate present; MBX_VOTE_COMBINED (0xFE) */
    uint8_t  present;  /* candidates present at this frame */
    uint8_t  best;     /* min(255, c0 + protected) of the winner; 0xFF under NONE / COMBINED */
    uint8_t  second;   /* the same of the runner-up by the same order; 0xFF if fewer than two present, or COMBINED */
    uint32_t agree;    /* select: bit j = candidate j is present and its w[0..2] equal the winner's; combine: bit j = candidate j present */
} mbx_vote_record;

/* opaque, immutable, on the current device; usable from several streams at once.  It lives in device memory and is never written
 * after creation, so a captured launch replays correctly. */
typedef struct mbx_vote_plan mbx_vote_plan;

/* cand_offset: S + 1 int32 in HOST memory; copied before the call returns.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for and in this order: a NULL out or cand_offset; S below 1; cand_offset[0]
 * other than 0; a group of no candidate or of more than MBX_VOTE_MAX_CANDIDATES, or offsets that do not ascend -- the text names the
 * first such stream. */
int mbx_vote_plan_create(mbx_vote_plan** out, const int32_t* cand_offset, int S);
int mbx_vote_plan_destroy(mbx_vote_plan* plan);   /* NULL allowed */
int mbx_vote_plan_streams(const mbx_vote_plan* plan);      /* S; MBE_STATUS_INVALID_ARGUMENT for NULL */
int mbx_vote_plan_candidates(const mbx_vote_plan* plan);   /* C; MBE_STATUS_INVALID_ARGUMENT for NULL */

/* One launch: the C * T candidate records -> S * T voted records and, where d_votes is given, S * T vote records.  d_present and
 * d_votes may be NULL.  T == 0 launches nothing and returns 0.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for and in this order: a NULL plan, d_cand_records or d_records; T below 0;
 * C * T above 2^31 - 1; a pointer below its alignment (Alignment); an output overlapping an input or the other output.
 * Then: a plan made on another device than the current one. */
int mbx_vote_select(const mbx_vote_plan* plan, int T, const mbx_param_record* d_cand_records, const uint8_t* d_present,
                    mbx_param_record* d_records, mbx_vote_record* d_votes, void* stream);

/* One launch: the C * T candidate rows of row_cells cells -> S * T combined rows and, where d_votes is given, S * T vote records.
 * row_cells is 184, 168 or 96 (184 for the mixed row), as mbx_deinterleave_soft takes it.  d_present and d_votes may be NULL.
 * The refusals of mbx_vote_select, with "row_cells is none of the three" between the pointers and T. */
int mbx_vote_combine(const mbx_vote_plan* plan, int row_cells, int T, const mbe_soft_bit* d_cand_soft, const uint8_t* d_present,
                     mbe_soft_bit* d_soft, mbx_vote_record* d_votes, void* stream);

/* Host only, no device: the definition.  cand_offset as mbx_vote_plan_create takes it, every array in HOST memory; present and votes
 * may be NULL.  The refusals of the plan and of the launch that concern them, in this order: NULLs, S, the offsets, (row_cells,) T, the
 * size. */
int mbx_vote_select_host(const int32_t* cand_offset, int S, int T, const mbx_param_record* cand_records, const uint8_t* present,
                         mbx_param_record* records, mbx_vote_record* votes);
int mbx_vote_combine_host(const int32_t* cand_offset, int S, int row_cells, int T, const mbe_soft_bit* cand_soft, const uint8_t* present,
                          mbe_soft_bit* soft, mbx_vote_record* votes);

/* Rows of the stream's workspace a voted step of this shape needs (see Workspace); mode is MBX_VOTE_SELECT for the hard step.
 * 0 for a NULL plan, an unknown codec or mode, or a negative T. */
size_t mbx_vote_workspace_frames(const mbx_vote_plan* plan, int codec, int mode, int T);

/* The voted hard step, a linear chain on `stream` -- no internal streams, no events, no host synchronisation: the codec's front launch
 * over the C * T candidate frames (d_cand_frames: C rows of T wire frames of `codec`) into the stream's workspace, the select launch,
 * then the stream stage exactly as mbx_process_records runs it on the S * T voted records: the expand launch where
 * mbx_uses_expand_launch(codec', S, T) says so (codec': the codec whose stream stage `codec` ends in), and the instance
 * mbx_last_kernel_name reports.  Pool indexing is identity (d_stream_index NULL) or d_stream_index[s] for voted stream s; state is ABI
 * triplets (d_resident NULL) or resident (mbx_process_batch_resident).  d_records receives the S * T voted records; d_pcm16, d_pcmf,
 * d_results and d_votes may be NULL; d_present may be NULL.
 * MBE_STATUS_INVALID_ARGUMENT, before a device is asked for and in this order: a NULL plan, d_cand_frames, d_state_pool, d_rng_pool or
 * d_records; a codec that is none of MBX_CODEC_*; T below 0; C * T above 2^31 - 1; a pointer below its alignment.  Then: a plan of
 * another device; a workspace that would have to grow during stream capture. */
int mbx_process_batch_voted(const mbx_vote_plan* plan, int codec, int T, const int32_t* d_stream_index, const uint8_t* d_cand_frames,
                            const uint8_t* d_present, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                            int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records,
                            mbx_vote_record* d_votes, void* stream);

/* The voted soft step.  MBX_VOTE_SELECT: the soft front over the C * T candidate frames (d_cand_soft: C rows of T frames of the
 * codec's cells), the select launch, the stream stage.  MBX_VOTE_COMBINE: the combine launch into the stream's workspace, the soft
 * front over the S * T combined frames, the stream stage.  Everything else as mbx_process_batch_voted; an unknown mode is refused
 * behind the codec. */
int mbx_process_batch_soft_voted(const mbx_vote_plan* plan, int codec, int mode, int T, const int32_t* d_stream_index,
                                 const mbe_soft_bit* d_cand_soft, const uint8_t* d_present, mbe_parms* d_state_pool, uint32_t* d_resident,
                                 mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                                 mbx_param_record* d_records, mbx_vote_record* d_votes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MBX_VOTE_PUBLIC_H */
