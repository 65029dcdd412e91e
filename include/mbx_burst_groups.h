/*
 * mbx_burst_groups.h -- burst groups of the MI355X batch launcher (libmbx_hip.so): the bursts of SEVERAL schedules decoded in one call.
 *
 * mbx_burst.h takes ONE schedule per call with one burst per stream; the mixed calls of mbx.h take any codec per stream but start
 * at frames.  A receiver that listens to several air interfaces at once has, in one tick, three DMR bursts of one stream beside one
 * P25 LDU of another.  A BURST GROUP is the bursts of ONE schedule in one tick: n_streams streams with bursts_per_stream consecutive
 * bursts each, stream-major, every stream named by a pool slot.  A call takes up to MBX_BURST_MAX_GROUPS groups, all hard or all
 * soft, and decodes them as ONE mixed ragged step with ONE gather launch in front of it that covers all groups.  The caller builds no
 * device array: the gather launch writes the step's frame_offset, stream_codec and stream_index itself.
 * Replaces, for every stream of every group at once, the caller's de-interleave loops and the mbe_process*Frame[f] /
 * mbe_process*FrameSoft calls behind them (ref include/mbelib-neo/mbelib.h:352,429,505,564).
 *
 * Conventions are those of mbx.h and mbx_burst.h: `stream` is a hipStream_t passed as void*, launchers are asynchronous on `stream`,
 * never synchronise, and return 0 or a negative MBE_STATUS_* / MBX_E* code with the reason in mbx_last_error().
 *
 * Rows.  Stream rows and frame rows run group after group; inside a group stream after stream, burst after burst, frame after
 * frame: frame k of burst i of stream j of group g is row
 *     row_of_group[g] + (j * bursts_per_stream + i) * frames_per_burst + k
 * of every output (PCM x 160, results, records: total_frames rows each).  mbx_burst_groups_rows gives row_of_group.
 *
 * Contract.  PCM, results, records, state, RNG state and elision words are BYTE-IDENTICAL to the route over the existing calls:
 * mbx_deinterleave[_soft] per group into mixed rows (MBX_MIXED_ROW_BYTES / MBX_MIXED_ROW_CELLS) at the group's first row, a host-made
 * frame_offset (step bursts_per_stream * frames_per_burst per stream), stream_codec (the schedule's codec) and stream_index, and one
 * mbx_process_batch[_soft]_mixed call with the same d_resident.  mbx_last_kernel_name(stream) reports mixed_stream_kernel_ragged
 * (d_resident: mixed_stream_kernel_ragged_res).  The call is a linear chain on `stream`: no internal streams, no events, no host
 * synchronisation, nothing uploaded; it can be captured into a graph once
 * mbx_reserve_stream(stream, mbx_burst_groups_workspace_frames(groups, n_groups, soft)) has been called.
 * n_groups == 0, or groups that are all empty, return 0 and launch nothing; a group with n_streams == 0 is skipped (its schedule
 * and its counts are still checked, its bursts and stream_index pointers are not looked at, not even their alignment).
 * No slot may be named twice across the groups of a call: two stream rows on one slot would race on its state.  On the device
 * route that is the caller's to keep, as in the mixed calls of mbx.h; the session checks it on the host.
 *
 * Refused before a device is asked for, MBE_STATUS_INVALID_ARGUMENT with the call named in mbx_last_error(): NULL groups (n_groups
 * > 0), a NULL schedule, NULL bursts of a group that has streams; n_groups outside 0 .. MBX_BURST_MAX_GROUPS; bursts_per_stream < 1
 * or a negative n_streams; a hard call with an LLR schedule; a hard burst_stride below mbx_burst_schedule_bytes(); a pointer below
 * its alignment; more than 2^31-1 frames in total.  After the context check: a schedule of another device than the current one.
 *
 * Alignment, in the style of the table in mbx_burst.h (kinds not named here keep their row there or in mbx.h):
 *   kind        bytes  which pointers
 *   bursts      1      bursts of a group in a hard call (fetched as mbx_burst.h says, per group)
 *   softbursts  2 | 1  bursts of a group in a soft call: 2, and 1 with an LLR8 schedule (the softbursts / llr16 / llr8 rows of mbx_burst.h)
 *   index       4      stream_index of a group
 * (groups and row_of_group are host arrays of the C types they are declared as.)
 * Sizes are exact: of group g nothing is read outside n_streams * bursts_per_stream bursts and n_streams index words, nothing is
 * written outside the total_frames rows of each output and the slots the groups name.
 */
#ifndef MBX_BURST_GROUPS_H
#define MBX_BURST_GROUPS_H

#include <stddef.h>
#include <stdint.h>

#include "mbx_burst.h"
#include "mbx_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_BURST_MAX_GROUPS 8

typedef struct mbx_burst_group {
    const mbx_burst_schedule* sched;
    const void*    bursts;            /* hard: burst_stride apart; soft: dense, mbx_burst_schedule_soft_bytes() each (LLRs as a cast) */
    size_t         burst_stride;      /* hard only */
    int            n_streams;         /* >= 0 */
    int            bursts_per_stream; /* >= 1; stream j of the group owns bursts [j*c, (j+1)*c) */
    const int32_t* stream_index;      /* n_streams pool slots; NULL: slots first_slot .. first_slot + n_streams - 1 */
    int            first_slot;
} mbx_burst_group;

/* The device route: `groups` is a HOST array, the bursts and stream_index of every group are DEVICE pointers.  soft != 0: every
 * group brings soft bursts.  d_resident as in mbx_process_batch_mixed (NULL: the ABI triplets are whole after the call);
 * d_pcm16, d_pcmf and d_results may each be NULL. */
int mbx_process_burst_groups(const mbx_burst_group* groups, int n_groups, int soft, mbe_parms* d_state_pool, uint32_t* d_resident,
                             mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                             mbx_param_record* d_records, void* stream);
/* workspace frames (the unit of mbx_reserve_stream / mbx_reserve) the call needs; 0 for groups it would refuse */
size_t mbx_burst_groups_workspace_frames(const mbx_burst_group* groups, int n_groups, int soft);
/* row_of_group[g] = first frame row of group g, row_of_group[n_groups] = total_frames (HOST memory, n_groups + 1 words).  0, or
 * MBE_STATUS_INVALID_ARGUMENT for what the call above refuses of counts and schedules.  No device is needed. */
int mbx_burst_groups_rows(const mbx_burst_group* groups, int n_groups, int32_t* row_of_group);

/* ---- sessions ---- */

/* mbx_session_create (mbx.h) for a session whose streams each have a codec: stream_codec[i] (HOST memory, `streams` bytes of
 * MBX_CODEC_*) is the codec of stream i for the session's life.  State, RNG and elision pools are as in every session (the default
 * state does not depend on the codec: reset, seed, get_state and set_state work unchanged); the slot buffers are sized for mixed rows.
 * A mixed session takes burst groups only: mbx_session_submit* and mbx_session_submit_bursts* return MBE_STATUS_INVALID_ARGUMENT
 * on it, mbx_last_error() saying so. */
int mbx_session_create_mixed(struct mbx_session** out, int streams, const uint8_t* stream_codec, size_t max_frames_per_submit, unsigned outputs);
/* The call above fed from HOST memory, on a mixed session or on a single-codec one (every stream's codec is then the session's):
 * the bursts and stream_index of every group are HOST pointers.  Checked on the host before anything is queued
 * (MBE_STATUS_INVALID_ARGUMENT; state, RNG state and outputs keep their bytes): everything the device route refuses; each group's
 * schedule codec is the codec of every stream the group names; slots are in range and none is named twice across the groups;
 * total frames <= max_frames_per_submit; and mbx_burst_validate per group for the forms that can be invalid
 * (MBE_STATUS_INVALID_BITS).  The bursts take the road bursts take: pinned 16-byte aligned buffers are read in place, others are
 * staged, each group at a 16-byte aligned offset of the slot's burst buffer; the device call follows on the compute stream and the
 * outputs (total_frames rows each) are copied out as for every submit. */
int mbx_session_submit_burst_groups(struct mbx_session* s, const mbx_burst_group* groups, int n_groups, int soft, int16_t* pcm16,
                                    float* pcmf, mbe_process_result* results);

#ifdef __cplusplus
}
#endif

#endif /* MBX_BURST_GROUPS_H */
