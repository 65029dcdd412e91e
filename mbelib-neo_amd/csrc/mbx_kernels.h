// mbx_kernels.h -- every __global__ kernel of libmbx_hip.so, declared exactly once.
// Included by the translation unit that defines a kernel (mbx_fec.hip, mbx_soft_front.hip, mbx_keystream.hip, mbx_pcm8.hip, mbx_mixdown.hip, mbx_levels.hip, mbx_hold.hip, mbx_agc.hip, mbx_limit.hip, mbx_resample.hip, mbx_filter.hip, mbx_bands.hip, mbx_vote.hip, mbx_expand.hip, mbx_stream.hip, mbx_burst.hip, mbx_api.hip) and by the
// one that launches it (mbx_api.hip; mbx_burst.hip, mbx_pcm8.hip, mbx_mixdown.hip, mbx_levels.hip, mbx_hold.hip, mbx_agc.hip, mbx_limit.hip, mbx_resample.hip, mbx_filter.hip, mbx_bands.hip and mbx_vote.hip launch their own), so a parameter list that drifts from its definition is a compile error (an unmatched
// overload at the launch site or in the instance table), not an unresolved symbol when the library is loaded.
// A new kernel: declare it here, define it, and -- a stream-stage instance -- give it its row in kInstances (mbx_api.hip).
#pragma once
#include "mbx_device.h"

struct mbx_row_level;   // include/mbx_levels.h
struct mbx_vote_record; // include/mbx_vote.h

// The four argument families of the stream-stage instances, written once: the declarations below, the definitions
// (mbx_stream.hip, MBX_*_KERNEL) and the launcher's function pointer types (mbx_api.hip, Instance) all take them from here.
#define MBX_OUT_PARAMS                                                                                                     \
    mbe_parms* __restrict__ state, mbx_stream_rng* __restrict__ rngs, int16_t* __restrict__ pcm16, float* __restrict__ pcmf, \
        mbe_process_result* __restrict__ results, DeviceTables tabs_in
// stream: S streams x Tn frames of records (and their expanded rows, or nullptr)
#define MBX_STREAM_PARAMS int S, int Tn, const mbx_param_record* __restrict__ records, const FrameParams* __restrict__ params, MBX_OUT_PARAMS
// slice: frames t0 .. t0 + n - 1 of the `stride` frames every stream has in the batch arrays
#define MBX_SLICE_PARAMS \
    int S, int stride, int t0, int n, const mbx_param_record* __restrict__ records, const FrameParams* __restrict__ params, MBX_OUT_PARAMS
// fused: one wire frame per stream, the front end in the stream's own wave
#define MBX_FUSED_PARAMS int S, int fec_codec, const uint8_t* __restrict__ frames, mbx_param_record* __restrict__ records, MBX_OUT_PARAMS
// one-launch: front blocks and stream blocks in one grid; after `int S` (the AMBE codecs) or `int S, int lead` (IMBE)
#define MBX_ONE_LAUNCH_PARAMS                                                                                                     \
    const uint8_t* __restrict__ frames, mbx_param_record* __restrict__ records, FrameParams* __restrict__ rows, uint32_t* __restrict__ flags, \
        uint32_t* __restrict__ fallbacks, uint32_t epoch, MBX_OUT_PARAMS
// ragged (a family of its own, outside the instance table): stream row s owns batch rows frame_offset[s] .. frame_offset[s + 1] - 1 of
// the `total` the arrays hold; workgroup b takes row order[b] (nullptr: row b)
#define MBX_RAGGED_PARAMS                                                                                                           \
    int S, int total, const int32_t* __restrict__ frame_offset, const int32_t* __restrict__ order, const mbx_param_record* __restrict__ records, \
        const FrameParams* __restrict__ params, MBX_OUT_PARAMS
// mixed (beside the ragged family): a ragged launch whose stream row s is of codec stream_codec[s]
#define MBX_MIXED_PARAMS const uint8_t* __restrict__ stream_codec, MBX_RAGGED_PARAMS

namespace mbx {

// ---- mbx_stream.hip: the stream-stage instances --------------------------------------------------------------------------------
__global__ void imbe_stream_kernel(MBX_STREAM_PARAMS);
__global__ void ambe_stream_kernel(MBX_STREAM_PARAMS);
__global__ void ambe2400_stream_kernel(MBX_STREAM_PARAMS);
__global__ void imbe_stream_kernel_one(MBX_STREAM_PARAMS);
__global__ void ambe_stream_kernel_one(MBX_STREAM_PARAMS);
__global__ void ambe2400_stream_kernel_one(MBX_STREAM_PARAMS);
__global__ void imbe_stream_kernel_lds(MBX_STREAM_PARAMS);
__global__ void ambe_stream_kernel_lds(MBX_STREAM_PARAMS);
__global__ void ambe2400_stream_kernel_lds(MBX_STREAM_PARAMS);
__global__ void imbe_stream_kernel_res(MBX_STREAM_PARAMS);
__global__ void ambe_stream_kernel_res(MBX_STREAM_PARAMS);
__global__ void ambe2400_stream_kernel_res(MBX_STREAM_PARAMS);
__global__ void imbe_stream_kernel_res1(MBX_STREAM_PARAMS);
__global__ void ambe_stream_kernel_res1(MBX_STREAM_PARAMS);
__global__ void ambe2400_stream_kernel_res1(MBX_STREAM_PARAMS);
__global__ void imbe_stream_kernel_lds_slice(MBX_SLICE_PARAMS);
__global__ void ambe_stream_kernel_lds_slice(MBX_SLICE_PARAMS);
__global__ void ambe2400_stream_kernel_lds_slice(MBX_SLICE_PARAMS);
__global__ void imbe_stream_kernel_one_fused(MBX_FUSED_PARAMS);
__global__ void imbe_stream_kernel_res1_fused(MBX_FUSED_PARAMS);
__global__ void imbe7100_stream_kernel_one_fused(MBX_FUSED_PARAMS);
__global__ void imbe7100_stream_kernel_res1_fused(MBX_FUSED_PARAMS);
__global__ void imbe_one_launch_kernel(int S, int lead, MBX_ONE_LAUNCH_PARAMS);
__global__ void imbe_one_launch_kernel_res(int S, int lead, MBX_ONE_LAUNCH_PARAMS);
__global__ void ambe_one_launch_kernel(int S, MBX_ONE_LAUNCH_PARAMS);
__global__ void ambe_one_launch_kernel_res(int S, MBX_ONE_LAUNCH_PARAMS);
__global__ void ambe2400_one_launch_kernel(int S, MBX_ONE_LAUNCH_PARAMS);
__global__ void ambe2400_one_launch_kernel_res(int S, MBX_ONE_LAUNCH_PARAMS);

// ---- mbx_stream.hip: the ragged stream-stage kernels (mbx_api.hip, kRagged) and the kernel that orders their workgroups ----------------------
__global__ void imbe_stream_kernel_ragged(MBX_RAGGED_PARAMS);
__global__ void ambe_stream_kernel_ragged(MBX_RAGGED_PARAMS);
__global__ void ambe2400_stream_kernel_ragged(MBX_RAGGED_PARAMS);
__global__ void imbe_stream_kernel_ragged_res(MBX_RAGGED_PARAMS);
__global__ void ambe_stream_kernel_ragged_res(MBX_RAGGED_PARAMS);
__global__ void ambe2400_stream_kernel_ragged_res(MBX_RAGGED_PARAMS);
__global__ void ragged_order_kernel(int, const int32_t*, int32_t*);
// ---- the mixed-codec launch set (mbx_process_batch_mixed): row codecs (mbx_stream.hip), front (mbx_fec.hip / mbx_soft_front.hip),
// expansion (mbx_expand.hip), stream stage (mbx_stream.hip; mbx_api.hip, kMixed) ----
__global__ void mixed_row_codec_kernel(int, int, const int32_t*, const uint8_t*, uint8_t*);
__global__ void fec_mixed_kernel(const uint8_t*, size_t, const uint8_t*, mbx_param_record*, DeviceTables);
__global__ void soft_front_mixed_kernel(const mbe_soft_bit*, size_t, const uint8_t*, mbx_param_record*, DeviceTables);
__global__ void expand_mixed_kernel(const mbx_param_record*, size_t, const uint8_t*, FrameParams*, DeviceTables);
__global__ void mixed_stream_kernel_ragged(MBX_MIXED_PARAMS);
__global__ void mixed_stream_kernel_ragged_res(MBX_MIXED_PARAMS);

// ---- mbx_stream.hip: single-frame kernels, frame server, per-stage kernels -------------------------------------------------------
__global__ void imbe_frame_kernel(int, const uint8_t*, mbx_param_record*, mbe_parms*, mbx_stream_rng*, int16_t*, float*, mbe_process_result*, uint32_t*,
                                  uint32_t, DeviceTables, FrameShadow);
__global__ void ambe_frame_kernel(const uint8_t*, mbx_param_record*, mbe_parms*, mbx_stream_rng*, int16_t*, float*, mbe_process_result*, uint32_t*,
                                  uint32_t, DeviceTables, FrameShadow);
__global__ void ambe2400_frame_kernel(const uint8_t*, mbx_param_record*, mbe_parms*, mbx_stream_rng*, int16_t*, float*, mbe_process_result*, uint32_t*,
                                      uint32_t, DeviceTables, FrameShadow);
__global__ void frame_server_kernel(mbx_frame_mailbox*, unsigned, mbe_parms*, mbx_stream_rng*, int16_t*, float*, mbe_process_result*,
                                    mbx_param_record*, DeviceTables, FrameShadow);
__global__ void synth_speech_kernel(int, mbe_parms*, mbe_parms*, mbx_stream_rng*, float*, int16_t*, DeviceTables);
__global__ void tone_kernel(int, const mbx_param_record*, const int32_t*, mbe_parms*, float*, int16_t*, int);
__global__ void enhance_kernel(int, mbe_parms*);
__global__ void smoothing_kernel(int, mbe_parms*, const mbe_parms*);
__global__ void comfort_noise_kernel(int, mbx_stream_rng*, float*, int16_t*);
__global__ void decode_parms_kernel(int, int, const mbx_param_record*, const FrameParams*, mbe_parms*, mbe_parms*, int32_t*, DeviceTables);
__global__ void state_copy_kernel(int, mbe_parms*);

// ---- mbx_fec.hip ---------------------------------------------------------------------------------------------------------------
__global__ void fec_imbe7200x4400_kernel(const uint8_t*, size_t, mbx_param_record*, DeviceTables);
__global__ void fec_ambe3600x2450_kernel(const uint8_t*, size_t, mbx_param_record*, DeviceTables);
__global__ void fec_imbe7100x4400_kernel(const uint8_t*, size_t, mbx_param_record*, DeviceTables);
__global__ void stage_in_kernel(const uint8_t*, uint8_t*, size_t);
__global__ void floattoshort_kernel(const float*, int16_t*, size_t);
constexpr int kLlrChunk = 2048;   // LLRs a workgroup of soft_from_llr_kernel converts at a time
template <int kLlrBytes>
__global__ void soft_from_llr_kernel(const uint8_t*, size_t, mbe_soft_bit*);
__global__ void result_histogram_kernel(const mbe_process_result*, size_t, unsigned long long*);
__global__ void fec_stage_kernel(int, int, const uint8_t*, size_t, uint8_t*, mbx_param_record*, DeviceTables);
__global__ void pack_cells_kernel(int, const char*, size_t, uint8_t*, int32_t*);
__global__ void ecc_words_kernel(int, const uint32_t*, size_t, uint32_t*, int32_t*, DeviceTables);
__global__ void fec_imbe7200x4400_soft_kernel(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);
__global__ void fec_ambe3600x2450_soft_kernel(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);
__global__ void fec_imbe7100x4400_soft_kernel(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);
__global__ void ecc_soft_words_kernel(int, const mbe_soft_bit*, size_t, uint32_t*, int32_t*, DeviceTables);

// ---- mbx_soft_front.hip: the front of a soft batch step, soft frames -> records, one wave per frame ---------------------------------
__global__ void soft_front_imbe_kernel(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);
__global__ void soft_front_imbe7100_kernel(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);
__global__ void soft_front_ambe_kernel(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);

// ---- mbx_keystream.hip: keystream input (include/mbx_keystream.h) -- the stage alone on records, and the hard and the soft front of a
// keyed step (frame stride, uniform codec or row codecs, keystream rows) ---------------------------------------------------------------
__global__ void keystream_apply_kernel(int, mbx_param_record*, size_t, const uint8_t*);
__global__ void fec_keyed_kernel(const uint8_t*, size_t, int, int, const uint8_t*, const uint8_t*, mbx_param_record*, DeviceTables);
__global__ void soft_front_keyed_kernel(const mbe_soft_bit*, size_t, int, int, const uint8_t*, const uint8_t*, mbx_param_record*, DeviceTables);

// ---- mbx_pcm8.hip: companded PCM out (include/mbx_pcm8.h) -- behind a step, its int16 rows -> G.711 bytes; a law (mbx_compand.h) and
// whether the pieces are 16-byte aligned in the input: samples, bytes, their count, whole pieces, samples in front and behind --------------
template <int kLaw, bool kAligned>
__global__ void pcm_compand_kernel(const int16_t*, uint8_t*, size_t, size_t, int, int);

// ---- mbx_mixdown.hip: mix-down out (include/mbx_mixdown.h) -- behind a step, its int16 rows -> talkgroup buses in one of three output
// forms (mbx_mixdown.h): the rows, bus_offset, the buses of the slots (short form: and their count) or of the workgroups (long form),
// the inputs (mbx_mixdown_plan.h), the bus rows.  What a lane of these and of the next two units' bus kernels does -- its bus, one
// input's piece, the walk, the tail of a long bus, the store -- is mbx_mixdown_lanes.h -----------------------------------------------
struct MixdownInput;
template <int kOut>
__global__ void mixdown_kernel(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, void*);
template <int kOut>
__global__ void mixdown_long_kernel(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, void*);

// ---- mbx_levels.hip: levels out and the gated mix-down (include/mbx_levels.h) -- behind a step, its int16 rows -> one level record per
// row (rows, their count, records); and the two mix-down kernels under a gate: their arguments with the records of the rows behind
// the rows and the gate (open_peak, loudest_n) in front of the bus rows (the lanes' pieces: mbx_mixdown_lanes.h) -------------------------
__global__ void pcm_levels_kernel(const int16_t*, size_t, ::mbx_row_level*);
template <int kOut>
__global__ void mixdown_gated_kernel(const int16_t*, const ::mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, int, uint32_t, int, void*);
template <int kOut>
__global__ void mixdown_gated_long_kernel(const int16_t*, const ::mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, uint32_t, int, void*);

// ---- mbx_hold.hip: the held gate (include/mbx_hold.h) -- the gated mix-down with a state record per input: one lane per short bus
// decides (records, the plan's tables, the hold, the state in place, a code byte per input), the short sum reads the codes, and one
// workgroup per long bus decides and sums (the hold: mbx_hold_plan.h; the lanes' pieces: mbx_mixdown_lanes.h) -------------------------
struct HoldParams;
__global__ void hold_decide_kernel(const ::mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, int, HoldParams, uint32_t*, uint8_t*);
template <int kOut>
__global__ void hold_sum_kernel(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, const uint8_t*, int, void*);
template <int kOut>
__global__ void hold_long_kernel(const int16_t*, const ::mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, HoldParams, uint32_t*, void*);

// ---- mbx_agc.hip: levelled rows (include/mbx_agc.h) -- behind a step and in front of every other output launch, its int16 rows under a
// per-stream gain: the parameters (mbx_agc_plan.h), the state in place and its size, the record of every entry (or nullptr), entries,
// frames per entry, rows in, rows out (which may be the rows in) ---------------------------------------------------------------------
struct AgcParams;
__global__ void pcm_agc_kernel(AgcParams, uint32_t*, int, const int32_t*, int, int, const int16_t*, int16_t*);

// ---- mbx_limit.hip: limited buses (include/mbx_limit.h) -- behind the sums instances of the bus kernels above (kOut = kMixdownSums,
// mbx_mixdown.h: acc itself as int32), a look-ahead peak limiter per bus in one of the three output forms: the parameters
// (mbx_limit_plan.h), the state in place, buses, frames per bus, sums in, rows out ------------------------------------------------------
struct LimitParams;
template <int kOut>
__global__ void bus_limit_kernel(LimitParams, uint32_t*, int, int, const int32_t*, void*);

// ---- mbx_resample.hip: wide rows (include/mbx_resample.h) -- behind a step or a bus launch, int16 rows upsampled by L through a
// polyphase FIR interpolator: the packed taps by value (mbx_resample_plan.h), the state in place and its size, the record of every
// entry (or nullptr), rows, frames per entry, rows in, rows out (160 L samples each) ----------------------------------------------------
struct ResampleTaps;
template <int L>
__global__ void pcm_resample_kernel(ResampleTaps, uint32_t*, int, const int32_t*, uint32_t, uint32_t, const int16_t*, int16_t*);

// ---- mbx_filter.hip: filtered rows (include/mbx_filter.h) -- behind a step and in front of the AGC, its int16 rows through a cascade
// of S second-order sections per stream: the coefficients by value (mbx_filter_plan.h), the state in place and its size, the record of
// every entry (or nullptr), entries, frames per entry, rows in, rows out (which may be the rows in) --------------------------------------
struct FilterParams;
template <int S>
__global__ void pcm_filter_kernel(FilterParams, uint32_t*, int, const int32_t*, int, int, const int16_t*, int16_t*);

// ---- mbx_bands.hip: band records (include/mbx_bands.h) -- behind a step, its int16 rows against a bank of K probes: the bank on the
// device (K x 160 dwords), K, rows in, their number, K records per row out, of the form kForm (mbx_bands_plan.h) -------------------------
template <int kForm>
__global__ void pcm_bands_kernel(const uint32_t*, int, const int16_t*, size_t, void*);

// ---- mbx_vote.hip: voted streams (include/mbx_vote.h) -- between the front and the stream stage, the candidates of every voted frame
// picked on their records or combined on their cells: the plan's offsets, T, (pieces of a row,) the C x T candidates, their present
// bytes or nullptr, the S x T voted array, the vote records or nullptr, the voted frames (combine: the pieces) of the launch -------------
__global__ void vote_select_kernel(const int32_t*, int, const mbx_param_record*, const uint8_t*, mbx_param_record*, ::mbx_vote_record*, size_t);
__global__ void vote_combine_kernel(const int32_t*, int, int, const mbe_soft_bit*, const uint8_t*, mbe_soft_bit*, ::mbx_vote_record*, size_t);

// ---- mbx_expand.hip ------------------------------------------------------------------------------------------------------------
__global__ void expand_imbe_kernel(const mbx_param_record*, size_t, FrameParams*, DeviceTables);
__global__ void expand_ambe_kernel(const mbx_param_record*, size_t, FrameParams*, DeviceTables);
__global__ void expand_ambe2400_kernel(const mbx_param_record*, size_t, FrameParams*, DeviceTables);

// ---- mbx_burst.hip: burst input, in front of a batch step -- received bursts -> wire frames / cell arrays by a caller's schedule -----------
// (one template per kind over the forms of mbx_burst_schedule_create_form / _create_llr: packed bits, bit bytes, dibit bytes; per-bit
// cells, dibit pairs, int16 and int8 LLRs; with or without an inversion sequence)
template <int kForm, bool kInvert>
__global__ void burst_gather_kernel(const uint8_t*, size_t, size_t, int, int, int, const uint16_t*, const uint8_t*, uint8_t*, int, int);
enum SoftCell { kCellBit, kCellDibit, kCellLlr16, kCellLlr8 };   // what a staged cell of a soft burst is
template <SoftCell kCell, bool kFlip>
__global__ void burst_gather_soft_kernel(const mbe_soft_bit*, size_t, int, int, int, const uint16_t*, mbe_soft_bit*, int, int);
// Burst groups (include/mbx_burst_groups.h): ONE gather launch over the bursts of up to eight schedules, its grid the concatenation
// of the groups' workgroups.  The descriptors travel BY VALUE in the kernel arguments -- every field a scalar load, nothing uploaded
// per call, the launch capturable.  The same launch writes the layout words of the mixed step behind it.
enum HardGather { kHardPacked, kHardPackedInvert, kHardBits, kHardDibits };              // the instances burst_gather launches, hard ...
enum SoftGather { kSoftBit, kSoftBitFlip, kSoftDibit, kSoftLlr16, kSoftLlr8 };           // ... and soft
struct GatherGroup {
    const void*     in;          // the group's bursts ...
    size_t          stride;      // ... hard: this many bytes apart; soft: dense
    const uint16_t* tab;         // wire table (hard) | cell table (soft)
    const uint8_t*  xor_tab;     // hard: the inversion sequence per output byte
    const int32_t*  index;       // pool slot of each stream of the group, or nullptr: first_slot + j
    uint32_t        n;           // bursts
    int             F, B;        // frames per burst, burst bits
    int             unit;        // frame bytes (hard) | cells (soft) of the codec
    int             staged;      // soft: staged cells of one burst
    int             per;         // hard: lstride; soft: bursts per workgroup
    int             instance;    // HardGather | SoftGather: form and inversion
    uint32_t        first_wg;    // of the grid
    int             first_row;   // frame row of the step
    int             first_stream;   // stream row of the step
    int             bursts_per_stream, codec, first_slot;
};
struct GatherGroups {
    GatherGroup g[8];            // (MBX_BURST_MAX_GROUPS) the groups that have a workgroup, in grid order
    int         count;
    int         S, total;        // stream rows and frame rows of the step
    int32_t*    frame_offset;    // [S + 1] ...
    int32_t*    stream_index;    // [S] ...
    uint8_t*    stream_codec;    // [S]: the layout words, in the workspace
};
__global__ void burst_gather_groups_kernel(GatherGroups, uint8_t*);
__global__ void burst_gather_soft_groups_kernel(GatherGroups, mbe_soft_bit*);

// ---- mbx_api.hip ---------------------------------------------------------------------------------------------------------------
// (C linkage: defined inside the extern "C" block of the entry points, so the profiler prints the bare name)
extern "C" __global__ void resident_materialize_kernel(int, const int32_t*, mbe_parms*, uint32_t*);

}  // namespace mbx
