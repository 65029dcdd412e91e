// mbx_hold.hip -- the held gate (include/mbx_hold.h): mbx_mixdown_gated with memory -- hysteresis, hang time and click-free ramps --
// behind mbx_pcm_levels, in two or three launches, with one 4-byte state record per input kept on the device between calls.  The
// arithmetic and the checks are mbx_hold_plan.h, host-only and shared with the host definition below; the plan, its tables, the way
// from its handle to a launch and the prelude of the host definition are those of mbx_mixdown.hip (mbx_mixdown_plan.h); a lane's bus,
// row load, add, long tail and store are mbx_mixdown_lanes.h, shared with mbx_mixdown.hip and mbx_levels.hip; the rank key is
// mbx_levels.h.
//
// Two rules shape the launches.  REPLAY: a captured graph that holds one call must advance the state once per replay, so nothing
// about the state is decided on the host -- the kernels read the record of the last frame and write the record of this one IN PLACE.
// OWNERSHIP: no lane reads a state word that another lane of the same launch writes.  In mixdown_gated_kernel the 20 lanes of a short
// bus each repeat the selection and sit in different waves and workgroups; letting one of them store the state would race with the
// other nineteen.  So every bus has ONE OWNER that reads and writes its records:
//
// hold_decide_kernel (short buses): ONE LANE PER BUS.  It walks the bus twice over the level records and the old state: once to find
//   the N-th largest key (gate_insert / gate_threshold_of, as mixdown_gated_kernel), once to write each input's new record and its CODE
//   byte (off / steady / rising / falling) into the state object's workspace.  A lane reads a record before it writes it and nobody
//   else touches it.  A short bus has at most 22 inputs by default; a plan may make any bus short, and the walk is correct up to 4,096.
// hold_sum_kernel<form> (short buses): the lane map of mixdown_kernel, 20 lanes of 8 samples per bus.  It reads the codes, skips inputs
//   that are off, adds steady ones as mixdown_add_input does, and applies q(n) to rising and falling ones -- only in the pieces the
//   ramp reaches: from sample R - 1 on a rising input is steady and a falling one contributes nothing, and its row is not loaded.
// hold_long_kernel<form> (long buses): ONE WORKGROUP OF 256 PER BUS decides AND sums -- the workgroup is the owner, so the decision
//   needs no launch of its own and the codes no trip through memory.  Lanes stride over the inputs (at most 16 each); with
//   loudest_n = N the N rounds of mixdown_gated_long_kernel name the threshold; every lane then writes the records of its inputs and
//   appends those that are not off to a LIST in LDS (position and code in 16 bits, an LDS counter hands out the places: the sum is
//   over integers, so the order of the list does not matter).  The 12 slices of mixdown_long_kernel then walk the list, not the bus:
//   under "the 3 loudest" a bus of 4,096 sums 3 inputs and the fallers, and ANY number may fall at once (loudest_n made smaller, or
//   a hold with loudest_n > 0 after one with 0), which a fixed "at most 8 rows" pass could not hold.
// So a call is hold_decide_kernel + hold_sum_kernel where the plan has short buses, and hold_long_kernel where it has long ones.
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include "mbx_levels.h"    // the arithmetic: the private header of this directory
#include <mbx_hold.h>      // the public header: include/, first on the include path
#include <mbx_limit.h>     // (mbx_mixdown_held_sums and its host twin are declared there)
#include "mbx_hold_plan.h"
#include "mbx_mixdown_lanes.h"

namespace mbx {

static_assert(sizeof(mbx_gate_input_state) == 4 && offsetof(mbx_gate_input_state, hang_left) == 0 && offsetof(mbx_gate_input_state, open) == 2
                  && offsetof(mbx_gate_input_state, on) == 3,
              "a state record is one little-endian word: hang_left, open, on (hold_state_word)");
static_assert(sizeof(mbx_mixdown_hold) == 8, "the hold is 8 bytes");
static_assert(MBX_HOLD_MAX_RAMP_LOG2 == kHoldMaxRampLog2, "one limit, in the public header and in mbx_hold_plan.h");

// the input `in` at position k of its bus, this frame: its key from its row's record (one 16-byte load) and its old state word, and
// its new record still without `on`
__device__ __forceinline__ uint64_t hold_key_of(const mbx_row_level* __restrict__ levels, const MixdownInput in, int32_t k, uint32_t old,
                                                const HoldParams& hp, uint32_t* next) {
    const uint4 v = *reinterpret_cast<const uint4*>(levels + in.row);
    const HoldDecision d = hold_decide(v.z & 0xFFFFu, hold_word_open(old), hold_word_hang(old), hp.open_peak, hp.close_peak, hp.hang_frames);
    *next = hold_state_word(d.hang, d.open, 0u);
    return hold_key(d, (uint64_t)v.x | ((uint64_t)v.y << 32), k);
}

// one lane per short bus: short_bus[g] is its bus.  state: the records of the plan's inputs, read and written in place; code: a byte per input
__global__ void __launch_bounds__(kHoldDecideBlock)
hold_decide_kernel(const mbx_row_level* __restrict__ levels, const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ short_bus,
                   const MixdownInput* __restrict__ input, int n_short, HoldParams hp, uint32_t* state, uint8_t* __restrict__ code) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)n_short) {
        return;
    }
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, short_bus, g);
    // FOUR inputs at a time, as mixdown_sum has them: four input words and four state words, then four records, in flight together --
    // the lane is alone with its bus, and one dependent load pair after another is all its time.  A short batch is filled up with
    // the batch's first input, whose key is not used and whose record is not written.
    constexpr int kBatch = 4;
    uint64_t top[kGateMaxLoudest] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t i = 0; hp.loudest_n > 0 && i < count; i += kBatch) {
        MixdownInput in[kBatch];
        uint32_t old[kBatch];
        uint64_t key[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int32_t at = lo + (i + j < count ? i + j : i);
            in[j] = input[at];
            old[j] = state[at];
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            uint32_t next;
            key[j] = hold_key_of(levels, in[j], i + j, old[j], hp, &next);
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            gate_insert(top, i + j < count ? key[j] : 0u);
        }
    }
    const uint64_t threshold = gate_threshold_of(top, hp.loudest_n);   // (>= 1: a closed input, key 0, is never on)
    for (int32_t i = 0; i < count; i += kBatch) {
        MixdownInput in[kBatch];
        uint32_t old[kBatch], next[kBatch];
        uint64_t key[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int32_t at = lo + (i + j < count ? i + j : i);
            in[j] = input[at];
            old[j] = state[at];
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            key[j] = hold_key_of(levels, in[j], i + j, old[j], hp, &next[j]);
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {   // (every record of the batch was read above: the stores come last)
            if (i + j < count) {
                const uint32_t on = key[j] >= threshold ? 1u : 0u;
                state[lo + i + j] = next[j] | (on << 24);
                code[lo + i + j] = (uint8_t)hold_code(hold_word_on(old[j]), on);
            }
        }
    }
}

// one input's piece under its code: nothing, the steady add of mbx_mixdown_lanes.h, or the 16 bytes of the row times gain and q(n)
__device__ __forceinline__ void hold_add_input(const int16_t* __restrict__ pcm16, const MixdownInput in, int piece, uint32_t code, int ramp_log2,
                                               int32_t acc[kMixdownPiece]) {
    const int mode = hold_piece_mode(code, piece, ramp_log2);
    if (mode == kHoldPieceSteady) {
        mixdown_add_input(pcm16, in, piece, acc);
    } else if (mode == kHoldPieceRamp) {
        int16_t x[kMixdownPiece];
        mixdown_load_piece(pcm16, in, piece, x);
#pragma unroll
        for (int i = 0; i < kMixdownPiece; ++i) {
            acc[i] += hold_ramped(mixdown_term(x[i], (int16_t)in.gain), hold_weight(code, piece * kMixdownPiece + i, ramp_log2), ramp_log2);
        }
    }
}

// the arguments of mixdown_kernel, the codes hold_decide_kernel wrote and the ramp
template <int kOut>
__global__ void __launch_bounds__(256)
hold_sum_kernel(const int16_t* __restrict__ pcm16, const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ short_bus,
                const MixdownInput* __restrict__ input, int n_short, const uint8_t* __restrict__ code, int ramp_log2, void* __restrict__ out) {
    const auto [slot, piece] = mixdown_short_slot();
    if (slot >= (size_t)n_short) {
        return;
    }
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, short_bus, slot);
    int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
    constexpr int kBatch = 4;   // four codes and four input words in flight together, as mixdown_sum has them
    for (int32_t i = 0; i < count; i += kBatch) {
        MixdownInput in[kBatch];
        uint32_t c[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int32_t k = i + j;
            in[j] = input[lo + (k < count ? k : i)];
            c[j] = k < count ? (uint32_t)code[lo + k] : (uint32_t)kHoldOff;
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            hold_add_input(pcm16, in[j], piece, c[j], ramp_log2, acc);
        }
    }
    mixdown_store<kOut>(out, bus, piece, acc);
}
template __global__ void hold_sum_kernel<kMixdownPcm16>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, const uint8_t*, int, void*);
template __global__ void hold_sum_kernel<kMixdownUlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, const uint8_t*, int, void*);
template __global__ void hold_sum_kernel<kMixdownAlaw>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, const uint8_t*, int, void*);
template __global__ void hold_sum_kernel<kMixdownSums>(const int16_t*, const int32_t*, const int32_t*, const MixdownInput*, int, const uint8_t*, int, void*);

static_assert(kMixdownMaxInputs <= (1 << 12) && kHoldFalling < 4, "a list entry, position | code << 12, fits 16 bits");

// one workgroup per long bus: long_bus[blockIdx.x] is its bus
template <int kOut>
__global__ void __launch_bounds__(256)
hold_long_kernel(const int16_t* __restrict__ pcm16, const mbx_row_level* __restrict__ levels, const int32_t* __restrict__ bus_offset,
                 const int32_t* __restrict__ long_bus, const MixdownInput* __restrict__ input, HoldParams hp, uint32_t* state, void* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) MixdownPart part;
    __shared__ uint64_t wave_max[kGateWaves];
    __shared__ uint16_t list[kMixdownMaxInputs];
    __shared__ int n_list;
    const auto [bus, lo, count] = mixdown_bus_at(bus_offset, long_bus, blockIdx.x);
    const int tid = (int)threadIdx.x;
    if (tid == 0) {
        n_list = 0;
    }
    uint64_t threshold = 1u;   // every open input; a closed one has the key 0
    if (hp.loudest_n > 0) {    // (uniform: the barriers inside are reached by all 256 lanes or by none)
        uint64_t key[kGateKeysPerLane];
#pragma unroll
        for (int j = 0; j < kGateKeysPerLane; ++j) {
            const int32_t k = tid + j * kMixdownBlock;
            uint32_t next;
            key[j] = k < count ? hold_key_of(levels, input[lo + k], k, state[lo + k], hp, &next) : 0u;
        }
        // N rounds, as in mixdown_gated_long_kernel: the largest key below the previous round's winner; the last winner is the threshold
        uint64_t below = ~(uint64_t)0;
        bool more = true;
#pragma unroll
        for (int r = 0; r < kGateMaxLoudest; ++r) {
            if (r < hp.loudest_n && more) {
                uint64_t m = 0;
#pragma unroll
                for (int j = 0; j < kGateKeysPerLane; ++j) {
                    m = (key[j] < below && key[j] > m) ? key[j] : m;
                }
#pragma unroll
                for (int x = 32; x > 0; x >>= 1) {
                    const uint64_t o = (uint64_t)__shfl_xor((uint32_t)m, x, 64) | ((uint64_t)__shfl_xor((uint32_t)(m >> 32), x, 64) << 32);
                    m = o > m ? o : m;
                }
                if ((tid & 63) == 0) {
                    wave_max[tid >> 6] = m;
                }
                __syncthreads();
                m = wave_max[0];
#pragma unroll
                for (int w = 1; w < kGateWaves; ++w) {
                    m = wave_max[w] > m ? wave_max[w] : m;
                }
                __syncthreads();   // (the next round writes wave_max again)
                threshold = m ? m : threshold;
                below = m;
                more = m != 0;
            }
        }
    }
    __syncthreads();   // n_list is 0 for every lane
    // the records of this lane's inputs, read once more and written (no other lane touches them), and the list of those to sum
    // (four at a time, the loads of a batch in flight together and in front of its stores: a bus of 4,096 is ONE workgroup's work, and
    // sixteen dependent load pairs one after another were most of its time)
    constexpr int kPass = 4;
    for (int j0 = 0; j0 < kGateKeysPerLane && tid + j0 * kMixdownBlock < count; j0 += kPass) {
        MixdownInput in[kPass];
        uint32_t old[kPass], next[kPass];
        uint64_t key[kPass];
#pragma unroll
        for (int j = 0; j < kPass; ++j) {
            const int32_t k = tid + (j0 + j) * kMixdownBlock;
            const int32_t at = lo + (k < count ? k : tid + j0 * kMixdownBlock);
            in[j] = input[at];
            old[j] = state[at];
        }
#pragma unroll
        for (int j = 0; j < kPass; ++j) {
            key[j] = hold_key_of(levels, in[j], tid + (j0 + j) * kMixdownBlock, old[j], hp, &next[j]);
        }
#pragma unroll
        for (int j = 0; j < kPass; ++j) {
            const int32_t k = tid + (j0 + j) * kMixdownBlock;
            if (k < count) {
                const uint32_t on = key[j] >= threshold ? 1u : 0u;
                state[lo + k] = next[j] | (on << 24);
                const uint32_t c = hold_code(hold_word_on(old[j]), on);
                if (c != kHoldOff) {
                    list[atomicAdd(&n_list, 1)] = (uint16_t)((uint32_t)k | (c << 12));   // (at most `count` <= 4,096 places are handed out)
                }
            }
        }
    }
    __syncthreads();
    const int32_t n = n_list;
    const int slice = tid / kMixdownPieces, piece = tid - slice * kMixdownPieces;
    if (slice < kMixdownSlices) {
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
        constexpr int kBatch = 4;
        for (int32_t i = slice; i < n; i += kBatch * kMixdownSlices) {
            MixdownInput in[kBatch];
            uint32_t c[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const int32_t at = i + j * kMixdownSlices;
                const uint32_t e = list[at < n ? at : i];
                in[j] = input[lo + (int32_t)(e & 4095u)];
                c[j] = at < n ? e >> 12 : (uint32_t)kHoldOff;
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                hold_add_input(pcm16, in[j], piece, c[j], hp.ramp_log2, acc);
            }
        }
        mixdown_part_put(part, slice, piece, acc);
    }
    __syncthreads();
    if (tid < kMixdownPieces) {
        int32_t acc[kMixdownPiece] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kMixdownSlices; ++j) {
            mixdown_part_add(part, j, tid, acc);
        }
        mixdown_store<kOut>(out, bus, tid, acc);
    }
}
template __global__ void hold_long_kernel<kMixdownPcm16>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, HoldParams, uint32_t*, void*);
template __global__ void hold_long_kernel<kMixdownUlaw>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, HoldParams, uint32_t*, void*);
template __global__ void hold_long_kernel<kMixdownAlaw>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, HoldParams, uint32_t*, void*);
template __global__ void hold_long_kernel<kMixdownSums>(const int16_t*, const mbx_row_level*, const int32_t*, const int32_t*, const MixdownInput*, HoldParams, uint32_t*, void*);

}  // namespace mbx

namespace {

using mbx::refuse;

int refuse(const char* who, mbx::HoldRefusal why, mbx::LevelsRefusal levels = mbx::kLevelsOk, mbx::MixdownRefusal mix = mbx::kMixdownOk) {
    if (why != mbx::kHoldGated) {
        return refuse(who, mbx::hold_refusal_text(why));
    }
    if (levels == mbx::kLevelsAlign || (levels == mbx::kGateMixdown && mix == mbx::kMixdownAlign)) {
        return mbx::misaligned(who, "mbx_levels.h");
    }
    return refuse(who, levels == mbx::kGateMixdown ? mbx::mixdown_refusal_text(mix) : mbx::levels_refusal_text(levels));
}

mbx::HoldParams params_of(const mbx_mixdown_hold& h) {
    return mbx::HoldParams{h.open_peak, h.close_peak, h.hang_frames, (int)h.loudest_n, (int)h.ramp_log2};
}

// what hold_records_refused says of n records a caller gave
mbx::HoldRefusal records_refused(const mbx_gate_input_state* r, int32_t n) {
    std::vector<uint32_t> words((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        words[(size_t)k] = mbx::hold_state_word(r[k].hang_left, r[k].open, r[k].on);
    }
    return mbx::hold_records_refused(words.data(), words.size());
}

// mbx_mixdown_held_host and its sums twin: `out_kind` is the caller's form, or kMixdownSums
int held_host(const char* who, int out_kind, const mbx_mixdown_hold* hold, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
              const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, mbx_gate_input_state* state, void* out) {
    const mbx::HoldRefusal bad_hold = mbx::hold_refused(hold != nullptr, hold ? hold->open_peak : 0u, hold ? hold->close_peak : 0u,
                                                        hold ? hold->loudest_n : 0u, hold ? hold->ramp_log2 : 0u);
    if (bad_hold != mbx::kHoldOk) {
        return refuse(who, bad_hold);
    }
    mbx::MixdownPlan plan;
    if (const char* const why = mbx::mixdown_host_out_refused(out_kind, n_buses, bus_offset, src_row, pcm16, nrows, out, &plan)) {
        return refuse(who, why);
    }
    if (!state && plan.inputs > 0) {
        return refuse(who, mbx::kHoldNoState);
    }
    if (records_refused(state, plan.inputs) != mbx::kHoldOk) {
        return refuse(who, mbx::kHoldRecord);
    }
    const mbx::HoldParams hp = params_of(*hold);
    std::vector<uint64_t> keys;
    std::vector<mbx::HoldDecision> decided;
    for (int b = 0; b < n_buses; ++b) {
        const int32_t lo = bus_offset[b], count = bus_offset[b + 1] - lo;
        keys.resize((size_t)count);
        decided.resize((size_t)count);
        for (int32_t k = 0; k < count; ++k) {   // (the levels of the rows as they are, before the gain)
            const mbx::Level l = mbx::level_of_row(pcm16 + (size_t)src_row[lo + k] * 160u);
            const mbx_gate_input_state& was = state[lo + k];
            decided[(size_t)k] = mbx::hold_decide(l.peak, was.open, was.hang_left, hp.open_peak, hp.close_peak, hp.hang_frames);
            keys[(size_t)k] = mbx::hold_key(decided[(size_t)k], l.energy, k);
        }
        const uint64_t threshold = mbx::gate_threshold(keys.data(), count, hp.loudest_n);
        int32_t acc[160] = {0};
        for (int32_t k = 0; k < count; ++k) {
            const int16_t* const x = pcm16 + (size_t)src_row[lo + k] * 160u;
            const int16_t g = gain_q12 ? gain_q12[lo + k] : (int16_t)mbx::kMixdownUnity;
            const uint32_t on = keys[(size_t)k] >= threshold ? 1u : 0u;
            const uint32_t code = mbx::hold_code(state[lo + k].on, on);
            for (int n = 0; n < 160; ++n) {   // THE definition: every term under its weight, whatever the code
                acc[n] += mbx::hold_ramped(mbx::mixdown_term(x[n], g), mbx::hold_weight(code, n, hp.ramp_log2), hp.ramp_log2);
            }
            state[lo + k] = mbx_gate_input_state{(uint16_t)decided[(size_t)k].hang, (uint8_t)decided[(size_t)k].open, (uint8_t)on};
        }
        mbx::mixdown_put_row(out_kind, acc, b, out);
    }
    return 0;
}

// mbx_mixdown_held and its sums twin, down ONE launch path: `out` is the caller's form (mixdown_out_of_form), or kMixdownSums
int held_launch(const char* who, const mbx_mixdown_plan* plan, const mbx_mixdown_hold* hold, mbx_gate_state* state, int out, const int16_t* d_pcm16,
                size_t nrows, const mbx_row_level* d_levels, void* d_out, void* stream) {
    mbx::LevelsRefusal levels = mbx::kLevelsOk;
    mbx::MixdownRefusal mix = mbx::kMixdownOk;
    const mbx::HoldRefusal why = mbx::held_launch_refused(plan ? &plan->plan : nullptr, plan, hold != nullptr, hold ? hold->open_peak : 0u,
                                                          hold ? hold->close_peak : 0u, hold ? hold->loudest_n : 0u, hold ? hold->ramp_log2 : 0u,
                                                          state != nullptr, state ? state->plan : nullptr, out, d_pcm16, nrows, d_levels, d_out,
                                                          &levels, &mix, out == mbx::kMixdownSums);
    if (why != mbx::kHoldOk) {
        return refuse(who, why, levels, mix);
    }
    mbx::MixdownTables t;
    const int rc = mbx::mixdown_tables(who, plan, &t);
    if (rc < 0) {
        return rc;
    }
    const mbx::MixdownPlan& p = plan->plan;
    const mbx::HoldParams hp = params_of(*hold);
    const hipStream_t strm = (hipStream_t)stream;
    mbx::mixdown_by_out(out, [&](auto k) {
        if (p.short_grid) {
            hipLaunchKernelGGL(mbx::hold_decide_kernel, dim3(mbx::hold_decide_grid(p)), dim3(mbx::kHoldDecideBlock), 0, strm, d_levels, t.bus_offset,
                               t.short_bus, t.input, p.n_short, hp, state->d_state, state->d_code);
            hipLaunchKernelGGL(mbx::hold_sum_kernel<k()>, dim3(p.short_grid), dim3(mbx::kMixdownBlock), 0, strm, d_pcm16, t.bus_offset, t.short_bus,
                               t.input, p.n_short, state->d_code, hp.ramp_log2, d_out);
        }
        if (p.long_grid) {
            hipLaunchKernelGGL(mbx::hold_long_kernel<k()>, dim3(p.long_grid), dim3(mbx::kMixdownBlock), 0, strm, d_pcm16, d_levels, t.bus_offset,
                               t.long_bus, t.input, hp, state->d_state, d_out);
        }
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "hold kernels", e);
}

}  // namespace

extern "C" {

int mbx_gate_state_create(mbx_gate_state** out, const mbx_mixdown_plan* plan) {
    const char* const who = "mbx_gate_state_create";
    if (!out) {
        return refuse(who, "no place for the handle");
    }
    *out = nullptr;
    if (!plan) {
        return refuse(who, "a plan is needed");
    }
    const int rc = mbx::mixdown_tables(who, plan, nullptr);   // (the check alone: the current device ready, and the plan's own)
    if (rc < 0) {
        return rc;
    }
    mbx_gate_state* st = new (std::nothrow) mbx_gate_state();
    if (!st) {
        return refuse(who, "out of memory");
    }
    st->plan = plan;
    st->device = plan->device;
    st->inputs = plan->plan.inputs;
    const size_t bytes = mbx::hold_alloc_bytes(st->inputs);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_state), bytes);
    if (e == hipSuccess) {
        e = hipMemset(st->d_state, 0, bytes);
    }
    if (e != hipSuccess) {
        (void)hipFree(st->d_state);
        delete st;
        return mbx::hip_failed("", "mbx_gate_state_create: the records", e);
    }
    st->d_code = reinterpret_cast<uint8_t*>(st->d_state) + mbx::hold_state_bytes(st->inputs);
    *out = st;
    return 0;
}

int mbx_gate_state_destroy(mbx_gate_state* st) {
    if (st) {
        (void)hipFree(st->d_state);
        (void)hipGetLastError();
        delete st;
    }
    return 0;
}

int mbx_gate_state_inputs(const mbx_gate_state* st) { return st ? st->inputs : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_gate_state_reset(mbx_gate_state* st, void* stream) {
    if (!st) {
        return refuse("mbx_gate_state_reset", "no state");
    }
    if (st->inputs == 0) {
        return 0;
    }
    const hipError_t e = hipMemsetAsync(st->d_state, 0, mbx::hold_state_bytes(st->inputs), (hipStream_t)stream);
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_gate_state_reset: hipMemsetAsync", e);
}

int mbx_gate_state_get(const mbx_gate_state* st, mbx_gate_input_state* host, void* stream) {
    const char* const who = "mbx_gate_state_get";
    if (!st) {
        return refuse(who, "no state");
    }
    if (!host && st->inputs > 0) {
        return refuse(who, "host memory for the records is needed");
    }
    hipError_t e = hipSuccess;
    if (st->inputs > 0) {
        e = hipMemcpyAsync(host, st->d_state, mbx::hold_state_bytes(st->inputs), hipMemcpyDeviceToHost, (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_gate_state_get: copy of the records", e);
}

int mbx_gate_state_set(mbx_gate_state* st, const mbx_gate_input_state* host, void* stream) {
    const char* const who = "mbx_gate_state_set";
    if (!st) {
        return refuse(who, "no state");
    }
    if (!host && st->inputs > 0) {
        return refuse(who, "host memory for the records is needed");
    }
    if (records_refused(host, st->inputs) != mbx::kHoldOk) {
        return refuse(who, mbx::kHoldRecord);
    }
    hipError_t e = hipSuccess;
    if (st->inputs > 0) {
        e = hipMemcpyAsync(st->d_state, host, mbx::hold_state_bytes(st->inputs), hipMemcpyHostToDevice, (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_gate_state_set: copy of the records", e);
}

int mbx_mixdown_held_host(int form, const mbx_mixdown_hold* hold, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                          const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, mbx_gate_input_state* state, void* out) {
    return held_host("mbx_mixdown_held_host", mbx::mixdown_out_of_form(form), hold, n_buses, bus_offset, src_row, gain_q12, pcm16, nrows, state, out);
}

int mbx_mixdown_held_sums_host(const mbx_mixdown_hold* hold, int n_buses, const int32_t* bus_offset, const int32_t* src_row,
                               const int16_t* gain_q12, const int16_t* pcm16, size_t nrows, mbx_gate_input_state* state, int32_t* out) {
    return held_host("mbx_mixdown_held_sums_host", mbx::kMixdownSums, hold, n_buses, bus_offset, src_row, gain_q12, pcm16, nrows, state, out);
}

int mbx_mixdown_held(const mbx_mixdown_plan* plan, const mbx_mixdown_hold* hold, mbx_gate_state* state, int form, const int16_t* d_pcm16,
                     size_t nrows, const mbx_row_level* d_levels, void* d_out, void* stream) {
    return held_launch("mbx_mixdown_held", plan, hold, state, mbx::mixdown_out_of_form(form), d_pcm16, nrows, d_levels, d_out, stream);
}

int mbx_mixdown_held_sums(const mbx_mixdown_plan* plan, const mbx_mixdown_hold* hold, mbx_gate_state* state, const int16_t* d_pcm16,
                          size_t nrows, const mbx_row_level* d_levels, int32_t* d_out, void* stream) {
    return held_launch("mbx_mixdown_held_sums", plan, hold, state, mbx::kMixdownSums, d_pcm16, nrows, d_levels, d_out, stream);
}

}  // extern "C"
