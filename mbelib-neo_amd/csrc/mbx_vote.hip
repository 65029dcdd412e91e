// mbx_vote.hip -- voted streams (include/mbx_vote.h): several receivers' copies of a frame picked (on records) or combined (on soft
// cells) in ONE launch between the front and the stream stage.  The key, the fields of a vote record, the sum of a cell and the
// refusals are mbx_vote_plan.h, host-only and shared with the host definitions below and with tests/vote_check.cpp.  The whole steps
// (mbx_process_batch_voted, mbx_process_batch_soft_voted) are mbx_api.hip's: they need the stream's workspace and the batch step.
//
// vote_select_kernel.  16 LANES PER VOTED FRAME, 4 frames per 64-lane wave, 16 per workgroup.  Lane j of a frame holds candidates j
// and 16 + j of its group: after the two offsets of the group (one address for the 16 lanes) it requests both records, one 16-byte load
// each, and both present bytes BEFORE anything is reduced -- nothing walks the group, no load waits for another candidate's.  The
// records are loaded whether a candidate is present or not (with nobody present the voted record is candidate 0's), so the present
// bytes are on no address path.  A lane's two keys (kVoteAbsent for a candidate that is not there) are reduced to the smallest of the
// group by the four DPP xor steps of pcm_levels_kernel (quad_perm, quad_perm, row_half_mirror, row_mirror: the 16 lanes of a frame are
// a DPP row); the keys of a group are all different, so the second pass over the keys that are not the smallest gives the runner-up.
// The winner's w[0..2] reach every lane as three OR reductions to which only the winner's lane contributes, each lane compares its
// two records, and the masks of the equal and of the present are two more.  Seven reductions of four DPP steps: no LDS, no
// ds_bpermute, no atomics, no scratch.  The lane that HOLDS the winner stores its 16 bytes; lane 0 stores the 8-byte vote record.
// Frames beyond the last load nothing and store nothing, and still walk the reductions, so that no lane reads a lane that has left.
//
// vote_combine_kernel.  A LANE KEEPS EIGHT CELLS, one 16-byte piece of a voted row (23, 21 or 12 pieces a row): consecutive lanes take
// consecutive pieces, so a wave's loads of one candidate are contiguous runs of its rows.  The lane loops over the candidates of its
// group with the NEXT candidate's piece and present byte requested before this one's cells are summed; eight int32 sums stay in
// registers (|V| <= 8160).  The combined piece leaves as one 16-byte store, and the lane of piece 0 stores the vote record.  The
// kernel moves C * T * row_cells * 2 bytes in and S * T * row_cells * 2 out and does some 40 vector instructions per piece and candidate.
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include <mbx_vote.h>
#include "mbx_vote_plan.h"

namespace mbx {

static_assert(sizeof(mbx_vote_record) == 8 && offsetof(mbx_vote_record, winner) == 0 && offsetof(mbx_vote_record, present) == 1 &&
                  offsetof(mbx_vote_record, best) == 2 && offsetof(mbx_vote_record, second) == 3 && offsetof(mbx_vote_record, agree) == 4,
              "a vote record is winner, present, best, second, agree");
static_assert(sizeof(VoteRecord) == 8 && offsetof(VoteRecord, agree) == 4, "VoteRecord is mbx_vote_record");
static_assert(sizeof(mbe_soft_bit) == 2 && kVotePieceCells * sizeof(mbe_soft_bit) == 16, "a piece is eight cells, 16 bytes");

// 16 bytes as one register quadruple (a clang vector: a select between two of them is four v_cndmask, where HIP's uint4, a struct, is
// chosen by address through scratch)
typedef uint32_t VoteQuad __attribute__((ext_vector_type(4)));

// a value of the lane `lane ^ m` of the 16 lanes of a frame, m = 1, 2, 4, 8 (band_row_xor of mbx_bands.hip)
template <int kXor>
__device__ __forceinline__ uint32_t vote_row_xor(uint32_t v) {
    constexpr int kCtrl = kXor == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : kXor == 2 ? 0x4E /* quad_perm [2,3,0,1] */
                        : kXor == 4 ? 0x141 /* row_half_mirror */ : 0x140 /* row_mirror */;
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t vote_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t vote_row_min(uint32_t v) {   // (lowest bit first: the mirrors need the lanes below them level)
    v = vote_min(v, vote_row_xor<1>(v));
    v = vote_min(v, vote_row_xor<2>(v));
    v = vote_min(v, vote_row_xor<4>(v));
    v = vote_min(v, vote_row_xor<8>(v));
    return v;
}
__device__ __forceinline__ uint32_t vote_row_or(uint32_t v) {
    v |= vote_row_xor<1>(v);
    v |= vote_row_xor<2>(v);
    v |= vote_row_xor<4>(v);
    v |= vote_row_xor<8>(v);
    return v;
}
// a / b where the quotient is a voted frame or a voted stream, below 2^31: in 32 bits wherever a itself fits (the 64-bit division is some
// 120 instructions in front of the first load)
__device__ __forceinline__ uint32_t vote_div(size_t a, uint32_t b) { return (a >> 32) == 0 ? (uint32_t)a / b : (uint32_t)(a / b); }
// the 8 bytes of a vote record as the two dwords they are in memory
__device__ __forceinline__ uint2 vote_record_words(const VoteRecord& v) {
    return uint2{(uint32_t)v.winner | ((uint32_t)v.present << 8) | ((uint32_t)v.best << 16) | ((uint32_t)v.second << 24), v.agree};
}

// offset: the plan's S + 1 offsets; cand: C x T records; present: C x T bytes or nullptr; out: S x T records; votes: S x T vote records or
// nullptr; n = S * T voted frames (cand and out 16-byte aligned, votes 8)
__global__ void __launch_bounds__(kVoteBlock)
vote_select_kernel(const int32_t* __restrict__ offset, int T, const mbx_param_record* __restrict__ cand, const uint8_t* __restrict__ present,
                   mbx_param_record* __restrict__ out, ::mbx_vote_record* __restrict__ votes, size_t n) {
    const int    tid = (int)threadIdx.x;
    const int    j = tid % kVoteLanes;
    const size_t f = (size_t)blockIdx.x * kVoteBlockFrames + (size_t)(tid / kVoteLanes);
    const bool   live = f < n;
    // No load is predicated: a lane beyond its group's last candidate requests the last one again and a frame beyond the last the last
    // frame (n >= 1), so that the four requests of a lane leave back to back with no branch, and no wait, between them.
    const size_t  fl = live ? f : n - 1;
    const uint32_t s = (uint32_t)fl / (uint32_t)T, t = (uint32_t)fl - s * (uint32_t)T;   // (n <= 2^31 - 1)
    const int32_t from = offset[s], size = offset[s + 1] - from;
    const bool    have0 = live && j < size, have1 = live && j + kVoteLanes < size;
    const int     j0 = j < size ? j : size - 1, j1 = j + kVoteLanes < size ? j + kVoteLanes : size - 1;
    const size_t  at0 = (size_t)(from + j0) * (size_t)T + t, at1 = (size_t)(from + j1) * (size_t)T + t;
    // every load of the group is requested here, before the first reduction
    const VoteQuad r0 = reinterpret_cast<const VoteQuad*>(cand)[at0], r1 = reinterpret_cast<const VoteQuad*>(cand)[at1];
    uint32_t       there0 = 1u, there1 = 1u;
    if (present) {   // (uniform)
        there0 = present[at0];
        there1 = present[at1];
    }
    there0 = have0 ? there0 : 0u;
    there1 = have1 ? there1 : 0u;
    const uint32_t k0 = there0 != 0u ? vote_key(r0.w, j) : kVoteAbsent;
    const uint32_t k1 = there1 != 0u ? vote_key(r1.w, j + kVoteLanes) : kVoteAbsent;
    const uint32_t key1 = vote_row_min(vote_min(k0, k1));
    const uint32_t key2 = vote_row_min(vote_min(k0 == key1 ? kVoteAbsent : k0, k1 == key1 ? kVoteAbsent : k1));
    const bool     none = key1 == kVoteAbsent;
    const bool     take0 = none ? j == 0 : k0 == key1;   // (nobody present: candidate 0's record as it stands)
    const bool     take1 = !none && k1 == key1;
    const uint32_t wx = vote_row_or(take0 ? r0.x : (take1 ? r1.x : 0u));
    const uint32_t wy = vote_row_or(take0 ? r0.y : (take1 ? r1.y : 0u));
    const uint32_t wz = vote_row_or(take0 ? r0.z : (take1 ? r1.z : 0u));
    const uint32_t equal = vote_row_or((have0 && r0.x == wx && r0.y == wy && r0.z == wz ? 1u << j : 0u) |
                                       (have1 && r1.x == wx && r1.y == wy && r1.z == wz ? 1u << (j + kVoteLanes) : 0u));
    const uint32_t mask = vote_row_or((there0 != 0u ? 1u << j : 0u) | (there1 != 0u ? 1u << (j + kVoteLanes) : 0u));
    if (live && (take0 || take1)) {
        reinterpret_cast<VoteQuad*>(out)[f] = take0 ? r0 : r1;
    }
    if (live && j == 0 && votes) {
        reinterpret_cast<uint2*>(votes)[f] = vote_record_words(vote_select_record(key1, key2, mask, equal));
    }
}

// what the eight cells of a present candidate's piece add to the eight sums
__device__ __forceinline__ void vote_piece_add(int32_t (&V)[kVotePieceCells], const VoteQuad& w) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        V[2 * i] += vote_cell_value(w[i] & 0xFFu, (w[i] >> 8) & 0xFFu);
        V[2 * i + 1] += vote_cell_value((w[i] >> 16) & 0xFFu, w[i] >> 24);
    }
}
__device__ __forceinline__ VoteQuad vote_piece_out(const int32_t (&V)[kVotePieceCells], const VoteQuad& w) {
    VoteQuad o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[i] = vote_cell_out(V[2 * i], w[i]) | (vote_cell_out(V[2 * i + 1], w[i] >> 16) << 16);
    }
    return o;
}

// offset: the plan's; pieces = row_cells / 8; cand: C x T rows of `pieces` 16-byte pieces; present: C x T bytes or nullptr; out: S x T
// rows; votes: S x T vote records or nullptr; total = S * T * pieces lanes with work
__global__ void __launch_bounds__(kVoteBlock)
vote_combine_kernel(const int32_t* __restrict__ offset, int T, int pieces, const mbe_soft_bit* __restrict__ cand_cells, const uint8_t* __restrict__ present,
                    mbe_soft_bit* __restrict__ out_cells, ::mbx_vote_record* __restrict__ votes, size_t total) {
    const VoteQuad* const cand = reinterpret_cast<const VoteQuad*>(cand_cells);
    const size_t g = (size_t)blockIdx.x * kVoteBlock + threadIdx.x;
    if (g >= total) {
        return;
    }
    const uint32_t f = vote_div(g, (uint32_t)pieces), p = (uint32_t)(g - (size_t)f * (size_t)pieces);
    const uint32_t s = f / (uint32_t)T, t = f - s * (uint32_t)T;
    const int32_t from = offset[s], size = offset[s + 1] - from;
    const size_t  at = (size_t)from * (size_t)T + t;   // the frame of candidate 0; T further on for every next candidate
    VoteQuad      cur = cand[at * (size_t)pieces + p];
    uint32_t      here = present ? present[at] : 1u;
    const VoteQuad zeroth = cur;
    VoteQuad      first = cur;
    uint32_t      mask = 0u;
    int32_t       V[kVotePieceCells] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < size; ++j) {
        // the next candidate's piece is on its way while this one's cells are summed (behind the last candidate the last one again: no
        // predicated load, so the request leaves before the wait for this one's)
        const size_t   ahead = at + (size_t)(j + 1 < size ? j + 1 : j) * (size_t)T;
        const VoteQuad next = cand[ahead * (size_t)pieces + p];
        const uint32_t next_here = present ? present[ahead] : 1u;
        if (here != 0u) {
            first = mask == 0u ? cur : first;
            mask |= 1u << j;
            vote_piece_add(V, cur);
        }
        cur = next;
        here = next_here;
    }
    reinterpret_cast<VoteQuad*>(out_cells)[g] = mask != 0u ? vote_piece_out(V, first) : zeroth;
    if (p == 0 && votes) {
        reinterpret_cast<uint2*>(votes)[f] = vote_record_words(vote_combine_record(mask));
    }
}

// ---- the two launches, for the entry points below and for the voted steps of mbx_api.hip (declared in mbx_host.h) -------------------
// (the caller has made the refusals of vote_select_refused / vote_combine_refused, T > 0, and has the plan's device current)
int vote_select_launch(const mbx_vote_plan* plan, int T, const mbx_param_record* d_cand, const uint8_t* d_present, mbx_param_record* d_records,
                       mbx_vote_record* d_votes, void* stream) {
    const size_t n = (size_t)plan->S * (size_t)T;
    hipLaunchKernelGGL(vote_select_kernel, dim3(vote_select_grid(n)), dim3(kVoteBlock), 0, (hipStream_t)stream, plan->d_offset, T, d_cand, d_present, d_records,
                       d_votes, n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_failed("", "vote_select_kernel", e);
}
int vote_combine_launch(const mbx_vote_plan* plan, int row_cells, int T, const mbe_soft_bit* d_cand, const uint8_t* d_present, mbe_soft_bit* d_soft,
                        mbx_vote_record* d_votes, void* stream) {
    const size_t n = (size_t)plan->S * (size_t)T;
    const int    pieces = row_cells / kVotePieceCells;
    hipLaunchKernelGGL(vote_combine_kernel, dim3(vote_combine_grid(n, row_cells)), dim3(kVoteBlock), 0, (hipStream_t)stream, plan->d_offset, T, pieces,
                       d_cand, d_present, d_soft, d_votes, n * (size_t)pieces);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_failed("", "vote_combine_kernel", e);
}

}  // namespace mbx

namespace {

int refuse(const char* who, mbx::VoteRefusal why) {
    return why == mbx::kVoteAlign ? mbx::misaligned(who, "mbx_vote.h") : mbx::refuse(who, mbx::vote_refusal_text(why));
}

// the offsets as the caller gives them: the pointers, S, the first offset, every group, the stream that broke it by name
int offsets_refused(const char* who, bool have_place, const int32_t* cand_offset, int S, int* largest) {
    int stream = 0;
    const mbx::VoteRefusal why = mbx::vote_offsets_refused(have_place, cand_offset, S, &stream, largest);
    if (why == mbx::kVoteGroup) {
        char text[160];
        mbx::vote_group_text(text, sizeof(text), stream, cand_offset[stream], cand_offset[stream + 1]);
        return mbx::refuse(who, text);
    }
    return why == mbx::kVoteOk ? 0 : refuse(who, why);
}

// the plan of a launch on the current device
int plan_ready(const char* who, const mbx_vote_plan* plan) {
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    return plan->device != dev ? mbx::refuse(who, "a plan of another device than the current one") : 0;
}

}  // namespace

extern "C" {

static_assert(MBX_VOTE_MAX_CANDIDATES == mbx::kVoteMaxCandidates && MBX_VOTE_NONE == mbx::kVoteNone && MBX_VOTE_COMBINED == mbx::kVoteCombined &&
                  MBX_VOTE_SELECT == mbx::kVoteSelect && MBX_VOTE_COMBINE == mbx::kVoteCombine,
              "one set of constants, in the public header and in mbx_vote_plan.h");

int mbx_vote_plan_create(mbx_vote_plan** out, const int32_t* cand_offset, int S) {
    const char* const who = "mbx_vote_plan_create";
    if (out) {
        *out = nullptr;
    }
    int largest = 0;
    int rc = offsets_refused(who, out != nullptr, cand_offset, S, &largest);
    if (rc < 0) {
        return rc;
    }
    int dev = -1;
    rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_vote_plan* p = new (std::nothrow) mbx_vote_plan();
    if (!p) {
        return mbx::refuse(who, "out of memory");
    }
    p->device = dev;
    p->S = S;
    p->C = cand_offset[S];
    p->largest = largest;
    const size_t bytes = ((size_t)S + 1u) * sizeof(int32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_offset), bytes);
    if (e == hipSuccess) {   // (a blocking copy from pageable memory: the caller's array may go when the call returns)
        e = hipMemcpy(p->d_offset, cand_offset, bytes, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {   // (the copy is on the null stream, and the launches that read the plan may be on a non-blocking one)
        e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipFree(p->d_offset);
        delete p;
        return mbx::hip_failed("", "mbx_vote_plan_create: the offsets", e);
    }
    *out = p;
    return 0;
}

int mbx_vote_plan_destroy(mbx_vote_plan* plan) {
    if (plan) {
        (void)hipFree(plan->d_offset);
        (void)hipGetLastError();
        delete plan;
    }
    return 0;
}

int mbx_vote_plan_streams(const mbx_vote_plan* plan) { return plan ? plan->S : MBE_STATUS_INVALID_ARGUMENT; }
int mbx_vote_plan_candidates(const mbx_vote_plan* plan) { return plan ? plan->C : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_vote_select_host(const int32_t* cand_offset, int S, int T, const mbx_param_record* cand_records, const uint8_t* present,
                         mbx_param_record* records, mbx_vote_record* votes) {
    const char* const who = "mbx_vote_select_host";
    if (!cand_records || !records) {
        return refuse(who, mbx::kVotePointers);
    }
    int       largest = 0;
    const int rc = offsets_refused(who, true, cand_offset, S, &largest);
    if (rc < 0) {
        return rc;
    }
    const mbx::VoteRefusal why = mbx::vote_shape_refused(cand_offset[S], T);
    if (why != mbx::kVoteOk) {
        return refuse(who, why);
    }
    for (int s = 0; s < S; ++s) {
        for (int t = 0; t < T; ++t) {
            const size_t at = (size_t)cand_offset[s] * (size_t)T + (size_t)t, to = (size_t)s * (size_t)T + (size_t)t;
            const mbx::VoteRecord v = mbx::vote_select_frame(cand_records + at, present ? present + at : nullptr, (size_t)T, cand_offset[s + 1] - cand_offset[s], records + to);
            if (votes) {
                votes[to] = mbx_vote_record{v.winner, v.present, v.best, v.second, v.agree};
            }
        }
    }
    return 0;
}

int mbx_vote_combine_host(const int32_t* cand_offset, int S, int row_cells, int T, const mbe_soft_bit* cand_soft, const uint8_t* present,
                          mbe_soft_bit* soft, mbx_vote_record* votes) {
    const char* const who = "mbx_vote_combine_host";
    if (!cand_soft || !soft) {
        return refuse(who, mbx::kVotePointers);
    }
    int       largest = 0;
    const int rc = offsets_refused(who, true, cand_offset, S, &largest);
    if (rc < 0) {
        return rc;
    }
    if (!mbx::vote_row_cells_ok(row_cells)) {
        return refuse(who, mbx::kVoteCells);
    }
    const mbx::VoteRefusal why = mbx::vote_shape_refused(cand_offset[S], T);
    if (why != mbx::kVoteOk) {
        return refuse(who, why);
    }
    for (int s = 0; s < S; ++s) {
        for (int t = 0; t < T; ++t) {
            const size_t at = (size_t)cand_offset[s] * (size_t)T + (size_t)t, to = (size_t)s * (size_t)T + (size_t)t;
            const mbx::VoteRecord v = mbx::vote_combine_frame(cand_soft + at * (size_t)row_cells, present ? present + at : nullptr, (size_t)T,
                                                              cand_offset[s + 1] - cand_offset[s], row_cells, soft + to * (size_t)row_cells);
            if (votes) {
                votes[to] = mbx_vote_record{v.winner, v.present, v.best, v.second, v.agree};
            }
        }
    }
    return 0;
}

int mbx_vote_select(const mbx_vote_plan* plan, int T, const mbx_param_record* d_cand_records, const uint8_t* d_present, mbx_param_record* d_records,
                    mbx_vote_record* d_votes, void* stream) {
    const char* const who = "mbx_vote_select";
    const mbx::VoteRefusal why = mbx::vote_select_refused(plan ? plan->S : 0, plan ? plan->C : 0, T, d_cand_records, d_present, d_records, d_votes);
    if (why != mbx::kVoteOk) {
        return refuse(who, why);
    }
    if (T == 0) {
        return 0;
    }
    const int rc = plan_ready(who, plan);
    return rc < 0 ? rc : mbx::vote_select_launch(plan, T, d_cand_records, d_present, d_records, d_votes, stream);
}

int mbx_vote_combine(const mbx_vote_plan* plan, int row_cells, int T, const mbe_soft_bit* d_cand_soft, const uint8_t* d_present, mbe_soft_bit* d_soft,
                     mbx_vote_record* d_votes, void* stream) {
    const char* const who = "mbx_vote_combine";
    const mbx::VoteRefusal why = mbx::vote_combine_refused(plan ? plan->S : 0, plan ? plan->C : 0, row_cells, T, d_cand_soft, d_present, d_soft, d_votes);
    if (why != mbx::kVoteOk) {
        return refuse(who, why);
    }
    if (T == 0) {
        return 0;
    }
    const int rc = plan_ready(who, plan);
    return rc < 0 ? rc : mbx::vote_combine_launch(plan, row_cells, T, d_cand_soft, d_present, d_soft, d_votes, stream);
}

}  // extern "C"
