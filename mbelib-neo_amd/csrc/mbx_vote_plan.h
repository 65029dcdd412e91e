// mbx_vote_plan.h -- voted streams (include/mbx_vote.h) in integers alone: what a group is, what mbx_vote_plan_create, mbx_vote_select,
// mbx_vote_combine and the two host definitions refuse and in which order, the key of a candidate, the fields of a vote record and the
// sum of a cell, stated ONCE for the kernels (vote_select_kernel, vote_combine_kernel, mbx_vote.hip), for the host definitions
// (mbx_vote_select_host, mbx_vote_combine_host) and for the CPU program that holds them to a plain second statement
// (tests/vote_check.cpp).  No HIP, no locks, no globals, in the manner of mbx_bands_plan.h.  The pointers of a launch are taken as
// numbers and never dereferenced.  Private to mbx_vote.hip and mbx_api.hip.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "mbx_compand.h"   // (MBX_COMPAND_FN)
#include "mbx_types.h"     // (mbx_param_record, mbe_soft_bit)

struct mbx_vote_plan {   // include/mbx_vote.h: immutable after mbx_vote_plan_create
    int      device = -1;
    int      S = 0, C = 0;
    int      largest = 0;          // candidates of the largest group
    int32_t* d_offset = nullptr;   // S + 1 offsets on the device
};

namespace mbx {

constexpr int     kVoteMaxCandidates = 32;             // MBX_VOTE_MAX_CANDIDATES
constexpr uint8_t kVoteNone = 0xFF, kVoteCombined = 0xFE;   // MBX_VOTE_NONE, MBX_VOTE_COMBINED
constexpr int     kVoteSelect = 0, kVoteCombine = 1;   // MBX_VOTE_SELECT, MBX_VOTE_COMBINE
constexpr size_t  kVoteMaxFrames = (size_t)INT32_MAX;  // C * T of one launch
constexpr uint32_t kVoteAbsent = 0xFFFFFFFFu;          // the key of a candidate that is not there: above every key of one that is
// vote_select_kernel's partition: 16 lanes per voted frame, lane j holds candidates j and 16 + j; 4 frames per wave, 16 per workgroup
constexpr int     kVoteLanes = 16;
constexpr int     kVoteBlock = 256;
constexpr int     kVoteBlockFrames = kVoteBlock / kVoteLanes;
// vote_combine_kernel's: a lane keeps one piece of eight cells (16 bytes) of a voted row
constexpr int     kVotePieceCells = 8;

struct VoteRecord {   // mbx_vote_record, field for field (static_assert in mbx_vote.hip)
    uint8_t  winner, present, best, second;
    uint32_t agree;
};

static inline bool vote_row_cells_ok(int row_cells) { return row_cells == 184 || row_cells == 168 || row_cells == 96; }
static inline bool vote_mode_ok(int mode) { return mode == kVoteSelect || mode == kVoteCombine; }

// ---- refusals, in their order ------------------------------------------------------------------------------------------------------
enum VoteRefusal {
    kVoteOk = 0,
    kVotePointers,   // a NULL: the handle's place, the offsets, the plan, the candidates, the voted array (combine: the vote records are optional too)
    kVoteStreams,    // S below 1
    kVoteFirst,      // cand_offset[0] is not 0
    kVoteGroup,      // a group of no candidate, of more than kVoteMaxCandidates, or offsets that descend (vote_group_text names the stream)
    kVoteCells,      // row_cells is none of 184, 168, 96
    kVoteFrames,     // T below 0
    kVoteSize,       // C * T above 2^31 - 1
    kVoteAlign,      // a pointer below the alignment of its kind
    kVoteOverlap,    // an output overlaps an input or another output
};
static inline const char* vote_refusal_text(VoteRefusal r) {
    switch (r) {
    case kVotePointers: return "a plan (or the offsets and a place for its handle), the candidates and a place for the voted array are needed";
    case kVoteStreams: return "S is at least 1";
    case kVoteFirst: return "cand_offset[0] is 0";
    case kVoteGroup: return "a group has 1 .. MBX_VOTE_MAX_CANDIDATES candidates";
    case kVoteCells: return "row_cells is 184, 168 or 96";
    case kVoteFrames: return "T is not negative";
    case kVoteSize: return "C * T is above 2^31-1";
    case kVoteAlign: return "a pointer is below the alignment of its kind (include/mbx_vote.h, Alignment)";
    case kVoteOverlap: return "an output overlaps the candidates, the present bytes or another output";
    default: return "";
    }
}
// the text of kVoteGroup: "stream 3: 33 candidates (offsets 10 .. 43), a group has 1 .. MBX_VOTE_MAX_CANDIDATES (32)"
static inline void vote_group_text(char* text, size_t room, int stream, int32_t from, int32_t to) {
    snprintf(text, room, "stream %d: %lld candidates (offsets %d .. %d), a group has 1 .. MBX_VOTE_MAX_CANDIDATES (32)", stream,
             (long long)to - (long long)from, (int)from, (int)to);
}

// the offsets as mbx_vote_plan_create and the host definitions are given them; *stream is the first group that is refused, *largest the
// largest group of offsets that pass
static inline VoteRefusal vote_offsets_refused(bool have_place, const int32_t* cand_offset, int S, int* stream, int* largest) {
    if (!have_place || !cand_offset) {
        return kVotePointers;
    }
    if (S < 1) {
        return kVoteStreams;
    }
    if (cand_offset[0] != 0) {
        return kVoteFirst;
    }
    int most = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t n = (int64_t)cand_offset[s + 1] - (int64_t)cand_offset[s];   // (descending offsets: n < 1)
        if (n < 1 || n > kVoteMaxCandidates) {
            *stream = s;
            return kVoteGroup;
        }
        most = (int)n > most ? (int)n : most;
    }
    *largest = most;
    return kVoteOk;
}

static inline bool vote_ranges_overlap(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) {
    return a_bytes != 0 && b_bytes != 0 && a < b + b_bytes && b < a + a_bytes;
}

// T and the size of a launch over C candidate rows (C >= 1: a plan's)
static inline VoteRefusal vote_shape_refused(int C, int T) {
    if (T < 0) {
        return kVoteFrames;
    }
    if ((size_t)T > kVoteMaxFrames / (size_t)C) {
        return kVoteSize;
    }
    return kVoteOk;
}

// mbx_vote_select: S and C are the plan's (0: no plan); every array 16-byte aligned but the present bytes and the 8-byte vote records
static inline VoteRefusal vote_select_refused(int S, int C, int T, const void* d_cand, const void* d_present, const void* d_records, const void* d_votes) {
    if (S == 0 || !d_cand || !d_records) {
        return kVotePointers;
    }
    const VoteRefusal shape = vote_shape_refused(C, T);
    if (shape != kVoteOk) {
        return shape;
    }
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_cand), pr = reinterpret_cast<uintptr_t>(d_present), to = reinterpret_cast<uintptr_t>(d_records),
                    vo = reinterpret_cast<uintptr_t>(d_votes);
    if ((in & 15u) != 0 || (to & 15u) != 0 || (vo & 7u) != 0) {
        return kVoteAlign;
    }
    const uintptr_t ct = (uintptr_t)C * (uintptr_t)T, st = (uintptr_t)S * (uintptr_t)T;
    const uintptr_t pr_bytes = d_present ? ct : 0, vo_bytes = d_votes ? st * 8u : 0;
    if (vote_ranges_overlap(to, st * 16u, in, ct * 16u) || vote_ranges_overlap(to, st * 16u, pr, pr_bytes) || vote_ranges_overlap(vo, vo_bytes, in, ct * 16u) ||
        vote_ranges_overlap(vo, vo_bytes, pr, pr_bytes) || vote_ranges_overlap(vo, vo_bytes, to, st * 16u)) {
        return kVoteOverlap;
    }
    return kVoteOk;
}
// mbx_vote_combine: the same with rows of row_cells cells
static inline VoteRefusal vote_combine_refused(int S, int C, int row_cells, int T, const void* d_cand, const void* d_present, const void* d_soft, const void* d_votes) {
    if (S == 0 || !d_cand || !d_soft) {
        return kVotePointers;
    }
    if (!vote_row_cells_ok(row_cells)) {
        return kVoteCells;
    }
    const VoteRefusal shape = vote_shape_refused(C, T);
    if (shape != kVoteOk) {
        return shape;
    }
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_cand), pr = reinterpret_cast<uintptr_t>(d_present), to = reinterpret_cast<uintptr_t>(d_soft),
                    vo = reinterpret_cast<uintptr_t>(d_votes);
    if ((in & 15u) != 0 || (to & 15u) != 0 || (vo & 7u) != 0) {
        return kVoteAlign;
    }
    const uintptr_t row = (uintptr_t)row_cells * 2u, ct = (uintptr_t)C * (uintptr_t)T, st = (uintptr_t)S * (uintptr_t)T;
    const uintptr_t pr_bytes = d_present ? ct : 0, vo_bytes = d_votes ? st * 8u : 0;
    if (vote_ranges_overlap(to, st * row, in, ct * row) || vote_ranges_overlap(to, st * row, pr, pr_bytes) || vote_ranges_overlap(vo, vo_bytes, in, ct * row) ||
        vote_ranges_overlap(vo, vo_bytes, pr, pr_bytes) || vote_ranges_overlap(vo, vo_bytes, to, st * row)) {
        return kVoteOverlap;
    }
    return kVoteOk;
}

// what a voted step keeps in the stream's workspace behind the rows of its stream stage, in bytes: the candidates' records of a
// select step, the combined cells of a combine step (row_cells: the codec's)
static inline size_t vote_workspace_bytes(int mode, int S, int C, int T, int row_cells) {
    return mode == kVoteCombine ? (size_t)S * (size_t)T * (size_t)row_cells * 2u : (size_t)C * (size_t)T * 16u;
}
static inline uint32_t vote_select_grid(size_t voted_frames) { return (uint32_t)((voted_frames + kVoteBlockFrames - 1) / kVoteBlockFrames); }
static inline uint32_t vote_combine_grid(size_t voted_frames, int row_cells) {
    return (uint32_t)((voted_frames * (size_t)(row_cells / kVotePieceCells) + kVoteBlock - 1) / kVoteBlock);
}

// ---- select: the arithmetic -----------------------------------------------------------------------------------------------------------
// THE key of present candidate j of a group, from w[3] of its record as mbx_unpack_records reads it: c0 = bits 0..7, protected = bits
// 8..15.  At most (510 << 16) | (255 << 8) | 31: below kVoteAbsent, and no two candidates of a group share one.
MBX_COMPAND_FN uint32_t vote_key(uint32_t w3, int j) {
    const uint32_t c0 = w3 & 0xFFu, prot = (w3 >> 8) & 0xFFu;
    return ((c0 + prot) << 16) | (c0 << 8) | (uint32_t)j;
}
// min(255, c0 + protected) of a key; 0xFF of kVoteAbsent
MBX_COMPAND_FN uint8_t vote_errors_of_key(uint32_t key) {
    const uint32_t total = key >> 16;
    return (uint8_t)(key == kVoteAbsent || total > 255u ? 255u : total);
}
MBX_COMPAND_FN bool vote_words_equal(const mbx_param_record& a, const mbx_param_record& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2]; }
// the vote record of a select from the smallest key, the second smallest (kVoteAbsent where there is none), the mask of the present
// candidates and the mask of those whose w[0..2] equal the winner's
MBX_COMPAND_FN VoteRecord vote_select_record(uint32_t key1, uint32_t key2, uint32_t present_mask, uint32_t equal_mask) {
    VoteRecord v;
    v.winner = key1 == kVoteAbsent ? kVoteNone : (uint8_t)(key1 & 0xFFu);
    v.present = (uint8_t)__builtin_popcount(present_mask);
    v.best = vote_errors_of_key(key1);
    v.second = vote_errors_of_key(key2);
    v.agree = key1 == kVoteAbsent ? 0u : (present_mask & equal_mask);
    return v;
}
// THE definition of one voted frame: the n candidates' records cand[j * stride], their present bytes present[j * stride] (nullptr:
// all present) -> the voted record and its vote record
static inline VoteRecord vote_select_frame(const mbx_param_record* cand, const uint8_t* present, size_t stride, int n, mbx_param_record* out) {
    uint32_t key1 = kVoteAbsent, key2 = kVoteAbsent, mask = 0;
    for (int j = 0; j < n; ++j) {
        if (present && present[(size_t)j * stride] == 0) {
            continue;
        }
        mask |= 1u << j;
        const uint32_t key = vote_key(cand[(size_t)j * stride].w[3], j);
        if (key < key1) {
            key2 = key1, key1 = key;
        } else if (key < key2) {
            key2 = key;
        }
    }
    const mbx_param_record& won = cand[key1 == kVoteAbsent ? 0 : (size_t)(key1 & 0xFFu) * stride];
    uint32_t equal = 0;
    for (int j = 0; j < n; ++j) {
        equal |= vote_words_equal(cand[(size_t)j * stride], won) ? 1u << j : 0u;
    }
    *out = won;
    return vote_select_record(key1, key2, mask, equal);
}

// ---- combine: the arithmetic -----------------------------------------------------------------------------------------------------------
// what a present candidate's cell adds to V: + reliability under a hard decision of one (any non-zero bit byte), - reliability under zero
MBX_COMPAND_FN int32_t vote_cell_value(uint32_t bit, uint32_t reliability) { return bit != 0u ? (int32_t)reliability : -(int32_t)reliability; }
// the combined cell as the 16-bit piece { bit, reliability } it is in memory (little endian: bit in the low byte); first_bit is the bit
// byte of the lowest-index present candidate, taken as it came
MBX_COMPAND_FN uint32_t vote_cell_out(int32_t V, uint32_t first_bit) {
    const uint32_t mag = (uint32_t)(V < 0 ? -V : V);
    const uint32_t bit = V > 0 ? 1u : (V < 0 ? 0u : (first_bit & 0xFFu));
    return bit | ((mag > 255u ? 255u : mag) << 8);
}
MBX_COMPAND_FN VoteRecord vote_combine_record(uint32_t present_mask) {
    VoteRecord v;
    v.winner = present_mask == 0u ? kVoteNone : kVoteCombined;
    v.present = (uint8_t)__builtin_popcount(present_mask);
    v.best = v.second = 0xFF;
    v.agree = present_mask;
    return v;
}
// THE definition of one voted row: the n candidates' rows cand[j * stride * row_cells ...] -> row_cells combined cells and the vote record
static inline VoteRecord vote_combine_frame(const mbe_soft_bit* cand, const uint8_t* present, size_t stride, int n, int row_cells, mbe_soft_bit* out) {
    uint32_t mask = 0;
    int      first = -1;
    for (int j = 0; j < n; ++j) {
        if (!present || present[(size_t)j * stride] != 0) {
            mask |= 1u << j;
            first = first < 0 ? j : first;
        }
    }
    for (int i = 0; i < row_cells; ++i) {
        if (first < 0) {   // nobody there: candidate 0's cells as they stand
            out[i] = cand[i];
            continue;
        }
        int32_t V = 0;
        for (int j = 0; j < n; ++j) {
            if (mask & (1u << j)) {
                const mbe_soft_bit& c = cand[(size_t)j * stride * (size_t)row_cells + (size_t)i];
                V += vote_cell_value(c.bit, c.reliability);
            }
        }
        const uint32_t cell = vote_cell_out(V, cand[(size_t)first * stride * (size_t)row_cells + (size_t)i].bit);
        out[i].bit = (uint8_t)(cell & 0xFFu);
        out[i].reliability = (uint8_t)(cell >> 8);
    }
    return vote_combine_record(mask);
}

}  // namespace mbx
