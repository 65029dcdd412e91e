// vote_check.cpp -- host check of voted streams (include/mbx_vote.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_vote_host.py; a program of its own, nothing of it is loaded anywhere else.
//   the select arithmetic the kernel and the host function share (mbelib-neo_amd/csrc/mbx_vote_plan.h) held to a second, plain statement
//     (sort the present candidates by total, c0, index): every group size 1 .. 32, strides 1 and 3, present bytes given or not, ties of
//     every kind -- and the kernel's partition walked as a wave walks it: 16 lanes with two keys each, four xor steps of min and of or;
//   the combine arithmetic held to a plain statement cell by cell, and the kernel's walk: pieces of eight cells as four dwords, the next
//     candidate behind the present one, the bit bytes of the first present candidate kept; 32 x {1, 255} saturating, {1, 0} alone;
//   every refusal of mbx_vote_plan_create, mbx_vote_select, mbx_vote_combine in its order: pointers as numbers, never dereferenced;
//   the byte counts of the workspace and the grids.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mbx_vote_plan.h"

#include <mbx_vote.h>

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            if (++failures <= 20) {      \
                printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);     \
                printf("\n");            \
            }                            \
        }                                \
    } while (0)

static_assert(sizeof(mbx_vote_record) == 8 && offsetof(mbx_vote_record, agree) == 4 && sizeof(mbx::VoteRecord) == 8, "the record");
static_assert(MBX_VOTE_MAX_CANDIDATES == mbx::kVoteMaxCandidates && MBX_VOTE_NONE == mbx::kVoteNone && MBX_VOTE_COMBINED == mbx::kVoteCombined &&
                  MBX_VOTE_SELECT == mbx::kVoteSelect && MBX_VOTE_COMBINE == mbx::kVoteCombine,
              "constants");
static_assert(mbx::kVoteLanes * 2 == mbx::kVoteMaxCandidates && mbx::kVoteBlock == 256 && mbx::kVoteBlockFrames == 16, "the select partition");
static_assert(184 % mbx::kVotePieceCells == 0 && 168 % mbx::kVotePieceCells == 0 && 96 % mbx::kVotePieceCells == 0, "a row is whole pieces");

uint32_t rng_state = 24680u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

bool same(const mbx::VoteRecord& a, const mbx::VoteRecord& b) {
    return a.winner == b.winner && a.present == b.present && a.best == b.best && a.second == b.second && a.agree == b.agree;
}

// ---- select ----------------------------------------------------------------------------------------------------------------------------
struct Ranked {
    uint32_t total, c0;
    int      j;
};
// the rule as a sentence: of the present candidates the one with the fewest errors, then the smaller c0, then the lower index
mbx::VoteRecord plain_select(const mbx_param_record* cand, const uint8_t* present, size_t stride, int n, mbx_param_record* out) {
    std::vector<Ranked> there;
    for (int j = 0; j < n; ++j) {
        if (!present || present[(size_t)j * stride]) {
            const uint32_t w3 = cand[(size_t)j * stride].w[3];
            there.push_back(Ranked{(w3 & 255u) + ((w3 >> 8) & 255u), w3 & 255u, j});
        }
    }
    std::sort(there.begin(), there.end(), [](const Ranked& a, const Ranked& b) {
        return a.total != b.total ? a.total < b.total : (a.c0 != b.c0 ? a.c0 < b.c0 : a.j < b.j);
    });
    mbx::VoteRecord v;
    v.present = (uint8_t)there.size();
    if (there.empty()) {
        *out = cand[0];
        v.winner = 0xFF, v.best = 0xFF, v.second = 0xFF, v.agree = 0;
        return v;
    }
    const mbx_param_record& won = cand[(size_t)there[0].j * stride];
    *out = won;
    v.winner = (uint8_t)there[0].j;
    v.best = (uint8_t)std::min<uint32_t>(255u, there[0].total);
    v.second = there.size() > 1 ? (uint8_t)std::min<uint32_t>(255u, there[1].total) : 0xFF;
    v.agree = 0;
    for (const Ranked& r : there) {
        const mbx_param_record& c = cand[(size_t)r.j * stride];
        if (c.w[0] == won.w[0] && c.w[1] == won.w[1] && c.w[2] == won.w[2]) {
            v.agree |= 1u << r.j;
        }
    }
    return v;
}

// the 16 lanes of a frame, a value each; one xor step of the kernel's reductions
template <class Op>
void butterfly(uint32_t (&v)[16], Op op) {
    for (int m = 1; m < 16; m <<= 1) {
        uint32_t next[16];
        for (int j = 0; j < 16; ++j) {
            next[j] = op(v[j], v[j ^ m]);
        }
        memcpy(v, next, sizeof(v));
    }
}
// vote_select_kernel, lane by lane (mbx_vote.hip): loads clamped to the group's last candidate, two keys a lane, seven reductions
mbx::VoteRecord wave_select(const mbx_param_record* cand, const uint8_t* present, size_t stride, int n, mbx_param_record* out) {
    mbx_param_record r[2][16];
    uint32_t         key[2][16], there[2][16];
    bool             have[2][16];
    for (int j = 0; j < 16; ++j) {
        for (int h = 0; h < 2; ++h) {
            const int c = j + 16 * h;
            have[h][j] = c < n;
            const size_t at = (size_t)(c < n ? c : n - 1) * stride;
            r[h][j] = cand[at];
            there[h][j] = have[h][j] ? (present ? present[at] : 1u) : 0u;
            key[h][j] = there[h][j] ? mbx::vote_key(r[h][j].w[3], c) : mbx::kVoteAbsent;
        }
    }
    auto least = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    auto either = [](uint32_t a, uint32_t b) { return a | b; };
    uint32_t v[16];
    for (int j = 0; j < 16; ++j) {
        v[j] = least(key[0][j], key[1][j]);
    }
    butterfly(v, least);
    const uint32_t key1 = v[0];
    for (int j = 0; j < 16; ++j) {
        CHECK(v[j] == key1, "every lane holds the minimum");
        v[j] = least(key[0][j] == key1 ? mbx::kVoteAbsent : key[0][j], key[1][j] == key1 ? mbx::kVoteAbsent : key[1][j]);
    }
    butterfly(v, least);
    const uint32_t key2 = v[0];
    const bool     none = key1 == mbx::kVoteAbsent;
    uint32_t       w[3];
    int            stores = 0;
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 16; ++j) {
            const bool take0 = none ? j == 0 : key[0][j] == key1, take1 = !none && key[1][j] == key1;
            v[j] = take0 ? r[0][j].w[k] : (take1 ? r[1][j].w[k] : 0u);
            if (k == 0 && (take0 || take1)) {
                *out = take0 ? r[0][j] : r[1][j];
                ++stores;
            }
        }
        butterfly(v, either);
        w[k] = v[0];
    }
    CHECK(stores == 1, "%d lanes store the voted record", stores);
    for (int j = 0; j < 16; ++j) {
        v[j] = 0;
        for (int h = 0; h < 2; ++h) {
            if (have[h][j] && r[h][j].w[0] == w[0] && r[h][j].w[1] == w[1] && r[h][j].w[2] == w[2]) {
                v[j] |= 1u << (j + 16 * h);
            }
        }
    }
    butterfly(v, either);
    const uint32_t equal = v[0];
    for (int j = 0; j < 16; ++j) {
        v[j] = (there[0][j] ? 1u << j : 0u) | (there[1][j] ? 1u << (j + 16) : 0u);
    }
    butterfly(v, either);
    return mbx::vote_select_record(key1, key2, v[0], equal);
}

void check_select() {
    CHECK(mbx::vote_key(0x00000102u, 0) > mbx::vote_key(0x00000201u, 1), "a tie on the total goes to the smaller c0");
    CHECK(mbx::vote_key(0x0000FFFFu, 31) == ((510u << 16) | (255u << 8) | 31u) && mbx::vote_key(0xFFFFFFFFu, 31) < mbx::kVoteAbsent, "the largest key");
    CHECK(mbx::vote_errors_of_key(mbx::vote_key(0x0000C864u, 3)) == 255 && mbx::vote_errors_of_key(mbx::kVoteAbsent) == 255 &&
              mbx::vote_errors_of_key(mbx::vote_key(0x00000102u, 9)) == 3,
          "best and second");
    for (int n = 1; n <= 32; ++n) {
        for (int round = 0; round < 40; ++round) {
            const size_t stride = round & 1 ? 3 : 1;
            std::vector<mbx_param_record> cand((size_t)n * stride);
            std::vector<uint8_t>          present((size_t)n * stride);
            for (size_t i = 0; i < cand.size(); ++i) {
                const uint32_t words = rnd() % 3u;   // few different words: agreement happens
                cand[i] = mbx_param_record{{words, words * 7u, ~words, (rnd() % 3u) | ((rnd() % 3u) << 8) | (rnd() << 16)}};
                if (rnd() % 17u == 0) {
                    cand[i].w[3] |= 0xFFFFu;
                }
                present[i] = (uint8_t)((round % 5 == 4) ? 0 : (rnd() % 3u ? 1 + rnd() % 255u : 0));
            }
            const uint8_t*   pr = round % 4 == 0 ? nullptr : present.data();
            mbx_param_record a, b, c;
            const mbx::VoteRecord want = plain_select(cand.data(), pr, stride, n, &a);
            const mbx::VoteRecord got = mbx::vote_select_frame(cand.data(), pr, stride, n, &b);
            const mbx::VoteRecord wave = wave_select(cand.data(), pr, stride, n, &c);
            CHECK(same(want, got) && memcmp(&a, &b, 16) == 0, "n %d round %d: the definition", n, round);
            CHECK(same(want, wave) && memcmp(&a, &c, 16) == 0, "n %d round %d: the wave (winner %d / %d, agree %08x / %08x)", n, round, want.winner, wave.winner,
                  want.agree, wave.agree);
        }
    }
}

// ---- combine ----------------------------------------------------------------------------------------------------------------------------
mbx::VoteRecord plain_combine(const mbe_soft_bit* cand, const uint8_t* present, size_t stride, int n, int cells, mbe_soft_bit* out) {
    mbx::VoteRecord v;
    v.best = v.second = 0xFF;
    v.agree = 0;
    int first = -1;
    for (int j = 0; j < n; ++j) {
        if (!present || present[(size_t)j * stride]) {
            v.agree |= 1u << j;
            first = first < 0 ? j : first;
        }
    }
    v.present = (uint8_t)__builtin_popcount(v.agree);
    v.winner = first < 0 ? 0xFF : 0xFE;
    for (int i = 0; i < cells; ++i) {
        long sum = 0;
        for (int j = 0; j < n; ++j) {
            if (v.agree & (1u << j)) {
                const mbe_soft_bit& c = cand[(size_t)j * stride * (size_t)cells + (size_t)i];
                sum += c.bit ? (long)c.reliability : -(long)c.reliability;
            }
        }
        if (first < 0) {
            out[i] = cand[i];
        } else {
            out[i].bit = sum > 0 ? 1 : (sum < 0 ? 0 : cand[(size_t)first * stride * (size_t)cells + (size_t)i].bit);
            out[i].reliability = (uint8_t)std::min(255l, sum < 0 ? -sum : sum);
        }
    }
    return v;
}
// vote_combine_kernel, lane by lane: a piece of eight cells as four little-endian dwords
void wave_combine(const mbe_soft_bit* cand, const uint8_t* present, size_t stride, int n, int cells, mbe_soft_bit* out) {
    for (int p = 0; p < cells / mbx::kVotePieceCells; ++p) {
        uint32_t cur[4], zeroth[4], first[4];
        memcpy(cur, cand + (size_t)p * 8u, 16);
        memcpy(zeroth, cur, 16);
        memcpy(first, cur, 16);
        uint32_t here = present ? present[0] : 1u, mask = 0;
        int32_t  V[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < n; ++j) {
            const size_t ahead = (size_t)(j + 1 < n ? j + 1 : j) * stride;
            uint32_t     next[4];
            memcpy(next, cand + ahead * (size_t)cells + (size_t)p * 8u, 16);
            const uint32_t next_here = present ? present[ahead] : 1u;
            if (here) {
                if (!mask) {
                    memcpy(first, cur, 16);
                }
                mask |= 1u << j;
                for (int i = 0; i < 4; ++i) {
                    V[2 * i] += mbx::vote_cell_value(cur[i] & 255u, (cur[i] >> 8) & 255u);
                    V[2 * i + 1] += mbx::vote_cell_value((cur[i] >> 16) & 255u, cur[i] >> 24);
                }
            }
            memcpy(cur, next, 16);
            here = next_here;
        }
        uint32_t o[4];
        for (int i = 0; i < 4; ++i) {
            o[i] = mask ? mbx::vote_cell_out(V[2 * i], first[i]) | (mbx::vote_cell_out(V[2 * i + 1], first[i] >> 16) << 16) : zeroth[i];
        }
        memcpy(out + (size_t)p * 8u, o, 16);
    }
}

void check_combine() {
    CHECK(mbx::vote_cell_out(32 * 255, 0) == (1u | (255u << 8)) && mbx::vote_cell_out(-32 * 255, 1) == (0u | (255u << 8)), "saturation");
    CHECK(mbx::vote_cell_out(0, 1) == 1u && mbx::vote_cell_out(0, 0) == 0u && mbx::vote_cell_out(0, 0xABCD01u) == 1u, "V = 0 keeps the first bit byte");
    CHECK(mbx::vote_cell_value(1, 0) == 0 && mbx::vote_cell_value(0, 9) == -9 && mbx::vote_cell_value(2, 9) == 9, "a cell's value");
    const int shapes[3] = {184, 168, 96};
    for (int n = 1; n <= 32; n += (n < 5 ? 1 : 9)) {
        for (int round = 0; round < 24; ++round) {
            const int    cells = shapes[round % 3];
            const size_t stride = round & 1 ? 3 : 1;
            std::vector<mbe_soft_bit> cand((size_t)n * stride * (size_t)cells), a((size_t)cells), b((size_t)cells), c((size_t)cells);
            std::vector<uint8_t>      present((size_t)n * stride);
            for (mbe_soft_bit& x : cand) {
                x.bit = (uint8_t)(rnd() & 1u);
                x.reliability = (uint8_t)(rnd() % 4u == 0 ? rnd() % 2u : (round % 6 == 5 ? 255u : rnd() % 256u));
            }
            for (uint8_t& x : present) {
                x = (uint8_t)((round % 8 == 7) ? 0 : (rnd() % 3u ? 1 + rnd() % 255u : 0));
            }
            const uint8_t* pr = round % 4 == 0 ? nullptr : present.data();
            const mbx::VoteRecord want = plain_combine(cand.data(), pr, stride, n, cells, a.data());
            const mbx::VoteRecord got = mbx::vote_combine_frame(cand.data(), pr, stride, n, cells, b.data());
            wave_combine(cand.data(), pr, stride, n, cells, c.data());
            CHECK(same(want, got) && memcmp(a.data(), b.data(), (size_t)cells * 2u) == 0, "n %d round %d: the definition", n, round);
            CHECK(memcmp(a.data(), c.data(), (size_t)cells * 2u) == 0, "n %d round %d: the wave", n, round);
            if (n == 1 && !pr) {
                CHECK(memcmp(a.data(), cand.data(), (size_t)cells * 2u) == 0, "identity ONE");
            }
        }
    }
}

// ---- the refusals ---------------------------------------------------------------------------------------------------------------------------
void check_refusals() {
    using namespace mbx;
    int stream = -1, largest = -1;
    const int32_t good[6] = {0, 1, 3, 6, 22, 54};
    CHECK(vote_offsets_refused(false, good, 5, &stream, &largest) == kVotePointers && vote_offsets_refused(true, nullptr, 5, &stream, &largest) == kVotePointers, "pointers");
    CHECK(vote_offsets_refused(true, good, 0, &stream, &largest) == kVoteStreams && vote_offsets_refused(true, good, -3, &stream, &largest) == kVoteStreams, "S");
    CHECK(vote_offsets_refused(true, good, 5, &stream, &largest) == kVoteOk && largest == 32, "the grouping of the tests, largest %d", largest);
    const int32_t first[3] = {1, 2, 3}, empty[4] = {0, 2, 2, 3}, big[3] = {0, 1, 34}, down[4] = {0, 4, 3, 5}, far[3] = {0, 1, INT32_MIN};
    CHECK(vote_offsets_refused(true, first, 2, &stream, &largest) == kVoteFirst, "cand_offset[0]");
    CHECK(vote_offsets_refused(true, empty, 3, &stream, &largest) == kVoteGroup && stream == 1, "an empty group, stream %d", stream);
    CHECK(vote_offsets_refused(true, big, 2, &stream, &largest) == kVoteGroup && stream == 1, "33 candidates, stream %d", stream);
    CHECK(vote_offsets_refused(true, down, 3, &stream, &largest) == kVoteGroup && stream == 1, "descending, stream %d", stream);
    CHECK(vote_offsets_refused(true, far, 2, &stream, &largest) == kVoteGroup && stream == 1, "no overflow in the difference");
    char text[160];
    vote_group_text(text, sizeof(text), 1, 1, 34);
    CHECK(strcmp(text, "stream 1: 33 candidates (offsets 1 .. 34), a group has 1 .. MBX_VOTE_MAX_CANDIDATES (32)") == 0, "%s", text);
    // the launches: pointers as numbers.  S = 5, C = 54
    const auto P = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
    CHECK(vote_select_refused(0, 0, -1, P(0x1001), nullptr, P(0x2003), P(0x3001)) == kVotePointers, "no plan");
    CHECK(vote_select_refused(5, 54, -1, nullptr, nullptr, P(0x2003), nullptr) == kVotePointers && vote_select_refused(5, 54, -1, P(0x1001), nullptr, nullptr, nullptr) == kVotePointers, "pointers first");
    CHECK(vote_select_refused(5, 54, -1, P(0x1001), nullptr, P(0x2003), P(0x3001)) == kVoteFrames, "T");
    CHECK(vote_select_refused(5, 54, INT32_MAX / 54 + 1, P(0x1001), nullptr, P(0x2003), nullptr) == kVoteSize && vote_shape_refused(54, INT32_MAX / 54) == kVoteOk, "the size");
    CHECK(vote_select_refused(5, 54, 3, P(0x10008), nullptr, P(0x20000), nullptr) == kVoteAlign && vote_select_refused(5, 54, 3, P(0x10000), nullptr, P(0x20008), nullptr) == kVoteAlign &&
              vote_select_refused(5, 54, 3, P(0x10000), P(0x7), P(0x20000), P(0x30004)) == kVoteAlign,
          "alignment");
    CHECK(vote_select_refused(5, 54, 3, P(0x10000), P(0x7), P(0x20000), P(0x30008)) == kVoteOk, "present bytes anywhere, votes at 8");
    CHECK(vote_select_refused(5, 54, 3, P(0x10000), nullptr, P(0x10000 + 54 * 3 * 16 - 16), nullptr) == kVoteOverlap && vote_select_refused(5, 54, 3, P(0x10000), nullptr, P(0x10000 + 54 * 3 * 16), nullptr) == kVoteOk,
          "records over candidates");
    CHECK(vote_select_refused(5, 54, 3, P(0x10000), P(0x20000 + 5 * 3 * 16 - 1), P(0x20000), nullptr) == kVoteOverlap && vote_select_refused(5, 54, 3, P(0x10000), nullptr, P(0x20000), P(0x20000 + 5 * 3 * 16 - 8)) == kVoteOverlap,
          "records over present, votes over records");
    CHECK(vote_select_refused(5, 54, 0, P(0x10000), nullptr, P(0x10000), P(0x10000)) == kVoteOk, "T = 0 moves nothing");
    CHECK(vote_combine_refused(0, 0, 7, -1, P(0x1001), nullptr, P(0x2003), nullptr) == kVotePointers && vote_combine_refused(5, 54, 7, -1, P(0x1001), nullptr, P(0x2003), nullptr) == kVoteCells, "row_cells behind the pointers");
    for (int cells : {184, 168, 96}) {
        CHECK(vote_combine_refused(5, 54, cells, -1, P(0x1001), nullptr, P(0x2003), nullptr) == kVoteFrames, "T behind row_cells");
        CHECK(vote_combine_refused(5, 54, cells, 1, P(0x10002), nullptr, P(0x80000), nullptr) == kVoteAlign, "cells at 16");
        CHECK(vote_combine_refused(5, 54, cells, 1, P(0x10000), nullptr, P(0x10000 + 54 * cells * 2 - 16), nullptr) == kVoteOverlap && vote_combine_refused(5, 54, cells, 1, P(0x10000), nullptr, P(0x10000 + 54 * cells * 2), nullptr) == kVoteOk, "overlap");
        CHECK(vote_combine_grid(5 * 3, cells) == (uint32_t)((15 * (cells / 8) + 255) / 256), "the grid");
    }
    CHECK(vote_combine_refused(5, 54, 72, 1, P(0x10000), nullptr, P(0x80000), nullptr) == kVoteCells, "72 is no row");
    CHECK(vote_workspace_bytes(kVoteSelect, 5, 54, 3, 184) == 54u * 3u * 16u && vote_workspace_bytes(kVoteCombine, 5, 54, 3, 96) == 5u * 3u * 192u, "workspace bytes");
    CHECK(vote_select_grid(1) == 1 && vote_select_grid(16) == 1 && vote_select_grid(17) == 2, "the select grid");
    CHECK(strstr(vote_refusal_text(kVoteAlign), "include/mbx_vote.h, Alignment") != nullptr && strlen(vote_refusal_text(kVotePointers)) > 0, "texts");
}

}  // namespace

int main() {
    check_select();
    check_combine();
    check_refusals();
    if (failures) {
        printf("vote_check: %d FAILED\n", failures);
        return 1;
    }
    printf("vote_check: ok (%d lanes per frame, up to %d candidates, pieces of %d cells)\n", mbx::kVoteLanes, mbx::kVoteMaxCandidates, mbx::kVotePieceCells);
    return 0;
}
