// levels_check.cpp -- host check of levels out and the gated mix-down (include/mbx_levels.h), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_levels_host.py; a program of its own, nothing of it is loaded anywhere else.
//   the level arithmetic the kernel and the host function share (mbelib-neo_amd/csrc/mbx_levels.h) on the extremes and against a naive
//     loop, and the kernel's partition walked as a wave walks it: 16 lanes per row, ten samples each, four xor steps;
//   the identities of the kernel's packed 16-bit arithmetic for every int16;
//   the rank key: its order, its uniqueness within a bus, equal energies, a row twice in a bus, the position back out of the key;
//   "the N-th largest key of a bus" against a plain sort for every N in 0 .. 8 and bus sizes 0, 1, N - 1, N, N + 1, 23, 257, 4096, and
//     the long kernel's rounds ("the largest key below the previous round's") against the same;
//   what mbx_pcm_levels and mbx_mixdown_gated refuse of their arguments (mbx_levels_plan.h): pointers as numbers, never dereferenced;
//   the record's size and offsets.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "mbx_levels_plan.h"   // (and through it the arithmetic, csrc/mbx_levels.h)

#include <mbx_levels.h>   // the public header of the same name (include/ is first on the include path)

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

static_assert(sizeof(mbx_row_level) == 16 && offsetof(mbx_row_level, energy) == 0 && offsetof(mbx_row_level, peak) == 8
                  && offsetof(mbx_row_level, clipped) == 10 && offsetof(mbx_row_level, zero) == 12, "the record");
static_assert(sizeof(mbx_mixdown_gate) == 4 && offsetof(mbx_mixdown_gate, open_peak) == 0 && offsetof(mbx_mixdown_gate, loudest_n) == 2, "the gate");
static_assert(mbx::kLevelLanes * mbx::kLevelSamples == 160 && mbx::kLevelSamples % 2 == 0, "a lane's share is whole dwords");
static_assert(MBX_GATE_MAX_LOUDEST == mbx::kGateMaxLoudest && MBX_SESSION_LEVELS == 32u && sizeof(mbx_row_level) == mbx::kLevelBytes, "constants");
static_assert((MBX_SESSION_LEVELS & (1u | 2u | 4u | 8u | MBX_SESSION_MIXDOWN)) == 0, "an outputs bit of its own");

uint32_t rng_state = 2468u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// ---- levels ---------------------------------------------------------------------------------------------------------------------------
struct Naive {
    long long energy = 0;
    int       peak = 0, clipped = 0;
};
Naive naive_level(const int16_t* x) {
    Naive l;
    for (int n = 0; n < 160; ++n) {
        const long long v = x[n];
        l.energy += v * v;
        const int a = (int)(v < 0 ? -v : v);
        l.peak = a > l.peak ? a : l.peak;
        l.clipped += x[n] == 32767 || x[n] == -32768;
    }
    return l;
}

// pcm_levels_kernel's walk of one row: 16 lanes, lane j takes the ten samples 10 j .. 10 j + 9; xor steps 1, 2, 4, 8
mbx::Level wave_walk(const int16_t* x) {
    mbx::Level lane[mbx::kLevelLanes];
    for (int j = 0; j < mbx::kLevelLanes; ++j) {
        for (int i = 0; i < mbx::kLevelSamples; ++i) {
            mbx::level_add_sample(lane[j], x[j * mbx::kLevelSamples + i]);
        }
    }
    for (int m = 1; m < mbx::kLevelLanes; m <<= 1) {
        mbx::Level next[mbx::kLevelLanes];
        for (int j = 0; j < mbx::kLevelLanes; ++j) {
            next[j] = lane[j];
            mbx::level_merge(next[j], lane[j ^ m]);
        }
        memcpy(lane, next, sizeof(lane));
    }
    for (int j = 1; j < mbx::kLevelLanes; ++j) {
        CHECK(lane[j].energy == lane[0].energy && lane[j].peak == lane[0].peak && lane[j].clipped == lane[0].clipped, "lane %d", j);
    }
    return lane[0];
}

void check_row(const char* what, const int16_t* x, long long energy, int peak, int clipped) {
    const mbx::Level l = mbx::level_of_row(x), w = wave_walk(x);
    const Naive n = naive_level(x);
    CHECK((long long)l.energy == energy && (int)l.peak == peak && (int)l.clipped == clipped, "%s: %llu %u %u", what, (unsigned long long)l.energy, l.peak, l.clipped);
    CHECK(n.energy == energy && n.peak == peak && n.clipped == clipped, "%s (naive)", what);
    CHECK(w.energy == l.energy && w.peak == l.peak && w.clipped == l.clipped, "%s (the wave's walk)", what);
    CHECK(mbx::level_peak_word(l) == ((uint32_t)peak | ((uint32_t)clipped << 16)), "%s (the record's word)", what);
}

void check_levels() {
    int16_t x[160];
    std::fill(x, x + 160, (int16_t)-32768);
    check_row("all -32768", x, 160ll << 30, 32768, 160);
    std::fill(x, x + 160, (int16_t)0);
    check_row("all 0", x, 0, 0, 0);
    for (int at : {0, 7, 8, 127, 128, 135, 159}) {
        std::fill(x, x + 160, (int16_t)0);
        x[at] = 32767;
        check_row("a single 32767", x, 32767ll * 32767, 32767, 1);
        x[at] = -32767;
        check_row("a single -32767", x, 32767ll * 32767, 32767, 0);
        x[at] = -32768;
        check_row("a single -32768", x, 1ll << 30, 32768, 1);
    }
    for (int n = 0; n < 160; ++n) {
        x[n] = (int16_t)(n & 1 ? -1 : 1);
    }
    check_row("+-1", x, 160, 1, 0);
    std::fill(x, x + 160, (int16_t)32767);
    check_row("all 32767", x, 160ll * 32767 * 32767, 32767, 160);
    for (int t = 0; t < 200; ++t) {
        for (int n = 0; n < 160; ++n) {
            x[n] = (int16_t)(rnd() & 0xFFFF);
        }
        const Naive n = naive_level(x);
        check_row("random", x, n.energy, n.peak, n.clipped);
    }
}

// the identities behind the kernel's packed 16-bit arithmetic (level_add_pair, mbx_levels.hip), for every int16
void check_packed_identities() {
    for (int v = -32768; v <= 32767; ++v) {
        const int16_t x = (int16_t)v;
        const int16_t s = (int16_t)(x >> 15);
        const uint16_t t = (uint16_t)(x ^ s), a = (uint16_t)(t - (uint16_t)s), c = (uint16_t)((uint16_t)(t + 1u) >> 15);
        mbx::Level l;
        mbx::level_add_sample(l, x);
        CHECK(a == l.peak && (uint64_t)a * a == l.energy && c == l.clipped && t <= 32767, "x = %d", v);
    }
}

// ---- keys and thresholds --------------------------------------------------------------------------------------------------------------
void check_keys() {
    // closed is 0, open is never 0, and 51 bits hold the largest
    CHECK(mbx::gate_key(5, 99, 0, 100) == 0 && mbx::gate_key(5, 100, 0, 100) != 0 && mbx::gate_key(0, 0, 4095, 0) == 1, "open and closed");
    CHECK(mbx::gate_key(160ull << 30, 32768, 0, 32768) < (1ull << 51), "51 bits");
    CHECK(mbx::gate_key(160ull << 30, 32768, 0, 32768) == (((160ull << 30) << 12) | 4095u) + 1u, "the largest key");
    // the order: energy first, then the earlier position; a row twice in a bus has equal energies at two positions
    CHECK(mbx::gate_key(7, 1, 4095, 0) > mbx::gate_key(6, 1, 0, 0), "energy before position");
    CHECK(mbx::gate_key(7, 1, 3, 0) > mbx::gate_key(7, 1, 4, 0), "the earlier position wins a tie");
    for (int32_t k : {0, 1, 255, 256, 4094, 4095}) {
        for (uint64_t e : {0ull, 1ull, 160ull << 30}) {
            CHECK(mbx::gate_key_position(mbx::gate_key(e, 0, k, 0)) == k, "position %d", k);
        }
    }
    // uniqueness within a bus of 4,096 inputs that share one energy (one row 4,096 times)
    std::vector<uint64_t> keys;
    for (int32_t k = 0; k < 4096; ++k) {
        keys.push_back(mbx::gate_key(12345, 9, k, 0));
    }
    for (int32_t k = 1; k < 4096; ++k) {
        CHECK(keys[(size_t)k] < keys[(size_t)k - 1], "strictly decreasing with the position, %d", k);
    }
}

// the definition by a plain sort: the N-th largest open key, or 1
uint64_t sorted_threshold(std::vector<uint64_t> keys, int n) {
    std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
    if (n == 0 || (size_t)n > keys.size() || keys[(size_t)n - 1] == 0) {
        return 1;
    }
    return keys[(size_t)n - 1];
}

// mixdown_gated_long_kernel's rounds over the whole bus: the largest key below the previous round's, N times or until none is left
uint64_t rounds_threshold(const std::vector<uint64_t>& keys, int n, int* found) {
    uint64_t below = ~(uint64_t)0, last = 0;
    *found = 0;
    for (int r = 0; r < n; ++r) {
        uint64_t m = 0;
        for (uint64_t k : keys) {
            m = (k < below && k > m) ? k : m;
        }
        if (m == 0) {
            break;
        }
        last = below = m;
        ++*found;
    }
    return last ? last : 1;
}

void check_thresholds() {
    for (int n = 0; n <= mbx::kGateMaxLoudest; ++n) {
        std::vector<int> sizes = {0, 1, n - 1, n, n + 1, 23, 257, 4096};
        for (int size : sizes) {
            if (size < 0) {
                continue;
            }
            for (int flavour = 0; flavour < 4; ++flavour) {   // all open and distinct | many closed | few energies (ties) | all closed
                std::vector<uint64_t> keys;
                for (int32_t k = 0; k < size; ++k) {
                    const uint64_t energy = flavour == 2 ? rnd() % 3 : ((uint64_t)rnd() << 14) ^ rnd();
                    const uint32_t peak = flavour == 3 ? 0 : (flavour == 1 ? rnd() % 4 : 50);
                    keys.push_back(mbx::gate_key(energy % (160ull << 30), peak, k, 2));
                }
                const uint64_t want = sorted_threshold(keys, n), got = mbx::gate_threshold(keys.data(), size, n);
                CHECK(got == want, "N %d, size %d, flavour %d: %llu, want %llu", n, size, flavour, (unsigned long long)got, (unsigned long long)want);
                long open = 0, taken = 0;
                for (uint64_t k : keys) {
                    open += k != 0;
                    taken += k >= got;
                }
                CHECK(taken == (n == 0 ? open : std::min<long>(n, open)), "N %d, size %d, flavour %d: %ld chosen of %ld open", n, size, flavour, taken, open);
                if (n > 0) {
                    int found = 0;
                    const uint64_t by_rounds = rounds_threshold(keys, n, &found);
                    // (with fewer than N open inputs the rounds end at the smallest open key where the definition says 1: the same choice)
                    bool same = found == std::min<long>(n, open);
                    for (uint64_t k : keys) {
                        same = same && (k >= by_rounds) == (k >= want);
                    }
                    CHECK(same && (open < n || by_rounds == want), "the rounds: N %d, size %d, flavour %d", n, size, flavour);
                }
            }
        }
    }
    // more than N inputs share the top energy: the first N positions are chosen
    std::vector<uint64_t> keys;
    for (int32_t k = 0; k < 10; ++k) {
        keys.push_back(mbx::gate_key(k == 4 ? 1 : 1000, 5, k, 0));
    }
    const uint64_t t = mbx::gate_threshold(keys.data(), 10, 3);
    for (int32_t k = 0; k < 10; ++k) {
        CHECK((keys[(size_t)k] >= t) == (k < 3), "tie at the top, position %d", k);
    }
}

// ---- refusals -------------------------------------------------------------------------------------------------------------------------
const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

void check_refusals() {
    using namespace mbx;
    CHECK(levels_launch_refused(at(0x1000), 4, at(0x2000)) == kLevelsOk, "a good call");
    CHECK(levels_launch_refused(at(0x1000), 0, at(0x1000)) == kLevelsOk, "no rows overlap nothing");
    CHECK(levels_launch_refused(nullptr, 4, at(0x2000)) == kLevelsPointers && levels_launch_refused(at(0x1000), 4, nullptr) == kLevelsPointers, "NULL");
    for (uintptr_t off : {1u, 2u, 4u, 8u}) {
        CHECK(levels_launch_refused(at(0x1000 + off), 4, at(0x2000)) == kLevelsAlign && levels_launch_refused(at(0x1000), 4, at(0x2000 + off)) == kLevelsAlign, "below 16");
    }
    CHECK(levels_launch_refused(at(0x1000), (size_t)INT32_MAX + 1, at(0x10)) == kLevelsRows, "too many rows");
    CHECK(levels_launch_refused(at(0x1000), 4, at(0x1000 + 4 * 320 - 16)) == kLevelsOverlap && levels_launch_refused(at(0x1000), 4, at(0x1000 + 4 * 320)) == kLevelsOk, "levels behind the rows");
    CHECK(levels_launch_refused(at(0x1040), 4, at(0x1000 + 16)) == kLevelsOverlap && levels_launch_refused(at(0x1040), 4, at(0x1000)) == kLevelsOk, "levels in front of the rows");
    CHECK(levels_grid(1) == 1 && levels_grid(16) == 1 && levels_grid(17) == 2 && levels_grid(65536) == 4096 && levels_grid(kLevelsMaxRows) == (1u << 27), "the grid");

    const int32_t off[3] = {0, 2, 3}, row[3] = {4, 4, 0};
    MixdownPlan plan;
    CHECK(plan_mixdown(2, off, row, 0, &plan) == kMixdownOk && plan.rows_needed == 5, "a plan");
    MixdownRefusal mix;
    // rows at 0x10000 (8 rows: 2,560 bytes), levels at 0x20000 (128 bytes), out at 0x30000 (2 buses: 640 / 320 bytes)
    const auto gated = [&](const MixdownPlan* p, bool have, unsigned peak, unsigned n, int form, uintptr_t in, size_t nrows, uintptr_t lv, uintptr_t out) {
        return gated_launch_refused(p, have, peak, n, form, at(in), nrows, at(lv), at(out), &mix);
    };
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x20000, 0x30000) == kLevelsOk && mix == kMixdownOk, "a good call");
    CHECK(gated(&plan, true, 32768, 8, 2, 0x10000, 8, 0x20000, 0x30008) == kLevelsOk, "the limits of the gate, bytes at 8");
    CHECK(gated(&plan, false, 0, 0, 0, 0x10000, 8, 0x20000, 0x30000) == kGateNull, "no gate");
    CHECK(gated(&plan, true, 0, 9, 0, 0x10000, 8, 0x20000, 0x30000) == kGateLoudest, "loudest_n 9");
    CHECK(gated(&plan, true, 32769, 0, 0, 0x10000, 8, 0x20000, 0x30000) == kGatePeak, "open_peak 32769");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0, 0x30000) == kLevelsPointers, "no levels");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x20008, 0x30000) == kLevelsAlign, "levels at 8");
    CHECK(gated(&plan, true, 0, 0, 3, 0x10000, 8, 0x20000, 0x30000) == kGateMixdown && mix == kMixdownForm, "form");
    CHECK(gated(&plan, true, 0, 0, 0, 0, 8, 0x20000, 0x30000) == kGateMixdown && mix == kMixdownPointers, "no rows");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x20000, 0) == kGateMixdown && mix == kMixdownPointers, "no out");
    CHECK(gated(nullptr, true, 0, 0, 0, 0x10000, 8, 0x20000, 0x30000) == kGateMixdown && mix == kMixdownPointers, "no plan");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10008, 8, 0x20000, 0x30000) == kGateMixdown && mix == kMixdownAlign, "rows at 8");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x20000, 0x30008) == kGateMixdown && mix == kMixdownAlign, "int16 buses at 8");
    CHECK(gated(&plan, true, 0, 0, 1, 0x10000, 8, 0x20000, 0x30004) == kGateMixdown && mix == kMixdownAlign, "byte buses at 4");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 4, 0x20000, 0x30000) == kGateMixdown && mix == kMixdownRows, "rows short of the plan");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x20000, 0x10000 + 2560 - 16) == kGateMixdown && mix == kMixdownOverlap, "out in the rows");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x10000 + 2560 - 16, 0x30000) == kLevelsOverlap, "levels in the rows");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x10000 + 2560, 0x30000) == kLevelsOk, "levels right behind the rows");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x30000 + 640 - 16, 0x30000) == kLevelsOverlap, "levels in the int16 buses");
    CHECK(gated(&plan, true, 0, 0, 1, 0x10000, 8, 0x30000 + 320, 0x30000) == kLevelsOk, "levels right behind the byte buses");
    CHECK(gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x30000 - 128 + 16, 0x30000) == kLevelsOverlap && gated(&plan, true, 0, 0, 0, 0x10000, 8, 0x30000 - 128, 0x30000) == kLevelsOk,
          "levels in front of the buses");
    for (int r = kLevelsPointers; r < kGateMixdown; ++r) {
        CHECK(levels_refusal_text((LevelsRefusal)r)[0] != 0, "a refusal without a text: %d", r);
    }
    CHECK(gate_refused(true, 32768, 8) == kLevelsOk && gate_refused(true, 0, 0) == kLevelsOk, "the gate's limits");
}

}  // namespace

int main() {
    check_levels();
    check_packed_identities();
    check_keys();
    check_thresholds();
    check_refusals();
    if (failures) {
        printf("levels_check: %d FAILED\n", failures);
        return 1;
    }
    printf("levels_check: ok (%d lanes per row, loudest_n up to %d)\n", mbx::kLevelLanes, mbx::kGateMaxLoudest);
    return 0;
}
