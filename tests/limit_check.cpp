// limit_check.cpp -- host check of limited buses (include/mbx_limit.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_limit_host.py; a program of its own, nothing of it is loaded anywhere else.
//   every refusal of mbelib-neo_amd/csrc/mbx_limit_plan.h: the parameters, the state, the shape of a call, a range of records, a record
//     -- pointers as numbers, never dereferenced;
//   the arithmetic of a whole row -- clamp, peak, n*, the decision, g(n), y -- against the rule of the header written out in 64 bits
//     with true floor divisions, over scripted and seeded rows, records and parameter sets;
//   the BOUNDS of the header asserted per sample, every product computed in 64 bits beside the 32-bit one: |s' * g(n)| <= ceiling << 15,
//     |y| <= ceiling, (g0 - g1) * R <= 2^22, the release term below 2^24; "need < g0 exactly when n* < 160";
//   the three identities; the record as a word, the grid and the allocation.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mbx_limit_plan.h"

#include <mbx_limit.h>   // the public header (include/ is first on the include path)

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

static_assert(sizeof(mbx_limit) == 8 && offsetof(mbx_limit, ceiling) == 0 && offsetof(mbx_limit, release_q8) == 2 && offsetof(mbx_limit, hold_frames) == 3
                  && offsetof(mbx_limit, ramp_log2) == 4 && offsetof(mbx_limit, zero) == 5,
              "the limit");
static_assert(sizeof(mbx_limit_record) == 4 && offsetof(mbx_limit_record, gain_q15) == 0 && offsetof(mbx_limit_record, hold_left) == 2, "the state record");
static_assert(MBX_LIMIT_UNITY_Q15 == mbx::kLimitUnity && MBX_LIMIT_MIN_CEILING == mbx::kLimitMinCeiling && MBX_LIMIT_MAX_CEILING == mbx::kLimitMaxCeiling
                  && MBX_LIMIT_RANGE_LOG2 == mbx::kLimitRangeLog2 && MBX_LIMIT_MAX_RAMP_LOG2 == mbx::kLimitMaxRampLog2
                  && MBX_LIMIT_MAX_RAMP_LOG2 == MBX_HOLD_MAX_RAMP_LOG2,
              "constants");

const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

long long floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// ---- refusals -------------------------------------------------------------------------------------------------------------------------
void check_refusals() {
    using namespace mbx;
    CHECK(!mixdown_form_ok(kMixdownSums) && kMixdownSums == 3, "the sums are no form: the public form 3 stays refused");
    CHECK(limit_refused(true, 24000, 3, 0) == kLimitOk && limit_refused(true, 1024, 0, 0) == kLimitOk && limit_refused(true, 32767, 7, 0) == kLimitOk, "good limits");
    CHECK(limit_refused(false, 24000, 3, 0) == kLimitNull, "no limit");
    CHECK(limit_refused(true, 1023, 3, 0) == kLimitCeiling && limit_refused(true, 0, 3, 0) == kLimitCeiling && limit_refused(true, 32768, 3, 0) == kLimitCeiling
              && limit_refused(true, 65535, 3, 0) == kLimitCeiling,
          "ceiling outside 1024 .. 32767");
    CHECK(limit_refused(true, 24000, 8, 0) == kLimitRamp && limit_refused(true, 24000, 255, 0) == kLimitRamp, "ramp_log2 8");
    CHECK(limit_refused(true, 24000, 3, 1) == kLimitZero && limit_refused(true, 24000, 7, 255) == kLimitZero, "a zero byte is not 0");
    CHECK(limit_refused(false, 0, 8, 1) == kLimitNull && limit_refused(true, 0, 8, 1) == kLimitCeiling && limit_refused(true, 1024, 8, 1) == kLimitRamp
              && limit_refused(true, 1024, 7, 1) == kLimitZero,
          "the order of the refusals");

    // the shape of a call: 4 x 2 rows of sums at 0x10000 (5120 bytes), out at 0x20000 (2560 bytes as int16, 1280 as bytes)
    for (int form = 0; form < 3; ++form) {
        CHECK(limit_rows_refused(4, 2, form, at(0x10000), at(0x20000), true) == kLimitOk, "apart: form %d", form);
        CHECK(limit_rows_refused(4, 2, form, at(0x10000), at(0x10000), true) == kLimitOverlap && limit_rows_refused(4, 2, form, at(0x10000), at(0x10000), false) == kLimitOverlap,
              "in place is an overlap: form %d", form);
        const uintptr_t bytes = 8u * 160u * (form == 0 ? 2u : 1u);
        CHECK(limit_rows_refused(4, 2, form, at(0x10000), at(0x10000 + 5120), true) == kLimitOk && limit_rows_refused(4, 2, form, at(0x10000), at(0x10000 - bytes), true) == kLimitOk,
              "right behind and right in front: form %d", form);
        CHECK(limit_rows_refused(4, 2, form, at(0x10000), at(0x10000 + 5120 - 16), true) == kLimitOverlap
                  && limit_rows_refused(4, 2, form, at(0x10000), at(0x10000 - bytes + 16), true) == kLimitOverlap,
              "a partial overlap: form %d", form);
    }
    CHECK(limit_rows_refused(0, 0, 0, at(0x10000), at(0x10000), true) == kLimitOk && limit_rows_refused(0, 5, 1, at(0x10000), at(0x10010), true) == kLimitOk, "nothing to do");
    CHECK(limit_rows_refused(-1, 2, 0, at(0x10000), at(0x20000), true) == kLimitCounts && limit_rows_refused(4, -1, 0, at(0x10000), at(0x20000), true) == kLimitCounts, "negative counts");
    CHECK(limit_rows_refused(65536, 32768, 0, at(0x10000), at(0x20000), true) == kLimitRows && limit_rows_refused(INT32_MAX, 2, 0, at(0x10000), at(0x20000), true) == kLimitRows,
          "n * T above 2^31 - 1");
    CHECK(limit_rows_refused(4, 2, 3, at(0x10000), at(0x20000), true) == kLimitForm && limit_rows_refused(4, 2, -1, at(0x10000), at(0x20000), true) == kLimitForm, "the form");
    CHECK(limit_rows_refused(4, 2, 0, nullptr, at(0x20000), true) == kLimitPointers && limit_rows_refused(4, 2, 0, at(0x10000), nullptr, true) == kLimitPointers, "NULL arrays");
    for (uintptr_t o : {2u, 4u, 8u}) {
        CHECK(limit_rows_refused(4, 2, 0, at(0x10000 + o), at(0x20000), true) == kLimitAlign && limit_rows_refused(4, 2, 0, at(0x10000), at(0x20000 + o), true) == kLimitAlign,
              "int16 rows at +%u", (unsigned)o);
        CHECK(limit_rows_refused(4, 2, 1, at(0x10000 + o), at(0x20000), true) == kLimitAlign, "sums at +%u", (unsigned)o);
        for (int form = 1; form < 3; ++form) {
            CHECK(limit_rows_refused(4, 2, form, at(0x10000), at(0x20000 + o), true) == (o == 8 ? kLimitOk : kLimitAlign), "byte rows at +%u", (unsigned)o);
        }
        CHECK(limit_rows_refused(4, 2, 0, at(0x10000 + o), at(0x20000 + o), false) == kLimitOk, "the host definition asks no alignment");
    }

    // the launcher: the parameters, the state, the shape, n against the state
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 4, 4, 2, 0, at(0x10000), at(0x20000)) == kLimitOk, "a good launch");
    CHECK(limit_launch_refused(false, 0, 8, 1, false, 0, -1, -1, 3, nullptr, nullptr) == kLimitNull, "no limit comes first");
    CHECK(limit_launch_refused(true, 24000, 8, 0, false, 0, -1, -1, 3, nullptr, nullptr) == kLimitRamp, "then the fields");
    CHECK(limit_launch_refused(true, 24000, 3, 0, false, 0, -1, -1, 3, nullptr, nullptr) == kLimitNoState, "then the state");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 2, -1, -1, 3, nullptr, nullptr) == kLimitCounts, "then the counts");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 2, 65536, 32768, 3, nullptr, nullptr) == kLimitRows, "then the rows");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 2, 4, 2, 3, nullptr, nullptr) == kLimitForm, "then the form");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 2, 4, 2, 0, nullptr, nullptr) == kLimitPointers, "then the pointers");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 2, 4, 2, 0, at(0x10008), at(0x20000)) == kLimitAlign, "then the alignment");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 2, 4, 2, 0, at(0x10000), at(0x10140)) == kLimitOverlap, "then the overlap");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 3, 4, 2, 0, at(0x10000), at(0x20000)) == kLimitBuses, "then n above the state");
    CHECK(limit_launch_refused(true, 24000, 3, 0, true, 5, 4, 2, 0, at(0x10000), at(0x20000)) == kLimitOk && limit_launch_refused(true, 24000, 3, 0, true, 0, 0, 1, 0, at(0x10000), at(0x20000)) == kLimitOk,
          "n below the state, and nothing on an empty one");

    // a range of records
    CHECK(limit_range_refused(true, 16, 0, 16) == kLimitOk && limit_range_refused(true, 16, 16, 0) == kLimitOk && limit_range_refused(true, 0, 0, 0) == kLimitOk, "good ranges");
    CHECK(limit_range_refused(false, 16, 0, 16) == kLimitNoState, "no state");
    CHECK(limit_range_refused(true, 16, -1, 2) == kLimitRange_ && limit_range_refused(true, 16, 0, -1) == kLimitRange_ && limit_range_refused(true, 16, 1, 16) == kLimitRange_
              && limit_range_refused(true, 16, 17, 0) == kLimitRange_ && limit_range_refused(true, 16, INT32_MAX, INT32_MAX) == kLimitRange_,
          "ranges outside the records");

    // records
    const uint32_t good[4] = {limit_word(32768, 0), limit_word(1, 255), limit_word(8, 1), kLimitFreshWord};
    CHECK(limit_records_refused(good, 4) == kLimitOk && limit_records_refused(good, 0) == kLimitOk, "good records");
    for (const uint32_t bad : {limit_word(0, 0), limit_word(32769, 0), limit_word(65535, 65535), limit_word(32768, 256), limit_word(32768, 65535)}) {
        uint32_t words[4];
        memcpy(words, good, sizeof(words));
        words[3] = bad;
        CHECK(limit_records_refused(words, 4) == kLimitRecord && limit_records_refused(words, 3) == kLimitOk && !limit_word_ok(bad), "record %08x", bad);
    }
    const mbx_limit_record rec = {0x1234, 0x0056};
    uint32_t word;
    memcpy(&word, &rec, 4);
    CHECK(word == limit_word(0x1234, 0x0056) && limit_word_gain(word) == 0x1234 && limit_word_hold(word) == 0x0056, "the record's word");
    const mbx_limit_record fresh = {32768, 0};
    memcpy(&word, &fresh, 4);
    CHECK(word == kLimitFreshWord, "a fresh record");
    for (int r = kLimitNull; r < kLimitRefusals; ++r) {
        CHECK(limit_refusal_text((LimitRefusal)r)[0] != 0, "a refusal without a text: %d", r);
    }
}

// ---- one row: the header's rule in 64 bits beside the shared 32-bit arithmetic -----------------------------------------------------------
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct RowStats {
    long rows = 0, attacks = 0, held = 0, slewed = 0, stopped = 0, idle = 0;
};

// the row `s` under `p` with the record (g0, h0) in front of it: returns the record behind it through *g1, *h1
void check_row(const int32_t s[160], const mbx::LimitParams& p, uint32_t g0, uint32_t h0, uint32_t* g1_out, uint32_t* h1_out, RowStats* stats) {
    using namespace mbx;
    const long long C = (long long)p.ceiling << 15, M = 1ll << 22, R = 1ll << p.ramp_log2;
    CHECK(C < (1ll << 30), "ceiling << 15 < 2^30");
    // the 64-bit restatement
    long long sc[160], a[160], P = 0, n_star = 160;
    for (int n = 0; n < 160; ++n) {
        sc[n] = s[n] < -M ? -M : s[n] > M ? M : s[n];
        a[n] = sc[n] < 0 ? -sc[n] : sc[n];
        P = a[n] > P ? a[n] : P;
    }
    const long long need = P <= (long long)p.ceiling ? 32768 : C / P;
    const long long thr0 = C / g0;
    for (int n = 159; n >= 0; --n) {
        CHECK((a[n] * g0 > C) == (a[n] > thr0), "a * g0 > C <=> a > thr0: a %lld g0 %u", a[n], g0);
        n_star = a[n] > thr0 ? n : n_star;
    }
    CHECK((n_star < 160) == (need < (long long)g0), "the attack condition: n* %lld, need %lld, g0 %u", n_star, need, g0);
    CHECK(need >= 8 && need <= 32768, "need is a gain of at least 8: %lld", need);
    long long g1, h1;
    uint32_t event;
    if (n_star < 160) {
        g1 = need, h1 = p.hold_frames, event = kLimitAttack;
        CHECK(((long long)g0 - g1) * R <= (1ll << 22) && g1 < (long long)g0, "(g0 - g1) * R <= 2^22");
    } else if (h0 > 0) {
        g1 = g0, h1 = h0 - 1, event = kLimitHeld;
    } else {
        const long long term = (32768 - (long long)g0) * p.release_q8 + 255;
        CHECK(term < (1ll << 24) && term >= 0, "the release term: %lld", term);
        const long long risen = g0 + (term >> 8);
        g1 = need < risen ? need : risen, h1 = 0;
        event = need < risen ? kLimitReleaseStopped : g0 == 32768 ? kLimitIdle : kLimitReleaseSlewed;
        CHECK(g1 >= (long long)g0 && g1 <= 32768, "a release never lowers the gain and stops at unity: %u -> %lld", g0, g1);
        if (p.release_q8 == 0) {
            CHECK(g1 == (long long)g0, "release_q8 = 0 never raises a gain");
        }
    }
    // the shared arithmetic, as mbx_bus_limit_host and the kernel walk it
    uint32_t peak = 0, first = 160u;
    const uint32_t thr = limit_threshold(p.ceiling, g0);
    int32_t x[160];
    for (int k = 159; k >= 0; --k) {
        x[k] = limit_clamped(s[k]);
        const uint32_t m = limit_magnitude(x[k]);
        peak = m > peak ? m : peak;
        first = m > thr ? (uint32_t)k : first;
    }
    const LimitDecision d = limit_decide(peak, first, g0, h0, p);
    CHECK((long long)peak == P && (long long)first == n_star && (long long)thr == thr0, "P %u / %lld, n* %u / %lld, thr0 %u / %lld", peak, P, first, n_star, thr, thr0);
    CHECK((long long)d.gain == g1 && (long long)d.hold == h1 && (long long)d.need == need && d.event == event, "the decision: {%u, %u, %u, %u}, want {%lld, %lld, %lld, %u}",
          d.gain, d.hold, d.need, d.event, g1, h1, need, event);
    CHECK(limit_word_ok(limit_word(d.gain, d.hold)), "a decision is a good record: %u %u", d.gain, d.hold);
    const LimitRamp ramp = limit_ramp(first < 160u, (int32_t)g0, (int32_t)d.gain, (int)first);
    CHECK(ramp.delta >= 0, "the shifted difference is not negative");
    for (int n = 0; n < 160; ++n) {
        long long g;
        if (n_star < 160) {
            const long long ahead = n_star - n, w = ahead < 0 ? 0 : ahead > R ? R : ahead;
            g = g1 + floor_div(((long long)g0 - g1) * w, R);
            CHECK(n < n_star - R ? g == (long long)g0 : n >= n_star ? g == g1 : (g >= g1 && g <= (long long)g0), "g0 until R in front of n*, g1 from n* on: n %d g %lld", n, g);
        } else {
            const long long w = n + 1 < R ? n + 1 : R;
            g = g0 + floor_div((g1 - (long long)g0) * w, R);
            CHECK(g >= (long long)g0 && g <= g1 && (n < R - 1 || g == g1), "the ramp up: n %d g %lld", n, g);
        }
        const int32_t got = limit_gain_at(ramp, n, p.ramp_log2);
        CHECK((long long)got == g && got >= 1 && got <= kLimitUnity, "g(%d): %d, want %lld", n, got, g);
        // BOUNDS, per sample
        const long long product = sc[n] * g;
        CHECK(product <= C && product >= -C, "|s' * g(n)| <= ceiling << 15: n %d, %lld * %lld", n, sc[n], g);
        const long long y = floor_div(product + 16384, 32768);
        CHECK(y <= (long long)p.ceiling && y >= -(long long)p.ceiling, "|y| <= ceiling: n %d, y %lld", n, y);
        const int16_t y16 = limit_scaled(x[n], got);
        CHECK((long long)y16 == y, "y[%d]: %d, want %lld", n, y16, y);
        CHECK(limit_byte(kMixdownUlaw, y16) == pcm16_to_ulaw(y16) && limit_byte(kMixdownAlaw, y16) == pcm16_to_alaw(y16), "the bytes are those of mbx_compand.h");
    }
    *g1_out = d.gain, *h1_out = d.hold;
    ++stats->rows;
    stats->attacks += event == kLimitAttack, stats->held += event == kLimitHeld, stats->slewed += event == kLimitReleaseSlewed;
    stats->stopped += event == kLimitReleaseStopped, stats->idle += event == kLimitIdle;
}

void check_rows() {
    using namespace mbx;
    const LimitParams sets[] = {{24000, 64, 2, 3}, {32767, 255, 0, 7}, {1024, 1, 255, 0}, {32767, 0, 0, 5}, {1024, 255, 1, 7}, {8000, 128, 3, 1}, {30000, 32, 0, 6}, {16384, 200, 5, 2}};
    const int32_t levels[] = {0, 1, 100, 1023, 1024, 1025, 8000, 23999, 24000, 24001, 32766, 32767, 32768, 32769, 65536, 300000, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, INT32_MAX};
    const uint32_t gains[] = {1, 7, 8, 9, 187, 1000, 8191, 16384, 24000, 32766, 32767, 32768};
    RowStats stats;
    int32_t s[160];
    for (const LimitParams& p : sets) {
        // scripted: every level as a lone spike at the ends and in the middle of the row, either sign, over a background, from every gain
        for (int32_t level : levels) {
            for (int pos : {0, 1, 2, 63, 127, 128, 158, 159}) {
                for (int sign : {1, -1}) {
                    for (uint32_t g0 : gains) {
                        for (int n = 0; n < 160; ++n) {
                            s[n] = (int32_t)(rnd() % 2001u) - 1000;
                        }
                        s[pos] = sign > 0 ? level : (level == INT32_MAX ? INT32_MIN : -level);
                        uint32_t g1, h1;
                        check_row(s, p, g0, g0 & 1u ? 0u : 3u, &g1, &h1, &stats);
                    }
                }
            }
        }
        // seeded: sequences of rows with the record carried, loud and quiet stretches
        uint32_t g = kLimitUnity, h = 0;
        for (int f = 0; f < 600; ++f) {
            const uint32_t kind = rnd() % 8u;
            const uint32_t amp = kind == 0 ? 0u : kind < 4 ? 2000u : kind < 6 ? 30000u : kind == 6 ? 200000u : 6000000u;
            for (int n = 0; n < 160; ++n) {
                s[n] = amp ? (int32_t)(rnd() % (2u * amp + 1u)) - (int32_t)amp : 0;
            }
            check_row(s, p, g, h, &g, &h, &stats);
        }
    }
    CHECK(stats.attacks > 1000 && stats.held > 1000 && stats.slewed > 100 && stats.stopped > 100 && stats.idle > 100, "every kind of row: %ld %ld %ld %ld %ld of %ld",
          stats.attacks, stats.held, stats.slewed, stats.stopped, stats.idle, stats.rows);

    // the first identity: ceiling 32767 on a fresh record over sums inside -32767 .. 32767 returns them bit for bit, at every ramp
    for (int r = 0; r <= kLimitMaxRampLog2; ++r) {
        const LimitParams p = {32767, 64, 2, r};
        for (int n = 0; n < 160; ++n) {
            s[n] = n == 0 ? 32767 : n == 159 ? -32767 : (int32_t)(rnd() % 65535u) - 32767;
        }
        uint32_t g1, h1;
        check_row(s, p, kLimitUnity, 0, &g1, &h1, &stats);
        CHECK(g1 == (uint32_t)kLimitUnity && h1 == 0, "the identity leaves a fresh record fresh");
        const LimitRamp ramp = limit_ramp(false, kLimitUnity, kLimitUnity, 160);
        for (int n = 0; n < 160; ++n) {
            CHECK(limit_scaled(limit_clamped(s[n]), limit_gain_at(ramp, n, r)) == (int16_t)s[n], "bit for bit: %d", s[n]);
        }
    }
    // -32768 under the ceiling 32767 is one LSB too large: an attack to 32767, y = -32767
    {
        const LimitParams p = {32767, 255, 0, 0};
        memset(s, 0, sizeof(s));
        s[40] = -32768;
        uint32_t g1, h1;
        check_row(s, p, kLimitUnity, 0, &g1, &h1, &stats);
        CHECK(g1 == 32767u && limit_scaled(-32768, 32767) == -32767, "-32768 under 32767: gain %u", g1);
    }
}

void check_grid() {
    using namespace mbx;
    CHECK(limit_grid(0) == 0 && limit_grid(1) == 1 && limit_grid(16) == 1 && limit_grid(17) == 2 && limit_grid(65) == 5, "16 buses per workgroup");
    CHECK(limit_grid((size_t)INT32_MAX) == 134217728u, "the largest launch: 2^27 workgroups");
    CHECK(limit_state_bytes(0) == 0 && limit_state_bytes(5) == 20 && limit_records_room(0) == 16 && limit_records_room(4) == 16 && limit_records_room(5) == 32, "4 bytes per record");
    CHECK(limit_sums_bytes(3) == 1920 && limit_alloc_bytes(0) == 16 && limit_alloc_bytes(5) == 32 + 3200 && limit_records_room(7) % 16 == 0, "the scratch behind the records, 16-byte aligned");
    CHECK(kLimitLanes * kLimitSamples == 160 && kLimitBlock % 64 == 0 && 64 % kLimitLanes == 0, "the lane map");
}

}  // namespace

int main() {
    check_refusals();
    check_rows();
    check_grid();
    if (failures) {
        printf("limit_check: %d FAILED\n", failures);
        return 1;
    }
    printf("limit_check: ok (ramp_log2 up to %d, range 2^%d, ceilings %d .. %d)\n", mbx::kLimitMaxRampLog2, mbx::kLimitRangeLog2, mbx::kLimitMinCeiling, mbx::kLimitMaxCeiling);
    return 0;
}
