// agc_check.cpp -- host check of levelled rows (include/mbx_agc.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_agc_host.py; a program of its own, nothing of it is loaded anywhere else.
//   every refusal of mbelib-neo_amd/csrc/mbx_agc_plan.h: the parameters, the state, the shape of a call, a range of records, a record
//     -- pointers as numbers, never dereferenced;
//   the int32 / uint32 bounds of the header at the extreme parameters, every intermediate computed in 64 bits beside the 32-bit one;
//   the decision against the rule of the header written out in 64 bits, over a sweep of (p, g0, env0) and parameter sets;
//   g(n) and the scaled sample against a plain 64-bit restatement with a true floor division, over a sweep of (g0, g1, x, ramp_log2);
//   the three identities; the record as a word, the grid and the allocation.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mbx_agc_plan.h"

#include <mbx_agc.h>   // the public header (include/ is first on the include path)

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

static_assert(sizeof(mbx_agc) == 12 && offsetof(mbx_agc, target_peak) == 0 && offsetof(mbx_agc, floor_peak) == 2 && offsetof(mbx_agc, min_gain_q10) == 4
                  && offsetof(mbx_agc, max_gain_q10) == 6 && offsetof(mbx_agc, release_q8) == 8 && offsetof(mbx_agc, rise_q8) == 9
                  && offsetof(mbx_agc, ramp_log2) == 10 && offsetof(mbx_agc, zero) == 11,
              "the agc");
static_assert(sizeof(mbx_agc_record) == 4 && offsetof(mbx_agc_record, gain_q10) == 0 && offsetof(mbx_agc_record, env) == 2, "the state record");
static_assert(MBX_AGC_UNITY_Q10 == mbx::kAgcUnity && MBX_AGC_MAX_GAIN_Q10 == mbx::kAgcMaxGain && MBX_AGC_MAX_RAMP_LOG2 == mbx::kAgcMaxRampLog2
                  && MBX_AGC_MAX_RAMP_LOG2 == MBX_HOLD_MAX_RAMP_LOG2,
              "constants");

const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

long long floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// ---- refusals -------------------------------------------------------------------------------------------------------------------------
void check_refusals() {
    using namespace mbx;
    CHECK(agc_refused(true, 8000, 200, 512, 8192, 3, 0) == kAgcOk, "a good agc");
    CHECK(agc_refused(true, 1, 1, 1, 1, 0, 0) == kAgcOk && agc_refused(true, 32767, 32768, 32768, 32768, 7, 0) == kAgcOk, "the limits");
    CHECK(agc_refused(false, 8000, 200, 512, 8192, 3, 0) == kAgcNull, "no agc");
    CHECK(agc_refused(true, 0, 200, 512, 8192, 3, 0) == kAgcTarget && agc_refused(true, 32768, 200, 512, 8192, 3, 0) == kAgcTarget
              && agc_refused(true, 65535, 200, 512, 8192, 3, 0) == kAgcTarget,
          "target_peak outside 1 .. 32767");
    CHECK(agc_refused(true, 8000, 0, 512, 8192, 3, 0) == kAgcFloor && agc_refused(true, 8000, 32769, 512, 8192, 3, 0) == kAgcFloor, "floor_peak outside 1 .. 32768");
    CHECK(agc_refused(true, 8000, 200, 0, 8192, 3, 0) == kAgcGain && agc_refused(true, 8000, 200, 512, 32769, 3, 0) == kAgcGain
              && agc_refused(true, 8000, 200, 32769, 32769, 3, 0) == kAgcGain && agc_refused(true, 8000, 200, 0, 0, 3, 0) == kAgcGain,
          "a gain outside 1 .. 32768");
    CHECK(agc_refused(true, 8000, 200, 8193, 8192, 3, 0) == kAgcGainOrder && agc_refused(true, 8000, 200, 32768, 1, 3, 0) == kAgcGainOrder, "min above max");
    CHECK(agc_refused(true, 8000, 200, 512, 8192, 8, 0) == kAgcRamp && agc_refused(true, 8000, 200, 512, 8192, 255, 0) == kAgcRamp, "ramp_log2 8");
    CHECK(agc_refused(true, 8000, 200, 512, 8192, 3, 1) == kAgcZero && agc_refused(true, 8000, 200, 512, 8192, 7, 255) == kAgcZero, "zero is not 0");
    // their order: everything wrong at once, then one thing fewer each time
    CHECK(agc_refused(false, 0, 0, 0, 0, 8, 1) == kAgcNull && agc_refused(true, 0, 0, 0, 0, 8, 1) == kAgcTarget && agc_refused(true, 1, 0, 0, 0, 8, 1) == kAgcFloor
              && agc_refused(true, 1, 1, 0, 0, 8, 1) == kAgcGain && agc_refused(true, 1, 1, 2, 1, 8, 1) == kAgcGainOrder
              && agc_refused(true, 1, 1, 1, 1, 8, 1) == kAgcRamp && agc_refused(true, 1, 1, 1, 1, 7, 1) == kAgcZero,
          "the order of the refusals");

    // the shape of a call; rows at 0x10000 (8 rows = 2560 bytes), out at 0x20000
    CHECK(agc_rows_refused(4, 2, at(0x10000), at(0x20000), 16) == kAgcOk && agc_rows_refused(4, 2, at(0x10000), at(0x10000), 16) == kAgcOk, "apart, and in place");
    CHECK(agc_rows_refused(0, 0, at(0x10000), at(0x20000), 16) == kAgcOk && agc_rows_refused(0, 5, at(0x10000), at(0x10010), 16) == kAgcOk, "nothing to do");
    CHECK(agc_rows_refused(-1, 2, at(0x10000), at(0x20000), 16) == kAgcCounts && agc_rows_refused(4, -1, at(0x10000), at(0x20000), 16) == kAgcCounts, "negative counts");
    CHECK(agc_rows_refused(65536, 32768, at(0x10000), at(0x10000), 16) == kAgcRows && agc_rows_refused(INT32_MAX, 2, at(0x10000), at(0x10000), 16) == kAgcRows
              && agc_rows_refused(INT32_MAX, INT32_MAX, at(0x10000), at(0x10000), 16) == kAgcRows,
          "n * T above 2^31 - 1");
    CHECK(agc_rows_refused(INT32_MAX, 1, at(0x10000), at(0x10000), 16) == kAgcOk && agc_rows_refused(1, INT32_MAX, at(0x10000), at(0x10000), 16) == kAgcOk
              && agc_rows_refused(65536, 32767, at(0x10000), at(0x10000), 16) == kAgcOk,
          "n * T of 2^31 - 1 and below");
    CHECK(agc_rows_refused(4, 2, nullptr, at(0x20000), 16) == kAgcPointers && agc_rows_refused(4, 2, at(0x10000), nullptr, 16) == kAgcPointers, "NULL rows");
    for (uintptr_t o : {2u, 4u, 8u}) {
        CHECK(agc_rows_refused(4, 2, at(0x10000 + o), at(0x20000), 16) == kAgcAlign && agc_rows_refused(4, 2, at(0x10000), at(0x20000 + o), 16) == kAgcAlign
                  && agc_rows_refused(4, 2, at(0x10000 + o), at(0x10000 + o), 16) == kAgcAlign,
              "rows at %u", (unsigned)o);
        CHECK(agc_rows_refused(4, 2, at(0x10000 + o), at(0x20000 + o), 0) == kAgcOk, "the host definition asks no alignment");
    }
    CHECK(agc_rows_refused(4, 2, at(0x10000), at(0x10000 + 2560 - 16), 16) == kAgcOverlap && agc_rows_refused(4, 2, at(0x10000 + 320), at(0x10000), 16) == kAgcOverlap
              && agc_rows_refused(4, 2, at(0x10000), at(0x10000 + 16), 16) == kAgcOverlap,
          "a partial overlap");
    CHECK(agc_rows_refused(4, 2, at(0x10000), at(0x10000 + 2560), 16) == kAgcOk && agc_rows_refused(4, 2, at(0x10000 + 2560), at(0x10000), 16) == kAgcOk,
          "out right behind the rows, and right in front of them");

    // the launcher: the parameters, the state, the shape
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 3, 0, true, 4, 2, at(0x10000), at(0x20000)) == kAgcOk, "a good launch");
    CHECK(agc_launch_refused(false, 0, 0, 0, 0, 0, 0, false, -1, -1, nullptr, nullptr) == kAgcNull, "no agc comes first");
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 8, 0, false, -1, -1, nullptr, nullptr) == kAgcRamp, "then the fields");
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 3, 0, false, -1, -1, nullptr, nullptr) == kAgcNoState, "then the state");
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 3, 0, true, -1, -1, nullptr, nullptr) == kAgcCounts, "then the counts");
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 3, 0, true, 4, 2, nullptr, nullptr) == kAgcPointers, "then the pointers");
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 3, 0, true, 4, 2, at(0x10008), at(0x20000)) == kAgcAlign, "then the alignment");
    CHECK(agc_launch_refused(true, 8000, 200, 512, 8192, 3, 0, true, 4, 2, at(0x10000), at(0x10140)) == kAgcOverlap, "then the overlap");

    // a range of records
    CHECK(agc_range_refused(true, 16, 0, 16) == kAgcOk && agc_range_refused(true, 16, 16, 0) == kAgcOk && agc_range_refused(true, 0, 0, 0) == kAgcOk, "good ranges");
    CHECK(agc_range_refused(false, 16, 0, 16) == kAgcNoState, "no state");
    CHECK(agc_range_refused(true, 16, -1, 2) == kAgcRange && agc_range_refused(true, 16, 0, -1) == kAgcRange && agc_range_refused(true, 16, 1, 16) == kAgcRange
              && agc_range_refused(true, 16, 17, 0) == kAgcRange && agc_range_refused(true, 16, INT32_MAX, INT32_MAX) == kAgcRange,
          "ranges outside the records");

    // records
    const uint32_t good[4] = {agc_word(1024, 0), agc_word(1, 32768), agc_word(32768, 1), kAgcFreshWord};
    CHECK(agc_records_refused(good, 4) == kAgcOk && agc_records_refused(good, 0) == kAgcOk, "good records");
    for (const uint32_t bad : {agc_word(0, 0), agc_word(32769, 0), agc_word(65535, 65535), agc_word(1024, 32769), agc_word(1024, 65535)}) {
        uint32_t words[4];
        memcpy(words, good, sizeof(words));
        words[3] = bad;
        CHECK(agc_records_refused(words, 4) == kAgcRecord && agc_records_refused(words, 3) == kAgcOk && !agc_word_ok(bad), "record %08x", bad);
    }
    const mbx_agc_record rec = {0x1234, 0x0567};
    uint32_t word;
    memcpy(&word, &rec, 4);
    CHECK(word == agc_word(0x1234, 0x0567) && agc_word_gain(word) == 0x1234 && agc_word_env(word) == 0x0567, "the record's word");
    const mbx_agc_record fresh = {1024, 0};
    memcpy(&word, &fresh, 4);
    CHECK(word == kAgcFreshWord, "a fresh record");
    for (int r = kAgcNull; r < kAgcRefusals; ++r) {
        CHECK(agc_refusal_text((AgcRefusal)r)[0] != 0, "a refusal without a text: %d", r);
    }
}

// ---- the decision, and its bounds -------------------------------------------------------------------------------------------------------
void check_decision() {
    using namespace mbx;
    const AgcParams sets[] = {
        {8000, 200, 512, 8192, 64, 32, 3},      {32767, 1, 1, 32768, 255, 255, 7},     {1, 32768, 1, 32768, 0, 0, 0},   {32767, 32768, 32768, 32768, 255, 255, 7},
        {1, 1, 1, 1, 255, 255, 0},              {32767, 1, 32768, 32768, 255, 255, 7}, {8000, 200, 1024, 1024, 64, 0, 5}, {12000, 300, 256, 16384, 1, 1, 4},
    };
    const uint32_t peaks[] = {0, 1, 2, 199, 200, 201, 255, 256, 257, 999, 8000, 16384, 32766, 32767, 32768};
    const uint32_t gains[] = {1, 2, 255, 256, 511, 512, 1023, 1024, 1025, 8191, 8192, 32767, 32768};
    const uint32_t envs[] = {0, 1, 2, 200, 255, 256, 257, 1000, 8000, 32767, 32768};
    for (const AgcParams& a : sets) {
        for (uint32_t p : peaks) {
            for (uint32_t g0 : gains) {
                for (uint32_t env0 : envs) {
                    const AgcDecision d = agc_decide(p, g0, env0, a);
                    long long g1, env, want;
                    uint32_t event;
                    if ((long long)p < a.floor_peak) {   // the rule of the header, case by case, in 64 bits
                        g1 = g0, env = env0, want = g0, event = kAgcFreeze;
                    } else {
                        const long long term = ((long long)env0 * a.release_q8 + 255) >> 8;
                        CHECK(term <= (long long)env0 && (long long)env0 * a.release_q8 + 255 < (1ll << 24), "the decay term: env0 %u", env0);
                        const long long decayed = (long long)env0 - term;
                        env = (long long)p > decayed ? (long long)p : decayed;
                        CHECK(env >= 1 && ((long long)a.target_peak << 10) < (1ll << 25), "the division: env %lld", env);
                        want = ((long long)a.target_peak << 10) / env;
                        want = want < a.min_gain ? a.min_gain : want > a.max_gain ? a.max_gain : want;
                        if (want <= (long long)g0) {
                            g1 = want, event = want == (long long)g0 ? kAgcHold : kAgcFall;
                        } else {
                            const long long slewed = (long long)g0 + (((long long)g0 * a.rise_q8 + 255) >> 8);
                            CHECK((long long)g0 * a.rise_q8 + 255 < (1ll << 24), "the rise term: g0 %u", g0);
                            g1 = want < slewed ? want : slewed;
                            event = want <= slewed ? kAgcRiseReached : kAgcRiseSlewed;
                        }
                    }
                    CHECK((long long)d.gain == g1 && (long long)d.env == env && (long long)d.want == want && d.event == event,
                          "p %u g0 %u env0 %u under {%u, %u, %u, %u, %u, %u}: {%u, %u, %u, %u}, want {%lld, %lld, %lld, %u}", p, g0, env0, a.target_peak, a.floor_peak,
                          a.min_gain, a.max_gain, a.release_q8, a.rise_q8, d.gain, d.env, d.want, d.event, g1, env, want, event);
                    // a good record in, a good record out; the gain inside the clamp unless it is on its way there or frozen
                    CHECK(agc_word_ok(agc_word(d.gain, d.env)), "a decision is a good record: %u %u", d.gain, d.env);
                    if (a.rise_q8 == 0) {
                        CHECK(d.gain <= g0, "rise_q8 = 0 never raises a gain");
                    }
                    if (event != kAgcFreeze && g0 >= a.min_gain) {
                        CHECK(d.gain >= a.min_gain && (d.gain <= a.max_gain || d.gain <= g0), "the clamp");
                    }
                }
            }
        }
    }
    // the envelope reaches 0: the decay term is a ceiling
    {
        const AgcParams a = {8000, 1, 1, 32768, 1, 0, 0};
        uint32_t env = 32768;
        int frames = 0;
        while (env > 0 && frames < 100000) {
            env = env - ((env * a.release_q8 + 255u) >> 8);
            ++frames;
        }
        CHECK(env == 0 && frames <= 32768, "release_q8 = 1 reaches 0 (%d frames)", frames);
    }
}

// ---- g(n) and the scaled sample ---------------------------------------------------------------------------------------------------------
void check_arithmetic() {
    using namespace mbx;
    const int32_t gains[] = {1, 2, 3, 511, 512, 1023, 1024, 1025, 4097, 8192, 16383, 32767, 32768};
    const int32_t xs[] = {-32768, -32767, -16385, -1025, -1024, -513, -512, -511, -33, -32, -31, -2, -1, 0, 1, 2, 31, 32, 33, 511, 512, 513, 1023, 1024, 16384, 32766, 32767};
    for (int r = 0; r <= kAgcMaxRampLog2; ++r) {
        const long long R = 1ll << r;
        for (int32_t g0 : gains) {
            for (int32_t g1 : gains) {
                CHECK(((long long)g1 - g0) * R < (1ll << 22) && ((long long)g1 - g0) * R > -(1ll << 22), "|(g1 - g0) * R| < 2^22");
                for (int n = 0; n < 160; ++n) {
                    const long long up = n + 1 < R ? n + 1 : R;
                    const long long want = g0 + floor_div(((long long)g1 - g0) * up, R);
                    const int32_t g = agc_gain_at(g0, g1, n, r);
                    CHECK((long long)g == want, "g(%d) from %d to %d at ramp_log2 %d: %d, want %lld", n, g0, g1, r, g, want);
                    CHECK(g >= (g0 < g1 ? g0 : g1) && g <= (g0 < g1 ? g1 : g0) && g >= 1 && g <= kAgcMaxGain, "g(n) lies between g0 and g1: %d", g);
                    if (n >= R - 1) {
                        CHECK(g == g1, "g(n) = g1 from n = R - 1 on: n %d, ramp_log2 %d", n, r);
                    }
                    if (n == 0 || n == R - 2 || n == R - 1 || n == 159) {   // the samples at the ends of the ramp, under every gain it has there
                        for (int32_t x : xs) {
                            const long long wide = (long long)x * g + 512;
                            CHECK(wide < (1ll << 31) && wide >= -(1ll << 31), "x * g + 512 stays in int32: %d * %d", x, g);
                            const long long y = floor_div(wide, 1024);
                            const long long clamped = y < -32768 ? -32768 : y > 32767 ? 32767 : y;
                            CHECK((long long)agc_scaled((int16_t)x, g) == clamped, "x %d at gain %d: %d, want %lld", x, g, agc_scaled((int16_t)x, g), clamped);
                        }
                    }
                }
            }
        }
    }
    // the identities: unity returns the sample; a static gain is (x * G + 512) >> 10; the extremes
    for (int32_t x = -32768; x <= 32767; ++x) {
        CHECK(agc_scaled((int16_t)x, kAgcUnity) == (int16_t)x, "unity: %d", x);
        const long long top = floor_div((long long)x * 32768 + 512, 1024), low = floor_div((long long)x + 512, 1024);
        CHECK((long long)agc_scaled((int16_t)x, 32768) == (top < -32768 ? -32768 : top > 32767 ? 32767 : top), "x 32: %d", x);
        CHECK((long long)agc_scaled((int16_t)x, 1) == low, "x 1/1024: %d", x);
    }
    CHECK(agc_scaled(-32768, 32768) == -32768 && agc_scaled(32767, 32768) == 32767 && agc_scaled(-32768, 1) == -32 && agc_scaled(32767, 1) == 32, "the corners");
    CHECK(agc_scaled(1023, 32768) == 32736 && agc_scaled(1024, 32768) == 32767 && agc_scaled(-1024, 32768) == -32768 && agc_scaled(-1025, 32768) == -32768, "where x 32 clips");
}

void check_grid() {
    using namespace mbx;
    CHECK(agc_grid(0) == 0 && agc_grid(1) == 1 && agc_grid(16) == 1 && agc_grid(17) == 2 && agc_grid(67) == 5, "16 entries per workgroup");
    CHECK(agc_grid((size_t)INT32_MAX) == 134217728u, "the largest launch: 2^27 workgroups");
    CHECK(agc_state_bytes(0) == 0 && agc_state_bytes(5) == 20 && agc_alloc_bytes(0) == 16 && agc_alloc_bytes(4) == 16 && agc_alloc_bytes(5) == 32, "4 bytes per record");
    CHECK(kAgcLanes * kAgcSamples == 160 && kAgcBlock % 64 == 0 && 64 % kAgcLanes == 0, "the lane map");
}

}  // namespace

int main() {
    check_refusals();
    check_decision();
    check_arithmetic();
    check_grid();
    if (failures) {
        printf("agc_check: %d FAILED\n", failures);
        return 1;
    }
    printf("agc_check: ok (ramp_log2 up to %d, gains up to %d)\n", mbx::kAgcMaxRampLog2, mbx::kAgcMaxGain);
    return 0;
}
