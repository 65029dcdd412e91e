// resample_check.cpp -- host check of wide rows (include/mbx_resample.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_resample_host.py; a program of its own, nothing of it is loaded anywhere else.
//   every refusal of mbelib-neo_amd/csrc/mbx_resample_plan.h and their order: the filter, the state, the shape of a call, a range of
//     records -- the pointers of a call as numbers, never dereferenced;
//   the phase bound at its edge: 65535 accepted, 65536 refused, and acc at +-32768 inputs inside int32, every partial sum computed in
//     64 bits beside the 32-bit one;
//   the packing of the taps; resample_sample against the rule of the header written out in 64 bits with a true floor division;
//   the four identities; records at the int16 extremes; the grid, the allocation and the sizes.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mbx_resample_plan.h"

#include <mbx_resample.h>   // the public header (include/ is first on the include path)

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

static_assert(sizeof(mbx_resample) == 388 && offsetof(mbx_resample, L) == 0 && offsetof(mbx_resample, K) == 1 && offsetof(mbx_resample, zero) == 2
                  && offsetof(mbx_resample, taps) == 4,
              "the resampler");
static_assert(sizeof(mbx_resample_record) == 64, "the state record");
static_assert(MBX_RESAMPLE_MAX_TAPS == mbx::kResampleMaxTaps && MBX_RESAMPLE_UNITY_Q14 == mbx::kResampleUnity && MBX_RESAMPLE_HISTORY == mbx::kResampleHistory
                  && MBX_RESAMPLE_MAX_TAPS == mbx::kResampleMaxK * mbx::kResampleMaxL,
              "constants");
// the bound of the header
static_assert(65535ll * 32768ll == 2147450880ll && 65535ll * 32768ll + 8192ll < (1ll << 31), "acc + 8192 fits int32");

const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

long long floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

uint32_t lcg = 12345u;
int16_t rnd16() {
    lcg = lcg * 1664525u + 1013904223u;
    return (int16_t)(lcg >> 16);
}

// the rule of the header in 64 bits: y[n*L+p] from x_ext, `at` pointing at x_ext[n]
long long rule(const int16_t* taps, int L, int K, int p, const int16_t* x, long long* acc_out) {
    long long acc = 0;
    for (int k = 0; k < K; ++k) {
        acc += (long long)taps[p + k * L] * (long long)x[-k];
    }
    if (acc_out) {
        *acc_out = acc;
    }
    const long long y = floor_div(acc + 8192, 16384);
    return y < -32768 ? -32768 : y > 32767 ? 32767 : y;
}

// ---- refusals -------------------------------------------------------------------------------------------------------------------------
void check_refusals() {
    using namespace mbx;
    int16_t taps[kResampleMaxTaps] = {};
    taps[0] = taps[1] = 16384;
    CHECK(resample_refused(true, 2, 2, 0, taps) == kResampleOk, "a good filter");
    CHECK(resample_refused(false, 2, 2, 0, nullptr) == kResampleNull, "no filter");
    for (unsigned L : {0u, 1u, 5u, 7u, 8u, 255u}) {
        CHECK(resample_refused(true, L, 2, 0, taps) == kResampleL, "L %u", L);
    }
    for (unsigned L : {2u, 3u, 4u, 6u}) {
        CHECK(resample_refused(true, L, 2, 0, taps) == kResampleOk && resample_refused(true, L, 32, 0, taps) == kResampleOk, "L %u", L);
    }
    for (unsigned K : {0u, 1u, 3u, 31u, 33u, 34u, 255u}) {
        CHECK(resample_refused(true, 2, K, 0, taps) == kResampleK, "K %u", K);
    }
    CHECK(resample_refused(true, 2, 2, 1, taps) == kResampleZero && resample_refused(true, 2, 2, 255, taps) == kResampleZero, "zero bytes");
    // a nonzero tap beyond K * L: the first one behind, and the very last
    for (int where : {4, 5, kResampleMaxTaps - 1}) {
        int16_t t2[kResampleMaxTaps];
        memcpy(t2, taps, sizeof(t2));
        t2[where] = -1;
        CHECK(resample_refused(true, 2, 2, 0, t2) == kResampleBeyond, "a tap at %d with K * L = 4", where);
        CHECK(resample_refused(true, 6, 32, 0, t2) == kResampleOk, "K * L = 192 has nothing beyond");
    }
    // the phase bound at its edge: 32767 + 32767 + 1 = 65535 is accepted, one more is refused; negative taps count by magnitude
    for (unsigned L : {2u, 3u, 4u, 6u}) {
        for (unsigned p = 0; p < L; ++p) {
            int16_t t3[kResampleMaxTaps] = {};
            t3[p] = 32767, t3[p + L] = -32767, t3[p + 2 * L] = 1;
            CHECK(resample_phase_sum(t3, (int)L, 4) == 65535 && resample_refused(true, L, 4, 0, t3) == kResampleOk, "a phase of 65535: L %u p %u", L, p);
            t3[p + 3 * L] = -1;
            CHECK(resample_phase_sum(t3, (int)L, 4) == 65536 && resample_refused(true, L, 4, 0, t3) == kResamplePhase, "a phase of 65536: L %u p %u", L, p);
            t3[p + 3 * L] = 0, t3[p] = -32768;
            CHECK(resample_phase_sum(t3, (int)L, 4) == 65536 && resample_refused(true, L, 4, 0, t3) == kResamplePhase, "-32768 counts 32768: L %u p %u", L, p);
        }
    }
    // their order: everything wrong at once, then one thing fewer each time
    int16_t bad[kResampleMaxTaps];
    for (int i = 0; i < kResampleMaxTaps; ++i) {
        bad[i] = 32767;
    }
    CHECK(resample_refused(false, 5, 3, 1, bad) == kResampleNull && resample_refused(true, 5, 3, 1, bad) == kResampleL && resample_refused(true, 2, 3, 1, bad) == kResampleK
              && resample_refused(true, 2, 4, 1, bad) == kResampleZero && resample_refused(true, 2, 4, 0, bad) == kResampleBeyond,
          "the order of the refusals");
    memset(bad + 8, 0, sizeof(bad) - 16);
    CHECK(resample_refused(true, 2, 4, 0, bad) == kResamplePhase, "then the phase bound");

    // the shape of a call; 8 rows in = 2560 bytes at 0x10000, out at 0x20000 (L times as many)
    CHECK(resample_rows_refused(4, 2, 6, at(0x10000), at(0x20000), 16) == kResampleOk, "apart");
    CHECK(resample_rows_refused(0, 0, 6, at(0x10000), at(0x10000), 16) == kResampleOk && resample_rows_refused(0, 5, 2, at(0x10000), at(0x10010), 16) == kResampleOk,
          "nothing to do overlaps nothing");
    CHECK(resample_rows_refused(-1, 2, 2, at(0x10000), at(0x20000), 16) == kResampleCounts && resample_rows_refused(4, -1, 2, at(0x10000), at(0x20000), 16) == kResampleCounts,
          "negative counts");
    // n * T * 160 * L against 2^31 - 1: at L = 2 the largest n * T is 6710886
    CHECK(resample_rows_refused(6710886, 1, 2, at(0x10000), at(0x100000000000), 16) == kResampleOk, "6710886 * 320 = 2147483520");
    CHECK(resample_rows_refused(6710887, 1, 2, at(0x10000), at(0x100000000000), 16) == kResampleSize && resample_rows_refused(2236963, 1, 6, at(0x10000), at(0x100000000000), 16) == kResampleSize
              && resample_rows_refused(2236962, 1, 6, at(0x10000), at(0x100000000000), 16) == kResampleOk,
          "one row more");
    CHECK(resample_rows_refused(INT32_MAX, INT32_MAX, 6, at(0x10000), at(0x20000), 16) == kResampleSize && resample_rows_refused(65536, 32768, 2, at(0x10000), at(0x20000), 16) == kResampleSize,
          "far beyond");
    CHECK(resample_rows_refused(4, 2, 2, nullptr, at(0x20000), 16) == kResamplePointers && resample_rows_refused(4, 2, 2, at(0x10000), nullptr, 16) == kResamplePointers, "NULL rows");
    for (uintptr_t o : {2u, 4u, 8u}) {
        CHECK(resample_rows_refused(4, 2, 2, at(0x10000 + o), at(0x20000), 16) == kResampleAlign && resample_rows_refused(4, 2, 2, at(0x10000), at(0x20000 + o), 16) == kResampleAlign,
              "rows at %u", (unsigned)o);
        CHECK(resample_rows_refused(4, 2, 2, at(0x10000 + o), at(0x20000 + o), 0) == kResampleOk, "the host definition asks no alignment");
    }
    // ANY overlap: the same array, out inside in, in inside out, by one 16
    CHECK(resample_rows_refused(4, 2, 2, at(0x10000), at(0x10000), 16) == kResampleOverlap, "in place");
    CHECK(resample_rows_refused(4, 2, 2, at(0x10000), at(0x10000 + 2560 - 16), 16) == kResampleOverlap, "out begins in the last 16 of in");
    CHECK(resample_rows_refused(4, 2, 2, at(0x10000 + 5120 - 16), at(0x10000), 16) == kResampleOverlap, "in begins in the last 16 of out");
    CHECK(resample_rows_refused(4, 2, 2, at(0x10000), at(0x10000 + 2560), 16) == kResampleOk && resample_rows_refused(4, 2, 2, at(0x10000 + 5120), at(0x10000), 16) == kResampleOk,
          "out right behind the rows, and right in front of them");
    CHECK(resample_rows_refused(4, 2, 6, at(0x10000 + 15360 - 16), at(0x10000), 16) == kResampleOverlap && resample_rows_refused(4, 2, 6, at(0x10000 + 15360), at(0x10000), 16) == kResampleOk,
          "out is L times the rows");

    // the launcher: the filter, the state, the shape
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, true, 4, 2, at(0x10000), at(0x20000)) == kResampleOk, "a good launch");
    CHECK(resample_launch_refused(false, 0, 0, 0, nullptr, false, -1, -1, nullptr, nullptr) == kResampleNull, "no filter comes first");
    CHECK(resample_launch_refused(true, 2, 3, 0, taps, false, -1, -1, nullptr, nullptr) == kResampleK, "then the fields");
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, false, -1, -1, nullptr, nullptr) == kResampleNoState, "then the state");
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, true, -1, -1, nullptr, nullptr) == kResampleCounts, "then the counts");
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, true, 65536, 32768, nullptr, nullptr) == kResampleSize, "then the size");
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, true, 4, 2, nullptr, nullptr) == kResamplePointers, "then the pointers");
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, true, 4, 2, at(0x10008), at(0x10000)) == kResampleAlign, "then the alignment");
    CHECK(resample_launch_refused(true, 2, 2, 0, taps, true, 4, 2, at(0x10000), at(0x10140)) == kResampleOverlap, "then the overlap");

    // a range of records
    CHECK(resample_range_refused(true, 16, 0, 16) == kResampleOk && resample_range_refused(true, 16, 16, 0) == kResampleOk && resample_range_refused(true, 0, 0, 0) == kResampleOk,
          "good ranges");
    CHECK(resample_range_refused(false, 16, 0, 16) == kResampleNoState, "no state");
    CHECK(resample_range_refused(true, 16, -1, 2) == kResampleRange && resample_range_refused(true, 16, 0, -1) == kResampleRange && resample_range_refused(true, 16, 1, 16) == kResampleRange
              && resample_range_refused(true, 16, 17, 0) == kResampleRange && resample_range_refused(true, 16, INT32_MAX, INT32_MAX) == kResampleRange,
          "ranges outside the records");
    for (int r = kResampleNull; r < kResampleRefusals; ++r) {
        CHECK(resample_refusal_text((ResampleRefusal)r)[0] != 0, "a refusal without a text: %d", r);
    }
}

// ---- the packing ------------------------------------------------------------------------------------------------------------------------
void check_packing() {
    using namespace mbx;
    CHECK(resample_pair(0x1234, (int16_t)0xFEDC) == 0x1234FEDCu && resample_pair(-1, 0) == 0xFFFF0000u && resample_pair(0, -1) == 0x0000FFFFu,
          "the older sample's tap is the low half");
    for (int L : {2, 3, 4, 6}) {
        for (int K : {2, 4, 16, 32}) {
            int16_t taps[kResampleMaxTaps] = {};
            for (int i = 0; i < K * L; ++i) {
                taps[i] = (int16_t)(i * 257 - 20000);
            }
            const ResampleTaps f = resample_pack(taps, L, K);
            CHECK(f.half == K / 2, "half of %d", K);
            for (int kk = 0; kk < kResamplePairs / L; ++kk) {
                for (int p = 0; p < L; ++p) {
                    const uint32_t got = f.pair[kk * L + p];
                    const uint32_t want = kk < K / 2 ? ((uint32_t)(uint16_t)taps[p + (2 * kk + 1) * L] | ((uint32_t)(uint16_t)taps[p + 2 * kk * L] << 16)) : 0u;
                    CHECK(got == want, "pair (%d, %d) at L %d K %d: %08x, want %08x", kk, p, L, K, got, want);
                }
            }
        }
    }
    // the dot product of two pairs, both halves signed, at the corners
    CHECK(resample_dot2(0x80008000u, 0x7FFF7FFFu, 0) == 2 * (-32768 * 32767) && resample_dot2(0x80008000u, 0x80008000u, -1) == 2147483647, "the corners of a pair");
    CHECK(resample_dot2(0x0001FFFFu, 0x00020003u, 10) == 10 + 2 - 3, "lo * lo + hi * hi + acc");
    CHECK(resample_rounded(0) == 0 && resample_rounded(8191) == 0 && resample_rounded(8192) == 1 && resample_rounded(-8192) == 0 && resample_rounded(-8193) == -1
              && resample_rounded(2147450880) == 32767 && resample_rounded(-2147450880) == -32768 && resample_rounded(32767 * 16384 + 8191) == 32767
              && resample_rounded(-32768 * 16384 - 8192) == -32768 && resample_rounded(-32768 * 16384 + 8191) == -32768 && resample_rounded(-32768 * 16384 + 8192) == -32767,
          "the rounding floors, the clamp holds the rails");
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
void check_arithmetic() {
    using namespace mbx;
    int16_t x[kResampleHistory + 160];
    // random filters inside the bound and random full-scale windows, against the 64-bit rule
    for (int L : {2, 3, 4, 6}) {
        for (int K : {2, 4, 6, 16, 30, 32}) {
            int16_t taps[kResampleMaxTaps] = {};
            for (int i = 0; i < K * L; ++i) {
                taps[i] = (int16_t)(rnd16() / (K / 2));   // a phase sums to at most K * 32768 / (K / 2) = 65536 in magnitude ...
            }
            while (resample_phase_sum(taps, L, K) > kResamplePhaseBound) {   // ... and is brought inside where it is not
                for (int i = 0; i < K * L; ++i) {
                    taps[i] = (int16_t)(taps[i] - taps[i] / 64);
                }
            }
            CHECK(resample_refused(true, (unsigned)L, (unsigned)K, 0, taps) == kResampleOk, "a random filter: L %d K %d", L, K);
            const ResampleTaps f = resample_pack(taps, L, K);
            for (int round = 0; round < 4; ++round) {
                for (int i = 0; i < kResampleHistory + 160; ++i) {
                    x[i] = round == 0 ? rnd16() : round == 1 ? (int16_t)-32768 : round == 2 ? (int16_t)32767 : (int16_t)(rnd16() < 0 ? -32768 : 32767);
                }
                for (int n = 0; n < 160; ++n) {
                    for (int p = 0; p < L; ++p) {
                        long long acc = 0;
                        const long long want = rule(taps, L, K, p, x + kResampleHistory + n, &acc);
                        CHECK(acc <= 2147450880ll && acc >= -2147450880ll && acc + 8192 < (1ll << 31), "acc stays in int32: %lld", acc);
                        const int16_t got = resample_sample(f, L, p, x + kResampleHistory + n);
                        CHECK((long long)got == want, "y[%d * %d + %d] at K %d: %d, want %lld", n, L, p, K, got, want);
                    }
                }
            }
        }
    }
    // the corner of the bound: a phase of 32767 + 32767 + 1 against -32768 throughout, and the sign that maximises every product
    for (int L : {2, 6}) {
        int16_t taps[kResampleMaxTaps] = {};
        for (int p = 0; p < L; ++p) {
            taps[p] = 32767, taps[p + L] = -32767, taps[p + 2 * L] = 1;
        }
        const ResampleTaps f = resample_pack(taps, L, 4);
        for (int i = 0; i < kResampleHistory + 160; ++i) {
            x[i] = -32768;
        }
        // (32767 is the largest sample, so the largest |acc| has every sample at -32768 under taps of one sign)
        int16_t same[kResampleMaxTaps] = {};
        for (int p = 0; p < L; ++p) {
            same[p] = 32767, same[p + L] = 32767, same[p + 2 * L] = 1;
        }
        const ResampleTaps g = resample_pack(same, L, 4);
        long long acc = 0;
        CHECK(rule(same, L, 4, 0, x + kResampleHistory + 5, &acc) == -32768 && acc == -2147450880ll, "the corner: %lld", acc);
        CHECK(resample_sample(g, L, L - 1, x + kResampleHistory + 5) == -32768 && resample_sample(g, L, 0, x + kResampleHistory) == -32768, "the corner clamps low");
        CHECK(resample_sample(f, L, 0, x + kResampleHistory + 5) == (int16_t)rule(taps, L, 4, 0, x + kResampleHistory + 5, nullptr), "mixed signs at the rails");
        for (int i = 0; i < kResampleHistory + 160; ++i) {
            x[i] = 32767;
        }
        CHECK(resample_sample(g, L, 0, x + kResampleHistory + 5) == 32767, "and high");
    }
}

// ---- the identities, through the definition as the host twin runs it --------------------------------------------------------------------
// one entry of T frames over `hist`; out: T * 160 * L; hist is updated
void run(const int16_t* taps, int L, int K, int T, int16_t* hist, const int16_t* in, int16_t* out) {
    const mbx::ResampleTaps f = mbx::resample_pack(taps, L, K);
    int16_t x[mbx::kResampleHistory + 160];
    memcpy(x + 160, hist, 64);
    for (int t = 0; t < T; ++t) {
        memcpy(x, x + 160, 64);
        memcpy(x + mbx::kResampleHistory, in + t * 160, 320);
        for (int n = 0; n < 160; ++n) {
            for (int p = 0; p < L; ++p) {
                out[(t * 160 + n) * L + p] = mbx::resample_sample(f, L, p, x + mbx::kResampleHistory + n);
            }
        }
    }
    if (T > 0) {
        memcpy(hist, x + 160, 64);
    }
}

void check_identities() {
    using namespace mbx;
    static int16_t in[3 * 160], out3[3 * 160 * 6], out1[3 * 160 * 6];
    for (int L : {2, 3, 4, 6}) {
        for (int K : {2, 16, 32}) {
            for (int i = 0; i < 3 * 160; ++i) {
                in[i] = rnd16();
            }
            in[0] = -32768, in[159] = 32767, in[160] = 32767, in[479] = -32768;
            int16_t hist[kResampleHistory], start[kResampleHistory];
            for (int i = 0; i < kResampleHistory; ++i) {   // records at the int16 extremes
                start[i] = (i & 1) ? (int16_t)32767 : (int16_t)-32768;
            }
            // HOLD
            int16_t taps[kResampleMaxTaps] = {};
            for (int p = 0; p < L; ++p) {
                taps[p] = 16384;
            }
            memcpy(hist, start, 64);
            run(taps, L, K, 3, hist, in, out3);
            for (int m = 0; m < 480; ++m) {
                for (int p = 0; p < L; ++p) {
                    CHECK(out3[m * L + p] == in[m], "hold: L %d K %d sample %d phase %d", L, K, m, p);
                }
            }
            CHECK(memcmp(hist, in + 480 - 32, 64) == 0, "the record is the last 32 input samples");
            // DELAY, and BATCHING: one call of T = 3 is three of T = 1
            memset(taps, 0, sizeof(taps));
            for (int p = 0; p < L; ++p) {
                taps[p + (K - 1) * L] = 16384;
            }
            memcpy(hist, start, 64);
            run(taps, L, K, 3, hist, in, out3);
            for (int m = 0; m < 480; ++m) {
                const int from = m - (K - 1);
                const int16_t want = from >= 0 ? in[from] : start[kResampleHistory + from];
                for (int p = 0; p < L; ++p) {
                    CHECK(out3[m * L + p] == want, "delay: L %d K %d sample %d phase %d: %d, want %d", L, K, m, p, out3[m * L + p], want);
                }
            }
            int16_t hist1[kResampleHistory];
            memcpy(hist1, start, 64);
            for (int t = 0; t < 3; ++t) {
                run(taps, L, K, 1, hist1, in + t * 160, out1 + t * 160 * L);
            }
            CHECK(memcmp(out1, out3, sizeof(int16_t) * 480 * L) == 0 && memcmp(hist, hist1, 64) == 0, "three calls of one frame: L %d K %d", L, K);
            // DC: every phase sums to exactly 16384, signs mixed
            memset(taps, 0, sizeof(taps));
            for (int p = 0; p < L; ++p) {
                int sum = 0;
                for (int k = 1; k < K; ++k) {
                    taps[p + k * L] = (int16_t)(rnd16() / (2 * K));
                    sum += taps[p + k * L];
                }
                taps[p] = (int16_t)(16384 - sum);
            }
            CHECK(resample_refused(true, (unsigned)L, (unsigned)K, 0, taps) == kResampleOk, "the DC filter");
            for (int16_t c : {(int16_t)-32768, (int16_t)-1, (int16_t)0, (int16_t)1, (int16_t)12345, (int16_t)32767}) {
                for (int i = 0; i < 160; ++i) {
                    in[i] = c;
                }
                for (int i = 0; i < kResampleHistory; ++i) {
                    hist[i] = c;
                }
                run(taps, L, K, 1, hist, in, out1);
                bool same = true;
                for (int i = 0; i < 160 * L; ++i) {
                    same = same && out1[i] == c;
                }
                CHECK(same, "dc: L %d K %d constant %d", L, K, c);
            }
        }
    }
}

void check_grid() {
    using namespace mbx;
    CHECK(resample_grid(0) == 0 && resample_grid(1) == 1 && resample_grid(16) == 1 && resample_grid(17) == 2 && resample_grid(67) == 5, "16 rows per workgroup");
    CHECK(resample_grid(6710886) == 419431u, "the largest launch");
    CHECK(resample_state_bytes(0) == 0 && resample_state_bytes(5) == 320 && resample_alloc_bytes(0) == 64 && resample_alloc_bytes(5) == 320, "64 bytes per record");
    CHECK(resample_wide_bytes(5, 6) == 9600 && resample_wide_bytes(8192, 6) == 15728640u && resample_wide_bytes(0, 2) == 0, "rows * 160 * L * 2");
    CHECK(resample_wide_bytes(8192, 6) < (size_t)65536 * 320, "8,192 buses at 48 kHz are fewer bytes than 65,536 int16 rows");
    CHECK(kResampleLanes * kResampleSamples == 160 && kResampleBlock % 64 == 0 && 64 % kResampleLanes == 0 && kResampleWindowWords == 96, "the lane map");
    CHECK(sizeof(ResampleTaps) == 388, "the filter by value: 388 bytes of kernel arguments");
}

}  // namespace

int main() {
    check_refusals();
    check_packing();
    check_arithmetic();
    check_identities();
    check_grid();
    if (failures) {
        printf("resample_check: %d FAILED\n", failures);
        return 1;
    }
    printf("resample_check: ok (taps up to %d, phase sums up to %d)\n", mbx::kResampleMaxTaps, mbx::kResamplePhaseBound);
    return 0;
}
