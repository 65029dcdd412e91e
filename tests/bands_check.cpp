// bands_check.cpp -- host check of band records (include/mbx_bands.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_bands_host.py; a program of its own, nothing of it is loaded anywhere else.
//   the record arithmetic the kernel and the host function share (mbelib-neo_amd/csrc/mbx_bands_plan.h) held to __int128: a vector at
//     exactly the bound against rows of -32768 (re = +-2,147,450,880, the power form 4,294,836,225), random rows and banks at the bound,
//     and the kernel's partition walked as a wave walks it -- 16 lanes per row, ten samples each, the interleaved image, four xor steps,
//     wrapping adds -- with every partial sum inside int32;
//   the bound: a vector at 65535 passes, one at 65536 is refused with its probe and c or s named;
//   every refusal of mbx_band_bank_create, mbx_pcm_bands and mbx_pcm_bands_host in its order: pointers as numbers, never dereferenced;
//   the byte counts: bands_out_bytes, the grid, and band_bytes of the sessions (mbx_session_plan.h).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mbx_bands_plan.h"
#include "mbx_session_plan.h"   // (band_bytes)

#include <mbx_bands.h>

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

static_assert(sizeof(mbx_band_record) == 8 && offsetof(mbx_band_record, re) == 0 && offsetof(mbx_band_record, im) == 4, "the record");
static_assert(MBX_BANDS_MAX_PROBES == mbx::kBandsMaxProbes && MBX_BANDS_VECTOR_BOUND == mbx::kBandsVectorBound && MBX_BANDS_COMPLEX == mbx::kBandsComplex
                  && MBX_BANDS_POWER == mbx::kBandsPower,
              "constants");
static_assert(mbx::kBandsLanes * mbx::kBandsSamples == 160 && mbx::kBandsSamples % 2 == 0, "a lane's share is whole dwords");
static_assert(mbx::kBandsBlock == 256 && mbx::kBandsBlockRows == 16 && mbx::kBandsProbeBytes == 640, "the partition");

typedef __int128 wide;

uint32_t rng_state = 97531u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

wide naive_sum(const int16_t* x, const int16_t* v) {
    wide acc = 0;
    for (int n = 0; n < 160; ++n) {
        acc += (wide)x[n] * (wide)v[n];
    }
    return acc;
}
uint64_t naive_power(wide re, wide im) { return (uint64_t)((re * re + im * im) >> 31); }

// a vector whose |v[n]| sum to exactly `total`, places at random; signs at random, or every sign that of align_to[n], so that the sum peaks
void vector_of(int16_t* v, uint32_t total, const int16_t* align_to) {
    memset(v, 0, 160 * sizeof(int16_t));
    uint32_t left = total;
    while (left > 0) {
        const int      n = (int)(rnd() % 160u);
        const uint32_t room = 32767u - (uint32_t)(v[n] < 0 ? -v[n] : v[n]);
        uint32_t       add = 1u + rnd() % 2048u;
        add = add > left ? left : add;
        add = add > room ? room : add;
        const bool neg = align_to ? align_to[n] < 0 : (rnd() & 1u) != 0u;
        const int  mag = (v[n] < 0 ? -v[n] : v[n]) + (int)add;
        v[n] = (int16_t)((v[n] < 0 || (v[n] == 0 && neg)) ? -mag : mag);
        left -= add;
    }
}

// pcm_bands_kernel's walk of one row against one probe's interleaved image: 16 lanes, lane j the dwords 5 j .. 5 j + 4; xor steps 1, 2,
// 4, 8 with the wrapping adds of the device; every lane ends with the total
void wave_walk(const int16_t* x, const uint32_t* image, int32_t* re_out, int32_t* im_out) {
    uint32_t re[mbx::kBandsLanes], im[mbx::kBandsLanes];
    for (int j = 0; j < mbx::kBandsLanes; ++j) {
        int32_t r = 0, i = 0;
        for (int d = 0; d < mbx::kBandsSamples / 2; ++d) {
            const int      n = j * mbx::kBandsSamples + 2 * d;
            const uint32_t w = (uint32_t)(uint16_t)x[n] | ((uint32_t)(uint16_t)x[n + 1] << 16);
            r = mbx::bands_dot2(w, image[2 * (j * 5 + d)], r);
            i = mbx::bands_dot2(w, image[2 * (j * 5 + d) + 1], i);
        }
        re[j] = (uint32_t)r, im[j] = (uint32_t)i;
    }
    for (int m = 1; m < mbx::kBandsLanes; m <<= 1) {
        uint32_t nr[mbx::kBandsLanes], ni[mbx::kBandsLanes];
        for (int j = 0; j < mbx::kBandsLanes; ++j) {
            nr[j] = re[j] + re[j ^ m], ni[j] = im[j] + im[j ^ m];
        }
        memcpy(re, nr, sizeof(re)), memcpy(im, ni, sizeof(im));
    }
    for (int j = 1; j < mbx::kBandsLanes; ++j) {
        CHECK(re[j] == re[0] && im[j] == im[0], "lane %d holds another total than lane 0", j);
    }
    *re_out = (int32_t)re[0], *im_out = (int32_t)im[0];
}

void check_record(const int16_t* x, const int16_t* probe, const char* what) {
    const wide re = naive_sum(x, probe), im = naive_sum(x, probe + 160);
    const int32_t got_re = mbx::bands_sum(x, probe), got_im = mbx::bands_sum(x, probe + 160);
    CHECK((wide)got_re == re && (wide)got_im == im, "%s: re %d im %d", what, got_re, got_im);
    CHECK((uint64_t)mbx::bands_power(got_re, got_im) == naive_power(re, im), "%s: power %u", what, mbx::bands_power(got_re, got_im));
    CHECK(naive_power(re, im) <= 4294836225ull, "%s: the power form leaves its bound", what);
    uint32_t image[mbx::kBandsProbeWords];
    mbx::bands_interleave(probe, image);
    int32_t walk_re = 0, walk_im = 0;
    wave_walk(x, image, &walk_re, &walk_im);
    CHECK(walk_re == got_re && walk_im == got_im, "%s: the wave's walk gives %d %d, the definition %d %d", what, walk_re, walk_im, got_re, got_im);
}

void check_arithmetic() {
    int16_t x[160], probe[320];
    // a vector at exactly the bound against rows of -32768: 65535 is 2 x 32767 + 1
    for (int sign = -1; sign <= 1; sign += 2) {
        for (int n = 0; n < 160; ++n) {
            x[n] = -32768;
        }
        memset(probe, 0, sizeof(probe));
        probe[0] = (int16_t)(sign * 32767), probe[77] = (int16_t)(sign * 32767), probe[159] = (int16_t)sign;
        probe[160 + 3] = (int16_t)(-sign * 32767), probe[160 + 4] = (int16_t)(-sign * 32767), probe[160 + 158] = (int16_t)-sign;
        CHECK(mbx::bands_vector_sum(probe) == 65535u && mbx::bands_vector_sum(probe + 160) == 65535u, "the vectors are at the bound");
        CHECK(mbx::bands_sum(x, probe) == -sign * 2147450880 && mbx::bands_sum(x, probe + 160) == sign * 2147450880, "re %d", mbx::bands_sum(x, probe));
        CHECK(mbx::bands_power(mbx::bands_sum(x, probe), mbx::bands_sum(x, probe + 160)) == 4294836225u, "power %u",
              mbx::bands_power(mbx::bands_sum(x, probe), mbx::bands_sum(x, probe + 160)));
        check_record(x, probe, "the rail row");
        // one vector alone at the bound: the power is half of it, rounded down
        memset(probe + 160, 0, 160 * sizeof(int16_t));
        CHECK(mbx::bands_power(mbx::bands_sum(x, probe), 0) == (uint32_t)(((unsigned __int128)2147450880ull * 2147450880ull) >> 31), "one vector");
        check_record(x, probe, "the rail row, one vector");
    }
    // a probe of zeros, an impulse
    memset(probe, 0, sizeof(probe));
    for (int n = 0; n < 160; ++n) {
        x[n] = (int16_t)((int)(rnd() % 65536u) - 32768);
    }
    CHECK(mbx::bands_sum(x, probe) == 0 && mbx::bands_power(0, 0) == 0u, "ZERO");
    for (int m = 0; m < 160; m += 53) {
        memset(probe, 0, sizeof(probe));
        probe[m] = 16384;
        CHECK(mbx::bands_sum(x, probe) == 16384 * (int32_t)x[m] && mbx::bands_sum(x, probe + 160) == 0, "IMPULSE at %d", m);
        check_record(x, probe, "an impulse");
    }
    // random rows of every loudness, rails among them, against vectors at exactly the bound: random signs, and signs aligned with the row
    for (int round = 0; round < 400; ++round) {
        const int scale = 1 + (int)(rnd() % 5u) * 8191;
        for (int n = 0; n < 160; ++n) {
            const int v = ((int)(rnd() % 65536u) - 32768) * scale / 32768;
            x[n] = (int16_t)(round % 7 == 0 ? ((rnd() & 1u) ? 32767 : -32768) : v);
        }
        vector_of(probe, 65535u, round & 1 ? x : nullptr);
        vector_of(probe + 160, round % 3 ? 65535u : rnd() % 65536u, round & 2 ? x : nullptr);
        CHECK(mbx::bands_vector_sum(probe) == 65535u, "vector_of");
        check_record(x, probe, "a random row");
    }
    // the partial sums of the definition, in its order, stay inside int32 at the worst row: checked as it goes under UBSan, and here
    for (int n = 0; n < 160; ++n) {
        x[n] = -32768;
    }
    vector_of(probe, 65535u, x);
    wide acc = 0;
    for (int n = 0; n < 160; ++n) {
        acc += (wide)x[n] * (wide)probe[n];
        CHECK(acc <= 2147450880 && acc >= -2147450880, "a partial sum at %d", n);
    }
    CHECK(acc == 2147450880, "the aligned vector reaches the bound");
}

void check_bound_and_refusals() {
    std::vector<int16_t> bank(3 * 320, 0);
    int      probe = -1;
    char     which = '?';
    uint32_t sum = 0;
    int16_t* const v = bank.data() + 2 * 320 + 160;   // s of probe 2
    v[0] = 32767, v[1] = -32767, v[2] = 1;
    CHECK(mbx::bands_bank_refused(true, bank.data(), 3, &probe, &which, &sum) == mbx::kBandsOk, "a vector at 65535 passes");
    v[2] = 2;
    CHECK(mbx::bands_bank_refused(true, bank.data(), 3, &probe, &which, &sum) == mbx::kBandsBound && probe == 2 && which == 's' && sum == 65536u,
          "a vector at 65536: probe %d %c %u", probe, which, sum);
    char text[120];
    mbx::bands_bound_text(text, sizeof(text), probe, which, sum);
    CHECK(strcmp(text, "probe 2: the |s[n]| sum to 65536, above MBX_BANDS_VECTOR_BOUND (65535)") == 0, "%s", text);
    bank[320 + 5] = -32768, bank[320 + 6] = -32768;   // c of probe 1, found first
    CHECK(mbx::bands_bank_refused(true, bank.data(), 3, &probe, &which, &sum) == mbx::kBandsBound && probe == 1 && which == 'c' && sum == 65536u, "c of probe 1");
    CHECK(mbx::bands_bank_refused(true, bank.data(), 1, &probe, &which, &sum) == mbx::kBandsOk, "K = 1 does not look at probe 1");
    std::vector<int16_t> rails(320, -32768);
    CHECK(mbx::bands_bank_refused(true, rails.data(), 1, &probe, &which, &sum) == mbx::kBandsBound && probe == 0 && which == 'c' && sum == 160u * 32768u, "rails");
    // the bank's refusals in their order: pointers, K, the bound
    CHECK(mbx::bands_bank_refused(false, nullptr, 0, &probe, &which, &sum) == mbx::kBandsPointers, "everything wrong: the pointers first");
    CHECK(mbx::bands_bank_refused(true, nullptr, 0, &probe, &which, &sum) == mbx::kBandsPointers, "no probes");
    CHECK(mbx::bands_bank_refused(false, bank.data(), 3, &probe, &which, &sum) == mbx::kBandsPointers, "no place");
    CHECK(mbx::bands_bank_refused(true, bank.data(), 0, &probe, &which, &sum) == mbx::kBandsProbes, "K = 0 before the bound");
    CHECK(mbx::bands_bank_refused(true, bank.data(), -1, &probe, &which, &sum) == mbx::kBandsProbes, "K = -1");
    CHECK(mbx::bands_bank_refused(true, bank.data(), 33, &probe, &which, &sum) == mbx::kBandsProbes, "K = 33 (never read)");
    // the launch's in theirs: pointers, form, size, alignment, overlap
    const void* const in = reinterpret_cast<const void*>(0x10000);
    const void* const out = reinterpret_cast<const void*>(0x90000);
    const auto at = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
    using mbx::bands_launch_refused;
    CHECK(bands_launch_refused(0, 7, nullptr, (size_t)1 << 40, at(0x10008)) == mbx::kBandsPointers, "everything wrong: the pointers first");
    CHECK(bands_launch_refused(0, 0, in, 4, out) == mbx::kBandsPointers, "no bank");
    CHECK(bands_launch_refused(8, 0, nullptr, 4, out) == mbx::kBandsPointers && bands_launch_refused(8, 0, in, 4, nullptr) == mbx::kBandsPointers, "NULLs");
    CHECK(bands_launch_refused(8, 7, at(0x10008), (size_t)1 << 40, at(0x10008)) == mbx::kBandsForm, "then the form");
    CHECK(bands_launch_refused(8, 2, in, 4, out) == mbx::kBandsForm && bands_launch_refused(8, -1, in, 4, out) == mbx::kBandsForm, "forms");
    CHECK(bands_launch_refused(8, 0, at(0x10008), (size_t)1 << 40, at(0x10008)) == mbx::kBandsSize, "then the size");
    CHECK(bands_launch_refused(8, 0, at(0x10008), 4, at(0x10008)) == mbx::kBandsAlign, "then the alignment");
    CHECK(bands_launch_refused(8, 0, in, 4, in) == mbx::kBandsOverlap, "then the overlap");
    for (uintptr_t off = 1; off < 16; off <<= 1) {
        CHECK(bands_launch_refused(8, 1, at(0x10000 + off), 4, out) == mbx::kBandsAlign && bands_launch_refused(8, 1, in, 4, at(0x90000 + off)) == mbx::kBandsAlign,
              "a pointer at +%d", (int)off);
    }
    CHECK(bands_launch_refused(8, 0, in, 4, out) == mbx::kBandsOk && bands_launch_refused(32, 1, in, 0, in) == mbx::kBandsOk, "fine (no rows overlap nothing)");
    // the size: nrows * K * record_bytes <= 2^31 - 1, at the edge for every K and both forms
    for (int K = 1; K <= 32; ++K) {
        for (int form = 0; form < 2; ++form) {
            const size_t per = (size_t)K * (form == 0 ? 8u : 4u), most = (size_t)INT32_MAX / per;
            CHECK(mbx::bands_shape_refused(K, form, most) == mbx::kBandsOk && mbx::bands_shape_refused(K, form, most + 1) == mbx::kBandsSize, "K %d form %d", K, form);
            CHECK(mbx::bands_out_bytes(most, K, form) <= (size_t)INT32_MAX && mbx::bands_out_bytes(most + 1, K, form) > (size_t)INT32_MAX, "K %d form %d", K, form);
            CHECK(mbx::band_bytes(most, K, form) == mbx::bands_out_bytes(most, K, form), "band_bytes is bands_out_bytes");
        }
    }
    CHECK(mbx::bands_shape_refused(32, 0, SIZE_MAX) == mbx::kBandsSize, "no wrap");
    // the overlap: the records against the rows, either side, to the byte
    const uintptr_t rows_end = 0x10000 + 4 * 320;
    CHECK(bands_launch_refused(2, 0, in, 4, at(rows_end)) == mbx::kBandsOk && bands_launch_refused(2, 0, in, 4, at(rows_end - 16)) == mbx::kBandsOverlap, "behind");
    CHECK(bands_launch_refused(2, 0, in, 4, at(0x10000 - 64)) == mbx::kBandsOk && bands_launch_refused(2, 0, in, 4, at(0x10000 - 48)) == mbx::kBandsOverlap, "in front");
    CHECK(bands_launch_refused(2, 1, in, 4, at(0x10000 - 32)) == mbx::kBandsOk && bands_launch_refused(2, 1, in, 4, at(0x10000 - 16)) == mbx::kBandsOverlap, "in front, power");
    // band_bytes, the grid
    CHECK(mbx::band_bytes(0, 8, 1) == 0 && mbx::band_bytes(1, 1, 1) == 4 && mbx::band_bytes(1, 1, 0) == 8 && mbx::band_bytes(65536, 8, 1) == 2097152
              && mbx::band_bytes(65536, 32, 0) == 16777216 && mbx::band_bytes(3, 17, 0) == 408,
          "band_bytes");
    CHECK(mbx::bands_grid(1) == 1 && mbx::bands_grid(16) == 1 && mbx::bands_grid(17) == 2 && mbx::bands_grid(16 * 2048) == 2048 && mbx::bands_grid(16 * 2048 + 1) == 2048
              && mbx::bands_grid((size_t)INT32_MAX) == 2048,
          "the grid");
    CHECK(mbx::bands_bank_bytes(32) == 20480 && mbx::bands_bank_bytes(1) == 640, "the bank");
    // every refusal has a text, and they differ
    const mbx::BandsRefusal all[] = {mbx::kBandsPointers, mbx::kBandsProbes, mbx::kBandsBound, mbx::kBandsForm, mbx::kBandsSize, mbx::kBandsAlign, mbx::kBandsOverlap};
    for (size_t a = 0; a < sizeof(all) / sizeof(all[0]); ++a) {
        CHECK(mbx::bands_refusal_text(all[a])[0] != 0, "refusal %d has no text", (int)all[a]);
        for (size_t b = a + 1; b < sizeof(all) / sizeof(all[0]); ++b) {
            CHECK(strcmp(mbx::bands_refusal_text(all[a]), mbx::bands_refusal_text(all[b])) != 0, "refusals %d and %d share a text", (int)all[a], (int)all[b]);
        }
    }
}

}  // namespace

int main() {
    check_arithmetic();
    check_bound_and_refusals();
    if (failures) {
        printf("bands_check: %d FAILED\n", failures);
        return 1;
    }
    printf("bands_check: ok (16 lanes per row, up to %d probes, bound %u)\n", mbx::kBandsMaxProbes, (unsigned)mbx::kBandsVectorBound);
    return 0;
}
