// mixdown_check.cpp -- host check of mix-down out (include/mbx_mixdown.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_mixdown_host.py; a program of its own, nothing of it is loaded anywhere else.
//   the arithmetic the kernels and the host function share (mbelib-neo_amd/csrc/mbx_mixdown.h) against a naive loop in int64 with a
//     floor DIVISION in place of the shift: the extremes of sample and gain, 4,096 inputs at both ends of the accumulator, the rounding
//     at half an LSB, random buses in all three forms;
//   the host-only plan (mbelib-neo_amd/csrc/mbx_mixdown_plan.h): every refusal with its text, an empty bus, a row twice in a bus, the
//     splits, the grid sizes, rows_needed, the words of the tables, what mbx_mixdown refuses of its arguments;
//   the long form's partition walked as the workgroup walks it: twelve slices through a [12][160] array plus the reduce of the first
//     twenty lanes equals the straight sum, for 1, 11, 12, 13 and 4,096 inputs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mbx_mixdown_plan.h"   // (and through it the arithmetic, csrc/mbx_mixdown.h)

#include <mbx_mixdown.h>   // the public header of the same name (include/ is first on the include path): the constants agree

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

static_assert(MBX_MIXDOWN_PCM16 == mbx::kMixdownPcm16 && MBX_MIXDOWN_ULAW == mbx::kMixdownUlaw && MBX_MIXDOWN_ALAW == mbx::kMixdownAlaw, "forms");
static_assert(MBX_MIXDOWN_UNITY == mbx::kMixdownUnity && MBX_MIXDOWN_MAX_INPUTS == mbx::kMixdownMaxInputs, "limits");
static_assert(mbx::kMixdownSlices * mbx::kMixdownPieces <= mbx::kMixdownBlock && mbx::kMixdownPieces * mbx::kMixdownPiece == 160, "the long form's lanes");

uint32_t rng_state = 12345u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// ---- the second definition ------------------------------------------------------------------------------------------------------------
int64_t floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
int64_t naive_term(int x, int g) { return floor_div((int64_t)x * (int64_t)g + 2048, 4096); }
int naive_clamp(int64_t acc) { return (int)(acc < -32768 ? -32768 : acc > 32767 ? 32767 : acc); }

// a bus of the CSR arrays, straight: 160 sums in int64
void naive_bus(const int16_t* pcm16, const int32_t* src_row, const int16_t* gain, int32_t lo, int32_t hi, int64_t acc[160]) {
    for (int n = 0; n < 160; ++n) {
        acc[n] = 0;
    }
    for (int32_t k = lo; k < hi; ++k) {
        for (int n = 0; n < 160; ++n) {
            acc[n] += naive_term(pcm16[(size_t)src_row[k] * 160 + n], gain ? gain[k] : 4096);
        }
    }
}

// ---- the kernels' walks, on the CPU ------------------------------------------------------------------------------------------------------
// short form: lane (slot, piece) loops over its bus's inputs
void short_walk(const int16_t* pcm16, const mbx::MixdownInput* input, int32_t lo, int32_t count, int32_t acc[160]) {
    for (int piece = 0; piece < mbx::kMixdownPieces; ++piece) {
        int32_t a[mbx::kMixdownPiece] = {0};
        for (int32_t i = 0; i < count; ++i) {
            const mbx::MixdownInput in = input[lo + i];
            mbx::mixdown_add_piece(pcm16 + (size_t)in.row * 160 + piece * mbx::kMixdownPiece, (int16_t)in.gain, a);
        }
        memcpy(acc + piece * mbx::kMixdownPiece, a, sizeof(a));
    }
}

// long form: lanes 0 .. 239 = slice * 20 + piece, slice j takes inputs j, j + 12, ...; partial sums into part[12][160]; lanes 0 .. 19 reduce
void long_walk(const int16_t* pcm16, const mbx::MixdownInput* input, int32_t lo, int32_t count, int32_t acc[160]) {
    std::vector<int32_t> part((size_t)mbx::kMixdownSlices * 160, 0x5A5A5A5A);   // (LDS is not zeroed: every word must be written)
    for (int tid = 0; tid < mbx::kMixdownBlock; ++tid) {
        const int slice = tid / mbx::kMixdownPieces, piece = tid - slice * mbx::kMixdownPieces;
        if (slice < mbx::kMixdownSlices) {
            int32_t a[mbx::kMixdownPiece] = {0};
            for (int32_t i = slice; i < count; i += mbx::kMixdownSlices) {
                const mbx::MixdownInput in = input[lo + i];
                mbx::mixdown_add_piece(pcm16 + (size_t)in.row * 160 + piece * mbx::kMixdownPiece, (int16_t)in.gain, a);
            }
            memcpy(&part[(size_t)slice * 160 + piece * mbx::kMixdownPiece], a, sizeof(a));
        }
    }
    for (int tid = 0; tid < mbx::kMixdownPieces; ++tid) {
        for (int i = 0; i < mbx::kMixdownPiece; ++i) {
            int32_t sum = 0;
            for (int j = 0; j < mbx::kMixdownSlices; ++j) {
                sum += part[(size_t)j * 160 + tid * mbx::kMixdownPiece + i];
            }
            acc[tid * mbx::kMixdownPiece + i] = sum;
        }
    }
}

// ---- the arithmetic -------------------------------------------------------------------------------------------------------------------
void check_terms() {
    const int ext[5] = {-32768, -1, 0, 1, 32767};
    for (int x : ext) {
        for (int g : ext) {
            CHECK(mbx::mixdown_term((int16_t)x, (int16_t)g) == naive_term(x, g), "x %d g %d", x, g);
        }
    }
    // every gain against a spread of samples, every sample against a spread of gains
    for (int g = -32768; g <= 32767; ++g) {
        for (int x : {-32768, -12345, -1, 0, 1, 2, 777, 32767}) {
            CHECK(mbx::mixdown_term((int16_t)x, (int16_t)g) == naive_term(x, g), "x %d g %d", x, g);
            CHECK(mbx::mixdown_term((int16_t)g, (int16_t)x) == naive_term(g, x), "x %d g %d", g, x);
        }
    }
    // a gain of 0 gives no term whatever the sample: what the kernels fill a batch of four inputs up with
    for (int x = -32768; x <= 32767; ++x) {
        CHECK(mbx::mixdown_term((int16_t)x, 0) == 0, "x %d", x);
    }
    // unity is the identity, minus unity the negation (but for -32768, which the clamp brings back)
    for (int x = -32768; x <= 32767; ++x) {
        CHECK(mbx::mixdown_term((int16_t)x, 4096) == x && mbx::mixdown_term((int16_t)x, -4096) == -x, "x %d", x);
    }
    // rounding at half an LSB: a product of +-2048 (0.5: up to 1 and to 0), +-2047 (just below: 0, and -0.4998 -> 0), +-6144 (1.5: 2, -1)
    struct { int x, g, want; } half[] = {{1, 2048, 1}, {-1, 2048, 0}, {2048, 1, 1}, {2048, -1, 0}, {1, 2047, 0}, {-1, 2047, 0}, {2047, -1, 0},
                                         {1, 6144, 2}, {-1, 6144, -1}, {3, 2048, 2}, {-3, 2048, -1}, {6144, 1, 2}, {6144, -1, -1},
                                         {1, 2049, 1}, {-1, 2049, -1}, {-1, 6145, -2}};
    for (const auto& h : half) {
        CHECK(mbx::mixdown_term((int16_t)h.x, (int16_t)h.g) == h.want, "x %d g %d", h.x, h.g);
        CHECK(naive_term(h.x, h.g) == h.want, "naive: x %d g %d", h.x, h.g);
    }
    CHECK(mbx::mixdown_clamp(32768) == 32767 && mbx::mixdown_clamp(-32769) == -32768 && mbx::mixdown_clamp(32767) == 32767
              && mbx::mixdown_clamp(-32768) == -32768 && mbx::mixdown_clamp(0) == 0 && mbx::mixdown_clamp(INT32_MAX) == 32767
              && mbx::mixdown_clamp(INT32_MIN) == -32768, "clamp");
    CHECK(mbx::mixdown_byte(mbx::kMixdownUlaw, 0) == 0xFF && mbx::mixdown_byte(mbx::kMixdownAlaw, 0) == 0xD5, "silence");
    CHECK(mbx::mixdown_byte(mbx::kMixdownUlaw, 1 << 30) == mbx::pcm16_to_ulaw(32767) && mbx::mixdown_byte(mbx::kMixdownAlaw, -(1 << 30)) == mbx::pcm16_to_alaw(-32768), "saturated bytes");
    CHECK(mbx::mixdown_form_ok(0) && mbx::mixdown_form_ok(1) && mbx::mixdown_form_ok(2) && !mbx::mixdown_form_ok(3) && !mbx::mixdown_form_ok(-1), "forms");
}

// 4,096 inputs of (x, g) on one row: the accumulator stays in int32 at both ends and the output saturates
void check_full_buses() {
    std::vector<int16_t> row(160);
    std::vector<mbx::MixdownInput> input(4096);
    struct { int x, g; int64_t each; int want; } ends[] = {{-32768, -32768, 262144, 32767}, {32767, -32768, -262136, -32768}, {32767, 32767, 262128, 32767}};
    for (const auto& e : ends) {
        for (auto& v : row) {
            v = (int16_t)e.x;
        }
        for (auto& in : input) {
            in = mbx::MixdownInput{0, e.g};
        }
        CHECK(naive_term(e.x, e.g) == e.each, "x %d g %d", e.x, e.g);
        int32_t a[160], b[160];
        short_walk(row.data(), input.data(), 0, 4096, a);
        long_walk(row.data(), input.data(), 0, 4096, b);
        for (int n = 0; n < 160; ++n) {
            CHECK((int64_t)a[n] == 4096 * e.each && a[n] == b[n], "x %d g %d sample %d: %d %d", e.x, e.g, n, a[n], b[n]);
            CHECK(mbx::mixdown_clamp(a[n]) == e.want, "x %d g %d", e.x, e.g);
        }
    }
}

// random rows and buses: the two walks against the naive loop, all three forms
void check_walks() {
    const int rows = 37;
    std::vector<int16_t> pcm((size_t)rows * 160);
    for (auto& v : pcm) {
        const uint32_t r = rnd();
        v = (r & 15u) == 0 ? (int16_t)((r & 16u) ? 32767 : -32768) : (int16_t)(r >> 4);
    }
    const int counts[] = {0, 1, 2, 11, 12, 13, 24, 25, 100, 4096};
    for (int count : counts) {
        std::vector<int32_t> src(count);
        std::vector<int16_t> gain(count);
        std::vector<mbx::MixdownInput> input(count);
        for (int k = 0; k < count; ++k) {
            src[k] = (int32_t)(rnd() % rows);
            const uint32_t r = rnd();
            gain[k] = (r & 7u) == 0 ? (int16_t)((r & 8u) ? 32767 : -32768) : (int16_t)((int)(r >> 4 & 0x3FFF) - 8192);
            input[k] = mbx::MixdownInput{src[k], gain[k]};
        }
        if (count >= 2) {
            src[1] = src[0];   // a row twice in the bus
            input[1].row = src[0];
        }
        int64_t want[160];
        int32_t a[160], b[160];
        naive_bus(pcm.data(), src.data(), gain.data(), 0, count, want);
        short_walk(pcm.data(), input.data(), 0, count, a);
        long_walk(pcm.data(), input.data(), 0, count, b);
        for (int n = 0; n < 160; ++n) {
            CHECK(want[n] == a[n] && want[n] == b[n], "count %d sample %d: %lld %d %d", count, n, (long long)want[n], a[n], b[n]);
            const int y = naive_clamp(want[n]);
            CHECK(mbx::mixdown_clamp(a[n]) == y, "count %d sample %d", count, n);
            CHECK(mbx::mixdown_byte(mbx::kMixdownUlaw, b[n]) == mbx::pcm16_to_ulaw((int16_t)y) && mbx::mixdown_byte(mbx::kMixdownAlaw, b[n]) == mbx::pcm16_to_alaw((int16_t)y),
                  "count %d sample %d", count, n);
        }
    }
}

// ---- the plan --------------------------------------------------------------------------------------------------------------------------
bool has(const char* text, const char* part) { return strstr(text, part) != nullptr; }

void check_refusals() {
    mbx::MixdownPlan p;
    const int32_t ok_off[3] = {0, 2, 3}, ok_row[3] = {4, 4, 0};
    CHECK(mbx::plan_mixdown(2, ok_off, ok_row, 0, &p) == mbx::kMixdownOk && p.n_buses == 2 && p.inputs == 3 && p.rows_needed == 5, "the good one");
    CHECK(mbx::plan_mixdown(0, ok_off, ok_row, 0, &p) == mbx::kMixdownBuses && mbx::plan_mixdown(-1, ok_off, ok_row, 0, &p) == mbx::kMixdownBuses, "n_buses");
    CHECK(has(mbx::mixdown_refusal_text(mbx::kMixdownBuses), "n_buses must be at least 1"), "text");
    CHECK(mbx::plan_mixdown(2, nullptr, ok_row, 0, &p) == mbx::kMixdownNull && mbx::plan_mixdown(2, ok_off, nullptr, 0, &p) == mbx::kMixdownNull, "NULL arrays");
    CHECK(has(mbx::mixdown_refusal_text(mbx::kMixdownNull), "bus_offset and src_row are needed"), "text");
    const int32_t none[3] = {0, 0, 0};
    CHECK(mbx::plan_mixdown(2, none, nullptr, 0, &p) == mbx::kMixdownOk && p.rows_needed == 0 && p.inputs == 0 && p.n_short == 2, "no inputs need no src_row");
    const int32_t first[3] = {1, 2, 3};
    CHECK(mbx::plan_mixdown(2, first, ok_row, 0, &p) == mbx::kMixdownFirst && has(mbx::mixdown_refusal_text(mbx::kMixdownFirst), "bus_offset[0] must be 0"), "first");
    const int32_t down[3] = {0, 2, 1};
    CHECK(mbx::plan_mixdown(2, down, ok_row, 0, &p) == mbx::kMixdownDecreasing && has(mbx::mixdown_refusal_text(mbx::kMixdownDecreasing), "must not decrease"), "decreasing");
    const int32_t wrap[3] = {0, INT32_MAX, INT32_MIN};   // (the difference is taken in 64 bits)
    CHECK(mbx::plan_mixdown(1, wrap, ok_row, 0, &p) == mbx::kMixdownTooLong && mbx::plan_mixdown(2, wrap, ok_row, 0, &p) == mbx::kMixdownTooLong, "too long comes first");
    const int32_t neg_off[2] = {0, -1};
    CHECK(mbx::plan_mixdown(1, neg_off, ok_row, 0, &p) == mbx::kMixdownDecreasing, "a negative offset decreases");
    std::vector<int32_t> many(4097, 0);
    const int32_t full[2] = {0, 4096}, over[2] = {0, 4097};
    CHECK(mbx::plan_mixdown(1, full, many.data(), 0, &p) == mbx::kMixdownOk && p.n_long == 1 && p.rows_needed == 1, "4096 inputs");
    CHECK(mbx::plan_mixdown(1, over, many.data(), 0, &p) == mbx::kMixdownTooLong && has(mbx::mixdown_refusal_text(mbx::kMixdownTooLong), "MBX_MIXDOWN_MAX_INPUTS"), "4097 inputs");
    const int32_t neg_row[3] = {4, -1, 0}, most_row[3] = {4, INT32_MAX, 0}, big_row[3] = {4, INT32_MAX - 1, 0};
    CHECK(mbx::plan_mixdown(2, ok_off, neg_row, 0, &p) == mbx::kMixdownRow && has(mbx::mixdown_refusal_text(mbx::kMixdownRow), "negative src_row"), "row");
    CHECK(mbx::plan_mixdown(2, ok_off, most_row, 0, &p) == mbx::kMixdownRowMost && has(mbx::mixdown_refusal_text(mbx::kMixdownRowMost), "2^31-1"), "row most");
    CHECK(mbx::plan_mixdown(2, ok_off, big_row, 0, &p) == mbx::kMixdownOk && p.rows_needed == INT32_MAX, "the largest row");
    CHECK(mbx::plan_mixdown(2, ok_off, ok_row, -1, &p) == mbx::kMixdownSplit && has(mbx::mixdown_refusal_text(mbx::kMixdownSplit), "long_above"), "split");
    CHECK(p.n_buses == 0 && p.words == 0, "a refused plan is empty");
    for (int r = mbx::kMixdownNoHandle; r <= mbx::kMixdownOverlap; ++r) {
        CHECK(mbx::mixdown_refusal_text((mbx::MixdownRefusal)r)[0] != 0, "refusal %d has no text", r);
    }
}

// buses of the given sizes on rows 0 .. rows - 1: offsets, rows, gains
struct Buses {
    std::vector<int32_t> off, row;
    std::vector<int16_t> gain;
    explicit Buses(const std::vector<int>& sizes, int rows = 9) {
        off.push_back(0);
        for (int n : sizes) {
            for (int k = 0; k < n; ++k) {
                row.push_back((int32_t)(rnd() % rows));
                gain.push_back((int16_t)((int)(rnd() & 0xFFFF) - 32768));
            }
            off.push_back((int32_t)row.size());
        }
    }
};

// the tables say what the arrays say: every bus in exactly one of the two lists, in the caller's order, the inputs word for word
void check_tables(const Buses& b, int long_above, const int16_t* gain) {
    mbx::MixdownPlan p;
    const int n = (int)b.off.size() - 1;
    CHECK(mbx::plan_mixdown(n, b.off.data(), b.row.data(), long_above, &p) == mbx::kMixdownOk, "plan");
    const int above = long_above ? long_above : mbx::kMixdownLongAbove;
    CHECK(p.long_above == above && p.n_short + p.n_long == n && p.long_grid == (uint32_t)p.n_long, "split");
    CHECK(p.short_grid == ((uint32_t)p.n_short * 20u + 255u) / 256u, "short grid %u for %d", p.short_grid, p.n_short);
    CHECK((uint64_t)p.short_grid * 256u >= (uint64_t)p.n_short * 20u, "every short lane is in the grid");
    CHECK(p.at_short == (size_t)n + 1 && p.at_long == p.at_short + p.n_short && p.at_inputs >= p.at_long + p.n_long && p.at_inputs % 2 == 0
              && p.at_inputs <= p.at_long + p.n_long + 1 && p.words == p.at_inputs + 2 * (size_t)p.inputs, "layout");
    std::vector<int32_t> words(p.words + 2, 0x77777777);   // a word in front and one behind
    mbx::fill_mixdown_tables(p, b.off.data(), b.row.data(), gain, words.data() + 1);
    CHECK(words.front() == 0x77777777 && words.back() == 0x77777777, "the tables stay in their words");
    const int32_t* w = words.data() + 1;
    std::vector<int> seen(n, 0);
    int last = -1;
    for (int i = 0; i < p.n_short; ++i) {
        const int bus = w[p.at_short + i];
        CHECK(bus > last && bus < n && b.off[bus + 1] - b.off[bus] <= above, "short bus %d", bus);
        last = bus;
        if (bus >= 0 && bus < n) {
            ++seen[bus];
        }
    }
    last = -1;
    for (int i = 0; i < p.n_long; ++i) {
        const int bus = w[p.at_long + i];
        CHECK(bus > last && bus < n && b.off[bus + 1] - b.off[bus] > above, "long bus %d", bus);
        last = bus;
        if (bus >= 0 && bus < n) {
            ++seen[bus];
        }
    }
    int32_t most = -1;
    for (int bus = 0; bus < n; ++bus) {
        CHECK(seen[bus] == 1 && w[bus] == b.off[bus], "bus %d", bus);
    }
    CHECK(w[n] == p.inputs && p.inputs == b.off[n], "the end");
    for (int32_t k = 0; k < p.inputs; ++k) {
        CHECK(w[p.at_inputs + 2 * k] == b.row[k] && w[p.at_inputs + 2 * k + 1] == (gain ? gain[k] : 4096), "input %d", k);
        most = b.row[k] > most ? b.row[k] : most;
    }
    CHECK(p.rows_needed == most + 1, "rows_needed %d", p.rows_needed);
}

void check_plans() {
    const int above = mbx::kMixdownLongAbove;
    // an empty bus, single inputs, buses at and round the default split, a full one
    const Buses mixed({3, 0, 1, above, above + 1, 2, 4096, 0, 13, above - 1});
    for (int split : {0, 1, 2, 12, 13, above, 4095, 4096, 5000, INT32_MAX}) {
        check_tables(mixed, split, mixed.gain.data());
        check_tables(mixed, split, nullptr);
    }
    mbx::MixdownPlan p;
    CHECK(mbx::plan_mixdown(10, mixed.off.data(), mixed.row.data(), 0, &p) == mbx::kMixdownOk && p.n_long == 2 && p.n_short == 8, "default: %d long", p.n_long);
    CHECK(mbx::plan_mixdown(10, mixed.off.data(), mixed.row.data(), 1, &p) == mbx::kMixdownOk && p.n_long == 7 && p.n_short == 3, "above 1: %d long", p.n_long);
    CHECK(mbx::plan_mixdown(10, mixed.off.data(), mixed.row.data(), 4096, &p) == mbx::kMixdownOk && p.n_long == 0 && p.short_grid == 1 && p.long_grid == 0, "all short");
    // grid sizes for 1, 3, 13 and 70 buses of two inputs: all short, and (long_above = 1) all long
    const struct { int buses; uint32_t short_grid; } grids[] = {{1, 1}, {3, 1}, {12, 1}, {13, 2}, {70, 6}};
    for (const auto& g : grids) {
        const Buses twos(std::vector<int>(g.buses, 2));
        CHECK(mbx::plan_mixdown(g.buses, twos.off.data(), twos.row.data(), 0, &p) == mbx::kMixdownOk && p.short_grid == g.short_grid && p.long_grid == 0, "%d buses", g.buses);
        CHECK(mbx::plan_mixdown(g.buses, twos.off.data(), twos.row.data(), 1, &p) == mbx::kMixdownOk && p.short_grid == 0 && p.long_grid == (uint32_t)g.buses, "%d buses", g.buses);
        check_tables(twos, 1, nullptr);
    }
    // a row twice in a bus and in many buses
    Buses same({2, 2, 2});
    for (auto& r : same.row) {
        r = 7;
    }
    check_tables(same, 0, same.gain.data());
    CHECK(mbx::plan_mixdown(3, same.off.data(), same.row.data(), 0, &p) == mbx::kMixdownOk && p.rows_needed == 8, "rows_needed");
}

void check_launch_arguments() {
    mbx::MixdownPlan p;
    const int32_t off[3] = {0, 2, 3}, row[3] = {4, 4, 0};
    CHECK(mbx::plan_mixdown(2, off, row, 0, &p) == mbx::kMixdownOk && p.rows_needed == 5, "plan");
    const auto at = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
    using namespace mbx;
    CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x20000)) == kMixdownOk, "good");
    CHECK(mixdown_launch_refused(&p, 3, at(0x10000), 5, at(0x20000)) == kMixdownForm && mixdown_launch_refused(&p, -1, at(0x10000), 5, at(0x20000)) == kMixdownForm, "form");
    CHECK(mixdown_launch_refused(nullptr, 0, at(0x10000), 5, at(0x20000)) == kMixdownPointers && mixdown_launch_refused(&p, 0, nullptr, 5, at(0x20000)) == kMixdownPointers
              && mixdown_launch_refused(&p, 0, at(0x10000), 5, nullptr) == kMixdownPointers, "pointers");
    for (uintptr_t o = 1; o < 16; ++o) {
        CHECK(mixdown_launch_refused(&p, 1, at(0x10000 + o), 5, at(0x20000)) == kMixdownAlign, "input at +%d", (int)o);
        CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x20000 + o)) == kMixdownAlign, "int16 out at +%d", (int)o);
        for (int form : {1, 2}) {
            CHECK(mixdown_launch_refused(&p, form, at(0x10000), 5, at(0x20000 + o)) == (o == 8 ? kMixdownOk : kMixdownAlign), "byte out at +%d", (int)o);
        }
    }
    CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 4, at(0x20000)) == kMixdownRows && mixdown_launch_refused(&p, 0, at(0x10000), 0, at(0x20000)) == kMixdownRows, "rows");
    // overlap: 5 rows are 1600 bytes; 2 buses are 640 bytes of int16 and 320 of bytes
    CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x10000 + 1600)) == kMixdownOk && mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x10000 + 1584)) == kMixdownOverlap, "behind");
    CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 6, at(0x10000 + 1600)) == kMixdownOverlap, "the caller's rows count, read or not");
    CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x10000 - 640)) == kMixdownOk && mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x10000 - 624)) == kMixdownOverlap, "in front");
    CHECK(mixdown_launch_refused(&p, 1, at(0x10000), 5, at(0x10000 - 320)) == kMixdownOk && mixdown_launch_refused(&p, 2, at(0x10000), 5, at(0x10000 - 312)) == kMixdownOverlap, "bytes in front");
    CHECK(mixdown_launch_refused(&p, 0, at(0x10000), 5, at(0x10000)) == kMixdownOverlap, "in place");
}

}  // namespace

int main() {
    check_terms();
    check_full_buses();
    check_walks();
    check_refusals();
    check_plans();
    check_launch_arguments();
    if (failures) {
        printf("mixdown_check: %d FAILED\n", failures);
        return 1;
    }
    printf("mixdown_check: ok (default split %d, %d slices of %d pieces)\n", mbx::kMixdownLongAbove, mbx::kMixdownSlices, mbx::kMixdownPieces);
    return 0;
}
