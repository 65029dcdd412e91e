// hold_check.cpp -- host check of the held gate (include/mbx_hold.h), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_hold_host.py; a program of its own, nothing of it is loaded anywhere else.
//   every refusal of mbelib-neo_amd/csrc/mbx_hold_plan.h: the hold, the state, a state record, and those of the gated launch it
//     reuses -- pointers as numbers, never dereferenced;
//   the decision function over all (open', hang' in {0, 1, 2}, p in {close - 1, close, open - 1, open}) against the rule written out;
//   q(n) over every ramp_log2 and every code against the table of the header, and a lane's piece mode against q(n);
//   the identity q = R -> ramped == term (and q = 0 -> 0) over the extremes of term, |ramped| <= |term| + 1 for every q;
//   the accumulator bound of a full bus;
//   the state record as a word, the sizes and the grids.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>

#include "mbx_hold_plan.h"

#include <mbx_hold.h>   // the public header (include/ is first on the include path)

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

static_assert(sizeof(mbx_mixdown_hold) == 8 && offsetof(mbx_mixdown_hold, open_peak) == 0 && offsetof(mbx_mixdown_hold, close_peak) == 2
                  && offsetof(mbx_mixdown_hold, hang_frames) == 4 && offsetof(mbx_mixdown_hold, loudest_n) == 6 && offsetof(mbx_mixdown_hold, ramp_log2) == 7,
              "the hold");
static_assert(sizeof(mbx_gate_input_state) == 4 && offsetof(mbx_gate_input_state, hang_left) == 0 && offsetof(mbx_gate_input_state, open) == 2
                  && offsetof(mbx_gate_input_state, on) == 3,
              "the state record");
static_assert(MBX_HOLD_MAX_RAMP_LOG2 == mbx::kHoldMaxRampLog2 && MBX_GATE_MAX_LOUDEST == mbx::kGateMaxLoudest, "constants");

const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

// ---- refusals -------------------------------------------------------------------------------------------------------------------------
void check_refusals() {
    using namespace mbx;
    CHECK(hold_refused(true, 900, 500, 3, 3) == kHoldOk && hold_refused(true, 0, 0, 0, 0) == kHoldOk, "good holds");
    CHECK(hold_refused(true, 32768, 32768, 8, 7) == kHoldOk, "the limits of the hold");
    CHECK(hold_refused(false, 900, 500, 3, 3) == kHoldNull, "no hold");
    CHECK(hold_refused(true, 500, 501, 0, 0) == kHoldClose && hold_refused(true, 0, 1, 0, 0) == kHoldClose, "close_peak above open_peak");
    CHECK(hold_refused(true, 32769, 0, 0, 0) == kHoldPeak && hold_refused(true, 65535, 65535, 0, 0) == kHoldPeak, "open_peak above 32768");
    CHECK(hold_refused(true, 900, 500, 9, 0) == kHoldLoudest && hold_refused(true, 900, 500, 255, 0) == kHoldLoudest, "loudest_n 9");
    CHECK(hold_refused(true, 900, 500, 8, 8) == kHoldRamp && hold_refused(true, 900, 500, 0, 255) == kHoldRamp, "ramp_log2 8");

    int here = 0, there = 0;
    CHECK(hold_state_refused(true, &here, &here) == kHoldOk, "the state of this plan");
    CHECK(hold_state_refused(false, nullptr, &here) == kHoldNoState, "no state");
    CHECK(hold_state_refused(true, &there, &here) == kHoldForeign, "the state of another plan");

    const uint32_t good[5] = {hold_state_word(0, 0, 0), hold_state_word(65535, 1, 1), hold_state_word(7, 1, 0), hold_state_word(0, 1, 1), hold_state_word(3, 0, 0)};
    CHECK(hold_records_refused(good, 5) == kHoldOk && hold_records_refused(good, 0) == kHoldOk, "good records");
    for (const uint32_t bad : {hold_state_word(0, 2, 0), hold_state_word(0, 1, 2), hold_state_word(0, 0, 1), hold_state_word(9, 255, 255), hold_state_word(0, 2, 1)}) {
        uint32_t words[5];
        memcpy(words, good, sizeof(words));
        words[4] = bad;
        CHECK(hold_records_refused(words, 5) == kHoldRecord && hold_records_refused(words, 4) == kHoldOk && !hold_word_ok(bad), "record %08x", bad);
    }

    const int32_t off[3] = {0, 2, 3}, row[3] = {4, 4, 0};
    MixdownPlan plan;
    CHECK(plan_mixdown(2, off, row, 0, &plan) == kMixdownOk && plan.rows_needed == 5, "a plan");
    LevelsRefusal lv;
    MixdownRefusal mix;
    // the plan's handle at &here; rows at 0x10000 (8 rows), levels at 0x20000, out at 0x30000
    const auto held = [&](const MixdownPlan* p, bool have_hold, unsigned open, unsigned close, unsigned n, unsigned ramp, bool have_state, const void* state_plan,
                          int form, uintptr_t in, size_t nrows, uintptr_t levels, uintptr_t out) {
        return held_launch_refused(p, &here, have_hold, open, close, n, ramp, have_state, state_plan, form, at(in), nrows, at(levels), at(out), &lv, &mix);
    };
    CHECK(held(&plan, true, 900, 500, 3, 3, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldOk && lv == kLevelsOk && mix == kMixdownOk, "a good call");
    CHECK(held(&plan, true, 32768, 0, 8, 7, true, &here, 2, 0x10000, 8, 0x20000, 0x30008) == kHoldOk, "the limits, bytes at 8");
    CHECK(held(&plan, false, 0, 0, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldNull, "no hold");
    CHECK(held(&plan, true, 500, 900, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldClose, "close above open");
    CHECK(held(&plan, true, 32769, 0, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldPeak, "open_peak 32769");
    CHECK(held(&plan, true, 900, 500, 9, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldLoudest, "loudest_n 9");
    CHECK(held(&plan, true, 900, 500, 0, 8, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldRamp, "ramp_log2 8");
    CHECK(held(&plan, true, 900, 500, 0, 0, false, nullptr, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldNoState, "no state");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &there, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldForeign, "a foreign state");
    // everything the gated launch refuses, by its own names
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0, 0x30000) == kHoldGated && lv == kLevelsPointers, "no levels");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x20008, 0x30000) == kHoldGated && lv == kLevelsAlign, "levels at 8");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 3, 0x10000, 8, 0x20000, 0x30000) == kHoldGated && lv == kGateMixdown && mix == kMixdownForm, "form");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0, 8, 0x20000, 0x30000) == kHoldGated && lv == kGateMixdown && mix == kMixdownPointers, "no rows");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0) == kHoldGated && mix == kMixdownPointers, "no out");
    CHECK(held(nullptr, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x30000) == kHoldGated && mix == kMixdownPointers, "no plan");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10008, 8, 0x20000, 0x30000) == kHoldGated && mix == kMixdownAlign, "rows at 8");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x30008) == kHoldGated && mix == kMixdownAlign, "int16 buses at 8");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 1, 0x10000, 8, 0x20000, 0x30004) == kHoldGated && mix == kMixdownAlign, "byte buses at 4");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 4, 0x20000, 0x30000) == kHoldGated && mix == kMixdownRows, "rows short of the plan");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x20000, 0x10000 + 2560 - 16) == kHoldGated && mix == kMixdownOverlap, "out in the rows");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x10000 + 2560 - 16, 0x30000) == kHoldGated && lv == kLevelsOverlap, "levels in the rows");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x30000 + 640 - 16, 0x30000) == kHoldGated && lv == kLevelsOverlap, "levels in the buses");
    CHECK(held(&plan, true, 900, 500, 0, 0, true, &here, 0, 0x10000, 8, 0x10000 + 2560, 0x30000) == kHoldOk, "levels right behind the rows");
    for (int r = kHoldNull; r < kHoldGated; ++r) {
        CHECK(hold_refusal_text((HoldRefusal)r)[0] != 0, "a refusal without a text: %d", r);
    }
}

// ---- the decision ---------------------------------------------------------------------------------------------------------------------
void check_decision() {
    using namespace mbx;
    for (const auto& peaks : {std::pair<uint32_t, uint32_t>{900, 500}, {900, 900}, {32768, 1}, {2, 1}}) {
        const uint32_t open_peak = peaks.first, close_peak = peaks.second;
        for (uint32_t hang_frames : {0u, 1u, 2u, 65535u}) {
            for (uint32_t was_open = 0; was_open <= 1; ++was_open) {
                for (uint32_t hang_was = 0; hang_was <= 2; ++hang_was) {
                    for (uint32_t p : {close_peak - 1, close_peak, open_peak - 1, open_peak}) {
                        const HoldDecision d = hold_decide(p, was_open, hang_was, open_peak, close_peak, hang_frames);
                        uint32_t open, hang;
                        if (p >= open_peak) {   // the rule of the header, case by case
                            open = 1, hang = hang_frames;
                        } else if (was_open && p >= close_peak) {
                            open = 1, hang = hang_frames;
                        } else if (was_open && hang_was > 0) {
                            open = 1, hang = hang_was - 1;
                        } else {
                            open = 0, hang = 0;
                        }
                        CHECK(d.open == open && d.hang == hang, "open' %u hang' %u p %u under {%u, %u, %u}: {%u, %u}, want {%u, %u}", was_open, hang_was, p, open_peak,
                              close_peak, hang_frames, d.open, d.hang, open, hang);
                        CHECK(hold_word_ok(hold_state_word(d.hang, d.open, 0)) && hold_word_ok(hold_state_word(d.hang, d.open, d.open)), "a decision is a good record");
                        CHECK((hold_key(d, 77, 5) != 0) == (d.open != 0) && (!d.open || hold_key(d, 77, 5) == gate_key(77, 0, 5, 0)), "the key of the decision");
                    }
                }
            }
        }
    }
    // a closed input below open_peak stays closed whatever its hang says; close_peak = 0 latches
    CHECK(hold_decide(899, 0, 2, 900, 500, 2).open == 0, "a closed input has no hang");
    CHECK(hold_decide(0, 1, 0, 900, 0, 0).open == 1 && hold_decide(0, 0, 0, 900, 0, 0).open == 0, "close_peak 0 latches an open input");
    // the record as a word, little-endian {uint16, uint8, uint8}
    const mbx_gate_input_state rec = {0x1234, 1, 1};
    uint32_t word;
    memcpy(&word, &rec, 4);
    CHECK(word == hold_state_word(0x1234, 1, 1) && hold_word_hang(word) == 0x1234 && hold_word_open(word) == 1 && hold_word_on(word) == 1, "the record's word");
    CHECK(hold_code(0, 0) == kHoldOff && hold_code(1, 1) == kHoldSteady && hold_code(0, 1) == kHoldRising && hold_code(1, 0) == kHoldFalling, "the codes");
}

// ---- q(n), the ramped term, a lane's piece ---------------------------------------------------------------------------------------------
void check_weights() {
    using namespace mbx;
    const int32_t extremes[] = {-(1 << 18) - 1, -(1 << 18), -32768, -2, -1, 0, 1, 2, 32767, (1 << 18) - 1, 1 << 18, (1 << 18) + 1};
    for (int r = 0; r <= kHoldMaxRampLog2; ++r) {
        const int32_t R = 1 << r;
        for (int n = 0; n < 160; ++n) {
            const int32_t up = n + 1 < R ? n + 1 : R;
            CHECK(hold_weight(kHoldSteady, n, r) == R && hold_weight(kHoldOff, n, r) == 0 && hold_weight(kHoldRising, n, r) == up
                      && hold_weight(kHoldFalling, n, r) == R - up,
                  "q(%d) at ramp_log2 %d", n, r);
            CHECK(hold_weight(kHoldRising, n, r) + hold_weight(kHoldFalling, n, r) == R, "a rising and a falling input weigh R together");
        }
        CHECK(hold_weight(kHoldRising, 0, r) == 1 && hold_weight(kHoldRising, R - 1, r) == R && hold_weight(kHoldFalling, R - 1, r) == 0, "the ends of the ramp, %d", r);
        // a lane's piece: skipped means every q is 0, steady means every q is R
        for (int piece = 0; piece < kMixdownPieces; ++piece) {
            for (uint32_t code : {(uint32_t)kHoldOff, (uint32_t)kHoldSteady, (uint32_t)kHoldRising, (uint32_t)kHoldFalling}) {
                const int mode = hold_piece_mode(code, piece, r);
                bool all_zero = true, all_full = true;
                for (int i = 0; i < kMixdownPiece; ++i) {
                    const int32_t q = hold_weight(code, piece * kMixdownPiece + i, r);
                    all_zero = all_zero && q == 0;
                    all_full = all_full && q == R;
                }
                CHECK(mode == (all_zero ? kHoldPieceSkip : all_full ? kHoldPieceSteady : kHoldPieceRamp), "piece %d, code %u, ramp_log2 %d: mode %d", piece, code, r, mode);
            }
        }
        // q = R gives the term itself, q = 0 gives 0, and every q stays within |term| + 1
        for (int32_t term : extremes) {
            CHECK(hold_ramped(term, R, r) == term && hold_ramped(term, 0, r) == 0, "term %d at ramp_log2 %d", term, r);
            for (int32_t q = 0; q <= R; ++q) {
                const int32_t y = hold_ramped(term, q, r);
                const long long exact2 = 2ll * term * q + R;   // floor((term * q + R / 2) / R) = floor(exact2 / (2 R)), without the shift
                long long want = exact2 / (2ll * R);
                if (exact2 % (2ll * R) != 0 && exact2 < 0) {
                    --want;
                }
                CHECK(y == (int32_t)want, "term %d, q %d, ramp_log2 %d: %d, want %lld", term, q, r, y, want);
                CHECK((y < 0 ? -y : y) <= (term < 0 ? -term : term) + 1, "|ramped| <= |term| + 1: term %d, q %d", term, q);
            }
        }
    }
    for (int32_t x : {-32768, 32767}) {   // the extremes of term are those of mixdown_term
        for (int32_t g : {-32768, 32767}) {
            const int32_t t = mixdown_term((int16_t)x, (int16_t)g);
            CHECK(t >= -(1 << 18) - 1 && t <= (1 << 18) + 1, "term %d", t);
        }
    }
}

// ---- the accumulator ------------------------------------------------------------------------------------------------------------------
void check_accumulator() {
    using namespace mbx;
    // a full bus of the largest terms, at every weight: the int32 sum is the int64 sum
    for (int r = 0; r <= kHoldMaxRampLog2; ++r) {
        for (int32_t q : {1 << r, (1 << r) - 1, 1}) {
            for (int sign : {-1, 1}) {
                const int32_t term = mixdown_term((int16_t)-32768, (int16_t)(sign < 0 ? 32767 : -32768));
                int32_t acc = 0;
                long long wide = 0;
                for (int k = 0; k < kMixdownMaxInputs; ++k) {
                    const int32_t y = hold_ramped(term, q, r);
                    wide += y;
                    acc = (int32_t)((uint32_t)acc + (uint32_t)y);   // (wraps without UB if it ever did: the check below would say so)
                }
                CHECK((long long)acc == wide && wide < (1ll << 31) && wide >= -(1ll << 31), "ramp_log2 %d, q %d: %lld", r, q, wide);
            }
        }
    }
    CHECK((long long)kMixdownMaxInputs * ((1ll << 18) + 2) < (1ll << 31), "4096 * (2^18 + 2) < 2^31");
}

void check_grids() {
    using namespace mbx;
    const int32_t off[4] = {0, 2, 30, 31}, row[31] = {0};
    MixdownPlan plan;
    CHECK(plan_mixdown(3, off, row, 0, &plan) == kMixdownOk && plan.n_short == 2 && plan.n_long == 1, "a plan of two short buses and a long one");
    CHECK(hold_decide_grid(plan) == 1, "one workgroup of lanes decides up to 256 short buses");
    plan.n_short = 256;
    CHECK(hold_decide_grid(plan) == 1, "256");
    plan.n_short = 257;
    CHECK(hold_decide_grid(plan) == 2, "257");
    plan.n_short = 0;
    CHECK(hold_decide_grid(plan) == 0, "no short bus: no launch");
    CHECK(hold_state_bytes(0) == 0 && hold_state_bytes(4096) == 16384, "4 bytes per input");
    CHECK(hold_alloc_bytes(0) == 16 && hold_alloc_bytes(1) == 16 && hold_alloc_bytes(4) == 32 && hold_alloc_bytes(4096) == 20480, "5 bytes per input, whole 16s, never empty");
    for (int32_t n : {0, 1, 3, 4, 5, 4096, 1 << 20}) {
        CHECK(hold_alloc_bytes(n) >= (size_t)n * 5u && hold_alloc_bytes(n) % 16 == 0, "the allocation holds the records and the codes: %d", n);
    }
}

}  // namespace

int main() {
    check_refusals();
    check_decision();
    check_weights();
    check_accumulator();
    check_grids();
    if (failures) {
        printf("hold_check: %d FAILED\n", failures);
        return 1;
    }
    printf("hold_check: ok (ramp_log2 up to %d, loudest_n up to %d)\n", mbx::kHoldMaxRampLog2, mbx::kGateMaxLoudest);
    return 0;
}
