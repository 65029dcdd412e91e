// keystream_check.cpp -- host check of keystream input (include/mbx_keystream.h), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_keystream_plan_host.py; a program of its own, nothing of it is loaded anywhere else.
//  1. the row -> words conversion every kernel and the host function share (mbelib-neo_amd/csrc/mbx_keystream_words.h) against a
//     bit-by-bit loop written from the header's sentence: every single-bit row, random rows, for 88 and 49 parameter bits;
//  2. the planner's rule for a keyed step (mbelib-neo_amd/csrc/mbx_launch_plan.h): over the cross product of shapes below,
//     plan_step(q with keyed, sw) == plan_step(q, sw with fuse_one = 0) field for field, for every value of MBX_FUSE_ONE, and a
//     keyed plan is never a one-launch or an in-wave fused step.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "mbx_keystream_words.h"
#include "mbx_launch_plan.h"

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

// the definition, bit by bit: parameter bit i (bit 31 - (i % 32) of w[i / 32]) takes bit 7 - (i & 7) of byte i >> 3; bits at and
// beyond nbits take nothing
void words_by_bits(const uint8_t row[12], int nbits, uint32_t w[3]) {
    w[0] = w[1] = w[2] = 0;
    for (int i = 0; i < nbits; ++i) {
        const uint32_t k = (row[i >> 3] >> (7 - (i & 7))) & 1u;
        w[i / 32] |= k << (31 - (i % 32));
    }
}

void check_row(const uint8_t row[12], int nbits) {
    uint32_t want[3];
    words_by_bits(row, nbits, want);
    const mbx::KeystreamWords a = mbx::keystream_words_of_row(row, nbits);
    uint32_t d[3];
    memcpy(d, row, 12);   // (a little-endian host, as the device is: what a dword load gives)
    const mbx::KeystreamWords b = mbx::keystream_words(d[0], d[1], d[2], nbits);
    CHECK(a.x == want[0] && a.y == want[1] && a.z == want[2], "bytes form, nbits %d: %08x %08x %08x, want %08x %08x %08x", nbits, a.x, a.y, a.z,
          want[0], want[1], want[2]);
    CHECK(b.x == want[0] && b.y == want[1] && b.z == want[2], "dword form, nbits %d: %08x %08x %08x, want %08x %08x %08x", nbits, b.x, b.y, b.z,
          want[0], want[1], want[2]);
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t next_u32() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

long check_words() {
    long rows = 0;
    static_assert(mbx::kKeystreamRowBytes == 12, "one row size");
    CHECK(mbx::keystream_nbits(0) == 88 && mbx::keystream_nbits(2) == 88 && mbx::keystream_nbits(1) == 49 && mbx::keystream_nbits(3) == 49,
          "nbits of the four codecs");
    CHECK(mbx::keystream_nbits(-1) == 0 && mbx::keystream_nbits(4) == 0 && mbx::keystream_nbits(9) == 0, "no such codec");
    for (int nbits : {88, 49}) {
        uint8_t row[12];
        memset(row, 0, sizeof(row));
        check_row(row, nbits), ++rows;
        for (int bit = 0; bit < 96; ++bit) {   // every single-bit row, the 8 / 47 ignored bits included
            memset(row, 0, sizeof(row));
            row[bit >> 3] = (uint8_t)(0x80u >> (bit & 7));
            check_row(row, nbits), ++rows;
            const mbx::KeystreamWords k = mbx::keystream_words_of_row(row, nbits);
            const int set = __builtin_popcount(k.x) + __builtin_popcount(k.y) + __builtin_popcount(k.z);
            CHECK(set == (bit < nbits ? 1 : 0), "bit %d of a row, nbits %d: %d bits set", bit, nbits, set);
        }
        memset(row, 0xff, sizeof(row));
        check_row(row, nbits), ++rows;
        for (int n = 0; n < 20000; ++n) {
            for (int j = 0; j < 12; ++j) {
                row[j] = (uint8_t)next_u32();
            }
            check_row(row, nbits), ++rows;
        }
    }
    return rows;
}

bool same_plan(const mbx::StepPlan& a, const mbx::StepPlan& b) {
    return a.form == b.form && a.instance == b.instance && a.front == b.front && a.expand == b.expand && a.rows == b.rows &&
           a.slice_frames == b.slice_frames && a.slice_groups == b.slice_groups && a.slice_own == b.slice_own && a.order == b.order &&
           a.front_lead == b.front_lead && a.workspace_frames == b.workspace_frames && a.order_offset == b.order_offset &&
           a.codec_offset == b.codec_offset && a.outside_capture_only == b.outside_capture_only;
}

long check_plans() {
    long plans = 0, would_fuse = 0;
    const mbx::DeviceFacts dev{1024, 6, 5, 2560};   // a whole MI355X: 256 CUs x 4 SIMDs; the waves per SIMD of the long launches (mbx_device.h)
    const int sizes[] = {1, 8, 256, 257, 5121}, frames[] = {1, 3, 4, 40};
    for (int fuse = 0; fuse <= 2; ++fuse) {
        mbx::LaunchSwitches sw;
        sw.fuse_one = fuse;
        mbx::LaunchSwitches off = sw;
        off.fuse_one = 0;
        for (int codec = 0; codec < 4; ++codec)
            for (int S : sizes)
                for (int T : frames)
                    for (int kind = 0; kind < 2; ++kind)
                        for (int bits = 0; bits < 64; ++bits) {
                            mbx::StepShape q;
                            q.codec = codec, q.S = S, q.T = T;
                            q.kind = kind ? mbx::kSoft : mbx::kFrames;
                            q.resident = (bits & 1) != 0;
                            q.ragged = (bits & 2) != 0;
                            q.mixed = (bits & 4) != 0;
                            q.aligned = (bits & 8) != 0;
                            q.own_workspace = q.slices_allowed = (bits & 16) != 0;
                            q.capturing = (bits & 32) != 0;
                            if (q.mixed) {
                                q.ragged = true;   // (mixed: ragged with a codec per stream)
                            }
                            q.total = (q.ragged || q.mixed) ? (size_t)S * (size_t)T : 0;
                            mbx::StepShape keyed = q;
                            keyed.keyed = true;
                            const mbx::StepPlan a = mbx::plan_step(keyed, sw, dev), b = mbx::plan_step(q, off, dev), u = mbx::plan_step(q, sw, dev);
                            ++plans;
                            CHECK(same_plan(a, b), "codec %d S %d T %d kind %d bits %d fuse %d: the keyed plan is not the MBX_FUSE_ONE=0 plan", codec, S, T,
                                  kind, bits, fuse);
                            CHECK(a.form != mbx::kOneLaunchStep && a.form != mbx::kFusedOneStep, "codec %d S %d T %d kind %d bits %d fuse %d: form %d", codec,
                                  S, T, kind, bits, fuse, (int)a.form);
                            CHECK(a.form != mbx::kNoLaunch, "a codec of the four has a plan");
                            if (u.form == mbx::kOneLaunchStep || u.form == mbx::kFusedOneStep) {
                                ++would_fuse;
                                CHECK(a.form == mbx::kStagedStep && a.front == mbx::kFecFront, "where the unkeyed step is one launch the keyed one is staged");
                            } else {
                                CHECK(same_plan(a, u), "codec %d S %d T %d kind %d bits %d fuse %d: a keyed plan differs from a staged unkeyed one", codec, S,
                                      T, kind, bits, fuse);
                            }
                        }
    }
    CHECK(would_fuse > 0, "the shapes hold steps whose unkeyed plan is a one-launch form");
    // the issue's example: 257 x 1 IMBE 7200x4400 on the slot's own workspace
    mbx::StepShape q;
    q.codec = 0, q.S = 257, q.T = 1, q.kind = mbx::kFrames, q.aligned = true, q.own_workspace = q.slices_allowed = true;
    const mbx::LaunchSwitches sw;
    CHECK(mbx::plan_step(q, sw, dev).instance == mbx::kOneLaunch + 0, "unkeyed 257 x 1: imbe_one_launch_kernel");
    q.keyed = true;
    const mbx::StepPlan p = mbx::plan_step(q, sw, dev);
    CHECK(p.form == mbx::kStagedStep && p.instance == mbx::kOne + 0 && p.expand && p.workspace_frames == 257, "keyed 257 x 1: imbe_stream_kernel_one on rows");
    printf("%ld plans, %ld of them one-launch forms when unkeyed\n", plans, would_fuse);
    return plans;
}

}  // namespace

int main() {
    const long rows = check_words();
    const long plans = check_plans();
    if (failures) {
        printf("keystream_check: %d FAILED\n", failures);
        return 1;
    }
    printf("%ld rows\nkeystream_check: ok (%ld rows, %ld plans)\n", rows, rows, plans);
    return 0;
}
