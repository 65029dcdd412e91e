// group_plan_check.cpp -- mbelib-neo_amd/csrc/mbx_group_plan.h held to its properties on the CPU, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_group_plan_host.py.  A program of its own: nothing of the library is linked.
//   * every assignment of (codec, form, F in {1, 3, 9}, bursts_per_stream in {1, 2}, n in {0, 1, 63, 64, 65}) to three groups:
//     workgroup, row and stream ranges tile the grid, the rows and the stream rows without gap or overlap, the totals and the LDS
//     maximum are right, the workspace regions are aligned, disjoint and inside the frames asked for;
//   * eight-group cases (every n at every place among full groups, all empty, all single);
//   * the refusals: group counts, negative counts, bursts_per_stream < 1, and totals at and above 2^31-1 frames.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "mbx_group_plan.h"

namespace {

using namespace mbx;

unsigned long long g_cases = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

const int kChannelBits[4] = {144, 72, 142, 72};
const int kFrameBytes[4] = {18, 9, 18, 9};
const int kCells[4] = {184, 96, 168, 96};
const int kForms[5] = {0, 1, 2, 16, 8};   // MBX_BURST_FORM_PACKED, BITS, DIBITS, LLR16, LLR8

// what a schedule of this shape launches its gather with (the arithmetic of mbx_burst_schedule_create, on a burst that is its
// frames' channel bits and 24 more): the plan only carries these numbers, the check needs them to differ between groups
GroupShape shape_of(int codec, int form, int F, int per, int n, bool soft) {
    GroupShape q;
    q.codec = codec, q.form = form, q.frames = F, q.n_streams = n, q.bursts_per_stream = per;
    const int B = F * kChannelBits[codec] + 24;
    if (soft) {
        const int bytes = form == 8 ? B : (form == 2 ? B : 2 * B);
        const int most = (form == 2 || form == 8) ? 32 : 16;
        const int nb = 32768 / bytes;
        q.bursts_per_wg = nb < 1 ? 1 : (nb > most ? most : nb);
        q.lds = (unsigned)(F * kCells[codec] * 2 + q.bursts_per_wg * bytes + 7) & ~3u;
    } else {
        const int items = F * kFrameBytes[codec];
        const int lstride = 4 * ((((B + 7) / 8 + 3) / 4) | 1);
        q.bursts_per_wg = 64;
        q.lds = (unsigned)(items * 16 + 64 * lstride + ((64 * items + 3) & ~3));
    }
    return q;
}

// the properties of an accepted plan, from the shapes alone
void check_plan(const GroupShape* g, int n_groups, const GroupPlan& p, bool soft) {
    ++g_cases;
    CHECK(p.n_groups == n_groups);
    uint64_t wg = 0, row = 0, stream = 0;
    unsigned lds = 0;
    for (int i = 0; i < n_groups; ++i) {
        const GroupPlace& at = p.place[i];
        const uint64_t bursts = (uint64_t)g[i].n_streams * (uint64_t)g[i].bursts_per_stream;
        CHECK(at.first_wg == wg && at.first_row == (int64_t)row && at.first_stream == (int64_t)stream);   // no gap, no overlap
        CHECK(at.bursts == bursts && (uint64_t)at.rows == bursts * (uint64_t)g[i].frames);
        CHECK((uint64_t)at.wgs * (uint64_t)g[i].bursts_per_wg >= bursts);                                  // every burst has a workgroup ...
        CHECK(at.wgs == 0 ? bursts == 0 : ((uint64_t)at.wgs - 1) * (uint64_t)g[i].bursts_per_wg < bursts);   // ... and no workgroup is idle
        wg += at.wgs, row += (uint64_t)at.rows, stream += (uint64_t)g[i].n_streams;
        if (bursts && g[i].lds > lds) {
            lds = g[i].lds;
        }
    }
    CHECK(p.grid == wg && (uint64_t)p.total_rows == row && (uint64_t)p.total_streams == stream && p.lds == lds);
    // the workspace: step rows | gathered rows | layout words
    const size_t unit = 4096 + 64, row_bytes = soft ? 368 : 18;
    const size_t step = (size_t)row + ((size_t)stream + 63) / 64 + ((size_t)row + unit - 1) / unit;   // (a mixed step's own)
    const GroupWorkspace w = group_workspace(p, step, unit, row_bytes);
    CHECK(w.gathered >= step * unit && w.gathered % 256 == 0 && w.gathered < step * unit + 256);
    CHECK(w.frame_offset >= w.gathered + (size_t)row * row_bytes && w.frame_offset % 4 == 0);
    CHECK(w.stream_index == w.frame_offset + 4 * ((size_t)stream + 1) && w.stream_codec == w.stream_index + 4 * (size_t)stream);
    CHECK(w.end == w.stream_codec + (size_t)stream && w.frames * unit >= w.end && (w.frames == 0 || (w.frames - 1) * unit < w.end));
}

const int kF[3] = {1, 3, 9}, kPer[2] = {1, 2}, kN[5] = {0, 1, 63, 64, 65};

// Every assignment to three groups.  The forms that have hard bursts bring the hard gather's numbers, the soft-only forms (LLR16, LLR8)
// the soft gathers'.  plan_groups reads of a shape only (frames, n_streams, bursts_per_stream, bursts_per_wg, lds) -- codec and form
// are carried --, so assignments that agree in those five are ONE input: each distinct input is planned once and stands for all the
// assignments that give it (their number is counted, and must come to 600^3).
struct Distinct {
    GroupShape shape;
    unsigned long long times;
};
bool same_input(const GroupShape& a, const GroupShape& b) {
    return a.frames == b.frames && a.n_streams == b.n_streams && a.bursts_per_stream == b.bursts_per_stream && a.bursts_per_wg == b.bursts_per_wg &&
           a.lds == b.lds;
}
void three_groups() {
    static Distinct all[4 * 5 * 3 * 2 * 5];
    int count = 0;
    for (int codec = 0; codec < 4; ++codec) {
        for (int form : kForms) {
            for (int F : kF) {
                for (int per : kPer) {
                    for (int n : kN) {
                        const GroupShape q = shape_of(codec, form, F, per, n, form == 16 || form == 8);
                        int at = 0;
                        while (at < count && !same_input(all[at].shape, q)) {
                            ++at;
                        }
                        if (at == count) {
                            all[count++] = Distinct{q, 0};
                        }
                        ++all[at].times;
                    }
                }
            }
        }
    }
    GroupShape g[3];
    GroupPlan p;
    unsigned long long stood_for = 0;
    for (int a = 0; a < count; ++a) {
        g[0] = all[a].shape;
        for (int b = 0; b < count; ++b) {
            g[1] = all[b].shape;
            // (the places of groups 0 and 1 do not depend on group 2: the whole plan and its workspace are checked once per pair,
            // with every third group the ranges, totals and the LDS maximum)
            g[2] = all[0].shape;
            CHECK(plan_groups(g, 3, &p) == kGroupsOk);
            check_plan(g, 3, p, false);
            check_plan(g, 3, p, true);
            g_cases -= 2;
            for (int c = 0; c < count; ++c) {
                g[2] = all[c].shape;
                CHECK(plan_groups(g, 3, &p) == kGroupsOk);
                uint32_t wg = 0;
                int32_t row = 0, stream = 0;
                unsigned lds = 0;
                for (int i = 0; i < 3; ++i) {
                    const GroupPlace& at = p.place[i];
                    const uint32_t bursts = (uint32_t)(g[i].n_streams * g[i].bursts_per_stream);
                    CHECK(at.first_wg == wg && at.first_row == row && at.first_stream == stream && at.bursts == bursts);
                    CHECK(at.rows == (int32_t)bursts * g[i].frames && at.wgs == (bursts + (uint32_t)g[i].bursts_per_wg - 1) / (uint32_t)g[i].bursts_per_wg);
                    wg += at.wgs, row += at.rows, stream += g[i].n_streams;
                    lds = bursts && g[i].lds > lds ? g[i].lds : lds;
                }
                CHECK(p.grid == wg && p.total_rows == row && p.total_streams == stream && p.lds == lds && p.n_groups == 3);
                ++g_cases;
                stood_for += all[a].times * all[b].times * all[c].times;
            }
        }
    }
    CHECK(stood_for == 600ull * 600ull * 600ull);
    printf("group_plan_check: %d distinct inputs of 600 assignments per group\n", count);
}

void eight_groups() {
    GroupShape g[8];
    GroupPlan p;
    for (int soft = 0; soft < 2; ++soft) {
        for (int place = 0; place < 8; ++place) {
            for (int n : kN) {
                for (int i = 0; i < 8; ++i) {
                    g[i] = shape_of(i & 3, kForms[i % 5], kF[i % 3], kPer[i & 1], i == place ? n : 64 + i, soft != 0);
                }
                CHECK(plan_groups(g, 8, &p) == kGroupsOk);
                check_plan(g, 8, p, soft != 0);
            }
        }
        for (int n : {0, 1}) {   // all empty: nothing to launch; all single
            for (int i = 0; i < 8; ++i) {
                g[i] = shape_of(i & 3, kForms[i % 5], kF[i % 3], 1, n, soft != 0);
            }
            CHECK(plan_groups(g, 8, &p) == kGroupsOk);
            check_plan(g, 8, p, soft != 0);
            CHECK(p.grid == (n ? 8u : 0u) && p.total_streams == 8 * n && (n || (p.total_rows == 0 && p.lds == 0)));
        }
    }
    CHECK(plan_groups(nullptr, 0, &p) == kGroupsOk && p.grid == 0 && p.total_rows == 0 && p.total_streams == 0);
    ++g_cases;
}

void refusals() {
    GroupShape g[8];
    GroupPlan p;
    for (int i = 0; i < 8; ++i) {
        g[i] = shape_of(0, 0, 1, 1, 4, false);
    }
    CHECK(plan_groups(g, -1, &p) == kGroupCount && plan_groups(g, 9, &p) == kGroupCount);
    g[5].n_streams = -1;
    CHECK(plan_groups(g, 8, &p) == kGroupNegative && plan_groups(g, 5, &p) == kGroupsOk);
    g[5].n_streams = 4, g[2].bursts_per_stream = 0;
    CHECK(plan_groups(g, 8, &p) == kGroupBurstsPer);
    g[2].bursts_per_stream = -3;
    CHECK(plan_groups(g, 8, &p) == kGroupBurstsPer);
    g[2].bursts_per_stream = 1;
    // exactly 2^31-1 frames pass, one more is refused -- in one group, and as the sum of several
    g[0] = shape_of(0, 0, 1, 1, 0x7fffffff - 28, false);
    CHECK(plan_groups(g, 8, &p) == kGroupsOk && p.total_rows == 0x7fffffff);
    check_plan(g, 8, p, false);
    g[7].n_streams = 5;
    CHECK(plan_groups(g, 8, &p) == kGroupTooManyFrames);
    g[7].n_streams = 4;
    g[0] = shape_of(0, 0, 9, 2, 0x7fffffff, false);   // the products would leave 32 bits, and 2^31 * 2^31 * 18 would leave 64
    CHECK(plan_groups(g, 1, &p) == kGroupTooManyFrames);
    g[0].bursts_per_stream = 0x7fffffff;
    CHECK(plan_groups(g, 1, &p) == kGroupTooManyFrames);
    g[0] = shape_of(0, 0, 9, 1, 0x7fffffff / 9, false);
    CHECK(plan_groups(g, 1, &p) == kGroupsOk);
    g[0].n_streams += 1;
    CHECK(plan_groups(g, 1, &p) == kGroupTooManyFrames);
    for (int r = kGroupCount; r <= kGroupTooManyFrames; ++r) {
        CHECK(group_refusal_text((GroupRefusal)r)[0] != 0);
    }
    g_cases += 12;
}

}  // namespace

int main() {
    three_groups();
    eight_groups();
    refusals();
    printf("group_plan_check: %llu cases ok\n", g_cases);
    return 0;
}
