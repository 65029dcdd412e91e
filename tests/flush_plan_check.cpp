// flush_plan_check.cpp -- the layout of a queue-mode flush (mbelib-neo_amd/csrc/mbe_flush_plan.h) against its stated properties, on the
// CPU: tests/test_flush_plan_host.py builds this with -fsanitize=address,undefined and runs it.  ONE FlushPlan object serves every
// case, as Batch reuses its own from flush to flush.  Every property is derived here a second time from the channels and the queue,
// not read back from the plan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "mbe_flush_plan.h"

namespace {

struct Ch {
    int  codec;
    bool soft;
    int  pending;
};
struct En {
    int channel;
};

long g_case = 0;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            fprintf(stderr, "flush_plan_check: case %ld, line %d: %s\n", g_case, __LINE__, #cond);   \
            abort();                                                                                 \
        }                                                                                            \
    } while (0)

size_t input_bytes(int codec, bool soft) {   // (include/mbx_types.h: wire frames of 18 / 9 / 18 / 9 bytes, 184 / 96 / 168 / 96 two-byte cells)
    static const size_t hard[4] = {18, 9, 18, 9}, cells[4] = {184, 96, 168, 96};
    return soft ? 2 * cells[codec] : hard[codec];
}

std::vector<En> queue_of(const std::vector<Ch>& ch, bool round_robin) {
    std::vector<En> q;
    if (!round_robin) {
        for (size_t c = 0; c < ch.size(); ++c) {
            q.insert(q.end(), (size_t)ch[c].pending, En{(int)c});
        }
        return q;
    }
    for (int t = 0;; ++t) {
        const size_t before = q.size();
        for (size_t c = 0; c < ch.size(); ++c) {
            if (t < ch[c].pending) {
                q.push_back(En{(int)c});
            }
        }
        if (q.size() == before) {
            return q;
        }
    }
}

void check(mbx::FlushPlan& p, const std::vector<Ch>& ch, const std::vector<En>& q) {
    ++g_case;
    p.build(ch.data(), ch.size(), q.data(), q.size());
    p.invert_rows();
    // groups: one per distinct key, in order of the first channel that has it, then hard before soft (stable)
    struct Want {
        Ch               key;
        std::vector<int> members;
    };
    std::vector<Want> first_seen, want;
    for (size_t c = 0; c < ch.size(); ++c) {
        if (ch[c].pending == 0) {
            continue;
        }
        size_t g = 0;
        while (g < first_seen.size() && !(first_seen[g].key.codec == ch[c].codec && first_seen[g].key.soft == ch[c].soft && first_seen[g].key.pending == ch[c].pending)) {
            ++g;
        }
        if (g == first_seen.size()) {
            first_seen.push_back(Want{ch[c], {}});
        }
        first_seen[g].members.push_back((int)c);   // ascending channel index
    }
    for (int soft = 0; soft < 2; ++soft) {
        for (const Want& w : first_seen) {
            if (w.key.soft == (soft != 0)) {
                want.push_back(w);
            }
        }
    }
    CHECK(p.groups.size() == want.size());
    size_t nhard = 0;
    while (nhard < want.size() && !want[nhard].key.soft) {
        ++nhard;
    }
    CHECK(p.form_g0[0] == 0 && p.form_g0[1] == nhard && p.form_g0[2] == want.size());
    CHECK(p.form_mixed[0] == (nhard > 1) && p.form_mixed[1] == (want.size() - nhard > 1));
    CHECK(p.any_mixed() == (p.form_mixed[0] || p.form_mixed[1]));
    // per group: row0, byte0, stride, its channels in the index list
    size_t rows = 0, bytes = 0, at = 0;
    std::vector<size_t> pos(ch.size(), 0), group(ch.size(), 0);
    for (size_t g = 0; g < want.size(); ++g) {
        const mbx::FlushGroup& pg = p.groups[g];
        const Ch& k = want[g].key;
        const bool mixed = p.form_mixed[k.soft];
        CHECK(pg.codec == k.codec && pg.soft == k.soft && pg.T == k.pending && pg.nch == want[g].members.size());
        CHECK(pg.row0 == rows && pg.byte0 == bytes && pg.index0 == at);
        CHECK(pg.stride == (mixed ? (k.soft ? (size_t)MBX_IMBE_SOFT_BITS * sizeof(mbe_soft_bit) : (size_t)MBX_IMBE_FRAME_BYTES) : input_bytes(k.codec, k.soft)));
        CHECK(mbx::flush_input_bytes(k.codec, k.soft) == input_bytes(k.codec, k.soft) && pg.stride >= input_bytes(k.codec, k.soft));
        CHECK(pg.byte0 % 16 == 0 || (mixed && g != p.form_g0[k.soft]));
        for (size_t i = 0; i < want[g].members.size(); ++i) {
            const int c = want[g].members[i];
            CHECK(p.channels.size() > at + i && p.channels[at + i] == c && p.group_of[(size_t)c] == g);
            pos[(size_t)c] = i;
            group[(size_t)c] = g;
        }
        at += pg.nch;
        rows += pg.nch * (size_t)pg.T;
        bytes += pg.nch * (size_t)pg.T * pg.stride;
        if (!mixed || g + 1 == p.form_g0[k.soft + 1]) {
            bytes = (bytes + 15) / 16 * 16;
        }
    }
    CHECK(p.channels.size() == at && p.rows == rows && p.bytes == bytes && rows == q.size());
    // rows of the entries, the inverse, the bytes of every frame
    CHECK(p.row_of.size() == q.size() && p.by_row.size() == rows);
    std::vector<size_t> seen(ch.size(), 0);
    std::vector<char> hit(rows, 0);
    std::vector<std::pair<size_t, size_t>> ranges;
    for (size_t e = 0; e < q.size(); ++e) {
        const size_t c = (size_t)q[e].channel;
        const mbx::FlushGroup& pg = p.groups[group[c]];
        const size_t local = pos[c] * (size_t)pg.T + seen[c]++;
        CHECK(p.row_of[e] == pg.row0 + local);
        CHECK(p.row_of[e] < rows && p.by_row[p.row_of[e]] == e && !hit[p.row_of[e]]);
        hit[p.row_of[e]] = 1;
        const size_t b0 = pg.byte0 + local * pg.stride, b1 = b0 + input_bytes(pg.codec, pg.soft);
        CHECK(p.byte_of(e, (int)c) == b0 && b1 <= p.bytes);
        ranges.emplace_back(b0, b1);
    }
    for (size_t r = 0; r < rows; ++r) {   // by_row is a permutation of [0, rows)
        CHECK(hit[r] && p.by_row[r] < q.size() && p.row_of[p.by_row[r]] == r);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i) {
        CHECK(ranges[i - 1].second <= ranges[i].first);
    }
    // mixed forms: offsets relative to the form's first row (channels + 1, the last = the form's rows) and codecs, in index order
    size_t no = 0, nc = 0;
    for (int f = 0; f < 2; ++f) {
        size_t fch = 0, frows = 0;
        for (size_t g = p.form_g0[f]; g < p.form_g0[f + 1]; ++g) {
            fch += p.groups[g].nch;
            frows += p.groups[g].nch * (size_t)p.groups[g].T;
        }
        CHECK(p.form_channels(f) == fch && p.form_rows(f) == frows);
        if (!p.form_mixed[f]) {
            continue;
        }
        CHECK(p.off_at[f] == no && p.codec_at[f] == nc && p.offsets.size() >= no + fch + 1 && p.codecs.size() >= nc + fch);
        const size_t i0 = p.groups[p.form_g0[f]].index0, r0 = p.groups[p.form_g0[f]].row0;
        for (size_t i = 0; i < fch; ++i) {
            const size_t c = (size_t)p.channels[i0 + i];
            CHECK((size_t)p.offsets[no + i] == p.groups[group[c]].row0 + pos[c] * (size_t)ch[c].pending - r0);
            CHECK(p.offsets[no + i + 1] - p.offsets[no + i] == ch[c].pending && p.codecs[nc + i] == ch[c].codec);
        }
        CHECK((size_t)p.offsets[no + fch] == frows);
        no += fch + 1;
        nc += fch;
    }
    CHECK(p.offsets.size() == no && p.codecs.size() == nc);
}

void check_both_orders(mbx::FlushPlan& p, const std::vector<Ch>& ch) {
    check(p, ch, queue_of(ch, false));
    check(p, ch, queue_of(ch, true));
}

}  // namespace

int main() {
    mbx::FlushPlan plan;
    check(plan, {}, {});   // the empty plan
    CHECK(plan.rows == 0 && plan.bytes == 0 && plan.groups.empty());
    // every assignment of (codec, form, 0..3 pending) to three channels: 32^3 cases, each queued channel-major and round-robin
    for (int a = 0; a < 32 * 32 * 32; ++a) {
        std::vector<Ch> ch;
        for (int k = 0, v = a; k < 3; ++k, v /= 32) {
            ch.push_back(Ch{v % 4, (v / 4) % 2 != 0, (v / 8) % 4});
        }
        check_both_orders(plan, ch);
    }
    // ~200 channels, up to 128 pending, few distinct counts (large groups) and many (groups of one)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&s](uint32_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33) % n;
    };
    for (int k = 0; k < 6; ++k) {
        static const int few[5] = {0, 1, 3, 64, 128};
        std::vector<Ch> ch;
        for (uint32_t c = 0, n = 190 + next(20); c < n; ++c) {
            ch.push_back(Ch{(int)next(4), k >= 4 ? false : next(2) != 0, k % 2 ? few[next(5)] : (int)next(129)});
        }
        check_both_orders(plan, ch);
    }
    check(plan, {}, {});   // ... and nothing is left of them
    CHECK(plan.rows == 0 && plan.bytes == 0 && plan.groups.empty() && plan.channels.empty() && plan.offsets.empty());
    printf("flush_plan_check: %ld cases ok\n", g_case);
    return 0;
}
