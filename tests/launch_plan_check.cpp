// launch_plan_check.cpp -- what a batch step launches (mbelib-neo_amd/csrc/mbx_launch_plan.h), on the CPU: tests/test_launch_plan_host.py
// builds this with -fsanitize=address,undefined and runs it.
//   no argument: the grid -- every decision of plan_step over the grid below, hashed (FNV-1a) and held to the count and hash that the
//     launcher's earlier select_instance / choose_slice_frames / needs_workspace and its order-kernel and workspace expressions gave
//     over the same grid (kParentCount, kParentHash: the PARENT's output, see EXPERIMENTS.md) --, the properties that need no parent,
//     checked at every grid point, and the switch parser on malformed input;
//   `case <codec> <S> <T> <entry>`: the kInstances index the call of a case of tests/instance_cases.py takes on a whole MI355X (1,024
//     SIMDs) under the switches of this process's environment, and the index mbx_batch_kernel_name's plan gives for it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "mbx_launch_plan.h"

namespace {

using mbx::DeviceFacts;
using mbx::LaunchSwitches;
using mbx::StepPlan;
using mbx::StepShape;

constexpr unsigned long long kParentCount = 12870144ULL;
constexpr uint64_t           kParentHash = 0x8785e233af7ae182ULL;

long long g_point = 0;

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            fprintf(stderr, "launch_plan_check: point %lld, line %d: %s\n", g_point, __LINE__, #cond);   \
            abort();                                                                                     \
        }                                                                                                \
    } while (0)

// ---- the grid ------------------------------------------------------------------------------------------------------------------
// One decision: what a step launches, as plain numbers (fields that a form does not have are 0).
struct Decision {
    int       launchable, form, instance, front, expand, rows, slice, groups, own, order, capture_only;
    long long lead;
    uint64_t  workspace, order_offset, codec_offset;
};
// ... and what the four exports predict for (codec, S, T)
struct Prediction {
    int uses_expand, slices, batch, batch_resident, stream, stream_resident;   // (the names as kInstances indices)
};

struct Fnv {
    uint64_t           h = 0xcbf29ce484222325ULL;
    unsigned long long count = 0;
    void word(uint64_t v) {
        for (int i = 0; i < 8; ++i) {
            h = (h ^ ((v >> (8 * i)) & 0xffu)) * 0x100000001b3ULL;
        }
    }
    void add(const Decision& d) {
        word((uint64_t)d.launchable | (uint64_t)d.form << 1 | (uint64_t)d.instance << 4 | (uint64_t)d.front << 10 | (uint64_t)d.expand << 12 |
             (uint64_t)d.rows << 13 | (uint64_t)d.groups << 14 | (uint64_t)d.own << 17 | (uint64_t)d.order << 18 | (uint64_t)d.capture_only << 19 |
             (uint64_t)(uint32_t)d.slice << 32);
        word((uint64_t)d.lead);
        word(d.workspace);
        word(d.order_offset);
        word(d.codec_offset);
        ++count;
    }
    void add(const Prediction& p) {
        word((uint64_t)p.uses_expand | (uint64_t)(uint32_t)p.slices << 32);
        word((uint64_t)p.batch | (uint64_t)p.batch_resident << 8 | (uint64_t)p.stream << 16 | (uint64_t)p.stream_resident << 24);
        ++count;
    }
};

using Env = std::vector<std::pair<const char*, const char*>>;
const char* const kSwitchNames[] = {"MBX_LDS_MIN_FRAMES", "MBX_NO_RES1", "MBX_NO_LDS_RESIDENT", "MBX_SLICE", "MBX_SLICE_GROUPS",
                                    "MBX_SLICE_OWN",      "MBX_RAGGED_ORDER", "MBX_FUSE_ONE",   "MBX_FRONT_LEAD"};
void set_env(const Env& env) {
    for (const char* n : kSwitchNames) {
        unsetenv(n);
    }
    for (const auto& kv : env) {
        setenv(kv.first, kv.second, 1);
    }
}
// the default switches, each switch alone at each of its meaningful values (ignored and clamped ones included), three pairs
const Env kEnvs[] = {
    {},
    {{"MBX_LDS_MIN_FRAMES", "0"}}, {{"MBX_LDS_MIN_FRAMES", "1"}}, {{"MBX_LDS_MIN_FRAMES", "2"}}, {{"MBX_LDS_MIN_FRAMES", "16"}},
    {{"MBX_LDS_MIN_FRAMES", "1048577"}},
    {{"MBX_NO_RES1", "1"}},
    {{"MBX_NO_LDS_RESIDENT", "1"}},
    {{"MBX_SLICE", "0"}}, {{"MBX_SLICE", "5"}}, {{"MBX_SLICE", "8"}}, {{"MBX_SLICE", "16"}}, {{"MBX_SLICE", "-5"}},
    {{"MBX_SLICE_GROUPS", "1"}}, {{"MBX_SLICE_GROUPS", "2"}}, {{"MBX_SLICE_GROUPS", "4"}}, {{"MBX_SLICE_GROUPS", "9"}},
    {{"MBX_SLICE_OWN", "0"}},
    {{"MBX_RAGGED_ORDER", "0"}},
    {{"MBX_FUSE_ONE", "0"}}, {{"MBX_FUSE_ONE", "1"}}, {{"MBX_FUSE_ONE", "x"}},
    {{"MBX_FRONT_LEAD", "-1"}}, {{"MBX_FRONT_LEAD", "0"}}, {{"MBX_FRONT_LEAD", "64"}},
    {{"MBX_SLICE", "16"}, {"MBX_SLICE_GROUPS", "2"}, {"MBX_SLICE_OWN", "0"}},
    {{"MBX_LDS_MIN_FRAMES", "1"}, {"MBX_FUSE_ONE", "0"}},
    {{"MBX_NO_LDS_RESIDENT", "1"}, {"MBX_SLICE", "16"}},
};
// 5,120 AMBE wave slots on 1,024 SIMDs: the 1.06 round-fill test flips between 9,660 and 9,661 streams; 6,144 IMBE slots
const int    kS[] = {0, 1, 2, 255, 256, 257, 5119, 5120, 5121, 6144, 6145, 9660, 9661, 10240, 10241, 65536};
const int    kT[] = {0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 128};
const size_t kTotals[] = {1, 255, 65536, 2147483647u};
const int    kSimds[] = {0, 256, 1024};

// Decider: begin(simds) after the environment of a switch set is in place; step(shape) -> Decision; predict(codec, S, T) -> Prediction
template <class Decider>
void walk_grid(Decider& d, Fnv& fnv) {
    for (const Env& env : kEnvs) {
        set_env(env);
        for (int simds : kSimds) {
            d.begin(simds);
            for (int codec = -1; codec <= 4; ++codec) {
                for (int S : kS) {
                    for (int T : kT) {
                        fnv.add(d.predict(codec, S, T));
                        for (int kind = 0; kind < 3; ++kind) {
                            for (int given = 0; given < (kind == 0 ? 2 : 1); ++given) {   // (rows there already: the records-based calls only)
                                for (int bits = 0; bits < 32; ++bits) {
                                    StepShape q;
                                    q.codec = codec, q.S = S, q.T = T;
                                    q.kind = (mbx::InputKind)kind;
                                    q.rows_given = given != 0;
                                    q.resident = bits & 1, q.aligned = bits & 2, q.own_workspace = bits & 4, q.capturing = bits & 8, q.slices_allowed = bits & 16;
                                    ++g_point;
                                    fnv.add(d.step(q));
                                }
                            }
                        }
                    }
                    for (size_t total : kTotals) {
                        for (int kind = 0; kind < 3; ++kind) {
                            for (int bits = 0; bits < 4; ++bits) {
                                StepShape q;
                                q.codec = codec, q.S = S, q.total = total;
                                q.kind = (mbx::InputKind)kind;
                                q.ragged = true;
                                q.resident = bits & 1, q.mixed = bits & 2;
                                q.own_workspace = true;
                                ++g_point;
                                fnv.add(d.step(q));
                            }
                        }
                    }
                }
            }
        }
    }
    set_env({});
}

// ---- plan_step on the grid, its properties checked at every point -------------------------------------------------------------------
constexpr size_t kRowBytes = 256;   // (sizeof(FrameParams): mbx_device.h)
DeviceFacts facts(int simds) { return DeviceFacts{simds, 6, 5, kRowBytes}; }   // (MBX_IMBE_ / MBX_AMBE_LDS_WAVES_PER_SIMD: mbx_device.h)

void check_properties(const StepShape& q, const StepPlan& p) {
    const bool known = q.codec >= 0 && q.codec <= 3;
    const bool ragged = q.ragged || q.mixed;
    // a codec outside 0..3 is never planned for a launch (a mixed step does not look at it) and answers as AMBE 3600x2450
    CHECK((p.form == mbx::kNoLaunch) == (!known && !q.mixed));
    if (!known && !q.mixed) {
        CHECK(ragged ? p.instance % 3 == 1 : (p.instance < mbx::kOneFused && p.instance % 3 == 1));
    }
    CHECK(p.instance >= 0 && p.instance < (q.mixed ? 2 : ragged ? 6 : mbx::kInstanceCount));
    const bool one_launch = !ragged && p.instance >= mbx::kOneLaunch && p.instance < mbx::kOneFused;
    CHECK(one_launch == (p.form == mbx::kOneLaunchStep));
    CHECK((!ragged && p.instance >= mbx::kOneFused) == (p.form == mbx::kFusedOneStep));
    // what needs the slot's flag words or side streams: never under capture, never without the slot's own workspace
    CHECK(p.outside_capture_only == (one_launch || p.slice_frames > 0));
    if (p.outside_capture_only) {
        CHECK(!q.capturing && q.own_workspace);
    }
    // slices: never resident state, never without leave; a positive multiple of eight, at least two slices
    CHECK((p.slice_frames > 0) == (!ragged && p.instance >= mbx::kSlice && p.instance < mbx::kOneLaunch));
    if (p.slice_frames > 0) {
        CHECK(!q.resident && q.slices_allowed && p.form == (known ? mbx::kStagedStep : mbx::kNoLaunch));
        CHECK(p.slice_frames % 8 == 0 && q.T >= 2 * p.slice_frames && q.S >= 2);
        CHECK(p.slice_groups >= 2 && p.slice_groups <= 4);
    } else {
        CHECK(p.slice_groups == 0 && !p.slice_own);
    }
    // rows: read where an expand launch writes them or the caller has them
    CHECK(!p.expand || p.rows);
    CHECK(!(p.expand && q.rows_given));
    if (ragged) {   // rows, then the order words, then (mixed) the codec bytes: inside the workspace, nothing overlapping
        CHECK(p.expand && p.order_offset == q.total);
        CHECK((p.codec_offset - p.order_offset) * kRowBytes >= (size_t)q.S * 4);
        CHECK(p.workspace_frames >= p.codec_offset && (p.workspace_frames - p.codec_offset) * kRowBytes >= (q.mixed ? q.total : 0));
        CHECK(!p.outside_capture_only && p.slice_frames == 0);
    } else {
        CHECK(!p.order && p.order_offset == 0 && p.codec_offset == 0);
        CHECK(p.workspace_frames == (one_launch ? (size_t)q.S : p.expand ? (size_t)q.S * (size_t)q.T : 0));
    }
}

Decision decision_of(const StepShape& q, const StepPlan& p) {
    Decision d{};
    d.launchable = p.form != mbx::kNoLaunch;
    // (a refused step is compared by what it would have been: the one-launch forms take known codecs only)
    d.form = p.form != mbx::kNoLaunch ? (int)p.form : (q.mixed ? mbx::kMixedStep : q.ragged ? mbx::kRaggedStep : mbx::kStagedStep);
    d.instance = p.instance;
    d.front = d.form == mbx::kOneLaunchStep || d.form == mbx::kFusedOneStep ? 0 : (int)p.front;
    d.expand = p.expand, d.rows = p.rows;
    d.slice = p.slice_frames, d.groups = p.slice_groups, d.own = p.slice_own;
    d.order = p.order;
    d.capture_only = p.outside_capture_only;
    d.lead = d.form == mbx::kOneLaunchStep ? p.front_lead : 0;
    d.workspace = p.workspace_frames;
    d.order_offset = p.order_offset, d.codec_offset = p.codec_offset;
    return d;
}

// the four exports' assumptions, as mbx_api.hip states them
StepShape batch_prediction(int codec, int S, int T, bool resident) {
    StepShape q;
    q.codec = codec, q.S = S, q.T = T;
    q.kind = mbx::kFrames;
    q.rows_given = q.aligned = q.own_workspace = q.slices_allowed = true;
    q.resident = resident;
    return q;
}
StepShape records_prediction(int codec, int S, int T) {
    StepShape q;
    q.codec = codec, q.S = S, q.T = T;
    q.own_workspace = q.slices_allowed = true;
    return q;
}
StepShape stream_prediction(int codec, int T) {
    StepShape q;
    q.codec = codec, q.T = T < 0 ? -T : T;
    q.rows_given = true;
    q.resident = T < 0;
    return q;
}

struct PlanDecider {
    LaunchSwitches sw;
    DeviceFacts    dev{};
    void begin(int simds) {
        sw = mbx::read_launch_switches();
        dev = facts(simds);
    }
    Decision step(const StepShape& q) {
        const StepPlan p = mbx::plan_step(q, sw, dev);
        check_properties(q, p);
        return decision_of(q, p);
    }
    Prediction predict(int codec, int S, int T) {
        Prediction r;
        r.uses_expand = mbx::plan_step(records_prediction(codec, S, T), sw, dev).expand;
        r.slices = mbx::plan_step(records_prediction(codec, S, T), sw, dev).slice_frames;
        r.batch = mbx::plan_step(batch_prediction(codec, S, T, false), sw, dev).instance;
        r.batch_resident = mbx::plan_step(batch_prediction(codec, S, T, true), sw, dev).instance;
        r.stream = mbx::plan_step(stream_prediction(codec, T), sw, dev).instance;
        r.stream_resident = mbx::plan_step(stream_prediction(codec, -T), sw, dev).instance;
        return r;
    }
};

// ---- the switch parser on what a person might type ---------------------------------------------------------------------------------------
long check_parser() {
    long n = 0;
    const auto with = [&n](const char* name, const char* value) {
        set_env(value ? Env{{name, value}} : Env{});
        ++n;
        return mbx::read_launch_switches();
    };
    const LaunchSwitches d = with("", nullptr);
    CHECK(d.lds_min_frames == 4 && d.res1 && d.lds_resident && d.slice == -1 && d.slice_groups == 3 && d.slice_own && d.ragged_order &&
          d.fuse_one == 2 && d.front_lead == INT_MAX);
    for (const char* v : {"0", "-1", "1048577", "x", ""}) {
        CHECK(with("MBX_LDS_MIN_FRAMES", v).lds_min_frames == 4);
    }
    CHECK(with("MBX_LDS_MIN_FRAMES", "1").lds_min_frames == 1 && with("MBX_LDS_MIN_FRAMES", "1048576").lds_min_frames == 1 << 20);
    for (const char* v : {"1", "0", ""}) {   // by presence
        CHECK(!with("MBX_NO_RES1", v).res1 && with("MBX_NO_RES1", v).lds_resident);
        CHECK(!with("MBX_NO_LDS_RESIDENT", v).lds_resident && with("MBX_NO_LDS_RESIDENT", v).res1);
    }
    CHECK(with("MBX_SLICE", "0").slice == 0 && with("MBX_SLICE", "5").slice == 5 && with("MBX_SLICE", "16").slice == 16 &&
          with("MBX_SLICE", "-5").slice == -5 && with("MBX_SLICE", "x").slice == 0);
    CHECK(with("MBX_SLICE_GROUPS", "1").slice_groups == 2 && with("MBX_SLICE_GROUPS", "9").slice_groups == 4 &&
          with("MBX_SLICE_GROUPS", "4").slice_groups == 4 && with("MBX_SLICE_GROUPS", "x").slice_groups == 2);
    CHECK(!with("MBX_SLICE_OWN", "0").slice_own && with("MBX_SLICE_OWN", "1").slice_own && with("MBX_SLICE_OWN", "").slice_own &&
          !with("MBX_SLICE_OWN", "00").slice_own && with("MBX_SLICE_OWN", "no").slice_own);
    CHECK(!with("MBX_RAGGED_ORDER", "0").ragged_order && with("MBX_RAGGED_ORDER", "1").ragged_order && with("MBX_RAGGED_ORDER", "").ragged_order);
    CHECK(with("MBX_FUSE_ONE", "0").fuse_one == 0 && with("MBX_FUSE_ONE", "1").fuse_one == 1 && with("MBX_FUSE_ONE", "2").fuse_one == 2 &&
          with("MBX_FUSE_ONE", "x").fuse_one == 2 && with("MBX_FUSE_ONE", "3").fuse_one == 2 && with("MBX_FUSE_ONE", "").fuse_one == 2);
    CHECK(with("MBX_FRONT_LEAD", "-1").front_lead == 0 && with("MBX_FRONT_LEAD", "0").front_lead == 0 && with("MBX_FRONT_LEAD", "64").front_lead == 64 &&
          with("MBX_FRONT_LEAD", "x").front_lead == 0);
    set_env({});
    return n;
}

// ---- one case of tests/instance_cases.py ---------------------------------------------------------------------------------------------
int run_case(int codec, int S, int T, const char* entry) {
    StepShape q;
    q.codec = codec, q.S = S, q.T = T;
    q.kind = strcmp(entry, "staged") == 0 ? mbx::kRecords : mbx::kFrames;   // (staged: mbx_fec_* + mbx_process_records)
    q.resident = strncmp(entry, "resident", 8) == 0;
    q.aligned = true;   // (the cases' frames sit on a 4-byte boundary where that matters)
    q.own_workspace = q.slices_allowed = strcmp(entry, "batch_ws") != 0;
    const LaunchSwitches sw = mbx::read_launch_switches();
    const StepPlan       real = mbx::plan_step(q, sw, facts(1024));
    const StepPlan       predicted = mbx::plan_step(batch_prediction(codec, S, T, q.resident), sw, facts(1024));
    CHECK(real.form != mbx::kNoLaunch && real.form != mbx::kRaggedStep && real.form != mbx::kMixedStep);
    printf("%d %d\n", real.instance, predicted.instance);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && strcmp(argv[1], "case") == 0) {
        return run_case(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argv[5]);
    }
    const long  parsed = check_parser();
    Fnv         fnv;
    PlanDecider plan;
    walk_grid(plan, fnv);
    printf("launch_plan_check: %llu decisions, hash 0x%016llx, %ld parser cases\n", fnv.count, (unsigned long long)fnv.h, parsed);
    if (fnv.count != kParentCount || fnv.h != kParentHash) {
        fprintf(stderr, "launch_plan_check: the parent gave %llu decisions, hash 0x%016llx\n", kParentCount, (unsigned long long)kParentHash);
        return 1;
    }
    printf("launch_plan_check: ok\n");
    return 0;
}
