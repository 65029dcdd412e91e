// device_list_check.cpp -- the device list of the per-frame library (mbelib-neo_amd/csrc/mbe_device_list.h) against its stated rules, on
// the CPU: tests/test_device_list_host.py builds this with -fsanitize=address,undefined and runs it.  Every text is handed over in a
// heap copy of its exact length, so that a parser reading past the terminator is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "mbe_device_list.h"

namespace {

long g_case = 0;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "device_list_check: case %ld, line %d: %s\n", g_case, __LINE__, #cond);   \
            abort();                                                                                  \
        }                                                                                             \
    } while (0)

struct Parsed {
    bool             ok;
    std::vector<int> devices;
    std::string      why;
};

Parsed parse(const char* text, int device_count, int fallback) {
    ++g_case;
    char* copy = nullptr;
    if (text) {
        const size_t n = strlen(text) + 1;
        copy = static_cast<char*>(malloc(n));
        memcpy(copy, text, n);
    }
    mbx::DeviceList list;
    list.n = -7;   // a refusal leaves *out alone
    const char* why = "untouched";
    Parsed p;
    p.ok = mbx::parse_device_list(copy, device_count, fallback, &list, &why);
    free(copy);
    if (p.ok) {
        CHECK(why == nullptr);
        CHECK(list.n >= 1 && list.n <= mbx::kMaxShards);
        p.devices.assign(list.device, list.device + list.n);
    } else {
        CHECK(list.n == -7);
        CHECK(why != nullptr && strcmp(why, "untouched") != 0 && why[0] != '\0');
        p.why = why;
    }
    return p;
}

void accepted(const char* text, int device_count, int fallback, const std::vector<int>& want) {
    const Parsed p = parse(text, device_count, fallback);
    CHECK(p.ok);
    CHECK(p.devices == want);
}

std::string refused(const char* text, int device_count) {
    const Parsed p = parse(text, device_count, 0);
    CHECK(!p.ok);
    return p.why;
}

std::string zeros(int n) {   // "0,0,...,0", n entries
    std::string s;
    for (int i = 0; i < n; ++i) {
        s += i ? ",0" : "0";
    }
    return s;
}

}  // namespace

int main() {
    // unset: one shard on the fallback device, whatever the runtime counts (today's behaviour)
    accepted(nullptr, 8, 0, {0});
    accepted(nullptr, 8, 5, {5});
    accepted(nullptr, 1, 0, {0});
    accepted(nullptr, 0, 3, {3});
    // all
    accepted("all", 1, 0, {0});
    accepted("all", 2, 7, {0, 1});
    accepted("all", 8, 0, {0, 1, 2, 3, 4, 5, 6, 7});
    accepted(" all ", 2, 0, {0, 1});
    // lists: one entry, repeats (each a shard of its own), spaces around items; MBX_DEVICES wins over the fallback
    accepted("0", 1, 0, {0});
    accepted("0", 8, 5, {0});
    accepted("0,0,0,0", 1, 0, {0, 0, 0, 0});
    accepted(" 1 , 0,1", 2, 0, {1, 0, 1});
    accepted("7,3", 8, 0, {7, 3});
    accepted("007", 8, 0, {7});
    accepted(zeros(32).c_str(), 1, 0, std::vector<int>(32, 0));
    // refusals, each with a text of its own
    std::set<std::string> texts;
    const std::string empty = refused("", 8);
    CHECK(refused("   ", 8) == empty);
    texts.insert(empty);
    const std::string empty_item = refused("0,,1", 8);
    CHECK(refused(",0", 8) == empty_item);
    CHECK(refused("0,", 8) == empty_item);
    CHECK(refused("0, ,1", 8) == empty_item);
    texts.insert(empty_item);
    const std::string not_digits = refused("0,x", 8);
    CHECK(refused("-1", 8) == not_digits);
    CHECK(refused("+1", 8) == not_digits);
    CHECK(refused("1 2", 8) == not_digits);
    CHECK(refused("0x1", 8) == not_digits);
    CHECK(refused("1.0", 8) == not_digits);
    CHECK(refused("all,0", 8) == not_digits);
    CHECK(refused("ALL", 8) == not_digits);
    CHECK(refused("0;1", 8) == not_digits);
    texts.insert(not_digits);
    const std::string beyond = refused("8", 8);
    CHECK(refused("0,1,2", 2) == beyond);
    CHECK(refused("1", 1) == beyond);
    CHECK(refused("0", 0) == beyond);
    CHECK(refused("99999999999999999999999999999999999999", 8) == beyond);   // (no overflow on the way)
    texts.insert(beyond);
    const std::string too_many = refused(zeros(33).c_str(), 1);
    CHECK(refused(zeros(64).c_str(), 8) == too_many);
    CHECK(refused("all", 33) == too_many);
    texts.insert(too_many);
    const std::string no_device = refused("all", 0);
    CHECK(refused("all", -1) == no_device);
    texts.insert(no_device);
    CHECK(texts.size() == 6);
    {   // why may be NULL
        ++g_case;
        mbx::DeviceList list;
        CHECK(!mbx::parse_device_list("", 8, 0, &list, nullptr));
        CHECK(mbx::parse_device_list("0", 8, 0, &list, nullptr) && list.n == 1 && list.device[0] == 0);
    }
    // placement: a thread's home is its ordinal modulo n; the channels of a batch walk the shards from the home on, each shard once
    // in every n consecutive k
    for (int n = 1; n <= 32; ++n) {
        for (int home = 0; home < n; ++home) {
            ++g_case;
            CHECK(mbx::home_shard(home, n) == home && mbx::home_shard(home + n, n) == home && mbx::home_shard(home + 5 * n, n) == home);
            CHECK(mbx::channel_shard(home, 0, n) == home);
            for (int k = 0; k <= 4 * n; ++k) {
                const int s = mbx::channel_shard(home, k, n);
                CHECK(s >= 0 && s < n);
                if (k + n <= 4 * n + 1) {   // the window k .. k + n - 1
                    std::set<int> seen;
                    for (int j = k; j < k + n; ++j) {
                        seen.insert(mbx::channel_shard(home, j, n));
                    }
                    CHECK((int)seen.size() == n);
                }
            }
        }
    }
    printf("device_list_check: %ld cases ok\n", g_case);
    return 0;
}
