// compand_check.cpp -- host check of companded PCM out (include/mbx_pcm8.h), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_pcm8_host.py; a program of its own, nothing of it is loaded anywhere else.
// The two functions every kernel instance and the host function share (mbelib-neo_amd/csrc/mbx_compand.h: the segment from the
// leading one) over all 65,536 int16 values against a second definition written differently -- the classic G.711 search through
// the segment end points --, and against what is pinned: the FNV-1a-32 of each 65,536-byte table, eight known answers, the number
// of distinct codes, encode(decode(c)) == c for every code but mu-law 0x7F, and decode(encode(x)) non-decreasing in x.
#include <cstdint>
#include <cstdio>

#include "mbx_compand.h"

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

// ---- the second definition: the first segment whose end point is not below the magnitude -------------------------------------------
const int kUlawEnd[8] = {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF};
const int kAlawEnd[8] = {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF};

int segment_of(int value, const int* end) {
    for (int i = 0; i < 8; ++i) {
        if (value <= end[i]) {
            return i;
        }
    }
    return 8;
}

uint8_t ulaw_by_search(int x) {
    int v = x >> 2, mask = 0xFF;
    if (v < 0) {
        v = -v;
        mask = 0x7F;
    }
    if (v > 8159) {
        v = 8159;
    }
    v += 0x84 >> 2;
    const int seg = segment_of(v, kUlawEnd);
    return (uint8_t)((seg >= 8 ? 0x7F : (seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask);
}

uint8_t alaw_by_search(int x) {
    int v = x >> 3, mask = 0xD5;
    if (v < 0) {
        v = -v - 1;
        mask = 0x55;
    }
    const int seg = segment_of(v, kAlawEnd);
    if (seg >= 8) {
        return (uint8_t)(0x7F ^ mask);
    }
    return (uint8_t)(((seg << 4) | ((seg < 2 ? v >> 1 : v >> seg) & 0xF)) ^ mask);
}

// ---- the standard expanders ---------------------------------------------------------------------------------------------------------
int ulaw_expand(uint8_t byte) {
    const int u = ~byte & 0xFF;
    const int t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}

int alaw_expand(uint8_t byte) {
    const int a = byte ^ 0x55;
    const int seg = (a & 0x70) >> 4;
    int t = (a & 0x0F) << 4;
    t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
    return (a & 0x80) ? t : -t;
}

uint32_t fnv1a32(const uint8_t* p, size_t n) {
    uint32_t h = 0x811C9DC5u;
    for (size_t i = 0; i < n; ++i) {
        h = (h ^ p[i]) * 0x01000193u;
    }
    return h;
}

uint8_t table[2][65536];

}  // namespace

int main() {
    typedef uint8_t (*Encode)(int16_t);
    typedef uint8_t (*Search)(int);
    typedef int (*Expand)(uint8_t);
    const char* const name[2] = {"mu-law", "A-law"};
    const Encode encode[2] = {mbx::pcm16_to_ulaw, mbx::pcm16_to_alaw};
    const Search search[2] = {ulaw_by_search, alaw_by_search};
    const Expand expand[2] = {ulaw_expand, alaw_expand};
    const uint32_t pin[2] = {0xF2471A71u, 0x826FE2C5u};
    const int codes[2] = {255, 256};
    static const struct {
        int     x;
        uint8_t byte[2];
    } known[8] = {{-32768, {0x00, 0x2A}}, {-1000, {0x4E, 0x7A}}, {-1, {0x7E, 0x55}}, {0, {0xFF, 0xD5}},
                  {3, {0xFF, 0xD5}},      {4, {0xFE, 0xD5}},     {1000, {0xCE, 0xFA}}, {32767, {0x80, 0xAA}}};
    long checked = 0;
    for (int law = 0; law < 2; ++law) {
        bool used[256] = {};
        int before = -40000;
        for (int x = -32768; x <= 32767; ++x) {
            const uint8_t b = encode[law]((int16_t)x);
            table[law][x + 32768] = b;
            CHECK(b == search[law](x), "%s of %d: %02X, by search %02X", name[law], x, b, search[law](x));
            CHECK(b == mbx::pcm16_compand(law, (int16_t)x), "%s of %d through pcm16_compand", name[law], x);
            used[b] = true;
            const int back = expand[law](b);
            CHECK(back >= before, "%s: decode(encode(%d)) = %d after %d", name[law], x, back, before);
            before = back;
            ++checked;
        }
        const uint32_t h = fnv1a32(table[law], 65536);
        CHECK(h == pin[law], "%s table: FNV-1a-32 0x%08X, pinned 0x%08X", name[law], h, pin[law]);
        for (const auto& k : known) {
            CHECK(encode[law]((int16_t)k.x) == k.byte[law], "%s of %d: %02X, known %02X", name[law], k.x, encode[law]((int16_t)k.x), k.byte[law]);
        }
        int distinct = 0;
        for (int c = 0; c < 256; ++c) {
            distinct += used[c] ? 1 : 0;
            const int back = expand[law]((uint8_t)c);
            CHECK(back >= -32768 && back <= 32767, "%s code %02X expands to %d", name[law], c, back);
            const uint8_t again = encode[law]((int16_t)back);
            if (law == 0 && c == 0x7F) {   // the one code that does not come back: it expands to 0, and 0 is 0xFF
                CHECK(back == 0 && again == 0xFF && !used[c], "mu-law 7F: expands to %d, encodes to %02X", back, again);
            } else {
                CHECK(again == c, "%s: encode(decode(%02X)) = %02X", name[law], c, again);
            }
        }
        CHECK(distinct == codes[law], "%s uses %d codes, %d expected", name[law], distinct, codes[law]);
    }
    CHECK(mbx::compand_log2(1u) == 0 && mbx::compand_log2(33u) == 5 && mbx::compand_log2(8192u) == 13 && mbx::compand_log2(4095u) == 11, "compand_log2");
    if (failures) {
        printf("compand_check: %d FAILED\n", failures);
        return 1;
    }
    printf("compand_check: ok (%ld samples, hashes 0x%08X 0x%08X)\n", checked, fnv1a32(table[0], 65536), fnv1a32(table[1], 65536));
    return 0;
}
