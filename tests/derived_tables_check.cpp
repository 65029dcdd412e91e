// derived_tables_check.cpp -- what mbx_init() does before a device is involved, on the CPU: the blob checks and the derived tables of
// mbelib-neo_amd/csrc/mbx_derive.h, and the per-frame cell arithmetic of mbelib-neo_amd/csrc/mbx_cells.h.
// tests/test_derived_tables_host.py builds this with -fsanitize=address,undefined and runs it on the committed blob (argv[1]).
// Every table is held to a definition written here a second time -- stepwise recurrences, bit-by-bit sums, the blob's own entries --
// that shares no code with the header; the whole struct (less the two tables that come from the host libm) is pinned by a hash taken
// from the derivation as it stood inside mbx_init() before it moved.  The program counts its cases; the test knows the number.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mbx_cells.h"
#include "mbx_codec.h"
#include "mbx_derive.h"

namespace {

long        g_cases = 0;
const char* g_what = "";

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            fprintf(stderr, "derived_tables_check: %s, case %ld, line %d: %s\n", g_what, g_cases, __LINE__, #cond);   \
            abort();                                                                                                  \
        }                                                                                                             \
    } while (0)

// FNV-1a over the struct with log2_int and ambep_f0 zeroed, from the parent's derivation loop run on the committed blob
constexpr uint32_t kPinnedHash = 0x16F2B5C6u;

uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

uint32_t hash_bytes(const void* p, size_t n) {   // FNV-1a, 32 bits
    const uint8_t* b = static_cast<const uint8_t*>(p);
    uint32_t h = 0x811C9DC5u;
    while (n--) {
        h ^= *b++;
        h *= 0x01000193u;
    }
    return h;
}

template <class T> bool all_zero(const T& v) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(&v);
    for (size_t i = 0; i < sizeof(T); ++i) {
        if (b[i]) {
            return false;
        }
    }
    return true;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;   // fixed seed: every run checks the same arrays
uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

// ---- the blob checks ---------------------------------------------------------------------------------------------------------------
void seal(mbx_tables& t) { t.checksum = hash_bytes(reinterpret_cast<const uint8_t*>(&t.checksum) + 4, sizeof(mbx_tables) - 16); }

void refused(const std::vector<uint8_t>& blob, size_t bytes, const char* text) {
    const char* r = mbx::check_blob(blob.data(), bytes);
    CHECK(r != nullptr && strcmp(r, text) == 0);
    ++g_cases;
}

void check_blob_checks(const std::vector<uint8_t>& good) {
    g_what = "blob checks";
    CHECK(mbx::check_blob(good.data(), good.size()) == nullptr);
    ++g_cases;
    for (int delta = -4; delta <= 4; delta += 8) {
        std::vector<uint8_t> b(good);
        b.resize(delta < 0 ? good.size() - 4 : good.size() + 4, 0);
        refused(b, b.size(), "table blob: wrong size");
    }
    auto with = [&](auto&& spoil, bool reseal, const char* text) {
        std::vector<uint8_t> b(good);
        mbx_tables           t;
        memcpy(&t, b.data(), sizeof(t));
        spoil(t);
        if (reseal) {
            seal(t);
        }
        memcpy(b.data(), &t, sizeof(t));
        refused(b, b.size(), text);
    };
    with([](mbx_tables& t) { t.magic ^= 0x100u; }, false, "table blob: wrong magic/version");
    with([](mbx_tables& t) { t.ambe_dg[7] = -t.ambe_dg[7] + 1.0f; }, false, "table blob: checksum mismatch");
    with([](mbx_tables& t) { t.ws[55] = 0.5f; }, true, "table blob: unexpected synthesis window shape");    // zero class
    with([](mbx_tables& t) { t.ws[105] = 0.5f; }, true, "table blob: unexpected synthesis window shape");   // one class
    with([](mbx_tables& t) { t.ws[264] = 0.0f; }, true, "table blob: unexpected synthesis window shape");   // ramp class
    with([](mbx_tables& t) { t.imbe_bo[47][78][0] = 58; }, true, "table blob: IMBE bit-layout entry out of range");
    with([](mbx_tables& t) { t.imbe_bo[0][0][1] = 12; }, true, "table blob: IMBE bit-layout entry out of range");
}

// ---- noise LCG and demodulation sequence ----------------------------------------------------------------------------------------------
void check_noise(const mbx::DerivedTables& d) {
    g_what = "lcg";
    for (int i = 0; i < 48; ++i) {
        const uint32_t x0 = i == 0 ? 0u : (i == 1 ? 53124u : (uint32_t)(((uint64_t)i * 1109u * 977u + 7u) % 53125u));
        uint32_t x = x0;
        for (int k = 0; k <= 160; ++k) {
            CHECK(((uint64_t)d.lcg_mul[k] * x0 + d.lcg_add[k]) % 53125u == x);
            x = (171u * x + 11213u) % 53125u;
            ++g_cases;
        }
    }
    for (int k = 0; k <= 160; ++k) {
        CHECK(d.lcg_mul[k] < 53125u && d.lcg_add[k] < 53125u && d.lcg_pack[k] == (d.lcg_mul[k] | d.lcg_add[k] << 16));
        ++g_cases;
    }
    g_what = "pr";
    for (uint32_t seed = 0; seed < 4096; ++seed) {
        const uint32_t x0 = 16u * seed;
        uint32_t       x = x0;
        for (int k = 1; k <= 114; ++k) {
            x = (173u * x + 13849u) % 65536u;
            CHECK(((d.pr_mul[k] * x0 + d.pr_add[k]) & 0xffffu) == x);
            const uint32_t pair = k <= 64 ? d.pr_lane[k - 1].x : d.pr_lane[k - 65].y;
            CHECK((((pair & 0xffffu) * x0 + (pair >> 16)) & 0xffffu) == x);
            const int s = k - 1;
            CHECK(((d.pr_bits[seed][s / 32] >> (31 - s % 32)) & 1u) == x / 32768u);
            ++g_cases;
        }
        CHECK((d.pr_bits[seed][3] & 0x3fffu) == 0u);   // bits 114..127: no step
        ++g_cases;
    }
    CHECK(all_zero(d.pr_bits[4096]));
    ++g_cases;
    uint32_t A[129], C[129];   // k plain steps of x -> 173 x + 13849 applied to the identity map
    A[0] = 1u;
    C[0] = 0u;
    for (int k = 1; k <= 128; ++k) {
        A[k] = (173u * A[k - 1]) % 65536u;
        C[k] = (173u * C[k - 1] + 13849u) % 65536u;
    }
    for (int k = 0; k < 116; ++k) {
        CHECK(d.pr_mul[k] == A[k] && d.pr_add[k] == C[k]);
        ++g_cases;
    }
    for (int j = 0; j < 64; ++j) {
        CHECK(d.pr_lane[j].x == (A[j + 1] | C[j + 1] << 16) && d.pr_lane[j].y == (A[j + 65] | C[j + 65] << 16));
        ++g_cases;
    }
}

// ---- FEC --------------------------------------------------------------------------------------------------------------------------------
void check_fec(const mbx_tables& t, const mbx::DerivedTables& d) {
    g_what = "golay_half_syn";
    for (uint32_t data = 0; data < 4096; ++data) {
        uint32_t parity = 0;
        for (int bit = 0; bit < 12; ++bit) {
            if ((data >> bit) & 1u) {
                parity ^= t.golay_gen[11 - bit];   // golay_gen[i]: the parity contribution of data bit 11 - i
            }
        }
        CHECK(((d.golay_half_syn[data >> 6] >> 16) ^ (d.golay_half_syn[data & 63] & 0xffffu)) == parity);
        ++g_cases;
    }
    g_what = "golay_rot";
    for (int i = 0; i < 12; ++i) {
        uint32_t want = 0;
        for (int b = 0; b < 11; ++b) {
            if ((t.golay_gen[i] >> b) & 1u) {
                want |= 1u << (b < 7 ? (b + 1) % 7 : b);   // the low seven bits rotated left by one, bits 7..10 where they are
            }
        }
        CHECK(d.golay_rot[i] == want);
        ++g_cases;
    }
    g_what = "hamming bases";
    for (int variant = 0; variant < 2; ++variant) {
        const uint32_t  data_mask = variant ? 0x7ff0u : 0x7f74u;   // data positions {4..14} (7100x4400), {2, 4, 5, 6, 8..14}
        const uint16_t* gen = variant ? t.hamming7100_gen : t.hamming_gen;
        const uint32_t* basis = variant ? d.ham7100_basis : d.ham_basis;
        int             pos = -1;
        for (int i = 0; i < 11; ++i) {
            do {
                ++pos;
            } while (!((data_mask >> pos) & 1u));   // the i-th data position
            CHECK(basis[i] < 32768u && (basis[i] & data_mask) == 1u << pos);
            for (int q = 0; q < 4; ++q) {
                uint32_t v = basis[i] & gen[q], par = 0;
                for (; v; v >>= 1) {
                    par ^= v & 1u;
                }
                CHECK(par == 0u);
            }
            ++g_cases;
        }
    }
}

// ---- IMBE expansion: the lane form and the block form of one ownership law -----------------------------------------------------------------
void check_imbe(const mbx_tables& t, const mbx::DerivedTables& d) {
    g_what = "imbe ownership";
    for (int l9 = 0; l9 < 48; ++l9) {
        const int L = l9 + 9;
        int       sum = 0;
        for (int b = 0; b < 6; ++b) {
            sum += t.imbe_ji[l9][b];
        }
        CHECK(sum == L);
        // the block form: blocks 1..6 tile the harmonics 1..L and the higher-order words 8..
        int own[64] = {0}, blk_of[64] = {0}, j_of[64] = {0}, len_of[64] = {0};
        int word_blk[64] = {0}, word_k[64] = {0}, words = 0;
        CHECK(d.imbe_blk_info[l9][0] == 0u && d.imbe_blk_info[l9][7] == 0u);
        CHECK(all_zero(d.imbe_blk_bm[l9][0]) && all_zero(d.imbe_blk_bm[l9][7]) && all_zero(d.imbe_blk_step[l9][0]) && all_zero(d.imbe_blk_step[l9][7]));
        for (int blk = 1; blk <= 6; ++blk) {
            const uint32_t info = d.imbe_blk_info[l9][blk];
            const int      m = (int)(info & 0xffu), l = (int)((info >> 8) & 0xffu), ji = (int)(info >> 16);
            CHECK(ji == t.imbe_ji[l9][blk - 1] && ji >= 1 && ji <= 10 && m == 8 + words && l >= 1 && l + ji - 1 <= L);
            for (int j = 1; j <= ji; ++j) {
                const int h = l + j - 1;
                ++own[h];
                blk_of[h] = blk;
                j_of[h] = j;
                len_of[h] = ji;
            }
            for (int k = 0; k < 12; ++k) {
                const bool has = k >= 2 && k <= ji;
                const int  Bm = has ? t.imbe_hoba[l9][words] : 0;
                CHECK(d.imbe_blk_bm[l9][blk][k] == Bm);
                const float step = (Bm >= 1 && Bm <= 11) ? t.imbe_quantstep[Bm - 1] * t.imbe_standdev[k - 2] : 0.0f;
                CHECK(bits_of(d.imbe_blk_step[l9][blk][k]) == bits_of(step));
                if (has) {
                    word_blk[words] = blk;
                    word_k[words] = k;
                    ++words;
                }
            }
        }
        CHECK(words == L - 6);
        for (int h = 0; h < 64; ++h) {
            CHECK(own[h] == ((h >= 1 && h <= L) ? 1 : 0));
        }
        // the lane form agrees with it wherever both describe a lane: word lane + 8, harmonic `lane`
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t map = d.imbe_lane_map[l9][lane];
            const int      hblk = (int)(map & 7u), hk = (int)((map >> 3) & 15u), iblk = (int)((map >> 7) & 7u);
            const int      iji = (int)((map >> 10) & 15u), ij = (int)((map >> 14) & 15u);
            CHECK(map >> 18 == 0u);
            if (lane < words) {
                CHECK(hblk == word_blk[lane] && hk == word_k[lane]);
                CHECK(bits_of(d.imbe_hoc_sd[l9][lane]) == bits_of(t.imbe_standdev[word_k[lane] - 2]));
            }
            const bool harmonic = lane >= 1 && lane <= L;
            if (harmonic) {
                CHECK(iblk == blk_of[lane] && iji == len_of[lane] && ij == j_of[lane] && ij <= iji);
            }
            for (int k = 1; k <= 10; ++k) {
                const float want = harmonic ? t.imbe_idct_cos[len_of[lane]][j_of[lane]][k] : 0.0f;
                CHECK(bits_of(d.imbe_idct_rows[l9][lane][k - 1]) == bits_of(want));
            }
        }
        ++g_cases;
    }
    g_what = "imbe_len_rows";
    for (int ji = 0; ji <= 10; ++ji) {
        for (int j = 1; j <= 10; ++j) {
            for (int k = 1; k <= 10; ++k) {
                const float want = (j <= ji && k <= ji) ? t.imbe_idct_cos[ji][j][k] : 0.0f;
                CHECK(bits_of(d.imbe_len_rows[ji][j - 1][k - 1]) == bits_of(want));
            }
        }
        ++g_cases;
    }
    g_what = "imbe_b0";
    for (int b0 = 0; b0 < 208; ++b0) {
        CHECK(d.imbe_b0[b0].x == bits_of(t.imbe_w0[b0]) && d.imbe_b0[b0].y == (uint32_t)(t.imbe_L[b0] + 256 * t.imbe_K[b0]));
        ++g_cases;
    }
    g_what = "imbe_L_lanes";
    for (int j = 0; j < 64; ++j) {
        for (int k = 0; k < 4; ++k) {
            const int b0 = j + 64 * k;
            CHECK(((d.imbe_L_lanes[j] >> (8 * k)) & 0xffu) == (b0 < 208 ? t.imbe_L[b0] : 0u));
        }
        ++g_cases;
    }
}

// ---- quotients (bit-equal to the documented float expression) and the two libm tables -------------------------------------------------------
long ulps_apart(float a, float b) { return labs((long)bits_of(a) - (long)bits_of(b)); }   // (both positive, or zero)

void check_quotients(const mbx_tables& t, const mbx::DerivedTables& d) {
    g_what = "l_ratio";
    for (int p = 0; p < 57; ++p) {
        for (int c = 0; c < 57; ++c) {
            const float num = (float)p, den = (float)c;
            CHECK(bits_of(d.l_ratio[p][c]) == (c ? bits_of(num / den) : 0u));
            ++g_cases;
        }
    }
    g_what = "imbe_rho_over_l / ambe_pred_over_l";
    for (int L = 0; L < 57; ++L) {
        const float fl = (float)L;
        float       rho = 0.7f;
        if (L <= 15) {
            rho = 0.4f;
        } else if (L <= 24) {
            const float scaled = 0.03f * fl;
            rho = scaled - 0.05f;
        }
        CHECK(bits_of(d.imbe_rho_over_l[L]) == (L ? bits_of(rho / fl) : 0u));
        ++g_cases;
        CHECK(bits_of(d.ambe_pred_over_l[L]) == (L ? bits_of(0.65f / fl) : 0u));
        ++g_cases;
    }
    g_what = "nfrac";
    for (int n = 0; n < 192; ++n) {
        CHECK(bits_of(d.nfrac[n]) == bits_of((float)n / 160.0f));
        ++g_cases;
    }
    g_what = "wola_inv";
    for (int n = 0; n < 160; ++n) {
        const float den = t.wola_denom[n];
        CHECK(bits_of(d.wola_inv[n]) == (den > 1e-10f ? bits_of(1.0f / den) : 0u));
        ++g_cases;
    }
    g_what = "log2_int";
    CHECK(bits_of(d.log2_int[0]) == 0u);
    for (int L = 1; L < 64; ++L) {
        CHECK(ulps_apart(d.log2_int[L], (float)log2((double)L)) <= 1);
        CHECK(L == 1 || d.log2_int[L] > d.log2_int[L - 1]);
        if ((L & (L - 1)) == 0) {
            int k = 0;
            while ((1 << k) < L) {
                ++k;
            }
            CHECK(d.log2_int[L] == (float)k);
        }
        ++g_cases;
    }
    g_what = "ambep_f0";
    for (int b0 = 0; b0 < 128; ++b0) {
        const float half = (float)b0 + 0.5f;
        const float slope = 2.1336e-2f * half;
        const float arg = -4.311767578125f - slope;
        CHECK(ulps_apart(d.ambep_f0[b0], (float)exp2((double)arg)) <= 1);
        CHECK(b0 == 0 || d.ambep_f0[b0] < d.ambep_f0[b0 - 1]);
        ++g_cases;
    }
}

// ---- validate_bits and pack_rows -----------------------------------------------------------------------------------------------------------
struct Frame {   // the four codecs' cell arrays, written here a second time (mbelib-neo_amd/csrc/mbx_codec.h is what the product reads)
    int rows, stride, width[8], bytes;
};
const Frame kFrames[4] = {
    {8, 23, {23, 23, 23, 23, 15, 15, 15, 7}, 18},
    {4, 24, {24, 23, 11, 14}, 9},
    {7, 24, {19, 24, 23, 23, 15, 15, 23}, 18},
    {4, 24, {24, 23, 11, 14}, 9},
};

struct Heap {   // an allocation of exactly n bytes: one byte past it is ASan's
    char* p;
    explicit Heap(size_t n) : p(static_cast<char*>(malloc(n))) { CHECK(p != nullptr); }
    ~Heap() { free(p); }
    Heap(const Heap&) = delete;
    Heap& operator=(const Heap&) = delete;
};

void check_packed(int codec, const char* cells) {
    const Frame&         f = kFrames[codec];
    const mbx::CodecShape& sh = mbx::kCodecs[codec];
    uint8_t              want[18] = {0};
    int                  before = 0;   // mbx_wire_bit_of_cell: the widths of the rows before + (width - 1 - col), bit 7 of byte 0 first
    for (int r = 0; r < f.rows; ++r) {
        for (int col = 0; col < f.width[r]; ++col) {
            const int bit = before + (f.width[r] - 1 - col);
            if (cells[r * f.stride + col]) {
                want[bit / 8] |= (uint8_t)(0x80 >> (bit % 8));
            }
        }
        before += f.width[r];
    }
    Heap out((size_t)f.bytes);
    memset(out.p, 0xA5, (size_t)f.bytes);
    mbx::pack_rows(cells, sh.rows, sh.stride, sh.width, reinterpret_cast<uint8_t*>(out.p), sh.frame_bytes);
    CHECK(memcmp(out.p, want, (size_t)f.bytes) == 0);
    CHECK(mbx::validate_bits(cells, (size_t)(f.rows * f.stride)) == 0);
    ++g_cases;
}

void check_cells() {
    g_what = "validate_bits / pack_rows";
    for (int codec = 0; codec < 4; ++codec) {
        const Frame&           f = kFrames[codec];
        const mbx::CodecShape& sh = mbx::kCodecs[codec];
        const int              n = f.rows * f.stride;
        CHECK(sh.rows == f.rows && sh.stride == f.stride && sh.cells == n && sh.frame_bytes == f.bytes);
        for (int r = 0; r < f.rows; ++r) {
            CHECK(sh.width[r] == f.width[r]);
        }
        Heap cells((size_t)n);
        for (int i = 0; i < 4096; ++i) {
            for (int c = 0; c < n; ++c) {
                cells.p[c] = (char)(rnd() & 1u);   // (the cells that are not on the wire too)
            }
            check_packed(codec, cells.p);
        }
        memset(cells.p, 0, (size_t)n);
        check_packed(codec, cells.p);
        memset(cells.p, 1, (size_t)n);
        check_packed(codec, cells.p);
        for (int one = 0; one < n; ++one) {
            memset(cells.p, 0, (size_t)n);
            cells.p[one] = 1;
            check_packed(codec, cells.p);
        }
        for (int c = 0; c < n; ++c) {
            cells.p[c] = (char)(rnd() & 1u);
        }
        static const uint8_t bad[3] = {2, 0x80, 0xFF};
        for (int at = 0; at < n; ++at) {   // every cell, on the wire or not
            for (int b = 0; b < 3; ++b) {
                const char keep = cells.p[at];
                cells.p[at] = (char)bad[b];
                CHECK(mbx::validate_bits(cells.p, (size_t)n) == MBE_STATUS_INVALID_BITS);
                cells.p[at] = keep;
                ++g_cases;
            }
        }
    }
    static const int counts[5] = {1, 7, 15, 23, 49};   // not multiples of eight: the tail loop, alone and behind whole words
    static const uint8_t bad[3] = {2, 0x80, 0xFF};
    for (int ci = 0; ci < 5; ++ci) {
        const int n = counts[ci];
        Heap      bits((size_t)n);
        for (int c = 0; c < n; ++c) {
            bits.p[c] = (char)(rnd() & 1u);
        }
        CHECK(mbx::validate_bits(bits.p, (size_t)n) == 0);
        ++g_cases;
        for (int at = 0; at < n; ++at) {
            for (int b = 0; b < 3; ++b) {
                const char keep = bits.p[at];
                bits.p[at] = (char)bad[b];
                CHECK(mbx::validate_bits(bits.p, (size_t)n) == MBE_STATUS_INVALID_BITS);
                bits.p[at] = keep;
                ++g_cases;
            }
        }
    }
    CHECK(mbx::validate_bits(nullptr, 8) == MBE_STATUS_INVALID_ARGUMENT);
    ++g_cases;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: derived_tables_check <mbx_tables.bin>\n");
        return 2;
    }
    std::vector<uint8_t> blob;
    FILE*                f = fopen(argv[1], "rb");
    CHECK(f != nullptr);
    for (int ch; (ch = fgetc(f)) != EOF;) {
        blob.push_back((uint8_t)ch);
    }
    fclose(f);
    check_blob_checks(blob);

    mbx_tables* t = new mbx_tables;   // (exact heap allocations, both)
    memcpy(t, blob.data(), sizeof(*t));
    mbx::DerivedTables* d = new mbx::DerivedTables;
    memset(static_cast<void*>(d), 0xA5, sizeof(*d));   // derive_tables() owes every byte, padding included
    g_what = "derive_tables";
    CHECK(mbx::derive_tables(*t, *d) == nullptr);
    {   // a parity-check row without a parity position: data bit 0 of the first mapping can have no code word
        const uint16_t keep = t->hamming_gen[0];
        t->hamming_gen[0] = 1u << 2;
        const char* r = mbx::derive_tables(*t, *d);
        CHECK(r != nullptr && strcmp(r, "mbx_init: Hamming generator rows admit no code word for a data bit") == 0);
        ++g_cases;
        t->hamming_gen[0] = keep;
        CHECK(mbx::derive_tables(*t, *d) == nullptr);
    }
    check_noise(*d);
    check_fec(*t, *d);
    check_imbe(*t, *d);
    check_quotients(*t, *d);

    g_what = "hash";
    const uint32_t whole = hash_bytes(d, sizeof(*d));
    CHECK(all_zero(d->pad_len_rows));
    ++g_cases;
    memset(d->log2_int, 0, sizeof(d->log2_int));
    memset(d->ambep_f0, 0, sizeof(d->ambep_f0));
    const uint32_t pinned = hash_bytes(d, sizeof(*d));
    printf("derived_tables_check: whole struct 0x%08X, without the libm tables 0x%08X\n", whole, pinned);
    CHECK(pinned == kPinnedHash);
    ++g_cases;
    delete d;
    delete t;

    check_cells();
    printf("derived_tables_check: %ld cases ok\n", g_cases);
    return 0;
}
