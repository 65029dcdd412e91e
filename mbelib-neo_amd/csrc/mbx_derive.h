// mbx_derive.h -- what mbx_init() (mbx_api.hip) does with the table blob before a device is involved: the checks that refuse a blob,
// and the DerivedTables (mbx_derived.h) computed from an accepted one.  Pure functions over host memory: no HIP, no locks, no
// globals -- so that a CPU program can check them under a sanitizer (tests/derived_tables_check.cpp holds every table to a definition
// of its own).  Host-only and private; internal linkage, nothing here is exported.
// The float tables are made with the expressions the device would evaluate (correctly rounded division, no contraction: build
// with -ffp-contract=off); log2_int and ambep_f0 alone come from the host libm.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "mbx_derived.h"
#include "mbx_tables.h"

namespace mbx {

static inline uint32_t fnv1a(const uint8_t* p, size_t n) {
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) {
        h = (h ^ p[i]) * 16777619u;
    }
    return h;
}

// nullptr for a blob mbx_init() takes, else why it is refused (MBX_EBADTABLE)
static inline const char* check_blob(const void* table_blob, size_t table_bytes) {
    if (!table_blob || table_bytes != sizeof(mbx_tables)) {
        return "table blob: wrong size";
    }
    const mbx_tables* host = static_cast<const mbx_tables*>(table_blob);
    if (host->magic != MBX_TABLES_MAGIC || host->version != MBX_TABLES_VERSION || host->total_bytes != sizeof(mbx_tables)) {
        return "table blob: wrong magic/version";
    }
    const uint32_t sum = fnv1a(reinterpret_cast<const uint8_t*>(&host->checksum) + 4, sizeof(mbx_tables) - 16);
    if (sum != host->checksum) {
        return "table blob: checksum mismatch";
    }
    // the voiced-bank kernel relies on the shape of the synthesis window (mbx_stream.hip): zero / ramp / one / ramp / zero
    for (int k = 0; k < 321; ++k) {
        const float v = host->ws[k];
        const bool ok = (k <= 55 || k >= 265) ? (v == 0.0f) : ((k >= 105 && k <= 215) ? (v == 1.0f) : (v > 0.0f && v < 1.0f));
        if (!ok) {
            return "table blob: unexpected synthesis window shape";
        }
    }
    // the IMBE expansion scatters payload bits without looking at the entries again (mbx_expand_imbe.h): word 0..57, bit 0..11
    for (int l9 = 0; l9 < 48; ++l9) {
        for (int i = 0; i < 79; ++i) {
            if (host->imbe_bo[l9][i][0] >= 58 || host->imbe_bo[l9][i][1] >= 12) {
                return "table blob: IMBE bit-layout entry out of range";
            }
        }
    }
    return nullptr;
}

// ---- the derivation, by table family: each writes its own members of a zeroed DerivedTables ----------------------------------------

// unvoiced-noise LCG and demodulation (PR) sequence: jump-ahead pairs, the lane-held pairs, every seed's 114 bits
static inline void derive_noise_tables(DerivedTables& d) {
    uint32_t a = 1, c = 0;   // x_k = a*x_0 + c (mod 53125)
    for (int k = 0; k <= 160; ++k) {
        d.lcg_mul[k] = a;
        d.lcg_add[k] = c;
        d.lcg_pack[k] = a | (c << 16);
        a = (uint32_t)(((uint64_t)a * 171u) % 53125u);
        c = (uint32_t)(((uint64_t)c * 171u + 11213u) % 53125u);
    }
    {   // x_k = 173 x_{k-1} + 13849 (mod 2^16)  =>  x_k = pr_mul[k] x_0 + pr_add[k]
        uint32_t m = 1u, a = 0u;
        for (int k = 0; k < 116; ++k) {
            d.pr_mul[k] = m;
            d.pr_add[k] = a;
            m = (173u * m) & 0xffffu;
            a = (173u * a + 13849u) & 0xffffu;
        }
    }
    for (int j = 0; j < 64; ++j) {
        uint32_t ac[2];
        for (int half = 0; half < 2; ++half) {   // x -> 173 x + 13849 mod 2^16, k = j + 1 + 64 half times
            uint32_t a = 1, c = 0;
            for (int k = 0; k < j + 1 + 64 * half; ++k) {
                a = (a * 173u) & 0xffffu;
                c = (c * 173u + 13849u) & 0xffffu;
            }
            ac[half] = a | (c << 16);
        }
        d.pr_lane[j] = make_uint2(ac[0], ac[1]);
    }
    memset(d.pr_bits, 0, sizeof(d.pr_bits));
    for (uint32_t seed = 0; seed < 4096; ++seed) {
        uint32_t x = (16u * seed) & 0xffffu;
        for (int k = 0; k < 114; ++k) {
            x = (173u * x + 13849u) & 0xffffu;
            d.pr_bits[seed][k >> 5] |= (x >> 15) << (31 - (k & 31));
        }
    }
}

// Golay rotation and half-syndromes, the two Hamming bases; nullptr, or why the generator rows are refused (MBX_EBADTABLE)
static inline const char* derive_fec_tables(const mbx_tables* host, DerivedTables& d) {
    for (int i = 0; i < 12; ++i) {
        const uint32_t g = host->golay_gen[i];
        d.golay_rot[i] = ((g & 0x3fu) << 1) | ((g >> 6) & 1u) | (g & 0x780u);
    }
    for (int j = 0; j < 64; ++j) {
        uint32_t hi = 0, lo = 0;
        for (int i = 0; i < 6; ++i) {
            if ((j >> (5 - i)) & 1) {
                hi ^= host->golay_gen[i];
                lo ^= host->golay_gen[6 + i];
            }
        }
        d.golay_half_syn[j] = (hi << 16) | lo;
    }
    for (int variant = 0; variant < 2; ++variant) {
        // code word of data bit i: data bits at positions {2,4,5,6,8..14} (7100x4400 mapping: {4..14}), parity
        // at {0,1,3,7} ({0,1,2,3}) chosen for a zero syndrome (ref src/ecc/ecc.c:128-155)
        static const int data_pos[2][11] = {{2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14}, {4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14}};
        static const int parity_pos[2][4] = {{0, 1, 3, 7}, {0, 1, 2, 3}};
        const uint16_t* gen = variant ? host->hamming7100_gen : host->hamming_gen;
        for (int i = 0; i < 11; ++i) {
            uint32_t found = 0xffffffffu;
            for (uint32_t p = 0; p < 16u && found == 0xffffffffu; ++p) {
                uint32_t c = 1u << data_pos[variant][i];
                for (int q = 0; q < 4; ++q) {
                    c |= ((p >> q) & 1u) << parity_pos[variant][q];
                }
                int syndrome = 0;
                for (int q = 0; q < 4; ++q) {
                    syndrome |= (__builtin_popcount(c & gen[q]) & 1) << q;
                }
                if (syndrome == 0) {
                    found = c;
                }
            }
            if (found == 0xffffffffu) {
                return "mbx_init: Hamming generator rows admit no code word for a data bit";
            }
            (variant ? d.ham7100_basis : d.ham_basis)[i] = found;
        }
    }
    return nullptr;
}

// IMBE parameter expansion: the ownership law per lane and per block, their inverse-DCT rows and quantiser steps, the b0 law
static inline void derive_imbe_tables(const mbx_tables* host, DerivedTables& d) {
    for (int l9 = 0; l9 < 48; ++l9) {   // who owns what in the IMBE parameter expansion (ref src/imbe/imbe7200x4400.c:233-270)
        const uint8_t* J = host->imbe_ji[l9];
        const int L = l9 + 9;
        for (int lane = 0; lane < 64; ++lane) {
            int hblk = 1, first = 0, ji = J[0];   // higher-order coefficient of word lane + 8
            for (int q = 1; q < 6; ++q) {
                if (lane >= first + (ji - 1)) {
                    first += ji - 1;
                    hblk = q + 1;
                    ji = J[q];
                }
            }
            const int hk = lane - first + 2;
            int iblk = 1, ifirst = 1, iji = J[0];   // harmonic `lane`
            for (int q = 1; q < 6; ++q) {
                if (lane >= ifirst + iji) {
                    ifirst += iji;
                    iblk = q + 1;
                    iji = J[q];
                }
            }
            const int ij = lane - ifirst + 1;
            const bool harm = lane >= 1 && lane <= L && iji >= 1 && iji <= 10 && ij >= 1 && ij <= 10;
            d.imbe_lane_map[l9][lane] = (uint32_t)hblk | ((uint32_t)(hk & 15) << 3) | ((uint32_t)iblk << 7)
                                        | ((uint32_t)(iji & 15) << 10) | ((uint32_t)(ij & 15) << 14);
            d.imbe_hoc_sd[l9][lane] = (hk >= 2 && hk <= 10) ? host->imbe_standdev[hk - 2] : 0.0f;
            for (int k = 1; k <= 10; ++k) {
                d.imbe_idct_rows[l9][lane][k - 1] = harm ? host->imbe_idct_cos[iji][ij][k] : 0.0f;
            }
        }
    }
    for (int b0 = 0; b0 < 208; ++b0) {
        uint32_t wbits;
        memcpy(&wbits, &host->imbe_w0[b0], 4);
        d.imbe_b0[b0] = make_uint2(wbits, (uint32_t)host->imbe_L[b0] | ((uint32_t)host->imbe_K[b0] << 8));
    }
    memset(d.imbe_L_lanes, 0, sizeof(d.imbe_L_lanes));
    for (int b0 = 0; b0 < 208; ++b0) {
        d.imbe_L_lanes[b0 & 63] |= (uint32_t)host->imbe_L[b0] << (8 * (b0 >> 6));
    }
    memset(d.imbe_len_rows, 0, sizeof(d.imbe_len_rows));
    for (int ji = 1; ji <= 10; ++ji) {
        for (int j = 1; j <= ji; ++j) {
            for (int k = 1; k <= ji; ++k) {
                d.imbe_len_rows[ji][j - 1][k - 1] = host->imbe_idct_cos[ji][j][k];
            }
        }
    }
    memset(d.imbe_blk_info, 0, sizeof(d.imbe_blk_info));
    memset(d.imbe_blk_bm, 0, sizeof(d.imbe_blk_bm));
    memset(d.imbe_blk_step, 0, sizeof(d.imbe_blk_step));
    for (int l9 = 0; l9 < 48; ++l9) {   // per block: where its words / harmonics start and how its coefficients are quantised
        int m = 8, l = 1;
        for (int blk = 1; blk <= 6; ++blk) {
            const int ji = host->imbe_ji[l9][blk - 1];
            d.imbe_blk_info[l9][blk] = (uint32_t)m | ((uint32_t)l << 8) | ((uint32_t)ji << 16);
            for (int k = 2; k <= ji && k <= 10; ++k) {
                const int Bm = (m - 8 < 50) ? host->imbe_hoba[l9][m - 8] : 0;
                d.imbe_blk_bm[l9][blk][k] = (uint8_t)Bm;
                d.imbe_blk_step[l9][blk][k] = (Bm > 0 && Bm <= 11) ? (host->imbe_quantstep[Bm - 1] * host->imbe_standdev[k - 2]) : 0.0f;
                ++m;
            }
            l += ji;
        }
    }
}

// the quotients the stream kernels load instead of dividing, and the two tables from the host libm
static inline void derive_quotient_tables(const mbx_tables* host, DerivedTables& d) {
    for (int L = 1; L < 64; ++L) {
        d.log2_int[L] = log2f((float)L);
    }
    for (int p = 0; p < 57; ++p) {
        for (int c = 1; c < 57; ++c) {
            d.l_ratio[p][c] = (float)p / (float)c;
        }
    }
    for (int L = 1; L < 57; ++L) {
        const float rho = (L <= 15) ? 0.4f : ((L <= 24) ? ((0.03f * (float)L) - 0.05f) : 0.7f);
        d.imbe_rho_over_l[L] = rho / (float)L;
        d.ambe_pred_over_l[L] = (float)0.65 / (float)L;
    }
    for (int n = 0; n < 192; ++n) {
        d.nfrac[n] = (float)n / (float)160;
    }
    for (int n = 0; n < 160; ++n) {
        d.wola_inv[n] = (host->wola_denom[n] > 1e-10f) ? (1.0f / host->wola_denom[n]) : 0.0f;
    }
    for (int b0 = 0; b0 < 128; ++b0) {   // ref src/ambe/ambe3600x2400.c:238 (same expression, host libm)
        d.ambep_f0[b0] = exp2f(-4.311767578125f - (2.1336e-2f * ((float)b0 + 0.5f)));
    }
}

// every derived table of a blob that passed check_blob(); nullptr, or why the blob is refused after all (MBX_EBADTABLE)
static inline const char* derive_tables(const mbx_tables& blob, DerivedTables& d) {
    memset(&d, 0, sizeof(d));
    derive_noise_tables(d);
    derive_imbe_tables(&blob, d);
    derive_quotient_tables(&blob, d);
    return derive_fec_tables(&blob, d);
}

}  // namespace mbx
