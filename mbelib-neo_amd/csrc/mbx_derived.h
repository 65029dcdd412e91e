// mbx_derived.h -- the tables derived from the blob on the host at mbx_init() (mbx_derive.h) and read by the kernels through
// DeviceTables::d (mbx_device.h).  Host and device: no hip_runtime.h, so that a plain host compiler sees the struct too
// (tests/derived_tables_check.cpp).
#pragma once
#include <stdint.h>

#include <hip/hip_vector_types.h>

#include "mbx_tables.h"

namespace mbx {

// Tables derived on the host at mbx_init() and kept next to the blob in HBM.
struct DerivedTables {
    uint32_t lcg_mul[161];    // 171^k mod 53125           (unvoiced-noise LCG jump-ahead)
    uint32_t lcg_add[161];    // additive term after k steps
    uint32_t lcg_pack[161];   // both in one word (each is below 53,125 < 2^16): lcg_mul[k] | lcg_add[k] << 16 -- one load per sample
    float    log2_int[64];    // log2f((float)L) from the host libm (AMBE gain term)
    // Wave-uniform quotients of the parameter decode: one scalar load each instead of a 12-instruction IEEE
    // division executed by all 64 lanes.  Made on the host with the same float expressions (correctly rounded
    // division, no contraction), so the values are the ones the device would compute.
    float    l_ratio[57][57];       // (float)prev_L / (float)cur_L
    float    imbe_rho_over_l[57];   // rho(L) / (float)L, rho = 0.4 | 0.03 L - 0.05 | 0.7 (imbe7200x4400.c log-magnitude prediction)
    float    ambe_pred_over_l[57];  // 0.65f / (float)L
    float    nfrac[192];            // (float)n / 160.0f, the interpolated branch's amplitude ramp
    uint32_t pr_mul[116];     // 173^k mod 2^16             (demodulation sequence jump-ahead, k = 0..115)
    uint32_t pr_add[116];     // additive term after k steps
    uint32_t ham_basis[11];   // Hamming(15,11) code word of data bit i (soft-decision candidates)
    uint32_t golay_rot[12];   // golay_gen[i] with its low seven bits rotated left by one (soft Golay table index, mbx_fec.hip)
    uint32_t ham7100_basis[11];   // the same for the IMBE 7100x4400 bit mapping
    // IMBE parameter expansion, per L (index L - 9) and lane: which block / position a lane owns
    uint32_t imbe_lane_map[48][64];       // hoc block | hoc index k << 3 | harmonic's block << 7 | block length << 10 | index j << 14
    float    imbe_hoc_sd[48][64];         // standdev[k - 2] of the higher-order coefficient in word lane + 8
    float    imbe_idct_rows[48][64][10];  // idct_cos[ji][j][1..10] of harmonic `lane`
    // the same per inverse-DCT block (index blk = 1..6) for the 8-lanes-per-frame expand kernel
    uint32_t imbe_blk_info[48][8];        // first word m | first harmonic l << 8 | block length << 16
    uint8_t  imbe_blk_bm[48][8][12];      // bit count of the higher-order coefficient k = 2..10 of the block (0 = none)
    float    imbe_blk_step[48][8][12];    // quantstep[Bm - 1] * standdev[k - 2] of that coefficient
    float    imbe_len_rows[11][10][10];    // idct_cos[ji][j][1..10] of output j = 1..10 of a block of LENGTH ji = 0..10 (zero past the length).
                                           // (Until round 4 a copy per (L, block): 154 KB of gathers that did not stay in L1 -- the expansion
                                           //  kernel's time was their volume.  4.4 KB by length: 24.6 -> 21.1 us for 65,536 frames.)
    uint32_t pad_len_rows[52];             // (to 18 x 256 B: the tables behind keep their alignment to cache lines)
    uint2    imbe_b0[208];                // b0 -> (w0 bits, L | K << 8): one look-up instead of three
    float    wola_inv[160];       // 1 / wola_denom[n] (0 where the reference skips the sample: denom <= 1e-10)
    float    ambep_f0[128];       // AMBE 3600x2400: exp2f(-4.311767578125f - 2.1336e-2f * (b0 + 0.5f)) from the host libm
    // Lane-parallel FEC of the one-launch T = 1 kernels (mbx_fec_frame.h, LaneFec): tables of 64 entries held ONE ENTRY PER LANE
    uint32_t golay_half_syn[64];  // entry j: (parity of the data word whose six HIGH bits are j) << 16 | (... whose six LOW bits are j):
                                  // the Golay syndrome of a code word is half_hi[data >> 6] ^ half_lo[data & 63] ^ its parity bits
    uint2    pr_lane[64];         // demodulation sequence in closed form, x_k = A_k x_0 + C_k mod 2^16: entry j = (A | C << 16) of
                                  // k = j + 1 (.x) and of k = j + 65 (.y)
    uint32_t pr_bits[4096 + 1][4];   // the demodulation sequence of every 12-bit seed, 114 bits each, big-endian: bit 31 - (k & 31) of word
                                     // k >> 5 = the sequence bit of step k + 1 (x_0 = 16 seed; bit = x >> 15); + one entry of padding
    uint32_t imbe_L_lanes[64];    // byte k of entry j: IMBE L of b0 = j + 64 k (0: no such b0 / invalid L) -- ONE dword per lane holds the
                                  // whole b0 -> L law, so a wave that asks for it before it knows b0 has L without a memory round trip
};
static_assert(sizeof(DerivedTables) == 263504, "DerivedTables is uploaded as it lies: host and device must agree on its layout");

}  // namespace mbx
