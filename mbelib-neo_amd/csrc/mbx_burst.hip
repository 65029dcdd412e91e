// mbx_burst.hip -- burst input (include/mbx_burst.h): the caller's de-interleave schedule, folded once on the host into two tables,
// and the gather kernels that apply them to every burst on the device: received bursts -> packed wire frames (hard) or the
// reference's cell arrays (soft), i.e. what the batch launchers of mbx_api.hip start from.  One kernel template per kind,
// burst_gather_kernel<form, invert> and burst_gather_soft_kernel<cell, flip>, serves every form a receiver holds its bursts in --
// packed bits, one byte per bit, one byte per dibit; soft per-bit cells, soft {dibit, reliability} pairs, one signed LLR per bit as
// int16 or int8 (converted in the gather: mbx_llr_cell.h) -- with or without a fixed inversion sequence.  The launchers that chain a gather in
// front of a batch step are in mbx_api.hip (they need the stream's workspace), the session submits in mbx_session.hip.
// Burst groups (include/mbx_burst_groups.h): burst_gather_groups_kernel and burst_gather_soft_groups_kernel run the same bodies over
// the bursts of up to eight schedules in ONE launch and write the layout words of the mixed step behind it.
//
// No air-interface table is written here: F, B, the strides and the tables are kernel arguments, one code object serves every
// schedule.  The frame shapes come from the one table in mbx_codec.h (through mbx_wire_bit_of_cell for the wire order).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "mbx.h"
#include "mbx_burst.h"
#include "mbx_codec.h"
#include "mbx_gather.h"
#include "mbx_host.h"
#include "mbx_kernels.h"
#include "mbx_llr_cell.h"

namespace mbx {

constexpr int      kGatherBursts = 64;     // hard gather: bursts per workgroup, one per lane of every wave
constexpr int      kSoftStageBytes = 32768;   // soft gather: a workgroup stages at most this much of soft bursts (and at most 16 bursts)
constexpr uint32_t kNoBit = 0xffffu;       // table entry of a frame bit / cell no received bit goes to
constexpr int      kSoftDibitBursts = 32;  // soft gather of dibit pairs: half the bytes per burst, twice the bursts of a workgroup at most
constexpr int      kSoftLlr8Bursts = 32;   // soft gather of int8 LLRs: likewise
constexpr uint32_t kInverted = 0x8000u;    // cell table: the received bit arrives inverted (entries are below MBX_BURST_MAX_BITS = 0x1000) ...
constexpr uint32_t kBitOf = 0x0fffu;       // ... and the received bit of an entry

// ---- hard bursts -> packed wire frames ---------------------------------------------------------------------------------------------
// A workgroup takes 64 consecutive bursts.  Their bytes go to LDS with coalesced loads (dwords when pointer and stride allow, bytes
// otherwise), burst j at j * lstride with lstride / 4 ODD: lane j of every wave then works on burst j, all lanes on the SAME
// received bit at a time, and the 32 lanes of a half hit 32 different banks.  Which bit that is comes from the schedule's table
// (wire bit -> burst bit, in LDS): one 16-bit read by eight lanes fetches the eight entries of an output byte, v_readlane makes
// each a scalar, so per bit a lane does one address add, one LDS byte read and a shift-and-merge.  The output bytes of the 64 bursts
// are collected in LDS as the image of the rows and leave as whole aligned dwords across the workgroup (single bytes only where a
// dword is not wholly inside a frame: the edges of the row range, the upper halves of 18-byte AMBE rows).
//   kForm      the form the bursts come in (MBX_BURST_FORM_*).  The working set is the PACKED image of the 64 bursts whatever the
//              form, so table, lstride and dynamic LDS do not depend on it: BITS and DIBITS bursts are converted WHILE they are
//              staged.  Four dibit bytes, one aligned dword, are exactly one packed byte, eight bit bytes are one: a lane makes a
//              whole LDS dword from 16 B (DIBITS) or 32 B (BITS) of its burst, neighbouring lanes from neighbouring pieces; the
//              four (two) bit fields of a dword are brought together by one multiplication.  Input dwords are read up to the one
//              that holds the burst's last byte (inside the stride: pointer and stride are multiples of 4 on this path); with any
//              other pointer or stride a lane builds one packed byte from its 4 / 8 input bytes, and reads none behind the burst's
//              last.  Of a BITS byte `& 1` counts, of a DIBITS byte `& 3`.
//   kInvert    the inversion sequence is applied, folded per OUTPUT byte: one XOR with xor_tab[item] per eight bits.  Without it
//              xor_tab is not read.  (Only a PACKED schedule is launched without: BITS and DIBITS read their table, zero or not.)
//   wire_tab   [F][fbytes * 8] burst bit of each wire bit, kNoBit for the bits that pad the last byte
//   xor_tab    [F * fbytes] a 1 where the wire bit's received bit arrives inverted (0 for the bits that pad the last byte)
//   lstride    bytes between two bursts in LDS
// dynamic LDS: table | 64 * lstride | 64 * F * fbytes
// (the body: `block` is the workgroup's place among those of ITS bursts -- blockIdx.x in burst_gather_kernel, the place inside its
// group in burst_gather_groups_kernel)
template <int kForm, bool kInvert>
__device__ __forceinline__ void
burst_gather_body(const uint8_t* __restrict__ bursts, size_t burst_stride, size_t n, int F, int B, int fbytes,
                  const uint16_t* __restrict__ wire_tab, const uint8_t* __restrict__ xor_tab, uint8_t* __restrict__ frames,
                  int frame_stride, int lstride, unsigned block) {
    static_assert(kInvert || kForm == MBX_BURST_FORM_PACKED, "not an instance that mbx::burst_gather launches");
    extern __shared__ uint32_t lds[];
    const int items = F * fbytes;   // output bytes of one burst; eight table entries each
    const int tab_dwords = items * 4;
    const uint16_t* tab = reinterpret_cast<const uint16_t*>(lds);
    uint8_t* in = reinterpret_cast<uint8_t*>(lds + tab_dwords);
    uint8_t* out = in + kGatherBursts * lstride;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t first = (size_t)block * kGatherBursts;
    const int here = (int)((n - first) < (size_t)kGatherBursts ? (n - first) : (size_t)kGatherBursts);
    for (int i = tid; i < tab_dwords; i += 256) {
        lds[i] = reinterpret_cast<const uint32_t*>(wire_tab)[i];
    }
    // stage the packed image of the bursts
    const int bbytes = (B + 7) >> 3;   // of the packed image
    const int nin = kForm == MBX_BURST_FORM_BITS ? B : (kForm == MBX_BURST_FORM_DIBITS ? B >> 1 : bbytes);   // bytes of a burst as it comes
    const uint8_t* src = bursts + first * burst_stride;
    if (((reinterpret_cast<uintptr_t>(bursts) | burst_stride) & 3u) == 0) {
        const int dw = (bbytes + 3) >> 2;
        const int nidw = (nin + 3) >> 2;   // (burst_stride is a multiple of 4 and >= nin: the last dword is inside the burst's stride)
        for (int j = wave; j < here; j += 4) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (size_t)j * burst_stride);
            uint32_t* d = reinterpret_cast<uint32_t*>(in + j * lstride);
            for (int i = lane; i < dw; i += 64) {
                if constexpr (kForm == MBX_BURST_FORM_PACKED) {
                    d[i] = s[i];
                } else {
                    uint32_t word = 0;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {   // packed byte m of the dword: bits 32 i + 8 m .. + 7 of the burst
                        uint32_t byte;
                        if constexpr (kForm == MBX_BURST_FORM_DIBITS) {
                            const int k = 4 * i + m;
                            const uint32_t w = k < nidw ? s[k] : 0u;
                            byte = ((w & 0x03030303u) * 0x40100401u) >> 24;   // d0 << 6 | d1 << 4 | d2 << 2 | d3: no field meets another
                        } else {
                            const int k = 8 * i + 2 * m;
                            const uint32_t w0 = k < nidw ? s[k] : 0u, w1 = k + 1 < nidw ? s[k + 1] : 0u;
                            byte = ((((w0 & 0x01010101u) * 0x08040201u) >> 24) << 4) | (((w1 & 0x01010101u) * 0x08040201u) >> 24);
                        }
                        word |= byte << (8 * m);
                    }
                    d[i] = word;
                }
            }
        }
    } else {
        constexpr int kPer = kForm == MBX_BURST_FORM_BITS ? 8 : (kForm == MBX_BURST_FORM_DIBITS ? 4 : 1);   // input bytes of a packed byte
        for (int j = wave; j < here; j += 4) {
            const uint8_t* s = src + (size_t)j * burst_stride;
            for (int i = lane; i < bbytes; i += 64) {
                uint32_t byte = 0;
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    const int q = i * kPer + k;
                    const uint32_t v = q < nin ? s[q] : 0u;
                    byte = kForm == MBX_BURST_FORM_BITS ? (byte << 1) | (v & 1u) : (kForm == MBX_BURST_FORM_DIBITS ? (byte << 2) | (v & 3u) : v);
                }
                in[j * lstride + i] = (uint8_t)byte;
            }
        }
    }
    __syncthreads();
    // gather the bytes of the rows: lane = burst (lanes behind `here` work on stale LDS bytes; their rows are not written out)
    const uint8_t* mine = in + lane * lstride;
    for (int item = wave; item < items; item += 4) {
        const uint32_t e = tab[item * 8 + (lane & 7)];
        uint32_t flips = 0;
        if constexpr (kInvert) {
            flips = xor_tab[item];
        }
        uint32_t byte = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)e, k);
            uint32_t bit = 0;
            if (j != kNoBit) {
                bit = ((uint32_t)mine[j >> 3] >> (7u - (j & 7u))) & 1u;
            }
            byte = (byte << 1) | bit;
        }
        out[lane * items + item] = (uint8_t)(byte ^ flips);
    }
    __syncthreads();
    // store rows first * F .. (first + here) * F - 1; out[row * fbytes + b] is byte b of the row
    uint8_t* dst = frames + first * (size_t)F * (size_t)frame_stride;
    const int region = (here * F - 1) * frame_stride + fbytes;   // from dst to behind the last byte written
    const int a = (int)(reinterpret_cast<uintptr_t>(dst) & 3u);
    const int ndw = (a + region + 3) >> 2;
    for (int m = tid; m < ndw; m += 256) {
        uint32_t word = 0, valid = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * m + k - a;
            if (q >= 0 && q < region) {
                // (frame_stride is the codec's frame size or the mixed row: 9 or 18, divisions by constants)
                const uint32_t row = frame_stride == MBX_AMBE_FRAME_BYTES ? (uint32_t)q / (uint32_t)MBX_AMBE_FRAME_BYTES : (uint32_t)q / (uint32_t)MBX_IMBE_FRAME_BYTES;
                const uint32_t off = (uint32_t)q - row * (uint32_t)frame_stride;
                if (off < (uint32_t)fbytes) {
                    word |= (uint32_t)out[row * (uint32_t)fbytes + off] << (8 * k);
                    valid |= 1u << k;
                }
            }
        }
        uint8_t* p = dst + (4 * m - a);
        if (valid == 15u) {
            *reinterpret_cast<uint32_t*>(p) = word;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (valid & (1u << k)) {
                    p[k] = (uint8_t)(word >> (8 * k));
                }
            }
        }
    }
}

template <int kForm, bool kInvert>
__global__ void __launch_bounds__(256)
burst_gather_kernel(const uint8_t* __restrict__ bursts, size_t burst_stride, size_t n, int F, int B, int fbytes,
                    const uint16_t* __restrict__ wire_tab, const uint8_t* __restrict__ xor_tab, uint8_t* __restrict__ frames,
                    int frame_stride, int lstride) {
    burst_gather_body<kForm, kInvert>(bursts, burst_stride, n, F, B, fbytes, wire_tab, xor_tab, frames, frame_stride, lstride, blockIdx.x);
}

// ---- soft bursts -> cell arrays ----------------------------------------------------------------------------------------------------
// A workgroup takes nb consecutive bursts (a contiguous range of staged cells, C per burst) into LDS as they come, with dword loads
// from the first aligned dword on, then every wave takes rows of the output: a lane owns the two cells of one aligned output dword,
// looks each up in the schedule's table (cell -> burst bit, in LDS), fetches it with one LDS read and stores the pair; cells
// without a received bit, and the cells of a mixed row behind the codec's array, are {0, 0}.
//   kCell      what a staged cell is (SoftCell, mbx_kernels.h):
//              kCellBit    one of C = B per-bit {bit, reliability} cells, 16 bits.
//              kCellDibit  a {dibit, reliability} pair, C = B / 2 of them per burst -- half the bytes, so up to kSoftDibitBursts
//                          bursts per workgroup.  Entry j gives pair j >> 1 as
//                          ((dibit >> (1 - (j & 1))) & 1) ^ flip | reliability << 8, i.e. of a dibit `& 3` counts.
//              kCellLlr16  one of C = B signed 16-bit LLRs, staged like per-bit cells; entry j gives soft_cell_from_llr(LLR j)
//                          (mbx_llr_cell.h) with the hard decision flipped where the entry carries kInverted.
//              kCellLlr8   one of C = B signed 8-bit LLRs: a staged piece is ONE byte -- half the bytes, up to kSoftLlr8Bursts
//                          bursts per workgroup -- so the range starts at any of four byte phases (16-bit cells: two); the LDS
//                          image keeps the source's dword alignment all the same.  One 8-bit LDS read per entry, then as LLR16.
//   kFlip      the table's entries carry kInverted where the received bit arrives inverted: per-bit cells give cell j with its
//              hard decision flipped.  Without it an entry is the received bit alone (a schedule without a sequence has no such
//              entry) and the fetch is the plain read of cell j: no mask, no shift.  (Only per-bit cells are launched without.)
//   cell_tab   [F][cells] burst bit of each cell of the reference's array, kNoBit for a cell that is not on the wire
// dynamic LDS: table | nb * C staged cells (+ one dword of slack for the alignment phase)
template <SoftCell kCell, bool kFlip>
__device__ __forceinline__ void
burst_gather_soft_body(const mbe_soft_bit* __restrict__ soft, size_t n, int F, int C, int cells, const uint16_t* __restrict__ cell_tab,
                       mbe_soft_bit* __restrict__ rows_out, int row_cells, int nb, unsigned block) {
    static_assert(kFlip || kCell == kCellBit, "not an instance that mbx::burst_gather launches");
    extern __shared__ uint32_t lds[];
    const int tab_dwords = (F * cells) >> 1;   // (every codec has an even number of cells)
    const uint16_t* tab = reinterpret_cast<const uint16_t*>(lds);
    uint16_t* in16 = reinterpret_cast<uint16_t*>(lds + tab_dwords);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t first = (size_t)block * (size_t)nb;
    const int here = (int)((n - first) < (size_t)nb ? (n - first) : (size_t)nb);
    for (int i = tid; i < tab_dwords; i += 256) {
        lds[i] = reinterpret_cast<const uint32_t*>(cell_tab)[i];
    }
    // staged cell i of the range sits at in[i + head] (Piece: what a staged cell is read as): an aligned dword of the source is an
    // aligned dword of LDS
    using Piece = std::conditional_t<kCell == kCellLlr8, uint8_t, uint16_t>;
    const Piece* in = reinterpret_cast<const Piece*>(in16);
    int head;
    if constexpr (kCell == kCellLlr8) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(soft) + first * (size_t)C;
        const int ncells = here * C;
        uint8_t* in8 = reinterpret_cast<uint8_t*>(in16);
        head = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
        const int lead = (4 - head) & 3;   // bytes in front of the first aligned dword ...
        const int edge = lead < ncells ? lead : ncells;   // ... as far as the range has them
        const int ndw = (ncells - edge) >> 2;
        const int tail = edge + 4 * ndw;   // the bytes behind the last whole dword: fewer than four
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + edge);   // (aligned wherever ndw > 0: then edge == lead)
        uint32_t* d32 = reinterpret_cast<uint32_t*>(in8 + head + edge);
        for (int m = tid; m < ndw; m += 256) {
            d32[m] = s32[m];
        }
        if (tid < edge) {
            in8[head + tid] = src[tid];
        } else if (tid >= 4 && tid - 4 < ncells - tail) {
            in8[head + tail + tid - 4] = src[tail + tid - 4];
        }
    } else {
        const uint16_t* src = reinterpret_cast<const uint16_t*>(soft) + first * (size_t)C;
        const int ncells = here * C;
        head = (int)((reinterpret_cast<uintptr_t>(src) >> 1) & 1u);
        const int ndw = (ncells - head) >> 1;
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + head);
        uint32_t* d32 = reinterpret_cast<uint32_t*>(in16) + head;
        for (int m = tid; m < ndw; m += 256) {
            d32[m] = s32[m];
        }
        if (tid == 0) {
            if (head) {
                in16[head] = src[0];
            }
            if ((ncells - head) & 1) {
                in16[ncells - 1 + head] = src[ncells - 1];
            }
        }
    }
    __syncthreads();
    const auto fetch = [](const Piece* b, uint32_t e) -> uint32_t {
        if constexpr (!kFlip) {
            return b[e];
        } else {
            const uint32_t j = e & kBitOf, flip = e >> 15;
            if constexpr (kCell == kCellDibit) {
                const uint32_t c = b[j >> 1];
                return ((((c & 0xffu) >> (1u - (j & 1u))) & 1u) ^ flip) | (c & 0xff00u);
            } else if constexpr (kCell == kCellLlr16) {
                return soft_cell_from_llr((int16_t)b[j]) ^ flip;
            } else if constexpr (kCell == kCellLlr8) {
                return soft_cell_from_llr((int8_t)b[j]) ^ flip;
            } else {
                return (uint32_t)b[j] ^ flip;
            }
        }
    };
    const int nrows = here * F;
    uint16_t* dst = reinterpret_cast<uint16_t*>(rows_out) + first * (size_t)F * (size_t)row_cells;
    const int a = (int)((reinterpret_cast<uintptr_t>(dst) >> 1) & 1u);   // (row_cells is even: every row has the phase of the first)
    const int pairs = (row_cells + 1 + a) >> 1;
    for (int r = wave; r < nrows; r += 4) {
        const int j = r / F, k = r - j * F;
        const uint16_t* t = tab + k * cells;
        const Piece* b = in + head + j * C;
        uint16_t* o = dst + (size_t)r * (size_t)row_cells;
        for (int p = lane; p < pairs; p += 64) {
            const int c0 = 2 * p - a, c1 = c0 + 1;
            uint32_t v0 = 0, v1 = 0;
            if (c0 >= 0 && c0 < cells) {
                const uint32_t e = t[c0];
                if (e != kNoBit) {
                    v0 = fetch(b, e);
                }
            }
            if (c1 < cells) {
                const uint32_t e = t[c1];
                if (e != kNoBit) {
                    v1 = fetch(b, e);
                }
            }
            if (c0 >= 0 && c1 < row_cells) {
                *reinterpret_cast<uint32_t*>(o + c0) = v0 | (v1 << 16);
            } else if (c0 >= 0) {
                o[c0] = (uint16_t)v0;
            } else {
                o[c1] = (uint16_t)v1;
            }
        }
    }
}

template <SoftCell kCell, bool kFlip>
__global__ void __launch_bounds__(256)
burst_gather_soft_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, int F, int C, int cells, const uint16_t* __restrict__ cell_tab,
                         mbe_soft_bit* __restrict__ rows_out, int row_cells, int nb) {
    burst_gather_soft_body<kCell, kFlip>(soft, n, F, C, cells, cell_tab, rows_out, row_cells, nb, blockIdx.x);
}

// ---- burst groups: the bursts of several schedules in one launch (include/mbx_burst_groups.h) ----------------------------------------
// The grid is the concatenation of the groups' workgroups.  A workgroup finds its group with a scalar loop over the (at most eight)
// first-workgroup values of the descriptors in the kernel arguments, then enters that group's instance of the body above by a scalar
// branch, as mixed_stream_kernel_ragged picks its codec body; its rows are written at the mixed row size from the group's first row.
// Dynamic LDS is the largest group's.  The same launch writes the layout words of the mixed step behind it into the workspace, with
// vector stores: the lanes that own a stream's FIRST burst write that stream's frame_offset, stream_index and stream_codec, the last
// workgroup writes frame_offset[S].  (Every stream has a first burst and every burst a lane: each word is written exactly once.)
__device__ __forceinline__ int group_of_workgroup(const GatherGroups& d) {
    int g = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        if (i < d.count && blockIdx.x >= d.g[i].first_wg) {
            g = i;
        }
    }
    return __builtin_amdgcn_readfirstlane(g);
}
// `per_wg`: bursts a workgroup of this group takes
__device__ __forceinline__ void write_group_layout(const GatherGroups& d, const GatherGroup& e, unsigned block, int per_wg) {
    const int tid = (int)threadIdx.x;
    if (tid < per_wg) {
        const uint32_t burst = block * (uint32_t)per_wg + (uint32_t)tid;
        if (burst < e.n) {
            const uint32_t j = burst / (uint32_t)e.bursts_per_stream;
            if (burst == j * (uint32_t)e.bursts_per_stream) {
                const int s = e.first_stream + (int)j;
                d.frame_offset[s] = e.first_row + (int)(burst * (uint32_t)e.F);
                d.stream_index[s] = e.index ? e.index[j] : e.first_slot + (int)j;
                d.stream_codec[s] = (uint8_t)e.codec;
            }
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        d.frame_offset[d.S] = d.total;
    }
}

__global__ void __launch_bounds__(256) burst_gather_groups_kernel(GatherGroups d, uint8_t* __restrict__ rows) {
    const GatherGroup& e = d.g[group_of_workgroup(d)];
    const unsigned block = blockIdx.x - e.first_wg;
    write_group_layout(d, e, block, kGatherBursts);
    const uint8_t* in = static_cast<const uint8_t*>(e.in);
    uint8_t* out = rows + (size_t)e.first_row * (size_t)MBX_MIXED_ROW_BYTES;
#define MBX_GROUP_HARD(form, invert) \
    burst_gather_body<form, invert>(in, e.stride, (size_t)e.n, e.F, e.B, e.unit, e.tab, e.xor_tab, out, MBX_MIXED_ROW_BYTES, e.per, block)
    switch (e.instance) {
    case kHardPacked: MBX_GROUP_HARD(MBX_BURST_FORM_PACKED, false); break;
    case kHardPackedInvert: MBX_GROUP_HARD(MBX_BURST_FORM_PACKED, true); break;
    case kHardBits: MBX_GROUP_HARD(MBX_BURST_FORM_BITS, true); break;
    default: MBX_GROUP_HARD(MBX_BURST_FORM_DIBITS, true); break;
    }
#undef MBX_GROUP_HARD
}

__global__ void __launch_bounds__(256) burst_gather_soft_groups_kernel(GatherGroups d, mbe_soft_bit* __restrict__ rows) {
    const GatherGroup& e = d.g[group_of_workgroup(d)];
    const unsigned block = blockIdx.x - e.first_wg;
    write_group_layout(d, e, block, e.per);
    const mbe_soft_bit* in = static_cast<const mbe_soft_bit*>(e.in);
    mbe_soft_bit* out = rows + (size_t)e.first_row * (size_t)MBX_MIXED_ROW_CELLS;
#define MBX_GROUP_SOFT(cell, flip) \
    burst_gather_soft_body<cell, flip>(in, (size_t)e.n, e.F, e.staged, e.unit, e.tab, out, MBX_MIXED_ROW_CELLS, e.per, block)
    switch (e.instance) {
    case kSoftBit: MBX_GROUP_SOFT(kCellBit, false); break;
    case kSoftBitFlip: MBX_GROUP_SOFT(kCellBit, true); break;
    case kSoftDibit: MBX_GROUP_SOFT(kCellDibit, true); break;
    case kSoftLlr16: MBX_GROUP_SOFT(kCellLlr16, true); break;
    default: MBX_GROUP_SOFT(kCellLlr8, true); break;
    }
#undef MBX_GROUP_SOFT
}

}  // namespace mbx

// ---- the schedule (host) -----------------------------------------------------------------------------------------------------------
struct mbx_burst_schedule {
    mbx::BurstShape shape;
    int       lstride = 0;      // hard gather: bytes between two bursts in LDS (a whole, odd number of dwords)
    unsigned  hard_lds = 0;     // dynamic LDS of the two kernels
    int       soft_bursts = 0;  // soft gather: bursts per workgroup
    int       staged_cells = 0; // soft gather: staged cells of one burst (cells, dibit pairs or LLRs)
    unsigned  soft_lds = 0;
    uint16_t* d_wire_tab = nullptr;   // [frames][frame_bytes * 8]
    uint16_t* d_cell_tab = nullptr;   // [frames][cells], kInverted on the inverted bits; the same allocation, behind the wire table
    uint8_t*  d_xor_tab = nullptr;    // [frames * frame_bytes] the inversion sequence per output byte; the same allocation, behind the cell table
    bool      inverts = false;        // the inversion sequence has a 1 on a bit that an entry names
};

namespace {

int refuse(const char* why) { return mbx::refuse("mbx_burst_schedule_create", why); }

using mbx::ready_device;

// the argument list of each kind, once
template <int kForm, bool kInvert>
void launch_hard(const mbx_burst_schedule* s, const uint8_t* in, size_t burst_stride, size_t n, uint8_t* out, int frame_stride, hipStream_t strm) {
    const mbx::BurstShape& sh = s->shape;
    const unsigned grid = (unsigned)((n + mbx::kGatherBursts - 1) / mbx::kGatherBursts);
    hipLaunchKernelGGL((mbx::burst_gather_kernel<kForm, kInvert>), dim3(grid), dim3(256), s->hard_lds, strm, in, burst_stride, n, sh.frames, sh.bits,
                       (int)sh.frame_bytes, s->d_wire_tab, s->d_xor_tab, out, frame_stride, s->lstride);
}

template <mbx::SoftCell kCell, bool kFlip>
void launch_soft(const mbx_burst_schedule* s, const mbe_soft_bit* in, size_t n, mbe_soft_bit* out, int row_cells, hipStream_t strm) {
    const mbx::BurstShape& sh = s->shape;
    const unsigned grid = (unsigned)((n + (size_t)s->soft_bursts - 1) / (size_t)s->soft_bursts);
    hipLaunchKernelGGL((mbx::burst_gather_soft_kernel<kCell, kFlip>), dim3(grid), dim3(256), s->soft_lds, strm, in, n, sh.frames, s->staged_cells,
                       (int)sh.cells, s->d_cell_tab, out, row_cells, s->soft_bursts);
}

}  // namespace

namespace mbx {

BurstShape burst_shape(const mbx_burst_schedule* sched) { return sched->shape; }

int burst_gather(const mbx_burst_schedule* sched, bool soft, const void* d_in, size_t burst_stride, size_t n, void* d_out, size_t row,
                 void* stream) {
    // the nine instances, by (soft, form, inverts): BITS and DIBITS bursts always read their inversion table, dibit pairs and LLRs
    // always look for kInverted; a packed schedule (soft: a per-bit one) does so only where its sequence inverts a bit
    const int form = sched->shape.form;
    const bool inverts = sched->inverts;
    if (soft) {
        const auto launch = form == MBX_BURST_FORM_LLR16    ? launch_soft<kCellLlr16, true>
                            : form == MBX_BURST_FORM_LLR8   ? launch_soft<kCellLlr8, true>
                            : form == MBX_BURST_FORM_DIBITS ? launch_soft<kCellDibit, true>
                            : inverts                       ? launch_soft<kCellBit, true>
                                                            : launch_soft<kCellBit, false>;
        launch(sched, static_cast<const mbe_soft_bit*>(d_in), n, static_cast<mbe_soft_bit*>(d_out), (int)row, (hipStream_t)stream);
    } else {
        const auto launch = form == MBX_BURST_FORM_DIBITS ? launch_hard<MBX_BURST_FORM_DIBITS, true>
                            : form == MBX_BURST_FORM_BITS ? launch_hard<MBX_BURST_FORM_BITS, true>
                            : inverts                     ? launch_hard<MBX_BURST_FORM_PACKED, true>
                                                          : launch_hard<MBX_BURST_FORM_PACKED, false>;
        launch(sched, static_cast<const uint8_t*>(d_in), burst_stride, n, static_cast<uint8_t*>(d_out), (int)row, (hipStream_t)stream);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_failed("", soft ? "the soft burst gather" : "the burst gather", e);
}

int burst_gather_per_workgroup(const mbx_burst_schedule* sched, bool soft) { return soft ? sched->soft_bursts : kGatherBursts; }
unsigned burst_gather_lds(const mbx_burst_schedule* sched, bool soft) { return soft ? sched->soft_lds : sched->hard_lds; }

int burst_groups_plan(const char* who, const mbx_burst_group* groups, int n_groups, bool soft, GroupShape* shapes, GroupPlan* plan) {
    const auto refused = [&](const char* why) { return mbx::refuse(who, why); };
    if (n_groups < 0 || n_groups > MBX_BURST_MAX_GROUPS) {
        return refused(group_refusal_text(kGroupCount));
    }
    if (n_groups > 0 && !groups) {
        return refused("groups is NULL");
    }
    for (int i = 0; i < n_groups; ++i) {
        const mbx_burst_group& g = groups[i];
        // (counts and alignment first: they need no schedule -- of one only whether its soft bursts are int8 LLRs)
        if (g.n_streams < 0) {
            return refused(group_refusal_text(kGroupNegative));
        }
        if (g.bursts_per_stream < 1) {
            return refused(group_refusal_text(kGroupBurstsPer));
        }
        // (of a group without streams neither pointer is looked at)
        if (g.n_streams > 0 && (!aligned_to(g.bursts, soft ? (g.sched ? g.sched->shape.soft_align() : 2) : 1) || !aligned_to(g.stream_index, 4))) {
            return misaligned(who, "mbx_burst_groups.h");
        }
        if (!g.sched) {
            return refused("a group without a schedule");
        }
        const BurstShape& sh = g.sched->shape;
        if (!soft && sh.llr()) {
            return refused("an LLR schedule has soft bursts only");
        }
        if (g.n_streams > 0 && !g.bursts) {
            return refused("a group without bursts");
        }
        if (!soft && g.burst_stride < sh.bytes) {
            return refused("a burst_stride below mbx_burst_schedule_bytes()");
        }
        GroupShape& q = shapes[i];
        q.codec = sh.codec, q.form = sh.form, q.frames = sh.frames;
        q.n_streams = g.n_streams, q.bursts_per_stream = g.bursts_per_stream;
        q.bursts_per_wg = burst_gather_per_workgroup(g.sched, soft);
        q.lds = burst_gather_lds(g.sched, soft);
    }
    const GroupRefusal r = plan_groups(shapes, n_groups, plan);
    return r == kGroupsOk ? 0 : refused(group_refusal_text(r));
}

int burst_gather_groups(const GroupGather* groups, int count, bool soft, unsigned grid, unsigned lds, const GroupLayout& layout, void* d_rows,
                        void* stream) {
    GatherGroups d{};
    d.count = count;
    d.S = layout.S, d.total = layout.total;
    d.frame_offset = layout.d_frame_offset, d.stream_index = layout.d_stream_index, d.stream_codec = layout.d_stream_codec;
    for (int i = 0; i < count; ++i) {
        const GroupGather& g = groups[i];
        const mbx_burst_schedule* s = g.sched;
        const BurstShape& sh = s->shape;
        GatherGroup& e = d.g[i];
        e.in = g.d_in, e.stride = g.burst_stride;
        e.tab = soft ? s->d_cell_tab : s->d_wire_tab;
        e.xor_tab = s->d_xor_tab;
        e.index = g.d_index;
        e.n = g.bursts;
        e.F = sh.frames, e.B = sh.bits;
        e.unit = soft ? (int)sh.cells : (int)sh.frame_bytes;
        e.staged = s->staged_cells;
        e.per = soft ? s->soft_bursts : s->lstride;
        // (the instance burst_gather launches for this schedule)
        if (soft) {
            e.instance = sh.form == MBX_BURST_FORM_LLR16    ? kSoftLlr16
                         : sh.form == MBX_BURST_FORM_LLR8   ? kSoftLlr8
                         : sh.form == MBX_BURST_FORM_DIBITS ? kSoftDibit
                         : s->inverts                       ? kSoftBitFlip
                                                            : kSoftBit;
        } else {
            e.instance = sh.form == MBX_BURST_FORM_DIBITS ? kHardDibits
                         : sh.form == MBX_BURST_FORM_BITS ? kHardBits
                         : s->inverts                     ? kHardPackedInvert
                                                          : kHardPacked;
        }
        e.first_wg = g.first_wg, e.first_row = g.first_row, e.first_stream = g.first_stream;
        e.bursts_per_stream = g.bursts_per_stream, e.codec = sh.codec, e.first_slot = g.first_slot;
    }
    if (soft) {
        hipLaunchKernelGGL(burst_gather_soft_groups_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, d, static_cast<mbe_soft_bit*>(d_rows));
    } else {
        hipLaunchKernelGGL(burst_gather_groups_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, d, static_cast<uint8_t*>(d_rows));
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_failed("", soft ? "the soft gather of the burst groups" : "the gather of the burst groups", e);
}

}  // namespace mbx

namespace {

// what the stand-alone gathers check alike: the schedule, its device, the count
int gather_ready(const char* who, const mbx_burst_schedule* sched, size_t n) {
    char text[200];
    int dev = -1;
    const int rc = ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    if (dev != sched->shape.device) {
        snprintf(text, sizeof(text), "the schedule was made on device %d, the current device is %d", sched->shape.device, dev);
        return mbx::refuse(who, text);
    }
    if (n > (size_t)0x7fffffff / (size_t)MBX_BURST_MAX_FRAMES) {
        return mbx::refuse(who, "too many bursts in one launch");
    }
    return 0;
}

int channel_bits(const mbx::CodecShape* sh) {   // of one frame
    int nbits = 0;
    for (int r = 0; r < sh->rows; ++r) {
        nbits += sh->width[r];
    }
    return nbits;
}

// what of mbx_burst_schedule_create_form's arguments can be refused before their tables are read: the text, or nullptr
// (mbx_burst_schedule_create_llr: `form` is the LLR form of its llr_bytes, 0 for a width there is none of)
const char* schedule_args_refused(const mbx::CodecShape* sh, int frames_per_burst, int burst_bits, const int* src_bit, const int* cell_row,
                                  const int* cell_col, int form, const uint8_t* invert, bool llr) {
    if (!sh) {
        return "no such codec";
    }
    if (!src_bit || !cell_row || !cell_col) {
        return "src_bit, cell_row and cell_col are all needed";
    }
    if (frames_per_burst < 1 || frames_per_burst > MBX_BURST_MAX_FRAMES) {
        return "frames_per_burst must be 1 .. MBX_BURST_MAX_FRAMES";
    }
    if (burst_bits < 1 || burst_bits > MBX_BURST_MAX_BITS) {
        return "burst_bits must be 1 .. MBX_BURST_MAX_BITS";
    }
    if (llr) {
        if (form != MBX_BURST_FORM_LLR16 && form != MBX_BURST_FORM_LLR8) {
            return "llr_bytes must be 2 (int16) or 1 (int8)";
        }
    } else if (form != MBX_BURST_FORM_PACKED && form != MBX_BURST_FORM_BITS && form != MBX_BURST_FORM_DIBITS) {
        return "form must be one of MBX_BURST_FORM_*";
    }
    if (form == MBX_BURST_FORM_DIBITS && (burst_bits & 1)) {
        return "the dibit form needs an even burst_bits";
    }
    for (int j = 0; invert && j < burst_bits; ++j) {
        if (invert[j] > 1) {
            return "an invert byte is not 0 or 1";
        }
    }
    if ((long long)frames_per_burst * channel_bits(sh) > burst_bits) {
        return "the burst has fewer bits than its frames have channel bits";
    }
    return nullptr;
}

// the caller's schedule folded into what the kernels read, in one array as it is uploaded:
// wire table | cell table | one XOR byte per output byte (zero where no bit is inverted)
struct FoldedSchedule {
    std::vector<uint16_t> tabs;
    size_t wire_entries = 0;   // F * frame_bytes * 8: the cell table starts here ...
    size_t tab_entries = 0;    // ... and the XOR bytes here
    bool   inverts = false;
};

// Host only, no device is asked for.  Returns the text of a refusal that only reading the tables can find, or nullptr.
const char* fold_schedule(FoldedSchedule* f, int codec, const mbx::CodecShape* sh, int F, int burst_bits, const int* src_bit, const int* cell_row,
                          const int* cell_col, const uint8_t* invert) {
    const int nbits = channel_bits(sh), fbits = sh->frame_bytes * 8;
    const size_t items = (size_t)F * (size_t)sh->frame_bytes;
    f->wire_entries = (size_t)F * (size_t)fbits;
    f->tab_entries = f->wire_entries + (size_t)F * (size_t)sh->cells;
    f->tabs.assign(f->tab_entries + (items + 1) / 2, (uint16_t)mbx::kNoBit);
    uint16_t* wire = f->tabs.data();
    uint16_t* cell = f->tabs.data() + f->wire_entries;
    uint8_t* flips = reinterpret_cast<uint8_t*>(f->tabs.data() + f->tab_entries);
    memset(flips, 0, ((items + 1) / 2) * sizeof(uint16_t));
    std::vector<uint8_t> named((size_t)burst_bits, 0);
    for (int k = 0; k < F; ++k) {
        for (int i = 0; i < nbits; ++i) {
            const size_t at = (size_t)k * (size_t)nbits + (size_t)i;
            const int w = mbx_wire_bit_of_cell(codec, cell_row[at], cell_col[at]);   // (the one table of mbx_codec.h, behind it)
            if (w < 0) {
                return "a cell that is not on the codec's wire";
            }
            if (wire[(size_t)k * fbits + w] != mbx::kNoBit) {
                return "a cell of a frame is named twice";
            }
            const int j = src_bit[at];
            if (j < 0 || j >= burst_bits) {
                return "a src_bit outside [0, burst_bits)";
            }
            if (named[(size_t)j]) {
                return "a burst bit is named twice";
            }
            named[(size_t)j] = 1;
            wire[(size_t)k * fbits + w] = (uint16_t)j;
            const bool flip = invert && invert[j];
            cell[(size_t)k * sh->cells + (size_t)cell_row[at] * sh->stride + cell_col[at]] = (uint16_t)(flip ? (uint32_t)j | mbx::kInverted : (uint32_t)j);
            if (flip) {
                flips[((size_t)k * fbits + w) >> 3] |= (uint8_t)(0x80u >> (w & 7));
                f->inverts = true;
            }
        }
    }
    // (nbits distinct wire bits per frame, all on the wire: every wire cell of every frame has its bit)
    return nullptr;
}

// largest of `count` bytes, `step` apart, is above `most`
bool any_byte_above(const uint8_t* bytes, size_t count, size_t step, uint32_t most) {
    uint32_t seen = 0;
    for (size_t i = 0; i < count; ++i) {
        seen |= bytes[i * step];
    }
    return seen > most;
}

}  // namespace

extern "C" {

int mbx_burst_schedule_create(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                              const int* cell_row, const int* cell_col) {
    return mbx_burst_schedule_create_form(out, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col, MBX_BURST_FORM_PACKED, nullptr);
}

// the two creators: every refusal first, then the device
static int create_schedule(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit, const int* cell_row,
                           const int* cell_col, int form, const uint8_t* invert, bool llr) {
    if (!out) {
        return refuse("no place for the handle");
    }
    *out = nullptr;
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    const int F = frames_per_burst;
    FoldedSchedule folded;
    const char* why = schedule_args_refused(sh, F, burst_bits, src_bit, cell_row, cell_col, form, invert, llr);
    if (!why) {
        why = fold_schedule(&folded, codec, sh, F, burst_bits, src_bit, cell_row, cell_col, invert);
    }
    if (why) {
        return refuse(why);
    }
    // every refusal is behind us: now the device
    int dev = -1;
    const int rc = ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_burst_schedule* s = new (std::nothrow) mbx_burst_schedule();
    if (!s) {
        return refuse("out of memory");
    }
    const size_t items = (size_t)F * (size_t)sh->frame_bytes;
    const size_t packed_bytes = ((size_t)burst_bits + 7) / 8;
    // an LLR schedule has no hard bursts (bytes 0), and its int8 bursts need not be a whole number of cells (soft_cells 0)
    const size_t bytes = llr ? 0 : form == MBX_BURST_FORM_BITS ? (size_t)burst_bits : (form == MBX_BURST_FORM_DIBITS ? (size_t)burst_bits / 2 : packed_bytes);
    const size_t soft_cells = form == MBX_BURST_FORM_LLR8 ? 0 : form == MBX_BURST_FORM_DIBITS ? (size_t)burst_bits / 2 : (size_t)burst_bits;
    const size_t soft_bytes = form == MBX_BURST_FORM_LLR8 ? (size_t)burst_bits : soft_cells * sizeof(mbe_soft_bit);
    s->shape = mbx::BurstShape{codec, F, burst_bits, dev, bytes, (size_t)sh->frame_bytes, (size_t)sh->cells, form, soft_cells, soft_bytes};
    s->inverts = folded.inverts;
    // the hard gather works on the PACKED image of the bursts whatever their form: lstride and the dynamic LDS do not depend on it
    const int bdw = (int)((packed_bytes + 3) / 4);
    s->lstride = 4 * (bdw | 1);
    s->hard_lds = (unsigned)(items * 16 + (size_t)mbx::kGatherBursts * (size_t)s->lstride + ((mbx::kGatherBursts * items + 3) & ~(size_t)3));
    const int nb = mbx::kSoftStageBytes / (int)soft_bytes;
    const int most = form == MBX_BURST_FORM_DIBITS ? mbx::kSoftDibitBursts : form == MBX_BURST_FORM_LLR8 ? mbx::kSoftLlr8Bursts : 16;
    s->soft_bursts = nb < 1 ? 1 : (nb > most ? most : nb);
    s->staged_cells = form == MBX_BURST_FORM_DIBITS ? burst_bits / 2 : burst_bits;
    // (the staged range and one dword of slack for its alignment phase: up to one 16-bit cell, or three int8 LLRs)
    s->soft_lds = (unsigned)((size_t)F * (size_t)sh->cells * 2 + (size_t)s->soft_bursts * soft_bytes + 4 + 3) & ~3u;
    const std::vector<uint16_t>& tabs = folded.tabs;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_wire_tab), tabs.size() * sizeof(uint16_t));
    if (e == hipSuccess) {
        e = hipMemcpy(s->d_wire_tab, tabs.data(), tabs.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)hipFree(s->d_wire_tab);
        delete s;
        return mbx::hip_failed("", "mbx_burst_schedule_create: upload of the tables", e);
    }
    s->d_cell_tab = s->d_wire_tab + folded.wire_entries;
    s->d_xor_tab = reinterpret_cast<uint8_t*>(s->d_wire_tab + folded.tab_entries);
    *out = s;
    return 0;
}

int mbx_burst_schedule_create_form(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                                   const int* cell_row, const int* cell_col, int form, const uint8_t* invert) {
    return create_schedule(out, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col, form, invert, false);
}

int mbx_burst_schedule_create_llr(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                                  const int* cell_row, const int* cell_col, int llr_bytes, const uint8_t* invert) {
    const int form = llr_bytes == 2 ? MBX_BURST_FORM_LLR16 : llr_bytes == 1 ? MBX_BURST_FORM_LLR8 : 0;
    return create_schedule(out, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col, form, invert, true);
}

int mbx_burst_schedule_destroy(mbx_burst_schedule* sched) {
    if (sched) {
        (void)hipFree(sched->d_wire_tab);
        (void)hipGetLastError();
        delete sched;
    }
    return 0;
}

int mbx_burst_schedule_codec(const mbx_burst_schedule* sched) { return sched ? sched->shape.codec : MBE_STATUS_INVALID_ARGUMENT; }
int mbx_burst_schedule_frames(const mbx_burst_schedule* sched) { return sched ? sched->shape.frames : MBE_STATUS_INVALID_ARGUMENT; }
int mbx_burst_schedule_bits(const mbx_burst_schedule* sched) { return sched ? sched->shape.bits : MBE_STATUS_INVALID_ARGUMENT; }
int mbx_burst_schedule_form(const mbx_burst_schedule* sched) { return sched ? sched->shape.form : MBE_STATUS_INVALID_ARGUMENT; }
size_t mbx_burst_schedule_bytes(const mbx_burst_schedule* sched) { return sched ? sched->shape.bytes : 0; }
size_t mbx_burst_schedule_soft_cells(const mbx_burst_schedule* sched) { return sched ? sched->shape.soft_cells : 0; }
size_t mbx_burst_schedule_soft_bytes(const mbx_burst_schedule* sched) { return sched ? sched->shape.soft_bytes : 0; }

int mbx_burst_validate(const mbx_burst_schedule* sched, const void* bursts, size_t burst_stride, size_t n, int soft) {
    if (!sched || !bursts) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const mbx::BurstShape& sh = sched->shape;
    if (sh.llr()) {   // every LLR is a valid one; hard bursts of an LLR schedule there are none
        if (!soft) {
            mbx_set_error_text("mbx_burst_validate: an LLR schedule has soft bursts only");
        }
        return soft ? 0 : MBE_STATUS_INVALID_ARGUMENT;
    }
    if (soft) {
        if (sh.form != MBX_BURST_FORM_DIBITS) {
            return mbx_validate_soft_bits(static_cast<const mbe_soft_bit*>(bursts), n * sh.soft_cells);
        }
        const mbe_soft_bit* c = static_cast<const mbe_soft_bit*>(bursts);
        return any_byte_above(&c->bit, n * sh.soft_cells, sizeof(mbe_soft_bit), 3u) ? MBE_STATUS_INVALID_BITS : 0;
    }
    if (burst_stride < sh.bytes) {
        mbx_set_error_text("mbx_burst_validate: burst_stride is below mbx_burst_schedule_bytes()");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (sh.form == MBX_BURST_FORM_PACKED) {
        return 0;   // every byte is eight bits
    }
    const uint32_t most = sh.form == MBX_BURST_FORM_BITS ? 1u : 3u;
    const uint8_t* b = static_cast<const uint8_t*>(bursts);
    for (size_t i = 0; i < n; ++i, b += burst_stride) {
        if (any_byte_above(b, sh.bytes, 1, most)) {
            return MBE_STATUS_INVALID_BITS;
        }
    }
    return 0;
}

int mbx_burst_groups_rows(const mbx_burst_group* groups, int n_groups, int32_t* row_of_group) {
    mbx::GroupShape shapes[MBX_BURST_MAX_GROUPS];
    mbx::GroupPlan plan;
    if (!row_of_group) {
        mbx_set_error_text("mbx_burst_groups_rows: row_of_group is NULL");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    // (soft: neither the stride nor the hard-only rule is this call's to judge; a NULL bursts pointer is the launcher's)
    if (n_groups < 0 || n_groups > MBX_BURST_MAX_GROUPS || (n_groups > 0 && !groups)) {
        mbx_set_error_text("mbx_burst_groups_rows: n_groups must be 0 .. MBX_BURST_MAX_GROUPS, with groups");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    for (int i = 0; i < n_groups; ++i) {
        if (!groups[i].sched) {
            mbx_set_error_text("mbx_burst_groups_rows: a group without a schedule");
            return MBE_STATUS_INVALID_ARGUMENT;
        }
        shapes[i].frames = groups[i].sched->shape.frames;
        shapes[i].n_streams = groups[i].n_streams, shapes[i].bursts_per_stream = groups[i].bursts_per_stream;
    }
    const mbx::GroupRefusal r = mbx::plan_groups(shapes, n_groups, &plan);
    if (r != mbx::kGroupsOk) {
        return mbx::refuse("mbx_burst_groups_rows", mbx::group_refusal_text(r));
    }
    for (int i = 0; i < n_groups; ++i) {
        row_of_group[i] = plan.place[i].first_row;
    }
    row_of_group[n_groups] = plan.total_rows;
    return 0;
}

size_t mbx_burst_workspace_frames(const mbx_burst_schedule* sched, int S, int soft) {
    if (!sched || S < 0) {
        return 0;
    }
    const size_t n = (size_t)S * (size_t)sched->shape.frames;
    const size_t row = soft ? sched->shape.cells * sizeof(mbe_soft_bit) : sched->shape.frame_bytes;
    const size_t unit = mbx_workspace_bytes(1);   // one workspace frame
    return n + (n * row + unit - 1) / unit;
}

int mbx_deinterleave(const mbx_burst_schedule* sched, const uint8_t* d_bursts, size_t burst_stride, size_t n, uint8_t* d_frames,
                     size_t frame_stride, void* stream) {
    if (!sched || !d_bursts || !d_frames) {
        mbx_set_error_text("mbx_deinterleave: schedule, d_bursts and d_frames are all needed");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const mbx::BurstShape& sh = sched->shape;
    if (sh.llr()) {
        mbx_set_error_text("mbx_deinterleave: an LLR schedule has soft bursts only (mbx_deinterleave_soft)");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (burst_stride < sh.bytes || (frame_stride != sh.frame_bytes && frame_stride != (size_t)MBX_MIXED_ROW_BYTES)) {
        mbx_set_error_text("mbx_deinterleave: burst_stride below mbx_burst_schedule_bytes(), or frame_stride neither the codec's frame size nor the mixed row");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    // (d_bursts and d_frames: alignment 1, nothing to refuse)
    const int rc = gather_ready("mbx_deinterleave", sched, n);
    if (rc < 0 || n == 0) {
        return rc;
    }
    return mbx::burst_gather(sched, false, d_bursts, burst_stride, n, d_frames, frame_stride, stream);
}

int mbx_deinterleave_soft(const mbx_burst_schedule* sched, const mbe_soft_bit* d_soft, size_t n, mbe_soft_bit* d_cells, size_t row_cells,
                          void* stream) {
    // (first: it needs no device, and of the schedule only whether its soft bursts are int8 LLRs)
    if (!mbx::aligned_to(d_soft, sched ? sched->shape.soft_align() : 2) || !mbx::aligned_to(d_cells, 2)) {
        return mbx::misaligned("mbx_deinterleave_soft", "mbx_burst.h");
    }
    if (!sched || !d_soft || !d_cells) {
        mbx_set_error_text("mbx_deinterleave_soft: schedule, d_soft and d_cells are all needed");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const mbx::BurstShape& sh = sched->shape;
    if (row_cells != sh.cells && row_cells != (size_t)MBX_MIXED_ROW_CELLS) {
        mbx_set_error_text("mbx_deinterleave_soft: row_cells neither the codec's cells nor the mixed row");
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const int rc = gather_ready("mbx_deinterleave_soft", sched, n);
    if (rc < 0 || n == 0) {
        return rc;
    }
    return mbx::burst_gather(sched, true, d_soft, 0, n, d_cells, row_cells, stream);
}

}  // extern "C"
