// mbx_burst.hip -- burst input (include/mbx_burst.h): the caller's de-interleave schedule, folded once on the host into two tables,
// and the two gather kernels that apply them to every burst on the device: received bursts -> packed wire frames (hard) or the
// reference's cell arrays (soft), i.e. what the batch launchers of mbx_api.hip start from.  The launchers that chain a gather in
// front of a batch step are in mbx_api.hip (they need the stream's workspace), the session submits in mbx_session.hip.
//
// No air-interface table is written here: F, B, the strides and the tables are kernel arguments, one code object serves every
// schedule.  The frame shapes come from the one table in mbx_codec.h (through mbx_wire_bit_of_cell for the wire order).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "mbx.h"
#include "mbx_burst.h"
#include "mbx_codec.h"
#include "mbx_gather.h"
#include "mbx_kernels.h"

void mbx_set_error_text(const char* text);   // mbx_api.hip: the per-thread text behind mbx_last_error()

namespace mbx {

constexpr int      kGatherBursts = 64;     // hard gather: bursts per workgroup, one per lane of every wave
constexpr int      kSoftStageBytes = 32768;   // soft gather: a workgroup stages at most this much of soft bursts (and at most 16 bursts)
constexpr uint32_t kNoBit = 0xffffu;       // table entry of a frame bit / cell no received bit goes to

// ---- hard bursts -> packed wire frames ---------------------------------------------------------------------------------------------
// A workgroup takes 64 consecutive bursts.  Their bytes go to LDS with coalesced loads (dwords when pointer and stride allow, bytes
// otherwise), burst j at j * lstride with lstride / 4 ODD: lane j of every wave then works on burst j, all lanes on the SAME
// received bit at a time, and the 32 lanes of a half hit 32 different banks.  Which bit that is comes from the schedule's table
// (wire bit -> burst bit, in LDS): one 16-bit read by eight lanes fetches the eight entries of an output byte, v_readlane makes
// each a scalar, so per bit a lane does one address add, one LDS byte read and a shift-and-merge.  The output bytes of the 64 bursts
// are collected in LDS as the image of the rows and leave as whole aligned dwords across the workgroup (single bytes only where a
// dword is not wholly inside a frame: the edges of the row range, the upper halves of 18-byte AMBE rows).
//   wire_tab   [F][fbytes * 8] burst bit of each wire bit, kNoBit for the bits that pad the last byte
//   lstride    bytes between two bursts in LDS
// dynamic LDS: table | 64 * lstride | 64 * F * fbytes
__global__ void __launch_bounds__(256)
burst_gather_kernel(const uint8_t* __restrict__ bursts, size_t burst_stride, size_t n, int F, int B, int fbytes,
                    const uint16_t* __restrict__ wire_tab, uint8_t* __restrict__ frames, int frame_stride, int lstride) {
    extern __shared__ uint32_t lds[];
    const int items = F * fbytes;   // output bytes of one burst; eight table entries each
    const int tab_dwords = items * 4;
    const uint16_t* tab = reinterpret_cast<const uint16_t*>(lds);
    uint8_t* in = reinterpret_cast<uint8_t*>(lds + tab_dwords);
    uint8_t* out = in + kGatherBursts * lstride;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t first = (size_t)blockIdx.x * kGatherBursts;
    const int here = (int)((n - first) < (size_t)kGatherBursts ? (n - first) : (size_t)kGatherBursts);
    for (int i = tid; i < tab_dwords; i += 256) {
        lds[i] = reinterpret_cast<const uint32_t*>(wire_tab)[i];
    }
    const int bbytes = (B + 7) >> 3;
    const uint8_t* src = bursts + first * burst_stride;
    if (((reinterpret_cast<uintptr_t>(bursts) | burst_stride) & 3u) == 0) {
        const int dw = (bbytes + 3) >> 2;   // (burst_stride is a multiple of 4 and >= bbytes: the last dword is inside the burst's stride)
        for (int j = wave; j < here; j += 4) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (size_t)j * burst_stride);
            uint32_t* d = reinterpret_cast<uint32_t*>(in + j * lstride);
            for (int i = lane; i < dw; i += 64) {
                d[i] = s[i];
            }
        }
    } else {
        for (int j = wave; j < here; j += 4) {
            for (int i = lane; i < bbytes; i += 64) {
                in[j * lstride + i] = src[(size_t)j * burst_stride + i];
            }
        }
    }
    __syncthreads();
    // lane = burst (lanes behind `here` work on stale LDS bytes; their rows are not written out)
    const uint8_t* mine = in + lane * lstride;
    for (int item = wave; item < items; item += 4) {
        const uint32_t e = tab[item * 8 + (lane & 7)];
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
        out[lane * items + item] = (uint8_t)byte;
    }
    __syncthreads();
    // rows first * F .. (first + here) * F - 1; out[row * fbytes + b] is byte b of the row
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

// ---- soft bursts -> cell arrays ----------------------------------------------------------------------------------------------------
// A workgroup takes nb consecutive bursts (a contiguous range of cells) into LDS with dword loads from the first aligned pair on,
// then every wave takes rows of the output: a lane owns the two cells of one aligned output dword, looks each up in the schedule's
// table (cell -> burst bit, in LDS), fetches it with one 16-bit LDS read and stores the pair; cells without a received bit, and
// the cells of a mixed row behind the codec's array, are {0, 0}.
//   cell_tab   [F][cells] burst bit of each cell of the reference's array, kNoBit for a cell that is not on the wire
// dynamic LDS: table | nb * B cells (+ one pair of slack for the alignment phase)
__global__ void __launch_bounds__(256)
burst_gather_soft_kernel(const mbe_soft_bit* __restrict__ soft, size_t n, int F, int B, int cells, const uint16_t* __restrict__ cell_tab,
                         mbe_soft_bit* __restrict__ rows_out, int row_cells, int nb) {
    extern __shared__ uint32_t lds[];
    const int tab_dwords = (F * cells) >> 1;   // (every codec has an even number of cells)
    const uint16_t* tab = reinterpret_cast<const uint16_t*>(lds);
    uint16_t* in16 = reinterpret_cast<uint16_t*>(lds + tab_dwords);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t first = (size_t)blockIdx.x * (size_t)nb;
    const int here = (int)((n - first) < (size_t)nb ? (n - first) : (size_t)nb);
    for (int i = tid; i < tab_dwords; i += 256) {
        lds[i] = reinterpret_cast<const uint32_t*>(cell_tab)[i];
    }
    // cell i of the range sits at in16[i + head]: an aligned dword of the source is an aligned dword of LDS
    const uint16_t* src = reinterpret_cast<const uint16_t*>(soft) + first * (size_t)B;
    const int ncells = here * B;
    const int head = (int)((reinterpret_cast<uintptr_t>(src) >> 1) & 1u);
    const int ndw = (ncells - head) >> 1;
    {
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
    const int nrows = here * F;
    uint16_t* dst = reinterpret_cast<uint16_t*>(rows_out) + first * (size_t)F * (size_t)row_cells;
    const int a = (int)((reinterpret_cast<uintptr_t>(dst) >> 1) & 1u);   // (row_cells is even: every row has the phase of the first)
    const int pairs = (row_cells + 1 + a) >> 1;
    for (int r = wave; r < nrows; r += 4) {
        const int j = r / F, k = r - j * F;
        const uint16_t* t = tab + k * cells;
        const uint16_t* b = in16 + head + j * B;
        uint16_t* o = dst + (size_t)r * (size_t)row_cells;
        for (int p = lane; p < pairs; p += 64) {
            const int c0 = 2 * p - a, c1 = c0 + 1;
            uint32_t v0 = 0, v1 = 0;
            if (c0 >= 0 && c0 < cells) {
                const uint32_t e = t[c0];
                if (e != kNoBit) {
                    v0 = b[e];
                }
            }
            if (c1 < cells) {
                const uint32_t e = t[c1];
                if (e != kNoBit) {
                    v1 = b[e];
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

}  // namespace mbx

// ---- the schedule (host) -----------------------------------------------------------------------------------------------------------
struct mbx_burst_schedule {
    mbx::BurstShape shape;
    int       lstride = 0;      // hard gather: bytes between two bursts in LDS (a whole, odd number of dwords)
    unsigned  hard_lds = 0;     // dynamic LDS of the two kernels
    int       soft_bursts = 0;  // soft gather: bursts per workgroup
    unsigned  soft_lds = 0;
    uint16_t* d_wire_tab = nullptr;   // [frames][frame_bytes * 8]
    uint16_t* d_cell_tab = nullptr;   // [frames][cells]; the same allocation, behind the wire table
};

namespace {

int refuse(const char* why) {
    char text[200];
    snprintf(text, sizeof(text), "mbx_burst_schedule_create: %s", why);
    mbx_set_error_text(text);
    return MBE_STATUS_INVALID_ARGUMENT;
}

int hip_fail(const char* what, hipError_t e) {
    char text[200];
    snprintf(text, sizeof(text), "%s: %s", what, hipGetErrorString(e));
    mbx_set_error_text(text);
    return MBX_ENODEVICE;
}

}  // namespace

namespace mbx {

BurstShape burst_shape(const mbx_burst_schedule* sched) { return sched->shape; }

int burst_gather(const mbx_burst_schedule* sched, bool soft, const void* d_in, size_t burst_stride, size_t n, void* d_out, size_t row,
                 void* stream) {
    const BurstShape& sh = sched->shape;
    if (soft) {
        const unsigned grid = (unsigned)((n + (size_t)sched->soft_bursts - 1) / (size_t)sched->soft_bursts);
        hipLaunchKernelGGL(burst_gather_soft_kernel, dim3(grid), dim3(256), sched->soft_lds, (hipStream_t)stream, static_cast<const mbe_soft_bit*>(d_in), n,
                           sh.frames, sh.bits, (int)sh.cells, sched->d_cell_tab, static_cast<mbe_soft_bit*>(d_out), (int)row, sched->soft_bursts);
    } else {
        const unsigned grid = (unsigned)((n + kGatherBursts - 1) / kGatherBursts);
        hipLaunchKernelGGL(burst_gather_kernel, dim3(grid), dim3(256), sched->hard_lds, (hipStream_t)stream, static_cast<const uint8_t*>(d_in), burst_stride,
                           n, sh.frames, sh.bits, (int)sh.frame_bytes, sched->d_wire_tab, static_cast<uint8_t*>(d_out), (int)row, sched->lstride);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(soft ? "burst_gather_soft_kernel" : "burst_gather_kernel", e);
}

}  // namespace mbx

namespace {

// what the stand-alone gathers check alike: the schedule, its device, the count
int gather_ready(const char* who, const mbx_burst_schedule* sched, size_t n) {
    char text[200];
    int dev = -1;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        return hip_fail("hipGetDevice", e);
    }
    if (!mbx_device_ready(dev)) {
        mbx_set_error_text("mbx_init() has not been called for the current device");
        return MBX_ENOTINIT;
    }
    if (dev != sched->shape.device) {
        snprintf(text, sizeof(text), "%s: the schedule was made on device %d, the current device is %d", who, sched->shape.device, dev);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (n > (size_t)0x7fffffff / (size_t)MBX_BURST_MAX_FRAMES) {
        snprintf(text, sizeof(text), "%s: too many bursts in one launch", who);
        mbx_set_error_text(text);
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return 0;
}

int misaligned(const char* who) {
    char text[200];
    snprintf(text, sizeof(text), "%s: a pointer is below the alignment of its kind (include/mbx_burst.h, Alignment)", who);
    mbx_set_error_text(text);
    return MBE_STATUS_INVALID_ARGUMENT;
}

}  // namespace

extern "C" {

int mbx_burst_schedule_create(mbx_burst_schedule** out, int codec, int frames_per_burst, int burst_bits, const int* src_bit,
                              const int* cell_row, const int* cell_col) {
    if (!out) {
        return refuse("no place for the handle");
    }
    *out = nullptr;
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!sh) {
        return refuse("no such codec");
    }
    if (!src_bit || !cell_row || !cell_col) {
        return refuse("src_bit, cell_row and cell_col are all needed");
    }
    if (frames_per_burst < 1 || frames_per_burst > MBX_BURST_MAX_FRAMES) {
        return refuse("frames_per_burst must be 1 .. MBX_BURST_MAX_FRAMES");
    }
    if (burst_bits < 1 || burst_bits > MBX_BURST_MAX_BITS) {
        return refuse("burst_bits must be 1 .. MBX_BURST_MAX_BITS");
    }
    int nbits = 0;   // channel bits of one frame
    for (int r = 0; r < sh->rows; ++r) {
        nbits += sh->width[r];
    }
    const int F = frames_per_burst, fbits = sh->frame_bytes * 8;
    if ((long long)F * nbits > burst_bits) {
        return refuse("the burst has fewer bits than its frames have channel bits");
    }
    std::vector<uint16_t> tabs((size_t)F * (size_t)fbits + (size_t)F * (size_t)sh->cells, (uint16_t)mbx::kNoBit);
    uint16_t* wire = tabs.data();
    uint16_t* cell = tabs.data() + (size_t)F * (size_t)fbits;
    std::vector<uint8_t> named((size_t)burst_bits, 0);
    for (int k = 0; k < F; ++k) {
        for (int i = 0; i < nbits; ++i) {
            const size_t at = (size_t)k * (size_t)nbits + (size_t)i;
            const int w = mbx_wire_bit_of_cell(codec, cell_row[at], cell_col[at]);   // (the one table of mbx_codec.h, behind it)
            if (w < 0) {
                return refuse("a cell that is not on the codec's wire");
            }
            if (wire[(size_t)k * fbits + w] != mbx::kNoBit) {
                return refuse("a cell of a frame is named twice");
            }
            const int j = src_bit[at];
            if (j < 0 || j >= burst_bits) {
                return refuse("a src_bit outside [0, burst_bits)");
            }
            if (named[(size_t)j]) {
                return refuse("a burst bit is named twice");
            }
            named[(size_t)j] = 1;
            wire[(size_t)k * fbits + w] = (uint16_t)j;
            cell[(size_t)k * sh->cells + (size_t)cell_row[at] * sh->stride + cell_col[at]] = (uint16_t)j;
        }
    }
    // (nbits distinct wire bits per frame, all on the wire: every wire cell of every frame has its bit)
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        return hip_fail("hipGetDevice", e);
    }
    if (!mbx_device_ready(dev)) {
        mbx_set_error_text("mbx_init() has not been called for the current device");
        return MBX_ENOTINIT;
    }
    mbx_burst_schedule* s = new (std::nothrow) mbx_burst_schedule();
    if (!s) {
        return refuse("out of memory");
    }
    s->shape = mbx::BurstShape{codec, F, burst_bits, dev, ((size_t)burst_bits + 7) / 8, (size_t)sh->frame_bytes, (size_t)sh->cells};
    const int bdw = (int)((s->shape.bytes + 3) / 4);
    s->lstride = 4 * (bdw | 1);
    const size_t items = (size_t)F * (size_t)sh->frame_bytes;
    s->hard_lds = (unsigned)(items * 16 + (size_t)mbx::kGatherBursts * (size_t)s->lstride + ((mbx::kGatherBursts * items + 3) & ~(size_t)3));
    int nb = mbx::kSoftStageBytes / (burst_bits * (int)sizeof(mbe_soft_bit));
    s->soft_bursts = nb < 1 ? 1 : (nb > 16 ? 16 : nb);
    s->soft_lds = (unsigned)((size_t)F * (size_t)sh->cells * 2 + ((size_t)s->soft_bursts * (size_t)burst_bits + 2) * 2 + 3) & ~3u;
    e = hipMalloc(reinterpret_cast<void**>(&s->d_wire_tab), tabs.size() * sizeof(uint16_t));
    if (e == hipSuccess) {
        e = hipMemcpy(s->d_wire_tab, tabs.data(), tabs.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)hipFree(s->d_wire_tab);
        delete s;
        return hip_fail("mbx_burst_schedule_create: upload of the tables", e);
    }
    s->d_cell_tab = s->d_wire_tab + (size_t)F * (size_t)fbits;
    *out = s;
    return 0;
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
size_t mbx_burst_schedule_bytes(const mbx_burst_schedule* sched) { return sched ? sched->shape.bytes : 0; }

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
    if (burst_stride < sh.bytes || (frame_stride != sh.frame_bytes && frame_stride != (size_t)MBX_MIXED_ROW_BYTES)) {
        mbx_set_error_text("mbx_deinterleave: burst_stride below ceil(burst_bits / 8), or frame_stride neither the codec's frame size nor the mixed row");
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
    if ((reinterpret_cast<uintptr_t>(d_soft) | reinterpret_cast<uintptr_t>(d_cells)) & 1u) {   // (first: it needs neither the schedule nor a device)
        return misaligned("mbx_deinterleave_soft");
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
