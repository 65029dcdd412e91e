// mbx_pcm8.hip -- companded PCM out (include/mbx_pcm8.h): the int16 rows a step wrote -> G.711 bytes, mu-law or A-law, in one launch
// BEHIND the step.  The arithmetic is mbx_compand.h, shared with the host function below; the kernel adds nothing but the moving.
//
// A streaming kernel: 2 B in and 1 B out per sample, some twenty integer instructions between them.  A lane takes a PIECE of 8
// samples, 16 B in and 8 B out; a launch has one lane per piece, as floattoshort_kernel has one per pair.  The pieces start `head`
// samples into the arrays, where the output is 8-byte aligned, so the phase is the same for every piece of a launch; when that
// sample is 16-byte aligned in the input as well (every pair of allocations, every pair of rows of them: 320 and 160 bytes are
// multiples of 16 and 8) the piece is one 16-byte load, otherwise eight 2-byte loads.  The at most 7 samples in front of the first
// piece and the at most 7 behind the last go one by one through the first lanes of the grid.  No LDS, no table, no loop.
#include "mbx_compand.h"
#include "mbx_host.h"
#include "mbx_kernels.h"
#include "mbx_pcm8.h"

namespace mbx {

template <int kLaw>
__device__ __forceinline__ uint32_t compand_pair(uint32_t w) {   // two samples of one dword -> their bytes in bits 0..15
    return (uint32_t)pcm16_compand(kLaw, (int16_t)(w & 0xFFFFu)) | ((uint32_t)pcm16_compand(kLaw, (int16_t)(w >> 16)) << 8);
}

// in: n samples, 2-byte aligned; out: n bytes; pieces: whole pieces of 8 samples from sample `head` (out + head is 8-byte aligned;
// kAligned: in + head is 16-byte aligned); head + 8 * pieces + tail == n, head and tail below 8.
template <int kLaw, bool kAligned>
__global__ void __launch_bounds__(256)
pcm_compand_kernel(const int16_t* __restrict__ in, uint8_t* __restrict__ out, size_t n, size_t pieces, int head, int tail) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < pieces) {
        const size_t at = (size_t)head + 8 * g;
        uint4 v;
        if constexpr (kAligned) {
            v = *reinterpret_cast<const uint4*>(in + at);
        } else {
            const uint16_t* const p = reinterpret_cast<const uint16_t*>(in + at);
            v.x = (uint32_t)p[0] | ((uint32_t)p[1] << 16);
            v.y = (uint32_t)p[2] | ((uint32_t)p[3] << 16);
            v.z = (uint32_t)p[4] | ((uint32_t)p[5] << 16);
            v.w = (uint32_t)p[6] | ((uint32_t)p[7] << 16);
        }
        uint2 o;
        o.x = compand_pair<kLaw>(v.x) | (compand_pair<kLaw>(v.y) << 16);
        o.y = compand_pair<kLaw>(v.z) | (compand_pair<kLaw>(v.w) << 16);
        *reinterpret_cast<uint2*>(out + at) = o;
    }
    if (g < (size_t)(head + tail)) {   // the edges: lanes 0 .. head - 1 in front, the next `tail` lanes behind
        const size_t i = g < (size_t)head ? g : n - (size_t)tail + (g - (size_t)head);
        out[i] = pcm16_compand(kLaw, in[i]);
    }
}
template __global__ void pcm_compand_kernel<kLawUlaw, true>(const int16_t*, uint8_t*, size_t, size_t, int, int);
template __global__ void pcm_compand_kernel<kLawUlaw, false>(const int16_t*, uint8_t*, size_t, size_t, int, int);
template __global__ void pcm_compand_kernel<kLawAlaw, true>(const int16_t*, uint8_t*, size_t, size_t, int, int);
template __global__ void pcm_compand_kernel<kLawAlaw, false>(const int16_t*, uint8_t*, size_t, size_t, int, int);

}  // namespace mbx

extern "C" {

static_assert(MBX_LAW_ULAW == mbx::kLawUlaw && MBX_LAW_ALAW == mbx::kLawAlaw, "one numbering of the laws, in the public header and in mbx_compand.h");

int mbx_pcm_compand_host(int law, const int16_t* pcm16, size_t nsamples, uint8_t* pcm8) {
    if (!pcm16 || !pcm8 || (law != MBX_LAW_ULAW && law != MBX_LAW_ALAW)) {
        return mbx::refuse("mbx_pcm_compand_host", "pcm16 and pcm8 are needed, law is MBX_LAW_ULAW or MBX_LAW_ALAW");
    }
    for (size_t i = 0; i < nsamples; ++i) {
        pcm8[i] = mbx::pcm16_compand(law, pcm16[i]);
    }
    return 0;
}

int mbx_pcm_compand(int law, const int16_t* d_pcm16, size_t nframes, uint8_t* d_pcm8, void* stream) {
    if (!d_pcm16 || !d_pcm8 || (law != MBX_LAW_ULAW && law != MBX_LAW_ALAW)) {
        return mbx::refuse("mbx_pcm_compand", "d_pcm16 and d_pcm8 are needed, law is MBX_LAW_ULAW or MBX_LAW_ALAW");
    }
    if (!mbx::aligned_to(d_pcm16, 2)) {
        return mbx::misaligned("mbx_pcm_compand", "mbx_pcm8.h");
    }
    if (nframes == 0) {
        return 0;
    }
    if (nframes > ((size_t)1 << 40)) {   // (the grid below stays under 2^31 workgroups)
        return mbx::refuse("mbx_pcm_compand", "more than 2^40 frames in one launch");
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    // the phase of the launch: the first sample whose byte is 8-byte aligned; its piece is one 16-byte load where the sample is
    // 16-byte aligned too
    const size_t n = nframes * 160u;   // (>= 160: head and tail always fit)
    const int head = (int)((8u - (reinterpret_cast<uintptr_t>(d_pcm8) & 7u)) & 7u);
    const bool wide = mbx::aligned_to(d_pcm16 + head, 16);
    const size_t pieces = (n - (size_t)head) / 8;
    const int tail = (int)(n - (size_t)head - 8 * pieces);
    const unsigned grid = (unsigned)((pieces + 255) / 256);
    const auto kernel = law == MBX_LAW_ALAW ? (wide ? mbx::pcm_compand_kernel<mbx::kLawAlaw, true> : mbx::pcm_compand_kernel<mbx::kLawAlaw, false>)
                                            : (wide ? mbx::pcm_compand_kernel<mbx::kLawUlaw, true> : mbx::pcm_compand_kernel<mbx::kLawUlaw, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_pcm16, d_pcm8, n, pieces, head, tail);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "pcm_compand_kernel", e);
}

}  // extern "C"
