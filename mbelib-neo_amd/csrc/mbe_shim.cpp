// mbe_shim.cpp -- libmbe_neo_amd.so: the reference's per-frame `mbe_*` C API (include/mbe_neo_amd.h)
// on top of the HIP launcher (include/mbx.h).  Host logic only: argument/result validation and
// bookkeeping follow the reference call for call; every number that the reference computes is
// computed by a kernel.  No CPU compute fallback -- if the GPU cannot be initialised the process
// aborts with a message.
//
// Per call: one frame is staged through a small per-thread device scratch area (allocated once
// per thread), the kernels run on a per-thread stream, outputs are copied back.  The reference's
// thread-local synthesis RNG state (src/core/mbe_adaptive.c:29-30, src/core/mbe_unvoiced_fft.c:29-30)
// is a thread_local mbx_stream_rng here.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <algorithm>
#include <vector>

#include "mbe_device_list.h"
#include "mbe_flush_plan.h"
#include "mbe_neo_amd.h"
#include "mbe_neo_shards.h"
#include "mbx.h"
#include "mbx_cells.h"
#include "mbx_codec.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "libmbe_neo_amd: %s: %s\nlibmbe_neo_amd has no CPU fallback; aborting.\n", what, mbx_last_error());
    abort();
}

std::once_flag g_once;
// MBX_DEVICES (mbe_device_list.h): the shards the per-frame API runs on, each on its device.  Unset: ONE shard on MBX_DEVICE (or 0).
// A thread lives on its HOME shard's device -- its Slot, so every synchronous call --; queue mode spreads the channels of a
// thread's batch over all shards.  Run on one card only so far (a device named several times); DESIGN.md §6.
mbx::DeviceList g_shards;
std::atomic<int> g_threads{0};   // threads that have made their Slot: the next one's ordinal
// pinned arrays of queue mode: with several shards they are allocated with the shard's device current and must be visible to it
// whichever device that is -- portable and mapped, said explicitly (the zero-copy flush has the kernels read and write them)
unsigned g_pin_flags = hipHostMallocDefault;
// MBE_NEO_FRAME_SERVER=1: synchronous calls are served by a resident wavefront (mbx_frame_server_start) instead of a launch each.
// OPT-IN: measured 20.9 us per call against 22.5 us (the state still crosses PCIe both ways in every call, which is what
// bounds it), and a kernel that stays on the device occupies one of HIP's few hardware queues while it lives -- other streams
// of the process that map onto the same queue wait for it (sessions from one host thread: 153 -> 104 M frames/s when the
// server's extra stream shifted their streams onto a shared queue).  EXPERIMENTS.md (round 4).
bool g_frame_server = false;
// MBE_NEO_FRAME_SHADOW=0 switches the device copy of the synchronous calls' state off (every call then takes its state from the
// caller's structs across PCIe, as before round 4): for A/B timing and as a way out should a host ever trip over it.
bool g_frame_shadow = true;

void init_once() {
    std::string path;
    if (const char* env = getenv("MBX_TABLES")) {
        path = env;
    } else {
        Dl_info info;
        if (dladdr(reinterpret_cast<void*>(&init_once), &info) && info.dli_fname) {
            path = info.dli_fname;
            const size_t slash = path.find_last_of('/');
            path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/data/mbx_tables.bin";
        }
    }
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "libmbe_neo_amd: cannot open table blob '%s' (set MBX_TABLES)\n", path.c_str());
        abort();
    }
    std::vector<unsigned char> blob(sizeof(mbx_tables) + 1);
    const size_t n = fread(blob.data(), 1, blob.size(), f);
    fclose(f);
    const char* dev = getenv("MBX_DEVICE");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        count = 0;
        (void)hipGetLastError();
    }
    const char* why = nullptr;
    if (!mbx::parse_device_list(getenv("MBX_DEVICES"), count, dev ? atoi(dev) : 0, &g_shards, &why)) {   // MBX_DEVICES wins over MBX_DEVICE
        fprintf(stderr, "libmbe_neo_amd: %s (MBX_DEVICES: 'all', or device indices separated by commas; %d device%s here)\n", why, count,
                count == 1 ? "" : "s");
        abort();
    }
    if (g_shards.n > 1) {
        g_pin_flags = hipHostMallocPortable | hipHostMallocMapped;
    }
    if (const char* fs = getenv("MBE_NEO_FRAME_SERVER")) {
        g_frame_server = atoi(fs) != 0;
    }
    if (const char* sh = getenv("MBE_NEO_FRAME_SHADOW")) {
        g_frame_shadow = atoi(sh) != 0;
    }
    for (int i = 0; i < g_shards.n; ++i) {   // once per DISTINCT device
        if (std::find(g_shards.device, g_shards.device + i, g_shards.device[i]) == g_shards.device + i
            && mbx_init(g_shards.device[i], blob.data(), n) != 0) {
            die("mbx_init");
        }
    }
}

#define HIP_OK(expr)                                   \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) {                        \
            fprintf(stderr, "libmbe_neo_amd: %s: %s\n", #expr, hipGetErrorString(e_)); \
            abort();                                   \
        }                                              \
    } while (0)

// Per-thread scratch for one frame, in PINNED HOST memory that the kernels read and write in place over PCIe (zero-copy):
// a single 20 ms frame is a few KB, so what a synchronous call costs is launch + synchronise latency, and every
// hipMemcpyAsync in front of or behind the kernels would add its own.  up() / down() on this block are plain host
// memcpys (down() is deferred to sync()); on anything else they are DMA copies on the thread's stream (queue mode).
struct Slot {
    hipStream_t       stream = nullptr;
    uint8_t*          block = nullptr;    // one hipHostMalloc allocation holding everything below
    size_t            block_bytes = 0;
    uint8_t*          frame = nullptr;    // 18 bytes
    mbx_param_record* rec = nullptr;
    mbe_parms*        state = nullptr;    // 3
    mbx_stream_rng*   rng = nullptr;
    float*            pcmf = nullptr;     // 160
    int16_t*          pcm16 = nullptr;    // 160
    mbe_process_result* res = nullptr;
    uint32_t*         words = nullptr;    // 4: in, out, errs
    uint32_t*         done = nullptr;     // completion word of the single-frame kernel (mbx_process_frame), polled by the host
    uint32_t          token = 0;
    // Device copy of the state of the synchronous mbe_process*Frame[f] calls (mbx_process_frame_shadow): a call whose structs
    // still are, byte for byte, what the previous call handed back reads its state from HBM instead of across PCIe.
    // shadow_valid: the copy equals state[0..2] / rng of the pinned block (true after a call whose kernel said so; any other
    // use of the pinned block -- up() -- clears it).
    mbe_parms*        d_shadow = nullptr;       // 3 structs, device memory
    mbx_stream_rng*   d_shadow_rng = nullptr;
    uint32_t*         shadow_ok = nullptr;      // pinned: written by the kernel
    bool              shadow_valid = false;
    // frame server (include/mbx.h): synchronous calls that come back to back are served by ONE resident wavefront from this
    // mailbox instead of a launch each.  It leaves by itself after kServerIdleUs without a request; the next call starts it again.
    mbx_frame_mailbox* mailbox = nullptr;
    hipStream_t       server_stream = nullptr;
    uint32_t          seq = 0;
    hipEvent_t        chunk_done[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // mbe_flush: small outputs, then four PCM chunks
    uint8_t*          frame_out = nullptr; // 18 bytes: a frame after one of the in-place sub-stages
    mbe_soft_bit*     soft = nullptr;     // one soft frame (184 cells)
    struct Pending {
        void*       dst;
        const void* src;
        size_t      n;
    } pending[12];
    int npending = 0;
    int ordinal = 0, home = 0, device = 0;   // the thread's number, its home shard (mbe_device_list.h) and that shard's device
    Slot() {
        std::call_once(g_once, init_once);
        ordinal = g_threads.fetch_add(1, std::memory_order_relaxed);
        home = mbx::home_shard(ordinal, g_shards.n);
        device = g_shards.device[home];
        HIP_OK(hipSetDevice(device));   // HIP's current device is per thread: every thread that decodes selects its home device
        HIP_OK(hipStreamCreate(&stream));
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t at = off;
            off += (bytes + 63u) & ~(size_t)63u;
            return at;
        };
        const size_t o_frame = take(32), o_rec = take(sizeof(mbx_param_record)), o_state = take(3 * sizeof(mbe_parms)),
                     o_rng = take(sizeof(mbx_stream_rng)), o_pcmf = take(160 * sizeof(float)), o_pcm16 = take(160 * sizeof(int16_t)),
                     o_res = take(sizeof(mbe_process_result)), o_words = take(4 * sizeof(uint32_t)), o_done = take(64), o_sok = take(64), o_fout = take(32),
                     o_mail = take(sizeof(mbx_frame_mailbox)),
                     o_soft = take(MBX_IMBE_SOFT_BITS * sizeof(mbe_soft_bit));   // the largest soft frame (184 cells)
        block_bytes = off;
        // fine-grained (coherent) pinned memory: what a kernel writes here is visible to the host while the kernel is still
        // running, in program order behind a system-scope fence -- the completion word below relies on that
        HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&block), block_bytes, hipHostMallocCoherent));
        memset(block, 0, block_bytes);
        frame = block + o_frame;
        rec = reinterpret_cast<mbx_param_record*>(block + o_rec);
        state = reinterpret_cast<mbe_parms*>(block + o_state);
        rng = reinterpret_cast<mbx_stream_rng*>(block + o_rng);
        pcmf = reinterpret_cast<float*>(block + o_pcmf);
        pcm16 = reinterpret_cast<int16_t*>(block + o_pcm16);
        res = reinterpret_cast<mbe_process_result*>(block + o_res);
        words = reinterpret_cast<uint32_t*>(block + o_words);
        done = reinterpret_cast<uint32_t*>(block + o_done);
        shadow_ok = reinterpret_cast<uint32_t*>(block + o_sok);
        void* sh = nullptr;
        // (mbx_stream_rng starts with a 64-bit word and needs 8-byte alignment -- include/mbx.h, Alignment --; three structs of 2,604 B end at 4 mod 8)
        const size_t rng_at = (3 * sizeof(mbe_parms) + 7u) & ~(size_t)7u;
        HIP_OK(hipMalloc(&sh, rng_at + sizeof(mbx_stream_rng)));
        d_shadow = static_cast<mbe_parms*>(sh);
        d_shadow_rng = reinterpret_cast<mbx_stream_rng*>(static_cast<char*>(sh) + rng_at);
        mailbox = reinterpret_cast<mbx_frame_mailbox*>(block + o_mail);
        frame_out = block + o_fout;
        soft = reinterpret_cast<mbe_soft_bit*>(block + o_soft);
    }
    bool mine(const void* p) const {
        const uint8_t* q = static_cast<const uint8_t*>(p);
        return q >= block && q < block + block_bytes;
    }
    void up(void* dst, const void* src, size_t n) {
        shadow_valid = false;   // the pinned block is about to hold something the device copy does not
        if (mine(dst)) {
            memcpy(dst, src, n);   // visible to every kernel launched after this point
        } else {
            HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream));
        }
    }
    void down(void* dst, const void* src, size_t n) {
        if (mine(src)) {
            if (npending == (int)(sizeof(pending) / sizeof(pending[0]))) {
                fprintf(stderr, "libmbe_neo_amd: too many deferred copies\n");
                abort();
            }
            pending[npending++] = Pending{dst, src, n};   // the kernels have not run yet: copied by sync()
        } else {
            HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream));
        }
    }
    // Wait for the single-frame kernel by polling its completion word (a few microseconds less than waking up on the
    // stream's completion signal).  The stream is queried now and then so that a faulted launch cannot spin forever.
    void wait_token(uint32_t want) {
        for (unsigned spins = 1;; ++spins) {
            if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == want) {
                return;
            }
            if ((spins & 0x3fffu) == 0u) {
                const hipError_t e = hipStreamQuery(stream);
                if (e == hipSuccess) {   // the kernel has retired: the word is there (or the launch never ran)
                    if (__atomic_load_n(done, __ATOMIC_ACQUIRE) != want) {
                        fprintf(stderr, "libmbe_neo_amd: single-frame kernel retired without its completion word\n");
                        abort();
                    }
                    return;
                }
                if (e != hipErrorNotReady) {
                    HIP_OK(e);
                }
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
    }
    // One frame through the frame server: fill the request, publish it, wait for its completion word.  The server is started
    // when there is none (first call of the thread, or it has left after its idle time-out); a request that races with a
    // server on its way out is simply not served by it (it touches nothing after alive = 0) and goes to the successor.
    static constexpr unsigned kServerIdleUs = 1000;
    void start_server() {
        if (!server_stream) {
            HIP_OK(hipStreamCreateWithFlags(&server_stream, hipStreamNonBlocking));
        }
        __atomic_store_n(&mailbox->alive, 1u, __ATOMIC_RELEASE);
        if (mbx_frame_server_start(mailbox, kServerIdleUs, state, rng, pcm16, pcmf, res, rec, d_shadow, d_shadow_rng, shadow_ok, server_stream) != 0) {
            fprintf(stderr, "libmbe_neo_amd: mbx_frame_server_start: %s\n", mbx_last_error());
            abort();
        }
    }
    void serve(int codec, int16_t* out16, float* outf, bool from_shadow) {
        mbx_frame_mailbox* mb = mailbox;
        mb->codec = codec;
        mb->want = (out16 ? MBX_FRAME_WANT_PCM16 : 0u) | (outf ? MBX_FRAME_WANT_PCMF : 0u) | (from_shadow ? MBX_FRAME_WANT_SHADOW : 0u);
        memcpy(mb->frame, frame, sizeof(mb->frame));   // (the packer wrote 18 | 9 bytes of a 32-byte field)
        const uint32_t want = ++seq;
        __atomic_store_n(&mb->seq_in, want, __ATOMIC_RELEASE);
        for (unsigned spins = 1;; ++spins) {
            if (__atomic_load_n(&mb->seq_out, __ATOMIC_ACQUIRE) == want) {
                return;
            }
            if (__atomic_load_n(&mb->alive, __ATOMIC_ACQUIRE) == 0u) {
                if (__atomic_load_n(&mb->seq_out, __ATOMIC_ACQUIRE) == want) {   // it served this one and then left
                    return;
                }
                start_server();
            }
            if ((spins & 0xfffffu) == 0u && server_stream) {
                const hipError_t e = hipStreamQuery(server_stream);   // a faulted server must not leave the host spinning for ever
                if (e != hipSuccess && e != hipErrorNotReady) {
                    HIP_OK(e);
                }
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
    }
    void stop_server() {   // thread exit, and before anything that synchronises the whole device
        if (server_stream) {
            __atomic_store_n(&mailbox->quit, 1u, __ATOMIC_RELEASE);
            (void)hipStreamSynchronize(server_stream);
            __atomic_store_n(&mailbox->quit, 0u, __ATOMIC_RELEASE);
            __atomic_store_n(&mailbox->alive, 0u, __ATOMIC_RELEASE);
        }
    }
    void sync() {
        HIP_OK(hipStreamSynchronize(stream));
        for (int i = 0; i < npending; ++i) {
            memcpy(pending[i].dst, pending[i].src, pending[i].n);
        }
        npending = 0;
    }
};

// What a decoding thread owns (stream, pinned block, the stream's expand workspace inside libmbx_hip) goes back when the
// thread ends: a host that spawns short-lived decode threads must not leak one of each per thread.
struct SlotHolder {
    Slot* p = nullptr;
    ~SlotHolder() {
        if (p) {
            // the stream's workspace slot lives in the context of the thread's home device: a host that has switched devices on this thread must
            // not have the release resolved against another device's context (the slot would leak, keyed by a dead hipStream_t)
            int before = -1;
            (void)hipGetDevice(&before);
            (void)hipSetDevice(p->device);
            p->stop_server();
            if (p->server_stream) {
                (void)hipStreamDestroy(p->server_stream);
            }
            (void)hipStreamSynchronize(p->stream);
            (void)mbx_release_stream(p->stream);
            for (hipEvent_t e : p->chunk_done) {
                if (e) {
                    (void)hipEventDestroy(e);
                }
            }
            (void)hipStreamDestroy(p->stream);
            (void)hipFree(p->d_shadow);
            (void)hipHostFree(p->block);
            if (before >= 0 && before != p->device) {
                (void)hipSetDevice(before);
            }
            (void)hipGetLastError();
            delete p;
        }
    }
};

Slot& slot() {
    thread_local SlotHolder holder;
    if (!holder.p) {
        holder.p = new Slot();
    }
    Slot* s = holder.p;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device) {   // the host application switched devices on this thread
        HIP_OK(hipSetDevice(s->device));
    }
    return *s;
}

struct ThreadRng {
    mbx_stream_rng r;
    ThreadRng() { mbx_rng_default(&r); }
};
thread_local ThreadRng t_rng;

void must(int rc, const char* what) {
    if (rc < 0) {
        die(what);
    }
}

// ---- result bookkeeping: ref src/internal/mbe_result.h:18-121 ---------------------------------
constexpr unsigned kContext = MBE_PROCESS_FLAG_SOFT_INPUT | MBE_PROCESS_FLAG_C0_VALID | MBE_PROCESS_FLAG_C4_VALID;
constexpr unsigned kStatus = MBE_PROCESS_FLAG_TONE | MBE_PROCESS_FLAG_ERASURE | MBE_PROCESS_FLAG_REPEAT | MBE_PROCESS_FLAG_MUTE;

using mbx::validate_bits;   // (mbx_cells.h; ref src/internal/mbe_result.h:18-29)

bool count_ok(int c) { return c >= 0 && c <= 184; }

int resolve_total_errors(const mbe_process_result* r, int* total_out) {
    if (!r) {
        *total_out = 0;
        return 0;
    }
    if ((r->flags & ~(kContext | kStatus)) != 0u) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!count_ok(r->c0_errors) || !count_ok(r->protected_errors) || !count_ok(r->c4_errors) || !count_ok(r->total_errors)
        || r->c0_errors > 184 - r->protected_errors) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const int parts = r->c0_errors + r->protected_errors;
    if (!count_ok(parts)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const int total = (r->total_errors == 0 && parts != 0) ? parts : r->total_errors;
    const bool c0v = (r->flags & MBE_PROCESS_FLAG_C0_VALID) != 0u, c4v = (r->flags & MBE_PROCESS_FLAG_C4_VALID) != 0u;
    if (!((parts == 0 || total == parts) && (!c0v || total >= r->c0_errors) && (!c4v || total >= r->c4_errors))) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    *total_out = total;
    return 0;
}

bool valid_L(int L) { return L >= 1 && L <= 56; }

// parameter bits + error context -> the record the stream kernels consume
mbx_param_record make_record(const char* bits, int nbits, const mbe_process_result* r, int total) {
    mbx_param_record rec;
    memset(&rec, 0, sizeof(rec));
    for (int i = 0; i < nbits; ++i) {
        if (bits[i]) {
            rec.w[i >> 5] |= 0x80000000u >> (i & 31);
        }
    }
    const unsigned ctx = r->flags & kContext;
    const int c0 = (ctx & MBE_PROCESS_FLAG_C0_VALID) ? r->c0_errors : 0;
    const int c4 = (ctx & MBE_PROCESS_FLAG_C4_VALID) ? r->c4_errors : 0;
    rec.w[3] = (uint32_t)c0 | ((uint32_t)(total - c0) << 8) | ((uint32_t)c4 << 16) | (ctx << 24);
    return rec;
}

// The shim links against the launcher's public ABI only: the packer and the FEC launch of a codec's front end (mbx_codec.h:
// CodecShape::front) are picked here, once.  `codec`: one of the four.
int pack_one(int codec, const char* cells, uint8_t* packed) {
    switch (mbx::kCodecs[codec].front) {
        case MBX_CODEC_IMBE7200X4400: return mbx_pack_imbe7200x4400(cells, 1, packed);
        case MBX_CODEC_IMBE7100X4400: return mbx_pack_imbe7100x4400(cells, 1, packed);
        default: return mbx_pack_ambe3600x2450(cells, 1, packed);
    }
}
int fec_one(int codec, const uint8_t* d_frame, mbx_param_record* d_rec, void* stream) {
    switch (mbx::kCodecs[codec].front) {
        case MBX_CODEC_IMBE7200X4400: return mbx_fec_imbe7200x4400(d_frame, 1, d_rec, stream);
        case MBX_CODEC_IMBE7100X4400: return mbx_fec_imbe7100x4400(d_frame, 1, d_rec, stream);
        default: return mbx_fec_ambe3600x2450(d_frame, 1, d_rec, stream);
    }
}

// mbe_decode*Frame
int decode_frame(int codec, const char* cells, char* bits_out, mbe_process_result* result) {
    const mbx::CodecShape& sh = mbx::kCodecs[codec];
    if (result) {
        memset(result, 0, sizeof(*result));
    }
    if (!bits_out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(cells, (size_t)sh.cells);
    if (rc < 0) {
        return rc;
    }
    uint8_t packed[MBX_IMBE_FRAME_BYTES];
    rc = pack_one(codec, cells, packed);
    if (rc < 0) {
        return rc;
    }
    Slot& s = slot();
    s.up(s.frame, packed, (size_t)sh.frame_bytes);
    must(fec_one(codec, s.frame, s.rec, s.stream), "mbx_fec");
    mbx_param_record rec;
    s.down(&rec, s.rec, sizeof(rec));
    s.sync();
    mbe_process_result r;
    mbx_unpack_records(&rec, 1, sh.data_bits, bits_out, &r);
    if (result) {
        *result = r;
    }
    return r.total_errors;
}

void sync_channel_for_direct_use(const mbe_parms* cur);   // queue mode, further down

// mbe_process*Dataf: ref src/imbe/imbe7200x4400.c:858-909, src/ambe/ambe3600x2450.c:851-898
int process_data(int codec, float* aout_f, short* aout_s, mbe_process_result* result, const char* bits, mbe_parms* cur, mbe_parms* prev,
                 mbe_parms* enh) {
    const int nbits = mbx::kCodecs[codec].data_bits;
    mbe_process_result local;
    if (!result) {
        memset(&local, 0, sizeof(local));
        result = &local;
    }
    if ((!aout_f && !aout_s) || !cur || !prev || !enh) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    sync_channel_for_direct_use(cur);   // queue mode: a channel whose state lives on the device comes home first
    int total = 0;
    int rc = resolve_total_errors(result, &total);
    if (rc < 0) {
        return rc;
    }
    rc = validate_bits(bits, (size_t)nbits);
    if (rc < 0) {
        return rc;
    }
    const mbx_param_record rec = make_record(bits, nbits, result, total);
    Slot& s = slot();
    s.up(s.rec, &rec, sizeof(rec));
    s.up(&s.state[0], cur, sizeof(mbe_parms));
    s.up(&s.state[1], prev, sizeof(mbe_parms));
    s.up(&s.state[2], enh, sizeof(mbe_parms));
    s.up(s.rng, &t_rng.r, sizeof(mbx_stream_rng));
    must(mbx_process_records(codec, 1, 1, s.rec, s.state, s.rng, aout_s ? s.pcm16 : nullptr, aout_f ? s.pcmf : nullptr, s.res,
                             s.stream),
         "mbx_process_records");
    if (aout_f) {
        s.down(aout_f, s.pcmf, 160 * sizeof(float));
    }
    if (aout_s) {
        s.down(aout_s, s.pcm16, 160 * sizeof(int16_t));
    }
    s.down(cur, &s.state[0], sizeof(mbe_parms));
    s.down(prev, &s.state[1], sizeof(mbe_parms));
    s.down(enh, &s.state[2], sizeof(mbe_parms));
    s.down(&t_rng.r, s.rng, sizeof(mbx_stream_rng));
    s.down(result, s.res, sizeof(mbe_process_result));
    s.sync();
    return result->total_errors;
}

void synth_speech(float* aout_f, short* aout_s, mbe_parms* cur, mbe_parms* prev) {
    Slot& s = slot();
    s.up(&s.state[0], cur, sizeof(mbe_parms));
    s.up(&s.state[1], prev, sizeof(mbe_parms));
    s.up(s.rng, &t_rng.r, sizeof(mbx_stream_rng));
    must(mbx_synthesize_speech(1, &s.state[0], &s.state[1], s.rng, aout_f ? s.pcmf : nullptr, aout_s ? s.pcm16 : nullptr,
                               s.stream),
         "mbx_synthesize_speech");
    if (aout_f) {
        s.down(aout_f, s.pcmf, 160 * sizeof(float));
    }
    if (aout_s) {
        s.down(aout_s, s.pcm16, 160 * sizeof(int16_t));
    }
    s.down(cur, &s.state[0], sizeof(mbe_parms));
    s.down(prev, &s.state[1], sizeof(mbe_parms));
    s.down(&t_rng.r, s.rng, sizeof(mbx_stream_rng));
    s.sync();
}

int ecc_word(int kind, uint32_t in, uint32_t* out) {
    Slot& s = slot();
    s.up(&s.words[0], &in, 4);
    must(mbx_ecc_words(kind, &s.words[0], 1, &s.words[1], reinterpret_cast<int32_t*>(&s.words[2]), s.stream), "mbx_ecc_words");
    uint32_t back[2];
    s.down(back, &s.words[1], 8);
    s.sync();
    *out = back[0];
    return (int)back[1];
}

// soft-decision code word (kind 0: 23 soft bits, kind 1: 15): one-wave launch
int ecc_soft_word(int kind, const mbe_soft_bit* in, uint32_t* out) {
    Slot& s = slot();
    const size_t width = kind == 0 ? 23 : 15;   // kind 2: Hamming with the 7100x4400 mapping
    s.up(s.soft, in, width * sizeof(mbe_soft_bit));
    must(mbx_ecc_soft_words(kind, s.soft, 1, &s.words[1], reinterpret_cast<int32_t*>(&s.words[2]), s.stream), "mbx_ecc_soft_words");
    uint32_t back[2];
    s.down(back, &s.words[1], 8);
    s.sync();
    *out = back[0];
    return (int)back[1];
}

// mbe_decode*SoftFrame: ref src/imbe/imbe7200x4400.c:746-778, src/ambe/ambe3600x2450.c:684-714
int decode_soft_frame(int codec, const mbe_soft_bit* cells, char* bits_out, mbe_process_result* result) {
    const int ncell = mbx::kCodecs[codec].cells, nbits = mbx::kCodecs[codec].data_bits;
    if (result) {
        memset(result, 0, sizeof(*result));
    }
    if (!bits_out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = mbx_validate_soft_bits(cells, (size_t)ncell);
    if (rc < 0) {
        return rc;
    }
    Slot& s = slot();
    s.up(s.soft, cells, (size_t)ncell * sizeof(mbe_soft_bit));
    must(mbx_fec_soft(codec, s.soft, 1, s.rec, s.stream), "mbx_fec_soft");
    mbx_param_record rec;
    s.down(&rec, s.rec, sizeof(rec));
    s.sync();
    mbe_process_result r;
    mbx_unpack_records(&rec, 1, nbits, bits_out, &r);
    if (result) {
        *result = r;
    }
    return r.total_errors;
}


// ==================================================================================================================
// Queue mode (include/mbe_neo_amd.h): the hard-decision mbe_process*Frame[f] calls of a thread -- and, with
// MBE_BATCH_QUEUE_SOFT, its mbe_process*SoftFrame[f] calls -- are recorded and run by mbe_flush() as batched launches,
// over a pool of channel states that lives on the device: all pending hard frames as ONE launch set and all pending soft frames as
// one -- a (codec, frames-per-channel) group alone in its input form by the single-codec launcher it has always had (one frame per
// channel: the one-launch forms), several groups together by mbx_process_batch_mixed / _soft_mixed, whatever their codecs and
// counts are.  Host
// work per queued frame: validation + packing (what the synchronous call does on the host as well) and a queue entry;
// a soft frame's cells (up to 368 B) go into the thread's cell arena, the entry keeps their offset.
// ==================================================================================================================
struct QEntry {
    void*               aout;
    mbe_process_result* result;
    char*               bits_out;
    int                 channel;      // index into Batch::channels
    uint8_t             codec;
    uint8_t             want_short;
    uint8_t             frame[MBX_IMBE_FRAME_BYTES];   // hard-decision entry: the packed wire frame
    size_t              soft_at;                       // soft entry: first cell in Batch::soft_cells
};

struct QChannel {
    mbe_parms *cur, *prev, *enh;
    int  codec = -1;       // codec of the frames pending for this channel (one codec per channel and flush)
    bool soft = false;     // ... and their input form (one per channel and flush as well)
    int  pending = 0;
    int  slot = -1;        // where its state lives in the device pool (resident mode: = channel index; write-back: per flush)
    bool on_device = false;
    mbx_stream_rng rng;    // the thread's RNG state at the channel's first queued frame; in write-back mode the channel's
                           // own state between flushes (the reference keeps it per thread, here it is per channel)
};

template <class U>
struct DevArr {   // grow-only device array
    U*     p = nullptr;
    size_t cap = 0;
    DevArr() = default;
    DevArr(const DevArr&) = delete;
    DevArr& operator=(const DevArr&) = delete;
    ~DevArr() {
        if (p) {
            (void)hipFree(p);
        }
    }
    void need(size_t n) {
        if (n > cap) {
            if (p) {
                HIP_OK(hipFree(p));
            }
            cap = n + n / 2 + 64;
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), cap * sizeof(U)));
        }
    }
};

template <class U>
struct PinArr {   // grow-only pinned host array
    U*     p = nullptr;
    size_t cap = 0;
    PinArr() = default;
    PinArr(const PinArr&) = delete;
    PinArr& operator=(const PinArr&) = delete;
    ~PinArr() {
        if (p) {
            (void)hipHostFree(p);
        }
    }
    void need(size_t n) {
        if (n > cap) {
            if (p) {
                HIP_OK(hipHostFree(p));
            }
            cap = n + n / 2 + 64;
            HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&p), cap * sizeof(U), g_pin_flags));
        }
    }
};

// How one flush runs, decided once its inputs are staged: where the kernels read and write -- the shard's PINNED arrays themselves
// (zero-copy) or their device twins -- and how the PCM comes back.
struct FlushRun {
    bool   zero_copy;
    int    chunks;        // PCM chunks of the copy-out: 4 from 8,192 rows on
    size_t per_chunk;     // rows of a chunk (the last may be shorter)
    const uint8_t* frames;
    const int32_t* index;
    const int32_t* offsets;
    const uint8_t* codecs;
    int16_t*            pcm16;     // nullptr: no queued call wants it
    float*              pcmf;
    mbe_process_result* results;
    mbx_param_record*   records;
};
constexpr int kMaxChunks = 4;

// The stream a (thread, shard) pair flushes on, with the five events of the copy-out and the copy helpers of the flush steps.
// With ONE shard the lane IS the thread's Slot -- its stream, its events, its up / down / sync --, as before there were shards;
// otherwise a stream of its own on the shard's device, made with the shard and given back with the thread.
struct Lane {
    Slot*       slot = nullptr;     // one shard: everything below is the Slot's
    int         device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t  own_events[1 + kMaxChunks] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t* chunk_done = own_events;   // mbe_flush: small outputs, then four PCM chunks
    Lane() = default;
    Lane(const Lane&) = delete;
    Lane& operator=(const Lane&) = delete;
    void open(int dev, Slot* home_slot) {   // home_slot: the thread's Slot when the list has one entry, else nullptr (`dev` is current)
        device = dev;
        slot = home_slot;
        if (slot) {
            stream = slot->stream;
            chunk_done = slot->chunk_done;
        } else {
            HIP_OK(hipStreamCreate(&stream));
        }
    }
    void up(void* dst, const void* src, size_t n) {
        if (slot) {
            slot->up(dst, src, n);
        } else {
            HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream));
        }
    }
    void down(void* dst, const void* src, size_t n) {
        if (slot) {
            slot->down(dst, src, n);
        } else {
            HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream));
        }
    }
    void sync() {
        if (slot) {
            slot->sync();
        } else {
            HIP_OK(hipStreamSynchronize(stream));
        }
    }
    void forget_pending() {   // (deferred copies exist on a Slot alone)
        if (slot) {
            slot->npending = 0;
        }
    }
    ~Lane() {
        if (slot || !stream) {
            return;   // the Slot's own: SlotHolder gives it back
        }
        // as SlotHolder does for the Slot: the stream's workspace slot lives in the context of the lane's device
        int before = -1;
        (void)hipGetDevice(&before);
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        (void)mbx_release_stream(stream);
        for (hipEvent_t e : own_events) {
            if (e) {
                (void)hipEventDestroy(e);
            }
        }
        (void)hipStreamDestroy(stream);
        if (before >= 0 && before != device) {
            (void)hipSetDevice(before);
        }
        (void)hipGetLastError();
    }
};

// One entry of MBX_DEVICES as a thread's batch sees it: a whole queue of its own -- entries, channels, pools, staging arrays, plan --
// on the entry's device, flushed on the thread's lane for it.  Made at the first channel placed on it; kept, like the arrays'
// capacity, until the thread ends.
struct Shard {
    int  mode = MBE_BATCH_STATE_WRITEBACK;                // Batch::mode, handed down by mbe_batchBegin
    Lane lane;                                            // (declared before the arrays: they are freed first, then the stream goes)
    long passes = 0, rows = 0;                            // since mbe_batchBegin: flush passes that launched something here, rows launched
    FlushRun run = {};                                    // the flush under way, between its two passes
    std::vector<QEntry>   q;
    std::vector<mbe_soft_bit> soft_cells;                 // cells of the queued soft frames, in call order; gathered into
                                                          // h_frames (pinned, group order) by the flush like packed frames
    std::vector<QChannel> channels;                       // pool slot = index
    DevArr<mbe_parms>      d_state;                       // [channels][3]
    DevArr<mbx_stream_rng> d_rng;
    DevArr<uint32_t>       d_elided;                      // resident mode: prev_mp_enhanced of the slot is elided (mbx_process_batch_resident)
    size_t                 resident = 0;                  // channels [0, resident) hold their state on the device
    DevArr<uint8_t>            d_frames;
    DevArr<mbx_param_record>   d_records;
    DevArr<int16_t>            d_pcm16;
    DevArr<float>              d_pcmf;
    DevArr<mbe_process_result> d_results;
    DevArr<int32_t>            d_index;
    PinArr<uint8_t>            h_frames;
    PinArr<mbx_param_record>   h_records;
    PinArr<int16_t>            h_pcm16;
    PinArr<float>              h_pcmf;
    PinArr<mbe_process_result> h_results;
    PinArr<int32_t>            h_index;
    DevArr<int32_t>            d_offsets;                 // a mixed launch set: first batch row of every channel (+ 1 entry) ...
    PinArr<int32_t>            h_offsets;
    DevArr<uint8_t>            d_codecs;                  // ... and its codec
    PinArr<uint8_t>            h_codecs;
    PinArr<mbe_parms>          h_state;
    PinArr<mbx_stream_rng>     h_rng;
    mbx::FlushPlan             plan;                      // the flush under way: groups, rows, bytes (mbe_flush_plan.h); reused from flush to flush
    std::vector<int>           upload;                    // ... and the channels whose state went up for it, in slot order
};

struct ChannelAt {
    int shard, channel;   // channel: index into Shard::channels
};

// What is global to a thread's batch; everything a flush works on is in the shards.
struct Batch {
    bool active = false;
    bool queue_soft = false;                              // MBE_BATCH_QUEUE_SOFT: mbe_process*SoftFrame[f] queue as well
    int  mode = MBE_BATCH_STATE_WRITEBACK;
    int  home = 0;                                        // the thread's home shard ...
    int  created = 0;                                     // ... and the channels it has created since mbe_batchBegin: the next one
                                                          // goes to channel_shard(home, created, shards) (mbe_device_list.h)
    std::unordered_map<const mbe_parms*, ChannelAt> index;   // cur_mp -> channel
    std::unordered_map<const mbe_parms*, ChannelAt> aux;     // prev_mp / prev_mp_enhanced -> channel (direct use of either struct)
    std::unique_ptr<Shard> shards[mbx::kMaxShards];       // [list entry]; null until its first channel

    size_t pending() const {
        size_t n = 0;
        for (int i = 0; i < g_shards.n; ++i) {
            n += shards[i] ? shards[i]->q.size() : 0;
        }
        return n;
    }
};

// HIP's current device while a shard is worked on.  One shard: the thread's home device is current already (slot()), nothing is called.
void use_device(int device) {
    if (g_shards.n > 1) {
        HIP_OK(hipSetDevice(device));
    }
}

// the shard of list entry `at`, made now if this is its first channel (the home device is current before and after)
Shard& shard_at(Batch& b, int at) {
    if (!b.shards[at]) {
        Slot& home = slot();
        b.shards[at].reset(new Shard());
        Shard& sh = *b.shards[at];
        sh.mode = b.mode;
        use_device(g_shards.device[at]);
        sh.lane.open(g_shards.device[at], g_shards.n == 1 ? &home : nullptr);
        use_device(home.device);
    }
    return *b.shards[at];
}

struct BatchHolder {   // freed with the thread (the arrays' destructors return the device and pinned memory)
    Batch* p = nullptr;
    ~BatchHolder() { delete p; }
};

Batch& batch() {
    thread_local BatchHolder holder;
    if (!holder.p) {
        holder.p = new Batch();
    }
    return *holder.p;
}

// grow the device pool to `n` channels, keeping what is resident
void pool_reserve(Shard& b, Lane& s, size_t n) {
    if (n <= b.d_state.cap / 3 && n <= b.d_rng.cap) {
        return;
    }
    const size_t cap = n + n / 2 + 64;
    mbe_parms* ns = nullptr;
    mbx_stream_rng* nr = nullptr;
    uint32_t* ne = nullptr;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&ns), cap * 3 * sizeof(mbe_parms)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&nr), cap * sizeof(mbx_stream_rng)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&ne), cap * sizeof(uint32_t)));
    HIP_OK(hipMemsetAsync(ne, 0, cap * sizeof(uint32_t), s.stream));
    if (b.resident) {
        HIP_OK(hipMemcpyAsync(ns, b.d_state.p, b.resident * 3 * sizeof(mbe_parms), hipMemcpyDeviceToDevice, s.stream));
        HIP_OK(hipMemcpyAsync(nr, b.d_rng.p, b.resident * sizeof(mbx_stream_rng), hipMemcpyDeviceToDevice, s.stream));
        HIP_OK(hipMemcpyAsync(ne, b.d_elided.p, b.resident * sizeof(uint32_t), hipMemcpyDeviceToDevice, s.stream));
    }
    s.sync();
    if (b.d_state.p) {
        HIP_OK(hipFree(b.d_state.p));
        HIP_OK(hipFree(b.d_rng.p));
        HIP_OK(hipFree(b.d_elided.p));
    }
    b.d_state.p = ns;
    b.d_state.cap = cap * 3;
    b.d_rng.p = nr;
    b.d_rng.cap = cap;
    b.d_elided.p = ne;
    b.d_elided.cap = cap;
}

// bring the state held in pool slots [first, first + count) back into the host structs of the channels that own them
// (`owners[i]` = channel of slot first + i); with_rng: the per-channel RNG state as well
void pool_download(Shard& b, Lane& s, size_t first, const std::vector<int>& owners, bool with_rng) {
    const size_t count = owners.size();
    if (count == 0) {
        return;
    }
    b.h_state.need(count * 3);
    // resident mode launches through mbx_process_batch_resident: the elided prev_mp_enhanced structs are written out first, so
    // that what goes home is the ABI triplet (bit-identical to what the synchronous calls would have left)
    if (b.mode == MBE_BATCH_STATE_RESIDENT) {
        must(mbx_resident_materialize((int)count, nullptr, b.d_state.p + 3 * first, b.d_elided.p + first, s.stream), "mbx_resident_materialize");
    }
    s.down(b.h_state.p, b.d_state.p + 3 * first, count * 3 * sizeof(mbe_parms));
    if (with_rng) {
        b.h_rng.need(count);
        s.down(b.h_rng.p, b.d_rng.p + first, count * sizeof(mbx_stream_rng));
    }
    s.sync();
    for (size_t i = 0; i < count; ++i) {
        QChannel& ch = b.channels[(size_t)owners[i]];
        *ch.cur = b.h_state.p[3 * i + 0];
        *ch.prev = b.h_state.p[3 * i + 1];
        *ch.enh = b.h_state.p[3 * i + 2];
        if (with_rng) {
            ch.rng = b.h_rng.p[i];
        }
    }
}

// parameter record -> the reference's imbe_d[88] / ambe_d[49] chars, eight cells per table look-up (the bit order of
// mbx_unpack_records: bit i of the record is bit 31 - (i & 31) of word i >> 5)
void unpack_bits_fast(const mbx_param_record& r, int nbits, char* out) {
    static const struct Lut {
        uint64_t v[256];
        Lut() {
            for (int b = 0; b < 256; ++b) {
                uint64_t x = 0;
                for (int k = 0; k < 8; ++k) {
                    x |= (uint64_t)((b >> (7 - k)) & 1) << (8 * k);   // little-endian: cell k of the byte is byte k of x
                }
                v[b] = x;
            }
        }
    } lut;
    int i = 0;
    for (; i + 8 <= nbits; i += 8) {
        const int j = i >> 3;
        const uint64_t x = lut.v[(r.w[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu];
        memcpy(out + i, &x, 8);
    }
    for (; i < nbits; ++i) {
        out[i] = (char)((r.w[i >> 5] >> (31 - (i & 31))) & 1u);
    }
}

// MBE_NEO_TRACE_FLUSH=1 (development): where a thread's flushes spend their wall time, summed per thread and printed to stderr when the
// thread leaves queue mode -- host preparation (grouping, frame gather), the trips into the HIP runtime,
// the wait for the device, and the scatter into the callers' buffers.
struct FlushTrace {
    double prep = 0, issue = 0, wait = 0, scatter = 0;
    long   flushes = 0, rows = 0, seen = 0;
};
static double trace_now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static const bool g_trace_flush = [] {
    const char* e = getenv("MBE_NEO_TRACE_FLUSH");
    return e && e[0] == '1';
}();
thread_local FlushTrace t_flush_trace;

template <class U>
U* flush_view(bool zero_copy, const PinArr<U>& h, const DevArr<U>& d) {
    return zero_copy ? h.p : d.p;
}

// ---- state upload.  Resident mode: the channels first seen since the last flush, appended at slots [resident, total).
//      Write-back mode: every channel that has frames this time, at slots [0, k); nothing stays afterwards. ----
void flush_upload_state(Shard& b, Lane& s) {
    const size_t total = b.channels.size();
    std::vector<int>& upload = b.upload;
    upload.clear();
    size_t first_slot = 0;
    if (b.mode == MBE_BATCH_STATE_RESIDENT) {
        first_slot = b.resident;
        for (size_t c = b.resident; c < total; ++c) {
            b.channels[c].slot = (int)c;
            upload.push_back((int)c);
        }
    } else {
        for (size_t c = 0; c < total; ++c) {
            if (b.channels[c].pending) {
                b.channels[c].slot = (int)upload.size();
                upload.push_back((int)c);
            }
        }
    }
    pool_reserve(b, s, first_slot + upload.size());
    if (upload.empty()) {
        return;
    }
    b.h_state.need(upload.size() * 3);
    b.h_rng.need(upload.size());
    for (size_t i = 0; i < upload.size(); ++i) {
        QChannel& ch = b.channels[(size_t)upload[i]];
        b.h_state.p[3 * i + 0] = *ch.cur;
        b.h_state.p[3 * i + 1] = *ch.prev;
        b.h_state.p[3 * i + 2] = *ch.enh;
        b.h_rng.p[i] = ch.rng;
        ch.on_device = true;
    }
    s.up(b.d_state.p + 3 * first_slot, b.h_state.p, upload.size() * 3 * sizeof(mbe_parms));
    s.up(b.d_rng.p + first_slot, b.h_rng.p, upload.size() * sizeof(mbx_stream_rng));
    HIP_OK(hipMemsetAsync(b.d_elided.p + first_slot, 0, upload.size() * sizeof(uint32_t), s.stream));   // whole triplets came up
    b.resident = first_slot + upload.size();
}

// SMALL flushes (many host threads, each with a share of the channels) move nothing with copy calls: the kernels read the frames
// and the index from, and write PCM / results / records to, the thread's PINNED host buffers directly (device-visible addresses),
// and the flush is then two or three trips into the HIP runtime -- launch, event, wait -- instead of a dozen.  What bounds the
// rate from many threads is the number of such trips, not the bytes (tools/fanin_evidence.py: no CPU throttling at sixteen
// threads, profiles/r05/fanin.json).  Large flushes keep the chunked copies: PCIe runs at its best with a DMA engine, and the
// host scatters one chunk while the next one crosses.  MBE_NEO_ZERO_COPY_FLUSH=0 switches it off (A/B timing).
// Every thread launches its own flush (a "pump" thread that launched for all of them was slower: EXPERIMENTS.md 6.4).
bool flush_zero_copy(size_t rows) {
    static const bool zero_copy_on = [] {
        const char* e = getenv("MBE_NEO_ZERO_COPY_FLUSH");
        return !(e && e[0] == '0');
    }();
    return zero_copy_on && rows < 8192;
}

// ---- inputs: the queued frames gathered into h_frames where the plan puts them, the plan's channels as pool slots, the offsets and
//      codecs of the mixed forms; every array sized; the views chosen; the inputs uploaded unless the kernels read them in place ----
FlushRun flush_stage_inputs(Shard& b, Lane& s) {
    const mbx::FlushPlan& p = b.plan;
    const size_t total = b.channels.size(), rows = p.rows;
    b.h_frames.need(p.bytes);
    b.h_index.need(total);
    bool any_short = false, any_float = false;
    for (size_t e = 0; e < b.q.size(); ++e) {
        const QEntry& qe = b.q[e];
        const QChannel& ch = b.channels[(size_t)qe.channel];
        memcpy(b.h_frames.p + p.byte_of(e, qe.channel), ch.soft ? static_cast<const void*>(&b.soft_cells[qe.soft_at]) : static_cast<const void*>(qe.frame),
               mbx::flush_input_bytes(ch.codec, ch.soft));
        any_short |= qe.want_short != 0;
        any_float |= qe.want_short == 0;
    }
    for (size_t i = 0; i < p.channels.size(); ++i) {
        b.h_index.p[i] = b.channels[(size_t)p.channels[i]].slot;
    }
    if (p.any_mixed()) {
        b.h_offsets.need(total + 2);
        b.h_codecs.need(total);
        b.d_offsets.need(total + 2);
        b.d_codecs.need(total);
        memcpy(b.h_offsets.p, p.offsets.data(), p.offsets.size() * sizeof(int32_t));
        memcpy(b.h_codecs.p, p.codecs.data(), p.codecs.size());
    }
    b.d_frames.need(p.bytes);
    b.d_index.need(total);
    b.d_records.need(rows);
    b.d_results.need(rows);
    b.h_records.need(rows);
    b.h_results.need(rows);
    if (any_short) {
        b.d_pcm16.need(rows * 160);
        b.h_pcm16.need(rows * 160);
    }
    if (any_float) {
        b.d_pcmf.need(rows * 160);
        b.h_pcmf.need(rows * 160);
    }
    const bool zc = flush_zero_copy(rows);
    const int chunks = rows >= 8192 ? kMaxChunks : 1;
    const FlushRun r = {zc, chunks, (rows + chunks - 1) / chunks,
                        flush_view(zc, b.h_frames, b.d_frames), flush_view(zc, b.h_index, b.d_index), flush_view(zc, b.h_offsets, b.d_offsets),
                        flush_view(zc, b.h_codecs, b.d_codecs), any_short ? flush_view(zc, b.h_pcm16, b.d_pcm16) : nullptr,
                        any_float ? flush_view(zc, b.h_pcmf, b.d_pcmf) : nullptr, flush_view(zc, b.h_results, b.d_results),
                        flush_view(zc, b.h_records, b.d_records)};
    if (!zc) {
        s.up(b.d_frames.p, b.h_frames.p, p.bytes);
        s.up(b.d_index.p, b.h_index.p, p.channels.size() * sizeof(int32_t));
        if (p.any_mixed()) {
            s.up(b.d_offsets.p, b.h_offsets.p, p.offsets.size() * sizeof(int32_t));
            s.up(b.d_codecs.p, b.h_codecs.p, p.codecs.size());
        }
    }
    return r;
}

// ---- launches: a mixed form as ONE launch set at its first group; a group alone in its form by the single-codec launcher of its
//      input form and state mode ----
void flush_launch(Shard& b, Lane& s, const FlushRun& r) {
    const mbx::FlushPlan& p = b.plan;
    const bool resident = b.mode == MBE_BATCH_STATE_RESIDENT;
    uint32_t* const elided = resident ? b.d_elided.p : nullptr;   // (no elision words in write-back mode)
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const mbx::FlushGroup& g = p.groups[gi];
        const int f = g.soft ? 1 : 0;
        if (p.form_mixed[f] && gi != p.form_g0[f]) {
            continue;   // (went out with the first group of its form)
        }
        const int32_t* const index = r.index + g.index0;
        const uint8_t* const frames = r.frames + g.byte0;
        const mbe_soft_bit* const cells = reinterpret_cast<const mbe_soft_bit*>(frames);
        // every launcher ends in the same arguments: the RNG pool, the group's rows of the four output arrays, the stream
        auto launch = [&](const char* name, auto fn, auto... head) {
            must(fn(head..., b.d_rng.p, r.pcm16 ? r.pcm16 + g.row0 * 160 : nullptr, r.pcmf ? r.pcmf + g.row0 * 160 : nullptr, r.results + g.row0,
                    r.records + g.row0, s.stream),
                 name);
        };
        if (p.form_mixed[f]) {
            const int nch = (int)p.form_channels(f);
            const uint8_t* const codecs = r.codecs + p.codec_at[f];
            const int32_t* const offsets = r.offsets + p.off_at[f];
            if (g.soft) {
                launch("mbx_process_batch_soft_mixed", mbx_process_batch_soft_mixed, nch, codecs, offsets, p.form_rows(f), index, cells, b.d_state.p, elided);
            } else {
                launch("mbx_process_batch_mixed", mbx_process_batch_mixed, nch, codecs, offsets, p.form_rows(f), index, frames, b.d_state.p, elided);
            }
        } else if (g.soft) {   // soft cells in: the soft twin of both launchers
            launch("mbx_process_batch_soft_resident", mbx_process_batch_soft_resident, g.codec, (int)g.nch, g.T, index, cells, b.d_state.p, elided);
        } else if (resident) {   // the pool owns the state between flushes: no prev_mp_enhanced traffic, lazy prev_mp
            launch("mbx_process_batch_resident", mbx_process_batch_resident, g.codec, (int)g.nch, g.T, index, frames, b.d_state.p, elided);
        } else {
            launch("mbx_process_batch_indexed", mbx_process_batch_indexed, g.codec, (int)g.nch, g.T, index, frames, b.d_state.p);
        }
    }
}

// ---- outputs: the small arrays first, then the PCM in chunks -- the host hands chunk k to the callers' buffers while
//      chunk k + 1 is still crossing PCIe (the scatter is as long as the copy: 5 MB per 16,384 frames each) ----
void flush_copy_out(Shard& b, Lane& s, const FlushRun& r) {
    const size_t rows = b.plan.rows;
    if (!s.chunk_done[0]) {
        HIP_OK(hipEventCreateWithFlags(&s.chunk_done[0], hipEventDisableTiming | hipEventBlockingSync));   // the long wait sleeps
        for (int k = 1; k <= kMaxChunks; ++k) {
            HIP_OK(hipEventCreateWithFlags(&s.chunk_done[k], hipEventDisableTiming));
        }
    }
    if (r.zero_copy) {   // everything is already where the host reads it once the kernels have retired: ONE event for all of it
        HIP_OK(hipEventRecord(s.chunk_done[0], s.stream));
        return;
    }
    HIP_OK(hipMemcpyAsync(b.h_results.p, b.d_results.p, rows * sizeof(mbe_process_result), hipMemcpyDeviceToHost, s.stream));
    HIP_OK(hipMemcpyAsync(b.h_records.p, b.d_records.p, rows * sizeof(mbx_param_record), hipMemcpyDeviceToHost, s.stream));
    HIP_OK(hipEventRecord(s.chunk_done[0], s.stream));
    for (int k = 0; k < r.chunks; ++k) {
        const size_t r0 = (size_t)k * r.per_chunk, r1 = r0 + r.per_chunk < rows ? r0 + r.per_chunk : rows;
        if (r0 < r1) {
            if (r.pcm16) {
                HIP_OK(hipMemcpyAsync(b.h_pcm16.p + r0 * 160, b.d_pcm16.p + r0 * 160, (r1 - r0) * 160 * sizeof(int16_t), hipMemcpyDeviceToHost, s.stream));
            }
            if (r.pcmf) {
                HIP_OK(hipMemcpyAsync(b.h_pcmf.p + r0 * 160, b.d_pcmf.p + r0 * 160, (r1 - r0) * 160 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
            }
        }
        HIP_OK(hipEventRecord(s.chunk_done[k + 1], s.stream));
    }
}

// ---- scatter into the callers' buffers: results and parameter bits, then the PCM chunk by chunk as it arrives ----
void flush_scatter(Shard& b, Lane& s, const FlushRun& r) {
    const mbx::FlushPlan& p = b.plan;
    for (size_t e = 0; e < b.q.size(); ++e) {
        const QEntry& qe = b.q[e];
        const size_t row = p.row_of[e];
        if (qe.result) {
            *qe.result = b.h_results.p[row];
        }
        unpack_bits_fast(b.h_records.p[row], mbx::kCodecs[qe.codec].data_bits, qe.bits_out);
    }
    for (int k = 0; k < r.chunks; ++k) {
        const size_t r0 = (size_t)k * r.per_chunk, r1 = r0 + r.per_chunk < p.rows ? r0 + r.per_chunk : p.rows;
        if (!r.zero_copy) {
            HIP_OK(hipEventSynchronize(s.chunk_done[k + 1]));
        }
        for (size_t row = r0; row < r1; ++row) {
            const QEntry& qe = b.q[p.by_row[row]];
            if (qe.want_short) {
                memcpy(qe.aout, b.h_pcm16.p + row * 160, 160 * sizeof(int16_t));
            } else {
                memcpy(qe.aout, b.h_pcmf.p + row * 160, 160 * sizeof(float));
            }
        }
    }
}

// ---- the queue is empty again; write-back mode: the host structs are current again, nothing stays on the device ----
void flush_finish(Shard& b, Lane& s) {
    s.forget_pending();
    b.q.clear();
    b.soft_cells.clear();
    for (QChannel& ch : b.channels) {
        ch.pending = 0;
        ch.codec = -1;
    }
    if (b.mode == MBE_BATCH_STATE_WRITEBACK) {
        pool_download(b, s, 0, b.upload, true);
        for (int c : b.upload) {
            b.channels[(size_t)c].on_device = false;
            b.channels[(size_t)c].slot = -1;
        }
        b.resident = 0;
    }
}

// One flush: where everything goes is planned on the host alone (mbe_flush_plan.h); the steps above carry the plan out.
// A shard's flush is a whole flush as it was before there were shards; with several, every shard with queued entries gets its work
// issued first (pass 1) and is waited for and scattered afterwards (pass 2), so that the devices work at the same time.
int flush_batch(Batch& all) {
    const size_t n = all.pending();
    if (n == 0) {
        return 0;
    }
    Slot& home = slot();
    const bool trace = g_trace_flush;
    double prep = 0, issue = 0, wait = 0, scatter = 0;   // summed over the shards
    long rows = 0;
    for (int i = 0; i < g_shards.n; ++i) {
        if (!all.shards[i] || all.shards[i]->q.empty()) {
            continue;
        }
        Shard& b = *all.shards[i];
        Lane& s = b.lane;
        use_device(s.device);
        const double tr0 = trace ? trace_now() : 0.0;
        flush_upload_state(b, s);
        b.plan.build(b.channels.data(), b.channels.size(), b.q.data(), b.q.size());
        b.run = flush_stage_inputs(b, s);
        const double tr1 = trace ? trace_now() : 0.0;
        flush_launch(b, s, b.run);
        flush_copy_out(b, s, b.run);
        b.plan.invert_rows();   // (host work behind the launches: the device is busy)
        b.passes += 1;
        b.rows += (long)b.plan.rows;
        if (trace) {
            const double tr2 = trace_now();
            prep += tr1 - tr0;
            issue += tr2 - tr1;
            rows += (long)b.plan.rows;
        }
    }
    for (int i = 0; i < g_shards.n; ++i) {   // (a shard of pass 1 still has its entries: flush_finish clears them)
        if (!all.shards[i] || all.shards[i]->q.empty()) {
            continue;
        }
        Shard& b = *all.shards[i];
        Lane& s = b.lane;
        use_device(s.device);
        const double tr2 = trace ? trace_now() : 0.0;
        if (b.plan.rows < 256) {
            HIP_OK(hipStreamSynchronize(s.stream));   // a small flush: spin, the sleeping wait's wake-up would be most of it
        } else {
            HIP_OK(hipEventSynchronize(s.chunk_done[0]));
        }
        const double tr3 = trace ? trace_now() : 0.0;
        flush_scatter(b, s, b.run);
        if (trace) {
            wait += tr3 - tr2;
            scatter += trace_now() - tr3;
        }
        flush_finish(b, s);
    }
    use_device(home.device);
    if (trace) {
        FlushTrace& t = t_flush_trace;
        if (++t.seen > 2) {   // (the first flushes of a thread allocate and upload: not the steady state)
            t.prep += prep;
            t.issue += issue;
            t.wait += wait;
            t.scatter += scatter;
            t.flushes += 1;
            t.rows += rows;
        }
    }
    return (int)n;
}

// forget one channel after bringing its state home (resident mode: the last channel of its shard takes its pool slot)
void release_channel(Batch& all, ChannelAt at) {
    Shard& b = *all.shards[at.shard];
    Lane& s = b.lane;
    const int c = at.channel;
    Slot& home = slot();
    use_device(s.device);
    QChannel& ch = b.channels[(size_t)c];
    const size_t last = b.channels.size() - 1;
    if (ch.on_device) {   // resident mode: slot == channel index
        pool_download(b, s, (size_t)c, std::vector<int>{c}, false);
        if ((size_t)c != last) {
            HIP_OK(hipMemcpyAsync(b.d_state.p + 3 * (size_t)c, b.d_state.p + 3 * last, 3 * sizeof(mbe_parms), hipMemcpyDeviceToDevice,
                                  s.stream));
            HIP_OK(hipMemcpyAsync(b.d_rng.p + c, b.d_rng.p + last, sizeof(mbx_stream_rng), hipMemcpyDeviceToDevice, s.stream));
            HIP_OK(hipMemcpyAsync(b.d_elided.p + c, b.d_elided.p + last, sizeof(uint32_t), hipMemcpyDeviceToDevice, s.stream));
            s.sync();
        }
        b.resident = last;
    }
    use_device(home.device);
    all.index.erase(ch.cur);
    all.aux.erase(ch.prev);
    all.aux.erase(ch.enh);
    if ((size_t)c != last) {
        b.channels[(size_t)c] = b.channels[last];
        if (b.channels[(size_t)c].on_device) {
            b.channels[(size_t)c].slot = c;
        }
        all.index[b.channels[(size_t)c].cur] = at;   // the maps of the whole batch follow the move
        all.aux[b.channels[(size_t)c].prev] = at;
        all.aux[b.channels[(size_t)c].enh] = at;
    }
    b.channels.pop_back();
}

// a synchronous call is about to use this struct (any of a channel's three): make sure the host copy is the current one.
// Outside queue mode, and for structs that belong to no queued channel, this is two look-ups in empty / small maps.
void sync_channel_for_direct_use(const mbe_parms* any) {
    Batch& b = batch();
    if (!any || !b.active || b.index.empty()) {
        return;
    }
    auto it = b.index.find(any);
    const ChannelAt* at = nullptr;
    if (it != b.index.end()) {
        at = &it->second;
    } else {
        auto ia = b.aux.find(any);
        if (ia != b.aux.end()) {
            at = &ia->second;
        }
    }
    if (at) {
        const mbe_parms* cur = b.shards[at->shard]->channels[(size_t)at->channel].cur;
        (void)flush_batch(b);   // the WHOLE batch, every shard
        release_channel(b, b.index.find(cur)->second);
    }
}

// the queued form of mbe_process*Frame[f] (cells) and mbe_process*SoftFrame[f] (soft: the frame's cells, `cells` unused)
int queue_frame(int codec, float* aout_f, short* aout_s, mbe_process_result* result, const char* cells, char* bits_out,
                mbe_parms* cur, mbe_parms* prev, mbe_parms* enh, const mbe_soft_bit* soft = nullptr) {
    const size_t ncell = (size_t)mbx::kCodecs[codec].cells;
    if (!bits_out || (!aout_f && !aout_s) || !cur || !prev || !enh) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = soft ? mbx_validate_soft_bits(soft, ncell) : validate_bits(cells, ncell);
    if (rc < 0) {
        return rc;
    }
    Batch& all = batch();
    auto it = all.index.find(cur);
    ChannelAt at;
    if (it == all.index.end()) {   // a new channel: placed now, and there it stays until it is released or the batch ends
        at.shard = mbx::channel_shard(all.home, all.created++, g_shards.n);
        Shard& b = shard_at(all, at.shard);
        at.channel = (int)b.channels.size();
        QChannel ch;
        ch.cur = cur;
        ch.prev = prev;
        ch.enh = enh;
        ch.rng = t_rng.r;
        b.channels.push_back(ch);
        all.index.emplace(cur, at);
        all.aux[prev] = at;
        all.aux[enh] = at;
    } else {
        at = it->second;
        QChannel& ch = all.shards[at.shard]->channels[(size_t)at.channel];
        if (ch.prev != prev || ch.enh != enh) {
            return MBE_STATUS_INVALID_ARGUMENT;   // a channel is its three structs; they cannot change while it is queued / resident
        }
        if (ch.pending && (ch.codec != codec || ch.soft != (soft != nullptr))) {   // one codec and one input form per channel and flush: run what is queued first
            (void)flush_batch(all);
            return queue_frame(codec, aout_f, aout_s, result, cells, bits_out, cur, prev, enh, soft);
        }
    }
    Shard& b = *all.shards[at.shard];
    const int c = at.channel;
    QChannel& ch = b.channels[(size_t)c];
    ch.codec = codec;
    ch.soft = soft != nullptr;
    ch.pending++;
    b.q.emplace_back();
    QEntry& qe = b.q.back();
    qe.aout = aout_s ? static_cast<void*>(aout_s) : static_cast<void*>(aout_f);
    qe.want_short = aout_s ? 1 : 0;
    qe.result = result;
    qe.bits_out = bits_out;
    qe.channel = c;
    qe.codec = (uint8_t)codec;
    if (soft) {
        qe.soft_at = b.soft_cells.size();
        b.soft_cells.insert(b.soft_cells.end(), soft, soft + ncell);
        return 0;
    }
    rc = pack_one(codec, cells, qe.frame);
    if (rc < 0) {
        b.q.pop_back();
        ch.pending--;
        return rc;
    }
    return 0;
}

bool queueing() { return batch().active; }

// mbe_process*SoftFrame[f] inside queue mode with MBE_BATCH_QUEUE_SOFT.  Only a call the synchronous path would run to the end
// is queued: with a NULL argument that path reports its own status after writing what the reference writes, so it keeps the call.
bool queue_soft_call(const void* aout, const void* cells, const char* bits_out, const mbe_parms* cur, const mbe_parms* prev,
                     const mbe_parms* enh) {
    const Batch& b = batch();
    return b.active && b.queue_soft && aout && cells && bits_out && cur && prev && enh;
}

// the queued soft call: a refused frame leaves *result cleared, as the synchronous call does; a queued one writes nothing before the flush
int queue_soft_frame(int codec, float* aout_f, short* aout_s, mbe_process_result* result, const mbe_soft_bit* cells, char* bits_out,
                     mbe_parms* cur, mbe_parms* prev, mbe_parms* enh) {
    const int rc = queue_frame(codec, aout_f, aout_s, result, nullptr, bits_out, cur, prev, enh, cells);
    if (rc < 0 && result) {
        memset(result, 0, sizeof(*result));
    }
    return rc;
}

// mbe_process*Frame[f], synchronous: frame decode + parameter processing as ONE launch of one wavefront (mbx_process_frame:
// FEC by lane 0, then the LDS-resident stream body) on the caller's structs copied into the thread's pinned block; the
// host waits on the kernel's completion word, not on the stream.  The record the FEC kernel hands
// to the stream stage is the one the reference's two calls hand over through imbe_d / result (c0, protected, c4, context
// flags), so the outcome is that of mbe_decode*Frame followed by mbe_process*Dataf.  Argument errors that the reference
// reports only AFTER the frame decode has written imbe_d / result take the two-call path below, which does the same.
int process_frame(int codec, float* aout_f, short* aout_s, mbe_process_result* result, const char* cells, char* bits_out,
                  mbe_parms* cur, mbe_parms* prev, mbe_parms* enh) {
    const mbx::CodecShape& sh = mbx::kCodecs[codec];
    if (!bits_out || (!aout_f && !aout_s) || !cur || !prev || !enh) {
        mbe_process_result local;
        mbe_process_result* r = result ? result : &local;
        const int rc = decode_frame(sh.front, cells, bits_out, r);
        if (rc < 0) {
            return rc;
        }
        return process_data(codec, aout_f, aout_s, r, bits_out, cur, prev, enh);
    }
    if (result) {
        memset(result, 0, sizeof(*result));
    }
    int rc = validate_bits(cells, (size_t)sh.cells);
    if (rc < 0) {
        return rc;
    }
    sync_channel_for_direct_use(cur);
    Slot& s = slot();
    rc = pack_one(codec, cells, s.frame);
    if (rc < 0) {
        return rc;
    }
    // The caller's structs still are what the previous call handed back (the usual case: a decoder calling frame after frame)?
    // Then the pinned block already holds them and the device has them in HBM: nothing is copied, and the kernel reads its state
    // from the device copy.  Compared by content: 7.8 KB, ~0.2 us.
    const bool from_shadow = s.shadow_valid && memcmp(cur, &s.state[0], sizeof(mbe_parms)) == 0
                             && memcmp(prev, &s.state[1], sizeof(mbe_parms)) == 0 && memcmp(enh, &s.state[2], sizeof(mbe_parms)) == 0
                             && memcmp(&t_rng.r, s.rng, sizeof(mbx_stream_rng)) == 0;
    if (!from_shadow) {
        s.up(&s.state[0], cur, sizeof(mbe_parms));
        s.up(&s.state[1], prev, sizeof(mbe_parms));
        s.up(&s.state[2], enh, sizeof(mbe_parms));
        s.up(s.rng, &t_rng.r, sizeof(mbx_stream_rng));
    }
    *s.shadow_ok = 0u;
    if (g_frame_server) {
        s.serve(codec, aout_s ? s.pcm16 : nullptr, aout_f ? s.pcmf : nullptr, from_shadow);
    } else {
        const uint32_t token = ++s.token;
        must(mbx_process_frame_shadow(codec, s.frame, s.state, s.rng, aout_s ? s.pcm16 : nullptr, aout_f ? s.pcmf : nullptr, s.res, s.rec,
                                      s.done, token, s.d_shadow, s.d_shadow_rng, s.shadow_ok, from_shadow ? 1 : 0, s.frame, s.stream),
             "mbx_process_frame_shadow");
        s.wait_token(token);
    }
    s.shadow_valid = g_frame_shadow && __atomic_load_n(s.shadow_ok, __ATOMIC_ACQUIRE) == 1u;
    if (aout_f) {
        memcpy(aout_f, s.pcmf, 160 * sizeof(float));
    }
    if (aout_s) {
        memcpy(aout_s, s.pcm16, 160 * sizeof(int16_t));
    }
    *cur = s.state[0];
    *prev = s.state[1];
    *enh = s.state[2];
    t_rng.r = *s.rng;
    mbx_unpack_records(s.rec, 1, sh.data_bits, bits_out, nullptr);
    const int total = s.res->total_errors;
    if (result) {
        *result = *s.res;
    }
    return total;
}

// The sixteen mbe_process*Frame[f] / mbe_process*SoftFrame[f] exports: a float form passes aout_f, a short form aout_s -- after it has
// refused a NULL buffer, before anything is written; a float form's NULL buffer is reported by the calls below, after the frame
// decode has cleared *result and written the parameter bits, as in the reference.
int hard_frame_call(int codec, float* aout_f, short* aout_s, mbe_process_result* result, const char* cells, char* bits_out, mbe_parms* cur,
                    mbe_parms* prev, mbe_parms* enh) {
    return queueing() ? queue_frame(codec, aout_f, aout_s, result, cells, bits_out, cur, prev, enh)
                      : process_frame(codec, aout_f, aout_s, result, cells, bits_out, cur, prev, enh);
}

// soft frames, ref src/imbe/imbe7200x4400.c:950-980, src/ambe/ambe3600x2450.c:939-969: mbe_decode*SoftFrame of the codec's front
// end, then mbe_process*Data[f] of its stream stage
int soft_frame_call(int codec, float* aout_f, short* aout_s, mbe_process_result* result, const mbe_soft_bit* cells, char* bits_out,
                    mbe_parms* cur, mbe_parms* prev, mbe_parms* enh) {
    if (queue_soft_call(aout_s ? static_cast<const void*>(aout_s) : aout_f, cells, bits_out, cur, prev, enh)) {
        return queue_soft_frame(codec, aout_f, aout_s, result, cells, bits_out, cur, prev, enh);
    }
    mbe_process_result local;
    if (!result) {
        result = &local;
    }
    const int rc = decode_soft_frame(mbx::kCodecs[codec].front, cells, bits_out, result);
    if (rc < 0) {
        return rc;
    }
    return process_data(mbx::kCodecs[codec].stream, aout_f, aout_s, result, bits_out, cur, prev, enh);
}

}  // namespace

extern "C" {

const char* mbe_versionString(void) { return "2.0.0+mi355x"; }

void mbe_initProcessResult(mbe_process_result* result) {
    if (result) {
        memset(result, 0, sizeof(*result));
    }
}

void mbe_setThreadRngSeed(uint32_t seed) { mbx_rng_seed(&t_rng.r, seed); }

void mbe_moveMbeParms(const mbe_parms* source_mp, mbe_parms* destination_mp) {
    sync_channel_for_direct_use(source_mp);        // queue mode: a struct of a resident channel is stale on the host
    sync_channel_for_direct_use(destination_mp);
    if (source_mp && destination_mp) {
        *destination_mp = *source_mp;
    }
}

void mbe_useLastMbeParms(mbe_parms* cur_mp, const mbe_parms* prev_mp) {
    sync_channel_for_direct_use(cur_mp);
    sync_channel_for_direct_use(prev_mp);
    if (cur_mp && prev_mp) {
        *cur_mp = *prev_mp;
    }
}

// defaults only, no signal processing: ref src/core/mbelib.c:367-410
void mbe_initMbeParms(mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    if (!cur_mp || !prev_mp || !prev_mp_enhanced) {
        return;
    }
    // queue mode: a host that resets a channel at call start gets a reset -- the channel leaves the device pool first,
    // otherwise mbe_batchEnd / mbe_batchRelease would write the old device state over these defaults
    sync_channel_for_direct_use(cur_mp);
    sync_channel_for_direct_use(prev_mp);
    sync_channel_for_direct_use(prev_mp_enhanced);
    mbe_parms p;
    memset(&p, 0, sizeof(p));
    p.w0 = (float)((4.0 * M_PI) / (134.0 + 39.5));
    p.L = (int)(0.9254 * (int)((M_PI / p.w0) + 0.25));
    p.K = 12;
    for (int l = 0; l <= 56; ++l) {
        p.Ml[l] = 1.0f;
    }
    p.localEnergy = 75000.0f;
    p.amplitudeThreshold = 20480;
    p.mutingThreshold = MBE_MUTING_THRESHOLD_IMBE;
    p.noiseSeed = -1.0f;
    *prev_mp = p;
    *cur_mp = p;
    *prev_mp_enhanced = p;
}

int mbe_requiresAdaptiveSmoothing(const mbe_parms* mp) { return mp ? ((mp->errorRate > 0.0125f) || (mp->errorCountTotal > 4)) : 0; }
int mbe_requiresMuting(const mbe_parms* mp) { return mp ? (mp->errorRate > mp->mutingThreshold) : 0; }
int mbe_isMaxFrameRepeat(const mbe_parms* mp) { return mp ? (mp->repeatCount >= MBE_MAX_FRAME_REPEATS) : 0; }

void mbe_synthesizeSilencef(float* aout_buf) {
    if (aout_buf) {
        memset(aout_buf, 0, 160 * sizeof(float));
    }
}

void mbe_synthesizeSilence(short* aout_buf) {
    if (aout_buf) {
        memset(aout_buf, 0, 160 * sizeof(short));
    }
}

// ---- ECC words ------------------------------------------------------------------------------
int mbe_checkGolayBlock(long int* block) {
    if (!block) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const uint32_t block_u = (uint32_t)(*block);
    uint32_t fixed;
    (void)ecc_word(0, block_u & 0x7fffffu, &fixed);
    // the reference corrects (block >> 11) as a whole (ref src/ecc/ecc.c:246-249): bits above the 23-bit code word pass through
    *block = (long)(int)((fixed >> 11) | ((block_u >> 23) << 12));
    return 0;
}

int mbe_golay2312(const char* in, char* out) {
    if (!out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(in, 23u);
    if (rc < 0) {
        return rc;
    }
    uint32_t cw = 0, fixed;
    for (int j = 22; j >= 0; --j) {
        cw = (cw << 1) | (uint32_t)(in[j] & 1);
    }
    const int errs = ecc_word(0, cw, &fixed);
    for (int j = 0; j < 23; ++j) {
        out[j] = (char)((fixed >> j) & 1u);
    }
    return errs;
}

int mbe_hamming1511(const char* in, char* out) {
    if (!out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(in, 15u);
    if (rc < 0) {
        return rc;
    }
    uint32_t cw = 0, fixed;
    for (int j = 14; j >= 0; --j) {
        cw = (cw << 1) | (uint32_t)(in[j] & 1);
    }
    const int errs = ecc_word(1, cw, &fixed);
    for (int j = 0; j < 15; ++j) {
        out[j] = (char)((fixed >> j) & 1u);
    }
    return errs;
}

// ---- IMBE 7100x4400: ref src/ecc/ecc.c:422-464, src/imbe/imbe7100x4400.c:381-479, 527-592 -------
int mbe_7100x4400hamming1511(const char* in, char* out) {
    if (!out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(in, 15u);
    if (rc < 0) {
        return rc;
    }
    uint32_t cw = 0, fixed;
    for (int j = 14; j >= 0; --j) {
        cw = (cw << 1) | (uint32_t)(in[j] & 1);
    }
    const int errs = ecc_word(2, cw, &fixed);
    for (int j = 0; j < 15; ++j) {
        out[j] = (char)((fixed >> j) & 1u);
    }
    return errs;
}

int mbe_decodeImbe7100x4400Frame(const char imbe_fr[7][24], char imbe_d[88], mbe_process_result* result) {
    return decode_frame(MBX_CODEC_IMBE7100X4400, reinterpret_cast<const char*>(imbe_fr), imbe_d, result);
}

int mbe_processImbe7100x4400Framef(float* aout_buf, mbe_process_result* result, const char imbe_fr[7][24], char imbe_d[88],
                                   mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return hard_frame_call(MBX_CODEC_IMBE7100X4400, aout_buf, nullptr, result, reinterpret_cast<const char*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processImbe7100x4400Frame(short* aout_buf, mbe_process_result* result, const char imbe_fr[7][24], char imbe_d[88],
                                  mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? hard_frame_call(MBX_CODEC_IMBE7100X4400, nullptr, aout_buf, result, reinterpret_cast<const char*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

// ---- tones and the status trace: ref src/core/mbelib.c:68-104 (format documented in mbelib.h:195-202), :745-856 ----
void mbe_formatProcessResult(char* str, size_t size, const mbe_process_result* result) {
    if (!str || size == 0u) {
        return;
    }
    size_t pos = 0u;
    const int total = (result && result->total_errors > 0) ? result->total_errors : 0;
    while (pos + 1u < size && (int)pos < total) {
        str[pos++] = '=';
    }
    if (result) {
        const unsigned order[4] = {MBE_PROCESS_FLAG_ERASURE, MBE_PROCESS_FLAG_TONE, MBE_PROCESS_FLAG_REPEAT, MBE_PROCESS_FLAG_MUTE};
        const char mark[4] = {'E', 'T', 'R', 'M'};
        for (int i = 0; i < 4 && pos + 1u < size; ++i) {
            if (result->flags & order[i]) {
                str[pos++] = mark[i];
            }
        }
    }
    str[pos] = '\0';
}

static void tone_call(float* aout_buf, const char* ambe_d, mbe_parms* cur_mp, const int* dstar_id) {
    if (!aout_buf) {
        return;
    }
    memset(aout_buf, 0, 160 * sizeof(float));
    if (!cur_mp) {
        return;
    }
    Slot& s = slot();
    int32_t id = 0;
    if (dstar_id) {
        id = *dstar_id;
        s.up(&s.words[0], &id, sizeof(id));
    } else {
        if (validate_bits(ambe_d, 49u) < 0) {
            return;
        }
        mbe_process_result none;
        memset(&none, 0, sizeof(none));
        const mbx_param_record rec = make_record(ambe_d, 49, &none, 0);
        s.up(s.rec, &rec, sizeof(rec));
    }
    s.up(&s.state[0], cur_mp, sizeof(mbe_parms));
    must(mbx_synthesize_tone(1, dstar_id ? nullptr : s.rec, dstar_id ? reinterpret_cast<const int32_t*>(&s.words[0]) : nullptr,
                             &s.state[0], s.pcmf, nullptr, s.stream),
         "mbx_synthesize_tone");
    s.down(aout_buf, s.pcmf, 160 * sizeof(float));
    s.down(cur_mp, &s.state[0], sizeof(mbe_parms));
    s.sync();
}

void mbe_synthesizeTonef(float* aout_buf, const char* ambe_d, mbe_parms* cur_mp) { tone_call(aout_buf, ambe_d, cur_mp, nullptr); }

void mbe_synthesizeTonefdstar(float* aout_buf, const char* ambe_d, mbe_parms* cur_mp, int ID1) {
    (void)ambe_d;
    tone_call(aout_buf, nullptr, cur_mp, &ID1);
}

// ---- soft-decision helpers: ref src/core/mbelib.c:107-158, src/ecc/ecc.c:303-357, 410-413 -----
mbe_soft_bit mbe_softBitFromHard(int bit, uint8_t reliability) {
    mbe_soft_bit s;
    s.bit = (uint8_t)(bit ? 1u : 0u);
    s.reliability = reliability;
    return s;
}

mbe_soft_bit mbe_softBitFromLlr(int16_t llr) {
    mbe_soft_bit s;
    (void)mbx_soft_bits_from_llr(&llr, &s, 1);
    return s;
}

int mbe_softBitsFromHard(const char* bits, mbe_soft_bit* soft, size_t count, uint8_t reliability) {
    if (!soft) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(bits, count);
    if (rc < 0) {
        return rc;
    }
    return mbx_soft_bits_from_hard(bits, soft, count, reliability);
}

int mbe_softBitsFromLlr(const int16_t* llr, mbe_soft_bit* soft, size_t count) { return mbx_soft_bits_from_llr(llr, soft, count); }

int mbe_golay2312Soft(const mbe_soft_bit* in, char* out) {
    if (!out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = mbx_validate_soft_bits(in, 23u);
    if (rc < 0) {
        return rc;
    }
    uint32_t w;
    const int diffs = ecc_soft_word(0, in, &w);
    for (int j = 0; j < 23; ++j) {
        out[j] = (char)((w >> j) & 1u);
    }
    return diffs;
}

int mbe_hamming1511Soft(const mbe_soft_bit* in, char* out) {
    if (!out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = mbx_validate_soft_bits(in, 15u);
    if (rc < 0) {
        return rc;
    }
    uint32_t w;
    const int diffs = ecc_soft_word(1, in, &w);
    for (int j = 0; j < 15; ++j) {
        out[j] = (char)((w >> j) & 1u);
    }
    return diffs;
}

int mbe_decodeImbe7200x4400SoftFrame(const mbe_soft_bit imbe_fr[8][23], char imbe_d[88], mbe_process_result* result) {
    return decode_soft_frame(MBX_CODEC_IMBE7200X4400, reinterpret_cast<const mbe_soft_bit*>(imbe_fr), imbe_d, result);
}

int mbe_decodeAmbe3600x2450SoftFrame(const mbe_soft_bit ambe_fr[4][24], char ambe_d[49], mbe_process_result* result) {
    return decode_soft_frame(MBX_CODEC_AMBE3600X2450, reinterpret_cast<const mbe_soft_bit*>(ambe_fr), ambe_d, result);
}


// ---- queue mode (include/mbe_neo_amd.h) -----------------------------------------------------------------------------
int mbe_batchBegin(int state_mode) {
    Batch& b = batch();
    const bool queue_soft = state_mode >= 0 && (state_mode & MBE_BATCH_QUEUE_SOFT) != 0;
    if (queue_soft) {
        state_mode &= ~MBE_BATCH_QUEUE_SOFT;
    }
    if (b.active || (state_mode != MBE_BATCH_STATE_WRITEBACK && state_mode != MBE_BATCH_STATE_RESIDENT)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    b.home = slot().home;   // the thread's device scratch and stream exist from here on
    b.created = 0;
    b.active = true;
    b.queue_soft = queue_soft;
    b.mode = state_mode;
    for (int i = 0; i < g_shards.n; ++i) {
        if (b.shards[i]) {
            b.shards[i]->mode = state_mode;
            b.shards[i]->passes = b.shards[i]->rows = 0;
        }
    }
    return 0;
}

int mbe_flush(void) {
    Batch& b = batch();
    return b.active ? flush_batch(b) : 0;
}

int mbe_batchPending(void) { return (int)batch().pending(); }

int mbe_batchRelease(mbe_parms* cur_mp) {
    Batch& b = batch();
    if (!b.active || !cur_mp) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    (void)flush_batch(b);
    auto it = b.index.find(cur_mp);
    if (it != b.index.end()) {
        release_channel(b, it->second);
    }
    return 0;
}

int mbe_batchEnd(void) {
    Batch& b = batch();
    if (!b.active) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const int ran = flush_batch(b);
    Slot& home = slot();
    for (int i = 0; i < g_shards.n; ++i) {
        if (!b.shards[i]) {
            continue;
        }
        Shard& sh = *b.shards[i];
        if (sh.resident) {   // resident mode: slot == channel index
            std::vector<int> owners(sh.resident);
            for (size_t c = 0; c < sh.resident; ++c) {
                owners[c] = (int)c;
            }
            use_device(sh.lane.device);
            pool_download(sh, sh.lane, 0, owners, false);
        }
        sh.channels.clear();
        sh.resident = 0;
    }
    use_device(home.device);
    if (g_trace_flush && t_flush_trace.flushes) {
        const FlushTrace& t = t_flush_trace;
        fprintf(stderr, "[flush trace] %ld flushes, %.0f rows each: prep %.1f us, issue %.1f us, wait %.1f us, scatter %.1f us per flush\n", t.flushes,
                (double)t.rows / (double)t.flushes, 1e6 * t.prep / t.flushes, 1e6 * t.issue / t.flushes, 1e6 * t.wait / t.flushes,
                1e6 * t.scatter / t.flushes);
        t_flush_trace = FlushTrace{};
    }
    b.index.clear();
    b.aux.clear();
    b.active = false;
    return ran;
}

// ---- the shards from outside (include/mbe_neo_shards.h) ---------------------------------------------------------------
int mbq_shard_count(void) {
    std::call_once(g_once, init_once);
    return g_shards.n;
}

int mbq_shard_device(int shard) { return shard >= 0 && shard < mbq_shard_count() ? g_shards.device[shard] : -1; }

int mbq_thread_home(void) { return slot().home; }

int mbq_channel_shard(const void* cur_mp) {
    const Batch& b = batch();
    auto it = b.index.find(static_cast<const mbe_parms*>(cur_mp));
    return b.active && it != b.index.end() ? it->second.shard : -1;
}

int mbq_shard_census(int shard, mbq_census* out) {
    if (!out || shard < 0 || shard >= mbq_shard_count()) {
        return -1;
    }
    memset(out, 0, sizeof(*out));
    if (const Shard* sh = batch().shards[shard].get()) {
        out->flush_passes = sh->passes;
        out->rows = sh->rows;
        out->channels = (int)sh->channels.size();
        out->resident = (int)sh->resident;
    }
    return 0;
}

// ---- frame decode ---------------------------------------------------------------------------
int mbe_decodeImbe7200x4400Frame(const char imbe_fr[8][23], char imbe_d[88], mbe_process_result* result) {
    return decode_frame(MBX_CODEC_IMBE7200X4400, reinterpret_cast<const char*>(imbe_fr), imbe_d, result);
}

int mbe_decodeAmbe3600x2450Frame(const char ambe_fr[4][24], char ambe_d[49], mbe_process_result* result) {
    return decode_frame(MBX_CODEC_AMBE3600X2450, reinterpret_cast<const char*>(ambe_fr), ambe_d, result);
}

// ---- parameters -> PCM ------------------------------------------------------------------------
int mbe_processImbe4400Dataf(float* aout_buf, mbe_process_result* result, const char imbe_d[88], mbe_parms* cur_mp,
                             mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return process_data(MBX_CODEC_IMBE7200X4400, aout_buf, nullptr, result, imbe_d, cur_mp, prev_mp, prev_mp_enhanced);
}

int mbe_processImbe4400Data(short* aout_buf, mbe_process_result* result, const char imbe_d[88], mbe_parms* cur_mp,
                            mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    if (!aout_buf) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return process_data(MBX_CODEC_IMBE7200X4400, nullptr, aout_buf, result, imbe_d, cur_mp, prev_mp, prev_mp_enhanced);
}

int mbe_processAmbe2450Dataf(float* aout_buf, mbe_process_result* result, const char ambe_d[49], mbe_parms* cur_mp,
                             mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return process_data(MBX_CODEC_AMBE3600X2450, aout_buf, nullptr, result, ambe_d, cur_mp, prev_mp, prev_mp_enhanced);
}

int mbe_processAmbe2450Data(short* aout_buf, mbe_process_result* result, const char ambe_d[49], mbe_parms* cur_mp,
                            mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    if (!aout_buf) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return process_data(MBX_CODEC_AMBE3600X2450, nullptr, aout_buf, result, ambe_d, cur_mp, prev_mp, prev_mp_enhanced);
}

// ---- frames -> PCM: ref src/imbe/imbe7200x4400.c:935-1001, src/ambe/ambe3600x2450.c:924-990 ------
int mbe_processImbe7200x4400Framef(float* aout_buf, mbe_process_result* result, const char imbe_fr[8][23], char imbe_d[88],
                                   mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return hard_frame_call(MBX_CODEC_IMBE7200X4400, aout_buf, nullptr, result, reinterpret_cast<const char*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processImbe7200x4400Frame(short* aout_buf, mbe_process_result* result, const char imbe_fr[8][23], char imbe_d[88],
                                  mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? hard_frame_call(MBX_CODEC_IMBE7200X4400, nullptr, aout_buf, result, reinterpret_cast<const char*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

int mbe_processAmbe3600x2450Framef(float* aout_buf, mbe_process_result* result, const char ambe_fr[4][24], char ambe_d[49],
                                   mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return hard_frame_call(MBX_CODEC_AMBE3600X2450, aout_buf, nullptr, result, reinterpret_cast<const char*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processAmbe3600x2450Frame(short* aout_buf, mbe_process_result* result, const char ambe_fr[4][24], char ambe_d[49],
                                  mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? hard_frame_call(MBX_CODEC_AMBE3600X2450, nullptr, aout_buf, result, reinterpret_cast<const char*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

// ---- synthesis pieces --------------------------------------------------------------------------
void mbe_synthesizeSpeechf(float* aout_buf, mbe_parms* cur_mp, mbe_parms* prev_mp) {
    if (!aout_buf) {
        return;
    }
    sync_channel_for_direct_use(cur_mp);
    sync_channel_for_direct_use(prev_mp);
    if (!cur_mp || !prev_mp || !valid_L(cur_mp->L) || !valid_L(prev_mp->L)) {
        mbe_synthesizeSilencef(aout_buf);
        return;
    }
    synth_speech(aout_buf, nullptr, cur_mp, prev_mp);
}

void mbe_synthesizeSpeech(short* aout_buf, mbe_parms* cur_mp, mbe_parms* prev_mp) {
    if (!aout_buf) {
        return;
    }
    sync_channel_for_direct_use(cur_mp);
    sync_channel_for_direct_use(prev_mp);
    if (!cur_mp || !prev_mp || !valid_L(cur_mp->L) || !valid_L(prev_mp->L)) {
        mbe_synthesizeSilence(aout_buf);
        return;
    }
    synth_speech(nullptr, aout_buf, cur_mp, prev_mp);
}

void mbe_spectralAmpEnhance(mbe_parms* cur_mp) {
    sync_channel_for_direct_use(cur_mp);
    if (!cur_mp || !valid_L(cur_mp->L)) {
        return;
    }
    Slot& s = slot();
    s.up(&s.state[0], cur_mp, sizeof(mbe_parms));
    must(mbx_spectral_amp_enhance(1, &s.state[0], s.stream), "mbx_spectral_amp_enhance");
    s.down(cur_mp, &s.state[0], sizeof(mbe_parms));
    s.sync();
}

void mbe_applyAdaptiveSmoothing(mbe_parms* cur_mp, const mbe_parms* prev_mp) {
    sync_channel_for_direct_use(cur_mp);
    sync_channel_for_direct_use(prev_mp);
    if (!cur_mp || !prev_mp || !valid_L(cur_mp->L) || !valid_L(prev_mp->L)) {
        return;
    }
    Slot& s = slot();
    s.up(&s.state[0], cur_mp, sizeof(mbe_parms));
    s.up(&s.state[1], prev_mp, sizeof(mbe_parms));
    must(mbx_adaptive_smoothing(1, &s.state[0], &s.state[1], s.stream), "mbx_adaptive_smoothing");
    s.down(cur_mp, &s.state[0], sizeof(mbe_parms));
    s.sync();
}

void mbe_floattoshort(const float* float_buf, short* aout_buf) {
    if (!float_buf || !aout_buf) {
        return;
    }
    Slot& s = slot();
    s.up(s.pcmf, float_buf, 160 * sizeof(float));
    must(mbx_floattoshort(s.pcmf, s.pcm16, 1, s.stream), "mbx_floattoshort");
    s.down(aout_buf, s.pcm16, 160 * sizeof(int16_t));
    s.sync();
}

void mbe_synthesizeComfortNoisef(float* aout_buf) {
    if (!aout_buf) {
        return;
    }
    Slot& s = slot();
    s.up(s.rng, &t_rng.r, sizeof(mbx_stream_rng));
    must(mbx_comfort_noise(1, s.rng, s.pcmf, nullptr, s.stream), "mbx_comfort_noise");
    s.down(aout_buf, s.pcmf, 160 * sizeof(float));
    s.down(&t_rng.r, s.rng, sizeof(mbx_stream_rng));
    s.sync();
}

void mbe_synthesizeComfortNoise(short* aout_buf) {
    if (!aout_buf) {
        return;
    }
    Slot& s = slot();
    s.up(s.rng, &t_rng.r, sizeof(mbx_stream_rng));
    must(mbx_comfort_noise(1, s.rng, nullptr, s.pcm16, s.stream), "mbx_comfort_noise");
    s.down(aout_buf, s.pcm16, 160 * sizeof(int16_t));
    s.down(&t_rng.r, s.rng, sizeof(mbx_stream_rng));
    s.sync();
}

// ---- soft IMBE 7100x4400: ref src/ecc/ecc.c:466-469, src/imbe/imbe7100x4400.c:481-525, 542-576 -------------
int mbe_7100x4400hamming1511Soft(const mbe_soft_bit* in, char* out) {
    if (!out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = mbx_validate_soft_bits(in, 15u);
    if (rc < 0) {
        return rc;
    }
    uint32_t w;
    const int diffs = ecc_soft_word(2, in, &w);
    for (int j = 0; j < 15; ++j) {
        out[j] = (char)((w >> j) & 1u);
    }
    return diffs;
}

int mbe_decodeImbe7100x4400SoftFrame(const mbe_soft_bit imbe_fr[7][24], char imbe_d[88], mbe_process_result* result) {
    return decode_soft_frame(MBX_CODEC_IMBE7100X4400, reinterpret_cast<const mbe_soft_bit*>(imbe_fr), imbe_d, result);
}

int mbe_processImbe7100x4400SoftFramef(float* aout_buf, mbe_process_result* result, const mbe_soft_bit imbe_fr[7][24],
                                       char imbe_d[88], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return soft_frame_call(MBX_CODEC_IMBE7100X4400, aout_buf, nullptr, result, reinterpret_cast<const mbe_soft_bit*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processImbe7100x4400SoftFrame(short* aout_buf, mbe_process_result* result, const mbe_soft_bit imbe_fr[7][24],
                                      char imbe_d[88], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? soft_frame_call(MBX_CODEC_IMBE7100X4400, nullptr, aout_buf, result, reinterpret_cast<const mbe_soft_bit*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

// ---- AMBE 3600x2400 (D-STAR): ref src/ambe/ambe3600x2400.c:563-627 (frame decode = the AMBE+2 one), :733-852 --
int mbe_decodeAmbe3600x2400Frame(const char ambe_fr[4][24], char ambe_d[49], mbe_process_result* result) {
    return decode_frame(MBX_CODEC_AMBE3600X2450, reinterpret_cast<const char*>(ambe_fr), ambe_d, result);
}

int mbe_decodeAmbe3600x2400SoftFrame(const mbe_soft_bit ambe_fr[4][24], char ambe_d[49], mbe_process_result* result) {
    return decode_soft_frame(MBX_CODEC_AMBE3600X2450, reinterpret_cast<const mbe_soft_bit*>(ambe_fr), ambe_d, result);
}

int mbe_processAmbe2400Dataf(float* aout_buf, mbe_process_result* result, const char ambe_d[49], mbe_parms* cur_mp,
                             mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return process_data(MBX_CODEC_AMBE3600X2400, aout_buf, nullptr, result, ambe_d, cur_mp, prev_mp, prev_mp_enhanced);
}

int mbe_processAmbe2400Data(short* aout_buf, mbe_process_result* result, const char ambe_d[49], mbe_parms* cur_mp,
                            mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    if (!aout_buf) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return process_data(MBX_CODEC_AMBE3600X2400, nullptr, aout_buf, result, ambe_d, cur_mp, prev_mp, prev_mp_enhanced);
}

int mbe_processAmbe3600x2400Framef(float* aout_buf, mbe_process_result* result, const char ambe_fr[4][24], char ambe_d[49],
                                   mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return hard_frame_call(MBX_CODEC_AMBE3600X2400, aout_buf, nullptr, result, reinterpret_cast<const char*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processAmbe3600x2400Frame(short* aout_buf, mbe_process_result* result, const char ambe_fr[4][24], char ambe_d[49],
                                  mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? hard_frame_call(MBX_CODEC_AMBE3600X2400, nullptr, aout_buf, result, reinterpret_cast<const char*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

int mbe_processAmbe3600x2400SoftFramef(float* aout_buf, mbe_process_result* result, const mbe_soft_bit ambe_fr[4][24],
                                       char ambe_d[49], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return soft_frame_call(MBX_CODEC_AMBE3600X2400, aout_buf, nullptr, result, reinterpret_cast<const mbe_soft_bit*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processAmbe3600x2400SoftFrame(short* aout_buf, mbe_process_result* result, const mbe_soft_bit ambe_fr[4][24],
                                      char ambe_d[49], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? soft_frame_call(MBX_CODEC_AMBE3600X2400, nullptr, aout_buf, result, reinterpret_cast<const mbe_soft_bit*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

// ---- soft frames -> PCM: ref src/imbe/imbe7200x4400.c:950-980, src/ambe/ambe3600x2450.c:939-969 --------
int mbe_processImbe7200x4400SoftFramef(float* aout_buf, mbe_process_result* result, const mbe_soft_bit imbe_fr[8][23],
                                       char imbe_d[88], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return soft_frame_call(MBX_CODEC_IMBE7200X4400, aout_buf, nullptr, result, reinterpret_cast<const mbe_soft_bit*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processImbe7200x4400SoftFrame(short* aout_buf, mbe_process_result* result, const mbe_soft_bit imbe_fr[8][23],
                                      char imbe_d[88], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? soft_frame_call(MBX_CODEC_IMBE7200X4400, nullptr, aout_buf, result, reinterpret_cast<const mbe_soft_bit*>(imbe_fr), imbe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

int mbe_processAmbe3600x2450SoftFramef(float* aout_buf, mbe_process_result* result, const mbe_soft_bit ambe_fr[4][24],
                                       char ambe_d[49], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return soft_frame_call(MBX_CODEC_AMBE3600X2450, aout_buf, nullptr, result, reinterpret_cast<const mbe_soft_bit*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                           prev_mp_enhanced);
}

int mbe_processAmbe3600x2450SoftFrame(short* aout_buf, mbe_process_result* result, const mbe_soft_bit ambe_fr[4][24],
                                      char ambe_d[49], mbe_parms* cur_mp, mbe_parms* prev_mp, mbe_parms* prev_mp_enhanced) {
    return aout_buf ? soft_frame_call(MBX_CODEC_AMBE3600X2450, nullptr, aout_buf, result, reinterpret_cast<const mbe_soft_bit*>(ambe_fr), ambe_d, cur_mp, prev_mp,
                                      prev_mp_enhanced)
                    : MBE_STATUS_INVALID_ARGUMENT;
}

}  // extern "C"

// ==================================================================================================================
// The classic call sequence, stage by stage: ref include/mbelib-neo/mbelib.h:286-307, 381-387, 457-463, 531-537.
// Each helper validates like the reference, runs its stage on the device (mbx_fec_stage: a slice of the frame kernel) and
// writes back exactly the cells the reference writes.
// ==================================================================================================================
namespace {

// rows [r0, r1] of a packed frame back into the caller's cell array (the other cells are left alone, like the reference)
void unpack_rows(int codec, const uint8_t* packed, char* cells, int r0, int r1) {
    const mbx::CodecShape& sh = mbx::kCodecs[codec];
    int pos = 0;
    for (int r = 0; r < sh.rows; ++r) {
        for (int j = sh.width[r] - 1; j >= 0; --j, ++pos) {
            if (r >= r0 && r <= r1) {
                cells[r * sh.stride + j] = (char)((packed[pos >> 3] >> (7 - (pos & 7))) & 1);
            }
        }
    }
}

// stage 1 (C0 ECC) or 2 (demodulation), in place; returns the reference's return value
int frame_stage(int codec, int stage, char* cells) {
    const mbx::CodecShape& sh = mbx::kCodecs[codec];
    int rc = validate_bits(cells, (size_t)sh.cells);
    if (rc < 0) {
        return rc;
    }
    uint8_t packed[MBX_IMBE_FRAME_BYTES], back[MBX_IMBE_FRAME_BYTES];
    rc = pack_one(codec, cells, packed);
    if (rc < 0) {
        return rc;
    }
    Slot& s = slot();
    s.up(s.frame, packed, (size_t)sh.frame_bytes);
    must(mbx_fec_stage(codec, stage, s.frame, 1, s.frame_out, s.rec, s.stream), "mbx_fec_stage");
    mbx_param_record rec;
    s.down(back, s.frame_out, (size_t)sh.frame_bytes);
    s.down(&rec, s.rec, sizeof(rec));
    s.sync();
    if (stage == MBX_STAGE_C0) {
        if (codec == MBX_CODEC_IMBE7100X4400) {   // cells 1..18 of row 0 only (ref src/imbe/imbe7100x4400.c:100-122)
            const char keep = cells[0];
            unpack_rows(codec, back, cells, 0, 0);
            cells[0] = keep;
        } else {
            unpack_rows(codec, back, cells, 0, 0);
        }
        return (int)(rec.w[3] & 0xffu);
    }
    const int last = (codec == MBX_CODEC_IMBE7200X4400) ? 6 : (codec == MBX_CODEC_IMBE7100X4400 ? 5 : 1);
    unpack_rows(codec, back, cells, 1, last);
    return 0;
}

int frame_data_ecc(int codec, char* cells, char* bits_out) {
    const mbx::CodecShape& sh = mbx::kCodecs[codec];
    if (!bits_out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(cells, (size_t)sh.cells);
    if (rc < 0) {
        return rc;
    }
    uint8_t packed[MBX_IMBE_FRAME_BYTES];
    rc = pack_one(codec, cells, packed);
    if (rc < 0) {
        return rc;
    }
    Slot& s = slot();
    s.up(s.frame, packed, (size_t)sh.frame_bytes);
    must(mbx_fec_stage(codec, MBX_STAGE_DATA, s.frame, 1, nullptr, s.rec, s.stream), "mbx_fec_stage");
    mbx_param_record rec;
    s.down(&rec, s.rec, sizeof(rec));
    s.sync();
    mbx_unpack_records(&rec, 1, sh.data_bits, bits_out, nullptr);
    return (int)(rec.w[3] & 0xffu);
}

// mbe_decode*Parms: parameter decode alone (expand + prediction), both structs updated like the reference
int decode_parms(int codec, const char* bits, mbe_parms* cur, mbe_parms* prev) {
    const int nbits = mbx::kCodecs[codec].data_bits;
    if (!cur || !prev) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int rc = validate_bits(bits, (size_t)nbits);
    if (rc < 0) {
        return rc;
    }
    mbe_process_result none;
    memset(&none, 0, sizeof(none));
    const mbx_param_record rec = make_record(bits, nbits, &none, 0);   // no error context: the tone gate stays open (total_errors < 0 in the reference)
    Slot& s = slot();
    s.up(s.rec, &rec, sizeof(rec));
    s.up(&s.state[0], cur, sizeof(mbe_parms));
    s.up(&s.state[1], prev, sizeof(mbe_parms));
    must(mbx_decode_parms(codec, s.rec, 1, &s.state[0], &s.state[1], reinterpret_cast<int32_t*>(&s.words[0]), s.stream), "mbx_decode_parms");
    int32_t ret = 0;
    s.down(cur, &s.state[0], sizeof(mbe_parms));
    s.down(prev, &s.state[1], sizeof(mbe_parms));
    s.down(&ret, &s.words[0], sizeof(ret));
    s.sync();
    return (int)ret;
}

void dump_bits(const char* bits, int n, const int* gaps, int ngaps, bool trailing_space) {
    if (!bits) {
        return;
    }
    for (int i = 0; i < n; ++i) {
        for (int g = 0; g < ngaps; ++g) {
            if (gaps[g] == i) {
                fprintf(stderr, " ");
            }
        }
        fprintf(stderr, "%i", bits[i]);
    }
    if (trailing_space) {
        fprintf(stderr, " ");
    }
}

void dump_row(const char* row, int hi, int gap_at = -1) {
    for (int j = hi; j >= 0; --j) {
        if (j == gap_at) {
            fprintf(stderr, " ");
        }
        fprintf(stderr, "%i", row[j]);
    }
}

void dump_ambe_frame(const char fr[4][24]) {   // ref src/ambe/ambe3600x2450.c:113-142, src/ambe/ambe3600x2400.c:100-129
    if (!fr) {
        return;
    }
    static const int hi[4] = {23, 22, 10, 13};
    for (int r = 0; r < 4; ++r) {
        fprintf(stderr, "ambe_fr c%d: ", r);
        dump_row(fr[r], hi[r]);
        fprintf(stderr, " ");
    }
}

}  // namespace

extern "C" {

int mbe_eccImbe7200x4400C0(char imbe_fr[8][23]) { return frame_stage(MBX_CODEC_IMBE7200X4400, MBX_STAGE_C0, reinterpret_cast<char*>(imbe_fr)); }
int mbe_demodulateImbe7200x4400Data(char imbe[8][23]) { return frame_stage(MBX_CODEC_IMBE7200X4400, MBX_STAGE_DEMODULATE, reinterpret_cast<char*>(imbe)); }
int mbe_eccImbe7200x4400Data(char imbe_fr[8][23], char* imbe_d) { return frame_data_ecc(MBX_CODEC_IMBE7200X4400, reinterpret_cast<char*>(imbe_fr), imbe_d); }
int mbe_decodeImbe4400Parms(const char* imbe_d, mbe_parms* cur_mp, mbe_parms* prev_mp) { return decode_parms(MBX_CODEC_IMBE7200X4400, imbe_d, cur_mp, prev_mp); }

int mbe_eccAmbe3600x2450C0(char ambe_fr[4][24]) { return frame_stage(MBX_CODEC_AMBE3600X2450, MBX_STAGE_C0, reinterpret_cast<char*>(ambe_fr)); }
int mbe_demodulateAmbe3600x2450Data(char ambe_fr[4][24]) { return frame_stage(MBX_CODEC_AMBE3600X2450, MBX_STAGE_DEMODULATE, reinterpret_cast<char*>(ambe_fr)); }
int mbe_eccAmbe3600x2450Data(char ambe_fr[4][24], char* ambe_d) { return frame_data_ecc(MBX_CODEC_AMBE3600X2450, reinterpret_cast<char*>(ambe_fr), ambe_d); }
int mbe_decodeAmbe2450Parms(const char* ambe_d, mbe_parms* cur_mp, mbe_parms* prev_mp) { return decode_parms(MBX_CODEC_AMBE3600X2450, ambe_d, cur_mp, prev_mp); }

int mbe_eccAmbe3600x2400C0(char ambe_fr[4][24]) { return frame_stage(MBX_CODEC_AMBE3600X2400, MBX_STAGE_C0, reinterpret_cast<char*>(ambe_fr)); }
int mbe_demodulateAmbe3600x2400Data(char ambe_fr[4][24]) { return frame_stage(MBX_CODEC_AMBE3600X2400, MBX_STAGE_DEMODULATE, reinterpret_cast<char*>(ambe_fr)); }
int mbe_eccAmbe3600x2400Data(char ambe_fr[4][24], char* ambe_d) { return frame_data_ecc(MBX_CODEC_AMBE3600X2400, reinterpret_cast<char*>(ambe_fr), ambe_d); }
int mbe_decodeAmbe2400Parms(const char* ambe_d, mbe_parms* cur_mp, mbe_parms* prev_mp) { return decode_parms(MBX_CODEC_AMBE3600X2400, ambe_d, cur_mp, prev_mp); }

int mbe_eccImbe7100x4400C0(char imbe_fr[7][24]) { return frame_stage(MBX_CODEC_IMBE7100X4400, MBX_STAGE_C0, reinterpret_cast<char*>(imbe_fr)); }
int mbe_demodulateImbe7100x4400Data(char imbe[7][24]) { return frame_stage(MBX_CODEC_IMBE7100X4400, MBX_STAGE_DEMODULATE, reinterpret_cast<char*>(imbe)); }
int mbe_eccImbe7100x4400Data(char imbe_fr[7][24], char* imbe_d) { return frame_data_ecc(MBX_CODEC_IMBE7100X4400, reinterpret_cast<char*>(imbe_fr), imbe_d); }

int mbe_convertImbe7100to7200(char* imbe_d) {   // ref src/imbe/imbe7100x4400.c:381-438
    int rc = validate_bits(imbe_d, 88u);
    if (rc < 0) {
        return rc;
    }
    mbe_process_result none;
    memset(&none, 0, sizeof(none));
    const mbx_param_record rec = make_record(imbe_d, 88, &none, 0);
    Slot& s = slot();
    s.up(s.rec, &rec, sizeof(rec));
    mbx_param_record* d_out = reinterpret_cast<mbx_param_record*>(s.frame_out);   // 32 bytes: room for one record
    must(mbx_fec_stage(MBX_CODEC_IMBE7100X4400, MBX_STAGE_CONVERT7100, s.rec, 1, nullptr, d_out, s.stream), "mbx_fec_stage");
    mbx_param_record out;
    s.down(&out, d_out, sizeof(out));
    s.sync();
    mbx_unpack_records(&out, 1, 88, imbe_d, nullptr);
    return 0;
}

// ---- stderr dump helpers (host text only): formats of the reference, ref src/imbe/imbe7200x4400.c:356-418,
//      src/imbe/imbe7100x4400.c:24-92, src/ambe/ambe3600x2450.c:91-142, src/ambe/ambe3600x2400.c:78-129 ----
void mbe_dumpImbe4400Data(const char* imbe_d) { dump_bits(imbe_d, 88, nullptr, 0, false); }

void mbe_dumpImbe7200x4400Data(const char* imbe_d) {
    static const int gaps[7] = {12, 24, 36, 48, 59, 70, 81};
    dump_bits(imbe_d, 88, gaps, 7, false);
}

void mbe_dumpImbe7200x4400Frame(const char imbe_fr[8][23]) {
    if (!imbe_fr) {
        return;
    }
    for (int i = 0; i < 4; ++i) {
        dump_row(imbe_fr[i], 22);
        fprintf(stderr, " ");
    }
    for (int i = 4; i < 7; ++i) {
        dump_row(imbe_fr[i], 14);
        fprintf(stderr, " ");
    }
    dump_row(imbe_fr[7], 6);
}

void mbe_dumpImbe7100x4400Data(const char* imbe_d) {
    static const int gaps[6] = {7, 19, 31, 43, 54, 65};
    dump_bits(imbe_d, 88, gaps, 6, false);
}

void mbe_dumpImbe7100x4400Frame(const char imbe_fr[7][24]) {
    if (!imbe_fr) {
        return;
    }
    dump_row(imbe_fr[0], 18, 11);
    fprintf(stderr, " ");
    dump_row(imbe_fr[1], 23, 11);
    fprintf(stderr, " ");
    for (int i = 2; i < 4; ++i) {
        dump_row(imbe_fr[i], 22, 10);
        fprintf(stderr, " ");
    }
    for (int i = 4; i < 6; ++i) {
        dump_row(imbe_fr[i], 14, 3);
        fprintf(stderr, " ");
    }
    dump_row(imbe_fr[6], 22);
}

void mbe_dumpAmbe2450Data(const char* ambe_d) { dump_bits(ambe_d, 49, nullptr, 0, true); }
void mbe_dumpAmbe2400Data(const char* ambe_d) { dump_bits(ambe_d, 49, nullptr, 0, true); }
void mbe_dumpAmbe3600x2450Frame(const char ambe_fr[4][24]) { dump_ambe_frame(ambe_fr); }
void mbe_dumpAmbe3600x2400Frame(const char ambe_fr[4][24]) { dump_ambe_frame(ambe_fr); }

}  // extern "C"
