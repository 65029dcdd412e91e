// mbx_api.hip -- the C-ABI of libmbx_hip.so (declared in include/mbx.h): table upload,
// launchers, host-buffer conveniences.  No CPU compute path exists here: if HIP is not
// usable every entry point fails with MBX_ENODEVICE.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "mbx.h"
#include "mbx_cells.h"
#include "mbx_codec.h"
#include "mbx_derive.h"
#include "mbx_device.h"
#include "mbx_gather.h"
#include "mbx_host.h"
#include "mbx_kernels.h"
#include "mbx_keystream.h"
#include "mbx_keystream_words.h"
#include "mbx_launch_plan.h"
#include "mbx_llr.h"
#include "mbx_llr_cell.h"
#include "mbx_vote.h"
#include "mbx_vote_plan.h"

namespace {

// ---- per-device contexts ---------------------------------------------------------------------------------------
// One Context per HIP device, created by mbx_init(device, ...).  Every launcher works on the context of the calling
// thread's CURRENT device (hipGetDevice), like any other HIP call, so one process can drive all eight GPUs of a node:
// mbx_init() each device once, then hipSetDevice(d) before launching on d.  The reference keeps its mutable helper
// state thread-local and is re-entrant per stream (ref include/mbelib-neo/mbelib.h:28-30); here the only mutable
// launcher state is the per-(device, hipStream_t) StreamSlot below, guarded by the context's mutex, so any number of
// host threads may launch concurrently on their own streams (or on a shared one: launches of one call stay together).
constexpr int kMaxDevices = 32;

struct StreamSlot {                      // what a hipStream_t owns inside a context
    mbx::FrameParams* workspace = nullptr;   // expand-stage output of launches on this stream; grow-only
    size_t            frames = 0;
    uint32_t*         flags = nullptr;       // one-launch T = 1 step: ready word per chunk of eight rows (behind the rows, same allocation)
    uint32_t          epoch = 0;             // ... == the epoch of the launch that wrote them; a new value every launch
    hipStream_t       side[4] = {nullptr, nullptr, nullptr, nullptr};   // sliced launches: the internal streams the groups' slices are issued on ...
    hipEvent_t        fork = nullptr, join[4] = {nullptr, nullptr, nullptr, nullptr};   // ... and the events that hang them between the caller's launches
    unsigned          launches = 0;          // parity = direction in which the next stream-kernel launch walks the streams
    int               exp_codec = -1;        // what mbx_expand_records() last left in the workspace
    size_t            exp_n = 0;
    const void*       exp_records = nullptr;
};

struct Context {
    std::mutex         mu;                   // guards slots / reserve_frames; held across the launches of one call
    std::atomic<bool>  ready{false};
    int                device = -1;
    mbx::DeviceTables  tabs{nullptr, nullptr, 0, 0};
    void*              d_blob = nullptr;
    void*              d_derived = nullptr;
    uint32_t           checksum = 0;
    int                simds = 0;            // 4 per CU
    size_t             reserve_frames = 0;   // mbx_reserve(): minimum workspace of every slot
    std::unordered_map<void*, StreamSlot> slots;
    std::mutex         name_mu;              // guards last_kernel alone; a leaf lock (launch_stream runs with `mu` held and without)
    std::unordered_map<void*, const char*> last_kernel;   // hipStream_t -> Instance::name of its last stream-stage launch (mbx_last_kernel_name)
};
Context    g_ctx[kMaxDevices];
std::mutex g_init_mu;                        // serialises mbx_init() / mbx_shutdown()

thread_local char t_err[256] = "";           // mbx_last_error() is per thread, like errno

using mbx::aligned_to;
using mbx::pack_rows;
using mbx::validate_bits;

int fail(int code, const char* what) {
    mbx_set_error_text(what);
    return code;
}

// The alignment table of include/mbx.h, host side, before anything is launched (a null pointer is aligned: whether it may be null is
// each caller's check): the kernels store records as 16-byte vectors, the RNG state as a 64-bit word, load IMBE wire frames in 16-bit
// pieces and soft cells as 16-bit words, and a pointer below its alignment must never reach them.
static bool batch_pointers_aligned(const mbx_param_record* records, const mbe_parms* state, const mbx_stream_rng* rng, const int16_t* pcm16,
                                   const float* pcmf, const mbe_process_result* results, const int32_t* stream_index, const uint32_t* resident,
                                   const int32_t* frame_offset) {
    return aligned_to(records, 16) && aligned_to(state, 4) && aligned_to(rng, 8) && aligned_to(pcm16, 2) && aligned_to(pcmf, 4) &&
           aligned_to(results, 4) && aligned_to(stream_index, 4) && aligned_to(resident, 4) && aligned_to(frame_offset, 4);
}
// wire frames: 18-byte IMBE frames (and the 18-byte rows of a mixed batch) are read in 16-bit pieces, 9-byte AMBE frames byte by byte
static bool frames_aligned(const void* d_frames, bool imbe_rows) { return aligned_to(d_frames, imbe_rows ? 2 : 1); }
static int misaligned(const char* who) { return mbx::misaligned(who, "mbx.h"); }

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) {                        \
            return mbx::hip_failed("", #expr, e_);     \
        }                                              \
    } while (0)

// context of the calling thread's current device, or nullptr with *rc set
Context* current_ctx(int* rc) {
    int dev = -1;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        *rc = e != hipSuccess ? mbx::hip_failed("", "hipGetDevice", e) : fail(MBX_ENODEVICE, "hipGetDevice");
        return nullptr;
    }
    Context& c = g_ctx[dev];
    if (!c.ready.load(std::memory_order_acquire)) {
        *rc = fail(MBX_ENOTINIT, "mbx_init() has not been called for the current device");
        return nullptr;
    }
    return &c;
}

#define REQUIRE_CTX(c)                 \
    int rc_ctx_ = 0;                   \
    Context* c = current_ctx(&rc_ctx_); \
    if (!c) {                          \
        return rc_ctx_;                \
    }

void release_side_streams(StreamSlot& slot) {
    for (int g = 0; g < 4; ++g) {
        if (slot.side[g]) {
            (void)hipStreamSynchronize(slot.side[g]);
            (void)hipStreamDestroy(slot.side[g]);
            slot.side[g] = nullptr;
        }
        if (slot.join[g]) {
            (void)hipEventDestroy(slot.join[g]);
            slot.join[g] = nullptr;
        }
    }
    if (slot.fork) {
        (void)hipEventDestroy(slot.fork);
        slot.fork = nullptr;
    }
}

void free_context(Context& c) {   // caller holds g_init_mu and c.mu
    (void)hipFree(c.d_blob);
    (void)hipFree(c.d_derived);
    for (auto& kv : c.slots) {
        (void)hipFree(kv.second.workspace);
        release_side_streams(kv.second);
    }
    c.slots.clear();
    {
        std::lock_guard<std::mutex> lock(c.name_mu);
        c.last_kernel.clear();
    }
    c.d_blob = c.d_derived = nullptr;
    c.tabs = mbx::DeviceTables{};   // (every field zero: mbx_init sets what it needs)
    c.reserve_frames = 0;
    c.checksum = 0;
    c.device = -1;
}

const mbx::LaunchSwitches& launch_switches() {   // the MBX_* launch switches (mbx_launch_plan.h): read once per process
    static const mbx::LaunchSwitches s = mbx::read_launch_switches();   // thread-safe static initialisation
    return s;
}

// Walking order of successive stream-kernel launches (see launch_stream): alternating by default; MBX_NO_REVERSE=1 in the
// environment or mbx_set_stream_order(0) fixes it (every launch walks the streams forward).
std::atomic<int>& stream_order_flag() {
    static std::atomic<int> flag{getenv("MBX_NO_REVERSE") == nullptr ? 1 : 0};   // thread-safe static initialisation
    return flag;
}
bool reverse_enabled() { return stream_order_flag().load(std::memory_order_relaxed) != 0; }
// 1: AMBE tone frames are synthesised (the reference's default build); MBX_DISABLE_TONES=1 in the environment starts with 0
std::atomic<int>& tones_flag() {
    static std::atomic<int> flag{[] {
        const char* e = getenv("MBX_DISABLE_TONES");
        return (e && e[0] == '1') ? 0 : 1;
    }()};
    return flag;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", what, e);
}

}  // namespace

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) {
            (void)hipFree(p);
        }
    }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
    template <class U> U* as() { return static_cast<U*>(p); }
};
}  // namespace

void mbx_set_error_text(const char* text) { snprintf(t_err, sizeof(t_err), "%s", text); }   // (mbx_host.h: for every host unit)

extern "C" {

const char* mbx_last_error(void) { return t_err; }

int mbx_init(int device, const void* table_blob, size_t table_bytes) {
    if (const char* refused = mbx::check_blob(table_blob, table_bytes)) {
        return fail(MBX_EBADTABLE, refused);
    }
    const mbx_tables* host = static_cast<const mbx_tables*>(table_blob);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        return fail(MBX_ENODEVICE, "no HIP device");
    }
    if (device < 0 || device >= count || device >= kMaxDevices) {
        return fail(MBX_ENODEVICE, "device index out of range");
    }
    std::lock_guard<std::mutex> init_lock(g_init_mu);
    HIP_TRY(hipSetDevice(device));   // the calling thread's current device from here on, like hipSetDevice itself
    Context& ctx = g_ctx[device];
    if (ctx.ready.load(std::memory_order_acquire)) {
        if (ctx.checksum == host->checksum) {
            return 0;   // same tables already resident: nothing to do (any thread may call mbx_init again)
        }
        // different tables: the caller must have no launches in flight on this device
        HIP_TRY(hipDeviceSynchronize());
        std::lock_guard<std::mutex> lock(ctx.mu);
        ctx.ready.store(false, std::memory_order_release);
        const int keep = ctx.tabs.ablate;
        free_context(ctx);
        ctx.tabs.ablate = keep;
    }

    std::vector<mbx::DerivedTables> dv(1);   // (263 KB: not on the stack)
    mbx::DerivedTables& d = dv[0];
    if (const char* refused = mbx::derive_tables(*host, d)) {
        return fail(MBX_EBADTABLE, refused);
    }

    std::lock_guard<std::mutex> lock(ctx.mu);
    HIP_TRY(hipMalloc(&ctx.d_blob, sizeof(mbx_tables)));
    HIP_TRY(hipMalloc(&ctx.d_derived, sizeof(mbx::DerivedTables)));
    HIP_TRY(hipMemcpy(ctx.d_blob, table_blob, sizeof(mbx_tables), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx.d_derived, &d, sizeof(d), hipMemcpyHostToDevice));
    ctx.tabs.t = static_cast<const mbx_tables*>(ctx.d_blob);
    ctx.tabs.tones_off = tones_flag().load(std::memory_order_relaxed) ? 0 : 1;
    ctx.tabs.d = static_cast<const mbx::DerivedTables*>(ctx.d_derived);
    ctx.device = device;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    ctx.simds = 4 * cus;
    ctx.checksum = host->checksum;
    ctx.ready.store(true, std::memory_order_release);
    return 0;
}

void mbx_shutdown(void) {
    std::lock_guard<std::mutex> init_lock(g_init_mu);
    int before = -1;
    (void)hipGetDevice(&before);
    for (int dev = 0; dev < kMaxDevices; ++dev) {
        Context& ctx = g_ctx[dev];
        if (!ctx.ready.load(std::memory_order_acquire)) {
            continue;
        }
        (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        std::lock_guard<std::mutex> lock(ctx.mu);
        ctx.ready.store(false, std::memory_order_release);
        free_context(ctx);
    }
    if (before >= 0) {
        (void)hipSetDevice(before);
    }
}

int mbx_set_stream_order(int alternate) { return stream_order_flag().exchange(alternate ? 1 : 0, std::memory_order_relaxed); }

// Tone synthesis on / off, process-wide: the run-time form of the reference's one compile-time option that changes what this
// path computes (NOTONES = -DDISABLE_AMBE_TONES, ref CMakeLists.txt:41,330-337; src/core/mbelib.c:747-751,815-819).  The flag
// lives in every context's DeviceTables (a kernel argument): launches issued after the call see the new value.
int mbx_set_tone_synthesis(int enabled) {
    const int before = tones_flag().exchange(enabled ? 1 : 0, std::memory_order_relaxed);
    for (int dev = 0; dev < kMaxDevices; ++dev) {
        std::lock_guard<std::mutex> lock(g_ctx[dev].mu);
        g_ctx[dev].tabs.tones_off = enabled ? 0 : 1;
    }
    return before;
}

int mbx_device_ready(int device) {
    return device >= 0 && device < kMaxDevices && g_ctx[device].ready.load(std::memory_order_acquire) ? 1 : 0;
}

uint32_t mbx_table_checksum(void) {
    int rc = 0;
    Context* c = current_ctx(&rc);
    return c ? c->checksum : 0u;
}

// Where cell [row][col] of the reference's frame array sits in the packed wire frame: bit index from the frame's first bit (bit 7 of
// byte 0 = index 0), -1 for a cell the codec does not use.  The row widths are the packers' (pack_rows: row after row, inside a row
// from the highest cell down to cell 0), declared in mbx_codec.h.
int mbx_wire_bit_of_cell(int codec, int row, int col) {
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!sh || row < 0 || row >= sh->rows || col < 0 || col >= sh->width[row]) {
        return -1;
    }
    int pos = 0;
    for (int r = 0; r < row; ++r) {
        pos += sh->width[r];
    }
    return pos + (sh->width[row] - 1 - col);
}

// Folds a caller's deinterleave schedule into one table: the caller knows, for each of the n channel bits of a voice burst in the order
// it receives them, the cell (cell_row[i], cell_col[i]) its air-interface tables send that bit to; wire_bit[i] is where the same bit
// goes in the packed wire frame.  Refuses a schedule that is not a bijection onto the codec's cells (a wrong table is caught here,
// once, not as noise in the audio).
int mbx_wire_permutation(int codec, const int* cell_row, const int* cell_col, int n, int* wire_bit) {
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!sh || !cell_row || !cell_col || !wire_bit) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    int total = 0;
    for (int r = 0; r < sh->rows; ++r) {
        total += sh->width[r];
    }
    if (n != total) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_wire_permutation: the schedule must name every channel bit of the codec once");
    }
    bool seen[192] = {false};
    for (int i = 0; i < n; ++i) {
        const int b = mbx_wire_bit_of_cell(codec, cell_row[i], cell_col[i]);
        if (b < 0 || seen[b]) {
            return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_wire_permutation: a cell outside the codec's frame, or named twice");
        }
        seen[b] = true;
        wire_bit[i] = b;
    }
    return 0;
}

static int pack_frames(const mbx::CodecShape& sh, const char* frames, size_t n, uint8_t* packed) {
    int rc = validate_bits(frames, n * (size_t)sh.cells);
    if (rc < 0) {
        return rc;
    }
    if (!packed) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < n; ++i) {
        pack_rows(frames + i * (size_t)sh.cells, sh.rows, sh.stride, sh.width, packed + i * (size_t)sh.frame_bytes, sh.frame_bytes);
    }
    return 0;
}
int mbx_pack_imbe7200x4400(const char* frames, size_t n, uint8_t* packed) { return pack_frames(mbx::kCodecs[MBX_CODEC_IMBE7200X4400], frames, n, packed); }
int mbx_pack_imbe7100x4400(const char* frames, size_t n, uint8_t* packed) { return pack_frames(mbx::kCodecs[MBX_CODEC_IMBE7100X4400], frames, n, packed); }
int mbx_pack_ambe3600x2450(const char* frames, size_t n, uint8_t* packed) { return pack_frames(mbx::kCodecs[MBX_CODEC_AMBE3600X2450], frames, n, packed); }

void mbx_unpack_records(const mbx_param_record* rec, size_t n, int nbits, char* bits, mbe_process_result* results) {
    for (size_t i = 0; i < n; ++i) {
        if (bits) {
            for (int b = 0; b < nbits; ++b) {
                bits[i * (size_t)nbits + b] = (char)((rec[i].w[b >> 5] >> (31 - (b & 31))) & 1u);
            }
        }
        if (results) {
            mbe_process_result& r = results[i];
            r.c0_errors = (int)(rec[i].w[3] & 0xffu);
            r.protected_errors = (int)((rec[i].w[3] >> 8) & 0xffu);
            r.c4_errors = (int)((rec[i].w[3] >> 16) & 0xffu);
            r.total_errors = r.c0_errors + r.protected_errors;
            r.flags = (rec[i].w[3] >> 24) & 0xffu;
        }
    }
}

void mbx_rng_default(mbx_stream_rng* rng) {
    memset(rng, 0, sizeof(*rng));
    rng->unvoiced_seed_state = 3147u;
}

void mbx_rng_seed(mbx_stream_rng* rng, uint32_t seed) {   // ref: src/core/mbelib.c:173-181
    if (seed == 0u) {
        seed = 0x6d25357bu;
    }
    rng->cn_seed48 = (((uint64_t)seed) ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1ULL);
    rng->cn_seeded = 1;
    rng->unvoiced_seed_state = seed % 53125u;
    rng->unvoiced_seed_override = 1;
}

// ---- workspace of the stream stage ------------------------------------------------------------------------------
// caller holds c->mu
static int ensure_workspace(Context* c, StreamSlot& slot, size_t frames, void* stream) {
    if (frames <= slot.frames) {
        return 0;
    }
    const size_t want = frames > c->reserve_frames ? frames : c->reserve_frames;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
        return fail(MBE_STATUS_INVALID_ARGUMENT,
                    "the expand workspace of this stream would have to grow during stream capture: call mbx_reserve_stream() first");
    }
    (void)hipGetLastError();
    if (slot.workspace) {   // earlier launches on this stream may still read it
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        HIP_TRY(hipFree(slot.workspace));
        slot.workspace = nullptr;
        slot.flags = nullptr;
        slot.frames = 0;
        slot.exp_codec = -1;
    }
    const size_t flag_bytes = (((want + 7) / 8 + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;   // (+ 1: the fall-back counter)
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&slot.workspace), want * sizeof(mbx::FrameParams) + flag_bytes));
    slot.frames = want;
    slot.flags = reinterpret_cast<uint32_t*>(slot.workspace + want);
    slot.epoch = 0;
    // (no launch has epoch 0.)  On the LAUNCH stream: a non-blocking stream is not ordered against the null stream, so a null-stream
    // memset could land after the first launch's front blocks have published their flags.  (Not capturing: checked above.)
    HIP_TRY(hipMemsetAsync(slot.flags, 0, flag_bytes, (hipStream_t)stream));
    return 0;
}

int mbx_reserve_stream(void* stream, size_t max_frames) {
    REQUIRE_CTX(c);
    std::lock_guard<std::mutex> lock(c->mu);
    return ensure_workspace(c, c->slots[stream], max_frames, stream);
}

int mbx_reserve(size_t max_frames) {
    REQUIRE_CTX(c);
    std::lock_guard<std::mutex> lock(c->mu);
    if (max_frames > c->reserve_frames) {
        c->reserve_frames = max_frames;   // every slot grows to at least this much the next time it has to grow at all
    }
    // Only the default stream's slot is sized here.  The slots of other streams are NOT walked: the library cannot know
    // whether a hipStream_t it saw earlier still exists, and synchronising a destroyed handle is undefined -- a stream
    // that must not allocate at its next launch (stream capture) is sized with mbx_reserve_stream() by its owner.
    return ensure_workspace(c, c->slots[nullptr], max_frames, nullptr);
}

int mbx_release_stream(void* stream) {
    REQUIRE_CTX(c);
    std::lock_guard<std::mutex> lock(c->mu);
    {   // what mbx_last_kernel_name knows of the stream goes with it: a later stream may be given the same handle
        std::lock_guard<std::mutex> names(c->name_mu);
        c->last_kernel.erase(stream);
    }
    auto it = c->slots.find(stream);
    if (it == c->slots.end()) {
        return 0;
    }
    if (it->second.workspace) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        HIP_TRY(hipFree(it->second.workspace));
    }
    release_side_streams(it->second);
    c->slots.erase(it);
    return 0;
}

size_t mbx_workspace_bytes(size_t max_frames) { return max_frames * sizeof(mbx::FrameParams); }

int mbx_ecc_soft_words(int kind, const mbe_soft_bit* d_in, size_t n, uint32_t* d_out, int32_t* d_errs, void* stream) {
    REQUIRE_CTX(c);
    if (!d_in || !d_out || kind < 0 || kind > 2 || n > 0x7fffffffu) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_in, 2) || !aligned_to(d_out, 4) || !aligned_to(d_errs, 4)) {
        return misaligned("mbx_ecc_soft_words");
    }
    if (n == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::ecc_soft_words_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, kind, d_in, n, d_out,
                       d_errs, c->tabs);
    return check_launch("ecc_soft_words_kernel");
}

int mbx_validate_soft_bits(const mbe_soft_bit* soft, size_t count) {
    if (!soft) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < count; ++i) {
        if (soft[i].bit > 1u) {
            return MBE_STATUS_INVALID_BITS;
        }
    }
    return 0;
}

int mbx_soft_bits_from_hard(const char* bits, mbe_soft_bit* soft, size_t count, uint8_t reliability) {
    if (!soft || !bits) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < count; ++i) {
        if ((unsigned char)bits[i] > 1u) {
            return MBE_STATUS_INVALID_BITS;
        }
    }
    for (size_t i = 0; i < count; ++i) {
        soft[i].bit = (uint8_t)(bits[i] ? 1u : 0u);
        soft[i].reliability = reliability;
    }
    return 0;
}

int mbx_soft_bits_from_llr(const int16_t* llr, mbe_soft_bit* soft, size_t count) {
    if (!llr || !soft) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < count; ++i) {
        const uint32_t cell = mbx::soft_cell_from_llr(llr[i]);
        soft[i].bit = (uint8_t)(cell & 1u);
        soft[i].reliability = (uint8_t)(cell >> 8);
    }
    return 0;
}

// ---- the stream-stage kernel instances (mbx_stream.hip) ------------------------------------------------------------------------------
// ONE table of what can run and ONE function that says what does (plan_step, mbx_launch_plan.h, with the switches it reads): the
// launchers launch the entry its plan names and report entry.name, mbx_batch_kernel_name / mbx_stream_kernel_name return the same
// entry's name.  A new instance: its declaration in mbx_kernels.h, its row here (rows by their first entry: Row, mbx_launch_plan.h),
// its case in plan_step.
using mbx::DeviceTables;
using mbx::FrameParams;
enum Family { kStreamArgs, kSliceArgs, kFusedArgs, kOneLaunchArgs, kOneLaunchLeadArgs };   // (one-launch: without / with the front blocks' lead)
struct Instance {
    const char* name;   // as the profiler prints it
    Family      family;   // which argument list the kernel takes (mbx_kernels.h) = which member of the union is set
    union {
        void (*stream)(MBX_STREAM_PARAMS);
        void (*slice)(MBX_SLICE_PARAMS);
        void (*fused)(MBX_FUSED_PARAMS);
        void (*one_launch)(int S, MBX_ONE_LAUNCH_PARAMS);
        void (*one_launch_lead)(int S, int lead, MBX_ONE_LAUNCH_PARAMS);
    };
    // (the family follows from the kernel's type: a kernel whose parameter list is none of the families' does not compile here)
    constexpr Instance(const char* n, void (*k)(MBX_STREAM_PARAMS)) : name(n), family(kStreamArgs), stream(k) {}
    constexpr Instance(const char* n, void (*k)(MBX_SLICE_PARAMS)) : name(n), family(kSliceArgs), slice(k) {}
    constexpr Instance(const char* n, void (*k)(MBX_FUSED_PARAMS)) : name(n), family(kFusedArgs), fused(k) {}
    constexpr Instance(const char* n, void (*k)(int S, MBX_ONE_LAUNCH_PARAMS)) : name(n), family(kOneLaunchArgs), one_launch(k) {}
    constexpr Instance(const char* n, void (*k)(int S, int lead, MBX_ONE_LAUNCH_PARAMS)) : name(n), family(kOneLaunchLeadArgs), one_launch_lead(k) {}
};
static const Instance kInstances[] = {
    {"imbe_stream_kernel", mbx::imbe_stream_kernel},
    {"ambe_stream_kernel", mbx::ambe_stream_kernel},
    {"ambe2400_stream_kernel", mbx::ambe2400_stream_kernel},
    {"imbe_stream_kernel_one", mbx::imbe_stream_kernel_one},
    {"ambe_stream_kernel_one", mbx::ambe_stream_kernel_one},
    {"ambe2400_stream_kernel_one", mbx::ambe2400_stream_kernel_one},
    {"imbe_stream_kernel_lds", mbx::imbe_stream_kernel_lds},
    {"ambe_stream_kernel_lds", mbx::ambe_stream_kernel_lds},
    {"ambe2400_stream_kernel_lds", mbx::ambe2400_stream_kernel_lds},
    {"imbe_stream_kernel_res", mbx::imbe_stream_kernel_res},
    {"ambe_stream_kernel_res", mbx::ambe_stream_kernel_res},
    {"ambe2400_stream_kernel_res", mbx::ambe2400_stream_kernel_res},
    {"imbe_stream_kernel_res1", mbx::imbe_stream_kernel_res1},
    {"ambe_stream_kernel_res1", mbx::ambe_stream_kernel_res1},
    {"ambe2400_stream_kernel_res1", mbx::ambe2400_stream_kernel_res1},
    {"imbe_stream_kernel_lds_slice", mbx::imbe_stream_kernel_lds_slice},
    {"ambe_stream_kernel_lds_slice", mbx::ambe_stream_kernel_lds_slice},
    {"ambe2400_stream_kernel_lds_slice", mbx::ambe2400_stream_kernel_lds_slice},
    {"imbe_one_launch_kernel", mbx::imbe_one_launch_kernel},
    {"ambe_one_launch_kernel", mbx::ambe_one_launch_kernel},
    {"ambe2400_one_launch_kernel", mbx::ambe2400_one_launch_kernel},
    {"imbe_one_launch_kernel_res", mbx::imbe_one_launch_kernel_res},
    {"ambe_one_launch_kernel_res", mbx::ambe_one_launch_kernel_res},
    {"ambe2400_one_launch_kernel_res", mbx::ambe2400_one_launch_kernel_res},
    {"imbe_stream_kernel_one_fused", mbx::imbe_stream_kernel_one_fused},
    {"imbe7100_stream_kernel_one_fused", mbx::imbe7100_stream_kernel_one_fused},
    {"imbe_stream_kernel_res1_fused", mbx::imbe_stream_kernel_res1_fused},
    {"imbe7100_stream_kernel_res1_fused", mbx::imbe7100_stream_kernel_res1_fused},
};
static_assert(sizeof(kInstances) / sizeof(kInstances[0]) == mbx::kInstanceCount, "kInstances: Row names the first entry of every row");
// The ragged stream-stage kernels (mbx_process_batch_ragged: a frame count per stream).  A table of their own: a ragged call has no
// shape to select by -- one kernel per codec column (as in kInstances) and state form, whatever the counts are: a ragged plan's
// instance is state form * 3 + column.
struct RaggedKernel {
    const char* name;
    void (*kernel)(MBX_RAGGED_PARAMS);
};
static const RaggedKernel kRagged[2][3] = {
    // ABI triplets
    {{"imbe_stream_kernel_ragged", mbx::imbe_stream_kernel_ragged},
     {"ambe_stream_kernel_ragged", mbx::ambe_stream_kernel_ragged},
     {"ambe2400_stream_kernel_ragged", mbx::ambe2400_stream_kernel_ragged}},
    // resident state
    {{"imbe_stream_kernel_ragged_res", mbx::imbe_stream_kernel_ragged_res},
     {"ambe_stream_kernel_ragged_res", mbx::ambe_stream_kernel_ragged_res},
     {"ambe2400_stream_kernel_ragged_res", mbx::ambe2400_stream_kernel_ragged_res}},
};
// The mixed-codec stream-stage kernels (mbx_process_batch_mixed: a codec and a frame count per stream), a row of their own beside
// kRagged: [0] ABI triplets, [1] resident state.  One workgroup holds the LDS and the registers of the largest body, an AMBE one.
struct MixedKernel {
    const char* name;
    void (*kernel)(MBX_MIXED_PARAMS);
};
static const MixedKernel kMixed[2] = {
    {"mixed_stream_kernel_ragged", mbx::mixed_stream_kernel_ragged},
    {"mixed_stream_kernel_ragged_res", mbx::mixed_stream_kernel_ragged_res},
};
// The kernels of a codec's own stages, keyed as its shape is (mbx_codec.h), every kernel named once.  A codec's frames go through the
// FEC kernels of the row CodecShape::front names and the expand kernel of the row CodecShape::stream names: a row that is nobody's
// front end has no FEC kernels, one that is nobody's stream stage no expand kernel.  (Its columns in kInstances: kCodecLaunch,
// mbx_launch_plan.h.)  A new codec: its shape in mbx_codec.h, its row here and in kCodecLaunch.
using FecKernel = void (*)(const uint8_t*, size_t, mbx_param_record*, DeviceTables);
using SoftFecKernel = void (*)(const mbe_soft_bit*, size_t, mbx_param_record*, DeviceTables);
using ExpandKernel = void (*)(const mbx_param_record*, size_t, FrameParams*, DeviceTables);
struct CodecKernels {
    FecKernel     fec;            // hard FEC: packed frames -> records, one frame per thread
    const char*   fec_name;
    SoftFecKernel fec_soft;       // soft FEC alone (mbx_fec_soft) ...
    SoftFecKernel soft_front;     // ... and as the front of a soft batch step (mbx_soft_front.hip); both one wavefront per frame
    ExpandKernel  expand;         // records -> FrameParams rows
};
static const CodecKernels kCodecKernels[4] = {
    {mbx::fec_imbe7200x4400_kernel, "fec_imbe7200x4400_kernel", mbx::fec_imbe7200x4400_soft_kernel, mbx::soft_front_imbe_kernel,
     mbx::expand_imbe_kernel},
    {mbx::fec_ambe3600x2450_kernel, "fec_ambe3600x2450_kernel", mbx::fec_ambe3600x2450_soft_kernel, mbx::soft_front_ambe_kernel,
     mbx::expand_ambe_kernel},
    {mbx::fec_imbe7100x4400_kernel, "fec_imbe7100x4400_kernel", mbx::fec_imbe7100x4400_soft_kernel, mbx::soft_front_imbe7100_kernel,
     nullptr},
    {nullptr, nullptr, nullptr, nullptr, mbx::expand_ambe2400_kernel},
};
using mbx::imbe_codec;

// FEC stage of hard-decision frames of `codec` (one of the four): n frames -> records
static int launch_fec(Context* c, int codec, const uint8_t* d_frames, size_t n, mbx_param_record* d_records, void* stream) {
    const CodecKernels& k = kCodecKernels[mbx::kCodecs[codec].front];
    hipLaunchKernelGGL(k.fec, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_frames, n, d_records, c->tabs);
    return check_launch(k.fec_name);
}
static int fec_export(int codec, const uint8_t* d_frames, size_t n, mbx_param_record* d_records, void* stream) {
    REQUIRE_CTX(c);
    if (!d_frames || !d_records) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_records, 16) || !frames_aligned(d_frames, imbe_codec(codec))) {
        return misaligned("mbx_fec");
    }
    return n == 0 ? 0 : launch_fec(c, codec, d_frames, n, d_records, stream);
}
int mbx_fec_imbe7200x4400(const uint8_t* d_frames, size_t n, mbx_param_record* d_records, void* stream) { return fec_export(MBX_CODEC_IMBE7200X4400, d_frames, n, d_records, stream); }
int mbx_fec_ambe3600x2450(const uint8_t* d_frames, size_t n, mbx_param_record* d_records, void* stream) { return fec_export(MBX_CODEC_AMBE3600X2450, d_frames, n, d_records, stream); }
int mbx_fec_imbe7100x4400(const uint8_t* d_frames, size_t n, mbx_param_record* d_records, void* stream) { return fec_export(MBX_CODEC_IMBE7100X4400, d_frames, n, d_records, stream); }

// soft frames of `codec` (one of the four), n <= 2^31-1 of them, -> records, one wavefront per frame: the front of a soft batch step
// (mbx_soft_front.hip), or the FEC-only kernel behind mbx_fec_soft
static int launch_soft_fec(Context* c, int codec, bool front, const mbe_soft_bit* d_soft, size_t n, mbx_param_record* d_records, void* stream) {
    const CodecKernels& k = kCodecKernels[mbx::kCodecs[codec].front];
    const SoftFecKernel kernel = front ? k.soft_front : k.fec_soft;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, d_soft, n, d_records, c->tabs);
    return check_launch(front ? "soft_front_kernel" : "fec_soft_kernel");
}

int mbx_fec_soft(int codec, const mbe_soft_bit* d_soft, size_t n, mbx_param_record* d_records, void* stream) {
    REQUIRE_CTX(c);
    if (!d_soft || !d_records || !mbx::codec_shape(codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_soft, 2) || !aligned_to(d_records, 16)) {
        return misaligned("mbx_fec_soft");
    }
    if (n == 0) {
        return 0;
    }
    if (n > 0x7fffffffu) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_fec_soft: more than 2^31-1 frames in one launch");
    }
    return launch_soft_fec(c, codec, false, d_soft, n, d_records, stream);
}

// frame-parallel half of the parameter decode: records of a codec with a stream stage of its own -> FrameParams rows at `out`
static int launch_expand(Context* c, int codec, const mbx_param_record* d_records, size_t n, mbx::FrameParams* out, void* stream) {
    const unsigned egrid = (unsigned)((n + 31) / 32);   // 8 frames per wave, 4 waves per workgroup (mbx_expand.hip)
    hipLaunchKernelGGL(kCodecKernels[codec].expand, dim3(egrid), dim3(256), 0, (hipStream_t)stream, d_records, n, out, c->tabs);
    return check_launch("expand_kernel");
}
// every stream-stage launch ends here: what ran on `stream` (the caller's, also for the slices of a sliced launch) is written down
// for mbx_last_kernel_name -- the table's own pointer, one store per launch, nothing on the device -- and the launch is checked
static void record_launch(Context* c, void* stream, const char* name) {
    std::lock_guard<std::mutex> lock(c->name_mu);
    c->last_kernel[stream] = name;
}
static void record_launch(Context* c, void* stream, const Instance& e) { record_launch(c, stream, e.name); }
static int launched(Context* c, void* stream, const Instance& e) {
    record_launch(c, stream, e);
    return check_launch(e.name);
}
// What every launcher of a batch step passes on.  `codec` is the call's own: a launcher asks the codec tables for the codec of the
// stage it launches (a 7100x4400 step has a front end of its own and streams as 7200x4400).
struct BatchCall {
    int                 codec, S, T;
    mbx_param_record*   records;        // S*T, stream-major: written by the front launch of a step that has one, only read otherwise
    mbe_parms*          state;          // three structs per stream, or per slot of the pool `stream_index` names
    mbx_stream_rng*     rng;
    int16_t*            pcm16;          // S*T*160 samples each, or nullptr
    float*              pcmf;
    mbe_process_result* results;        // S*T, or nullptr
    void*               stream;
    const int32_t*      stream_index;   // row of the batch -> slot of state / rng, or nullptr: identity
    uint32_t*           resident;       // elision words of resident state, or nullptr: plain triplets
    // a RAGGED step (mbx_process_batch_ragged): stream row i owns batch rows frame_offset[i] .. frame_offset[i + 1] - 1; T is unused
    const int32_t*      frame_offset = nullptr;   // S + 1 offsets on the device, or nullptr: S x T, stream-major
    size_t              total = 0;                // the host's copy of frame_offset[S]: rows of every batch array
    // a MIXED ragged step (mbx_process_batch_mixed): stream row i is of codec stream_codec[i]; `codec` is unused
    const uint8_t*      stream_codec = nullptr;   // S bytes on the device, or nullptr: every stream is of `codec`
    // a KEYED step (include/mbx_keystream.h): the front launch XORs row r of the keystream onto the record of batch row r
    const uint8_t*      keystream = nullptr;      // MBX_KEYSTREAM_ROW_BYTES per batch row on the device, or nullptr: the unkeyed step
};
static bool call_args_ok(const BatchCall& b) { return b.records && b.state && b.rng && b.S >= 0 && b.T >= 0; }
static bool call_aligned(const BatchCall& b) {
    return batch_pointers_aligned(b.records, b.state, b.rng, b.pcm16, b.pcmf, b.results, b.stream_index, b.resident, b.frame_offset) &&
           aligned_to(b.keystream, 4);   // (kind `keystream`, include/mbx_keystream.h: the kernels load a row as three dwords)
}
static size_t batch_rows(const BatchCall& b) { return b.frame_offset ? b.total : (size_t)b.S * (size_t)b.T; }
// the tables of a launch: the context's + what this launch walks (`reverse`: see launch_stream)
static mbx::DeviceTables launch_tables(const Context* c, bool reverse, const BatchCall& b) {
    mbx::DeviceTables tabs = c->tabs;
    tabs.reverse = (reverse && reverse_enabled()) ? 1 : 0;
    tabs.stream_map = b.stream_index;
    tabs.resident = b.resident;
    return tabs;
}

// ---- planning (mbx_launch_plan.h) ---------------------------------------------------------------------------------------------------
// Every launcher below: its own argument and alignment checks, a StepShape, ONE plan, the workspace grown to the plan's size, the plan
// issued.  Nothing below this section asks the environment, a codec's facts or a frame count what to launch.
using mbx::InputKind;
using mbx::kFrames;
using mbx::kRecords;
using mbx::kSoft;
using mbx::StepPlan;
using mbx::StepShape;
// (`c` may be nullptr: a prediction without a device context knows no wave slots)
static StepPlan plan_of(const Context* c, const StepShape& q) {
    return mbx::plan_step(q, launch_switches(), {c ? c->simds : 0, MBX_IMBE_LDS_WAVES_PER_SIMD, MBX_AMBE_LDS_WAVES_PER_SIMD, sizeof(mbx::FrameParams)});
}
// what a batch call knows of its step; `own_workspace`: the rows go through the stream slot's own workspace (then the launch may be sliced)
static StepShape step_shape(const BatchCall& b, InputKind kind, const void* d_input, bool own_workspace) {
    StepShape q;
    q.codec = b.codec, q.S = b.S, q.T = b.T, q.total = b.total;
    q.kind = kind;
    q.resident = b.resident != nullptr;
    q.ragged = b.frame_offset != nullptr;
    q.mixed = b.stream_codec != nullptr;
    q.aligned = (reinterpret_cast<uintptr_t>(d_input) & 3u) == 0;
    q.own_workspace = q.slices_allowed = own_workspace;
    q.keyed = b.keystream != nullptr;
    return q;
}
// THE plan of a step on `stream`.  A plan that needs the slot's flag words (a captured launch would be replayed with the same epoch,
// and a replay would find the flags of the replay before it) or side streams holds outside stream capture only: then, and only then,
// the stream is asked, and a step that is being captured is planned again as such (it takes the staged kernels, unsliced).
static StepPlan plan_on_stream(const Context* c, StepShape& q, void* stream) {
    StepPlan plan = plan_of(c, q);
    if (plan.outside_capture_only) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        q.capturing = stream && hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
        (void)hipGetLastError();
        if (q.capturing) {
            plan = plan_of(c, q);
        }
    }
    return plan;
}

// A sliced launch (why, and what was measured: mbx_launch_plan.h): the streams in plan.slice_groups groups, the frames in slices of
// plan.slice_frames, the slices of each group issued in order on an internal HIP stream of its own, forked from and joined to the
// caller's stream with events.  Caller holds c->mu.  0: issued (*rc); 1: its streams, events or waits could not be had and nothing
// has been launched (take the plain launch)
static int issue_slices(Context* c, StreamSlot& slot, const mbx::DeviceTables& tabs, const BatchCall& b, const mbx::FrameParams* params,
                        const StepPlan& plan, int* rc) {
    const int S = b.S, T = b.T, Tc = plan.slice_frames, groups = plan.slice_groups;
    void* const stream = b.stream;
    if (!slot.fork) {   // first sliced launch on this stream: the internal streams of the groups (at most four, MBX_SLICE_GROUPS) and their events
        bool ok = hipEventCreateWithFlags(&slot.fork, hipEventDisableTiming) == hipSuccess;
        for (int g = 0; g < groups && ok; ++g) {
            ok = hipStreamCreateWithFlags(&slot.side[g], hipStreamNonBlocking) == hipSuccess
                 && hipEventCreateWithFlags(&slot.join[g], hipEventDisableTiming) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            release_side_streams(slot);
            return 1;
        }
    }
    if (hipEventRecord(slot.fork, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    const Instance& e = kInstances[plan.instance];
    int result = 0;
    record_launch(c, stream, e);   // one record for the whole sliced launch, under the caller's stream
    // Group 0 runs on the caller's stream itself (plan.slice_own) -- its kernels are queued before the stream waits for the other groups.
    // Every fork-side wait is queued BEFORE any group's kernels: should one fail, nothing has been launched yet and the state is
    // untouched (the caller then gets the plain launch).  A wait queued on an internal stream and never followed by work is harmless.
    for (int g = (plan.slice_own ? 1 : 0); g < groups; ++g) {
        if (hipStreamWaitEvent(slot.side[g], slot.fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            return 1;
        }
    }
    for (int g = 0; g < groups; ++g) {
        const int s0 = (int)((long long)S * g / groups), Sg = (int)((long long)S * (g + 1) / groups) - s0;
        const bool on_caller = plan.slice_own && g == 0;
        hipStream_t st = on_caller ? (hipStream_t)stream : slot.side[g];
        mbx::DeviceTables tg = tabs;
        if (tg.stream_map) {
            tg.stream_map += s0;
        }
        const size_t f0 = (size_t)s0 * (size_t)T;
        BatchCall part = b;   // this group's rows of the batch
        part.records += f0;
        const mbx::FrameParams* pg = params ? params + f0 : nullptr;
        if (!tabs.stream_map) {   // (state and RNG state are addressed through the stream map when there is one: then only the batch rows are offset)
            part.state += 3 * (size_t)s0;
            part.rng += s0;
        }
        part.pcm16 = b.pcm16 ? b.pcm16 + f0 * 160 : nullptr;
        part.pcmf = b.pcmf ? b.pcmf + f0 * 160 : nullptr;
        part.results = b.results ? b.results + f0 : nullptr;
        for (int t0 = 0; t0 < T; t0 += Tc) {
            const int n = (T - t0) < Tc ? (T - t0) : Tc;
            hipLaunchKernelGGL(e.slice, dim3((unsigned)Sg), dim3(64), 0, st, Sg, T, t0, n, part.records, pg, part.state, part.rng, part.pcm16, part.pcmf, part.results,
                               tg);
        }
        const int lrc = check_launch(e.name);
        if (lrc < 0) {
            result = lrc;
        }
        if (!on_caller && (hipEventRecord(slot.join[g], st) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, slot.join[g], 0) != hipSuccess)) {
            (void)hipGetLastError();
            result = fail(MBX_ENODEVICE, "sliced launch: join");
        }
    }
    *rc = result;
    return 0;
}

// Stream-stage launch of an S x T step.  `params` = FrameParams rows written by the expand stage, or nullptr: the IMBE stream kernel
// then expands each record itself (one launch less, no workspace traffic).
//
// `reverse`: successive launches over the same streams walk them in opposite directions.  A decoder is called for the
// same streams every 20 ms; the state of 65,536 of them (512 MB) does not fit the 256 MB Infinity Cache, so in a fixed
// order every launch finds none of it there, while a launch that starts where the previous one ended finds its last
// quarter-gigabyte.  The results do not depend on the order.  The alternation is kept per (device, hipStream_t) slot
// and per session -- whoever re-walks the same state -- not process-wide.
// `slot` (the caller holds c->mu): what a sliced plan is issued on; nullptr where the shape allows no slices.
static int launch_stream(Context* c, bool reverse, const BatchCall& b, const mbx::FrameParams* params, StreamSlot* slot, const StepShape& q, StepPlan plan) {
    const mbx::DeviceTables tabs = launch_tables(c, reverse, b);
    if (plan.slice_frames > 0) {
        int rc = 0;
        if (issue_slices(c, *slot, tabs, b, params, plan, &rc) == 0) {
            return rc;
        }
        StepShape plain = q;   // the same step without leave to slice
        plain.slices_allowed = false;
        plan = plan_of(c, plain);
    }
    const Instance& e = kInstances[plan.instance];
    hipLaunchKernelGGL(e.stream, dim3((unsigned)b.S), dim3(64), 0, (hipStream_t)b.stream, b.S, b.T, b.records, params, b.state, b.rng, b.pcm16,
                       b.pcmf, b.results, tabs);
    return launched(c, b.stream, e);
}

// The stream stage of a ragged or mixed step: ONE launch of S one-wave workgroups whose frame loops run frame_offset[s + 1] -
// frame_offset[s] times, on the rows of the expand launch at `ws`, behind the order kernel where the plan has one (its S words:
// behind the rows, at plan.order_offset).
static int launch_ragged(Context* c, const BatchCall& b, mbx::FrameParams* ws, const StepPlan& plan) {
    const int32_t* order = nullptr;
    if (plan.order) {
        int32_t* const order_ws = reinterpret_cast<int32_t*>(ws + plan.order_offset);
        // (one workgroup of the 1,024 threads the kernel strides by: mbx_stream.hip, kOrderThreads)
        hipLaunchKernelGGL(mbx::ragged_order_kernel, dim3(1), dim3(1024), 0, (hipStream_t)b.stream, b.S, b.frame_offset, order_ws);
        const int rc = check_launch("ragged_order_kernel");
        if (rc < 0) {
            return rc;
        }
        order = order_ws;
    }
    if (plan.form == mbx::kMixedStep) {   // the same launch with a codec per stream
        const MixedKernel& e = kMixed[plan.instance];
        hipLaunchKernelGGL(e.kernel, dim3((unsigned)b.S), dim3(64), 0, (hipStream_t)b.stream, b.stream_codec, b.S, (int)b.total, b.frame_offset, order,
                           b.records, ws, b.state, b.rng, b.pcm16, b.pcmf, b.results, launch_tables(c, false, b));
        record_launch(c, b.stream, e.name);
        return check_launch(e.name);
    }
    const RaggedKernel& e = kRagged[plan.instance / 3][plan.instance % 3];
    hipLaunchKernelGGL(e.kernel, dim3((unsigned)b.S), dim3(64), 0, (hipStream_t)b.stream, b.S, (int)b.total, b.frame_offset, order, b.records, ws,
                       b.state, b.rng, b.pcm16, b.pcmf, b.results, launch_tables(c, false, b));
    record_launch(c, b.stream, e.name);
    return check_launch(e.name);
}

// The whole T = 1 step as ONE launch (which shapes take which form: plan_step): the front end in the stream's own wave ...
static int launch_fused_one(Context* c, bool reverse, const BatchCall& b, const uint8_t* d_frames, const StepPlan& plan) {
    const Instance& e = kInstances[plan.instance];
    const mbx::DeviceTables tabs = launch_tables(c, reverse, b);
    hipLaunchKernelGGL(e.fused, dim3((unsigned)b.S), dim3(64), 0, (hipStream_t)b.stream, b.S, b.codec, d_frames, b.records, b.state, b.rng, b.pcm16,
                       b.pcmf, b.results, tabs);
    return launched(c, b.stream, e);
}
// ... or front blocks and stream blocks in one grid, rows handed over through the slot's workspace and flag words.  Caller holds
// c->mu; the slot's workspace holds S rows and its flags
static int launch_one_launch(Context* c, StreamSlot& slot, bool reverse, const BatchCall& b, const uint8_t* d_frames, const StepPlan& plan) {
    const Instance& e = kInstances[plan.instance];
    const mbx::DeviceTables tabs = launch_tables(c, reverse, b);
    if (++slot.epoch == 0u) {
        slot.epoch = 1u;
    }
    const unsigned chunks = (unsigned)((b.S + 7) / 8);
    uint32_t* const fallbacks = slot.flags + (slot.frames + 7) / 8;
    if (e.family == kOneLaunchLeadArgs) {
        hipLaunchKernelGGL(e.one_launch_lead, dim3(9u * chunks), dim3(64), 0, (hipStream_t)b.stream, b.S, plan.front_lead, d_frames, b.records,
                           slot.workspace, slot.flags, fallbacks, slot.epoch, b.state, b.rng, b.pcm16, b.pcmf, b.results, tabs);
    } else {
        hipLaunchKernelGGL(e.one_launch, dim3(9u * chunks), dim3(64), 0, (hipStream_t)b.stream, b.S, d_frames, b.records, slot.workspace, slot.flags,
                           fallbacks, slot.epoch, b.state, b.rng, b.pcm16, b.pcmf, b.results, tabs);
    }
    return launched(c, b.stream, e);
}

// (records-based: what mbx_process_records launches for the shape, on the stream slot's own workspace, not being captured)
static StepShape predicted_step(int codec, int S, int T) {
    StepShape q;
    q.codec = codec, q.S = S, q.T = T;
    q.own_workspace = q.slices_allowed = true;
    return q;
}
extern "C" int mbx_uses_expand_launch(int codec, int S, int T) { return plan_of(nullptr, predicted_step(codec, S, T)).expand ? 1 : 0; }

int mbx_expand_records(int codec, const mbx_param_record* d_records, size_t n, void* stream) {
    REQUIRE_CTX(c);
    if (!d_records || !mbx::codec_streams(codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_records, 16)) {
        return misaligned("mbx_expand_records");
    }
    if (n == 0) {
        return 0;
    }
    std::lock_guard<std::mutex> lock(c->mu);
    StreamSlot& slot = c->slots[stream];
    int rc = ensure_workspace(c, slot, n, stream);
    if (rc < 0) {
        return rc;
    }
    rc = launch_expand(c, codec, d_records, n, slot.workspace, stream);
    slot.exp_codec = rc < 0 ? -1 : codec;
    slot.exp_n = n;
    slot.exp_records = d_records;
    return rc;
}

// The two halves with a CALLER-OWNED workspace, so that they can run on DIFFERENT streams: the frame-parallel front end
// (FEC + expansion) of batch k + 1 does not depend on the stream stage of batch k, only on the frames -- a host that decodes
// batch after batch (recorded traffic, many sites) MAY let them overlap and order them with events of its own.  Measured on
// MI355X at T = 1 (bench.py --overlap-front-end): slower than everything on one stream (255 against 265 M frames/s) -- the
// HBM-bound stream kernel slows down by what it shares, and two cross-stream hand-overs per step cost what the overlap saves.
int mbx_expand_records_ws(int codec, const mbx_param_record* d_records, size_t n, void* d_workspace, size_t workspace_bytes,
                          void* stream) {
    REQUIRE_CTX(c);
    if (!d_records || !mbx::codec_streams(codec) || !d_workspace || workspace_bytes < mbx_workspace_bytes(n)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_records, 16) || !aligned_to(d_workspace, 16)) {
        return misaligned("mbx_expand_records_ws");
    }
    if (n == 0) {
        return 0;
    }
    return launch_expand(c, codec, d_records, n, static_cast<mbx::FrameParams*>(d_workspace), stream);
}

// the stream stage alone, on rows that are there: never sliced, nothing of the slot but its launch counter
static StepShape rows_shape(const BatchCall& b) {
    StepShape q;
    q.codec = b.codec, q.S = b.S, q.T = b.T;
    q.rows_given = true;
    q.resident = b.resident != nullptr;
    return q;
}
// (the records of these calls are read, never written: a BatchCall holds the pointer a front launch would write through)
int mbx_stream_expanded_ws(int codec, int S, int T, const mbx_param_record* d_records, mbe_parms* d_state, uint32_t* d_resident,
                           mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                           const void* d_workspace, size_t workspace_bytes, void* stream) {
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, const_cast<mbx_param_record*>(d_records), d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, d_resident};
    if (!call_args_ok(b) || !mbx::codec_streams(codec) || !d_workspace || workspace_bytes < mbx_workspace_bytes((size_t)S * (size_t)T)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!call_aligned(b) || !aligned_to(d_workspace, 16)) {
        return misaligned("mbx_stream_expanded_ws");
    }
    if (S == 0 || T == 0) {
        return 0;
    }
    const StepShape q = rows_shape(b);
    const StepPlan plan = plan_of(c, q);
    unsigned order;
    {
        std::lock_guard<std::mutex> lock(c->mu);
        order = c->slots[stream].launches++;
    }
    return launch_stream(c, (order & 1u) != 0u, b, static_cast<const mbx::FrameParams*>(d_workspace), nullptr, q, plan);
}

// the stream stage on the rows the last mbx_expand_records() left in the stream's own workspace
static int stream_expanded(const BatchCall& b) {
    REQUIRE_CTX(c);
    if (!call_args_ok(b) || !mbx::codec_streams(b.codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!call_aligned(b)) {
        return misaligned("mbx_stream_expanded");
    }
    if (b.S == 0 || b.T == 0) {
        return 0;
    }
    const StepShape q = rows_shape(b);
    const StepPlan plan = plan_of(c, q);
    std::lock_guard<std::mutex> lock(c->mu);
    StreamSlot& slot = c->slots[b.stream];
    if (slot.exp_codec != b.codec || slot.exp_n != (size_t)b.S * (size_t)b.T || slot.exp_records != b.records) {
        return fail(MBE_STATUS_INVALID_ARGUMENT,
                    "mbx_stream_expanded: the last mbx_expand_records() on this stream was not for this codec / batch / record array");
    }
    return launch_stream(c, (slot.launches++ & 1u) != 0u, b, slot.workspace, nullptr, q, plan);
}

int mbx_stream_expanded(int codec, int S, int T, const mbx_param_record* d_records, mbe_parms* d_state,
                        mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                        void* stream) {
    return stream_expanded({codec, S, T, const_cast<mbx_param_record*>(d_records), d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr});
}

// the same on resident state (mbx_process_batch_resident): bench.py brackets the stream kernel alone with it
int mbx_stream_expanded_resident(int codec, int S, int T, const mbx_param_record* d_records, mbe_parms* d_state, uint32_t* d_resident,
                                 mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                                 void* stream) {
    if (!d_resident) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return stream_expanded({codec, S, T, const_cast<mbx_param_record*>(d_records), d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, d_resident});
}

// ---- the batch step ------------------------------------------------------------------------------------------------------------
// Every batch entry point ends here: it makes the checks that are its own, fills the record and says what the step starts from
// (InputKind, mbx_launch_plan.h) and whose workspace the FrameParams rows go to.
//   caller_ws == nullptr: the stream slot's own workspace, grown here under c->mu, which is then held to the last launch -- the
//   workspace cannot be grown (freed) by another thread between the launches of this call, and two threads that share one
//   hipStream_t cannot interleave their steps.  The front launch is issued inside the lock as well.
//   caller_ws: the caller's rows.  Nothing of the slot is touched but its launch counter, c->mu is held only to read and bump it
//   (and across the in-wave fused launch of a T = 1 IMBE step, which needs no rows), the launch is never sliced and never one
//   that needs the slot's flag words: the step can be captured into a graph.
// The launch counter is bumped once per step, whatever its form.
struct CallerWorkspace {
    void*  p;
    size_t bytes;
};
// The front launch of a KEYED step (BatchCall::keystream; mbx_keystream.hip): the hard or the soft front of the unkeyed step of the same
// form -- frames a codec's own size apart and a uniform codec, or the rows and row codecs of a mixed step -- with the keystream row of
// every frame XORed onto its record before the record's one store.  Everything behind it is the unkeyed step's.
static int launch_keyed_front(Context* c, bool soft, const BatchCall& b, const uint8_t* row_codec, const void* d_input, size_t n) {
    const mbx::CodecShape* sh = row_codec ? nullptr : &mbx::kCodecs[b.codec];
    const hipStream_t st = (hipStream_t)b.stream;
    if (soft) {
        hipLaunchKernelGGL(mbx::soft_front_keyed_kernel, dim3((unsigned)n), dim3(64), 0, st, static_cast<const mbe_soft_bit*>(d_input), n,
                           sh ? sh->cells : MBX_MIXED_ROW_CELLS, b.codec, row_codec, b.keystream, b.records, c->tabs);
        return check_launch("soft_front_keyed_kernel");
    }
    hipLaunchKernelGGL(mbx::fec_keyed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const uint8_t*>(d_input), n,
                       sh ? sh->frame_bytes : MBX_MIXED_ROW_BYTES, b.codec, row_codec, b.keystream, b.records, c->tabs);
    return check_launch("fec_keyed_kernel");
}
// The staged launches of a MIXED step (BatchCall::stream_codec): the codec of every batch row into the step's own workspace (behind
// the rows and the order words, at plan.codec_offset), then what a ragged step launches, by kernels that look the codec of a row or a
// stream up -- one front launch and one expand launch over all rows, (the order,) one stream-stage launch, whatever the mix.
static int run_mixed_stages(Context* c, const BatchCall& b, const StepPlan& plan, const void* d_input, mbx::FrameParams* ws) {
    const size_t n = b.total;
    const hipStream_t st = (hipStream_t)b.stream;
    uint8_t* const row_codec = reinterpret_cast<uint8_t*>(ws + plan.codec_offset);
    hipLaunchKernelGGL(mbx::mixed_row_codec_kernel, dim3((unsigned)((b.S + 3) / 4)), dim3(256), 0, st, b.S, (int)n, b.frame_offset, b.stream_codec, row_codec);
    int rc = check_launch("mixed_row_codec_kernel");
    if (rc >= 0 && b.keystream) {   // a keyed step: the keyed front over the same rows and row codecs
        rc = launch_keyed_front(c, plan.front == mbx::kSoftFront, b, row_codec, d_input, n);
    } else if (rc >= 0 && plan.front == mbx::kFecFront) {
        hipLaunchKernelGGL(mbx::fec_mixed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const uint8_t*>(d_input), n, row_codec,
                           b.records, c->tabs);
        rc = check_launch("fec_mixed_kernel");
    } else if (rc >= 0) {
        hipLaunchKernelGGL(mbx::soft_front_mixed_kernel, dim3((unsigned)n), dim3(64), 0, st, static_cast<const mbe_soft_bit*>(d_input), n, row_codec,
                           b.records, c->tabs);
        rc = check_launch("soft_front_mixed_kernel");
    }
    if (rc >= 0) {
        hipLaunchKernelGGL(mbx::expand_mixed_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, b.records, n, row_codec, ws, c->tabs);
        rc = check_launch("expand_mixed_kernel");
    }
    return rc < 0 ? rc : launch_ragged(c, b, ws, plan);
}
// the staged launches of a step: the front launch (where the plan has one), expand (where the stream stage reads rows: to `ws`) and the
// stream kernel; `order` = the launch counter that decides the walking direction; `slot`: see launch_stream
static int run_stages(Context* c, unsigned order, const BatchCall& b, const StepShape& q, const StepPlan& plan, const void* d_input, mbx::FrameParams* ws,
                      StreamSlot* slot) {
    const size_t n = batch_rows(b);
    int rc = 0;
    if (b.keystream && plan.front != mbx::kNoFront) {
        rc = launch_keyed_front(c, plan.front == mbx::kSoftFront, b, nullptr, d_input, n);
    } else if (plan.front == mbx::kFecFront) {
        rc = launch_fec(c, b.codec, static_cast<const uint8_t*>(d_input), n, b.records, b.stream);
    } else if (plan.front == mbx::kSoftFront) {
        rc = launch_soft_fec(c, b.codec, true, static_cast<const mbe_soft_bit*>(d_input), n, b.records, b.stream);
    }
    if (rc >= 0 && plan.expand) {
        rc = launch_expand(c, mbx::kCodecs[b.codec].stream, b.records, n, ws, b.stream);
    }
    if (rc < 0) {
        return rc;
    }
    if (plan.form == mbx::kRaggedStep) {
        return launch_ragged(c, b, ws, plan);
    }
    return launch_stream(c, (order & 1u) != 0u, b, plan.rows ? ws : nullptr, slot, q, plan);
}
// A planned step on the stream slot's own workspace (run_batch without a caller's; a burst launch, behind its gather): the workspace
// grown to the plan's size, the launch counter bumped, the plan's form issued.  Caller holds c->mu and has made run_batch's checks.
static int issue_on_slot(Context* c, StreamSlot& slot, const BatchCall& b, const StepShape& q, const StepPlan& plan, const void* d_input) {
    const int rc = ensure_workspace(c, slot, plan.workspace_frames, b.stream);
    if (rc < 0) {
        return rc;
    }
    if (plan.workspace_frames) {
        slot.exp_codec = -1;   // the rows of an earlier mbx_expand_records() are about to be replaced
    }
    const unsigned order = slot.launches++;
    switch (plan.form) {
    case mbx::kOneLaunchStep:
        return launch_one_launch(c, slot, (order & 1u) != 0u, b, static_cast<const uint8_t*>(d_input), plan);
    case mbx::kFusedOneStep:
        return launch_fused_one(c, (order & 1u) != 0u, b, static_cast<const uint8_t*>(d_input), plan);
    case mbx::kMixedStep:
        return run_mixed_stages(c, b, plan, d_input, slot.workspace);
    default:   // (a ragged step walks its streams in the order kernel's order or the grid's: no direction)
        return run_stages(c, plan.form == mbx::kRaggedStep ? 0u : order, b, q, plan, d_input, slot.workspace, &slot);
    }
}
static int run_batch(Context* c, const char* who, const BatchCall& b, InputKind kind, const void* d_input, const CallerWorkspace* caller_ws) {
    const bool mixed = b.stream_codec != nullptr;   // every stream brings its codec (wire frames or soft cells only): b.codec is not looked at
    const mbx::CodecShape* sh = mbx::codec_shape(b.codec);
    if (!d_input || !call_args_ok(b) || (kind == kRecords && (mixed || !mbx::codec_streams(b.codec))) || (kind == kSoft && !sh && !mixed) ||
        (mixed && !b.frame_offset)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!call_aligned(b) || (kind == kSoft && !aligned_to(d_input, 2)) || (kind == kFrames && !frames_aligned(d_input, mixed || imbe_codec(b.codec))) ||
        (caller_ws && !aligned_to(caller_ws->p, 16))) {
        return !aligned_to(b.keystream, 4) ? mbx::misaligned(who, "mbx_keystream.h") : misaligned(who);   // (the table that has the pointer's row)
    }
    const size_t n = batch_rows(b);
    if (b.S == 0 || n == 0) {
        return 0;
    }
    if (!sh && !mixed) {   // (a hard-frame step has always come to its codec only here, after the empty batch)
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    char text[128];
    if ((kind == kSoft || b.frame_offset) && n > 0x7fffffffu) {   // (ragged offsets are int32_t)
        snprintf(text, sizeof(text), "%s: more than 2^31-1 frames in one launch", who);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    StepShape q = step_shape(b, kind, d_input, caller_ws == nullptr);
    const StepPlan plan = plan_on_stream(c, q, b.stream);
    if (caller_ws) {
        unsigned order;
        {
            std::lock_guard<std::mutex> lock(c->mu);
            StreamSlot& slot = c->slots[b.stream];
            if (plan.form == mbx::kFusedOneStep) {
                return launch_fused_one(c, (slot.launches++ & 1u) != 0u, b, static_cast<const uint8_t*>(d_input), plan);
            }
            if (plan.expand && (!caller_ws->p || caller_ws->bytes < mbx_workspace_bytes(plan.workspace_frames))) {
                snprintf(text, sizeof(text), "%s: workspace missing or smaller than mbx_workspace_bytes(S*T)", who);
                return fail(MBE_STATUS_INVALID_ARGUMENT, text);
            }
            order = slot.launches++;
        }
        return run_stages(c, order, b, q, plan, d_input, static_cast<mbx::FrameParams*>(caller_ws->p), nullptr);
    }
    std::lock_guard<std::mutex> lock(c->mu);
    return issue_on_slot(c, c->slots[b.stream], b, q, plan, d_input);
}

int mbx_process_records(int codec, int S, int T, const mbx_param_record* d_records, mbe_parms* d_state,
                        mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                        void* stream) {
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, const_cast<mbx_param_record*>(d_records), d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr};
    return run_batch(c, "mbx_process_records", b, kRecords, d_records, nullptr);
}

int mbx_process_records_ws(int codec, int S, int T, const mbx_param_record* d_records, mbe_parms* d_state,
                           mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                           void* d_workspace, size_t workspace_bytes, void* stream) {
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, const_cast<mbx_param_record*>(d_records), d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr};
    const CallerWorkspace ws{d_workspace, workspace_bytes};
    return run_batch(c, "mbx_process_records_ws", b, kRecords, d_records, &ws);
}

// (mbx_process_batch and its _ws form refuse what they can before they ask for a context; the other batch calls ask first)
int mbx_process_batch(int codec, int S, int T, const uint8_t* d_frames, mbe_parms* d_state, mbx_stream_rng* d_rng,
                      int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records,
                      void* stream) {
    if (!d_frames || !d_records || S < 0 || T < 0 || !mbx::codec_shape(codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!batch_pointers_aligned(d_records, d_state, d_rng, d_pcm16, d_pcmf, d_results, nullptr, nullptr, nullptr) ||
        !frames_aligned(d_frames, imbe_codec(codec))) {
        return misaligned("mbx_process_batch");
    }
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, d_records, d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr};
    return run_batch(c, "mbx_process_batch", b, kFrames, d_frames, nullptr);
}

int mbx_stage_in(void* d_dst, const void* pinned_src, size_t bytes, void* stream) {
    if (!d_dst || !pinned_src) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (bytes == 0) {
        return 0;
    }
    if ((reinterpret_cast<uintptr_t>(d_dst) | reinterpret_cast<uintptr_t>(pinned_src)) & 15u) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_stage_in: both buffers must be 16-byte aligned");
    }
    const size_t threads = (bytes >> 4) + 1;
    hipLaunchKernelGGL(mbx::stage_in_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(pinned_src), static_cast<uint8_t*>(d_dst), bytes);
    return check_launch("stage_in_kernel");
}

// one frame of one stream (b.S = b.T = 1) as one launch of one wavefront
static int launch_frame(const BatchCall& b, const uint8_t* d_frame, uint32_t* d_done, uint32_t token, const mbx::FrameShadow& shadow) {
    REQUIRE_CTX(c);
    if (!d_frame || !call_args_ok(b) || !mbx::codec_shape(b.codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!call_aligned(b) || !frames_aligned(d_frame, imbe_codec(b.codec)) || !aligned_to(d_done, 4) || !aligned_to(shadow.state, 4) ||
        !aligned_to(shadow.rng, 8) || !aligned_to(shadow.ok, 4)) {
        return misaligned("mbx_process_frame");
    }
    const mbx::DeviceTables tabs = launch_tables(c, false, b);
    const hipStream_t stream = (hipStream_t)b.stream;
    if (imbe_codec(b.codec)) {
        hipLaunchKernelGGL(mbx::imbe_frame_kernel, dim3(1), dim3(64), 0, stream, b.codec, d_frame, b.records, b.state, b.rng, b.pcm16, b.pcmf,
                           b.results, d_done, token, tabs, shadow);
    } else if (b.codec == MBX_CODEC_AMBE3600X2400) {
        hipLaunchKernelGGL(mbx::ambe2400_frame_kernel, dim3(1), dim3(64), 0, stream, d_frame, b.records, b.state, b.rng, b.pcm16, b.pcmf,
                           b.results, d_done, token, tabs, shadow);
    } else {
        hipLaunchKernelGGL(mbx::ambe_frame_kernel, dim3(1), dim3(64), 0, stream, d_frame, b.records, b.state, b.rng, b.pcm16, b.pcmf, b.results,
                           d_done, token, tabs, shadow);
    }
    return check_launch("frame_kernel");
}

int mbx_process_frame(int codec, const uint8_t* d_frame, mbe_parms* d_state, mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf,
                      mbe_process_result* d_result, mbx_param_record* d_record, uint32_t* d_done, uint32_t token, void* stream) {
    return launch_frame({codec, 1, 1, d_record, d_state, d_rng, d_pcm16, d_pcmf, d_result, stream, nullptr, nullptr}, d_frame, d_done, token,
                        mbx::FrameShadow{});
}

int mbx_process_frame_shadow(int codec, const uint8_t* d_frame, mbe_parms* d_state, mbx_stream_rng* d_rng, int16_t* d_pcm16, float* d_pcmf,
                             mbe_process_result* d_result, mbx_param_record* d_record, uint32_t* d_done, uint32_t token,
                             mbe_parms* d_shadow_state, mbx_stream_rng* d_shadow_rng, uint32_t* d_shadow_ok, int use_shadow,
                             const uint8_t* h_frame, void* stream) {
    if (!d_shadow_state || !d_shadow_rng || !d_shadow_ok) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    mbx::FrameShadow shadow;
    shadow.state = d_shadow_state;
    shadow.rng = d_shadow_rng;
    shadow.ok = d_shadow_ok;
    shadow.use = use_shadow ? 1u : 0u;
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (h_frame && sh) {   // the frame's bytes travel with the launch (no such codec: launch_frame refuses the call)
        memcpy(shadow.frame_words, h_frame, (size_t)sh->frame_bytes);
        shadow.have_frame = 1u;
    }
    return launch_frame({codec, 1, 1, d_record, d_state, d_rng, d_pcm16, d_pcmf, d_result, stream, nullptr, nullptr}, d_frame, d_done, token, shadow);
}

int mbx_frame_server_start(mbx_frame_mailbox* mailbox, unsigned idle_us, mbe_parms* d_state, mbx_stream_rng* d_rng, int16_t* d_pcm16,
                           float* d_pcmf, mbe_process_result* d_result, mbx_param_record* d_record, mbe_parms* d_shadow_state,
                           mbx_stream_rng* d_shadow_rng, uint32_t* d_shadow_ok, void* stream) {
    REQUIRE_CTX(c);
    if (!mailbox || (reinterpret_cast<uintptr_t>(mailbox) & 63u) || idle_us == 0 || idle_us > 1000000u || !d_state || !d_rng || !d_record
        || ((d_shadow_state != nullptr) != (d_shadow_rng != nullptr)) || ((d_shadow_state != nullptr) != (d_shadow_ok != nullptr))) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    mbx::FrameShadow shadow;
    shadow.state = d_shadow_state;
    shadow.rng = d_shadow_rng;
    shadow.ok = d_shadow_ok;
    mbx::DeviceTables tabs = c->tabs;
    tabs.reverse = 0;
    tabs.stream_map = nullptr;
    tabs.resident = nullptr;
    hipLaunchKernelGGL(mbx::frame_server_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, mailbox, idle_us * 100u, d_state, d_rng,
                       d_pcm16, d_pcmf, d_result, d_record, tabs, shadow);
    return check_launch("frame_server_kernel");
}

int mbx_process_batch_ws(int codec, int S, int T, const uint8_t* d_frames, mbe_parms* d_state, mbx_stream_rng* d_rng,
                         int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!d_frames || !d_records || S < 0 || T < 0 || !mbx::codec_shape(codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, d_records, d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr};
    const CallerWorkspace ws{d_workspace, workspace_bytes};
    return run_batch(c, "mbx_process_batch_ws", b, kFrames, d_frames, &ws);
}

int mbx_process_batch_indexed(int codec, int S, int T, const int32_t* d_stream_index, const uint8_t* d_frames,
                              mbe_parms* d_state_pool, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf,
                              mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    REQUIRE_CTX(c);
    if (!d_stream_index) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const BatchCall b{codec, S, T, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, nullptr};
    return run_batch(c, "mbx_process_batch_indexed", b, kFrames, d_frames, nullptr);
}

// ---- resident state (sessions, queue mode) ------------------------------------------------------------------------------
// The drop-in batch calls above keep the reference's three structs per stream whole after every launch: a caller may read
// them at any time.  A caller that OWNS the state for a while (a session; the queue mode's device pool) does not need that:
// after every ordinary frame prev_mp_enhanced is a field-for-field copy of cur_mp (ref src/imbe/imbe7200x4400.c:842-856,
// src/ambe/ambe3600x2450.c:790-800), so d_resident[slot] != 0 says "elided" and the kernels neither write nor read that struct;
// and of prev_mp a launch fetches only what the decode reads.  At T = 1 that is 8.9 KB of state traffic per frame instead of
// 14.1 KB.  mbx_resident_materialize() brings the triplets back to the ABI form (bit-identical to what mbx_process_batch
// would have left), after which d_resident is zero again.
int mbx_process_batch_resident(int codec, int S, int T, const int32_t* d_stream_index, const uint8_t* d_frames,
                               mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16,
                               float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    REQUIRE_CTX(c);
    if (!d_resident) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const BatchCall b{codec, S, T, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, d_resident};
    return run_batch(c, "mbx_process_batch_resident", b, kFrames, d_frames, nullptr);
}

namespace mbx {
// prev_mp_enhanced := cur_mp for every listed slot whose struct is elided; one wavefront per slot
__global__ void __launch_bounds__(64)
resident_materialize_kernel(int n, const int32_t* __restrict__ index, mbe_parms* __restrict__ state, uint32_t* __restrict__ resident) {
    const int i = blockIdx.x;
    if (i >= n) {
        return;
    }
    const size_t slot = index ? (size_t)index[i] : (size_t)i;
    if (resident[slot] == 0u) {
        return;
    }
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&state[3 * slot + 0]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&state[3 * slot + 2]);
    for (int k = threadIdx.x; k < (int)(sizeof(mbe_parms) / 4); k += 64) {
        dst[k] = src[k];
    }
    if (threadIdx.x == 0) {
        resident[slot] = 0u;
    }
}
}  // namespace mbx

int mbx_resident_materialize(int n, const int32_t* d_stream_index, mbe_parms* d_state_pool, uint32_t* d_resident, void* stream) {
    REQUIRE_CTX(c);
    (void)c;
    if (!d_state_pool || !d_resident || n < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_state_pool, 4) || !aligned_to(d_resident, 4) || !aligned_to(d_stream_index, 4)) {
        return misaligned("mbx_resident_materialize");
    }
    if (n == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::resident_materialize_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, n, d_stream_index,
                       d_state_pool, d_resident);
    return check_launch("resident_materialize_kernel");
}

// ---- soft-decision batches: run_batch with kSoft ------------------------------------------------------------------------------------
int mbx_process_batch_soft(int codec, int S, int T, const mbe_soft_bit* d_soft, mbe_parms* d_state, mbx_stream_rng* d_rng,
                           int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records,
                           void* stream) {
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, d_records, d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr};
    return run_batch(c, "mbx_process_batch_soft", b, kSoft, d_soft, nullptr);
}

int mbx_process_batch_soft_ws(int codec, int S, int T, const mbe_soft_bit* d_soft, mbe_parms* d_state, mbx_stream_rng* d_rng,
                              int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records,
                              void* d_workspace, size_t workspace_bytes, void* stream) {
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, d_records, d_state, d_rng, d_pcm16, d_pcmf, d_results, stream, nullptr, nullptr};
    const CallerWorkspace ws{d_workspace, workspace_bytes};
    return run_batch(c, "mbx_process_batch_soft_ws", b, kSoft, d_soft, &ws);
}

// (index NULL = identity, d_resident NULL = plain triplets: nothing here that is this export's own to refuse)
int mbx_process_batch_soft_resident(int codec, int S, int T, const int32_t* d_stream_index, const mbe_soft_bit* d_soft,
                                    mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16,
                                    float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    REQUIRE_CTX(c);
    const BatchCall b{codec, S, T, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, d_resident};
    return run_batch(c, "mbx_process_batch_soft_resident", b, kSoft, d_soft, nullptr);
}

// ---- burst launches (include/mbx_burst.h): the gather of mbx_burst.hip, then issue_on_slot ------------------------------------------
// One launch in front of the step the frames calls run for (codec, S, T = frames per burst), on the caller's stream.  The gathered
// frames live in the stream slot's workspace BEHIND the S * T rows of the step (256-byte aligned: a T = 1 step takes its one-launch
// kernel), so c->mu is held from the growth of the workspace to the last launch, as run_batch holds it.  (The workspace is grown ONCE,
// to mbx_burst_workspace_frames, which covers the rows of whatever the step's plan is: nothing grows -- frees -- it behind the gather.)
static int process_bursts(const char* who, bool soft, const mbx_burst_schedule* sched, int S, const int32_t* d_stream_index, const void* d_bursts,
                          size_t burst_stride, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf,
                          mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    char text[160];
    // (alignment first: it needs neither the schedule nor a device)
    if (!batch_pointers_aligned(d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, d_stream_index, d_resident, nullptr) ||
        !aligned_to(d_bursts, soft ? (sched ? mbx::burst_shape(sched).soft_align() : 2) : 1)) {
        return misaligned(who);
    }
    if (!sched || !d_bursts || !d_records || !d_state_pool || !d_rng_pool || S < 0) {
        snprintf(text, sizeof(text), "%s: schedule, bursts, state, RNG state and records are all needed", who);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    const mbx::BurstShape sh = mbx::burst_shape(sched);
    if (!soft && sh.llr()) {
        snprintf(text, sizeof(text), "%s: an LLR schedule has soft bursts only", who);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    if (!soft && burst_stride < sh.bytes) {
        snprintf(text, sizeof(text), "%s: burst_stride is below mbx_burst_schedule_bytes()", who);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    REQUIRE_CTX(c);
    if (sh.device != c->device) {
        snprintf(text, sizeof(text), "%s: the schedule was made on device %d, the current device is %d", who, sh.device, c->device);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    if (S == 0) {
        return 0;
    }
    const size_t n = (size_t)S * (size_t)sh.frames;
    if (n > 0x7fffffffu) {
        snprintf(text, sizeof(text), "%s: more than 2^31-1 frames in one launch", who);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    const BatchCall b{sh.codec, S, sh.frames, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, d_resident};
    StepShape q = step_shape(b, soft ? kSoft : kFrames, nullptr, true);   // (the gathered frames: 256-byte aligned)
    const StepPlan plan = plan_on_stream(c, q, stream);
    std::lock_guard<std::mutex> lock(c->mu);
    StreamSlot& slot = c->slots[stream];
    int rc = ensure_workspace(c, slot, mbx_burst_workspace_frames(sched, S, soft ? 1 : 0), stream);
    if (rc < 0) {
        return rc;
    }
    slot.exp_codec = -1;   // rows an earlier mbx_expand_records() left behind the step's own are being replaced
    void* const gathered = slot.workspace + n;
    rc = mbx::burst_gather(sched, soft, d_bursts, burst_stride, (size_t)S, gathered, soft ? sh.cells : sh.frame_bytes, stream);
    if (rc < 0) {
        return rc;
    }
    return issue_on_slot(c, slot, b, q, plan, gathered);
}

int mbx_process_bursts(const mbx_burst_schedule* sched, int S, const int32_t* d_stream_index, const uint8_t* d_bursts, size_t burst_stride,
                       mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf,
                       mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    return process_bursts("mbx_process_bursts", false, sched, S, d_stream_index, d_bursts, burst_stride, d_state_pool, d_resident, d_rng_pool, d_pcm16,
                          d_pcmf, d_results, d_records, stream);
}

int mbx_process_bursts_soft(const mbx_burst_schedule* sched, int S, const int32_t* d_stream_index, const mbe_soft_bit* d_soft, mbe_parms* d_state_pool,
                            uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                            mbx_param_record* d_records, void* stream) {
    return process_bursts("mbx_process_bursts_soft", true, sched, S, d_stream_index, d_soft, 0, d_state_pool, d_resident, d_rng_pool, d_pcm16, d_pcmf,
                          d_results, d_records, stream);
}

// ---- burst groups (include/mbx_burst_groups.h): ONE gather over the bursts of up to eight schedules, then ONE mixed step -------------
// As process_bursts: check, a mixed StepShape, plan_on_stream, c->mu held from the ONE growth of the workspace (to
// mbx_burst_groups_workspace_frames, which covers the step's own rows) to the last launch.  The workspace (mbx_group_plan.h): the
// step's rows | the gathered mixed rows | the layout words frame_offset, stream_index, stream_codec, which the gather launch itself
// writes -- nothing is uploaded, and the mixed step (run_mixed_stages) runs unchanged on those arrays.
static StepShape groups_step_shape(const mbx::GroupPlan& gp, bool soft, bool resident) {
    StepShape q;
    q.S = gp.total_streams, q.total = (size_t)gp.total_rows;
    q.kind = soft ? kSoft : kFrames;
    q.resident = resident;
    q.ragged = q.mixed = true;
    q.aligned = true;   // (the gathered rows: 256-byte aligned)
    q.own_workspace = q.slices_allowed = true;
    return q;
}
static mbx::GroupWorkspace groups_workspace(const Context* c, const mbx::GroupPlan& gp, const StepShape& q, bool soft) {
    const size_t row = soft ? (size_t)MBX_MIXED_ROW_CELLS * sizeof(mbe_soft_bit) : (size_t)MBX_MIXED_ROW_BYTES;
    return mbx::group_workspace(gp, plan_of(c, q).workspace_frames, sizeof(mbx::FrameParams), row);
}

size_t mbx_burst_groups_workspace_frames(const mbx_burst_group* groups, int n_groups, int soft) {
    mbx::GroupShape shapes[MBX_BURST_MAX_GROUPS];
    mbx::GroupPlan gp;
    if (mbx::burst_groups_plan("mbx_burst_groups_workspace_frames", groups, n_groups, soft != 0, shapes, &gp) < 0 || gp.total_rows == 0) {
        return 0;
    }
    // (the workspace of a step does not depend on the device or on the elision words: no context is asked for)
    return groups_workspace(nullptr, gp, groups_step_shape(gp, soft != 0, false), soft != 0).frames;
}

int mbx_process_burst_groups(const mbx_burst_group* groups, int n_groups, int soft_in, mbe_parms* d_state_pool, uint32_t* d_resident,
                             mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                             mbx_param_record* d_records, void* stream) {
    const char* const who = "mbx_process_burst_groups";
    const bool soft = soft_in != 0;
    char text[160];
    if (!batch_pointers_aligned(d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, nullptr, d_resident, nullptr)) {
        return mbx::misaligned(who, "mbx_burst_groups.h");
    }
    mbx::GroupShape shapes[MBX_BURST_MAX_GROUPS];
    mbx::GroupPlan gp;
    int rc = mbx::burst_groups_plan(who, groups, n_groups, soft, shapes, &gp);
    if (rc < 0) {
        return rc;
    }
    if (!d_state_pool || !d_rng_pool || (gp.total_rows > 0 && !d_records)) {
        snprintf(text, sizeof(text), "%s: state, RNG state and records are all needed", who);
        return fail(MBE_STATUS_INVALID_ARGUMENT, text);
    }
    REQUIRE_CTX(c);
    for (int i = 0; i < n_groups; ++i) {
        const int dev = mbx::burst_shape(groups[i].sched).device;
        if (dev != c->device) {
            snprintf(text, sizeof(text), "%s: a schedule was made on device %d, the current device is %d", who, dev, c->device);
            return fail(MBE_STATUS_INVALID_ARGUMENT, text);
        }
    }
    if (gp.total_rows == 0) {
        return 0;
    }
    StepShape q = groups_step_shape(gp, soft, d_resident != nullptr);
    const StepPlan plan = plan_on_stream(c, q, stream);
    const mbx::GroupWorkspace w = groups_workspace(c, gp, q, soft);
    mbx::GroupGather gather[MBX_BURST_MAX_GROUPS];
    int count = 0;
    for (int i = 0; i < n_groups; ++i) {   // the groups that have a workgroup, in grid order
        const mbx::GroupPlace& p = gp.place[i];
        if (p.bursts) {
            gather[count++] = mbx::GroupGather{groups[i].sched, groups[i].bursts, groups[i].burst_stride, p.bursts, groups[i].bursts_per_stream,
                                               groups[i].stream_index, groups[i].first_slot, p.first_wg, p.first_row, p.first_stream};
        }
    }
    std::lock_guard<std::mutex> lock(c->mu);
    StreamSlot& slot = c->slots[stream];
    rc = ensure_workspace(c, slot, w.frames, stream);
    if (rc < 0) {
        return rc;
    }
    slot.exp_codec = -1;   // rows an earlier mbx_expand_records() left behind the step's own are being replaced
    uint8_t* const base = reinterpret_cast<uint8_t*>(slot.workspace);
    void* const gathered = base + w.gathered;
    const mbx::GroupLayout layout{gp.total_streams, gp.total_rows, reinterpret_cast<int32_t*>(base + w.frame_offset),
                                  reinterpret_cast<int32_t*>(base + w.stream_index), base + w.stream_codec};
    rc = mbx::burst_gather_groups(gather, count, soft, gp.grid, gp.lds, layout, gathered, stream);
    if (rc < 0) {
        return rc;
    }
    BatchCall b{0, gp.total_streams, 0, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, layout.d_stream_index, d_resident};
    b.frame_offset = layout.d_frame_offset;
    b.total = (size_t)gp.total_rows;
    b.stream_codec = layout.d_stream_codec;
    return issue_on_slot(c, slot, b, q, plan, gathered);
}

// ---- ragged batches: run_batch with BatchCall::frame_offset ---------------------------------------------------------------------------
// (what can be refused without a device is refused before one is asked for, as mbx_process_batch does)
// (`mixed`: d_stream_codec is the codec of every stream row and `codec` is not looked at)
static int process_batch_ragged(const char* who, InputKind kind, bool mixed, int codec, int S, const uint8_t* d_stream_codec,
                                const int32_t* d_frame_offset, size_t total_frames, const int32_t* d_stream_index, const void* d_input,
                                mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf,
                                mbe_process_result* d_results, mbx_param_record* d_records, void* stream, const uint8_t* d_keystream = nullptr) {
    const bool empty = S == 0 || total_frames == 0;   // (a batch without frames has no frame and no record array to name)
    if (!d_frame_offset || !d_state_pool || !d_rng_pool || S < 0 || (mixed ? !d_stream_codec : !mbx::codec_shape(codec)) ||
        (!empty && (!d_input || !d_records))) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!batch_pointers_aligned(d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, d_stream_index, d_resident, d_frame_offset) ||
        (kind == kSoft && !aligned_to(d_input, 2)) || (kind == kFrames && !frames_aligned(d_input, mixed || imbe_codec(codec))) ||
        !aligned_to(d_keystream, 4)) {
        return !aligned_to(d_keystream, 4) ? mbx::misaligned(who, "mbx_keystream.h") : misaligned(who);
    }
    REQUIRE_CTX(c);
    if (empty) {
        return 0;
    }
    BatchCall b{codec, S, 0, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, d_resident};
    b.frame_offset = d_frame_offset;
    b.total = total_frames;
    b.stream_codec = mixed ? d_stream_codec : nullptr;
    b.keystream = d_keystream;
    return run_batch(c, who, b, kind, d_input, nullptr);
}
int mbx_process_batch_ragged(int codec, int S, const int32_t* d_frame_offset, size_t total_frames, const int32_t* d_stream_index,
                             const uint8_t* d_frames, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                             int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    return process_batch_ragged("mbx_process_batch_ragged", kFrames, false, codec, S, nullptr, d_frame_offset, total_frames, d_stream_index, d_frames, d_state_pool,
                                d_resident, d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, stream);
}
int mbx_process_batch_soft_ragged(int codec, int S, const int32_t* d_frame_offset, size_t total_frames, const int32_t* d_stream_index,
                                  const mbe_soft_bit* d_soft, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                                  int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    return process_batch_ragged("mbx_process_batch_soft_ragged", kSoft, false, codec, S, nullptr, d_frame_offset, total_frames, d_stream_index, d_soft, d_state_pool,
                                d_resident, d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, stream);
}

// ---- mixed ragged batches: a ragged batch call with BatchCall::stream_codec ---------------------------------------------------------------
int mbx_process_batch_mixed(int S, const uint8_t* d_stream_codec, const int32_t* d_frame_offset, size_t total_frames, const int32_t* d_stream_index,
                            const uint8_t* d_frames, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16,
                            float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    return process_batch_ragged("mbx_process_batch_mixed", kFrames, true, 0, S, d_stream_codec, d_frame_offset, total_frames, d_stream_index, d_frames,
                                d_state_pool, d_resident, d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, stream);
}
int mbx_process_batch_soft_mixed(int S, const uint8_t* d_stream_codec, const int32_t* d_frame_offset, size_t total_frames,
                                 const int32_t* d_stream_index, const mbe_soft_bit* d_soft, mbe_parms* d_state_pool, uint32_t* d_resident,
                                 mbx_stream_rng* d_rng_pool, int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results,
                                 mbx_param_record* d_records, void* stream) {
    return process_batch_ragged("mbx_process_batch_soft_mixed", kSoft, true, 0, S, d_stream_codec, d_frame_offset, total_frames, d_stream_index, d_soft,
                                d_state_pool, d_resident, d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, stream);
}

// ---- keystream input (include/mbx_keystream.h): run_batch with BatchCall::keystream --------------------------------------------------
// The caller steps in where the reference's callers do, between mbe_decodeImbe7200x4400Frame / mbe_decodeAmbe3600x2450Frame and
// mbe_processImbe4400Dataf / mbe_processAmbe2450Dataf (ref src/imbe/imbe7200x4400.c:935-948, src/ambe/ambe3600x2450.c:684-714).
int mbx_keystream_apply_host(int codec, mbx_param_record* records, size_t n, const uint8_t* keystream) {
    const int nbits = mbx::keystream_nbits(codec);
    if (!records || !keystream || nbits == 0) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_keystream_apply_host: records and keystream are needed, codec is one of MBX_CODEC_*");
    }
    for (size_t i = 0; i < n; ++i) {
        const mbx::KeystreamWords k = mbx::keystream_words_of_row(keystream + i * (size_t)MBX_KEYSTREAM_ROW_BYTES, nbits);
        records[i].w[0] ^= k.x;
        records[i].w[1] ^= k.y;
        records[i].w[2] ^= k.z;
    }
    return 0;
}

int mbx_apply_keystream(int codec, mbx_param_record* d_records, size_t n, const uint8_t* d_keystream, void* stream) {
    static_assert(MBX_KEYSTREAM_ROW_BYTES == mbx::kKeystreamRowBytes, "one row size, stated in the public header and in the words header");
    const int nbits = mbx::keystream_nbits(codec);
    if (!d_records || !d_keystream || nbits == 0) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_apply_keystream: d_records and d_keystream are needed, codec is one of MBX_CODEC_*");
    }
    if (!aligned_to(d_records, 16)) {
        return misaligned("mbx_apply_keystream");
    }
    if (!aligned_to(d_keystream, 4)) {
        return mbx::misaligned("mbx_apply_keystream", "mbx_keystream.h");
    }
    REQUIRE_CTX(c);
    (void)c;
    if (n == 0) {
        return 0;
    }
    if (n > 0x7fffffffu) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_apply_keystream: more than 2^31-1 records in one launch");
    }
    hipLaunchKernelGGL(mbx::keystream_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nbits, d_records, n, d_keystream);
    return check_launch("keystream_apply_kernel");
}

// S x T: every uniform form in one entry point -- index or none, resident words or ABI triplets, hard frames or soft cells.  Without
// a keystream it is the unkeyed call of the same form, launch for launch.
int mbx_process_batch_keyed(int codec, int S, int T, const int32_t* d_stream_index, const uint8_t* d_frames, const mbe_soft_bit* d_soft,
                            const uint8_t* d_keystream, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                            int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    if ((d_frames != nullptr) == (d_soft != nullptr)) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_process_batch_keyed: exactly one of d_frames and d_soft is given");
    }
    REQUIRE_CTX(c);
    BatchCall b{codec, S, T, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, d_resident};
    b.keystream = d_keystream;
    return d_soft ? run_batch(c, "mbx_process_batch_keyed", b, kSoft, d_soft, nullptr) : run_batch(c, "mbx_process_batch_keyed", b, kFrames, d_frames, nullptr);
}

// ragged, and mixed where d_stream_codec is given (rows of MBX_MIXED_ROW_BYTES / MBX_MIXED_ROW_CELLS, `codec` unused)
int mbx_process_batch_ragged_keyed(int codec, const uint8_t* d_stream_codec, int S, const int32_t* d_frame_offset, size_t total_frames,
                                   const int32_t* d_stream_index, const uint8_t* d_frames, const mbe_soft_bit* d_soft,
                                   const uint8_t* d_keystream, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                                   int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, void* stream) {
    if ((d_frames != nullptr) == (d_soft != nullptr)) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_process_batch_ragged_keyed: exactly one of d_frames and d_soft is given");
    }
    return process_batch_ragged("mbx_process_batch_ragged_keyed", d_soft ? kSoft : kFrames, d_stream_codec != nullptr, d_stream_codec ? 0 : codec, S,
                                d_stream_codec, d_frame_offset, total_frames, d_stream_index, d_soft ? static_cast<const void*>(d_soft) : d_frames,
                                d_state_pool, d_resident, d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, stream, d_keystream);
}

// ---- voted streams (include/mbx_vote.h): the vote launch of mbx_vote.hip between the front launch and the records step -----------------
// One entry for the hard and the soft step: what plan_step says of a StepShape with `vote` set -- the frames the front launch runs
// over, where in the stream's workspace the candidates' records (select) or the combined cells (combine) sit behind the rows, and the
// stream stage of the records step of the same S x T -- issued as a linear chain on the caller's stream under c->mu.
static StepShape voted_shape(const mbx_vote_plan* plan, int codec, int mode, bool soft, int T, bool resident, const void* d_cand) {
    StepShape q;
    q.codec = codec, q.S = plan->S, q.T = T;
    q.kind = soft ? kSoft : kFrames;
    q.resident = resident;
    q.aligned = (reinterpret_cast<uintptr_t>(d_cand) & 3u) == 0;
    q.own_workspace = true;
    q.vote = mode == mbx::kVoteCombine ? mbx::kCombineVote : mbx::kSelectVote;
    q.candidates = plan->C;
    q.row_cells = mbx::kCodecs[codec].cells;
    return q;
}
static int process_batch_voted(const char* who, const mbx_vote_plan* plan, int codec, int mode, bool soft, int T, const int32_t* d_stream_index,
                               const void* d_cand, const uint8_t* d_present, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool,
                               int16_t* d_pcm16, float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, mbx_vote_record* d_votes,
                               void* stream) {
    if (!plan || !d_cand || !d_state_pool || !d_rng_pool || !d_records) {
        return mbx::refuse(who, "a plan, the candidates, the state pool, the RNG pool and a place for the voted records are needed");
    }
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!sh) {
        return mbx::refuse(who, "codec is one of MBX_CODEC_*");
    }
    if (!mbx::vote_mode_ok(mode) || (mode == mbx::kVoteCombine && !soft)) {
        return mbx::refuse(who, "mode is MBX_VOTE_SELECT or MBX_VOTE_COMBINE");
    }
    const mbx::VoteRefusal shape = mbx::vote_shape_refused(plan->C, T);
    if (shape != mbx::kVoteOk) {
        return mbx::refuse(who, mbx::vote_refusal_text(shape));
    }
    if (!aligned_to(d_votes, 8) || (soft && !aligned_to(d_cand, 16))) {
        return mbx::misaligned(who, "mbx_vote.h");
    }
    if (!batch_pointers_aligned(d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, d_stream_index, d_resident, nullptr) ||
        (!soft && !frames_aligned(d_cand, imbe_codec(codec)))) {
        return misaligned(who);
    }
    REQUIRE_CTX(c);
    if (plan->device != (int)(c - g_ctx)) {
        return mbx::refuse(who, "a plan of another device than the current one");
    }
    if (T == 0) {
        return 0;
    }
    const BatchCall b{codec, plan->S, T, d_records, d_state_pool, d_rng_pool, d_pcm16, d_pcmf, d_results, stream, d_stream_index, d_resident};
    const StepShape q = voted_shape(plan, codec, mode, soft, T, d_resident != nullptr, d_cand);
    const StepPlan vp = plan_of(c, q);   // (never one that holds outside capture only: see plan_step)
    if (vp.form != mbx::kStagedStep) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    std::lock_guard<std::mutex> lock(c->mu);
    StreamSlot& slot = c->slots[stream];
    int rc = ensure_workspace(c, slot, vp.workspace_frames, stream);
    if (rc < 0) {
        return rc;
    }
    slot.exp_codec = -1;   // the rows of an earlier mbx_expand_records() are about to be replaced
    const unsigned order = slot.launches++;
    void* const behind = slot.workspace + vp.vote_offset;
    if (vp.vote == mbx::kCombineVote) {
        mbe_soft_bit* const cells = static_cast<mbe_soft_bit*>(behind);
        rc = mbx::vote_combine_launch(plan, sh->cells, T, static_cast<const mbe_soft_bit*>(d_cand), d_present, cells, d_votes, stream);
        if (rc >= 0) {
            rc = launch_soft_fec(c, codec, true, cells, vp.front_frames, d_records, stream);
        }
    } else {
        mbx_param_record* const cand_records = static_cast<mbx_param_record*>(behind);
        rc = soft ? launch_soft_fec(c, codec, true, static_cast<const mbe_soft_bit*>(d_cand), vp.front_frames, cand_records, stream)
                  : launch_fec(c, codec, static_cast<const uint8_t*>(d_cand), vp.front_frames, cand_records, stream);
        if (rc >= 0) {
            rc = mbx::vote_select_launch(plan, T, cand_records, d_present, d_records, d_votes, stream);
        }
    }
    if (rc < 0) {
        return rc;
    }
    StepPlan rest = vp;   // behind the vote: the records step's expand launch and stream kernel
    rest.front = mbx::kNoFront;
    return run_stages(c, order, b, q, rest, d_records, slot.workspace, nullptr);
}

size_t mbx_vote_workspace_frames(const mbx_vote_plan* plan, int codec, int mode, int T) {
    if (!plan || !mbx::codec_shape(codec) || !mbx::vote_mode_ok(mode) || T < 0) {
        return 0;
    }
    return plan_of(nullptr, voted_shape(plan, codec, mode, true, T, false, nullptr)).workspace_frames;
}

int mbx_process_batch_voted(const mbx_vote_plan* plan, int codec, int T, const int32_t* d_stream_index, const uint8_t* d_cand_frames,
                            const uint8_t* d_present, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16,
                            float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, mbx_vote_record* d_votes, void* stream) {
    return process_batch_voted("mbx_process_batch_voted", plan, codec, MBX_VOTE_SELECT, false, T, d_stream_index, d_cand_frames, d_present, d_state_pool,
                               d_resident, d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, d_votes, stream);
}
int mbx_process_batch_soft_voted(const mbx_vote_plan* plan, int codec, int mode, int T, const int32_t* d_stream_index, const mbe_soft_bit* d_cand_soft,
                                 const uint8_t* d_present, mbe_parms* d_state_pool, uint32_t* d_resident, mbx_stream_rng* d_rng_pool, int16_t* d_pcm16,
                                 float* d_pcmf, mbe_process_result* d_results, mbx_param_record* d_records, mbx_vote_record* d_votes, void* stream) {
    return process_batch_voted("mbx_process_batch_soft_voted", plan, codec, mode, true, T, d_stream_index, d_cand_soft, d_present, d_state_pool, d_resident,
                               d_rng_pool, d_pcm16, d_pcmf, d_results, d_records, d_votes, stream);
}

int mbx_synthesize_speech(int S, mbe_parms* d_cur, mbe_parms* d_prev, mbx_stream_rng* d_rng, float* d_pcmf,
                          int16_t* d_pcm16, void* stream) {
    REQUIRE_CTX(c);
    if (!d_cur || !d_prev || !d_rng || S < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_cur, 4) || !aligned_to(d_prev, 4) || !aligned_to(d_rng, 8) || !aligned_to(d_pcmf, 4) || !aligned_to(d_pcm16, 2)) {
        return misaligned("mbx_synthesize_speech");
    }
    if (S == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::synth_speech_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, S, d_cur, d_prev,
                       d_rng, d_pcmf, d_pcm16, c->tabs);
    return check_launch("synth_speech_kernel");
}

int mbx_floattoshort(const float* d_in, int16_t* d_out, size_t nframes, void* stream) {
    REQUIRE_CTX(c);
    if (!d_in || !d_out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_in, 8) || !aligned_to(d_out, 4)) {   // (the kernel moves two samples per lane: a float pair in, one dword out)
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_floattoshort: d_in must be 8-byte aligned and d_out 4-byte aligned");
    }
    if (nframes == 0) {
        return 0;
    }
    const size_t nsamples = nframes * 160u;
    const unsigned grid = (unsigned)((nsamples / 2 + 255) / 256);
    hipLaunchKernelGGL(mbx::floattoshort_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_in, d_out, nsamples);
    return check_launch("floattoshort_kernel");
}

// (include/mbx_llr.h)  One launch: a grid-stride over chunks of mbx::kLlrChunk LLRs (mbx_kernels.h), at most 2,048 workgroups.
int mbx_soft_from_llr(const void* d_llr, int llr_bytes, size_t count, mbe_soft_bit* d_soft, void* stream) {
    if (!d_llr || !d_soft || (llr_bytes != 1 && llr_bytes != 2)) {
        return fail(MBE_STATUS_INVALID_ARGUMENT, "mbx_soft_from_llr: d_llr and d_soft are needed, llr_bytes is 2 (int16) or 1 (int8)");
    }
    if (!aligned_to(d_llr, (uintptr_t)llr_bytes) || !aligned_to(d_soft, 2)) {
        return mbx::misaligned("mbx_soft_from_llr", "mbx_llr.h");
    }
    REQUIRE_CTX(c);
    if (count == 0) {
        return 0;
    }
    const size_t chunks = (count + mbx::kLlrChunk - 1) / mbx::kLlrChunk;
    const unsigned grid = (unsigned)(chunks < 2048 ? chunks : 2048);
    const auto kernel = llr_bytes == 2 ? mbx::soft_from_llr_kernel<2> : mbx::soft_from_llr_kernel<1>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t*>(d_llr), count, d_soft);
    return check_launch("soft_from_llr_kernel");
}

int mbx_result_histogram(const mbe_process_result* d_results, size_t n, mbx_result_hist* d_hist, void* stream) {
    static_assert(sizeof(mbx_result_hist) == mbx::kResultHistWords * sizeof(unsigned long long), "mbx_result_hist is 14 64-bit counters");
    REQUIRE_CTX(c);
    if (!d_results || !d_hist) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_results, 4) || !aligned_to(d_hist, 8)) {   // (64-bit atomic adds on the counters)
        return misaligned("mbx_result_histogram");
    }
    if (n == 0) {
        return 0;
    }
    const size_t blocks = (n + 1023) / 1024;   // four frames per thread, at most 4,096 workgroups
    hipLaunchKernelGGL(mbx::result_histogram_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, d_results, n,
                       reinterpret_cast<unsigned long long*>(d_hist));
    return check_launch("result_histogram_kernel");
}

int mbx_spectral_amp_enhance(int S, mbe_parms* d_parms, void* stream) {
    REQUIRE_CTX(c);
    if (!d_parms || S < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_parms, 4)) {
        return misaligned("mbx_spectral_amp_enhance");
    }
    if (S == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::enhance_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, S, d_parms);
    return check_launch("enhance_kernel");
}

int mbx_adaptive_smoothing(int S, mbe_parms* d_cur, const mbe_parms* d_prev, void* stream) {
    REQUIRE_CTX(c);
    if (!d_cur || !d_prev || S < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_cur, 4) || !aligned_to(d_prev, 4)) {
        return misaligned("mbx_adaptive_smoothing");
    }
    if (S == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::smoothing_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, S, d_cur, d_prev);
    return check_launch("smoothing_kernel");
}

int mbx_comfort_noise(int S, mbx_stream_rng* d_rng, float* d_pcmf, int16_t* d_pcm16, void* stream) {
    REQUIRE_CTX(c);
    if (!d_rng || S < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_rng, 8) || !aligned_to(d_pcmf, 4) || !aligned_to(d_pcm16, 2)) {
        return misaligned("mbx_comfort_noise");
    }
    if (S == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::comfort_noise_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, S, d_rng, d_pcmf,
                       d_pcm16);
    return check_launch("comfort_noise_kernel");
}

int mbx_synthesize_tone(int S, const mbx_param_record* d_records, const int32_t* d_dstar_ids, mbe_parms* d_cur, float* d_pcmf,
                        int16_t* d_pcm16, void* stream) {
    REQUIRE_CTX(c);
    if (!d_cur || S < 0 || (!d_records && !d_dstar_ids)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_records, 16) || !aligned_to(d_dstar_ids, 4) || !aligned_to(d_cur, 4) || !aligned_to(d_pcmf, 4) || !aligned_to(d_pcm16, 2)) {
        return misaligned("mbx_synthesize_tone");
    }
    if (S == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::tone_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, S, d_records, d_dstar_ids, d_cur,
                       d_pcmf, d_pcm16, c->tabs.tones_off);
    return check_launch("tone_kernel");
}

int mbx_state_copy(int S, mbe_parms* d_state, void* stream) {
    REQUIRE_CTX(c);
    if (!d_state || S < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_state, 4)) {
        return misaligned("mbx_state_copy");
    }
    if (S == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::state_copy_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, S, d_state);
    return check_launch("state_copy_kernel");
}

int mbx_ecc_words(int kind, const uint32_t* d_in, size_t n, uint32_t* d_out, int32_t* d_errs, void* stream) {
    REQUIRE_CTX(c);
    if (!d_in || !d_out || kind < 0 || kind > 2) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_in, 4) || !aligned_to(d_out, 4) || !aligned_to(d_errs, 4)) {
        return misaligned("mbx_ecc_words");
    }
    if (n == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::ecc_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kind,
                       d_in, n, d_out, d_errs, c->tabs);
    return check_launch("ecc_words_kernel");
}

#ifdef MBX_ABLATE
// development build only (make ablate -> libmbx_hip_ablate.so): timing-only stage mask for every initialised device
void mbx_debug_set_ablation(int mask) {
    for (int dev = 0; dev < kMaxDevices; ++dev) {
        g_ctx[dev].tabs.ablate = mask;
    }
}
#endif

int mbx_pack_cells(int codec, const char* d_cells, size_t n, uint8_t* d_packed, int32_t* d_status, void* stream) {
    REQUIRE_CTX(c);
    (void)c;
    if (!d_cells || !d_packed || !mbx::codec_shape(codec)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_cells, 4) || !aligned_to(d_status, 4)) {   // (the cells are read four at a time)
        return misaligned("mbx_pack_cells");
    }
    if (n == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::pack_cells_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, (hipStream_t)stream, codec, d_cells, n,
                       d_packed, d_status);
    return check_launch("pack_cells_kernel");
}

int mbx_fec_stage(int codec, int stage, const void* d_in, size_t n, uint8_t* d_frames_out, mbx_param_record* d_out, void* stream) {
    REQUIRE_CTX(c);
    if (!d_in || !mbx::codec_shape(codec)
        || !(stage == MBX_STAGE_C0 || stage == MBX_STAGE_DEMODULATE || stage == MBX_STAGE_DATA || stage == MBX_STAGE_CONVERT7100)
        || ((stage == MBX_STAGE_DATA || stage == MBX_STAGE_CONVERT7100) && !d_out)
        || ((stage == MBX_STAGE_C0 || stage == MBX_STAGE_DEMODULATE) && !d_frames_out)) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_out, 16) || (stage == MBX_STAGE_CONVERT7100 && !aligned_to(d_in, 16))) {   // (packed frames: byte loads and stores)
        return misaligned("mbx_fec_stage");
    }
    if (n == 0) {
        return 0;
    }
    hipLaunchKernelGGL(mbx::fec_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codec, stage,
                       static_cast<const uint8_t*>(d_in), n, d_frames_out, d_out, c->tabs);
    return check_launch("fec_stage_kernel");
}

int mbx_decode_parms(int codec, const mbx_param_record* d_records, size_t n, mbe_parms* d_cur, mbe_parms* d_prev, int32_t* d_rc,
                     void* stream) {
    REQUIRE_CTX(c);
    if (!d_records || !d_cur || !d_prev || !d_rc || !mbx::codec_streams(codec) || n > 0x7fffffffu) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    if (!aligned_to(d_records, 16) || !aligned_to(d_cur, 4) || !aligned_to(d_prev, 4) || !aligned_to(d_rc, 4)) {
        return misaligned("mbx_decode_parms");
    }
    if (n == 0) {
        return 0;
    }
    std::lock_guard<std::mutex> lock(c->mu);
    StreamSlot& slot = c->slots[stream];
    int rc = ensure_workspace(c, slot, n, stream);
    if (rc < 0) {
        return rc;
    }
    slot.exp_codec = -1;
    rc = launch_expand(c, codec, d_records, n, slot.workspace, stream);
    if (rc < 0) {
        return rc;
    }
    hipLaunchKernelGGL(mbx::decode_parms_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, codec, (int)n, d_records, slot.workspace,
                       d_cur, d_prev, d_rc, c->tabs);
    return check_launch("decode_parms_kernel");
}

#ifdef MBX_TESTING
// libmbx_hip_testing.so only (make testing; the tests load it through MBX_HIP_LIBRARY in a child process): fault injection for the
// fall-back path of the one-launch kernels, which no ordinary launch has ever taken.  every = 2^k > 0 makes the front blocks of chunks
// 0, 2^k, 2 * 2^k, ... do nothing, so that their stream blocks wait out their ~40 us and decode their own frames; 0 switches it off.
extern "C" int mbx_testing_set_front_skip(int every) {
    REQUIRE_CTX(c);
    if (every < 0 || (every & (every - 1)) != 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    std::lock_guard<std::mutex> lock(c->mu);
    c->tabs.front_skip = every;
    return 0;
}
#endif

// diagnostics: how many stream blocks of the one-launch kernel have expanded their own frame since the stream's workspace was
// allocated (a stream block does that when its front block's rows are not there in time); synchronises the stream.  -1: no workspace.
long long mbx_front_fallbacks(void* stream) {
    int crc;
    Context* c = current_ctx(&crc);
    if (!c) {
        return crc;
    }
    std::lock_guard<std::mutex> lock(c->mu);
    auto it = c->slots.find(stream);
    if (it == c->slots.end() || !it->second.flags) {
        return -1;
    }
    uint32_t v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess
        || hipMemcpy(&v, it->second.flags + (it->second.frames + 7) / 8, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return MBX_ENODEVICE;
    }
    return (long long)v;
}

// what ran, not what a shape predicts: the Instance::name of the last stream-stage launch issued on `stream` in the current device's
// context (a sliced launch: its slice instance), or NULL when there has been none since mbx_init
const char* mbx_last_kernel_name(void* stream) {
    int crc;
    Context* c = current_ctx(&crc);
    if (!c) {
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(c->name_mu);
    auto it = c->last_kernel.find(stream);
    return it == c->last_kernel.end() ? nullptr : it->second;
}

// 0, or the slice length in frames a launch of this shape is cut into (mbx_process_records and the batch calls on top of it)
int mbx_launch_slices(int codec, int S, int T) {
    int crc;
    return plan_of(current_ctx(&crc), predicted_step(codec, S, T)).slice_frames;   // (no context: no wave slots, 0)
}

// the dominant kernel of mbx_process_batch / _resident for a batch shape (frames 4-byte aligned, as device allocations are; a launch
// on the stream slot's own workspace that is not being captured into a graph)
const char* mbx_batch_kernel_name(int codec, int S, int T, int resident) {
    StepShape q = predicted_step(codec, S, T);
    q.kind = kFrames;
    q.aligned = true;
    q.rows_given = true;   // (a resident one-frame AMBE launch is named as on rows, also where MBX_LDS_MIN_FRAMES=1 leaves it none)
    q.resident = resident != 0;
    int crc;
    return kInstances[plan_of(resident ? nullptr : current_ctx(&crc), q).instance].name;   // (resident state is never sliced: no wave slots asked for)
}

const char* mbx_stream_kernel_name(int codec, int T) {
    StepShape q;
    q.codec = codec, q.T = T < 0 ? -T : T;
    q.resident = T < 0;    // the instances of the resident launches (mbx_process_batch_resident) with -T frames per stream ...
    q.rows_given = true;   // ... on rows from the expand launch wherever the shape has one
    return kInstances[plan_of(nullptr, q).instance].name;
}

// ---- host-buffer conveniences ------------------------------------------------------------


int mbx_fec_host(int codec, const uint8_t* frames, size_t n, mbx_param_record* records) {
    REQUIRE_CTX(c);
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!frames || !records || !sh) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const size_t fb = (size_t)sh->frame_bytes;
    DevBuf df, dr;
    HIP_TRY(df.alloc(n * fb));
    HIP_TRY(dr.alloc(n * sizeof(mbx_param_record)));
    HIP_TRY(hipMemcpy(df.p, frames, n * fb, hipMemcpyHostToDevice));
    const int rc = n == 0 ? 0 : launch_fec(c, codec, df.as<uint8_t>(), n, dr.as<mbx_param_record>(), nullptr);
    if (rc < 0) {
        return rc;
    }
    HIP_TRY(hipMemcpy(records, dr.p, n * sizeof(mbx_param_record), hipMemcpyDeviceToHost));
    return 0;
}

// `h`: a batch call whose pointers are HOST buffers (records / pcm16 / pcmf / results may be NULL: not wanted); frames in (hard: packed
// bytes, soft: mbe_soft_bit arrays), everything else as mbx_process_batch
static int process_batch_host_impl(const BatchCall& h, const void* frames, size_t frame_bytes, bool soft) {
    const int codec = h.codec, S = h.S, T = h.T;
    const size_t n = (size_t)S * (size_t)T;
    DevBuf df, ds, dg, d16, dfl, dres, drec;
    HIP_TRY(df.alloc(n * frame_bytes));
    HIP_TRY(ds.alloc((size_t)S * 3 * sizeof(mbe_parms)));
    HIP_TRY(dg.alloc((size_t)S * sizeof(mbx_stream_rng)));
    HIP_TRY(d16.alloc(n * 160 * sizeof(int16_t)));
    HIP_TRY(dfl.alloc(n * 160 * sizeof(float)));
    HIP_TRY(dres.alloc(n * sizeof(mbe_process_result)));
    HIP_TRY(drec.alloc(n * sizeof(mbx_param_record)));
    HIP_TRY(hipMemcpy(df.p, frames, n * frame_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ds.p, h.state, (size_t)S * 3 * sizeof(mbe_parms), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dg.p, h.rng, (size_t)S * sizeof(mbx_stream_rng), hipMemcpyHostToDevice));
    int rc = soft ? mbx_process_batch_soft(codec, S, T, df.as<mbe_soft_bit>(), ds.as<mbe_parms>(), dg.as<mbx_stream_rng>(),
                                           h.pcm16 ? d16.as<int16_t>() : nullptr, h.pcmf ? dfl.as<float>() : nullptr,
                                           h.results ? dres.as<mbe_process_result>() : nullptr, drec.as<mbx_param_record>(), nullptr)
                  : mbx_process_batch(codec, S, T, df.as<uint8_t>(), ds.as<mbe_parms>(), dg.as<mbx_stream_rng>(),
                                      h.pcm16 ? d16.as<int16_t>() : nullptr, h.pcmf ? dfl.as<float>() : nullptr,
                                      h.results ? dres.as<mbe_process_result>() : nullptr, drec.as<mbx_param_record>(), nullptr);
    if (rc < 0) {
        return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h.state, ds.p, (size_t)S * 3 * sizeof(mbe_parms), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h.rng, dg.p, (size_t)S * sizeof(mbx_stream_rng), hipMemcpyDeviceToHost));
    if (h.pcm16) {
        HIP_TRY(hipMemcpy(h.pcm16, d16.p, n * 160 * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    if (h.pcmf) {
        HIP_TRY(hipMemcpy(h.pcmf, dfl.p, n * 160 * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (h.results) {
        HIP_TRY(hipMemcpy(h.results, dres.p, n * sizeof(mbe_process_result), hipMemcpyDeviceToHost));
    }
    if (h.records) {
        HIP_TRY(hipMemcpy(h.records, drec.p, n * sizeof(mbx_param_record), hipMemcpyDeviceToHost));
    }
    return 0;
}

int mbx_process_batch_host(int codec, int S, int T, const uint8_t* frames, mbe_parms* state, mbx_stream_rng* rng,
                           int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    REQUIRE_CTX(c);
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!frames || !state || !rng || S < 0 || T < 0 || !sh) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    return process_batch_host_impl({codec, S, T, records, state, rng, pcm16, pcmf, results, nullptr, nullptr, nullptr}, frames,
                                   (size_t)sh->frame_bytes, false);
}

int mbx_process_batch_soft_host(int codec, int S, int T, const mbe_soft_bit* soft, mbe_parms* state, mbx_stream_rng* rng,
                                int16_t* pcm16, float* pcmf, mbe_process_result* results, mbx_param_record* records) {
    REQUIRE_CTX(c);
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!soft || !state || !rng || S < 0 || T < 0 || !sh) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const size_t cells = (size_t)sh->cells;
    int rc = mbx_validate_soft_bits(soft, (size_t)S * (size_t)T * cells);
    if (rc < 0) {
        return rc;
    }
    return process_batch_host_impl({codec, S, T, records, state, rng, pcm16, pcmf, results, nullptr, nullptr, nullptr}, soft,
                                   cells * sizeof(mbe_soft_bit), true);
}

int mbx_fec_soft_host(int codec, const mbe_soft_bit* soft, size_t n, mbx_param_record* records) {
    REQUIRE_CTX(c);
    const mbx::CodecShape* sh = mbx::codec_shape(codec);
    if (!soft || !records || !sh) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const size_t cells = (size_t)sh->cells;
    int rc = mbx_validate_soft_bits(soft, n * cells);
    if (rc < 0) {
        return rc;
    }
    DevBuf df, dr;
    HIP_TRY(df.alloc(n * cells * sizeof(mbe_soft_bit)));
    HIP_TRY(dr.alloc(n * sizeof(mbx_param_record)));
    HIP_TRY(hipMemcpy(df.p, soft, n * cells * sizeof(mbe_soft_bit), hipMemcpyHostToDevice));
    rc = mbx_fec_soft(codec, df.as<mbe_soft_bit>(), n, dr.as<mbx_param_record>(), nullptr);
    if (rc < 0) {
        return rc;
    }
    HIP_TRY(hipMemcpy(records, dr.p, n * sizeof(mbx_param_record), hipMemcpyDeviceToHost));
    return 0;
}

int mbx_ecc_soft_words_host(int kind, const mbe_soft_bit* in, size_t n, uint32_t* out, int32_t* errs) {
    REQUIRE_CTX(c);
    if (!in || !out || kind < 0 || kind > 2) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    const size_t width = kind == 0 ? 23 : 15;
    int rc = mbx_validate_soft_bits(in, n * width);
    if (rc < 0) {
        return rc;
    }
    DevBuf di, dout, de;
    HIP_TRY(di.alloc(n * width * sizeof(mbe_soft_bit) + 2));
    HIP_TRY(dout.alloc(n * sizeof(uint32_t)));
    HIP_TRY(de.alloc(n * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(di.p, in, n * width * sizeof(mbe_soft_bit), hipMemcpyHostToDevice));
    rc = mbx_ecc_soft_words(kind, di.as<mbe_soft_bit>(), n, dout.as<uint32_t>(), de.as<int32_t>(), nullptr);
    if (rc < 0) {
        return rc;
    }
    HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (errs) {
        HIP_TRY(hipMemcpy(errs, de.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

int mbx_synthesize_speech_host(int S, mbe_parms* cur, mbe_parms* prev, mbx_stream_rng* rng, float* pcmf, int16_t* pcm16) {
    REQUIRE_CTX(c);
    if (!cur || !prev || !rng || S < 0) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    DevBuf dc, dp, dg, dfl, d16;
    HIP_TRY(dc.alloc((size_t)S * sizeof(mbe_parms)));
    HIP_TRY(dp.alloc((size_t)S * sizeof(mbe_parms)));
    HIP_TRY(dg.alloc((size_t)S * sizeof(mbx_stream_rng)));
    HIP_TRY(dfl.alloc((size_t)S * 160 * sizeof(float)));
    HIP_TRY(d16.alloc((size_t)S * 160 * sizeof(int16_t)));
    HIP_TRY(hipMemcpy(dc.p, cur, (size_t)S * sizeof(mbe_parms), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dp.p, prev, (size_t)S * sizeof(mbe_parms), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dg.p, rng, (size_t)S * sizeof(mbx_stream_rng), hipMemcpyHostToDevice));
    int rc = mbx_synthesize_speech(S, dc.as<mbe_parms>(), dp.as<mbe_parms>(), dg.as<mbx_stream_rng>(),
                                   pcmf ? dfl.as<float>() : nullptr, pcm16 ? d16.as<int16_t>() : nullptr, nullptr);
    if (rc < 0) {
        return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cur, dc.p, (size_t)S * sizeof(mbe_parms), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(prev, dp.p, (size_t)S * sizeof(mbe_parms), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rng, dg.p, (size_t)S * sizeof(mbx_stream_rng), hipMemcpyDeviceToHost));
    if (pcmf) {
        HIP_TRY(hipMemcpy(pcmf, dfl.p, (size_t)S * 160 * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (pcm16) {
        HIP_TRY(hipMemcpy(pcm16, d16.p, (size_t)S * 160 * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

int mbx_floattoshort_host(const float* in, int16_t* out, size_t nframes) {
    REQUIRE_CTX(c);
    if (!in || !out) {
        return MBE_STATUS_INVALID_ARGUMENT;
    }
    DevBuf di, dout;
    HIP_TRY(di.alloc(nframes * 160 * sizeof(float)));
    HIP_TRY(dout.alloc(nframes * 160 * sizeof(int16_t)));
    HIP_TRY(hipMemcpy(di.p, in, nframes * 160 * sizeof(float), hipMemcpyHostToDevice));
    int rc = mbx_floattoshort(di.as<float>(), dout.as<int16_t>(), nframes, nullptr);
    if (rc < 0) {
        return rc;
    }
    HIP_TRY(hipMemcpy(out, dout.p, nframes * 160 * sizeof(int16_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
