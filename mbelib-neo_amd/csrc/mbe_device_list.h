// mbe_device_list.h -- which devices the per-frame library (mbe_shim.cpp) runs on, and where a thread and a queued channel go.
// MBX_DEVICES is a list of SHARDS: every entry is a HIP device index and a shard of its own -- streams, pools and launch sets --, so a
// device named twice carries two independent shards.  Text and integer work on the host alone: no HIP, no globals, no getenv -- the
// caller reads the environment and asks the runtime for the device count --, so that a CPU program can check it under a sanitizer
// (tests/device_list_check.cpp states every property).  Private to the shim; nothing here is exported.
#pragma once

namespace mbx {

constexpr int kMaxShards = 32;

struct DeviceList {
    int n = 0;                  // shards
    int device[kMaxShards];     // [shard] its HIP device
};

// text: the value of MBX_DEVICES, NULL when it is unset; device_count: what the runtime reports; fallback_device: MBX_DEVICE, or 0.
//   unset          one shard on fallback_device (not held against device_count: the device is refused where it is first used)
//   "all"          0 .. device_count - 1
//   "a,b,..."      decimal indices, spaces around an item allowed, repeats allowed: every occurrence is a shard
// false: refused, *out untouched and *why the reason (a string literal; one of its own per rule).
inline bool parse_device_list(const char* text, int device_count, int fallback_device, DeviceList* out, const char** why) {
    DeviceList list;
    const char* none = nullptr;
    const char*& reason = why ? *why : none;
    reason = nullptr;
    auto space = [](char c) { return c == ' ' || c == '\t'; };
    if (!text) {
        list.n = 1;
        list.device[0] = fallback_device;
        *out = list;
        return true;
    }
    const char* p = text;
    while (space(*p)) {
        ++p;
    }
    if (*p == '\0') {
        reason = "MBX_DEVICES is empty";
        return false;
    }
    if (p[0] == 'a' && p[1] == 'l' && p[2] == 'l') {
        const char* q = p + 3;
        while (space(*q)) {
            ++q;
        }
        if (*q == '\0') {
            if (device_count <= 0) {
                reason = "MBX_DEVICES=all, but the runtime reports no device";
                return false;
            }
            if (device_count > kMaxShards) {
                reason = "MBX_DEVICES has more than 32 entries";
                return false;
            }
            list.n = device_count;
            for (int d = 0; d < device_count; ++d) {
                list.device[d] = d;
            }
            *out = list;
            return true;
        }
    }
    for (;;) {   // one item per turn; p stands at its first character
        while (space(*p)) {
            ++p;
        }
        if (*p == ',' || *p == '\0') {
            reason = "MBX_DEVICES has an empty item";
            return false;
        }
        long value = 0;
        bool beyond = false;
        while (*p >= '0' && *p <= '9') {
            value = value * 10 + (*p - '0');
            if (value >= device_count) {   // (also keeps a long run of digits from overflowing)
                beyond = true;
                value = 0;
            }
            ++p;
        }
        while (space(*p)) {
            ++p;
        }
        if (*p != ',' && *p != '\0') {
            reason = "MBX_DEVICES has an item that is not a decimal device index";
            return false;
        }
        if (beyond || device_count <= 0) {
            reason = "MBX_DEVICES names a device index the runtime does not have";
            return false;
        }
        if (list.n == kMaxShards) {
            reason = "MBX_DEVICES has more than 32 entries";
            return false;
        }
        list.device[list.n++] = (int)value;
        if (*p == '\0') {
            break;
        }
        ++p;
    }
    *out = list;
    return true;
}

// Threads are numbered as they first use the library; a thread's HOME shard carries its synchronous calls and the first channel of
// each of its batches.
inline int home_shard(int thread_ordinal, int n) { return thread_ordinal % n; }
// The k-th channel a thread creates in a batch (k counts up from 0 at mbe_batchBegin and never down, also across releases).
inline int channel_shard(int home, int k, int n) { return (home + k) % n; }

}  // namespace mbx
