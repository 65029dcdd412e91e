/*
 * mbe_neo_shards.h -- where libmbe_neo_amd.so runs the per-frame API when it has several devices (not in the reference).
 *
 * The per-frame functions are those of mbe_neo_amd.h and stay as they are; a program written against the reference header
 * needs nothing from here.  The environment variable MBX_DEVICES, read once at the library's first call, lists the SHARDS
 * the library works on:
 *
 *     MBX_DEVICES=all          one shard per device of the machine, 0 .. count-1
 *     MBX_DEVICES=0,1,2,3      the devices named, in that order; spaces around an index are allowed
 *     MBX_DEVICES=0,0,0,0      a device may be named more than once: every occurrence is a shard of its own, with its own
 *                              streams, pools and launch sets (four independent shards on one card)
 *     unset                    one shard on device $MBX_DEVICE (or 0), exactly as before there were shards
 *
 * MBX_DEVICES wins over MBX_DEVICE when both are set.  At most 32 entries.  An empty list or item, an item that is not a
 * decimal index, an index the machine does not have, or "all" on a machine without a device stops the process at the
 * first call with a message on stderr (the library has no CPU path to fall back to).
 *
 * Threads.  Host threads are numbered in the order in which they first use the library; thread number t has the HOME shard
 * t % shards.  Its synchronous calls run there: a host with one thread per channel is spread over the list.
 * Queue mode.  The k-th channel a thread creates between mbe_batchBegin and mbe_batchEnd (k = 0, 1, ...; it only goes up,
 * also across releases) is placed on shard (home + k) % shards when its first frame is queued, and stays there until it is
 * released or the batch ends.  mbe_flush() issues every shard's launches before it waits for any of them, so the devices
 * work at the same time; it returns the total over the shards, as mbe_batchPending() reports the total queued.  Everything
 * that forces a flush flushes the whole batch.  What a channel's frames decode to does not depend on its shard.
 *
 * The functions below only report.  They are the library's way to show the placement to a test or to an operator.
 * So far all of this has run on ONE card (a device named several times); see DESIGN.md, section 6.
 */
#ifndef MBE_NEO_SHARDS_H
#define MBE_NEO_SHARDS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    long long flush_passes;   /* flushes of the calling thread that launched something on this shard ... */
    long long rows;           /* ... and the frames (batch rows) they launched, both since the thread's last mbe_batchBegin */
    int channels;             /* channels of the calling thread's batch that are on this shard now */
    int resident;             /* ... of which hold their state on the device now */
} mbq_census;

int mbq_shard_count(void);                      /* entries of the list; 1 when MBX_DEVICES is unset.  Initialises the library. */
int mbq_shard_device(int shard);                /* the shard's HIP device, or -1 when there is no such shard */
int mbq_thread_home(void);                      /* the calling thread's home shard */
int mbq_channel_shard(const void* cur_mp);      /* the shard of a channel known to the calling thread's batch, else -1 */
int mbq_shard_census(int shard, mbq_census* out);   /* 0, or -1 (no such shard, out == NULL) */

#ifdef __cplusplus
}
#endif
#endif /* MBE_NEO_SHARDS_H */
