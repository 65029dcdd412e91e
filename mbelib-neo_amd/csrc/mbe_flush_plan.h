// mbe_flush_plan.h -- where everything of a queue-mode flush (mbe_shim.cpp, flush_batch) goes: which channels launch together, which
// batch row and which bytes of the frame array every queued frame gets, and the index, offset and codec arrays of the launches.
// Integer work on the host alone: no HIP, no allocation once its vectors have grown -- so that a CPU program can check it under a
// sanitizer (tests/flush_plan_check.cpp states every property).  Private to the shim; nothing here is exported.
//
// GROUPS.  The channels with frames pending are grouped by (codec, input form, pending count): one group is one rectangular batch of
// nch channels x T frames.  Groups stand in the order of the first channel that has their key, then all hard-input groups before all
// soft-input ones (stable); the channels of a group in ascending channel index.
// FORMS.  Input form f (0 hard, 1 soft) owns groups [form_g0[f], form_g0[f + 1]).  A form with ONE group keeps the group's own
// launcher and frames of the codec's own size; a form with SEVERAL is mixed: one ragged launch set over all its channels, its frames
// rows of one size (the largest codec's), its rows one array.
// ROWS AND BYTES.  Batch rows run through the groups in order; so do the bytes of the frame array, rounded up to 16 where a launch's
// frames end (after every unmixed group, after the last group of a mixed form).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "mbx_codec.h"
#include "mbx_types.h"

namespace mbx {

// one frame as the batch launchers take it: packed wire bytes, or the reference's array of soft cells
inline size_t flush_input_bytes(int codec, bool soft) {
    return soft ? (size_t)kCodecs[codec].cells * sizeof(mbe_soft_bit) : (size_t)kCodecs[codec].frame_bytes;
}

struct FlushGroup {
    int    codec, T;      // T: frames pending on each of its channels
    bool   soft;
    size_t nch;           // channels
    size_t row0;          // first batch row
    size_t byte0;         // where its frames start in the frame array
    size_t stride;        // bytes from one frame to the next
    size_t index0;        // its channels are FlushPlan::channels[index0, index0 + nch)
};

struct __attribute__((visibility("hidden"))) FlushPlan {   // (hidden: no symbol named after the plan among the shim's exports)
    std::vector<FlushGroup> groups;
    size_t form_g0[3] = {0, 0, 0};
    bool   form_mixed[2] = {false, false};
    size_t rows = 0, bytes = 0;
    std::vector<int32_t>  channels;    // the channels with frames pending, in group order (the launches' stream index, once mapped to pool slots)
    std::vector<uint32_t> group_of;    // [channel] its group (channels with nothing pending: unspecified)
    std::vector<uint32_t> row_of;      // [queue entry] its batch row: row0 + position of its channel in the group * T + earlier entries of the channel
    std::vector<uint32_t> by_row;      // [batch row] its queue entry: filled by invert_rows(), not by build()
    // mixed forms: first row of every channel relative to the form's first row (channels + 1 entries, the last = the form's rows) and
    // every channel's codec, in the order of `channels`; form f's start at offsets[off_at[f]] and codecs[codec_at[f]]
    std::vector<int32_t>  offsets;
    std::vector<uint8_t>  codecs;
    size_t off_at[2] = {0, 0}, codec_at[2] = {0, 0};

    bool any_mixed() const { return form_mixed[0] || form_mixed[1]; }
    // channels and rows of form f (what a mixed launch set covers)
    size_t form_channels(int f) const {
        return form_g0[f] == form_g0[f + 1] ? 0 : groups[form_g0[f + 1] - 1].index0 + groups[form_g0[f + 1] - 1].nch - groups[form_g0[f]].index0;
    }
    size_t form_rows(int f) const {
        const size_t end = form_g0[f + 1] < groups.size() ? groups[form_g0[f + 1]].row0 : rows;
        return form_g0[f] == form_g0[f + 1] ? 0 : end - groups[form_g0[f]].row0;
    }
    // where the frame of queue entry e (of channel c) goes in the frame array
    size_t byte_of(size_t e, int c) const {
        const FlushGroup& g = groups[group_of[(size_t)c]];
        return g.byte0 + (row_of[e] - g.row0) * g.stride;
    }

    // Channel: anything with .codec, .soft, .pending; Entry: anything with .channel -- the queue's entries in call order, .pending of
    // them for every channel.
    template <class Channel, class Entry>
    void build(const Channel* ch, size_t total, const Entry* q, size_t n) {
        find_groups(ch, total);
        lay_out();
        place(ch, total, q, n);
    }

    // by_row from row_of.  Apart from build(): only the scatter reads it, so the flush fills it while the device works.
    void invert_rows() {
        by_row.resize(rows);
        for (size_t e = 0; e < row_of.size(); ++e) {
            by_row[row_of[e]] = (uint32_t)e;
        }
    }

private:
    // scratch of build(), kept for its capacity
    std::vector<FlushGroup> sorted_;
    std::vector<uint32_t>   first_, seen_, remap_;   // [channel] position in its group, entries met so far; [group] its place after the sort
    // [codec * 2 + soft][pending] -> group, all -1 outside build(): the key of a group looked up without hashing.  A table grows to the
    // largest pending count its (codec, form) has ever had in this thread and stays: 4 bytes per count, where every queued frame
    // already costs an entry of ~50 bytes -- nothing at realistic counts, but a channel that once queued a million frames leaves 4 MB.
    std::vector<int32_t>    key_[8];

    // the groups, in order of the first channel with their key, then hard before soft; group_of and first_ of every pending channel
    template <class Channel>
    void find_groups(const Channel* ch, size_t total) {
        groups.clear();
        sorted_.clear();
        group_of.assign(total, 0);
        first_.assign(total, 0);
        for (size_t c = 0; c < total; ++c) {
            if (ch[c].pending == 0) {
                continue;
            }
            std::vector<int32_t>& table = key_[(size_t)ch[c].codec * 2 + (ch[c].soft ? 1 : 0)];
            if (table.size() <= (size_t)ch[c].pending) {
                table.resize((size_t)ch[c].pending + 1, -1);
            }
            int32_t& gi = table[(size_t)ch[c].pending];
            if (gi < 0) {
                gi = (int32_t)groups.size();
                groups.push_back(FlushGroup{ch[c].codec, ch[c].pending, ch[c].soft, 0, 0, 0, 0, 0});
            }
            group_of[c] = (uint32_t)gi;
            first_[c] = (uint32_t)groups[(size_t)gi].nch++;
        }
        remap_.assign(groups.size(), 0);
        for (int soft = 0; soft < 2; ++soft) {
            for (size_t gi = 0; gi < groups.size(); ++gi) {
                if (groups[gi].soft == (soft != 0)) {
                    remap_[gi] = (uint32_t)sorted_.size();
                    sorted_.push_back(groups[gi]);
                }
            }
            form_g0[soft + 1] = sorted_.size();
        }
        for (const FlushGroup& g : groups) {   // the tables go back to all -1 for the next flush
            key_[(size_t)g.codec * 2 + (g.soft ? 1 : 0)][(size_t)g.T] = -1;
        }
        groups.swap(sorted_);
        for (size_t c = 0; c < total; ++c) {
            if (ch[c].pending) {
                group_of[c] = remap_[group_of[c]];
            }
        }
        form_mixed[0] = form_g0[1] - form_g0[0] > 1;
        form_mixed[1] = form_g0[2] - form_g0[1] > 1;
    }

    // rows, bytes and index entries of every group
    void lay_out() {
        rows = bytes = 0;
        size_t at = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            FlushGroup& g = groups[gi];
            g.row0 = rows;
            g.byte0 = bytes;
            g.index0 = at;
            g.stride = !form_mixed[g.soft] ? flush_input_bytes(g.codec, g.soft)
                                           : (g.soft ? MBX_IMBE_SOFT_BITS * sizeof(mbe_soft_bit) : (size_t)MBX_IMBE_FRAME_BYTES);
            at += g.nch;
            rows += g.nch * (size_t)g.T;
            bytes += g.nch * (size_t)g.T * g.stride;
            if (!form_mixed[g.soft] || gi + 1 == form_g0[g.soft + 1]) {   // (the rows of a mixed form are one array)
                bytes = (bytes + 15u) & ~(size_t)15u;                     // frame arrays start 16-byte aligned
            }
        }
        channels.resize(at);
    }

    // every channel into the index list, every queue entry onto its row, the offsets and codecs of the mixed forms
    template <class Channel, class Entry>
    void place(const Channel* ch, size_t total, const Entry* q, size_t n) {
        for (size_t c = 0; c < total; ++c) {
            if (ch[c].pending) {
                channels[groups[group_of[c]].index0 + first_[c]] = (int32_t)c;
            }
        }
        seen_.assign(total, 0);
        row_of.resize(n);
        for (size_t e = 0; e < n; ++e) {
            const size_t c = (size_t)q[e].channel;
            const FlushGroup& g = groups[group_of[c]];
            row_of[e] = (uint32_t)(g.row0 + (size_t)first_[c] * (size_t)g.T + seen_[c]++);
        }
        offsets.clear();
        codecs.clear();
        for (int f = 0; f < 2; ++f) {
            off_at[f] = offsets.size();
            codec_at[f] = codecs.size();
            if (!form_mixed[f]) {
                continue;
            }
            int32_t row = 0;
            for (size_t gi = form_g0[f]; gi < form_g0[f + 1]; ++gi) {
                for (size_t k = 0; k < groups[gi].nch; ++k) {
                    offsets.push_back(row);
                    codecs.push_back((uint8_t)groups[gi].codec);
                    row += groups[gi].T;
                }
            }
            offsets.push_back(row);
        }
    }
};

}  // namespace mbx
