// mbx_codec.h -- what a codec IS on the host side, declared once: the shape of its frame in every form the launchers and the
// mbe_* shim handle it in (the reference's cell array, the packed wire frame, the parameter bits), and which codec's FEC front end
// and stream stage its frames go through.  Host-only and private: included by mbx_api.hip, mbx_session.hip, mbx_burst.hip and mbe_shim.cpp, each
// of which compiles its own copy of these constants; nothing here is exported.  (The kernels of mbx_fec.hip unpack the same rows
// with widths of their own: device code does not read this table.)
// A new codec, or a change to a frame form: its row here, its row in kCodecKernels (mbx_api.hip), its case in the shim's
// pack_one / fec_one.
#pragma once

#include "mbx_types.h"

namespace mbx {

struct CodecShape {
    int rows, stride, cells;   // the reference's frame array: char / mbe_soft_bit [rows][stride], cells = rows * stride
    int width[8];              // cells of each row that are on the wire: row r is sent from cell width[r]-1 down to cell 0
    int frame_bytes;           // the packed wire frame
    int data_bits;             // parameter bits after FEC (imbe_d / ambe_d)
    int front;                 // the codec whose FEC front end a frame takes ...
    int stream;                // ... and the codec whose stream stage follows it (the records are then in that codec's order)
};

constexpr CodecShape kAmbe3600x2450 = {4, 24, MBX_AMBE_SOFT_BITS, {24, 23, 11, 14}, MBX_AMBE_FRAME_BYTES, 49,
                                       MBX_CODEC_AMBE3600X2450, MBX_CODEC_AMBE3600X2450};
// D-STAR: the frame and the FEC front end of 3600x2450, a parameter decode and frame policy of its own
constexpr CodecShape with_stream(CodecShape s, int stream) {
    s.stream = stream;
    return s;
}

constexpr CodecShape kCodecs[4] = {   // indexed by MBX_CODEC_*
    {8, 23, MBX_IMBE_SOFT_BITS, {23, 23, 23, 23, 15, 15, 15, 7}, MBX_IMBE_FRAME_BYTES, 88, MBX_CODEC_IMBE7200X4400, MBX_CODEC_IMBE7200X4400},
    kAmbe3600x2450,
    // own FEC / demodulation front end; what it hands on is a 7200x4400 record
    {7, 24, MBX_IMBE7100_SOFT_BITS, {19, 24, 23, 23, 15, 15, 23}, MBX_IMBE7100_FRAME_BYTES, 88, MBX_CODEC_IMBE7100X4400, MBX_CODEC_IMBE7200X4400},
    with_stream(kAmbe3600x2450, MBX_CODEC_AMBE3600X2400),
};
static_assert(MBX_CODEC_IMBE7200X4400 == 0 && MBX_CODEC_AMBE3600X2450 == 1 && MBX_CODEC_IMBE7100X4400 == 2 && MBX_CODEC_AMBE3600X2400 == 3,
              "kCodecs is indexed by MBX_CODEC_*");

// the codec's row, or nullptr: no such codec
inline const CodecShape* codec_shape(int codec) {
    return (codec >= 0 && codec < (int)(sizeof(kCodecs) / sizeof(kCodecs[0]))) ? &kCodecs[codec] : nullptr;
}

// a codec with a stream stage of its own: what the records-based entry points take
inline bool codec_streams(int codec) {
    const CodecShape* sh = codec_shape(codec);
    return sh && sh->stream == codec;
}

}  // namespace mbx
