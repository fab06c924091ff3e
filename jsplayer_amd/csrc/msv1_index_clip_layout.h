// The parts of the scratch of the clip calls of an MSVideo1 seek index (clip_frames, msv1_seek.cpp; Msv1ClipScratch, msv1_seek.h) for
// a slice of pairs.  Plain C++, no HIP, so that a program of its own can run it under a sanitizer.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jsp {

// What a call's scratch holds besides the parts every call has.
enum ClipForm {
    CLIP_GRID = 0,   // jsp_index_delta_frames, _tight_frames: no code counts
    CLIP_RECT = 1,   // jsp_index_crop_frames, _path_frames: code counts
    CLIP_PAN = 2     // jsp_index_pan_frames: code counts, and the pairs' origins in front
};

// The parts for slices of S pairs of frames of nb blocks (nwg workgroups, `bound` bytes a frame), laid end to end, each 16-byte
// aligned; a part a form does not have is empty.  The host's pinned side has the parts before status_at (what goes up), status, totals
// and counts (what comes back) at the same offsets, and is host_bytes long: its last 16 bytes take a refused block's writer frame.
struct ClipLayout {
    size_t origins_at, pairs_at, bases_at, status_at, totals_at, counts_at, first_at, records_at, out_at, bytes, host_bytes;
};
inline ClipLayout clip_layout(ClipForm form, size_t S, size_t nb, size_t nwg, size_t bound) {
    const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    ClipLayout l{};
    l.origins_at = 0;
    l.pairs_at = l.origins_at + (form == CLIP_PAN ? up16(4 * sizeof(int32_t) * S) : 0);
    l.bases_at = l.pairs_at + up16(2 * sizeof(int32_t) * S);
    l.status_at = l.bases_at + up16(sizeof(uint64_t) * S);
    l.totals_at = l.status_at + up16(sizeof(uint32_t) * S);
    l.counts_at = l.totals_at + up16(sizeof(uint32_t) * S * nwg);
    l.first_at = l.counts_at + (form == CLIP_GRID ? 0 : up16(sizeof(uint32_t) * S * nwg));
    l.records_at = l.first_at + up16(sizeof(uint32_t) * S * nwg);
    l.out_at = l.records_at + up16(2 * sizeof(uint32_t) * S * nb);
    l.bytes = l.out_at + S * bound;
    l.host_bytes = (form == CLIP_GRID ? l.first_at : l.records_at) + 16;
    return l;
}

}  // namespace jsp
