// jsp_seek for MSVideo1 (msv1_seek.cpp, msv1_seek_kernels.hip): what the seek needs from a staged batch, and its kernel launcher.
#pragma once
#include "msv1.h"

struct jsp_staged;

namespace jsp {

// What a staged batch holds for the seek kernel: its stream buffer, block tables and frame records in HBM.
struct Msv1SeekView {
    Msv1Geometry geo{};
    const uint8_t* d_stream = nullptr;
    const uint32_t* d_desc = nullptr;       // frame f's table at f * desc_pitch
    size_t desc_pitch = 0;
    const Msv1FrameArgs* d_frames = nullptr;
    const Msv1FrameArgs* h_frames = nullptr;
    const int32_t* d_palette = nullptr;
    uint32_t* d_signif = nullptr;           // one word per frame (device) ...
    uint32_t* h_signif = nullptr;           // ... and its pinned host copy
    int nframes = 0;
};
// False when `st` is not a batch of the MSVideo1 staging (msv1_codec.cpp).
bool msv1_seek_view(jsp_staged* st, Msv1SeekView& out);
// ONE launch writes `dst` as frames [0, v.nframes) of the batch leave it when each frame's destination starts out holding the picture
// before it: every block from the last frame that coded it, else from `base` (the picture before the batch; null: left as it is);
// the pixels no block covers from `base` as well.  cmp_row_lo != ~0u: the stage-2 compare of the last frame (its coded blocks against
// the picture before it, rows >= cmp_row_lo) ORs v.d_signif[v.nframes - 1].
void msv1_launch_seek(const Msv1SeekView& v, int32_t* dst, const int32_t* base, uint32_t cmp_row_lo, hipStream_t stream);

}  // namespace jsp
