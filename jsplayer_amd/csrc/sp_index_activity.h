// The launchers of the ScreenPressor seek index's activity map (sp_index_activity_kernels.hip) and distance map
// (sp_index_distance_kernels.hip), called from sp_index.cpp.
#pragma once
#include "sp.h"

namespace jsp::sp {

// Activity map of the seek index (sp_index_activity_kernel): out[(k * nby + by) * nbx + bx], k < n, = the pixels of block (bx, by),
// clipped to the picture, that differ between the pictures launch_index_show would write for frames first + k and first + k - 1 (the
// picture before frame 0: zeros) — ONE launch, launch_index_play's walk with a compare-and-count where it has a store.  Only non-zero
// counts are stored: the caller zeroes `out` first.  d_frames and d_keymask are launch_index_play's.
void launch_index_activity(const Geometry& g, uint16_t* out, int first, int n, const int32_t* d_keys, size_t pic_stride,
                           const IndexPlayFrame* d_frames, const uint32_t* d_keymask, const PBlock* d_blocks, const uint32_t* d_payload,
                           const uint32_t* d_bitmap, hipStream_t stream);

// Distance map of the seek index (sp_index_distance_kernel, sp_index_distance_kernels.hip): out[(k * nby + by) * nbx + bx], k < n, = the
// pixels of block (bx, by), clipped to the picture, that differ between the picture launch_index_show would write for frame first + k
// and the reference R — the picture of frame ref_frame (-1: zeros) when ref_picture is null, else the device picture ref_picture of
// X * Y words (4-byte aligned, only read; ref_frame is not looked at) — ONE launch.  EVERY element is stored: the caller zeroes
// nothing.  d_frames and d_keymask are launch_index_play's.
void launch_index_distance(const Geometry& g, uint16_t* out, int ref_frame, const int32_t* ref_picture, int first, int n, const int32_t* d_keys,
                           size_t pic_stride, const IndexPlayFrame* d_frames, const uint32_t* d_keymask, const PBlock* d_blocks,
                           const uint32_t* d_payload, const uint32_t* d_bitmap, hipStream_t stream);

}  // namespace jsp::sp
