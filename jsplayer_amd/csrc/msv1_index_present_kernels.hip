// jsp_index_present: the windows of n frames of an MSVideo1 seek index on one sheet — ONE launch, no full-size picture anywhere.
//
// A workgroup (256 lanes) owns one rectangle of output pixels of one cell (blockIdx.z); index_present_device.h has the shape and
// phase 2.  Phase 1, here: a source tile of 64 x 64 pixels is 16 x 16 blocks of 4x4, a lane per block.  The tile's origin is a
// multiple of 4, so a lane's 4x4 pixels are one whole block or lie wholly in the X % 4 / Y % 4 remainder.  A block the rectangle
// reaches is composed exactly as msv1_index_show_kernel composes it into a destination that held zeros: the last frame <= t that
// coded it (index_last_writer) decoded from its code (index_decode), else the block of `before`, else zeros; remainder pixels come
// from `before`, or are zero.  The 16 pixels go to LDS as four 16-byte rows — px[] is only ever indexed by constants.
//
// jsp_index_tensor (msv1_index_tensor_kernel) is the same kernel with another last step: the lane's finished words go out as elements of
// a dense N x 3 x H x W or N x H x W x 3 tensor (store_elements) and not as words of a sheet.
#include <type_traits>

#include "index_present_device.h"
#include "msv1_block_io.h"

namespace jsp {
namespace {

using namespace ipresent;

struct Msv1PresentSrc {
    const Msv1IndexChunk* chunks;
    const uint32_t* frame_chunk;
    const int32_t* palette;
    const uint32_t* bitmap;
    const int32_t* frames;     // the frame of every cell
    const uint32_t* before;    // the picture before the index, or null
    size_t pitch;              // table entries per frame (nblocks)
    int nblocks, nbx, nby;
    int before_vec;            // blocks of `before` may be read 16 bytes a row
};

// Phase 1 of both kernels below: compose (index_present_device.h) for a tile of 16 x 16 blocks, a lane per block.
template <int BITS>
struct Msv1Compose {
    const Msv1PresentSrc& s;
    uint32_t* tile;
    const uint32_t* s_pal;
    int t, X, Y;           // the cell's frame; the picture's size
    __device__ __forceinline__ void operator()(int tx0, int ty0, int sx0, int sy0, int sx1, int sy1) const {
        const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
        const int x = tx0 + lx * 4, y = ty0 + ly * 4;                  // the lane's 4x4 pixels
        if (x > sx1 || x + 3 < sx0 || y > sy1 || y + 3 < sy0) return;  // (what is left lies inside the picture at least in part)
        const int bx = x >> 2, by = y >> 2;
        uint32_t px[16];
        if (bx < s.nbx && by < s.nby) {
            const int blk = by * s.nbx + bx;
            int w;
            const uint32_t m = index_last_writer(s.bitmap, s.nblocks, blk, t, w);
            if (m != 0u) {
                index_decode<BITS>(s.chunks, s.frame_chunk, s.pitch, 32 * w + 31 - __builtin_clz(m), blk, s_pal, px);
            } else if (s.before != nullptr) {
                const uint32_t* p = s.before + (size_t)y * (size_t)X + (size_t)x;
                if (s.before_vec) load_block<true>(p, X, px);
                else load_block<false>(p, X, px);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) px[i] = 0u;
            }
        } else {   // pixels no block covers
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int xx = x + (i & 3), yy = y + (i >> 2);
                px[i] = (s.before != nullptr && xx < X && yy < Y) ? *(cgu32*)(s.before + (size_t)yy * (size_t)X + (size_t)xx) : 0u;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<uint4*>(tile + (ly * 4 + r) * T + lx * 4) = make_uint4(px[r * 4], px[r * 4 + 1], px[r * 4 + 2], px[r * 4 + 3]);
    }
};

template <int BITS, int MODE, int FILTER, bool WIDE>
__global__ __launch_bounds__(kIndexPresentWG) void msv1_index_present_kernel(const Msv1PresentSrc s, const IndexPresentArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[T * T];
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS, false>(s_pal, s.palette);   // (present_words has a barrier before the first decode)
    const Msv1Compose<BITS> compose{s, tile, s_pal, s.frames[blockIdx.z], a.fw, a.fh};
    present_rect<MODE, FILTER, WIDE, 4>(a, sheet_cell(a), tile, compose);
}

// jsp_index_tensor: the same rectangle, its words stored as elements of a dense tensor.  MODE is one of the two canvas conversions.
template <int BITS, int MODE, int FILTER, bool WIDE>
__global__ __launch_bounds__(kIndexPresentWG) void msv1_index_tensor_kernel(const Msv1PresentSrc s, const IndexPresentArgs a, const IndexTensorArgs t) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[T * T];
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS, false>(s_pal, s.palette);
    const Msv1Compose<BITS> compose{s, tile, s_pal, s.frames[blockIdx.z], a.fw, a.fh};
    PresentLane l;
    if (present_words<MODE, FILTER, WIDE, 4>(a, tile, compose, l)) store_elements(a, t, l);
}

Msv1PresentSrc present_src(const Msv1Geometry& geo, const Msv1IndexChunk* d_chunks, const uint32_t* d_frame_chunk, const int32_t* d_palette,
                           const uint32_t* d_bitmap, const int32_t* d_frames, const int32_t* before) {
    Msv1PresentSrc s;
    s.chunks = d_chunks;
    s.frame_chunk = d_frame_chunk;
    s.palette = d_palette;
    s.bitmap = d_bitmap;
    s.frames = d_frames;
    s.before = reinterpret_cast<const uint32_t*>(before);
    s.pitch = (size_t)std::max(geo.nblocks, 1);
    s.nblocks = std::max(geo.nblocks, 0);
    s.nbx = std::max(geo.nbx, 0);
    s.nby = std::max(geo.nby, 0);
    s.before_vec = (geo.X & 3) == 0 && !(reinterpret_cast<uintptr_t>(before) & 15);
    return s;
}

}  // namespace

void msv1_launch_index_present(const Msv1Geometry& geo, const Msv1IndexChunk* d_chunks, const uint32_t* d_frame_chunk, const int32_t* d_palette,
                               const uint32_t* d_bitmap, const int32_t* d_frames, int n, const int32_t* before, const IndexPresentArgs& a, int mode,
                               int filter, hipStream_t stream) {
    const Msv1PresentSrc s = present_src(geo, d_chunks, d_frame_chunk, d_palette, d_bitmap, d_frames, before);
    const dim3 grid = present_grid(a, n);
    auto go = [&](auto B) {
        dispatch_mode(mode, [&](auto M) {
            dispatch_filter(filter, a.step, [&](auto F, auto W) {
                hipLaunchKernelGGL((msv1_index_present_kernel<decltype(B)::value, decltype(M)::value, decltype(F)::value, decltype(W)::value>), grid,
                                   dim3(kIndexPresentWG), 0, stream, s, a);
            });
        });
    };
    if (geo.bits == 16) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, 8>{});
}

void msv1_launch_index_tensor(const Msv1Geometry& geo, const Msv1IndexChunk* d_chunks, const uint32_t* d_frame_chunk, const int32_t* d_palette,
                              const uint32_t* d_bitmap, const int32_t* d_frames, int n, const int32_t* before, const IndexPresentArgs& a,
                              const IndexTensorArgs& t, int mode, int filter, hipStream_t stream) {
    const Msv1PresentSrc s = present_src(geo, d_chunks, d_frame_chunk, d_palette, d_bitmap, d_frames, before);
    const dim3 grid = present_grid(a, n);
    auto go = [&](auto B) {
        dispatch_canvas_mode(mode, [&](auto M) {
            dispatch_filter(filter, a.step, [&](auto F, auto W) {
                hipLaunchKernelGGL((msv1_index_tensor_kernel<decltype(B)::value, decltype(M)::value, decltype(F)::value, decltype(W)::value>), grid,
                                   dim3(kIndexPresentWG), 0, stream, s, a, t);
            });
        });
    };
    if (geo.bits == 16) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, 8>{});
}

}  // namespace jsp
