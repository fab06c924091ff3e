// jsp_index_present: the windows of n frames of an MSVideo1 seek index on one sheet — ONE launch, no full-size picture anywhere.
//
// A workgroup (256 lanes) owns one rectangle of output pixels of one cell (blockIdx.z); index_present_device.h has the shape and
// phase 2.  Phase 1, here: a source tile of 64 x 64 pixels is 16 x 16 blocks of 4x4, a lane per block.  The tile's origin is a
// multiple of 4, so a lane's 4x4 pixels are one whole block or lie wholly in the X % 4 / Y % 4 remainder.  A block the rectangle
// reaches is composed exactly as msv1_index_show_kernel composes it into a destination that held zeros: by index_block
// (msv1_block_io.h), an undefined block being zeros; remainder pixels come from `before`, or are zero.  The 16 pixels go to LDS as four 16-byte rows — px[] is only ever indexed by constants.
//
// jsp_index_tensor (msv1_index_tensor_kernel) is the same kernel with another last step: the lane's finished words go out as elements of
// a dense N x 3 x H x W or N x H x W x 3 tensor (store_elements) and not as words of a sheet.
#include <type_traits>

#include "index_present_device.h"
#include "msv1_block_io.h"

namespace jsp {
namespace {

using namespace ipresent;

// Phase 1 of both kernels below: compose (index_present_device.h) for a tile of 16 x 16 blocks, a lane per block.
template <int BITS>
struct Msv1Compose {
    const Msv1IndexSrc& s;
    uint32_t* tile;
    const uint32_t* s_pal;
    int t;                 // the cell's frame
    __device__ __forceinline__ void operator()(int tx0, int ty0, int sx0, int sy0, int sx1, int sy1) const {
        const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
        const int x = tx0 + lx * 4, y = ty0 + ly * 4;                  // the lane's 4x4 pixels
        if (x > sx1 || x + 3 < sx0 || y > sy1 || y + 3 < sy0) return;  // (what is left lies inside the picture at least in part)
        const int bx = x >> 2, by = y >> 2;
        uint32_t px[16];
        if (bx < s.nbx && by < s.nby) {
            index_block<BITS>(s, t, by * s.nbx + bx, bx, by, s.before_vec != 0, s_pal, px);
        } else {   // pixels no block covers
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int xx = x + (i & 3), yy = y + (i >> 2);
                px[i] = (s.before != nullptr && xx < s.X && yy < s.Y) ? *(cgu32*)(s.before + (size_t)yy * (size_t)s.X + (size_t)xx) : 0u;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<uint4*>(tile + (ly * 4 + r) * T + lx * 4) = make_uint4(px[r * 4], px[r * 4 + 1], px[r * 4 + 2], px[r * 4 + 3]);
    }
};

// (frames: the frame of every cell)
template <int BITS, int MODE, int FILTER, bool WIDE>
__global__ __launch_bounds__(kIndexPresentWG) void msv1_index_present_kernel(const Msv1IndexSrc s, const int32_t* __restrict__ frames,
                                                                             const IndexPresentArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[T * T];
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS, false>(s_pal, s.palette);   // (present_words has a barrier before the first decode)
    const Msv1Compose<BITS> compose{s, tile, s_pal, frames[blockIdx.z]};
    present_rect<MODE, FILTER, WIDE, 4>(a, sheet_cell(a), tile, compose);
}

// jsp_index_tensor: the same rectangle, its words stored as elements of a dense tensor.  MODE is one of the two canvas conversions.
template <int BITS, int MODE, int FILTER, bool WIDE>
__global__ __launch_bounds__(kIndexPresentWG) void msv1_index_tensor_kernel(const Msv1IndexSrc s, const int32_t* __restrict__ frames,
                                                                            const IndexPresentArgs a, const IndexTensorArgs t) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[T * T];
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS, false>(s_pal, s.palette);
    const Msv1Compose<BITS> compose{s, tile, s_pal, frames[blockIdx.z]};
    PresentLane l;
    if (present_words<MODE, FILTER, WIDE, 4>(a, tile, compose, l)) store_elements(a, t, l);
}

// f(std::integral_constant<int, BITS>{}) for the index's bit depth (16, else 8)
template <class F>
void dispatch_bits(int bits, F&& f) {
    if (bits == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 8>{});
}

}  // namespace

void msv1_launch_index_present(const Msv1IndexSrc& src, const int32_t* d_frames, int n, const IndexPresentArgs& a, int mode, int filter,
                               hipStream_t stream) {
    const dim3 grid = present_grid(a, n);
    dispatch_bits(src.bits, [&](auto B) {
        dispatch_mode(mode, [&](auto M) {
            dispatch_filter(filter, a.step, [&](auto F, auto W) {
                hipLaunchKernelGGL((msv1_index_present_kernel<decltype(B)::value, decltype(M)::value, decltype(F)::value, decltype(W)::value>), grid,
                                   dim3(kIndexPresentWG), 0, stream, src, d_frames, a);
            });
        });
    });
}

void msv1_launch_index_tensor(const Msv1IndexSrc& src, const int32_t* d_frames, int n, const IndexPresentArgs& a, const IndexTensorArgs& t,
                              int mode, int filter, hipStream_t stream) {
    const dim3 grid = present_grid(a, n);
    dispatch_bits(src.bits, [&](auto B) {
        dispatch_canvas_mode(mode, [&](auto M) {
            dispatch_filter(filter, a.step, [&](auto F, auto W) {
                hipLaunchKernelGGL((msv1_index_tensor_kernel<decltype(B)::value, decltype(M)::value, decltype(F)::value, decltype(W)::value>), grid,
                                   dim3(kIndexPresentWG), 0, stream, src, d_frames, a, t);
            });
        });
    });
}

}  // namespace jsp
