// jsp_sp_index_present: the windows of n frames of a ScreenPressor seek index on one sheet — ONE launch, no full-size picture anywhere.
//
// A workgroup (256 lanes) owns one rectangle of output pixels of one cell (blockIdx.z); index_present_device.h has the shape and
// phase 2.  Phase 1, here: a source tile of 64 x 64 pixels is 4 x 4 blocks of 16x16 (its origin is a multiple of 16), a WAVE per
// block as in sp_index_show_kernel — the four waves take the four blocks of a block row of the tile side by side, four rows in turn.
// A block the rectangle reaches is composed by index_compose (sp_index_compose.h), exactly what the show kernel stores, and goes to
// LDS as one 16-byte chunk per lane.  Whether a block is composed is wave-uniform, as index_compose needs it.
//
// jsp_sp_index_tensor (sp_index_tensor_kernel) is the same kernel with another last step: the lane's finished words go out as elements
// of a dense N x 3 x H x W or N x H x W x 3 tensor (store_elements) and not as words of a sheet.
#include <type_traits>

#include "index_present_device.h"
#include "sp_index_compose.h"

namespace jsp::sp {
namespace {

using namespace jsp::ipresent;
using namespace index_walk;

struct SpPresentSrc {
    const uint32_t* keys;
    const IndexThumbRec* recs;   // per cell: what launch_index_show takes as arguments for its frame
    const uint4* blocks;
    const uint32_t* payload;
    const uint32_t* bitmap;
    long pic_stride;
    int nbx, nblocks;
};

// Phase 1 of both kernels below: compose (index_present_device.h) for a tile of 4 x 4 blocks, a wave per block.
template <bool VEC>
struct SpCompose {
    const SpPresentSrc& s;
    uint32_t* tile;
    IndexThumbRec rec;     // the cell's frame
    const uint32_t* key;   // ... and its key picture
    int X, Y;
    int wave, lane;
    __device__ __forceinline__ SpCompose(const SpPresentSrc& src, uint32_t* lds, const IndexPresentArgs& a)
        : s(src), tile(lds), rec(src.recs[blockIdx.z]), key(src.keys + (size_t)rec.key_slot * (size_t)src.pic_stride), X(a.fw), Y(a.fh),
          wave(__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))), lane(threadIdx.x & 63) {}
    __device__ __forceinline__ void operator()(int tx0, int ty0, int sx0, int sy0, int sx1, int sy1) const {
        const int bx = (tx0 >> 4) + wave;
        if (bx * 16 > sx1 || bx * 16 + 15 < sx0) return;               // (wave-uniform; what is left has bx < nbx)
        const int ly = lane >> 2, cx0 = (lane & 3) * 4;                 // row and first column inside the block
        for (int r = 0; r < 4; ++r) {
            const int by = (ty0 >> 4) + r;
            if (by * 16 > sy1 || by * 16 + 15 < sy0) continue;          // (uniform)
            const int y = by * 16 + ly, x0 = bx * 16 + cx0;
            const bool mine = y < Y && x0 < X;
            const size_t i0 = (size_t)y * (size_t)X + (size_t)x0;
            uint32_t px[4];
            index_compose<VEC>(px, key, s.blocks, s.payload, s.bitmap, rec.t, rec.k, (long)rec.slot_base, X, s.nblocks, by * s.nbx + bx, ly, cx0,
                               x0, i0, mine);
            *reinterpret_cast<uint4*>(tile + (r * 16 + ly) * T + wave * 16 + cx0) = make_uint4(px[0], px[1], px[2], px[3]);
        }
    }
};

template <bool VEC, int MODE, int FILTER, bool WIDE>
__global__ __launch_bounds__(kIndexPresentWG) void sp_index_present_kernel(const SpPresentSrc s, const IndexPresentArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[T * T];
    const SpCompose<VEC> compose(s, tile, a);
    present_rect<MODE, FILTER, WIDE, 16>(a, sheet_cell(a), tile, compose);
}

// jsp_sp_index_tensor: the same rectangle, its words stored as elements of a dense tensor.  MODE is one of the two canvas conversions.
template <bool VEC, int MODE, int FILTER, bool WIDE>
__global__ __launch_bounds__(kIndexPresentWG) void sp_index_tensor_kernel(const SpPresentSrc s, const IndexPresentArgs a, const IndexTensorArgs t) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[T * T];
    const SpCompose<VEC> compose(s, tile, a);
    PresentLane l;
    if (present_words<MODE, FILTER, WIDE, 16>(a, tile, compose, l)) store_elements(a, t, l);
}

// `vec`: the key pictures may be read 16 bytes at once
SpPresentSrc present_src(const Geometry& g, const int32_t* d_keys, size_t pic_stride, const IndexThumbRec* d_recs, const PBlock* d_blocks,
                         const uint32_t* d_payload, const uint32_t* d_bitmap, bool& vec) {
    SpPresentSrc s;
    s.keys = reinterpret_cast<const uint32_t*>(d_keys);
    s.recs = d_recs;
    s.blocks = reinterpret_cast<const uint4*>(d_blocks);
    s.payload = d_payload;
    s.bitmap = d_bitmap;
    s.pic_stride = (long)pic_stride;
    s.nbx = g.nbx;
    s.nblocks = g.nbx * g.nby;
    vec = (g.X & 3) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0 && (pic_stride & 3) == 0;
    return s;
}

}  // namespace

void launch_index_present(const Geometry& g, const int32_t* d_keys, size_t pic_stride, const IndexThumbRec* d_recs, int n, const PBlock* d_blocks,
                          const uint32_t* d_payload, const uint32_t* d_bitmap, const IndexPresentArgs& a, int mode, int filter, hipStream_t stream) {
    bool vec;
    const SpPresentSrc s = present_src(g, d_keys, pic_stride, d_recs, d_blocks, d_payload, d_bitmap, vec);
    const dim3 grid = present_grid(a, n);
    auto go = [&](auto V) {
        dispatch_mode(mode, [&](auto M) {
            dispatch_filter(filter, a.step, [&](auto F, auto W) {
                hipLaunchKernelGGL((sp_index_present_kernel<decltype(V)::value, decltype(M)::value, decltype(F)::value, decltype(W)::value>), grid,
                                   dim3(kIndexPresentWG), 0, stream, s, a);
            });
        });
    };
    if (vec) go(std::true_type{});
    else go(std::false_type{});
}

void launch_index_tensor(const Geometry& g, const int32_t* d_keys, size_t pic_stride, const IndexThumbRec* d_recs, int n, const PBlock* d_blocks,
                         const uint32_t* d_payload, const uint32_t* d_bitmap, const IndexPresentArgs& a, const IndexTensorArgs& t, int mode,
                         int filter, hipStream_t stream) {
    bool vec;
    const SpPresentSrc s = present_src(g, d_keys, pic_stride, d_recs, d_blocks, d_payload, d_bitmap, vec);
    const dim3 grid = present_grid(a, n);
    auto go = [&](auto V) {
        dispatch_canvas_mode(mode, [&](auto M) {
            dispatch_filter(filter, a.step, [&](auto F, auto W) {
                hipLaunchKernelGGL((sp_index_tensor_kernel<decltype(V)::value, decltype(M)::value, decltype(F)::value, decltype(W)::value>), grid,
                                   dim3(kIndexPresentWG), 0, stream, s, a, t);
            });
        });
    };
    if (vec) go(std::true_type{});
    else go(std::false_type{});
}

}  // namespace jsp::sp
