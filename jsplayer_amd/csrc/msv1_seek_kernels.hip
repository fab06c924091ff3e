// MSVideo1 seek for gfx950 (MI355X): frames K..N of a staged batch composed into ONE picture in one launch.
//
// An MSVideo1 inter frame codes a 4x4 block or leaves it as it was (a skip; nothing written after an 8-bit end marker or a
// truncated stream); there is no motion.  So block b of frame N is block b as coded by the LAST frame <= N whose table codes it,
// or the picture before the range when none does.  One work-item per block, blocks in raster order as in msv1_kernels.hip:
//   * the lane walks its table column from the last frame backwards (four entries in flight per step; one coalesced dword per
//     lane and frame), stopping at the first code offset;
//   * decodes that code (decode_block, msv1_decode.h) from the 20 bytes it needs, read as aligned dwords and zeroed past the end
//     of its frame's data — the 16-bit odd last byte and the codes past the end of a truncated frame exactly as the temporal
//     kernel handles them;
//   * or copies the block from the picture before the range when nothing in the range coded it;
//   * for the stage-2 compare (MSVideo1.hx:195-205) of the last frame, a block the last frame coded is also decoded as the
//     SECOND writer left it (or taken from the picture before) and compared, rows >= cmp_row_lo.
// Every pixel of `dst` is written at most once, with the same 16-byte row stores as the other block kernels.  Work-items past
// the last block copy the pixels no block covers (X % 4 / Y % 4 remainders) from the picture before.
#include "msv1_block_io.h"

namespace jsp {
namespace {

constexpr int WG = 256;
constexpr int SCAN = INDEX_SCAN;   // table entries a lane has in flight per step of its backward walk: the index walk's (msv1_block_io.h), 4

// The last frame <= `from` whose table codes block `blk` (its code offset in `o`), or -1.
__device__ __forceinline__ int last_writer(const uint32_t* __restrict__ desc, size_t pitch, int blk, int from, uint32_t& o) {
    for (int g = from; g >= 0; g -= SCAN) {
        uint32_t e[SCAN];
#pragma unroll
        for (int k = 0; k < SCAN; ++k) e[k] = g - k >= 0 ? *(cgu32*)(desc + (size_t)(g - k) * pitch + blk) : MSV1_DESC_SKIP;
#pragma unroll
        for (int k = 0; k < SCAN; ++k)
            if (e[k] < MSV1_DESC_UNTOUCHED) { o = e[k]; return g - k; }
    }
    return -1;
}

template <int BITS, bool VEC>
__global__ __launch_bounds__(WG) void msv1_seek_kernel(const uint8_t* __restrict__ stream, const uint32_t* __restrict__ desc, size_t pitch,
                                                       const Msv1FrameArgs* __restrict__ frames, int nframes, const int32_t* __restrict__ palette,
                                                       uint32_t* __restrict__ dst, const uint32_t* __restrict__ base, uint32_t cmp_row_lo,
                                                       uint32_t* __restrict__ signif, int nblocks, int nbx, int X, int cx, int cy, long nrem) {
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, palette);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    if (gid >= nblocks) {   // a pixel no block covers: the right strip [0, cy) x [cx, X), then the rows [cy, Y)
        const long r = gid - nblocks;
        if (r >= nrem || base == nullptr || base == dst) return;
        const size_t i = uncovered_pixel(r, X, cx, cy);
        *(gu32*)(dst + i) = *(cgu32*)(base + i);
        return;
    }
    const int blk = (int)gid;
    const int by = blk / nbx;
    const int bx = blk - by * nbx;
    const size_t di = (size_t)by * 4u * (size_t)X + (size_t)bx * 4u;
    uint32_t o = 0;
    const int wf = last_writer(desc, pitch, blk, nframes - 1, o);
    uint32_t px[16];
    if (wf < 0) {   // nothing in the range coded the block: it shows the picture before the range
        if (base != nullptr && base != dst) {
            load_block<VEC>(base + di, X, px);
            store_block<VEC>(dst + di, X, px);
        }
        return;
    }
    decode_at<BITS>(stream, o, frames[wf].stream_end, s_pal, px);
    bool diff = false;
    if (cmp_row_lo != 0xFFFFFFFFu && wf == nframes - 1) {
        // the picture before the last frame at this block: what the frame before it that coded the block made of it, else the
        // picture before the range (`dst` itself when that is where it lies — read before this lane writes it)
        uint32_t pv[16];
        uint32_t o2 = 0;
        const int wf2 = last_writer(desc, pitch, blk, nframes - 2, o2);
        if (wf2 >= 0) decode_at<BITS>(stream, o2, frames[wf2].stream_end, s_pal, pv);
        else load_block<VEC>((base != nullptr ? base : dst) + di, X, pv);
#pragma unroll
        for (int y = 0; y < 4; ++y)
            if ((uint32_t)(by * 4 + y) >= cmp_row_lo)
                diff |= (pv[y * 4] != px[y * 4]) | (pv[y * 4 + 1] != px[y * 4 + 1]) | (pv[y * 4 + 2] != px[y * 4 + 2]) | (pv[y * 4 + 3] != px[y * 4 + 3]);
    }
    store_block<VEC>(dst + di, X, px);
    // one word per launch: raise_flag's rule, with the ballot taken once (the instructions this kernel has always had)
    const unsigned long long m = __ballot(diff);
    if (m != 0ull && (threadIdx.x & 63) == __ffsll((long long)m) - 1 &&
        __hip_atomic_load(signif, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        atomicOr(signif, 1u);
}

// ---- skip stills: which frames of a staged range change the picture (msv1_change_scan_kernel) -------------------------------
// The last entry of walk[0, j) whose frame codes block `blk` (its code offset in `o`), as a frame index, or -1.  walk[] lists the
// frames that can code anything (no early-outs), ascending; SCAN entries in flight per step as in last_writer.
__device__ __forceinline__ int last_writer_walk(const uint32_t* __restrict__ desc, size_t pitch, const uint32_t* __restrict__ walk,
                                                int blk, int j, uint32_t& o) {
    for (int g = j - 1; g >= 0; g -= SCAN) {
        uint32_t e[SCAN];
#pragma unroll
        for (int k = 0; k < SCAN; ++k) e[k] = g - k >= 0 ? *(cgu32*)(desc + (size_t)walk[g - k] * pitch + blk) : MSV1_DESC_SKIP;
#pragma unroll
        for (int k = 0; k < SCAN; ++k)
            if (e[k] < MSV1_DESC_UNTOUCHED) { o = e[k]; return (int)walk[g - k]; }
    }
    return -1;
}

// One work-item per block (raster order) and per SEGMENT of the walk list (blockIdx.y: entries [y * seg, (y + 1) * seg)).  A lane
// walks its table column forward through its segment, SCAN entries in flight per step, and remembers only WHERE the block was
// last coded (frame, code offset).  At a frame that is judged (rows[f] != ~0u) and codes the block in a block row reaching
// rows[f], it decodes the new code and the block's previous state — the last earlier writer in the range (found by a backward
// search when the segment has not met one yet), else `before` — and compares the rows >= rows[f]: the rule and the decode of
// msv1_seek_kernel's stage-2 compare.  A difference ORs signif[f] and lowers *first_hit; lanes stop at frames past *first_hit
// (an optimisation only: every frame <= the earliest difference is walked by every lane whatever it sees of other lanes' stores).
// Writes no picture.
// ALL (jsp_index_build): every judged frame is judged — no stop at the first hit, first_hit unused.  The jsp_find_change form (ALL = false)
// is unchanged.
template <int BITS, bool VEC, bool ALL = false>
__global__ __launch_bounds__(WG) void msv1_change_scan_kernel(const uint8_t* __restrict__ stream, const uint32_t* __restrict__ desc, size_t pitch,
                                                              const Msv1FrameArgs* __restrict__ frames, const int32_t* __restrict__ palette,
                                                              const uint32_t* __restrict__ walk, int nwalk, int seg, const uint32_t* __restrict__ rows,
                                                              uint32_t* __restrict__ signif, uint32_t* __restrict__ first_hit,
                                                              const uint32_t* __restrict__ before, int nblocks, int nbx, int X) {
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, palette);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    if (gid >= nblocks) return;
    const int blk = (int)gid;
    const int by = blk / nbx;
    const int bx = blk - by * nbx;
    const uint32_t row_top = (uint32_t)by * 4u + 3u;   // the block's last pixel row
    const int j0 = (int)blockIdx.y * seg;
    const int j1 = min(nwalk, j0 + seg);
    int wf = -2;              // frame that last coded the block (-1: none in the range; -2: not looked up yet)
    uint32_t wo = 0;          // ... and its code offset
    for (int j = j0; j < j1; j += SCAN) {
        if (!ALL && walk[j] > __hip_atomic_load(first_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        uint32_t e[SCAN];
#pragma unroll
        for (int k = 0; k < SCAN; ++k) e[k] = j + k < j1 ? *(cgu32*)(desc + (size_t)walk[j + k] * pitch + blk) : MSV1_DESC_UNTOUCHED;
#pragma unroll
        for (int k = 0; k < SCAN; ++k) {
            if (e[k] >= MSV1_DESC_UNTOUCHED) continue;
            const int f = (int)walk[j + k];
            const uint32_t row = rows[f];
            if (row != 0xFFFFFFFFu && row_top >= row) {
                if (wf == -2) wf = last_writer_walk(desc, pitch, walk, blk, j + k, wo);
                uint32_t px[16], pv[16];
                decode_at<BITS>(stream, e[k], frames[f].stream_end, s_pal, px);
                if (wf >= 0) decode_at<BITS>(stream, wo, frames[wf].stream_end, s_pal, pv);
                else load_block<VEC>(before + (size_t)by * 4u * (size_t)X + (size_t)bx * 4u, X, pv);
                bool diff = false;
#pragma unroll
                for (int y = 0; y < 4; ++y)
                    if ((uint32_t)(by * 4 + y) >= row)
                        diff |= (pv[y * 4] != px[y * 4]) | (pv[y * 4 + 1] != px[y * 4 + 1]) | (pv[y * 4 + 2] != px[y * 4 + 2]) | (pv[y * 4 + 3] != px[y * 4 + 3]);
                raise_flag_lane(signif + f, diff);
                if (!ALL && diff && __hip_atomic_load(first_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)f) atomicMin(first_hit, (uint32_t)f);
            }
            wf = f;
            wo = e[k];
        }
    }
}

// ---- seek index (jsp_index_build / jsp_index_show) -----------------------------------------------------------------------
// Build, once per staged chunk: frames [a, b) of the index are frames [0, b - a) of the chunk's tables.  One work-item per block and
// per bitmap word (blockIdx.y) overlapping the chunk: the lane reads its table column for the word's frames (one coalesced dword per
// lane and frame, all in flight at once) and writes
//   * bitmap[w * nblocks + blk] bit k: frame 32 w + k codes the block (entry below MSV1_DESC_UNTOUCHED) — word-major, so that the
//     show kernel's lanes read consecutive dwords;
//   * rows[w * nby + by] bit k |= frame 32 w + k codes a block of block row by (what the host parser leaves in block_changes[by]);
//     a segmented OR over the wave's lanes of one row, then one atomic per row and wave;
//   * stop[f] = min(stop[f], the first block frame f leaves untouched) — an 8-bit end marker or the end of a host-parsed stream
//     (the untouched blocks are a suffix, so the wave's lowest lane is its first); one atomic per frame and wave that has any.
// Words shared with the chunk before keep its bits (nothing else writes the word meanwhile: the chunks follow each other on one stream).
__global__ __launch_bounds__(WG) void msv1_coded_bitmap_kernel(const uint32_t* __restrict__ desc, size_t pitch, int a, int b, uint32_t* __restrict__ bitmap,
                                                               uint32_t* __restrict__ rows, uint32_t* __restrict__ stop, int nblocks, int nbx, int nby) {
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    const int w = a / 32 + (int)blockIdx.y;
    const int f0 = max(a, 32 * w), f1 = min(b, 32 * w + 32);
    const bool in = gid < nblocks;
    const int blk = in ? (int)gid : 0;
    uint32_t coded = 0, untouched = 0;
    if (in) {
        uint32_t e[32];   // (MSV1_DESC_SKIP for frames outside the chunk: neither coded nor untouched)
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int f = 32 * w + k;
            e[k] = f >= f0 && f < f1 ? *(cgu32*)(desc + (size_t)(f - a) * pitch + blk) : MSV1_DESC_SKIP;
        }
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            coded |= (e[k] < MSV1_DESC_UNTOUCHED ? 1u : 0u) << k;
            untouched |= (e[k] == MSV1_DESC_UNTOUCHED ? 1u : 0u) << k;
        }
        uint32_t* word = bitmap + (size_t)w * (size_t)nblocks + blk;
        *word = (32 * w < a ? *word : 0u) | coded;
    }
    // rows: lanes of one block row are consecutive; after the shuffles the first lane of each row holds the row's OR
    const int lane = threadIdx.x & 63;
    const int row = in ? blk / nbx : -1;
    uint32_t v = coded;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(v, d);
        const int orow = __shfl_down(row, d);
        if (lane + d < 64 && orow == row) v |= o;
    }
    const int up = __shfl_up(row, 1);
    if (in && v != 0u && (lane == 0 || up != row)) atomicOr(rows + (size_t)w * (size_t)nby + row, v);
    if (__ballot(untouched != 0u) != 0ull) {
        for (int k = 0; k < 32; ++k) {
            const unsigned long long m = __ballot((untouched >> k) & 1u);
            if (m != 0ull && lane == __ffsll((long long)m) - 1) atomicMin(stop + 32 * w + k, (uint32_t)blk);
        }
    }
}

// The index kernels below read the index as one record (Msv1IndexSrc, by value) and compose a block by one rule (index_block,
// msv1_block_io.h): the last frame <= t that coded it, else `before`, else nothing.  What a kernel writes is an argument of its own.

// Show frame t: one work-item per block, as msv1_seek_kernel, storing the block index_block composes (an undefined block leaves `dst`
// as it is).  Work-items past the last block copy the pixels no block covers from `before`.
template <int BITS, bool VEC>
__global__ __launch_bounds__(WG) void msv1_index_show_kernel(const Msv1IndexSrc s, int t, uint32_t* __restrict__ dst, int cx, int cy, long nrem) {
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, s.palette);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    if (gid >= s.nblocks) {   // a pixel no block covers, as in msv1_seek_kernel
        const long r = gid - s.nblocks;
        if (r >= nrem || s.before == nullptr) return;
        const size_t i = uncovered_pixel(r, s.X, cx, cy);
        *(gu32*)(dst + i) = *(cgu32*)(s.before + i);
        return;
    }
    const int blk = (int)gid;
    const int by = blk / s.nbx;
    const int bx = blk - by * s.nbx;
    uint32_t px[16];
    if (index_block<BITS>(s, t, blk, bx, by, VEC, s_pal, px)) store_block<VEC>(dst + (size_t)by * 4u * (size_t)s.X + (size_t)bx * 4u, s.X, px);
}

// index_last_writer with a lower bound: the bitmap word of block `blk` that holds the last frame in (tp, t] coding it, masked to those
// frames (index_word_frame(w, m) is that frame; w is set), or 0 when nothing in the span coded the block.  The top word is masked to the
// frames <= t, the bottom word (that of frame tp + 1) to the frames > tp, and the walk down (SCAN words in flight per step) stops at the
// bottom word.  (cw, cv) is the top word the lane fetched last and (pw, pv) the one before it: consecutive spans of a run fetch a word
// once while the run's frames stay in it, and a span of stride <= 32 — two words at most — finds its bottom word in (pw, pv).
__device__ __forceinline__ uint32_t index_last_writer_span(const Msv1IndexSrc& s, int blk, int tp, int t, int& w, int& cw, uint32_t& cv, int& pw,
                                                           uint32_t& pv) {
    const int lo = tp + 1, wb = lo >> 5;
    const uint32_t mask_lo = 0xFFFFFFFFu << (lo & 31);
    w = t >> 5;
    if (w != cw) {
        pw = cw; pv = cv;
        cw = w; cv = *(cgu32*)(s.bitmap + (size_t)w * (size_t)s.nblocks + blk);
    }
    uint32_t m = cv & (0xFFFFFFFFu >> (31 - (t & 31)));
    if (w == wb) return m & mask_lo;
    while (m == 0u && w > wb) {
        uint32_t e[SCAN];
#pragma unroll
        for (int k = 0; k < SCAN; ++k) {
            const int i = w - 1 - k;
            e[k] = i < wb ? 0u : i == pw ? pv : *(cgu32*)(s.bitmap + (size_t)i * (size_t)s.nblocks + blk);
            if (i == wb) e[k] &= mask_lo;
        }
        int step = SCAN;
#pragma unroll
        for (int k = SCAN - 1; k >= 0; --k)
            if (e[k] != 0u) { m = e[k]; step = k + 1; }
        w -= step;
    }
    return m;
}

// Play (jsp_index_play): frames t_k = first + k * stride, k < n, each into dsts[k] exactly as msv1_index_show_kernel(t_k) writes it — ONE
// launch.  One work-item per block as there, and per SEGMENT of the run (blockIdx.y: destinations [y * seg, (y + 1) * seg)).  The lane
// composes its segment's first frame as the show kernel does (index_block) and keeps the 16 pixels in registers; `have` says whether
// the block is defined yet (Show leaves an undefined block alone, and so does every store here).  For each further
// frame it asks for the last writer in (t_{k-1}, t_k] (index_last_writer_span): a coded block overwrites the whole block, so only the
// last writer of the gap is decoded, and the registers stay when there is none.  A null dsts[k] (a frame before the index's first
// adopting one, where Show writes nothing) is walked but not stored.  k is wave-uniform: all lanes of a wave store to the same
// destination in the same iteration, with the show kernel's row stores.  Work-items past the last block copy the pixels no block covers
// from `before` into every non-null destination of the segment.
template <int BITS, bool VEC>
__global__ __launch_bounds__(WG) void msv1_index_play_kernel(const Msv1IndexSrc s, int first, int n, int stride, int seg,
                                                             uint32_t* const* __restrict__ dsts, int cx, int cy, long nrem) {
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, s.palette);
    const int k0 = (int)blockIdx.y * seg;
    const int k1 = min(n, k0 + seg);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    if (gid >= s.nblocks) {   // a pixel no block covers, as in msv1_seek_kernel
        const long r = gid - s.nblocks;
        if (r >= nrem || s.before == nullptr) return;
        const size_t i = uncovered_pixel(r, s.X, cx, cy);
        const uint32_t v = *(cgu32*)(s.before + i);
        for (int k = k0; k < k1; ++k) {
            uint32_t* d = dsts[k];
            if (d != nullptr) *(gu32*)(d + i) = v;
        }
        return;
    }
    const int blk = (int)gid;
    const int by = blk / s.nbx;
    const int bx = blk - by * s.nbx;
    const size_t di = (size_t)by * 4u * (size_t)s.X + (size_t)bx * 4u;
    int t = first + k0 * stride;
    uint32_t px[16];
    bool have = index_block<BITS>(s, t, blk, bx, by, VEC, s_pal, px);
    int cw = -1, pw = -1;
    uint32_t cv = 0u, pv = 0u;
    for (int k = k0;;) {
        uint32_t* d = dsts[k];
        if (have && d != nullptr) store_block<VEC>(d + di, s.X, px);
        if (++k >= k1) break;
        const int tp = t;
        t += stride;
        int w;
        const uint32_t m = index_last_writer_span(s, blk, tp, t, w, cw, cv, pw, pv);
        if (m != 0u) {
            index_decode<BITS>(s, index_word_frame(w, m), blk, s_pal, px);
            have = true;
        }
    }
}

// Thumbnails (jsp_index_thumbs): the pictures of n frames of the index, each reduced S x S pixels to one (box mean, rounded half up),
// into one sheet — ONE launch, no full-size picture anywhere.  blockIdx.y is the thumbnail, frames[blockIdx.y] its frame; a lane per
// 4x4 block and thumbnail composes the block as the show kernel does (index_block; an undefined block is zeros) and sums its 16
// pixels, R and B together under 0x00FF00FF, G apart: at S = 16 a field ends at most at 256 * 255 + 128 < 2^16, so the 16-bit fields
// never carry into each other.
//   S = 4:  the lane's block is the output pixel; lanes in block raster order, one dword store each (a wave writes 256 contiguous bytes
//           of a thumbnail row, or the end of one row and the start of the next).
//   S = 8 / 16: G = S / 4; the G x G blocks of one output pixel are G * G consecutive lanes (lane & (G - 1) the block column, the next
//           bits the block row), output pixels in raster order.  A wave covers 16 / 4 output pixels of a thumbnail row, so per block
//           row it reads 32 / 16 consecutive bitmap and table dwords.  The partial sums are added with __shfl_xor inside the group
//           (no LDS memory, no barrier) and the group's first lane stores.
// Only whole output pixels are enumerated (tw = 4 nbx / S, th = 4 nby / S), so every lane of a live group has a block inside the
// picture; the trailing block column / row that fills no output pixel and the X % 4, Y % 4 remainders are never read.  A group is
// aligned to G * G lanes and lives or returns as one, so the shuffles only meet live lanes.
template <int BITS, int S>
__global__ __launch_bounds__(WG) void msv1_index_thumbs_kernel(const Msv1IndexSrc s, const int32_t* __restrict__ frames, uint32_t* __restrict__ out,
                                                               int tw, int th, int cols) {
    constexpr int G = S / 4, GG = G * G;                            // blocks per output pixel: a side, all
    constexpr int LG = S == 4 ? 0 : S == 8 ? 1 : 2;                 // log2(G)
    constexpr uint32_t SH = 4 + 2 * LG, HALF = (uint32_t)(S * S) / 2u;   // log2(S * S), the rounding term
    __shared__ uint32_t s_pal[BITS == 8 ? 256 : 1];
    load_palette<BITS>(s_pal, s.palette);
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    const long q = gid >> (2 * LG);                                 // output pixel of the thumbnail, raster order
    if (q >= (long)tw * th) return;
    const int sub = (int)(gid & (GG - 1));
    const int py = (int)(q / tw);
    const int px_ = (int)(q - (long)py * tw);
    const int by = py * G + (sub >> LG);
    const int bx = px_ * G + (sub & (G - 1));
    const int k = (int)blockIdx.y;
    uint32_t px[16];
    index_block<BITS>(s, frames[k], by * s.nbx + bx, bx, by, s.before_vec != 0, s_pal, px);
    uint32_t rb = 0, g = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        rb += px[i] & 0x00FF00FFu;
        g += (px[i] >> 8) & 0xFFu;
    }
#pragma unroll
    for (int d = 1; d < GG; d <<= 1) {
        rb += (uint32_t)__shfl_xor((int)rb, d);
        g += (uint32_t)__shfl_xor((int)g, d);
    }
    if (sub != 0) return;
    const uint32_t r = ((rb >> 16) + HALF) >> SH, b = ((rb & 0xFFFFu) + HALF) >> SH;
    const size_t sheet_pitch = (size_t)cols * (size_t)tw;
    const size_t at = (size_t)(k / cols) * (size_t)th * sheet_pitch + (size_t)(k % cols) * (size_t)tw + (size_t)py * sheet_pitch + (size_t)px_;
    *(gu32*)(out + at) = (r << 16) | (((g + HALF) >> SH) << 8) | b;
}

// The seek and show kernels' work: one work-item per block, then one per pixel no block covers (nrem of them: the columns from cx on
// in the block rows, the rows from cy on), and whether rows of `dst` and `src` may move 16 bytes at a time.  False: nothing to do.
// (geo: a batch's Msv1Geometry or an index's Msv1IndexSrc)
struct PictureGrid { int cx, cy; long nrem; dim3 grid; bool vec; };
template <class Geo>
bool picture_grid(const Geo& geo, const void* dst, const void* src, PictureGrid& g) {
    if (geo.X <= 0 || geo.Y <= 0) return false;
    g.cx = geo.nbx * 4;
    g.cy = geo.nby * 4;
    g.nrem = (long)(geo.X - g.cx) * g.cy + (long)geo.X * (geo.Y - g.cy);
    const long work = (long)std::max(geo.nblocks, 0) + g.nrem;
    if (work <= 0) return false;
    g.vec = (geo.X & 3) == 0 && !(reinterpret_cast<uintptr_t>(dst) & 15) && !(reinterpret_cast<uintptr_t>(src) & 15);
    g.grid = dim3((unsigned)((work + WG - 1) / WG));
    return true;
}

// How many times over a launch of one work-item per block must run (its segments along grid.y) to put ~8 waves on every SIMD: a 1080p
// picture alone gives ~2.
long segments_to_fill(int nblocks) {
    const long waves_one = std::max(1L, ((long)nblocks + 63) / 64);
    return std::max(1L, (8L * 1024L + waves_one - 1) / waves_one);
}

// Segments of the walk list: segments_to_fill, at least 16 entries each
dim3 scan_grid(const Msv1Geometry& geo, int nwalk, int& seg) {
    long nseg = std::min(segments_to_fill(geo.nblocks), std::max(1L, ((long)nwalk + 15) / 16));
    nseg = std::min(nseg, 65535L);
    seg = (int)(((long)nwalk + nseg - 1) / nseg);
    nseg = ((long)nwalk + seg - 1) / seg;
    return dim3((unsigned)((geo.nblocks + WG - 1) / WG), (unsigned)nseg);
}
}  // namespace

void msv1_launch_seek(const Msv1SeekView& v, int32_t* dst, const int32_t* base, uint32_t cmp_row_lo, hipStream_t stream) {
    const Msv1Geometry& geo = v.geo;
    PictureGrid g;
    if (v.nframes <= 0 || !picture_grid(geo, dst, base, g)) return;
    uint32_t* signif = v.d_signif + (v.nframes - 1);
    dispatch_bits_vec(geo.bits, g.vec, [&](auto B, auto V) {
        hipLaunchKernelGGL((msv1_seek_kernel<decltype(B)::value, decltype(V)::value>), g.grid, dim3(WG), 0, stream, v.d_stream, v.d_desc, v.desc_pitch,
                           v.d_frames, v.nframes, v.d_palette, reinterpret_cast<uint32_t*>(dst), reinterpret_cast<const uint32_t*>(base), cmp_row_lo,
                           signif, geo.nblocks, std::max(geo.nbx, 1), geo.X, g.cx, g.cy, g.nrem);
    });
}

void msv1_launch_change_scan(const Msv1SeekView& v, const uint32_t* d_walk, int nwalk, const uint32_t* d_rows, uint32_t* d_first_hit,
                             const int32_t* before, hipStream_t stream) {
    const Msv1Geometry& geo = v.geo;
    if (nwalk <= 0 || geo.nblocks <= 0) return;
    int seg = 0;
    const dim3 grid = scan_grid(geo, nwalk, seg), block(WG);
    const bool vec = (geo.X & 3) == 0 && !(reinterpret_cast<uintptr_t>(before) & 15);
    dispatch_bits_vec(geo.bits, vec, [&](auto B, auto V) {
        auto launch = [&](auto ALL) {
            hipLaunchKernelGGL((msv1_change_scan_kernel<decltype(B)::value, decltype(V)::value, decltype(ALL)::value>), grid, block, 0, stream, v.d_stream,
                               v.d_desc, v.desc_pitch, v.d_frames, v.d_palette, d_walk, nwalk, seg, d_rows, v.d_signif, d_first_hit,
                               reinterpret_cast<const uint32_t*>(before), geo.nblocks, std::max(geo.nbx, 1), geo.X);
        };
        if (d_first_hit) launch(std::false_type{});
        else launch(std::true_type{});
    });
}

void msv1_launch_coded_bitmap(const Msv1SeekView& v, int a, uint32_t* d_bitmap, uint32_t* d_rows, uint32_t* d_stop, hipStream_t stream) {
    const Msv1Geometry& geo = v.geo;
    if (v.nframes <= 0 || geo.nblocks <= 0) return;
    const int b = a + v.nframes;
    const dim3 grid((unsigned)((geo.nblocks + WG - 1) / WG), (unsigned)((b - 1) / 32 - a / 32 + 1)), block(WG);
    hipLaunchKernelGGL(msv1_coded_bitmap_kernel, grid, block, 0, stream, v.d_desc, v.desc_pitch, a, b, d_bitmap, d_rows, d_stop, geo.nblocks,
                       std::max(geo.nbx, 1), geo.nby);
}

void msv1_launch_index_show(const Msv1IndexSrc& src, int t, int32_t* dst, hipStream_t stream) {
    PictureGrid g;
    if (!picture_grid(src, dst, src.before, g)) return;
    dispatch_bits_vec(src.bits, g.vec, [&](auto B, auto V) {
        hipLaunchKernelGGL((msv1_index_show_kernel<decltype(B)::value, decltype(V)::value>), g.grid, dim3(WG), 0, stream, src, t,
                           reinterpret_cast<uint32_t*>(dst), g.cx, g.cy, g.nrem);
    });
}

int msv1_index_play_auto_segments(const Msv1IndexSrc& src, int n) {   // (never more segments than frames)
    return (int)std::min(segments_to_fill(src.nblocks), (long)std::max(n, 1));
}

void msv1_launch_index_play(const Msv1IndexSrc& src, int first, int n, int stride, int segs, int32_t* const* d_dsts, bool dsts_aligned16,
                            hipStream_t stream) {
    PictureGrid g;
    if (n <= 0 || !picture_grid(src, nullptr, src.before, g)) return;
    const bool vec = g.vec && dsts_aligned16;
    const int seg = (n + std::min(std::max(segs, 1), n) - 1) / std::min(std::max(segs, 1), n);   // destinations per segment
    const dim3 grid(g.grid.x, (unsigned)((n + seg - 1) / seg));
    dispatch_bits_vec(src.bits, vec, [&](auto B, auto V) {
        hipLaunchKernelGGL((msv1_index_play_kernel<decltype(B)::value, decltype(V)::value>), grid, dim3(WG), 0, stream, src, first, n, stride, seg,
                           reinterpret_cast<uint32_t* const*>(d_dsts), g.cx, g.cy, g.nrem);
    });
}

// f(std::integral_constant<int, BITS>{}, std::integral_constant<int, S>{}) for the thumbnail kernel that `bits` (16, else 8) and
// `scale` (4, 8 or 16; any other: nothing) select.
template <class F>
void dispatch_bits_scale(int bits, int scale, F&& f) {
    auto with_bits = [&](auto B) {
        if (scale == 4) f(B, std::integral_constant<int, 4>{});
        else if (scale == 8) f(B, std::integral_constant<int, 8>{});
        else if (scale == 16) f(B, std::integral_constant<int, 16>{});
    };
    if (bits == 16) with_bits(std::integral_constant<int, 16>{});
    else with_bits(std::integral_constant<int, 8>{});
}

void msv1_launch_index_thumbs(const Msv1IndexSrc& src, const int32_t* d_frames, int n, int scale, int cols, int32_t* out, hipStream_t stream) {
    const int tw = src.nbx * 4 / scale, th = src.nby * 4 / scale;
    if (n <= 0 || cols <= 0 || tw <= 0 || th <= 0) return;
    const long lanes = (long)tw * th * (scale / 4) * (scale / 4);
    const dim3 grid((unsigned)((lanes + WG - 1) / WG), (unsigned)n);
    dispatch_bits_scale(src.bits, scale, [&](auto B, auto S) {
        hipLaunchKernelGGL((msv1_index_thumbs_kernel<decltype(B)::value, decltype(S)::value>), grid, dim3(WG), 0, stream, src, d_frames,
                           reinterpret_cast<uint32_t*>(out), tw, th, cols);
    });
}

}  // namespace jsp
