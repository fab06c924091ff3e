// The MSVideo1 16-bit encoder (jsp_msv1_encode_frames): what its host side (msv1_encode.cpp) and its two kernels
// (msv1_encode_kernels.hip, which states THE RULE) share.  A slice of pictures a launch, grid.y = the picture.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace jsp {

constexpr int MSV1_ENCODE_SLOT_WORDS = 5;   // a block's code as the sizes launch keeps it: the word | colour 0 << 16, then colours 1..7

// Pictures of nbx x nby blocks, row y of one at base + y * pitch ints (pitch signed, |pitch| >= 4 nbx), and the scratch of a slice.
struct Msv1EncodeArgs {
    const int32_t* const* pictures;  // per picture of the slice: its base (device pointers, in device memory) ...
    const int32_t* const* previous;  // ... and the base of the picture it is coded against, null for a key frame
    ptrdiff_t pitch;
    int nbx, nb;                     // blocks a row, blocks a picture
    const uint64_t* bases;           // per picture: where its frame starts in `out`
    uint32_t* totals;                // per picture and workgroup: the bytes of its codes and skip words
    uint32_t* first_coded;           // per picture and workgroup: its first coded block, MSV1_DELTA_NONE when it has none
    uint32_t* records;               // per picture and block: (offset within the workgroup's output << 8 | L); L = code length,
                                     // MSV1_DELTA_SKIP for a run head, 0 for nothing
    uint32_t* slots;                 // per picture and block: MSV1_ENCODE_SLOT_WORDS words, of which a code of L bytes fills L / 4 + 1
    uint8_t* out;                    // the frames of the slice back to back (16-byte aligned)
};

// vec: every base is 16-byte aligned and pitch % 4 == 0 — a block's rows move as 16 bytes; else as scalar words.
void msv1_launch_encode_sizes(const Msv1EncodeArgs& a, int npictures, bool vec, hipStream_t stream);
void msv1_launch_encode_gather(const Msv1EncodeArgs& a, int npictures, hipStream_t stream);

}  // namespace jsp
