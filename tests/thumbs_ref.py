"""The numpy reference of the thumbnail contract (include/jsplayer_amd.h, jsp_index_thumbs): box mean of s x s pixels per channel,
rounded half up, in integer arithmetic, and the sheet layout.  A plain helper module (no tests of its own)."""
import numpy as np

SCALES = (4, 8, 16)


def thumb_size(w, h, s):
    """(TW, TH): whole s x s squares of the picture's whole 4x4 blocks."""
    return (4 * (w // 4)) // s, (4 * (h // 4)) // s


def thumbnail(picture, w, h, s):
    """`picture`: w * h words 0x00RRGGBB (any integer dtype of 32 bits), rows in the frame's order -> (TH, TW) int32."""
    assert s in SCALES
    tw, th = thumb_size(w, h, s)
    assert tw > 0 and th > 0
    pic = np.asarray(picture).reshape(-1).view(np.uint32).reshape(h, w)[:th * s, :tw * s].astype(np.int64)
    shift = {4: 4, 8: 6, 16: 8}[s]
    out = np.zeros((th, tw), dtype=np.int64)
    for pos in (16, 8, 0):
        c = ((pic >> pos) & 0xFF).reshape(th, s, tw, s).sum(axis=(1, 3))
        out |= ((c + (s * s) // 2) >> shift) << pos
    return out.astype(np.uint32).view(np.int32)


def cell_origin(k, cols, tw, th):
    """Index of thumbnail k's pixel (0, 0) in a sheet of pitch cols * tw."""
    return (k // cols) * th * (cols * tw) + (k % cols) * tw


def sheet(thumbs, cols, fill=0):
    """The thumbnails (each (TH, TW)) laid out `cols` to a row -> (ceil(n / cols) * TH, cols * TW) int32; cells past the last
    thumbnail hold `fill`."""
    n = len(thumbs)
    th, tw = thumbs[0].shape
    rows, pitch = -(-n // cols) * th, cols * tw
    out = np.full(rows * pitch, fill & 0xFFFFFFFF, dtype=np.uint32).view(np.int32)
    for k, t in enumerate(thumbs):
        at = cell_origin(k, cols, tw, th)
        for y in range(th):
            out[at + y * pitch: at + y * pitch + tw] = t[y]
    return out.reshape(rows, pitch)
