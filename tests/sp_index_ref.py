"""Reference for the ScreenPressor seek index (jsp_sp_index_*), shared by the CPU and GPU tests: the clips, the oracle's sequential
run they are pinned to, and a numpy restatement of what the index composes.

The premise of the index: with every inter frame literalised (HostDecoder::literalise_motion) no block reads the picture before it
anywhere but at its own position, so pixel p of frame t is the literal of the LAST frame in (k, t] whose changed rectangle covers
p, else pixel p of the key picture k.  `compose` walks the literalised records of k..t backwards with a covered mask, the key
picture underneath — per pixel what sp_index_show_kernel does per lane.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np

from jsplayer_amd import streamgen as sg


@dataclass
class Clip:
    name: str
    w: int
    h: int
    bpp: int
    version: int
    key_row: int
    chunks: List[bytes] = field(repr=False)
    keys: List[bool] = field(repr=False)
    frames: List[np.ndarray] = field(repr=False)   # the encoder's pictures


def make_clip(cfg: int, w: int, h: int, n: int, bpp: int, version: int, key_every: int = 13, key_row: int = 36) -> Clip:
    """A clip with everything the index must cope with: coded key frames every `key_every` frames, a flat key frame (followed by
    inter frames), a key frame right behind a key frame, unchanged frames, and two frames that move 45 - 60 % of their blocks (far
    above the quarter up to which staging literalises)."""
    flat = key_every + 4 if key_every else 0
    kw = dict(key_every=key_every, flat_at=(flat, 2 * key_every + 1) if key_every else (), unchanged_at=(3, 4, n - 2),
              p_mix_at={6: dict(unchanged=0.3, motion=0.6), 8: dict(unchanged=0.35, motion=0.45), n - 4: dict(unchanged=0.2, motion=0.55)})
    chunks, keys, frames = sg.sp_clip(cfg, w, h, n, bpp=bpp, version=version, **kw)
    return Clip(f"v{version}_{bpp}bpp_{w}x{h}_n{n}_k{key_every}", w, h, bpp, version, key_row, chunks, keys,
                [f.astype(np.uint32) for f in frames])


def oracle_run(clip: Clip, preinit: int = 36):
    """OracleScreenPressor over the clip frame by frame, every destination first filled with the picture before it (the rule
    jsp_sp_index_show is defined by).  Returns (pictures, verdicts): verdicts[t] = DecompressP's for an inter frame; for a key
    frame the Manager's frames_differ_significantly — frame 0: True; behind a key frame: their bytes differ; else the pixels
    from row key_row on differ from the picture before."""
    from oracle_binding import OracleScreenPressor
    orc = OracleScreenPressor(clip.w, clip.h, clip.bpp)
    orc.Preinit(preinit)
    bufs = [np.zeros(clip.w * clip.h, dtype=np.int32) for _ in range(2)]
    pictures, verdicts = [], []
    prev = None
    for t, (src, key) in enumerate(zip(clip.chunks, clip.keys)):
        dst = bufs[0] if prev is not bufs[0] else bufs[1]
        if prev is not None:
            dst[:] = prev
        if key:
            assert orc.DecompressI(src, dst) == 0, t
            now = orc.PreviousFrame()
            assert now is dst
            if t == 0:
                v = True
            elif clip.keys[t - 1]:
                v = bytes(clip.chunks[t - 1]) != bytes(src)
            else:
                first = clip.key_row * clip.w
                v = bool(np.any(now[first:] != prev[first:]))
        else:
            data, v = orc.DecompressP(src, dst)
            now = orc.PreviousFrame()
            assert data is now and now is not None
        prev = now
        pictures.append(now.view(np.uint32).copy())
        verdicts.append(bool(v))
    orc.close()
    return pictures, verdicts


class Composer:
    """The index's composition in numpy, fed by the product's host stage (hoststage_binding.HostStage) frame by frame: key frames
    expanded to pictures, inter frames literalised and kept as (literal image, changed mask), `picture(t)` = the walk backwards."""

    def __init__(self, clip: Clip, preinit: int = 36):
        import hoststage_binding as hb
        self.clip, self.hb = clip, hb
        w, h = clip.w, clip.h
        hs = hb.HostStage(w, h, clip.bpp)
        hs.preinit(preinit)
        self.key_of, self.key_pic, self.lit, self.mask, self.verdict_p = [], {}, {}, {}, {}
        self.motion_share = {}
        nbx = (w + 15) // 16
        before = None
        for t, (src, key) in enumerate(zip(clip.chunks, clip.keys)):
            if key:
                d = hs.decode(True, src)
                assert d["status"] == 0 and d["kind"] in (hb.KIND_FLAT, hb.KIND_INTRA), (t, d["error"])
                self.key_of.append(t)
                self.key_pic[t] = hb.expand_iframe(d, w, h).reshape(h, w)
            else:
                hs.set_dst_column(before.reshape(h, w)[:, w - 1].astype(np.int32))
                d = hs.decode(False, src)
                assert d["status"] == 0, (t, d["error"])
                self.key_of.append(self.key_of[-1])
                self.verdict_p[t] = d["significant"]
                if d["kind"] == hb.KIND_INTER:
                    moved = sum(1 for b in d["blocks"] if b[0] & hb.PB_MOTION)
                    self.motion_share[t] = moved / len(d["blocks"])
                    d = hs.literalise_motion(d)
                    lit, mask = np.zeros((h, w), np.uint32), np.zeros((h, w), bool)
                    for bi in np.nonzero(d["blocks"][:, 0])[0]:
                        b = d["blocks"][bi]
                        assert not (b[0] & hb.PB_MOTION) and (b[0] & hb.PB_DATA), (t, bi)
                        x1, y1, x2, y2 = (int(v) for v in b[1:5])
                        off = int(np.frombuffer(b[12:16].tobytes(), dtype=np.uint32)[0])
                        assert off % 4 == 0, "a rectangle's literals start on a 16-byte boundary"
                        by, bx = divmod(int(bi), nbx)
                        ys, xs = slice(by * 16 + y1, by * 16 + y2), slice(bx * 16 + x1, bx * 16 + x2)
                        lit[ys, xs] = d["payload"][off:off + (y2 - y1) * (x2 - x1)].reshape(y2 - y1, x2 - x1)
                        mask[ys, xs] = True
                    self.lit[t], self.mask[t] = lit, mask
            before = self.picture(t)   # (what the next frame's destination holds: its last column is the one read of it)
        hs.close()

    def picture(self, t: int) -> np.ndarray:
        k = self.key_of[t]
        out = self.key_pic[k].copy()
        covered = np.zeros(out.shape, bool)
        for f in range(t, k, -1):   # most recent first: the first rectangle to cover a pixel is its last writer
            if f not in self.mask:
                continue               # an unchanged frame
            take = self.mask[f] & ~covered
            out[take] = self.lit[f][take]
            covered |= self.mask[f]
            if covered.all():
                break
        return out.reshape(-1)
