"""The clips, runs and references of the distance-map tests (a helper module, numpy only, no tests of its own): what
test_index_distance_gpu.py and test_sp_index_distance_gpu.py ask the GPU for, and what test_index_distance_ref_cpu.py holds against
a brute-force compare of the oracle's whole pictures first.  Everything is built once a process and nobody changes it.

MSVideo1: msv1_range_clips.long_clip(seed=5, n=96), an index over MSV1_N = 72 frames from clip frame 0 (nothing before the index)
or 3 (a picture before it), at MSV1_SIZES; msv1_tight_clips.directed at 12 x 8 and 128 x 128 (blocks that take an earlier picture
again, blocks that change in one pixel).  ScreenPressor: the five clips of sp_activity_clips and two generated ones."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import index_activity_ref as ar
import index_distance_ref as dr
import sp_activity_clips as ac
import sp_index_ref as ref
from msv1_range_clips import long_clip, truth_run

# ---- MSVideo1 ------------------------------------------------------------------------------------------------------------------
MSV1_N = 72            # words 0, 1, 2 of the bitmap; the key frame at 70 repaints the picture as it is
MSV1_STARTS = (0, 3)
MSV1_SIZES = (
    (64, 32),          # whole cells
    (52, 28),          # edge cells with dead lanes
    (54, 30),          # remainder pixels
    (272, 16),         # 17 cell columns: two workgroups, a tail group that leaves
    (8, 8),            # smaller than a cell
    (3, 3),            # no block: every element 0, for either kind of reference
)
MSV1_PICTURE_AT = 40   # the device picture of the tests is P(40)
REMAINDER_POISON = 0x0BADF00D


def msv1_runs(n=MSV1_N):
    return ((0, n), (1, 1), (31, 3), (32, 33), (n - 1, 1))


def msv1_ref_frames(n=MSV1_N):
    return (-1, 0, 31, 32, n - 1)


@lru_cache(maxsize=None)
def msv1_case(bits, w, h, start, n=MSV1_N):
    """The clip, its plan and THE PICTURES P(-1), P(0) .. P(n - 1) of the index over clip frames start .. start + n - 1, from the
    oracle's sequential run."""
    frames, keys, pal, plan = long_clip(bits, w, h, seed=5, n=96)
    assert not plan["raises"]
    truth = truth_run(bits, w, h, pal, frames[:start + n], keys[:start + n], plan["lines"], key_row=plan["lines"])
    assert all(t is not None for t in truth)
    pics = [t[0] for t in truth]
    coded = plan["coded"]
    p_before, p = ar.msv1_pictures(pics[start:], coded[start:start + n], w, h, pics[start - 1] if start > 0 else None)
    p_before = np.asarray(p_before, dtype=np.int32)
    p = [np.asarray(x, dtype=np.int32) for x in p]
    for x in [p_before] + p:
        x.setflags(write=False)
    return SimpleNamespace(bits=bits, w=w, h=h, start=start, n=n, frames=frames, keys=keys, pal=pal, lines=plan["lines"],
                           coded=coded[start:start + n], p_before=p_before, p=p)


@lru_cache(maxsize=None)
def msv1_pictures_for(bits, w, h, start):
    """The device pictures a case is compared with: name -> (h * w,) int32.
      frame      P(MSV1_PICTURE_AT);
      poisoned   the same with its X % 4 / Y % 4 remainder pixels poisoned: the same map;
      random     P(MSV1_PICTURE_AT) with a random half of its pixels replaced by random words, remainder pixels included."""
    c = msv1_case(bits, w, h, start)
    base = c.p[MSV1_PICTURE_AT]
    poisoned = np.where(dr.whole_block_mask(w, h).reshape(-1), base, np.int32(REMAINDER_POISON)).astype(np.int32)
    rng = np.random.default_rng(1000 * w + h + bits + start)
    noise = rng.integers(0, 1 << 32, size=w * h, dtype=np.uint64).astype(np.uint32).view(np.int32)
    random = np.where(rng.random(w * h) < 0.5, noise, base).astype(np.int32)
    out = {"frame": base, "poisoned": poisoned, "random": random}
    for x in out.values():
        x.setflags(write=False)
    return out


def msv1_reference(c, ref):
    """R of a case: `ref` a frame number (-1: the picture before the index) or the name of a device picture."""
    if isinstance(ref, str):
        return msv1_pictures_for(c.bits, c.w, c.h, c.start)[ref]
    return dr.msv1_reference(c.p_before, c.p, ref)


@lru_cache(maxsize=None)
def msv1_truth(bits, w, h, start, ref):
    """THE DEFINITION over the whole index of a case against one reference: (n, rows, cols) uint16."""
    c = msv1_case(bits, w, h, start)
    out = dr.distance(c.p, msv1_reference(c, ref), w, h, whole_blocks_only=True)
    out.setflags(write=False)
    return out


def msv1_references():
    return msv1_ref_frames() + ("frame", "poisoned", "random")


def cells_of_blocks(blocks, w, h):
    """The cells (r, q) of the grid that hold the 4 x 4 blocks `blocks` (table order), with how many of them each holds."""
    nbx = w // 4
    out = {}
    for b in blocks:
        at = ((b // nbx) // 4, (b % nbx) // 4)
        out[at] = out.get(at, 0) + 1
    return out


def coded_cells(coded, w, h):
    """(n, nb) bool, which frame codes which block -> (n, rows, cols) bool, which frame codes a block of which cell."""
    cols, rows = ar.grid(w, h)
    nbx, nby = w // 4, h // 4
    out = np.zeros((coded.shape[0], rows, cols), dtype=bool)
    for b in range(nbx * nby):
        out[:, (b // nbx) // 4, (b % nbx) // 4] |= coded[:, b]
    return out


MSV1_DIRECTED_SIZES = ((12, 8), (128, 128))
MSV1_DIRECTED_REFS = (1, 4)   # frame 1: `back` (4) returns to it at the spots; frame 4: `one_pixel` (5) is one pixel a block away


@lru_cache(maxsize=None)
def msv1_directed(bits, w, h):
    """msv1_tight_clips.directed(bits, w, h), indexed from frame 0: the clip and THE PICTURES from the oracle's run."""
    import msv1_tight_clips as tc
    from msv1_range_clips import make_plan, palette
    clip, pal = tc.directed(bits, w, h), palette(bits)
    truth = truth_run(bits, w, h, pal, clip.frames, clip.keys, 36, key_row=36)
    assert all(t is not None for t in truth)
    coded = make_plan(bits, w, h, clip.frames, clip.keys, 36)["coded"]
    p_before, p = ar.msv1_pictures([t[0] for t in truth], coded, w, h, None)
    p = [np.asarray(x, dtype=np.int32) for x in p]
    for x in p:
        x.setflags(write=False)
    return SimpleNamespace(bits=bits, w=w, h=h, start=0, n=len(p), frames=clip.frames, keys=clip.keys, pal=pal, lines=36, coded=coded,
                           p_before=np.asarray(p_before, dtype=np.int32), p=p, clip=clip)


@lru_cache(maxsize=None)
def msv1_directed_truth(bits, w, h, ref):
    c = msv1_directed(bits, w, h)
    out = dr.distance(c.p, c.p[ref], w, h, whole_blocks_only=True)
    out.setflags(write=False)
    return out


# ---- ScreenPressor ---------------------------------------------------------------------------------------------------------------
# The five clips of sp_activity_clips have an event in every block at every frame (the beat; a key frame): no value of theirs is ever
# stored for a frame without an event.  Two generated clips of test_sp_index_gpu.CLIPS (unchanged frames, blocks that rest) stand
# beside them for the repeat store: name -> make_clip's arguments.
SP_GENERATED = {
    "gen_37x23": (53, 37, 23, 41, 24, 2, 13, 5),     # X % 4 != 0: the scalar path
    "gen_64x48": (56, 64, 48, 41, 16, 3, 13, 36),    # the vector path
}
SP_NAMES = ac.NAMES + tuple(SP_GENERATED)
# (reference, the frame the region is restored at) of sp_activity_clips: the frame before each ZERO_AT
SP_RETURNS = tuple((z - 1, r) for z, r in zip(ac.ZERO_AT, ac.RESTORE_AT))
SP_PICTURE_AT = {True: 50, False: 20}   # the device picture of a clip is made from this frame (directed: True)


@lru_cache(maxsize=None)
def sp_case(name):
    """clip (sp_index_ref.Clip), key_row (also the codec's Preinit lines), pictures P(0) .. P(n - 1) of the oracle's sequential run."""
    if name in SP_GENERATED:
        clip = ref.make_clip(*SP_GENERATED[name])
        pictures = ref.oracle_run(clip, preinit=clip.key_row)[0]
        return SimpleNamespace(name=name, clip=clip, key_row=clip.key_row, pictures=pictures, n=len(clip.keys), directed=False)
    clip = ac.clip(name)
    return SimpleNamespace(name=name, clip=clip, key_row=ac.KEY_ROW, pictures=ac.oracle(name)[0], n=ac.N, directed=True)


@lru_cache(maxsize=None)
def sp_composer(name):
    c = sp_case(name)
    return ac.composer(name) if c.directed else ref.Composer(c.clip, preinit=c.key_row)


def sp_ref_frames(name):
    """-1 and 0; the directed clips: the frame before each ZERO_AT, 31, 32 and 63 (key frames at bit 0 and bit 31), REPEAT_AT; the
    generated ones: their key frames, the frame before one and a frame in the middle of a key interval."""
    if sp_case(name).directed:
        return tuple(sorted({-1, 0, 31, 32, 63, ac.REPEAT_AT} | {r for r, _ in SP_RETURNS}))
    keys = [t for t, k in enumerate(sp_case(name).clip.keys) if k]
    return tuple(sorted({-1, 0, 20, sp_case(name).n - 1} | set(keys[1:4]) | {k - 1 for k in keys[1:3]}))


def sp_references(name):
    return sp_ref_frames(name) + ("picture",)


def sp_runs(name):
    """Runs that start on a key frame, before one and behind one, a run of one frame, the whole clip."""
    n = sp_case(name).n
    if sp_case(name).directed:
        return ((0, n), (32, 8), (63, 3), (30, 5), (19, 3), (33, 31), (65, 5), (17, 1), (n - 1, 1), (1, 62))
    k = [t for t, key in enumerate(sp_case(name).clip.keys) if key][1]
    return ((0, n), (k, 8), (k - 2, 5), (k + 1, 20), (3, 1), (n - 1, 1), (1, n - 2))


@lru_cache(maxsize=None)
def sp_picture_for(name):
    """The device picture of a clip: P(SP_PICTURE_AT) with every seventh pixel of the picture's left half given a word no frame
    holds — the cells of the right half show the frame itself, so that some elements are 0.  A picture of one cell (13 x 9) is
    the frame as it is: with a foreign word anywhere its only cell would never be 0."""
    c = sp_case(name)
    w, h = c.clip.w, c.clip.h
    pic = np.asarray(c.pictures[SP_PICTURE_AT[c.directed]]).view(np.uint32).copy()
    cols, rows = ar.grid(w, h)
    if (cols, rows) != (1, 1):
        assert cols > 1
        ys, xs = np.nonzero(np.ones((h, 16 * (cols // 2)), dtype=bool))   # whole cell columns: the left half, rounded down
        pic.reshape(h, w)[ys[::7], xs[::7]] = 0x7E57ED
    pic.setflags(write=False)
    return pic


def sp_reference(name, ref_):
    c = sp_case(name)
    if isinstance(ref_, str):
        return sp_picture_for(name)
    return np.zeros(c.clip.w * c.clip.h, dtype=np.uint32) if ref_ < 0 else np.asarray(c.pictures[ref_]).view(np.uint32)


@lru_cache(maxsize=None)
def sp_truth(name, ref_):
    """THE DEFINITION over the whole clip against one reference: (n, rows, cols) uint16."""
    c = sp_case(name)
    out = dr.distance(c.pictures, sp_reference(name, ref_), c.clip.w, c.clip.h)
    out.setflags(write=False)
    return out
