"""Inputs for the occupancy map's data-structure tests whose expected result is a closed form, independent of
oracle/occupancy_ref.c. TEST INFRASTRUCTURE ONLY, no GPU.

Under a pose whose rotation block is zero the world point of every valid pixel is the pose's translation, exactly:
0*x + 0*y + 0*z + o equals o in float for finite x, y, z, and the norm of (point - origin) is 0. So n planes of 1 x 1 pixels at
disparity 160, each with its own translation, put exactly one chosen key per plane into the map:

    axis key = floor((1.0 / resolution) * float64(float32(t))) + 32768, kept iff 0 <= key < 65536 on every axis
    expected (keys, hits) = np.unique(packed kept keys, return_counts=True)

    closed_form(t, resolution)           -> (keys uint64 ascending, hits uint32) of translations t (n, 3)
    zero_rotation_poses(t)               -> float32 (n, 12)
    unit_planes(n)                       -> int16 (n, 1, 1), every pixel valid
    planes_for_keys(keys, mult, seed)    -> (planes, poses): key i on mult[i] planes, in a shuffled order
    lattice_case(n_distinct, seed, ends) -> (planes, poses, keys, hits): exactly n_distinct keys over the 48-bit range
    lattice(n)                           -> the lattice case of n keys the tests use (LATTICE_SIZES), made once, read-only
    one_byte_case(byte)                  -> the same for keys that differ in one byte only
    PATTERNS / pattern(name)             -> single planes with a per-wavefront key pattern, for the leader reduction
"""
import functools

import numpy as np

RESOLUTION = 0.1
VALID = 160                      # a disparity of 10 px: any valid pixel does
KEY_MAX = (1 << 48) - 1          # the largest packed key: k0 = k1 = k2 = 65535. NOT the empty word, which is all 64 ones
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def pack(k):
    k = np.asarray(k, np.uint64).reshape(-1, 3)
    return (k[:, 0] << np.uint64(32)) | (k[:, 1] << np.uint64(16)) | k[:, 2]


def unpack(keys):
    keys = np.asarray(keys, np.uint64).reshape(-1)
    m = np.uint64(0xFFFF)
    return np.stack([(keys >> np.uint64(32)) & m, (keys >> np.uint64(16)) & m, keys & m], axis=1).astype(np.int64)


def closed_form(t, resolution=RESOLUTION):
    t = np.asarray(t, np.float32).reshape(-1, 3)
    k = np.floor((1.0 / resolution) * t.astype(np.float64)) + 32768.0
    keep = ((k >= 0) & (k < 65536)).all(axis=1)
    keys, hits = np.unique(pack(k[keep].astype(np.int64)), return_counts=True)
    return keys.astype(np.uint64), hits.astype(np.uint32)


def zero_rotation_poses(t):
    t = np.asarray(t, np.float32).reshape(-1, 3)
    poses = np.zeros((len(t), 12), np.float32)
    poses[:, 3], poses[:, 7], poses[:, 11] = t[:, 0], t[:, 1], t[:, 2]
    return poses


def unit_planes(n):
    return np.full((n, 1, 1), VALID, np.int16)


def key_centres(keys, resolution=RESOLUTION):
    """The centre of each key's voxel as float32: half a cell from every face, about 200 float32 roundings at 3276 m."""
    return ((unpack(keys) - 32768 + 0.5) * resolution).astype(np.float32)


def planes_for_keys(keys, mult, seed, resolution=RESOLUTION):
    t = np.repeat(key_centres(keys, resolution), np.asarray(mult, np.int64), axis=0)
    t = t[np.random.default_rng(seed).permutation(len(t))]
    return unit_planes(len(t)), zero_rotation_poses(t)


def multiplicity(n):
    """1 2 3 1 2 3 ... along the ascending keys: neighbours in the sorted order never carry the same count."""
    return (1 + np.arange(n) % 3).astype(np.uint32)


def lattice_case(n_distinct, seed, ends=False):
    """Exactly n_distinct keys uniform over the whole 48-bit range (with ends: key 0 and KEY_MAX among them), key i of the
    ascending order on 1 + i % 3 planes -> (planes, poses, expected keys, expected hits)."""
    rng = np.random.default_rng(seed)
    keys = np.array([0, KEY_MAX][:n_distinct] if ends else [], np.uint64)
    while len(keys) < n_distinct:
        more = rng.integers(0, 1 << 48, n_distinct - len(keys), dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, more]))
    hits = multiplicity(n_distinct)
    planes, poses = planes_for_keys(keys, hits, seed + 1)
    return planes, poses, keys, hits


SORT_SHAPES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)   # a wavefront step, a tile, a last tile of one key; every digit
MANY_TILES = 70000                                            # 69 tiles: the scan's serial walk along a digit's row
PAST_CAPACITY = (1500, 2000, 2300)                            # into 2048 slots, where the bound of 1024 probes binds
WITH_ENDS = 5000                                              # this case holds key 0 and KEY_MAX
LATTICE_SIZES = SORT_SHAPES + (MANY_TILES,) + PAST_CAPACITY + (3,)


@functools.lru_cache(maxsize=None)
def lattice(n):
    case = lattice_case(n, seed=n, ends=n == WITH_ENDS)
    for a in case:
        a.setflags(write=False)
    return case


ONE_BYTE_BASE = 0x5AC3963CA569


def one_byte_case(byte, n_planes=300):
    """Keys that differ in byte `byte` (0 = lowest) only. A byte has 256 values: all of them, the first n_planes - 256 of the
    ascending order on two planes -> (planes, poses, expected keys, expected hits)."""
    base = ONE_BYTE_BASE & ~(0xFF << (8 * byte))
    keys = np.array([base | (d << (8 * byte)) for d in range(256)], np.uint64)
    hits = np.ones(256, np.uint32)
    hits[:n_planes - 256] = 2
    planes, poses = planes_for_keys(keys, hits, 100 + byte)
    return planes, poses, keys, hits


# ---- leader reduction: single planes under an identity rotation and the default model (fx = fy = 400, cx = 320, cy = 240,
# baseline 0.12: z = 48 / d, x = (col - 320) * z / 400). The restatement gives the expected map; tests/test_occupancy_restatement
# reads the structure each plane claims off occupancy_ref.pixel_keys. Close to the camera 64 columns span less than a voxel, so a
# pixel's voxel is chosen by its disparity; the translation keeps the points away from voxel faces.

def _d16(z):
    return int(round(16 * 48.0 / z))


def _pose(t):
    p = np.asarray(IDENTITY, np.float32).copy()
    p[3], p[7], p[11] = t
    return p[None]


def pattern(name):
    """-> (plane int16 (h, w), pose (1, 12)); scale 1."""
    if name == "abab":                       # two disparities alternating by column: two keys interleaved across the wavefront
        plane = np.where(np.arange(64) % 2 == 0, _d16(0.3), _d16(0.4)).astype(np.int16)[None]
        return plane, _pose((-0.05, 0.03, 0.05))
    if name == "runs":                       # K K - K K - per 6 lanes: a run of 4 with an invalid lane inside and one behind it
        z = 0.1 + 0.1 * (np.arange(128) // 6 % 5)
        plane = np.array([_d16(v) for v in z], np.int16)
        plane[np.arange(128) % 6 == 2] = 0
        plane[np.arange(128) % 6 == 5] = -16
        return plane[None], _pose((0.02, 0.03, 0.05))
    if name in ("tail65", "tail129"):        # the last wavefront holds one lane, with the key of lane 0 of the first
        w = int(name[4:])
        plane = np.array([_d16(0.2 + 0.1 * (c % 7)) for c in range(w)], np.int16)
        plane[0] = plane[-1] = _d16(0.1)
        return plane[None], _pose((-0.08 if w == 65 else 0.01, 0.03, 0.05))
    if name == "blocks":                     # 3 x 100 at one disparity: the voxel of the right-hand columns has pixels in
        plane = np.full((3, 100), _d16(0.3), np.int16)   # wavefronts 0..3 of block 0 and in block 1 (pixels 256..299)
        return plane, _pose((0.0, 0.03, 0.05))
    raise KeyError(name)


PATTERNS = ("abab", "runs", "tail65", "tail129", "blocks")
