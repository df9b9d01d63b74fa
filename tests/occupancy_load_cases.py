"""A literal Python transcription of the .bt reader (include/sbm.h, "occupancy map: load a .bt stream"): octomap's readBinary as
this library states it, down to the leaves of the pruned tree and the depth-16 voxels below them. TEST INFRASTRUCTURE ONLY, no
GPU, no library.

    parse(data)            -> Parsed: status (0, SIZE or UNSUPPORTED), resolution, size, nodes, leaves [(first Morton code, depth,
                              occupied)] in stream order, and the counts of sbm_occ_binary_header
    leaf_arrays(parsed)    -> (first packed keys uint64, depths int32, occupied uint8): what sbm_occ_binary_leaves returns
    centre_leaves(parsed)  -> (centre keys uint64, depths int32): what octomap's begin_leafs() reports for the same leaves
    expand(parsed, cmin, cmax) -> (packed keys uint64 ascending, float32 values): the loaded map, what fetch_logodds returns
    malformed()            -> {name: (stream, status)}: the streams a loader must refuse, built from one good stream
"""
import re

import numpy as np

from occupancy_ray_cases import F
from occupancy_tree_cases import DEPTH, HEADER, centre_key, unmorton

OK, SIZE, UNSUPPORTED, NULL, OCC_FULL = 0, -2, -23, -1, -25
MAGIC = b"# Octomap OcTree binary file"
SPACE = b" \t\n\v\f\r"


class Parsed:
    def __init__(self):
        self.status, self.resolution, self.size, self.nodes, self.leaves = OK, 0.0, 0, 0, []

    @property
    def voxels(self):
        return sum(8 ** (DEPTH - d) for _, d, _ in self.leaves)

    @property
    def occupied(self):
        return sum(1 for _, _, o in self.leaves if o)

    @property
    def leaves_at(self):
        return [sum(1 for _, d, _ in self.leaves if d == k) for k in range(DEPTH + 1)]

    def key_bounds(self):
        lo, hi = [65535] * 3, [0] * 3
        for code, d, _ in self.leaves:
            k = unmorton(code)
            for a in range(3):
                lo[a] = min(lo[a], k[a])
                hi[a] = max(hi[a], k[a] + (1 << (DEPTH - d)) - 1)
        return lo, hi


def _header(b, pos, out):
    """readHeader: tokens up to the line `data` -> (status, position of the body)"""
    n = len(b)

    def skip_line(i):
        while i < n and b[i] != 0x0A:
            i += 1
        return min(i + 1, n)

    def token(i):
        while i < n and b[i] in SPACE:
            i += 1
        j = i
        while j < n and b[j] not in SPACE:
            j += 1
        return b[i:j], j

    ident = b""
    while True:
        t, pos = token(pos)
        if not t:
            return SIZE, pos, ident            # the stream ends inside the header
        if t == b"data":
            return OK, skip_line(pos), ident
        if t[:1] == b"#":
            pos = skip_line(pos)
        elif t == b"id":
            ident, pos = token(pos)
            if not ident:
                return SIZE, pos, ident
        elif t in (b"res", b"size"):
            while pos < n and b[pos] in SPACE:
                pos += 1
            j = pos
            while j < n and b[j] not in SPACE and j - pos < 63:
                j += 1
            text = b[pos:j].decode("latin-1")
            if t == b"res":                    # strtod: the longest prefix that is a number
                m = re.match(r"[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|inf(inity)?|nan)", text, re.I)
                if not m:
                    return SIZE, pos, ident
                out.resolution = float(m.group(0))
            else:
                m = re.match(r"\d+", text)
                if not m or int(m.group(0)) >= 1 << 32:
                    return SIZE, pos, ident
                out.size = int(m.group(0))
            pos += m.end()
        else:
            pos = skip_line(pos)


def parse(data):
    b = bytes(data)
    p = Parsed()
    if b[:len(MAGIC)] != MAGIC:
        p.status = UNSUPPORTED
        return p
    pos = b.find(b"\n")
    pos = len(b) if pos < 0 else pos + 1
    st, pos, ident = _header(b, pos, p)
    if st == OK and ident not in (b"OcTree", b"1"):
        st = UNSUPPORTED
    if st == OK and not p.resolution > 0.0:
        st = SIZE
    if st == OK and p.size > 0:
        p.nodes = 1
        at = [pos]

        def node(code, depth):
            """readBinaryNode: the record of this node, then those of its 11 children in child order"""
            if len(b) - at[0] < 2:
                return SIZE
            word = b[at[0]] | b[at[0] + 1] << 8
            at[0] += 2
            if not word:                       # childless: it keeps the clamp max it was given
                p.leaves.append((code << (3 * (DEPTH - depth)), depth, True))
                return OK
            for c in range(8):
                kind = word >> (2 * c) & 3     # bits (2c, 2c + 1): 1,0 free = 1; 0,1 occupied = 2; 1,1 inner = 3
                if not kind:
                    continue
                p.nodes += 1
                if kind != 3:
                    p.leaves.append(((code << 3 | c) << (3 * (DEPTH - depth - 1)), depth + 1, kind == 2))
                elif depth + 1 >= DEPTH:
                    return SIZE
                else:
                    st = node(code << 3 | c, depth + 1)
                    if st != OK:
                        return st
            return OK

        st = node(0, 0)
    if st == OK and p.nodes != p.size:
        st = SIZE
    p.status = st
    return p


def leaf_arrays(p):
    keys = np.array([centre_key(code, DEPTH) for code, _, _ in p.leaves], np.uint64)
    return keys, np.array([d for _, d, _ in p.leaves], np.int32), np.array([o for _, _, o in p.leaves], np.uint8)


def centre_leaves(p):
    return (np.array([centre_key(code >> (3 * (DEPTH - d)), d) for code, d, _ in p.leaves], np.uint64),
            np.array([d for _, d, _ in p.leaves], np.int32))


def _unmorton_array(codes):
    """unmorton on a uint64 array -> packed keys"""
    codes = np.asarray(codes, np.uint64)
    k = [np.zeros(len(codes), np.uint64) for _ in range(3)]
    for bit in range(DEPTH):
        for a in range(3):
            k[a] |= ((codes >> np.uint64(3 * bit + a)) & np.uint64(1)) << np.uint64(bit)
    return k[0] << np.uint64(32) | k[1] << np.uint64(16) | k[2]


def expand_leaves(codes, depths, values):
    """Leaves (first Morton code, depth, float32 value) -> (packed keys ascending, values) of the voxels below them"""
    parts_c, parts_v = [], []
    for code, d, v in zip(codes, depths, values):
        m = 8 ** (DEPTH - int(d))
        parts_c.append(np.uint64(int(code)) + np.arange(m, dtype=np.uint64))
        parts_v.append(np.full(m, v, np.float32))
    if not parts_c:
        return np.zeros(0, np.uint64), np.zeros(0, np.float32)
    keys, vals = _unmorton_array(np.concatenate(parts_c)), np.concatenate(parts_v)
    order = np.argsort(keys)
    return keys[order], vals[order]


def expand(p, cmin, cmax):
    return expand_leaves([c for c, _, _ in p.leaves], [d for _, d, _ in p.leaves], [F(cmax) if o else F(cmin) for _, _, o in p.leaves])


def expand_centres(keys, depths, values):
    """The same from octomap's centre keys (begin_leafs): the first code is the centre's with the low bits cleared"""
    from occupancy_ray_cases import morton
    codes = [morton(int(k)) >> (3 * (DEPTH - int(d))) << (3 * (DEPTH - int(d))) for k, d in zip(keys, depths)]
    return expand_leaves(codes, depths, values)


def stream(size, body, resolution=0.1):
    return (HEADER % (size, resolution)).encode() + bytes(body)


def malformed(good):
    """The streams a loader must refuse, made from `good` (a stream with at least two records) -> {name: (stream, status)}"""
    head = good[:good.index(b"data\n") + 5]
    body = good[len(head):]
    size = parse(good).size
    deep = bytearray()
    for _ in range(15):                     # a chain of 11 children down to a depth-15 record ...
        deep += bytes((3, 0))
    deep += bytes((3, 0))                   # ... whose child 0 is 11 again: depth 17 (octomap would read on)
    deep += bytes((0, 0))
    return {
        "cut_in_record": (good[:len(head) + 3], SIZE),
        "cut_between_records": (good[:len(head) + 2], SIZE),
        "cut_in_header": (good[:len(head) - 9], SIZE),
        "depth17": (stream(17, deep), SIZE),
        "size_plus_one": (good.replace(b"size %d\n" % size, b"size %d\n" % (size + 1)), SIZE),
        "size_minus_one": (good.replace(b"size %d\n" % size, b"size %d\n" % (size - 1)), SIZE),
        "color_id": (good.replace(b"id OcTree", b"id ColorOcTree"), UNSUPPORTED),
        "no_data": (head.replace(b"data\n", b"") + body, SIZE),
        "res_zero": (good.replace(b"res 0.1", b"res 0"), SIZE),
        "legacy": (np.int32(3).tobytes() + np.float64(0.1).tobytes() + np.uint32(size).tobytes() + body, UNSUPPORTED),
    }


def fixture():
    """tests/golden/occupancy_load.npz and the streams it speaks of -> (fixture dict, {stream id: (bytes, RayParams)}). The
    recorded streams stay where they were recorded: `tree_<name>` is <name>_bt of occupancy_tree.npz, `rays_<name>` of
    occupancy_rays.npz, `octomap_<name>` bt_<name> of occupancy_octomap.npz; size1 is made here."""
    import pathlib

    from occupancy_ray_cases import RayParams
    golden = pathlib.Path(__file__).resolve().parent / "golden"
    fx = dict(np.load(golden / "occupancy_load.npz"))
    src = {n: dict(np.load(golden / f"occupancy_{n}.npz")) for n in ("tree", "rays", "octomap")}
    streams = {}
    for sid in (str(s) for s in fx["streams"]):
        kind, _, name = sid.partition("_")
        if sid == "size1":
            streams[sid] = (stream(1, bytes((0, 0))), RayParams())
        elif kind == "octomap":
            streams[sid] = (src[kind][f"bt_{name}"].tobytes(), RayParams())
        else:
            streams[sid] = (src[kind][f"{name}_bt"].tobytes(), RayParams(*[float(v) for v in src[kind][f"{name}_params"][:5]]))
    return fx, streams
