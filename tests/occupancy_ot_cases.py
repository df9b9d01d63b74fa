"""A literal Python transcription of the .ot format (include/sbm.h, "occupancy map: the .ot format"): octomap's
AbstractOcTree::write / read for an OcTree as this library states them. TEST INFRASTRUCTURE ONLY, no GPU, no library.

    write(voxels, resolution)  -> bytes: the stream of the pruned LOGODDS tree over {packed key: float32}
    body(tree)                 -> bytes: 5 bytes per node of an occupancy_tree_cases.Tree, pre-order
    parse(data, map_resolution=None) -> Parsed: status, resolution, size, nodes, leaves [(first Morton code, depth, value bits)]
    leaf_arrays(parsed)        -> (first packed keys uint64, depths int32, value bits uint32): what sbm_occ_ot_leaves returns
    expand(parsed)             -> (packed keys ascending, float32 values): the loaded map, what fetch_logodds returns
    records(tree)              -> nested (value, [None | subtree] * 8) -> body; random_tree(rng, ...) for round trips
    hand_built() / malformed(good)   the streams of tests/golden/occupancy_ot.npz
"""
import struct

import numpy as np

from occupancy_load_cases import NULL, OCC_FULL, OK, SIZE, UNSUPPORTED, Parsed as _BtParsed, _header, expand_leaves  # noqa: F401
from occupancy_tree_cases import DEPTH, Tree, centre_key

MAGIC = b"# Octomap OcTree file"
HEADER = "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\nid OcTree\nsize %d\nres %g\ndata\n"
FAN, SCAN_TILE = 16, 1024      # SBM_OCC_OT_FAN, SBM_OCC_OT_SCAN_TILE of include/sbm.h: the device parse's tile constants


def bits(v):
    return int(np.float32(v).view(np.uint32))


def body(tree):
    """Every node of the pruned tree in depth-first pre-order: its float, then the mask of its children (0 for a leaf)"""
    out = bytearray()
    for code, d, v, leaf in tree._walk(DEPTH, True):
        mask = 0
        if not leaf:
            for c in range(8):
                if (code << 3 | c) in tree.level[d + 1]:
                    mask |= 1 << c
        out += struct.pack("<IB", bits(v), mask)
    return bytes(out)


def stream(size, data, resolution=0.1):
    return (HEADER % (size, resolution)).encode() + bytes(data)


def write(voxels, resolution=0.1):
    tree = Tree(voxels, resolution)
    return stream(tree.size, body(tree), resolution)


class Parsed(_BtParsed):
    """leaves: (first Morton code, depth, value bits)"""

    @property
    def occupied(self):
        raise AttributeError("an .ot leaf holds a value")

    @property
    def value_range(self):
        v = np.array([b for _, _, b in self.leaves], np.uint32).view(np.float32)
        return (float(v.min()), float(v.max())) if len(v) else (0.0, 0.0)


def printed(resolution):
    return float("%g" % resolution)


def parse(data, map_resolution=None):
    """read() as the header section states it. The checks in their order: first line, header tokens, id, res, the map's
    resolution, 5 * size against the body, the tree's shape over the first `size` records, then the leaf values."""
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
    if st == OK and map_resolution is not None and p.resolution != printed(map_resolution):
        st = SIZE
    if st == OK and 5 * p.size > len(b) - pos:
        st = SIZE
    if st == OK and p.size > 0:
        at = [0]
        bad_value = [False]

        def node(code, depth):
            if at[0] >= p.size:
                return SIZE                    # still open after `size` records
            value, mask = struct.unpack_from("<IB", b, pos + 5 * at[0])
            at[0] += 1
            if not mask:
                if (value & 0x7F800000) == 0x7F800000:
                    bad_value[0] = True        # NaN or infinite
                p.leaves.append((code << (3 * (DEPTH - depth)), depth, value))
                return OK
            if depth >= DEPTH:
                return SIZE                    # a child bit at depth 16
            for c in range(8):
                if mask >> c & 1:
                    st = node(code << 3 | c, depth + 1)
                    if st != OK:
                        return st
            return OK

        st = node(0, 0)
        p.nodes = at[0]
        if st == OK and p.nodes != p.size:
            st = SIZE                          # the tree completes before `size` records
        if st == OK and bad_value[0]:
            st = UNSUPPORTED
    p.status = st
    return p


def leaf_arrays(p):
    return (np.array([centre_key(code, DEPTH) for code, _, _ in p.leaves], np.uint64), np.array([d for _, d, _ in p.leaves], np.int32),
            np.array([v for _, _, v in p.leaves], np.uint32))


def centre_leaves(p):
    return (np.array([centre_key(code >> (3 * (DEPTH - d)), d) for code, d, _ in p.leaves], np.uint64),
            np.array([d for _, d, _ in p.leaves], np.int32))


def expand(p):
    return expand_leaves([c for c, _, _ in p.leaves], [d for _, d, _ in p.leaves],
                         np.array([v for _, _, v in p.leaves], np.uint32).view(np.float32))


# ---- streams made by hand: a record tree is (value, [child or None] * 8) --------------------------------------------------------
def leaf(value):
    return (value, [None] * 8)


def records(node):
    out = []

    def walk(n):
        value, kids = n
        out.append(struct.pack("<IB", bits(value), sum(1 << c for c in range(8) if kids[c] is not None)))
        for k in kids:
            if k is not None:
                walk(k)

    walk(node)
    return b"".join(out)


def count(node):
    return 1 + sum(count(k) for k in node[1] if k is not None)


def of_records(node, resolution=0.1):
    return stream(count(node), records(node), resolution)


def chain(children, value=0.5, inner=0.5, bottom=None):
    """single children down from the root: children[d] is the child index taken at depth d; `bottom` or a leaf ends it"""
    node = bottom if bottom is not None else leaf(value)
    for c in reversed(children):
        kids = [None] * 8
        kids[c] = node
        node = (inner, kids)
    return node


def comb(teeth, tail=7, value=0.25):
    """A deep, narrow tree with about 17 * teeth records and `teeth` + 1 voxels: the root's child 0 holds `teeth` depth-16 chains
    that fork at successive depths of one spine, and the root's child `tail` is one more chain, whose parent search goes all the
    way back to record 0."""
    def spine(d, left):
        """subtree at depth d on the spine with `left` teeth to place"""
        if d == DEPTH:
            return leaf(value)
        kids = [None] * 8
        if left > 1 and d < DEPTH - 1:
            per = max(1, left // 2)
            kids[1] = spine(d + 1, per)
            kids[2] = spine(d + 1, left - per)
        else:
            kids[3] = spine(d + 1, 1)
        return (value, kids)

    kids = [None] * 8
    kids[0] = spine(1, teeth)
    kids[tail] = chain([5] * (DEPTH - 1), value, value)
    return (value, kids)


def sized(n, depth=0, value=0.25):
    """A record tree of exactly n records whose leaves are all depth 16 (n = 1: a childless root), deep rather than wide"""
    if n == 1 and depth in (0, DEPTH):
        return leaf(value)
    lo = DEPTH - depth                                  # the records of the smallest subtree one depth down: a chain
    hi = sum(8 ** k for k in range(DEPTH - depth))      # and of the largest
    rest = n - 1
    assert lo <= rest <= 8 * hi, (n, depth)
    c = max(min(8, rest // lo), -(-rest // hi))
    kids = [None] * 8
    for k in range(c):
        kids[k] = sized(rest // c + (1 if k < rest % c else 0), depth + 1, value)
    return (value, kids)


def of_voxels(voxels, inner=0.0):
    """The unpruned record tree of {packed key: float32}: every voxel a depth-16 leaf, inner values `inner` (a reader keeps none)"""
    from occupancy_ray_cases import morton
    root = (inner, [None] * 8)
    for key, v in voxels.items():
        code, node = morton(int(key)), root
        for d in range(DEPTH):
            c = code >> (3 * (DEPTH - 1 - d)) & 7
            if node[1][c] is None:
                node[1][c] = leaf(v) if d == DEPTH - 1 else (inner, [None] * 8)
            node = node[1][c]
    return root


def unpruned(codes, values, resolution=0.1):
    """of_records(of_voxels(...)) for many voxels, in numpy: distinct depth-16 Morton codes and their float32 values -> the
    stream with every voxel a depth-16 leaf and inner values 0"""
    codes = np.asarray(codes, np.uint64)
    order = np.argsort(codes)
    codes, values = codes[order], np.asarray(values, np.float32)[order]
    first, depth, mask, value = [], [], [], []
    for d in range(DEPTH + 1):
        pref = np.unique(codes >> np.uint64(3 * (DEPTH - d)))
        m = np.zeros(len(pref), np.uint8)
        if d < DEPTH:
            child = np.unique(codes >> np.uint64(3 * (DEPTH - d - 1)))
            np.bitwise_or.at(m, np.searchsorted(pref, child >> np.uint64(3)), (1 << (child & np.uint64(7)).astype(np.uint8)).astype(np.uint8))
        first.append(pref << np.uint64(3 * (DEPTH - d)))
        depth.append(np.full(len(pref), d, np.uint8))
        mask.append(m)
        value.append(values.view(np.uint32) if d == DEPTH else np.zeros(len(pref), np.uint32))
    first, depth, mask, value = (np.concatenate(x) for x in (first, depth, mask, value))
    pre = np.lexsort((depth, first))                    # pre-order: by first code, the shallower node first
    rec = np.zeros(len(pre), np.dtype([("v", "<u4"), ("m", "u1")]))
    rec["v"], rec["m"] = value[pre], mask[pre]
    return stream(len(rec), rec.tobytes(), resolution)


def search_levels(n):
    """The levels of the device parse's minima hierarchy over n records: lengths n, ceil(n / FAN), ... down to 1"""
    lens = [n]
    while lens[-1] > 1:
        lens.append(-(-lens[-1] // FAN))
    return lens


def random_tree(rng, depth=0, p_child=0.3, max_depth=DEPTH):
    """A random record tree (not necessarily what prune() would leave: a reader takes any)"""
    if depth == max_depth or (depth > 0 and rng.random() < 0.35):
        return leaf(np.float32(rng.normal()))
    kids = [random_tree(rng, depth + 1, p_child, max_depth) if rng.random() < p_child else None for _ in range(8)]
    if all(k is None for k in kids):
        kids[int(rng.integers(8))] = random_tree(rng, depth + 1, p_child, max_depth)
    return (np.float32(rng.normal()), kids)


def hand_built():
    """{name: stream}: well-formed streams no scan produces"""
    eight = (1.0, [leaf(np.float32(0.1 * c - 0.3)) for c in range(8)])
    outside = chain([4] * 15, inner=9.0, bottom=(9.0, [leaf(9.0), leaf(-7.5), None, None, leaf(-3.0), None, None, None]))
    inner_ok = (0.75, [None, chain([2] * 14, 0.75, 0.75), None, None, None, None, chain([6, 1] * 7, -0.5, -0.5), None])
    inner_wrong = (123.0, [None, chain([2] * 14, 0.75, -55.0), None, None, None, None, chain([6, 1] * 7, -0.5, 3.0), None])
    return {"childless_root": of_records(leaf(0.5)), "chain16": of_records(chain([7, 0, 3, 5] * 4, 1.25, 1.25)),
            "eight_leaves": of_records(eight), "outside_clamps": of_records(outside), "inner_right": of_records(inner_ok),
            "inner_wrong": of_records(inner_wrong)}


def malformed(good):
    """The streams a reader must refuse, from `good` (a stream of at least three records) -> {name: (stream, status)}"""
    head = good[:good.index(b"data\n") + 5]
    data = good[len(head):]
    size = parse(good).size
    assert size >= 3 and len(data) == 5 * size
    deep = chain([0] * 16)                      # ... whose depth-16 record gets a child bit
    deep_bytes = bytearray(records(deep))
    deep_bytes[-1] = 0x10
    nan = bytearray(data)
    last_leaf = max(i for i in range(size) if data[5 * i + 4] == 0)
    nan[5 * last_leaf:5 * last_leaf + 4] = struct.pack("<I", 0x7FC00000)
    early = bytearray(data)                     # the root loses its children: the tree completes after one record
    early[4] = 0
    resize = lambda s: good.replace(b"size %d\n" % size, b"size %d\n" % s)   # noqa: E731
    return {
        "cut_in_record": (good[:len(head) + 5 * (size - 1) + 3], SIZE),
        "cut_between_records": (good[:len(head) + 5 * (size - 1)], SIZE),
        "cut_in_header": (good[:len(head) - 9], SIZE),
        "size_plus_one": (resize(size + 1) + bytes(5), SIZE),            # with five more bytes, so that the shape decides
        "size_minus_one": (resize(size - 1), SIZE),
        "depth17": (stream(17, deep_bytes), SIZE),
        "complete_early": (head + bytes(early), SIZE),
        "color_id": (good.replace(b"id OcTree", b"id ColorOcTree"), UNSUPPORTED),
        "bt_first_line": (good.replace(MAGIC, b"# Octomap OcTree binary file"), UNSUPPORTED),
        "res_zero": (good.replace(b"res 0.1", b"res 0"), SIZE),
        "nan_leaf": (head + bytes(nan), UNSUPPORTED),
    }


def fixture():
    import pathlib
    return dict(np.load(pathlib.Path(__file__).resolve().parent / "golden" / "occupancy_ot.npz"))
