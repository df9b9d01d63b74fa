"""A literal Python transcription of the occupancy map's colours (include/sbm.h, "occupancy map: colour per voxel"): octomap's
ColorOcTree::setNodeColor and averageNodeColor per depth-16 voxel on top of tests/occupancy_edit_cases.py (whose Tree holds the
voxels), the colour of every node of the pruned tree after prune(); updateInnerOccupancy(); on top of
tests/occupancy_tree_cases.py, and the ColorOcTree stream. TEST INFRASTRUCTURE ONLY, no GPU, no library.

    WHITE, word(r, g, b), rgb(word)         a colour word r | g << 8 | b << 16; white is "no colour set"
    SET, AVERAGE                            the op of a colour batch
    Map(params, resolution)                 ec.Tree with .color(keys, words, op) in item order, .color_points(points, words, op),
                                            .last_color (items, found, unknown, skipped), .colored() -> (keys, log-odds, words)
    ColorTree(voxels, colors, resolution)   tc.Tree with .color[d][code]; .leaves_colors(max_depth); .body(); .stream()
    parse(data, map_resolution)             -> status, leaves [(first Morton code, depth, value bits, colour word)]
    expand(leaves)                          -> (keys ascending, float32 values, colour words): the loaded map
    FX, NAMES, case_of(name), recorded(name), run_case(case), run_counts(case)   tests/golden/occupancy_color.npz
"""
import pathlib
import struct

import numpy as np

import occupancy_edit_cases as ec
import occupancy_ot_cases as otc
import occupancy_ray_cases as rc
import occupancy_tree_cases as tc
from occupancy_load_cases import OK, SIZE, UNSUPPORTED, _header

F = np.float32
WHITE = 0x00FFFFFF
SET, AVERAGE = 0, 1
SCAN, COLOR, SET_VALUES, SNAPSHOT, RESUME, EDIT = 0, 1, 2, 3, 4, 5    # the kinds of a step; EDIT: items with ec.UPDATE / SET / DELETE ops
DEPTHS = (16, 15, 12, 0)                                           # the maxDepth of a snapshot's leaf lists
HEADER = "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\nid ColorOcTree\nsize %d\nres %g\ndata\n"


def word(r, g, b):
    return (int(r) & 255) | (int(g) & 255) << 8 | (int(b) & 255) << 16


def rgb(w):
    return int(w) & 255, int(w) >> 8 & 255, int(w) >> 16 & 255


def step_color(prev, new, op):
    """setColor, or averageNodeColor: the colour itself if none is set, else (prev + new) / 2 per channel in int"""
    new = int(new) & WHITE
    if op == SET or prev == WHITE:
        return new
    return word(*[(a + b) // 2 for a, b in zip(rgb(prev), rgb(new))])


class Map(ec.Tree):
    def __init__(self, rp=None, resolution=0.1):
        super().__init__(rp, resolution)
        self.c = {}                                   # packed key -> colour word, of voxels whose colour is not white
        self.last_color = dict(items=0, found=0, unknown=0, skipped=0)

    def delete_node(self, key, depth=0):
        n = super().delete_node(key, depth)
        for k in [k for k in self.c if k not in self.v]:
            del self.c[k]                             # a deleted voxel goes with its colour: created again, it is white
        return n

    def color(self, keys, words, op):
        """Items in item order: search(key) first, so an unknown voxel is a no-op; a key with a bit above 47 is skipped."""
        found = skipped = 0
        for key, w in zip((int(k) for k in keys), words):
            if key >> 48:
                skipped += 1
            elif key in self.v:
                found += 1
                c = step_color(self.c.get(key, WHITE), w, op)
                if c == WHITE:
                    self.c.pop(key, None)
                else:
                    self.c[key] = c
        self.last_color = dict(items=len(keys), found=found, unknown=len(keys) - found - skipped, skipped=skipped)
        return self

    def color_points(self, points, words, op):
        """The key is coordToKeyChecked; an item whose point has none is skipped."""
        factor = 1.0 / self.resolution
        keys = []
        for p in np.asarray(points, np.float32).reshape(-1, 3):
            k = rc.key3(p, factor)
            keys.append(1 << 48 if k is None else rc.pack3(k))
        return self.color(keys, words, op)

    def colored(self):
        keys, lo = self.leaves()
        return keys, lo, np.array([self.c.get(int(k), WHITE) for k in keys], np.uint32)

    def search_colors(self, points, thres=0.0):
        """-> (state int32, value bits uint32, colour words uint32) of search(point) per point"""
        factor = 1.0 / self.resolution
        st, val, col = [], [], []
        for p in np.asarray(points, np.float32).reshape(-1, 3):
            k = rc.key3(p, factor)
            key = None if k is None else rc.pack3(k)
            if key is None or key not in self.v:
                st.append(tc.CELL_OUT if key is None else tc.CELL_UNKNOWN), val.append(0x7FC00000), col.append(WHITE)
            else:
                v = self.v[key]
                st.append(tc.CELL_OCCUPIED if v >= F(thres) else tc.CELL_FREE), val.append(int(F(v).view(np.uint32))), col.append(self.c.get(key, WHITE))
        return np.array(st, np.int32), np.array(val, np.uint32), np.array(col, np.uint32)

    def tree(self):
        return ColorTree(self.v, self.c, self.resolution)

    def load(self, leaves):
        """AbstractOcTree::read, then what the map holds: every voxel of a leaf's cube with the leaf's float and colour"""
        keys, values, words = expand(leaves)
        self.v = {int(k): F(v) for k, v in zip(keys, values)}
        self.c = {int(k): int(w) for k, w in zip(keys, words) if int(w) != WHITE}
        return self


def average_child_color(words):
    """getAverageChildColor: int sums over the children whose colour is set, divided by their count; white if none is"""
    on = [rgb(w) for w in words if w != WHITE]
    if not on:
        return WHITE
    return word(*[sum(c[a] for c in on) // len(on) for a in range(3)])


class ColorTree(tc.Tree):
    """The colours after prune(); updateInnerOccupancy();, bottom-up over the levels of tc.Tree: a collapsed node takes child 0's
    colour and, if that is set, the average of its children; any other node takes the average of its children."""

    def __init__(self, voxels, colors, resolution=0.1):
        super().__init__(voxels, resolution)
        self.color = [dict() for _ in range(tc.DEPTH + 1)]
        self.color[tc.DEPTH] = {rc.morton(int(k)): int(colors.get(int(k), WHITE)) for k in voxels}
        for d in range(tc.DEPTH - 1, -1, -1):
            for code in self.level[d]:
                kids = [self.color[d + 1][code << 3 | c] for c in range(8) if (code << 3 | c) in self.level[d + 1]]
                if code in self.collapsed[d] and kids[0] == WHITE:
                    self.color[d][code] = WHITE
                else:
                    self.color[d][code] = average_child_color(kids)

    def leaves_colors(self, max_depth=0):
        rows = self._walk(max_depth or tc.DEPTH, False)
        return self._arrays(rows) + (np.array([self.color[d][c] for c, d, _, _ in rows], np.uint32),)

    def body(self):
        """Every node of the pruned tree in pre-order: its float, r, g, b, then the mask of its children (0 for a leaf)"""
        out = bytearray()
        for code, d, v, leaf in self._walk(tc.DEPTH, True):
            mask = 0
            if not leaf:
                for c in range(8):
                    if (code << 3 | c) in self.level[d + 1]:
                        mask |= 1 << c
            out += struct.pack("<I", otc.bits(v)) + bytes(rgb(self.color[d][code])) + bytes([mask])
        return bytes(out)

    def stream(self):
        return (HEADER % (self.size, self.resolution)).encode() + self.body()


class Parsed:
    def __init__(self):
        self.status, self.resolution, self.size, self.nodes, self.leaves = OK, 0.0, 0, 0, []


def parse(data, map_resolution=None):
    """read() of a ColorOcTree stream: occupancy_ot_cases.parse with the other id and eight bytes per record.
    leaves: (first Morton code, depth, value bits, colour word)"""
    b = bytes(data)
    p = Parsed()
    if b[:len(otc.MAGIC)] != otc.MAGIC:
        p.status = UNSUPPORTED
        return p
    pos = b.find(b"\n")
    pos = len(b) if pos < 0 else pos + 1
    st, pos, ident = _header(b, pos, p)
    if st == OK and ident != b"ColorOcTree":
        st = UNSUPPORTED
    if st == OK and not p.resolution > 0.0:
        st = SIZE
    if st == OK and map_resolution is not None and p.resolution != otc.printed(map_resolution):
        st = SIZE
    if st == OK and 8 * p.size > len(b) - pos:
        st = SIZE
    if st == OK and p.size > 0:
        at = [0]
        bad_value = [False]

        def node(code, depth):
            if at[0] >= p.size:
                return SIZE
            value, r, g, bl, mask = struct.unpack_from("<IBBBB", b, pos + 8 * at[0])
            at[0] += 1
            if not mask:
                if (value & 0x7F800000) == 0x7F800000:
                    bad_value[0] = True
                p.leaves.append((code << (3 * (tc.DEPTH - depth)), depth, value, word(r, g, bl)))
                return OK
            if depth >= tc.DEPTH:
                return SIZE
            for c in range(8):
                if mask >> c & 1:
                    st = node(code << 3 | c, depth + 1)
                    if st != OK:
                        return st
            return OK

        st = node(0, 0)
        p.nodes = at[0]
        if st == OK and p.nodes != p.size:
            st = SIZE
        if st == OK and bad_value[0]:
            st = UNSUPPORTED
    p.status = st
    return p


def expand(leaves):
    """-> (packed keys ascending, float32 values, colour words): every voxel of a leaf's cube holds the leaf's float and colour"""
    out = {}
    for first, d, value, w in leaves:
        for m in range(first, first + (1 << (3 * (tc.DEPTH - d)))):
            out[tc.centre_key(m, tc.DEPTH)] = (value, w)
    keys = np.array(sorted(out), np.uint64)
    return (keys, np.array([out[int(k)][0] for k in keys], np.uint32).view(np.float32), np.array([out[int(k)][1] for k in keys], np.uint32))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def apply_step(m, s):
    """One step of a case on a Map -> what the step records: None, or for a snapshot (leaf lists, stream, loaded voxels)"""
    if s["kind"] == SCAN:
        m.insert(s["points"], s["origin"])
    elif s["kind"] == COLOR:
        if s["form"]:
            m.color_points(s["points"], s["words"], s["op"])
        else:
            m.color(s["keys"], s["words"], s["op"])
    elif s["kind"] == SET_VALUES:
        for k, v in zip(s["keys"], s["values"]):
            m.set_node_value(int(k), v)
    elif s["kind"] == EDIT:
        m.edit(s["keys"], s["ops"], s["values"])
    elif s["kind"] == SNAPSHOT:
        t = m.tree()
        data = t.stream()
        return [t.leaves_colors(d) for d in DEPTHS], data, expand(parse(data, m.resolution).leaves)
    elif s["kind"] == RESUME:
        m.load(parse(m.tree().stream(), m.resolution).leaves)
    return None


def run_case(case, resolution=0.1):
    """-> per step: (keys, log-odds, words, found) or, for a snapshot, ([leaf lists], stream, (keys, values, words))"""
    m = Map(case["params"], resolution)
    out = []
    for s in case["steps"]:
        snap = apply_step(m, s)
        out.append(snap if snap is not None else m.colored() + (m.last_color["found"] if s["kind"] == COLOR else 0,))
    return out


def run_counts(case, resolution=0.1):
    """-> per step the counts of its colour batch (items, found, unknown, skipped), None for a step of another kind"""
    m = Map(case["params"], resolution)
    out = []
    for s in case["steps"]:
        apply_step(m, s)
        out.append(dict(m.last_color) if s["kind"] == COLOR else None)
    return out


GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "occupancy_color.npz"
FX = dict(np.load(GOLDEN)) if GOLDEN.exists() else {}
NAMES = [str(n) for n in FX.get("names", [])]


def case_of(name):
    """A fixture case as tools/make_occupancy_color_fixtures.py describes one"""
    st = FX[f"{name}_steps"].astype(np.int64)       # per step: kind, items, form, op
    ends = np.cumsum(st[:, 1])
    steps = []
    for i, (kind, n, form, op) in enumerate(st):
        a = slice(ends[i] - n, ends[i])
        steps.append(dict(kind=int(kind), form=int(form), op=int(op), keys=FX[f"{name}_keys"][a], points=FX[f"{name}_points"][a],
                          words=FX[f"{name}_words"][a], values=FX[f"{name}_values"][a], ops=FX[f"{name}_ops"][a], origin=FX[f"{name}_origins"][i]))
    return dict(params=rc.RayParams(*[float(v) for v in FX[f"{name}_params"]]), steps=steps)


def recorded(name):
    """What octomap answered, in the shape of run_case"""
    st = FX[f"{name}_steps"].astype(np.int64)
    nv = FX[f"{name}_nvoxels"].astype(np.int64)
    ends = np.cumsum(nv)
    nl = FX[f"{name}_nleaves"].astype(np.int64).reshape(-1, len(DEPTHS))
    lends = np.cumsum(nl.reshape(-1))
    ns = FX[f"{name}_nstream"].astype(np.int64)
    sends = np.cumsum(ns)
    out, snap = [], 0
    for i, (kind, _, _, _) in enumerate(st):
        a = slice(ends[i] - nv[i], ends[i])
        vox = (FX[f"{name}_voxel_keys"][a], FX[f"{name}_voxel_values"][a], FX[f"{name}_voxel_words"][a])
        if kind != SNAPSHOT:
            out.append(vox + (int(FX[f"{name}_found"][i]),))
            continue
        lists = []
        for j in range(len(DEPTHS)):
            e = lends[snap * len(DEPTHS) + j]
            b = slice(e - nl[snap, j], e)
            lists.append((FX[f"{name}_leaf_keys"][b], FX[f"{name}_leaf_depths"][b].astype(np.int32), FX[f"{name}_leaf_values"][b], FX[f"{name}_leaf_words"][b]))
        out.append((lists, FX[f"{name}_streams"][sends[snap] - ns[snap]:sends[snap]].tobytes(), vox))
        snap += 1
    return out


def same(mine, theirs):
    """A step of run_case against a step of recorded, exact in every integer, float bit and byte"""
    def arrays(a, b):
        return all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else np.asarray(x),
                                  np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else np.asarray(y)) for x, y in zip(a, b))
    if isinstance(mine[0], list):
        return all(arrays(a, b) for a, b in zip(mine[0], theirs[0])) and bytes(mine[1]) == bytes(theirs[1]) and arrays(mine[2], theirs[2])
    return arrays(mine[:3], theirs[:3]) and mine[3] == theirs[3]
