"""A literal Python transcription of the occupancy tree (include/sbm.h, "occupancy map: the octree above the voxels"): the
sixteen levels over a {packed key: value} dict of depth-16 voxels, as octomap has them after updateInnerOccupancy() and prune().
TEST INFRASTRUCTURE ONLY, no GPU, no library: numpy float32 scalars are binary32.

    max_likelihood(voxels, mode, constants)   the MAXLIKELIHOOD reading of a voxel dict -> {packed key: float32}
    Tree(voxels, resolution)                  the tree over {packed key: float32}
    Tree.nodes_at / leaves_at                 per depth, of the pruned tree; .size, .num_leaves, .key_min, .key_max
    Tree.search(point, depth, thres)          -> (SBM_OCC_CELL_*, float32 value or None, found depth or -1)
    Tree.leaves(max_depth)                    -> (centre keys uint64, depths int32, values float32) in octomap's iteration order
    Tree.all_nodes()                          the same for every node of the pruned tree, with a leaf flag: begin_tree()
    Tree.binary(cmax)                         -> the two bytes of every non-leaf node, depth first
    Tree.stream(cmax)                         -> the whole .bt file
    unpack_stage(fixture, name, tag, ...)     one reading's records of tests/golden/occupancy_tree.npz as named arrays
"""
import numpy as np

from occupancy_ray_cases import F, key3, morton, pack3

CELL_OUT, CELL_UNKNOWN, CELL_FREE, CELL_OCCUPIED = -1, 0, 1, 2
LOGODDS, MAXLIKELIHOOD = 0, 1
HITS, LOGODDS_MODE = "hits", "logodds"
DEPTH = 16
HEADER = ("# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
          "id OcTree\nsize %d\nres %g\ndata\n")


def max_likelihood(voxels, mode, constants):
    """toMaxLikelihood per voxel. constants: (hit, miss, clamp min, clamp max, threshold) as float32 log-odds."""
    cmin, cmax, thres = F(constants[2]), F(constants[3]), F(constants[4])
    if mode == HITS:
        return {k: cmax for k in voxels}
    return {k: (cmax if F(v) >= thres else cmin) for k, v in voxels.items()}


def unmorton(code):
    """The key prefixes (x, y, z) of a Morton code: bit 3b is x's bit b, 3b + 1 y's, 3b + 2 z's."""
    k = [0, 0, 0]
    for b in range(DEPTH):
        for a in range(3):
            k[a] |= (code >> (3 * b + a) & 1) << b
    return k


def centre_key(code, depth):
    """adjustKeyAtDepth of the node with this Morton prefix, packed."""
    level = DEPTH - depth
    k = unmorton(code)
    if level:
        k = [(p << level) | (1 << (level - 1)) for p in k]
    return pack3(k)


class Tree:
    def __init__(self, voxels, resolution=0.1):
        self.resolution, self.factor = resolution, 1.0 / resolution
        # level[d]: {Morton prefix of d child indices: value}, the float maximum over the voxels below
        self.level = [dict() for _ in range(DEPTH + 1)]
        self.level[DEPTH] = {morton(int(k)): F(v) for k, v in voxels.items()}
        # collapsed[d]: the prefixes whose 8 ^ (16 - d) voxels are all stored and equal (isNodeCollapsible, bottom up)
        self.collapsed = [set() for _ in range(DEPTH + 1)]
        for d in range(DEPTH - 1, -1, -1):
            kids = {}
            for code, v in self.level[d + 1].items():
                kids.setdefault(code >> 3, []).append((code, v))
            for code, ch in kids.items():
                self.level[d][code] = max(v for _, v in ch)
                if len(ch) == 8 and all(v == ch[0][1] for _, v in ch) and (d + 1 == DEPTH or all(c in self.collapsed[d + 1] for c, _ in ch)):
                    self.collapsed[d].add(code)
        # top[d][code]: the depth of the shallowest collapsed node at or above the node, or None
        self.top = [dict() for _ in range(DEPTH + 1)]
        for d in range(DEPTH + 1):
            for code in self.level[d]:
                above = self.top[d - 1][code >> 3] if d else None
                self.top[d][code] = above if above is not None else (d if code in self.collapsed[d] else None)
        self.nodes_at = [sum(1 for c in self.level[d] if self.in_pruned(c, d)) for d in range(DEPTH + 1)]
        self.leaves_at = [sum(1 for c in self.level[d] if self.in_pruned(c, d) and self.is_leaf(c, d)) for d in range(DEPTH + 1)]
        self.size, self.num_leaves = sum(self.nodes_at), sum(self.leaves_at)
        keys = [unmorton(c) for c in self.level[DEPTH]]
        self.key_min = [min(k[a] for k in keys) for a in range(3)] if keys else [65535] * 3
        self.key_max = [max(k[a] for k in keys) for a in range(3)] if keys else [0] * 3

    def in_pruned(self, code, d):
        """no collapsed proper ancestor"""
        return d == 0 or self.top[d - 1][code >> 3] is None

    def is_leaf(self, code, d):
        return d == DEPTH or code in self.collapsed[d]

    def search(self, point, depth=0, thres=0.0):
        depth = depth or DEPTH
        key = key3([F(c) for c in point], self.factor)
        if key is None:
            return CELL_OUT, None, -1
        code = morton(pack3(key)) >> (3 * (DEPTH - depth))
        v = self.level[depth].get(code)
        if v is None:
            return CELL_UNKNOWN, None, -1
        top = self.top[depth][code]
        return (CELL_OCCUPIED if v >= F(thres) else CELL_FREE), v, (depth if top is None else top)

    def search_all(self, points, depth=0, thres=0.0):
        """-> (state int32, value bits uint32, found depth int32)"""
        out = [self.search(p, depth, thres) for p in np.asarray(points, np.float32).reshape(-1, 3)]
        nan = np.uint32(0x7FC00000)
        return (np.array([s for s, _, _ in out], np.int32).reshape(-1),
                np.array([nan if v is None else np.float32(v).view(np.uint32) for _, v, _ in out], np.uint32).reshape(-1),
                np.array([f for _, _, f in out], np.int32).reshape(-1))

    def _walk(self, max_depth, inner):
        """Depth first, children 0..7 -> (code, depth, value, is leaf) of the leaves at depth <= max_depth and the nodes at
        max_depth; with `inner` also the nodes on the way."""
        out = []
        if not self.level[0]:
            return out
        stack = [(0, 0)]
        while stack:
            code, d = stack.pop()
            leaf = self.is_leaf(code, d)
            if leaf or d == max_depth or inner:
                out.append((code, d, self.level[d][code], leaf))
            if not leaf and d < max_depth:
                stack.extend((code << 3 | c, d + 1) for c in range(7, -1, -1) if (code << 3 | c) in self.level[d + 1])
        return out

    @staticmethod
    def _arrays(rows):
        return (np.array([centre_key(c, d) for c, d, _, _ in rows], np.uint64), np.array([d for _, d, _, _ in rows], np.int32),
                np.array([v for _, _, v, _ in rows], np.float32))

    def leaves(self, max_depth=0):
        return self._arrays(self._walk(max_depth or DEPTH, False))

    def all_nodes(self):
        rows = self._walk(DEPTH, True)
        return self._arrays(rows) + (np.array([leaf for _, _, _, leaf in rows], np.uint8),)

    def binary(self, cmax):
        """writeBinaryNode: per non-leaf node of the pruned tree two bits per child, 00 none, 01 occupied leaf, 10 free leaf,
        11 inner, child c in bits (2c, 2c + 1) with the first of the pair lower. A leaf is occupied iff it holds clamp max."""
        body = bytearray()
        for code, d, _, leaf in self._walk(DEPTH, True):
            if leaf:
                continue
            word = 0
            for c in range(8):
                child = code << 3 | c
                if child not in self.level[d + 1]:
                    continue
                if self.is_leaf(child, d + 1):
                    word |= (2 if self.level[d + 1][child] == F(cmax) else 1) << (2 * c)
                else:
                    word |= 3 << (2 * c)
            body.extend((word & 0xFF, word >> 8))
        return bytes(body)

    def stream(self, cmax):
        return (HEADER % (self.size, self.resolution)).encode() + self.binary(cmax)

    def expanded(self, max_depth=0):
        """leaves(max_depth) expanded to depth-16 voxels -> {packed key: value}: every entry covers its cube."""
        out = {}
        for code, d, v, _ in self._walk(max_depth or DEPTH, False):
            lo = code << (3 * (DEPTH - d))
            for m in range(lo, lo + (1 << (3 * (DEPTH - d)))):
                out[centre_key(m, DEPTH)] = v
        return out


def unpack_stage(fx, name, tag, max_depths, search_depths):
    """The records of tree `name` under reading `tag` ("lo" or "ml") in tests/golden/occupancy_tree.npz -> tree_key / tree_depth /
    tree_value / tree_leaf (begin_tree), leafs<maxDepth>_key / _depth / _value, num_nodes, num_leaves, and search<depth>_found /
    _value / _depth. The file keeps the six leaf lists end to end and the seven searches as rows."""
    p = f"{name}_{tag}_"
    out = {k: fx[p + k] for k in ("tree_key", "tree_value", "tree_leaf", "num_nodes", "num_leaves")}
    out["tree_depth"] = fx[p + "tree_depth"].astype(np.int32)
    ends = np.cumsum(fx[p + "leafs_n"])
    for md, n, e in zip(max_depths, fx[p + "leafs_n"], ends):
        out[f"leafs{md}_key"] = fx[p + "leafs_key"][e - n:e]
        out[f"leafs{md}_depth"] = fx[p + "leafs_depth"][e - n:e].astype(np.int32)
        out[f"leafs{md}_value"] = fx[p + "leafs_value"][e - n:e]
    for i, d in enumerate(search_depths):
        for k in ("found", "value", "depth"):
            out[f"search{d}_{k}"] = fx[p + f"search_{k}"][i]
    return out
