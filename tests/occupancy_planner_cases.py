"""A literal Python transcription of the occupancy map's read side for planners (include/sbm.h, "occupancy map: the read side
for planners"), over occupancy_tree_cases.Tree: octomap's begin_leafs_bbx, getUnknownLeafCenters, getMetricMin / getMetricMax and
getRayIntersection, statement by statement. TEST INFRASTRUCTURE ONLY, no GPU, no library: numpy float32 scalars are binary32 and
Python floats are binary64, and nothing here fuses a multiply with an add.

    leaves_bbx(tree, kmin, kmax, max_depth)          OcTreeIterator.hxx:335-460 -> (centre keys, depths, values), iteration order
    leaves_bbx_points(tree, pmin, pmax, max_depth)   the point constructor: coordToKeyChecked on both corners first
    overlaps(key, depth, kmin, kmax)                 singleIncrement's test of one node by itself
    key_to_coord(key, depth, resolution)             OcTreeBaseImpl.hxx:394-405, in double
    unknown_plan(resolution, pmin, pmax, depth)      the clamped corners, step size and step counts of getUnknownLeafCenters
    unknown_centers(tree, pmin, pmax, depth)         OcTreeBaseImpl.hxx:1046-1082 -> (n, 3) float32 in push order
    metric(tree, pruned=True)                        the const getMetricMin / getMetricMax -> (min[3], max[3]) in double
    metric_calc(tree)                                calcMinMax, the non-const path: its maximum is (centre - half) + size
    ray_intersection(resolution, o, d, c, delta)     OccupancyOcTreeBase.hxx:768-853 -> (found, float32[3]; NaN where not found)
"""
import math

import numpy as np

from occupancy_ray_cases import F, key3, morton, pack3
from occupancy_tree_cases import DEPTH, centre_key, unmorton

DBL_MAX = 1.7976931348623157e308
MAX_CELLS = 1 << 30
SIZE, UNSUPPORTED = -2, -23


def child_key(pos, off, parent):
    """computeChildKey (OcTreeKey.h:193-204)"""
    return tuple(parent[a] + off if pos >> a & 1 else parent[a] - off - (0 if off else 1) for a in range(3))


def overlaps(key, depth, kmin, kmax):
    """singleIncrement's test of a node at depth >= 1 with centre key `key`: loose by one key at the upper side of a cube"""
    off = 32768 >> depth
    return all(kmin[a] <= key[a] + off and kmax[a] >= key[a] - off for a in range(3))


def _arrays(rows):
    return (np.array([pack3(k) for k, _, _ in rows], np.uint64), np.array([d for _, d, _ in rows], np.int32),
            np.array([v for _, _, v in rows], np.float32))


def leaves_bbx(tree, kmin, kmax, max_depth=0):
    max_depth = max_depth or DEPTH
    out = []
    if not tree.level[0]:
        return _arrays(out)
    stack = [(0, 0, (32768, 32768, 32768))]      # the constructor pushes the root twice and operator++ pops one: never tested
    while stack:
        code, d, key = stack[-1]
        if d < max_depth and not tree.is_leaf(code, d):      # operator++'s loop: singleIncrement
            stack.pop()
            off = 32768 >> (d + 1)
            for i in range(7, -1, -1):
                child = code << 3 | i
                if child not in tree.level[d + 1]:
                    continue
                ck = child_key(i, off, key)
                if overlaps(ck, d + 1, kmin, kmax):
                    stack.append((child, d + 1, ck))
        else:                                                # the iterator stands here; the next ++ pops it
            out.append((key, d, tree.level[d][code]))
            stack.pop()
    return _arrays(out)


def corners_have_keys(tree, pmin, pmax):
    return key3([F(c) for c in pmin], tree.factor) is not None and key3([F(c) for c in pmax], tree.factor) is not None


def leaves_bbx_points(tree, pmin, pmax, max_depth=0, octomap=False):
    """A corner without a key: the library visits nothing, which is what octomap's constructor says it does ("set to end
    iterator"). octomap=True is what its loop does in fact -- THE DIVERGENCE: the constructor clears the tree pointer but leaves
    the root on the stack, operator!= compares the stack sizes, and the loop visits the root once."""
    if not corners_have_keys(tree, pmin, pmax):
        root = [((32768, 32768, 32768), 0, tree.level[0][0])] if octomap and tree.level[0] else []
        return _arrays(root)
    return leaves_bbx(tree, key3([F(c) for c in pmin], tree.factor), key3([F(c) for c in pmax], tree.factor), max_depth)


def leaves_bbx_by_node(tree, kmin, kmax, max_depth=0):
    """What one lane per node decides: the entries of leaves(max_depth) whose own test passes (the root passes untested)"""
    k, d, v = tree.leaves(max_depth)
    keep = [i for i in range(len(k)) if d[i] == 0 or
            overlaps(((int(k[i]) >> 32) & 0xFFFF, (int(k[i]) >> 16) & 0xFFFF, int(k[i]) & 0xFFFF), int(d[i]), kmin, kmax)]
    return k[keep], d[keep], v[keep]


def key_to_coord(key, depth, resolution):
    if depth == 0:
        return 0.0
    if depth == DEPTH:
        return (float(int(key) - 32768) + 0.5) * resolution
    return (math.floor((float(key) - 32768.0) / float(1 << (DEPTH - depth))) + 0.5) * (resolution * float(1 << (DEPTH - depth)))


def coord_to_key(coord, depth, factor):
    """The UNCHECKED coordToKey(coordinate, depth) before its cast to 16 bits -> int, or None where floor() fits no int"""
    v = factor * float(coord)
    if not math.isfinite(v) or not -2147483648.0 <= math.floor(v) < 2147483648.0:
        return None
    keyval = int(math.floor(v))
    diff = DEPTH - depth
    return keyval + 32768 if not diff else ((keyval >> diff) << diff) + (1 << (diff - 1)) + 32768


def unknown_plan(resolution, pmin, pmax, depth=0):
    """-> (status, lo float32[3], step float32, steps[3]). SIZE where a corner's key leaves 0..65535 (octomap wraps the cast),
    UNSUPPORTED for more than 2^30 cells. A negative or NaN step count (pmax below pmin on an axis), which octomap casts to
    unsigned with no defined result, is 0 steps."""
    depth = depth or DEPTH
    factor = 1.0 / resolution
    lo, hi = [], []
    for a in range(3):
        for p, out in ((pmin, lo), (pmax, hi)):
            k = coord_to_key(F(p[a]), depth, factor)
            if k is None or not 0 <= k <= 65535:
                return SIZE, None, None, None
            out.append(F(key_to_coord(k, depth, resolution)))
    step = F(resolution * math.pow(2, DEPTH - depth))
    steps = []
    for a in range(3):
        diff = F(hi[a] - lo[a])
        n = math.floor(float(F(diff / step)))
        steps.append(int(n) if n > 0 else 0)
    if steps[0] * steps[1] * steps[2] > MAX_CELLS:
        return UNSUPPORTED, None, None, None
    return 0, np.array(lo, np.float32), step, steps


def axis_table(start, step, n):
    """The running float sum of one axis: entry i is the coordinate after i + 1 increments"""
    out, p = np.empty(n, np.float32), F(start)
    for i in range(n):
        p = F(p + step)
        out[i] = p
    return out


def unknown_centers(tree, pmin, pmax, depth=0):
    """-> (status, (n, 3) float32, steps)"""
    st, lo, step, steps = unknown_plan(tree.resolution, pmin, pmax, depth)
    if st:
        return st, np.zeros((0, 3), np.float32), None
    depth = depth or DEPTH
    tx, ty, tz = (axis_table(lo[a], step, steps[a]) for a in range(3))
    out = []
    for x in tx:
        for y in ty:
            for z in tz:
                key = key3([x, y, z], tree.factor)
                if key is None or (morton(pack3(key)) >> (3 * (DEPTH - depth))) not in tree.level[depth]:
                    out.append((x, y, z))
    return 0, np.array(out, np.float32).reshape(-1, 3), steps


def _leaf_boxes(tree, pruned):
    if pruned:
        k, d, _ = tree.leaves(0)
        return [(((int(q) >> 32) & 0xFFFF, (int(q) >> 16) & 0xFFFF, int(q) & 0xFFFF), int(dd)) for q, dd in zip(k, d)]
    return [(tuple(unmorton(c)), DEPTH) for c in sorted(tree.level[DEPTH])]


def metric(tree, pruned=True):
    """The const getMetricMin / getMetricMax: centre -+ getNodeSize(depth) / 2.0 over the leaves; six zeros for an empty tree.
    pruned=False: over the voxels, the expanded tree."""
    if not tree.level[0]:
        return [0.0] * 3, [0.0] * 3
    lo, hi = [DBL_MAX] * 3, [-DBL_MAX] * 3
    for key, d in _leaf_boxes(tree, pruned):
        half = (tree.resolution * float(1 << (DEPTH - d))) / 2.0
        for a in range(3):
            c = key_to_coord(key[a], d, tree.resolution)
            if c - half < lo[a]:
                lo[a] = c - half
            if c + half > hi[a]:
                hi[a] = c + half
    return lo, hi


def metric_calc(tree, pruned=True):
    """calcMinMax (the non-const getMetricMin / getMetricMax, which volume() goes through): the maximum is (centre - half) + size"""
    if not tree.level[0]:
        return [0.0] * 3, [0.0] * 3
    lo, hi = [DBL_MAX] * 3, [-DBL_MAX] * 3
    for key, d in _leaf_boxes(tree, pruned):
        size = tree.resolution * float(1 << (DEPTH - d))
        half = size / 2.0
        for a in range(3):
            x = key_to_coord(key[a], d, tree.resolution) - half
            if x < lo[a]:
                lo[a] = x
            x += size
            if x > hi[a]:
                hi[a] = x
    return lo, hi


def metric_size(lo, hi):
    return [hi[a] - lo[a] for a in range(3)]


def volume(lo, hi):
    x, y, z = metric_size(lo, hi)
    return x * y * z


def _dot(a, b):
    """Vector3::dot: products and sums in float, returned as double"""
    return float(F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])))


def ray_intersection(resolution, origin, direction, centre, delta=0.0):
    with np.errstate(all="ignore"):
        o, d, c = ([F(v) for v in p] for p in (origin, direction, centre))
        half = F(resolution / 2.0)
        normal = [[F(1), F(0), F(0)], [F(0), F(1), F(0)], [F(0), F(0), F(1)]]
        neg = [[F(c[b] - half) if b == a else c[b] for b in range(3)] for a in range(3)]      # pointXNeg, pointYNeg, pointZNeg
        pos = [[F(c[b] + half) if b == a else c[b] for b in range(3)] for a in range(3)]
        out_d, found = DBL_MAX, False
        for a in range(3):
            line_dot_normal = _dot(normal[a], d)
            if line_dot_normal != 0.0:                       # a NaN passes, as in the source
                u, v = [b for b in range(3) if b != a]
                for point in (neg[a], pos[a]):
                    dist = float(np.float64(_dot([F(point[b] - o[b]) for b in range(3)], normal[a])) / np.float64(line_dot_normal))
                    fd = F(dist)
                    hit = [F(F(d[b] * fd) + o[b]) for b in range(3)]
                    if not (float(hit[u]) < float(neg[u][u]) - 1e-6 or float(hit[u]) > float(pos[u][u]) + 1e-6 or
                            float(hit[v]) < float(neg[v][v]) - 1e-6 or float(hit[v]) > float(pos[v][v]) + 1e-6):
                        out_d = min_std(out_d, dist)
                        found = True
        if not found:
            return False, np.full(3, np.nan, np.float32)
        t = F(out_d + delta)
        return True, np.array([F(F(d[b] * t) + o[b]) for b in range(3)], np.float32)


def min_std(a, b):
    """std::min(a, b): b where b < a, else a -- a NaN second argument leaves a"""
    return b if b < a else a
