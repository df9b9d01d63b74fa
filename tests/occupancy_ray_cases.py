"""A literal Python transcription of the occupancy map's log-odds mode (include/sbm.h, "occupancy map: ray-cast free space"):
octomap's insertPointCloud(scan, origin, maxrange, lazy_eval=false, discretize=false) without a bounding box, stated per
depth-16 voxel, and the .bt writer for a map with free and occupied leaves. TEST INFRASTRUCTURE ONLY, no GPU, no library:
numpy float32 scalars are binary32, Python floats are binary64, math.sqrt and both divisions are correctly rounded.

    logodds(p) / constants(params)          float32 log-odds; (hit, miss, cmin, cmax, thres) of a RayParams
    coord_key(c, factor) / key3(p, factor)  coordToKeyChecked on one axis / a point (None where it fails)
    ray_keys(origin, end, resolution)       computeRayKeys -> (list of key triples or None, stop): SAME, KEY, LENGTH, OUT
    scan_sets(points, origin, max_range, resolution, census=None)   computeUpdate -> (free set, occupied set), packed keys
    Tree(params, resolution).insert(points, origin)                 one scan; .leaves() -> (keys uint64 ascending, float32)
    write_binary(keys, logodds, resolution, thres)                  -> (bytes of the .bt stream, node count)
    plane_points(disp, scale, model, pose)  the points sbm_occ_insert_rays feeds for one plane (front half of occupancy_ref)
"""
import math
import sys

import numpy as np

F = np.float32
DBL_MAX = sys.float_info.max
SAME, KEY, LENGTH, OUT = "same", "key", "length", "out"
MAX_STEPS = 3 * 65536      # each step moves one key by one on one axis


class RayParams:
    """sbm_occ_ray_params: octomap's defaults (AbstractOccupancyOcTree.cpp:42-47); max_range < 0 means no limit."""

    def __init__(self, prob_hit=0.7, prob_miss=0.4, clamp_min=0.1192, clamp_max=0.971, occupancy_thres=0.5, max_range=-1.0):
        self.prob_hit, self.prob_miss, self.clamp_min, self.clamp_max = prob_hit, prob_miss, clamp_min, clamp_max
        self.occupancy_thres, self.max_range = occupancy_thres, max_range


def logodds(p):
    return F(math.log(p / (1 - p)))


def constants(rp):
    return tuple(logodds(p) for p in (rp.prob_hit, rp.prob_miss, rp.clamp_min, rp.clamp_max, rp.occupancy_thres))


def pack3(k):
    return (k[0] << 32) | (k[1] << 16) | k[2]


def coord_key(c, factor):
    v = factor * float(c)
    if not math.isfinite(v):
        return None
    f = math.floor(v)
    if not (-32768 <= f < 32768):
        return None
    return int(f) + 32768


def key3(p, factor):
    k = tuple(coord_key(c, factor) for c in p)
    return None if None in k else k


def sub3(a, b):
    return [F(a[i]) - F(b[i]) for i in range(3)]


def norm(v):
    """Vector3::norm: the sum in float, left to right, its square root in double."""
    with np.errstate(over="ignore", invalid="ignore"):
        return math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def ray_keys(origin, end, resolution):
    """OcTreeBaseImpl::computeRayKeys. The origin cell is included, the end cell is not."""
    factor = 1.0 / resolution
    ko, ke = key3(origin, factor), key3(end, factor)
    if ko is None or ke is None:
        return None, OUT
    if ko == ke:
        return [], SAME
    ray = [ko]
    d = sub3(end, origin)
    length = F(norm(d))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = [d[i] / length for i in range(3)]
    step, tmax, tdelta = [0] * 3, [DBL_MAX] * 3, [DBL_MAX] * 3
    for i in range(3):
        step[i] = 1 if d[i] > 0 else -1 if d[i] < 0 else 0
        if step[i]:
            border = (float(ko[i] - 32768) + 0.5) * resolution
            border += float(F(step[i] * resolution * 0.5))
            tmax[i] = (border - float(origin[i])) / float(d[i])
            tdelta[i] = resolution / abs(float(d[i]))
    cur = list(ko)
    for _ in range(MAX_STEPS):
        if tmax[0] < tmax[1]:
            dim = 0 if tmax[0] < tmax[2] else 2
        else:
            dim = 1 if tmax[1] < tmax[2] else 2
        cur[dim] = (cur[dim] + step[dim]) & 0xFFFF
        tmax[dim] += tdelta[dim]
        if tuple(cur) == ke:
            return ray, KEY
        if min(min(tmax[0], tmax[1]), tmax[2]) > float(length):
            return ray, LENGTH
        ray.append(tuple(cur))
    raise AssertionError("a ray ran into the step bound")


def scan_sets(points, origin, max_range, resolution, census=None):
    """computeUpdate without a bounding box. census (a dict) counts the rays by how they stopped, and the ray steps."""
    factor = 1.0 / resolution
    origin = [F(c) for c in origin]
    free, occupied = set(), set()
    for p in np.asarray(points, np.float32).reshape(-1, 3):
        if not np.isfinite(p).all():
            continue
        v = sub3(p, origin)
        n = norm(v)
        if max_range < 0 or n <= max_range:
            end = p
            k = key3(p, factor)
            if k is not None:
                occupied.add(pack3(k))
        else:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                if n > 0:
                    v = [c / F(n) for c in v]
                end = [origin[i] + v[i] * F(max_range) for i in range(3)]
        ray, stop = ray_keys(origin, end, resolution)
        if census is not None:
            census[stop] = census.get(stop, 0) + 1
            census["steps"] = census.get("steps", 0) + (len(ray) if ray else 0)
        if ray:
            free.update(pack3(k) for k in ray)
    free -= occupied
    return free, occupied


class Tree:
    """The depth-16 leaves of an octomap::OcTree under insertPointCloud."""

    def __init__(self, rp=None, resolution=0.1):
        self.rp = rp or RayParams()
        self.resolution = resolution
        self.hit, self.miss, self.cmin, self.cmax, self.thres = constants(self.rp)
        self.v = {}

    def update(self, key, u):
        """updateNode(key, log_odds_update) and updateNodeLogOdds at the leaf."""
        v = self.v.get(key)
        if v is not None and ((u >= 0 and v >= self.cmax) or (u <= 0 and v <= self.cmin)):
            return
        v = (F(0) if v is None else v) + u
        self.v[key] = min(max(v, self.cmin), self.cmax)

    def insert(self, points, origin, census=None):
        free, occupied = scan_sets(points, origin, self.rp.max_range, self.resolution, census)
        for k in free:
            self.update(k, self.miss)
        for k in occupied:
            self.update(k, self.hit)
        return self

    def leaves(self):
        keys = np.array(sorted(self.v), np.uint64)
        return keys, np.array([self.v[int(k)] for k in keys], np.float32)


def morton(key):
    k0, k1, k2 = (key >> 32) & 0xFFFF, (key >> 16) & 0xFFFF, key & 0xFFFF
    m = 0
    for b in range(16):
        m |= ((k0 >> b & 1) | (k1 >> b & 1) << 1 | (k2 >> b & 1) << 2) << (3 * b)
    return m


def write_binary(keys, logodds_values, resolution, thres):
    """OcTree::writeBinary: toMaxLikelihood (occupied iff logodds >= thres), prune(), then writeBinaryNode depth first."""
    leaves = sorted((morton(int(k)), bool(F(v) >= F(thres))) for k, v in zip(keys, logodds_values))
    body = bytearray()

    def node(lo, hi, level):
        """The inner node over leaves[lo:hi] with `level` key bits undecided -> nodes written, this one included."""
        shift = 3 * (level - 1)
        full = 1 << shift
        edge = [lo]
        for c in range(8):
            e = edge[c]
            while e < hi and (leaves[e][0] >> shift) & 7 == c:
                e += 1
            edge.append(e)
        word, nodes, inner = 0, 1, []
        for c in range(8):
            a, b = edge[c], edge[c + 1]
            if a == b:
                continue
            kinds = {occ for _, occ in leaves[a:b]}
            if b - a == full and len(kinds) == 1:       # what prune() leaves as one leaf (or a depth-16 leaf itself)
                word |= (2 if leaves[a][1] else 1) << (2 * c)     # bits (2c, 2c+1): 0,1 occupied; 1,0 free
                nodes += 1
            else:
                word |= 3 << (2 * c)
                inner.append((a, b))
        body.extend((word & 0xFF, word >> 8))
        for a, b in inner:
            nodes += node(a, b, level - 1)
        return nodes

    nodes = node(0, len(leaves), 16) if leaves else 0
    head = ("# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
            "id OcTree\nsize %d\nres %g\ndata\n" % (nodes, resolution)).encode()
    return head + bytes(body), nodes


def plane_points(disp, scale, model, pose):
    """The points of one plane, row major: the pixels with d > 0 and a finite reprojection, after both transforms, where that
    point is finite (occupancy_ref.world gives NaN for a skipped pixel; both forms skip a point that is not finite)."""
    import occupancy_ref as occ
    world = occ.world(disp, scale, model, pose).reshape(-1, 3)
    return np.ascontiguousarray(world[np.isfinite(world).all(axis=1)])
