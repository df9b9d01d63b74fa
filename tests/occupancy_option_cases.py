"""A literal Python transcription of the occupancy map's insert options (include/sbm.h, "occupancy map: insert options"):
octomap's discretize flag (computeDiscreteUpdate), its bounding box (setBBXMin / setBBXMax / useBBXLimit inside computeUpdate)
and its change detection (updateNodeRecurs), stated per depth-16 voxel on top of tests/occupancy_ray_cases.py. TEST
INFRASTRUCTURE ONLY, no GPU, no library.

    wrapped_key(c, factor)                  the UNCHECKED coordToKey on one axis (None where the point is dropped)
    key_coord(k, resolution)                keyToCoord on one axis, as point3d's float
    discretize(points, resolution)          computeDiscreteUpdate's point list: one voxel centre per distinct wrapped key
    Box()                                   .set(min, max) -> False where a point has no key (the box is then unchanged);
                                            .has_point(p) in float, .has_key(k) by key, both inclusive
    scan_sets(points, origin, max_range, resolution, box=None, census=None)   computeUpdate -> (free set, occupied set)
    Tree(params, resolution)                rc.Tree with .box, .use_box, .detect and .changes {packed key: CREATED | FLIPPED};
                                            .insert(points, origin, discretize=False); .changed() -> (keys ascending, uint8
                                            created flags); .reset_changes(); .clear()
    FX, NAMES, case_of(name), recorded(name)   tests/golden/occupancy_options.npz: a case's scans with their switches, and
                                            what octomap answered after every scan
    run_case(case)                          a case through a Tree -> what recorded() holds
"""
import math
import pathlib

import numpy as np

import occupancy_ray_cases as rc

F = np.float32
CREATED, FLIPPED = 1, 2        # octomap's KeyBoolMap holds true for the first and false for the second


def wrapped_key(c, factor):
    v = factor * float(c)
    if not math.isfinite(float(c)) or not math.isfinite(v):
        return None
    f = math.floor(v)
    if not (-2 ** 31 <= f < 2 ** 31):
        return None
    return (int(f) + 32768) & 0xFFFF


def key_coord(k, resolution):
    return F((float(k - 32768) + 0.5) * resolution)


def discretize(points, resolution):
    factor = 1.0 / resolution
    seen, out = set(), []
    for p in np.asarray(points, np.float32).reshape(-1, 3):
        k = tuple(wrapped_key(c, factor) for c in p)
        if None in k or k in seen:
            continue
        seen.add(k)
        out.append([key_coord(c, resolution) for c in k])
    return np.asarray(out, np.float32).reshape(-1, 3)


class Box:
    """bbx_min / bbx_max and their keys. A fresh box is the origin's voxel corner: both points (0, 0, 0)."""

    def __init__(self, resolution=0.1):
        self.factor = 1.0 / resolution
        self.min = self.max = np.zeros(3, np.float32)
        self.min_key = self.max_key = (32768, 32768, 32768)

    def set(self, lo, hi):
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        klo, khi = rc.key3(lo, self.factor), rc.key3(hi, self.factor)
        if klo is None or khi is None:
            return False
        self.min, self.max, self.min_key, self.max_key = lo, hi, klo, khi
        return True

    def has_point(self, p):
        return all(F(p[i]) >= self.min[i] and F(p[i]) <= self.max[i] for i in range(3))

    def has_key(self, k):
        return all(self.min_key[i] <= k[i] <= self.max_key[i] for i in range(3))


def scan_sets(points, origin, max_range, resolution, box=None, census=None):
    """computeUpdate; box None is the branch without a bounding box, which is rc.scan_sets. census["steps"] counts the cells
    the rays marked."""
    if box is None:
        return rc.scan_sets(points, origin, max_range, resolution, census)
    factor = 1.0 / resolution
    origin = [F(c) for c in origin]
    free, occupied = set(), set()
    for p in np.asarray(points, np.float32).reshape(-1, 3):
        if not np.isfinite(p).all():
            continue
        v = rc.sub3(p, origin)
        n = rc.norm(v)
        within = max_range < 0 or n <= max_range
        if box.has_point(p) and within:
            k = rc.key3(p, factor)
            if k is not None:
                occupied.add(rc.pack3(k))
        end = p
        if max_range >= 0 and n > max_range:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                if n > 0:
                    v = [c / F(n) for c in v]
                end = [origin[i] + v[i] * F(max_range) for i in range(3)]
        ray, _ = rc.ray_keys(origin, end, resolution)
        for k in ray or []:
            if not box.has_key(k):
                break                       # the first cell outside ends the ray
            free.add(rc.pack3(k))
            if census is not None:
                census["steps"] = census.get("steps", 0) + 1
    free -= occupied
    return free, occupied


class Tree(rc.Tree):
    def __init__(self, rp=None, resolution=0.1):
        super().__init__(rp, resolution)
        self.box, self.use_box, self.detect, self.changes = Box(resolution), False, False, {}

    def update(self, key, u):
        """updateNode and, at the leaf, updateNodeRecurs' change detection"""
        v = self.v.get(key)
        if v is not None and ((u >= 0 and v >= self.cmax) or (u <= 0 and v <= self.cmin)):
            return
        super().update(key, u)
        if not self.detect:
            return
        if v is None:
            self.changes.setdefault(key, CREATED)
        elif (v >= self.thres) != (self.v[key] >= self.thres):
            if key not in self.changes:
                self.changes[key] = FLIPPED
            elif self.changes[key] == FLIPPED:
                del self.changes[key]

    def insert(self, points, origin, discretize_points=False, census=None):
        if discretize_points:
            points = discretize(points, self.resolution)
        free, occupied = scan_sets(points, origin, self.rp.max_range, self.resolution, self.box if self.use_box else None, census)
        for k in free:
            self.update(k, self.miss)
        for k in occupied:
            self.update(k, self.hit)
        return self

    def changed(self):
        keys = np.array(sorted(self.changes), np.uint64)
        return keys, np.array([self.changes[int(k)] == CREATED for k in keys], np.uint8)

    def reset_changes(self):
        self.changes = {}

    def clear(self):
        """sbm_occ_reset: the voxels and the change states go, the switches and the box stay"""
        self.v, self.changes = {}, {}


def run_case(case, resolution=0.1):
    """A case of tools/make_occupancy_option_fixtures.py -> after every scan (leaf keys, log-odds, changed keys, created flags)"""
    t = Tree(case["params"], resolution)
    out = []
    for s in case["scans"]:
        apply_switches(t, s)
        t.insert(s["points"], s["origin"], s["discretize"])
        out.append(t.leaves() + t.changed())
    return out


def apply_switches(t, s):
    """What a scan record asks for before its insert, on a Tree or on anything with the same methods"""
    if s["box"] is not None:
        assert t.box.set(*s["box"])
    t.use_box, t.detect = s["use_box"], s["detect"]
    if s["reset_changes"]:
        t.reset_changes()


GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "occupancy_options.npz"
FX = dict(np.load(GOLDEN)) if GOLDEN.exists() else {}
NAMES = [str(n) for n in FX.get("names", [])]


def case_of(name):
    """A fixture case as tools/make_occupancy_option_fixtures.py describes one"""
    n = FX[f"{name}_npoints"]
    ends = np.cumsum(n)
    sw, boxes = FX[f"{name}_switches"].astype(bool), FX[f"{name}_boxes"]
    scans = [dict(origin=FX[f"{name}_origins"][i], points=FX[f"{name}_points"][ends[i] - n[i]:ends[i]], use_box=bool(sw[i][0]),
                  detect=bool(sw[i][1]), discretize=bool(sw[i][2]), reset_changes=bool(sw[i][3]),
                  box=(boxes[i][:3], boxes[i][3:]) if sw[i][4] else None) for i in range(len(n))]
    return dict(params=rc.RayParams(*[float(v) for v in FX[f"{name}_params"]]), scans=scans)


def recorded(name):
    """-> per scan (leaf keys, log-odds, changed keys, created flags)"""
    nl, nc = FX[f"{name}_nleaves"].astype(np.int64), FX[f"{name}_nchanges"].astype(np.int64)
    a, b = np.cumsum(nl), np.cumsum(nc)
    return [(FX[f"{name}_keys"][a[i] - nl[i]:a[i]], FX[f"{name}_logodds"][a[i] - nl[i]:a[i]], FX[f"{name}_changed_keys"][b[i] - nc[i]:b[i]],
             FX[f"{name}_changed_created"][b[i] - nc[i]:b[i]]) for i in range(len(nl))]
