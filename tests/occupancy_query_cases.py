"""A literal Python transcription of the occupancy map's queries (include/sbm.h, "occupancy map: queries"): octomap's
search(point) and castRay(origin, direction, end, ignoreUnknownCells, maxRange), stated per depth-16 voxel over a
{packed key: value} dict. TEST INFRASTRUCTURE ONLY, no GPU, no library: numpy float32 scalars are binary32, Python floats are
binary64, math.sqrt and both divisions are correctly rounded.

    Map(voxels, mode, thres, resolution)    the voxel state behind both calls: mode LOGODDS (values float32), HITS (values
                                            counts) or NONE
    Map.search(point)                       -> (SBM_OCC_CELL_*, value or None)
    Map.cast_ray(origin, direction, ignore_unknown=False, max_range=-1.0, census=None)   -> (SBM_OCC_RAY_*, end float32 (3,))
    view_rays(width, height, scale, model, pose, pixels=None)   the rays sbm_occ_cast_view_device casts -> (origins, directions)
"""
import math

import numpy as np

from occupancy_ray_cases import DBL_MAX, MAX_STEPS, F, key3, norm, pack3

CELL_OUT, CELL_UNKNOWN, CELL_FREE, CELL_OCCUPIED = -1, 0, 1, 2
RAY_NONE, RAY_HIT, RAY_RANGE, RAY_UNKNOWN, RAY_BOUNDS = 0, 1, 2, 3, 4
NONE, HITS, LOGODDS = "none", "hits", "logodds"
NAN3 = np.full(3, np.nan, np.float32)


def centre(key, resolution):
    """keyToCoord of a key triple, as point3d's floats."""
    return np.array([F((float(k - 32768) + 0.5) * resolution) for k in key], np.float32)


def transform_point(p, t):
    """Stereo.cpp:189-198: per row r1 * x + r2 * y + r3 * z + o in float, left to right."""
    t = [F(v) for v in t]
    with np.errstate(over="ignore", invalid="ignore"):
        return [t[4 * r] * p[0] + t[4 * r + 1] * p[1] + t[4 * r + 2] * p[2] + t[4 * r + 3] for r in range(3)]


def view_rays(width, height, scale, model, pose, pixels=None):
    """All pixels row major, or only the (row, col) of `pixels`."""
    if pixels is None:
        pixels = [(row, col) for row in range(height) for col in range(width)]
    origins, dirs = np.empty((len(pixels), 3), np.float32), np.empty((len(pixels), 3), np.float32)

    def T(p):
        if model.has_local:
            p = transform_point(p, list(model.local))
        return transform_point(p, pose)

    o = T([F(0), F(0), F(0)])
    for i, (row, col) in enumerate(pixels):
        q = T([F((float(int(col) * scale) - model.cx_l) / model.fx_l), F((float(int(row) * scale) - model.cy_l) / model.fy_l), F(1)])
        origins[i] = o
        with np.errstate(over="ignore", invalid="ignore"):
            dirs[i] = [q[j] - o[j] for j in range(3)]
    return origins, dirs


class Map:
    def __init__(self, voxels, mode, thres=0.0, resolution=0.1):
        self.v, self.mode, self.thres, self.resolution = voxels, mode, F(thres), resolution
        self.factor = 1.0 / resolution

    def cell(self, key):
        """-> (state, value) of a key triple"""
        v = self.v.get(pack3(key)) if self.mode != NONE else None
        if v is None:
            return CELL_UNKNOWN, None
        if self.mode == HITS:
            return CELL_OCCUPIED, v
        return (CELL_OCCUPIED if F(v) >= self.thres else CELL_FREE), v

    def search(self, point):
        key = key3([F(c) for c in point], self.factor)
        if key is None:
            return CELL_OUT, None
        return self.cell(key)

    def cast_ray(self, origin, direction, ignore_unknown=False, max_range=-1.0, census=None):
        res = self.resolution
        origin = [F(c) for c in origin]
        d = [F(c) for c in direction]
        key = key3(origin, self.factor)                                   # 1 origin
        if key is None:
            return RAY_NONE, NAN3
        state, _ = self.cell(key)                                         # 2 start
        if state == CELL_OCCUPIED:
            return RAY_HIT, centre(key, res)
        if state == CELL_UNKNOWN and not ignore_unknown:
            return RAY_UNKNOWN, centre(key, res)
        length = norm(d)                                                  # 3 normal
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if length > 0:
                d = [c / F(length) for c in d]
        step, tmax, tdelta = [0] * 3, [DBL_MAX] * 3, [DBL_MAX] * 3        # 4 steps
        for i in range(3):
            step[i] = 1 if d[i] > 0 else -1 if d[i] < 0 else 0
            if step[i]:
                border = (float(key[i] - 32768) + 0.5) * res
                border += float(step[i]) * res * 0.5
                tmax[i] = (border - float(origin[i])) / float(d[i])
                with np.errstate(divide="ignore"):
                    tdelta[i] = float(np.float64(res) / abs(np.float64(d[i])))
        if step == [0, 0, 0]:
            return RAY_NONE, NAN3
        ranged = max_range > 0.0
        range_sq = max_range * max_range
        cur = list(key)
        for _ in range(MAX_STEPS):                                        # 5 loop
            if tmax[0] < tmax[1]:
                dim = 0 if tmax[0] < tmax[2] else 2
            else:
                dim = 1 if tmax[1] < tmax[2] else 2
            if (step[dim] < 0 and cur[dim] == 0) or (step[dim] > 0 and cur[dim] == 65535):
                return RAY_BOUNDS, centre(cur, res)
            cur[dim] += step[dim]
            tmax[dim] += tdelta[dim]
            if census is not None:
                census["steps"] = census.get("steps", 0) + 1
            end = centre(cur, res)
            if ranged:
                dist = 0.0
                for j in range(3):
                    with np.errstate(over="ignore"):
                        dist += float((end[j] - origin[j]) * (end[j] - origin[j]))
                if dist > range_sq:
                    return RAY_RANGE, end
            state, _ = self.cell(cur)
            if state == CELL_OCCUPIED:
                return RAY_HIT, end
            if state == CELL_UNKNOWN and not ignore_unknown:
                return RAY_UNKNOWN, end
        raise AssertionError("a ray ran into the step bound")

    def cast_rays(self, origins, dirs, ignore_unknown=False, max_range=-1.0, census=None):
        """-> (status int32 (n,), end float32 (n, 3)); origins (3,) or (n, 3)"""
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        origins = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), dirs.shape)
        out = [self.cast_ray(o, d, ignore_unknown, max_range, census) for o, d in zip(origins, dirs)]
        return np.array([s for s, _ in out], np.int32), np.array([e for _, e in out], np.float32).reshape(-1, 3)

    def search_all(self, points):
        """-> (state int32 (n,), value uint32 (n,)): the bits sbm_occ_search writes"""
        out = [self.search(p) for p in np.asarray(points, np.float32).reshape(-1, 3)]
        absent = np.float32(np.nan).view(np.uint32) if self.mode == LOGODDS else np.uint32(0)
        bits = [absent if v is None else (np.float32(v).view(np.uint32) if self.mode == LOGODDS else np.uint32(v)) for _, v in out]
        return np.array([s for s, _ in out], np.int32), np.array(bits, np.uint32)
