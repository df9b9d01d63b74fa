"""The occupancy voxel map of the reference's buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561): a device-side set of
octomap keys fed straight from disparity planes, and the octomap binary stream (.bt) written from its distinct keys. Its second
mode is octomap's insertPointCloud: float log-odds per voxel, free space ray-cast from each scan's origin, with octomap's three
insert switches: discretize, the bounding box and change detection."""
import ctypes
import os

import numpy as np

from ._abi import (ERR_OCC_FULL, OCC_COLOR_AVERAGE, OCC_COLOR_SET, OCC_COLOR_WHITE, OccColorInfo, OCC_EDIT_CHUNK, OCC_EDIT_DELETE, OCC_EDIT_SET, OCC_EDIT_UPDATE, OccEditInfo, OCC_CELL_FREE, OCC_CELL_OCCUPIED, OCC_CELL_OUT, OCC_CELL_UNKNOWN, OCC_RAY_BOUNDS,  # noqa: F401
                   OCC_RAY_HIT, OCC_RAY_NONE, OCC_RAY_RANGE, OCC_RAY_UNKNOWN, OCC_TREE_LOGODDS, OCC_TREE_MAXLIKELIHOOD, OccParams,
                   OccBinaryHeader, OccGrowthInfo, OccOtHeader, OccQueryParams, OccRayParams, OccTreeCounts, StereoBMError, _check, _torch, load_library)


def occ_params(resolution=0.1, range_max=5.0, tree_depth=16):
    """The reference's constants by default. range_max is squared and compared with the NORM, as the reference does."""
    return OccParams(float(resolution), float(range_max), int(tree_depth))


def occ_validate(params):
    """Status code of sbm_occ_params_validate (0 = ok)."""
    return load_library().sbm_occ_params_validate(ctypes.byref(params))


def occ_write_binary(keys, path, resolution=0.1):
    """Write the .bt stream OcTree::writeBinary produces for a tree holding exactly these packed keys (uint64, any order) as
    occupied leaves. Host code: needs no GPU."""
    keys = np.ascontiguousarray(np.asarray(keys, np.uint64).reshape(-1))
    _check(load_library().sbm_occ_write_binary(keys.ctypes.data if len(keys) else None, len(keys), float(resolution),
                                               os.fsencode(path)))


def occ_ray_params(prob_hit=0.7, prob_miss=0.4, clamp_min=0.1192, clamp_max=0.971, occupancy_thres=0.5, max_range=-1.0):
    """octomap's constants by default; max_range < 0 means no limit."""
    return OccRayParams(float(prob_hit), float(prob_miss), float(clamp_min), float(clamp_max), float(occupancy_thres),
                        float(max_range))


def occ_ray_validate(params):
    """Status code of sbm_occ_ray_params_validate (0 = ok)."""
    return load_library().sbm_occ_ray_params_validate(ctypes.byref(params))


def occ_ray_logodds(params=None):
    """float32 (5,): the log-odds of hit, miss, clamp min, clamp max and the occupancy threshold."""
    out = np.empty(5, np.float32)
    _check(load_library().sbm_occ_ray_logodds(ctypes.byref(params if params is not None else occ_ray_params()), out.ctypes.data))
    return out


def occ_write_binary_logodds(keys, logodds, path, resolution=0.1, occupancy_thres_log=0.0):
    """Write the .bt stream OcTree::writeBinary produces for a tree whose leaves are these packed keys (uint64, each once) with
    these float log-odds: occupied iff logodds >= occupancy_thres_log, pruned. Host code: needs no GPU."""
    keys = np.ascontiguousarray(np.asarray(keys, np.uint64).reshape(-1))
    logodds = np.ascontiguousarray(np.asarray(logodds, np.float32).reshape(-1))
    if len(keys) != len(logodds):
        raise StereoBMError(-2, f"{len(keys)} keys with {len(logodds)} log-odds")
    _check(load_library().sbm_occ_write_binary_logodds(keys.ctypes.data if len(keys) else None,
                                                       logodds.ctypes.data if len(keys) else None, len(keys), float(resolution),
                                                       float(occupancy_thres_log), os.fsencode(path)))


def _stream(data):
    """A .bt stream as a contiguous uint8 array (bytes, bytearray, memoryview or a numpy array of bytes)"""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), np.uint8)


def occ_binary_info(data):
    """What a .bt stream holds, parsed on the host (no GPU): dict of resolution, size (the header's), nodes (read), leaves,
    occupied, voxels (depth-16 voxels below the leaves), leaves_at per depth 0..16, key_min / key_max per axis."""
    b = _stream(data)
    h = OccBinaryHeader()
    _check(load_library().sbm_occ_binary_info(b.ctypes.data if len(b) else None, len(b), ctypes.byref(h)))
    return dict(resolution=h.resolution, size=h.size, nodes=h.nodes, leaves=h.leaves, occupied=h.occupied, voxels=h.voxels,
                leaves_at=list(h.leaves_at), key_min=list(h.key_min), key_max=list(h.key_max))


def occ_binary_leaves(data):
    """The leaves of a .bt stream in stream order, parsed on the host (no GPU) -> (packed key of each cube's lowest voxel uint64,
    depth int32, occupied uint8)."""
    b = _stream(data)
    L = load_library()
    n = ctypes.c_size_t()
    ptr = b.ctypes.data if len(b) else None
    st = L.sbm_occ_binary_leaves(ptr, len(b), None, None, None, 0, ctypes.byref(n))
    if st != -2 or not n.value:      # -2 with a count: the arrays are too small, as asked
        _check(st)
    keys, depth, occ = np.empty(n.value, np.uint64), np.empty(n.value, np.int32), np.empty(n.value, np.uint8)
    if n.value:
        _check(L.sbm_occ_binary_leaves(ptr, len(b), keys.ctypes.data, depth.ctypes.data, occ.ctypes.data, n.value, ctypes.byref(n)))
    return keys, depth, occ


def occ_ot_info(data):
    """What an .ot stream holds, parsed on the host (no GPU): dict of resolution, size (the header's), nodes (records read), leaves,
    voxels (depth-16 voxels below the leaves), leaves_at per depth 0..16, value_min / value_max over the finite leaf values,
    key_min / key_max per axis."""
    b = _stream(data)
    h = OccOtHeader()
    _check(load_library().sbm_occ_ot_info(b.ctypes.data if len(b) else None, len(b), ctypes.byref(h)))
    return dict(resolution=h.resolution, size=h.size, nodes=h.nodes, leaves=h.leaves, voxels=h.voxels, leaves_at=list(h.leaves_at),
                value_min=h.value_min, value_max=h.value_max, key_min=list(h.key_min), key_max=list(h.key_max))


def occ_ot_leaves(data):
    """The leaves of an .ot stream in stream order, parsed on the host (no GPU) -> (packed key of each cube's lowest voxel uint64,
    depth int32, value float32)."""
    b = _stream(data)
    L = load_library()
    n = ctypes.c_size_t()
    ptr = b.ctypes.data if len(b) else None
    st = L.sbm_occ_ot_leaves(ptr, len(b), None, None, None, 0, ctypes.byref(n))
    if st != -2 or not n.value:      # -2 with a count: the arrays are too small, as asked
        _check(st)
    keys, depth, value = np.empty(n.value, np.uint64), np.empty(n.value, np.int32), np.empty(n.value, np.float32)
    if n.value:
        _check(L.sbm_occ_ot_leaves(ptr, len(b), keys.ctypes.data, depth.ctypes.data, value.ctypes.data, n.value, ctypes.byref(n)))
    return keys, depth, value


def occ_stamped_ot_info(data):
    """occ_ot_info for an `id OcTreeStamped` stream (the plain five-byte records), parsed on the host (no GPU)."""
    b = _stream(data)
    h = OccOtHeader()
    _check(load_library().sbm_occ_stamp_ot_info(b.ctypes.data if len(b) else None, len(b), ctypes.byref(h)))
    return dict(resolution=h.resolution, size=h.size, nodes=h.nodes, leaves=h.leaves, voxels=h.voxels, leaves_at=list(h.leaves_at),
                value_min=h.value_min, value_max=h.value_max, key_min=list(h.key_min), key_max=list(h.key_max))


def occ_stamped_ot_leaves(data):
    """The leaves of an `id OcTreeStamped` stream in stream order, parsed on the host (no GPU) -> (packed key of each cube's lowest
    voxel uint64, depth int32, value float32). The stream carries no stamps."""
    b = _stream(data)
    n = occ_stamped_ot_info(b)["leaves"]
    keys, depth, value = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.float32)
    got = ctypes.c_size_t()
    _check(load_library().sbm_occ_stamp_ot_leaves(b.ctypes.data if len(b) else None, len(b), keys.ctypes.data if n else None,
                                                  depth.ctypes.data if n else None, value.ctypes.data if n else None, n, ctypes.byref(got)))
    return keys[:got.value], depth[:got.value], value[:got.value]


def occ_color_ot_info(data):
    """occ_ot_info for a ColorOcTree stream (eight bytes per node), parsed on the host (no GPU)."""
    b = _stream(data)
    h = OccOtHeader()
    _check(load_library().sbm_occ_color_ot_info(b.ctypes.data if len(b) else None, len(b), ctypes.byref(h)))
    return dict(resolution=h.resolution, size=h.size, nodes=h.nodes, leaves=h.leaves, voxels=h.voxels, leaves_at=list(h.leaves_at),
                value_min=h.value_min, value_max=h.value_max, key_min=list(h.key_min), key_max=list(h.key_max))


def occ_color_ot_leaves(data):
    """The leaves of a ColorOcTree stream in stream order, parsed on the host (no GPU) -> (packed key of each cube's lowest voxel
    uint64, depth int32, value float32, colour word uint32)."""
    b = _stream(data)
    L = load_library()
    n = ctypes.c_size_t()
    ptr = b.ctypes.data if len(b) else None
    st = L.sbm_occ_color_ot_leaves(ptr, len(b), None, None, None, None, 0, ctypes.byref(n))
    if st != -2 or not n.value:      # -2 with a count: the arrays are too small, as asked
        _check(st)
    keys, depth, value, color = np.empty(n.value, np.uint64), np.empty(n.value, np.int32), np.empty(n.value, np.float32), np.empty(n.value, np.uint32)
    if n.value:
        _check(L.sbm_occ_color_ot_leaves(ptr, len(b), keys.ctypes.data, depth.ctypes.data, value.ctypes.data, color.ctypes.data, n.value, ctypes.byref(n)))
    return keys, depth, value, color


def occ_color_words(colors):
    """(n, 3) uint8 r, g, b, or (n,) words -> (n,) uint32 words r | g << 8 | b << 16"""
    c = np.asarray(colors)
    if c.ndim == 2:
        c = c.astype(np.uint32) & np.uint32(255)
        c = c[:, 0] | c[:, 1] << np.uint32(8) | c[:, 2] << np.uint32(16)
    return np.ascontiguousarray(c, np.uint32).reshape(-1)


def occ_color_rgb(words):
    """(n,) colour words -> (n, 3) uint8 r, g, b"""
    w = np.asarray(words).astype(np.uint32)
    return np.stack([w & 255, w >> 8 & 255, w >> 16 & 255], axis=1).astype(np.uint8)


def occ_query_params(max_range=-1.0, occupancy_thres_log=0.0, ignore_unknown=False):
    """castRay's defaults; max_range <= 0 means no limit. occupancy_thres_log is occ_ray_logodds(params)[4]."""
    return OccQueryParams(float(max_range), float(occupancy_thres_log), int(bool(ignore_unknown)))


def occ_query_validate(params):
    """Status code of sbm_occ_query_params_validate (0 = ok)."""
    return load_library().sbm_occ_query_params_validate(ctypes.byref(params))


def occ_growth_step(capacity, need=0, max_capacity=0):
    """The growth policy (sbm_occ_growth_step, host code): the capacity a step goes to from `capacity` when `need` voxels are
    known, under the ceiling max_capacity (0: 2^30). Raises StereoBMError(ERR_OCC_FULL) at the ceiling."""
    nxt = ctypes.c_size_t()
    _check(load_library().sbm_occ_growth_step(int(capacity), int(need), int(max_capacity), ctypes.byref(nxt)))
    return nxt.value


def _poses(poses, n):
    p = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    if p.shape[0] != n:
        raise StereoBMError(-2, f"{p.shape[0]} poses for {n} planes")
    return p


class OccupancyMap:
    """A map for up to `capacity` voxels on the device of `engine` (a StereoBM or StereoSGBM), which must outlive it: the map
    uses the engine's handle, stream and scratch. Not thread-safe. grow=True lets the table rehash itself into a larger one
    instead of filling up, up to max_capacity voxels (0: the create limit of 2^30)."""

    def __init__(self, engine, capacity, params=None, **kw):
        grow, max_capacity = kw.pop("grow", False), kw.pop("max_capacity", 0)
        if params is not None and kw:
            raise TypeError("pass either an OccParams or keyword parameters")
        self._p = params if params is not None else occ_params(**kw)
        self._engine = engine
        self._L = engine._L
        self._m = ctypes.c_void_p()
        _check(self._L.sbm_occ_create(engine._h, ctypes.byref(self._p), int(capacity), ctypes.byref(self._m)), engine._h)
        if grow or max_capacity:
            self.set_growth(grow, max_capacity)

    def close(self):
        m = getattr(self, "_m", None)
        if m:
            self._L.sbm_occ_destroy(m)
            self._m = None

    def __del__(self):
        self.close()

    @property
    def resolution(self):
        return self._p.resolution

    def reset(self):
        """Empty the map; the table is kept."""
        _check(self._L.sbm_occ_reset(self._m), self._engine._h)

    def insert(self, disparity, model, poses, scale=1, sync=True):
        """Planes (n,H,W) or (H,W): a torch CUDA int16 tensor, or a numpy int16 array (the host form, always synchronous);
        poses: n x 12 floats (r11 r12 r13 o14 / ...). Raises StereoBMError(ERR_OCC_FULL) when points found the table full."""
        if isinstance(disparity, np.ndarray):
            d = np.ascontiguousarray(disparity, np.int16)
            d = d[None] if d.ndim == 2 else d
            n, h, w = d.shape
            p = _poses(poses, n)
            _check(self._L.sbm_occ_insert(self._m, n, d.ctypes.data, w, h, int(scale), ctypes.byref(model), p.ctypes.data),
                   self._engine._h)
            return
        torch = _torch()
        if not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.int16 or not disparity.is_cuda or \
                disparity.dim() not in (2, 3) or disparity.device.index != self._engine._device:
            raise StereoBMError(-2, "disparity must be a CUDA int16 (n,H,W) or (H,W) tensor on the engine's device")
        d3, n, h, w = self._engine._as3d(disparity)
        p = _poses(poses, n)   # read before the call returns
        torch.cuda.current_stream(d3.device).synchronize()
        _check(self._L.sbm_occ_insert_device(self._m, n, d3.data_ptr(), w, h, int(scale), ctypes.byref(model), p.ctypes.data,
                                             1 if sync else 0), self._engine._h)
        if sync:
            self._engine._inflight.clear()
        else:
            self._engine._inflight.append((d3,))

    def _ray_params(self, params, kw):
        if params is not None and kw:
            raise TypeError("pass either an OccRayParams or keyword parameters")
        self._rp = params if params is not None else occ_ray_params(**kw)
        return ctypes.byref(self._rp)

    def insert_cloud(self, points, origin, params=None, sync=True, **kw):
        """octomap's insertPointCloud(scan, origin, maxrange): points (m, 3) as a torch CUDA float32 tensor or a numpy array
        (the host form, always synchronous), origin three floats. The parameters of the last log-odds insert are the ones
        write_binary_logodds thresholds with. discretize=True casts one ray per end voxel instead of one per point."""
        discrete = "_discrete" if kw.pop("discretize", False) else ""
        rp = self._ray_params(params, kw)
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3))
        if isinstance(points, np.ndarray):
            p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            _check(getattr(self._L, f"sbm_occ_insert_cloud{discrete}")(self._m, len(p), p.ctypes.data if len(p) else None, o.ctypes.data,
                                                                       rp), self._engine._h)
            return
        torch = _torch()
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or not points.is_cuda or points.dim() != 2 or \
                points.shape[1] != 3 or points.device.index != self._engine._device:
            raise StereoBMError(-2, "points must be a CUDA float32 (m, 3) tensor on the engine's device")
        p = points.contiguous()
        torch.cuda.current_stream(p.device).synchronize()
        _check(getattr(self._L, f"sbm_occ_insert_cloud{discrete}_device")(self._m, p.shape[0], p.data_ptr() if p.shape[0] else None,
                                                                          o.ctypes.data, rp, 1 if sync else 0), self._engine._h)
        if sync:
            self._engine._inflight.clear()
        else:
            self._engine._inflight.append((p,))

    def insert_rays(self, disparity, model, poses, scale=1, params=None, sync=True, **kw):
        """The arguments of insert(); plane i is one scan from the origin (o14, o24, o34) of pose i. discretize=True as for
        insert_cloud."""
        discrete = "_discrete" if kw.pop("discretize", False) else ""
        rp = self._ray_params(params, kw)
        if isinstance(disparity, np.ndarray):
            d = np.ascontiguousarray(disparity, np.int16)
            d = d[None] if d.ndim == 2 else d
            n, h, w = d.shape
            p = _poses(poses, n)
            _check(getattr(self._L, f"sbm_occ_insert_rays{discrete}")(self._m, n, d.ctypes.data, w, h, int(scale), ctypes.byref(model),
                                                                      p.ctypes.data, rp), self._engine._h)
            return
        torch = _torch()
        if not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.int16 or not disparity.is_cuda or \
                disparity.dim() not in (2, 3) or disparity.device.index != self._engine._device:
            raise StereoBMError(-2, "disparity must be a CUDA int16 (n,H,W) or (H,W) tensor on the engine's device")
        d3, n, h, w = self._engine._as3d(disparity)
        p = _poses(poses, n)   # read before the call returns
        torch.cuda.current_stream(d3.device).synchronize()
        _check(getattr(self._L, f"sbm_occ_insert_rays{discrete}_device")(self._m, n, d3.data_ptr(), w, h, int(scale), ctypes.byref(model),
                                                                         p.ctypes.data, rp, 1 if sync else 0), self._engine._h)
        if sync:
            self._engine._inflight.clear()
        else:
            self._engine._inflight.append((d3,))

    # ---- insert options: octomap's bounding box and change detection, for the log-odds inserts that follow --------------------
    def set_bbx(self, lo, hi):
        """setBBXMin(lo), setBBXMax(hi): two points of three floats. A point without a key raises (code -2) and the box stays."""
        lo = np.ascontiguousarray(np.asarray(lo, np.float32).reshape(3))
        hi = np.ascontiguousarray(np.asarray(hi, np.float32).reshape(3))
        _check(self._L.sbm_occ_set_bbx(self._m, lo.ctypes.data, hi.ctypes.data), self._engine._h)

    def use_bbx_limit(self, enable=True):
        _check(self._L.sbm_occ_use_bbx_limit(self._m, int(bool(enable))), self._engine._h)

    def bbx(self):
        """dict: min, max (float32 (3,)), min_key, max_key (uint16 (3,)), enabled"""
        lo, hi, klo, khi = np.empty(3, np.float32), np.empty(3, np.float32), np.empty(3, np.uint16), np.empty(3, np.uint16)
        on = ctypes.c_int()
        _check(self._L.sbm_occ_get_bbx(self._m, lo.ctypes.data, hi.ctypes.data, klo.ctypes.data, khi.ctypes.data, ctypes.byref(on)),
               self._engine._h)
        return dict(min=lo, max=hi, min_key=klo, max_key=khi, enabled=bool(on.value))

    def enable_change_detection(self, enable=True):
        _check(self._L.sbm_occ_enable_change_detection(self._m, int(bool(enable))), self._engine._h)

    def change_detection_enabled(self):
        on = ctypes.c_int()
        _check(self._L.sbm_occ_change_detection_enabled(self._m, ctypes.byref(on)), self._engine._h)
        return bool(on.value)

    def reset_change_detection(self):
        _check(self._L.sbm_occ_reset_change_detection(self._m), self._engine._h)

    def num_changes(self):
        v = ctypes.c_size_t()
        _check(self._L.sbm_occ_num_changes(self._m, ctypes.byref(v)), self._engine._h)
        return v.value

    def changes(self):
        """octomap's changedKeys -> (packed keys uint64 ascending, uint8: 1 created, 0 occupancy flipped) as numpy arrays."""
        n = self.num_changes()
        keys, created = np.empty(n, np.uint64), np.empty(n, np.uint8)
        got = ctypes.c_size_t()
        _check(self._L.sbm_occ_fetch_changes(self._m, keys.ctypes.data if n else None, created.ctypes.data if n else None, n,
                                             ctypes.byref(got)), self._engine._h)
        return keys[:got.value], created[:got.value]

    def changes_device(self):
        """The same as torch CUDA tensors: keys int64, created uint8."""
        torch = _torch()
        n = self.num_changes()
        dev = torch.device("cuda", self._engine._device)
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        created = torch.empty((n,), dtype=torch.uint8, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_fetch_changes_device(self._m, keys.data_ptr() if n else None, created.data_ptr() if n else None, n,
                                                    ctypes.byref(got)), self._engine._h)
        return keys[:got.value], created[:got.value]

    # ---- growth: a larger table on the device, by hand (reserve) or whenever an insert or a load needs it (set_growth) ----------
    @property
    def capacity(self):
        """The nominal capacity in voxels; the table has the power of two >= twice as many slots."""
        v = ctypes.c_size_t()
        _check(self._L.sbm_occ_capacity(self._m, ctypes.byref(v)), self._engine._h)
        return v.value

    def reserve(self, capacity):
        """Move the map into a table for at least `capacity` voxels; everything it holds stays. Never shrinks."""
        _check(self._L.sbm_occ_reserve(self._m, int(capacity)), self._engine._h)
        self._engine._inflight.clear()

    def set_growth(self, enable=True, max_capacity=0):
        """Let inserts and loads grow the table instead of reporting ERR_OCC_FULL, up to max_capacity voxels (0: 2^30). With
        growth on, sync=False calls may synchronise internally."""
        _check(self._L.sbm_occ_set_growth(self._m, int(bool(enable)), int(max_capacity)), self._engine._h)

    def growth(self):
        """dict: enabled, capacity, slots, max_capacity, grown (tables moved), moved (slots carried), redone (launches run again)"""
        g = OccGrowthInfo()
        _check(self._L.sbm_occ_get_growth(self._m, ctypes.byref(g)), self._engine._h)
        return dict(enabled=g.enabled, capacity=g.capacity, slots=g.slots, max_capacity=g.max_capacity, grown=g.grown, moved=g.moved,
                    redone=g.redone)

    # ---- edits by key: octomap's updateNode, setNodeValue and deleteNode on batches of items ----------------------------------------
    def edit(self, items, ops, values, params=None, sync=True, **kw):
        """Mixed items in item order: `items` packed keys (n,) or points (n, 3); ops (n,) uint8 of OCC_EDIT_UPDATE / SET / DELETE,
        or None for all updates; values (n,) float32: the log-odds update or the value to set. All three as torch CUDA tensors
        (keys int64, points and values float32, ops uint8) or all as numpy arrays (the host form, always synchronous). Items that
        name the same voxel take effect in item order. A call given ops may delete and is synchronous whatever `sync` says.
        Raises StereoBMError(ERR_OCC_FULL) when a voxel found no slot."""
        rp = self._ray_params(params, kw)
        if isinstance(items, np.ndarray) or not hasattr(items, "data_ptr"):
            it = np.asarray(items)
            points = it.ndim == 2
            it = np.ascontiguousarray(it, np.float32).reshape(-1, 3) if points else np.ascontiguousarray(it, np.uint64).reshape(-1)
            n = len(it)
            v = np.ascontiguousarray(np.asarray(values, np.float32).reshape(-1))
            o = None if ops is None else np.ascontiguousarray(np.asarray(ops, np.uint8).reshape(-1))
            if len(v) != n or (o is not None and len(o) != n):
                raise StereoBMError(-2, f"{n} items with {len(v)} values" + ("" if o is None else f" and {len(o)} ops"))
            call = self._L.sbm_occ_edit_points if points else self._L.sbm_occ_edit
            _check(call(self._m, n, it.ctypes.data if n else None, o.ctypes.data if o is not None and n else None,
                        v.ctypes.data if n else None, rp), self._engine._h)
            self._engine._inflight.clear()
            return
        torch = _torch()
        points = items.dim() == 2
        want = torch.float32 if points else torch.int64
        for t, dtype, what in ((items, want, "items"), (values, torch.float32, "values")) + (() if ops is None else ((ops, torch.uint8, "ops"),)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.device.index != self._engine._device:
                raise StereoBMError(-2, f"{what} must be a CUDA {dtype} tensor on the engine's device")
        it, v, o = items.contiguous(), values.contiguous().reshape(-1), None if ops is None else ops.contiguous().reshape(-1)
        n = it.shape[0]
        if (points and it.shape[1] != 3) or v.shape[0] != n or (o is not None and o.shape[0] != n):
            raise StereoBMError(-2, "items (n,) keys or (n, 3) points, with n values and n ops")
        torch.cuda.current_stream(it.device).synchronize()
        call = self._L.sbm_occ_edit_points_device if points else self._L.sbm_occ_edit_device
        _check(call(self._m, n, it.data_ptr() if n else None, o.data_ptr() if o is not None and n else None, v.data_ptr() if n else None, rp,
                    1 if sync else 0), self._engine._h)
        self._after(sync or o is not None, (it, v, o))

    def update_nodes(self, items, values, params=None, sync=True, **kw):
        """octomap's updateNode(key | point, float) per item. values: (n,) log-odds updates, or one bool for every item --
        updateNode(., occupied): the hit or the miss log-odds of the parameters, formed on the host."""
        if isinstance(values, (bool, np.bool_)):
            rp = params if params is not None else occ_ray_params(**kw)
            params, kw = rp, {}
            u = float(occ_ray_logodds(rp)[0 if values else 1])
            n = len(items)
            values = np.full(n, u, np.float32) if not hasattr(items, "data_ptr") else _torch().full((n,), u, dtype=_torch().float32, device=items.device)
        self.edit(items, None, values, params, sync, **kw)

    def set_node_values(self, items, values, params=None, sync=True, **kw):
        """octomap's setNodeValue(key | point, float) per item."""
        n = len(items)
        if hasattr(items, "data_ptr"):
            ops = _torch().full((n,), OCC_EDIT_SET, dtype=_torch().uint8, device=items.device)
        else:
            ops = np.full(n, OCC_EDIT_SET, np.uint8)
        self.edit(items, ops, values, params, sync, **kw)

    def delete_nodes(self, keys, depth=0):
        """octomap's deleteNode(key, depth) per key: every stored voxel that agrees with a key in the top `depth` bits of each
        component goes, with all it holds (depth 0 means 16). keys: packed, a torch CUDA int64 tensor or a numpy array; points
        (n, 3) as a numpy array are turned into keys on the host (a point without a key is left out). Synchronous; either mode."""
        if hasattr(keys, "data_ptr"):
            torch = _torch()
            if keys.dtype != torch.int64 or not keys.is_cuda or keys.dim() != 1 or keys.device.index != self._engine._device:
                raise StereoBMError(-2, "keys must be a CUDA int64 (n,) tensor on the engine's device")
            k = keys.contiguous()
            torch.cuda.current_stream(k.device).synchronize()
            _check(self._L.sbm_occ_delete_device(self._m, k.shape[0], k.data_ptr() if k.shape[0] else None, int(depth)), self._engine._h)
        else:
            k = np.asarray(keys)
            if k.ndim == 2:
                f = np.floor(np.float64(1.0 / self._p.resolution) * k.astype(np.float32).astype(np.float64))
                with np.errstate(invalid="ignore"):
                    ok = ((f >= -32768) & (f < 32768)).all(axis=1)
                q = (f[ok] + 32768).astype(np.uint64)
                k = q[:, 0] << np.uint64(32) | q[:, 1] << np.uint64(16) | q[:, 2]
            k = np.ascontiguousarray(k, np.uint64).reshape(-1)
            _check(self._L.sbm_occ_delete(self._m, len(k), k.ctypes.data if len(k) else None, int(depth)), self._engine._h)
        self._engine._inflight.clear()

    def delete_box(self, min_key, max_key, outside=False):
        """Remove every voxel inside (outside=True: outside) the key box, both ends inclusive; min > max on an axis is the empty
        box. Synchronous; either mode; the insert's own box is not touched."""
        lo = np.ascontiguousarray(np.asarray(min_key, np.uint16).reshape(3))
        hi = np.ascontiguousarray(np.asarray(max_key, np.uint16).reshape(3))
        _check(self._L.sbm_occ_delete_box(self._m, lo.ctypes.data, hi.ctypes.data, int(bool(outside))), self._engine._h)
        self._engine._inflight.clear()

    def last_edit(self):
        """dict: items, skipped, lost (to a full table), created, removed of the last edit or delete call. Synchronises."""
        e = OccEditInfo()
        _check(self._L.sbm_occ_last_edit(self._m, ctypes.byref(e)), self._engine._h)
        return dict(items=e.items, skipped=e.skipped, lost=e.lost, created=e.created, removed=e.removed)

    # ---- time stamps per voxel: octomap's OcTreeStamped on the map's own clock ------------------------------------------------------
    def enable_stamps(self):
        """One uint32 stamp per voxel from here on (existing voxels: 0). Log-odds maps only; a map holds colours or stamps, not
        both. Every updateNode of a scan or an edit then stamps its voxel with the map's clock unless octomap's early return
        applies (the voxel exists and sits at the clamp in the direction of the update)."""
        _check(self._L.sbm_occ_stamp_enable(self._m), self._engine._h)

    def stamps_enabled(self):
        on = ctypes.c_int()
        _check(self._L.sbm_occ_stamp_enabled(self._m, ctypes.byref(on)), self._engine._h)
        return bool(on.value)

    def set_time(self, clock):
        """The map's clock, a uint32 the caller sets: what the stamping calls write. The library never reads the wall clock."""
        _check(self._L.sbm_occ_stamp_set_time(self._m, int(clock) & 0xFFFFFFFF), self._engine._h)

    def time(self):
        c = ctypes.c_uint32()
        _check(self._L.sbm_occ_stamp_time(self._m, ctypes.byref(c)), self._engine._h)
        return c.value

    def degrade_outdated(self, time_thres, params=None):
        """octomap's degradeOutdatedNodes(time_thres): every occupied voxel with (uint32)(clock - stamp) > time_thres gets one miss
        update, clamped; the stamps stay. -> how many voxels it degraded. Synchronous."""
        p = params if params is not None else getattr(self, "_rp", None) or occ_ray_params()   # as the snapshot: the last insert's
        n = ctypes.c_uint64()
        _check(self._L.sbm_occ_stamp_degrade(self._m, int(time_thres) & 0xFFFFFFFF, ctypes.byref(p), ctypes.byref(n)), self._engine._h)
        self._engine._inflight.clear()
        return n.value

    def forget_older_than(self, time_thres):
        """Delete every voxel with (uint32)(clock - stamp) > time_thres, whatever its value (an extension, not octomap) -> how
        many. Synchronous; last_edit() holds its counts."""
        n = ctypes.c_uint64()
        _check(self._L.sbm_occ_stamp_forget(self._m, int(time_thres) & 0xFFFFFFFF, ctypes.byref(n)), self._engine._h)
        self._engine._inflight.clear()
        return n.value

    def search_stamps(self, points, occupancy_thres_log=0.0, sync=True):
        """search(point) with the voxel's stamp, on (n, 3) points: a numpy array -> numpy (int32 states, uint32 value words, uint32
        stamps), or a torch CUDA float32 tensor -> three torch int32 tensors. An unknown voxel, a point outside the key space and
        every voxel of a map without stamps answer 0."""
        if isinstance(points, np.ndarray):
            p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            n = len(p)
            state, value, stamp = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(n, np.uint32)
            _check(self._L.sbm_occ_stamp_search(self._m, n, p.ctypes.data if n else None, float(occupancy_thres_log), state.ctypes.data if n else None,
                                                value.ctypes.data if n else None, stamp.ctypes.data if n else None), self._engine._h)
            return state, value, stamp
        torch = _torch()
        p = self._cuda_f32(points, "points")
        n = p.shape[0]
        state, value, stamp = (torch.empty((n,), dtype=torch.int32, device=p.device) for _ in range(3))
        torch.cuda.current_stream(p.device).synchronize()
        _check(self._L.sbm_occ_stamp_search_device(self._m, n, p.data_ptr() if n else None, float(occupancy_thres_log), state.data_ptr() if n else None,
                                                   value.data_ptr() if n else None, stamp.data_ptr() if n else None, 1 if sync else 0), self._engine._h)
        self._after(sync, (p, state, value, stamp))
        return state, value, stamp

    def fetch_stamps(self, allow_overflow=False):
        """(packed keys uint64 ascending, log-odds float32, stamps uint32) of a log-odds map as numpy arrays."""
        n = self.size()
        keys, lo, stamps = np.empty(n, np.uint64), np.empty(n, np.float32), np.empty(n, np.uint32)
        got = ctypes.c_size_t()
        st = self._L.sbm_occ_stamp_fetch(self._m, keys.ctypes.data if n else None, lo.ctypes.data if n else None, stamps.ctypes.data if n else None, n,
                                         ctypes.byref(got))
        if not (st == ERR_OCC_FULL and allow_overflow):
            _check(st, self._engine._h)
        return keys[:got.value], lo[:got.value], stamps[:got.value]

    def fetch_stamps_device(self):
        """The same as torch CUDA tensors: keys int64, log-odds float32, stamps int32."""
        torch = _torch()
        n = self.size()
        dev = torch.device("cuda", self._engine._device)
        keys, lo, stamps = torch.empty((n,), dtype=torch.int64, device=dev), torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_stamp_fetch_device(self._m, keys.data_ptr() if n else None, lo.data_ptr() if n else None, stamps.data_ptr() if n else None, n,
                                                  ctypes.byref(got)), self._engine._h)
        return keys[:got.value], lo[:got.value], stamps[:got.value]

    # ---- colour per voxel: octomap's ColorOcTree::setNodeColor and averageNodeColor on batches of items ----------------------------
    def _color(self, items, colors, op, sync):
        if isinstance(items, np.ndarray) or not hasattr(items, "data_ptr"):
            it = np.asarray(items)
            points = it.ndim == 2
            it = np.ascontiguousarray(it, np.float32).reshape(-1, 3) if points else np.ascontiguousarray(it, np.uint64).reshape(-1)
            n = len(it)
            c = occ_color_words(colors)
            if len(c) != n:
                raise StereoBMError(-2, f"{n} items with {len(c)} colours")
            call = self._L.sbm_occ_color_points if points else self._L.sbm_occ_color_keys
            _check(call(self._m, n, it.ctypes.data if n else None, c.ctypes.data if n else None, op), self._engine._h)
            self._engine._inflight.clear()
            return
        torch = _torch()
        points = items.dim() == 2
        want = torch.float32 if points else torch.int64
        for t, dtype, what in ((items, want, "items"), (colors, torch.int32, "colors")):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.device.index != self._engine._device:
                raise StereoBMError(-2, f"{what} must be a CUDA {dtype} tensor on the engine's device")
        it, c = items.contiguous(), colors.contiguous().reshape(-1)
        n = it.shape[0]
        if (points and it.shape[1] != 3) or c.shape[0] != n:
            raise StereoBMError(-2, "items (n,) keys or (n, 3) points, with n colour words")
        torch.cuda.current_stream(it.device).synchronize()
        call = self._L.sbm_occ_color_points_device if points else self._L.sbm_occ_color_keys_device
        _check(call(self._m, n, it.data_ptr() if n else None, c.data_ptr() if n else None, op, 1 if sync else 0), self._engine._h)
        self._after(sync, (it, c))

    def set_colors(self, items, colors, sync=True):
        """octomap's setNodeColor(key, r, g, b) per item, in item order. `items` packed keys (n,) or points (n, 3); colors (n, 3)
        uint8 r, g, b or (n,) words r | g << 8 | b << 16. Both as numpy arrays (the host form, synchronous) or as torch CUDA
        tensors (keys int64, points float32, colour WORDS int32). An item whose voxel is unknown does nothing; white (255, 255,
        255) unsets. Log-odds maps only."""
        self._color(items, colors, OCC_COLOR_SET, sync)

    def average_colors(self, items, colors, sync=True):
        """octomap's averageNodeColor per item, in item order: the item's colour where the voxel has none, else (prev + new) / 2
        per channel in int. Arguments as set_colors."""
        self._color(items, colors, OCC_COLOR_AVERAGE, sync)

    def last_colors(self):
        """dict: items, found, unknown (a valid key without a voxel), skipped (no key) of the last colour batch. Synchronises."""
        e = OccColorInfo()
        _check(self._L.sbm_occ_color_last(self._m, ctypes.byref(e)), self._engine._h)
        return dict(items=e.items, found=e.found, unknown=e.unknown, skipped=e.skipped)

    def search_colors(self, points, occupancy_thres_log=0.0, sync=True):
        """search(point) with the voxel's colour, on (n, 3) points: a numpy array -> numpy (int32 states, uint32 value words, uint32
        colour words), or a torch CUDA float32 tensor -> three torch int32 tensors. An unknown voxel, a point outside the key
        space and every voxel of a map without colours answer OCC_COLOR_WHITE. occ_color_rgb turns words into (n, 3) uint8."""
        if isinstance(points, np.ndarray):
            p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            n = len(p)
            state, value, color = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(n, np.uint32)
            _check(self._L.sbm_occ_color_search(self._m, n, p.ctypes.data if n else None, float(occupancy_thres_log), state.ctypes.data if n else None,
                                                value.ctypes.data if n else None, color.ctypes.data if n else None), self._engine._h)
            return state, value, color
        torch = _torch()
        p = self._cuda_f32(points, "points")
        n = p.shape[0]
        state, value, color = (torch.empty((n,), dtype=torch.int32, device=p.device) for _ in range(3))
        torch.cuda.current_stream(p.device).synchronize()
        _check(self._L.sbm_occ_color_search_device(self._m, n, p.data_ptr() if n else None, float(occupancy_thres_log), state.data_ptr() if n else None,
                                                   value.data_ptr() if n else None, color.data_ptr() if n else None, 1 if sync else 0), self._engine._h)
        self._after(sync, (p, state, value, color))
        return state, value, color

    def fetch_colors(self, allow_overflow=False):
        """(packed keys uint64 ascending, log-odds float32, colour words uint32) of a log-odds map as numpy arrays."""
        n = self.size()
        keys, lo, col = np.empty(n, np.uint64), np.empty(n, np.float32), np.empty(n, np.uint32)
        got = ctypes.c_size_t()
        st = self._L.sbm_occ_color_fetch(self._m, keys.ctypes.data if n else None, lo.ctypes.data if n else None, col.ctypes.data if n else None, n,
                                         ctypes.byref(got))
        if not (st == ERR_OCC_FULL and allow_overflow):
            _check(st, self._engine._h)
        return keys[:got.value], lo[:got.value], col[:got.value]

    def fetch_colors_device(self):
        """The same as torch CUDA tensors: keys int64, log-odds float32, colour words int32."""
        torch = _torch()
        n = self.size()
        dev = torch.device("cuda", self._engine._device)
        keys, lo, col = torch.empty((n,), dtype=torch.int64, device=dev), torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_color_fetch_device(self._m, keys.data_ptr() if n else None, lo.data_ptr() if n else None, col.data_ptr() if n else None, n,
                                                  ctypes.byref(got)), self._engine._h)
        return keys[:got.value], lo[:got.value], col[:got.value]

    def load_color_ot(self, data_or_path, sync=True):
        """AbstractOcTree::read of a ColorOcTree stream -- bytes (or a uint8 array), or the path of a file: the map's content is
        replaced by the stream's voxels, each with its leaf's float and its leaf's colour. A plain OcTree stream is refused
        (load_ot reads that)."""
        if isinstance(data_or_path, (str, os.PathLike)):
            st = self._L.sbm_occ_color_ot_read(self._m, os.fsencode(data_or_path), 1 if sync else 0)
        else:
            b = _stream(data_or_path)
            st = self._L.sbm_occ_color_ot_load(self._m, b.ctypes.data if len(b) else None, len(b), 1 if sync else 0)
        _check(st, self._engine._h)
        self._engine._inflight.clear()

    def load_binary(self, data_or_path, params=None, sync=True, **kw):
        """octomap's readBinary: replace the map's content by the voxels of a .bt stream -- bytes (or a uint8 array), or the
        path of a file (str or os.PathLike). Occupied leaves hold the clamp-max log-odds of `params`, free leaves clamp min;
        the map is then a log-odds map that further insert_cloud / insert_rays scans continue."""
        rp = self._ray_params(params, kw)
        if isinstance(data_or_path, (str, os.PathLike)):
            st = self._L.sbm_occ_read_binary(self._m, os.fsencode(data_or_path), rp, 1 if sync else 0)
        else:
            b = _stream(data_or_path)
            st = self._L.sbm_occ_load_binary(self._m, b.ctypes.data if len(b) else None, len(b), rp, 1 if sync else 0)
        _check(st, self._engine._h)
        if sync:
            self._engine._inflight.clear()

    def load_ot(self, data_or_path, sync=True):
        """octomap's AbstractOcTree::read: replace the map's content by the voxels of an .ot stream -- bytes (or a uint8 array),
        or the path of a file (str or os.PathLike). Every voxel holds its leaf's float, unclamped; the map is then a log-odds map
        that further insert_cloud / insert_rays scans continue."""
        if isinstance(data_or_path, (str, os.PathLike)):
            st = self._L.sbm_occ_ot_read(self._m, os.fsencode(data_or_path), 1 if sync else 0)
        else:
            b = _stream(data_or_path)
            st = self._L.sbm_occ_ot_load(self._m, b.ctypes.data if len(b) else None, len(b), 1 if sync else 0)
        _check(st, self._engine._h)
        if sync:
            self._engine._inflight.clear()

    def load_stamped_ot(self, data_or_path, sync=True):
        """AbstractOcTree::read of an `id OcTreeStamped` stream -- bytes (or a uint8 array), or the path of a file: as load_ot, and
        every stamp is 0 afterwards (the stream carries none). A plain OcTree stream is refused (load_ot reads that)."""
        if isinstance(data_or_path, (str, os.PathLike)):
            st = self._L.sbm_occ_stamp_ot_read(self._m, os.fsencode(data_or_path), 1 if sync else 0)
        else:
            b = _stream(data_or_path)
            st = self._L.sbm_occ_stamp_ot_load(self._m, b.ctypes.data if len(b) else None, len(b), 1 if sync else 0)
        _check(st, self._engine._h)
        if sync:
            self._engine._inflight.clear()

    def fetch_logodds(self, allow_overflow=False):
        """(packed keys uint64 ascending, log-odds float32) of a log-odds map as numpy arrays."""
        n = self.size()
        keys, lo = np.empty(n, np.uint64), np.empty(n, np.float32)
        got = ctypes.c_size_t()
        st = self._L.sbm_occ_fetch_logodds(self._m, keys.ctypes.data if n else None, lo.ctypes.data if n else None, n,
                                           ctypes.byref(got))
        if not (st == ERR_OCC_FULL and allow_overflow):
            _check(st, self._engine._h)
        return keys[:got.value], lo[:got.value]

    def write_binary_logodds(self, path, params=None):
        """tree.writeBinary(path) of a log-odds map, thresholded with `params` (default: those of the last log-odds insert)."""
        rp = params if params is not None else getattr(self, "_rp", None) or occ_ray_params()
        keys, lo = self.fetch_logodds()
        occ_write_binary_logodds(keys, lo, path, self._p.resolution, float(occ_ray_logodds(rp)[4]))

    # ---- queries: octomap's search and castRay, per depth-16 voxel; the map is not changed ------------------------------------
    def _query_params(self, params, kw):
        if params is not None and kw:
            raise TypeError("pass either an OccQueryParams or keyword parameters")
        return params if params is not None else occ_query_params(**kw)

    def _cuda_f32(self, a, what, cols=3):
        torch = _torch()
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or not a.is_cuda or a.dim() != 2 or a.shape[1] != cols or \
                a.device.index != self._engine._device:
            raise StereoBMError(-2, f"{what} must be a CUDA float32 (n, {cols}) tensor on the engine's device")
        return a.contiguous()

    def search(self, points, occupancy_thres_log=0.0, sync=True):
        """octomap's search(point) on (n, 3) points: a torch CUDA float32 tensor (-> torch int32 states, int32 value words) or
        a numpy array (the host form -> numpy int32 states, uint32 value words). A state is OCC_CELL_OUT / UNKNOWN / FREE /
        OCCUPIED; the value word holds the float log-odds (NaN where nothing is stored) in log-odds mode, the hit count in hit
        mode: view it as float32 for a log-odds map."""
        if isinstance(points, np.ndarray):
            p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            state, value = np.empty(len(p), np.int32), np.empty(len(p), np.uint32)
            _check(self._L.sbm_occ_search(self._m, len(p), p.ctypes.data if len(p) else None, float(occupancy_thres_log),
                                          state.ctypes.data if len(p) else None, value.ctypes.data if len(p) else None), self._engine._h)
            return state, value
        torch = _torch()
        p = self._cuda_f32(points, "points")
        n = p.shape[0]
        state = torch.empty((n,), dtype=torch.int32, device=p.device)
        value = torch.empty((n,), dtype=torch.int32, device=p.device)
        torch.cuda.current_stream(p.device).synchronize()
        _check(self._L.sbm_occ_search_device(self._m, n, p.data_ptr() if n else None, float(occupancy_thres_log),
                                             state.data_ptr() if n else None, value.data_ptr() if n else None, 1 if sync else 0),
               self._engine._h)
        self._after(sync, (p, state, value))
        return state, value

    def _after(self, sync, held):
        if sync:
            self._engine._inflight.clear()
        else:
            self._engine._inflight.append(held)

    def cast_rays(self, origins, directions, params=None, sync=True, **kw):
        """octomap's castRay on n rays -> (status, end): OCC_RAY_* per ray and the (n, 3) end points (NaN for OCC_RAY_NONE).
        directions (n, 3) as a torch CUDA float32 tensor, with origins such a tensor or three floats that every ray starts
        from; or both as numpy arrays (the host form, always synchronous)."""
        qp = self._query_params(params, kw)
        if isinstance(directions, np.ndarray):
            d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
            o = np.ascontiguousarray(np.asarray(origins, np.float32)).reshape(-1, 3)
            shared = len(o) == 1 and np.ndim(origins) == 1
            if not shared and len(o) != len(d):
                raise StereoBMError(-2, f"{len(o)} origins for {len(d)} rays")
            status, end = np.empty(len(d), np.int32), np.empty((len(d), 3), np.float32)
            _check(self._L.sbm_occ_cast_rays(self._m, len(d), o.ctypes.data if len(o) else None, int(shared),
                                             d.ctypes.data if len(d) else None, ctypes.byref(qp), status.ctypes.data if len(d) else None,
                                             end.ctypes.data if len(d) else None), self._engine._h)
            return status, end
        torch = _torch()
        d = self._cuda_f32(directions, "directions")
        n = d.shape[0]
        shared = not isinstance(origins, torch.Tensor)
        if shared:
            o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(3))
            o_ptr = o.ctypes.data
        else:
            o = self._cuda_f32(origins, "origins")
            if o.shape[0] != n:
                raise StereoBMError(-2, f"{o.shape[0]} origins for {n} rays")
            o_ptr = o.data_ptr() if n else None
        status = torch.empty((n,), dtype=torch.int32, device=d.device)
        end = torch.empty((n, 3), dtype=torch.float32, device=d.device)
        torch.cuda.current_stream(d.device).synchronize()
        _check(self._L.sbm_occ_cast_rays_device(self._m, n, o_ptr, int(shared), d.data_ptr() if n else None, ctypes.byref(qp),
                                                status.data_ptr() if n else None, end.data_ptr() if n else None, 1 if sync else 0),
               self._engine._h)
        self._after(sync, (o, d, status, end))
        return status, end

    def ray_intersections(self, origins, directions, centres, delta=0.0, sync=True):
        """octomap's getRayIntersection on n rays -> (found, xyz): int32 per ray and the (n, 3) points where each ray enters the
        voxel around its centre (NaN where found is 0). directions and centres (n, 3) as torch CUDA float32 tensors, with origins
        such a tensor or three floats that every ray starts from; or all as numpy arrays (the host form, always synchronous).
        The directions are not normalised."""
        if isinstance(directions, np.ndarray):
            d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
            c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
            o = np.ascontiguousarray(np.asarray(origins, np.float32)).reshape(-1, 3)
            shared = len(o) == 1 and np.ndim(origins) == 1
            if (not shared and len(o) != len(d)) or len(c) != len(d):
                raise StereoBMError(-2, f"{len(o)} origins and {len(c)} centres for {len(d)} rays")
            n = len(d)
            found, xyz = np.empty(n, np.int32), np.empty((n, 3), np.float32)
            _check(self._L.sbm_occ_ray_intersections(self._m, n, o.ctypes.data if len(o) else None, int(shared), d.ctypes.data if n else None,
                                                     c.ctypes.data if n else None, float(delta), xyz.ctypes.data if n else None,
                                                     found.ctypes.data if n else None), self._engine._h)
            return found, xyz
        torch = _torch()
        d = self._cuda_f32(directions, "directions")
        c = self._cuda_f32(centres, "centres")
        n = d.shape[0]
        shared = not isinstance(origins, torch.Tensor)
        if shared:
            o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(3))
            o_ptr = o.ctypes.data
        else:
            o = self._cuda_f32(origins, "origins")
            o_ptr = o.data_ptr() if n else None
        if (not shared and o.shape[0] != n) or c.shape[0] != n:
            raise StereoBMError(-2, f"origins and centres must hold {n} rows")
        found = torch.empty((n,), dtype=torch.int32, device=d.device)
        xyz = torch.empty((n, 3), dtype=torch.float32, device=d.device)
        torch.cuda.current_stream(d.device).synchronize()
        _check(self._L.sbm_occ_ray_intersections_device(self._m, n, o_ptr, int(shared), d.data_ptr() if n else None,
                                                        c.data_ptr() if n else None, float(delta), xyz.data_ptr() if n else None,
                                                        found.data_ptr() if n else None, 1 if sync else 0), self._engine._h)
        self._after(sync, (o, d, c, found, xyz))
        return found, xyz

    def cast_view(self, width, height, model, pose, scale=1, params=None, sync=True, **kw):
        """One ray per pixel of a width x height virtual camera at `pose` (12 floats), built on the device -> torch CUDA
        (height, width) int32 statuses and (height, width, 3) float32 end points: cast_rays on the rays the header states."""
        torch = _torch()
        qp = self._query_params(params, kw)
        p = _poses(pose, 1)
        dev = torch.device("cuda", self._engine._device)
        status = torch.empty((int(height), int(width)), dtype=torch.int32, device=dev)
        end = torch.empty((int(height), int(width), 3), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_cast_view_device(self._m, int(width), int(height), int(scale), ctypes.byref(model), p.ctypes.data,
                                                ctypes.byref(qp), status.data_ptr(), end.data_ptr(), 1 if sync else 0), self._engine._h)
        self._after(sync, (status, end))
        return status, end

    def size(self):
        v = ctypes.c_size_t()
        _check(self._L.sbm_occ_size(self._m, ctypes.byref(v)), self._engine._h)
        return v.value

    def overflow(self):
        v = ctypes.c_uint64()
        _check(self._L.sbm_occ_overflow(self._m, ctypes.byref(v)), self._engine._h)
        return v.value

    def keys(self, allow_overflow=False):
        """(packed keys uint64 ascending, hit counts uint32) as numpy arrays. A map that overflowed raises unless
        allow_overflow is set."""
        n = self.size()
        keys, hits = np.empty(n, np.uint64), np.empty(n, np.uint32)
        got = ctypes.c_size_t()
        st = self._L.sbm_occ_fetch(self._m, keys.ctypes.data if n else None, hits.ctypes.data if n else None, n, ctypes.byref(got))
        if not (st == ERR_OCC_FULL and allow_overflow):
            _check(st, self._engine._h)
        return keys[:got.value], hits[:got.value]

    def keys_device(self, allow_overflow=False):
        """The same as torch CUDA tensors: keys int64 (the packed keys are below 2^48), hits int32."""
        torch = _torch()
        n = self.size()
        dev = torch.device("cuda", self._engine._device)
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        hits = torch.empty((n,), dtype=torch.int32, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        st = self._L.sbm_occ_fetch_device(self._m, keys.data_ptr() if n else None, hits.data_ptr() if n else None, n, ctypes.byref(got))
        if not (st == ERR_OCC_FULL and allow_overflow):
            _check(st, self._engine._h)
        return keys[:got.value], hits[:got.value]

    def write_binary(self, path):
        """tree.writeBinary(path) of the reference: the .bt stream of the stored voxels."""
        occ_write_binary(self.keys()[0], path, self._p.resolution)

    def tree(self, reading=OCC_TREE_LOGODDS, params=None, sync=True):
        """A built OccupancyTree over this map: the sixteen levels above the voxels, as a snapshot. reading OCC_TREE_LOGODDS
        (log-odds maps) or OCC_TREE_MAXLIKELIHOOD, whose constants come from `params` (default: those of the last log-odds
        insert)."""
        return OccupancyTree(self).build(reading, params, sync)

    def profile(self):
        return self._engine._profile(("occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast",
                                     "occ_load"))


class OccupancyTree:
    """octomap's tree above the voxels of an OccupancyMap (sbm_occ_tree): a snapshot, built and queried on the device. The
    engine of the map must outlive it; the map is read by build() only."""

    def __init__(self, omap):
        self._map = omap
        self._engine = omap._engine
        self._L = omap._L
        self._t = ctypes.c_void_p()
        _check(self._L.sbm_occ_tree_create(omap._m, ctypes.byref(self._t)), self._engine._h)

    def close(self):
        t = getattr(self, "_t", None)
        if t:
            self._L.sbm_occ_tree_destroy(t)
            self._t = None

    def __del__(self):
        self.close()

    def build(self, reading=OCC_TREE_LOGODDS, params=None, sync=True):
        """A new snapshot of the map; returns self."""
        if params is None and reading == OCC_TREE_MAXLIKELIHOOD:
            params = getattr(self._map, "_rp", None) or occ_ray_params()
        self._rp = params
        _check(self._L.sbm_occ_tree_build(self._t, int(reading), ctypes.byref(params) if params is not None else None,
                                          1 if sync else 0), self._engine._h)
        return self

    def info(self):
        """dict: voxels, nodes, leaves (calcNumNodes and getNumLeafNodes after prune()), nodes_at / leaves_at per depth 0..16,
        key_min / key_max per axis over the stored voxels."""
        c = OccTreeCounts()
        _check(self._L.sbm_occ_tree_info(self._t, ctypes.byref(c)), self._engine._h)
        return dict(voxels=c.voxels, nodes=c.nodes, leaves=c.leaves, nodes_at=list(c.nodes_at), leaves_at=list(c.leaves_at),
                    key_min=list(c.key_min), key_max=list(c.key_max))

    def search(self, points, depth=0, occupancy_thres_log=0.0, sync=True):
        """octomap's search(point, depth) on (n, 3) points -> (state, value word, found depth): torch CUDA int32 tensors for a
        torch CUDA float32 tensor, numpy int32 / uint32 / int32 for a numpy array (the host form). The value word holds the
        node's float (NaN where there is none)."""
        if isinstance(points, np.ndarray):
            p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            n = len(p)
            state, value, found = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(n, np.int32)
            _check(self._L.sbm_occ_tree_search(self._t, n, p.ctypes.data if n else None, int(depth), float(occupancy_thres_log),
                                               state.ctypes.data if n else None, value.ctypes.data if n else None,
                                               found.ctypes.data if n else None), self._engine._h)
            return state, value, found
        torch = _torch()
        p = self._map._cuda_f32(points, "points")
        n = p.shape[0]
        state, value, found = (torch.empty((n,), dtype=torch.int32, device=p.device) for _ in range(3))
        torch.cuda.current_stream(p.device).synchronize()
        _check(self._L.sbm_occ_tree_search_device(self._t, n, p.data_ptr() if n else None, int(depth), float(occupancy_thres_log),
                                                  state.data_ptr() if n else None, value.data_ptr() if n else None,
                                                  found.data_ptr() if n else None, 1 if sync else 0), self._engine._h)
        self._map._after(sync, (p, state, value, found))
        return state, value, found

    def _leaf_count(self, max_depth):
        i = self.info()
        d = int(max_depth) or 16
        if not 0 < d <= 16:
            raise StereoBMError(-2, f"max_depth {max_depth} is outside 0..16")
        return sum(i["leaves_at"][:d + 1]) + i["nodes_at"][d] - i["leaves_at"][d]

    def leaves(self, max_depth=0):
        """octomap's begin_leafs(max_depth) -> (centre keys uint64, depths int32, values float32) as numpy arrays, in
        octomap's iteration order."""
        n = self._leaf_count(max_depth)
        keys, depth, value = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.float32)
        got = ctypes.c_size_t()
        _check(self._L.sbm_occ_tree_leaves(self._t, int(max_depth), keys.ctypes.data if n else None, depth.ctypes.data if n else None,
                                           value.ctypes.data if n else None, n, ctypes.byref(got)), self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value]

    def leaves_device(self, max_depth=0):
        """The same as torch CUDA tensors: keys int64, depths int32, values float32."""
        torch = _torch()
        n = self._leaf_count(max_depth)
        dev = torch.device("cuda", self._engine._device)
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        depth = torch.empty((n,), dtype=torch.int32, device=dev)
        value = torch.empty((n,), dtype=torch.float32, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_tree_leaves_device(self._t, int(max_depth), keys.data_ptr() if n else None,
                                                  depth.data_ptr() if n else None, value.data_ptr() if n else None, n,
                                                  ctypes.byref(got)), self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value]

    def _box(self, lo, hi):
        """-> (by points, two host arrays of three)"""
        points = np.asarray(lo).dtype.kind == "f" or np.asarray(hi).dtype.kind == "f"
        dt = np.float32 if points else np.uint16
        if not points and (np.asarray(lo).min() < 0 or np.asarray(hi).min() < 0 or np.asarray(lo).max() > 65535 or np.asarray(hi).max() > 65535):
            raise StereoBMError(-2, "a key lies in 0..65535")
        return points, np.ascontiguousarray(np.asarray(lo, dt).reshape(3)), np.ascontiguousarray(np.asarray(hi, dt).reshape(3))

    def _leaves_bbx(self, lo, hi, max_depth, device):
        points, lo, hi = self._box(lo, hi)
        call = getattr(self._L, "sbm_occ_bbx_leaves" + ("_points" if points else "") + ("_device" if device else ""))
        got = ctypes.c_size_t()
        st = call(self._t, lo.ctypes.data, hi.ctypes.data, int(max_depth), None, None, None, 0, ctypes.byref(got))       # the count
        if st not in (0, -2) or (st == -2 and got.value == 0):
            _check(st, self._engine._h)
        n = got.value
        if device:
            torch = _torch()
            dev = torch.device("cuda", self._engine._device)
            keys = torch.empty((n,), dtype=torch.int64, device=dev)
            depth = torch.empty((n,), dtype=torch.int32, device=dev)
            value = torch.empty((n,), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ptr = [a.data_ptr() if n else None for a in (keys, depth, value)]
        else:
            keys, depth, value = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.float32)
            ptr = [a.ctypes.data if n else None for a in (keys, depth, value)]
        _check(call(self._t, lo.ctypes.data, hi.ctypes.data, int(max_depth), ptr[0], ptr[1], ptr[2], n, ctypes.byref(got)), self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value]

    def leaves_bbx(self, lo, hi, max_depth=0):
        """octomap's begin_leafs_bbx(min, max, max_depth) -> (centre keys uint64, depths int32, values float32) as numpy arrays in
        octomap's iteration order. lo / hi: three integer keys each (both ends inclusive), or three floats each (the point
        form: a corner without a key visits nothing)."""
        return self._leaves_bbx(lo, hi, max_depth, False)

    def leaves_bbx_device(self, lo, hi, max_depth=0):
        """The same as torch CUDA tensors: keys int64, depths int32, values float32."""
        return self._leaves_bbx(lo, hi, max_depth, True)

    def _unknown(self, pmin, pmax, depth, device):
        lo = np.ascontiguousarray(np.asarray(pmin, np.float32).reshape(3))
        hi = np.ascontiguousarray(np.asarray(pmax, np.float32).reshape(3))
        call = self._L.sbm_occ_unknown_device if device else self._L.sbm_occ_unknown
        got = ctypes.c_size_t()
        st = call(self._t, lo.ctypes.data, hi.ctypes.data, int(depth), None, 0, ctypes.byref(got))       # the count
        if st not in (0, -2) or (st == -2 and got.value == 0):
            _check(st, self._engine._h)
        n = got.value
        if device:
            torch = _torch()
            dev = torch.device("cuda", self._engine._device)
            xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ptr = xyz.data_ptr() if n else None
        else:
            xyz = np.empty((n, 3), np.float32)
            ptr = xyz.ctypes.data if n else None
        _check(call(self._t, lo.ctypes.data, hi.ctypes.data, int(depth), ptr, n, ctypes.byref(got)), self._engine._h)
        return xyz[:got.value]

    def unknown_centers(self, pmin, pmax, depth=0):
        """octomap's getUnknownLeafCenters(centres, pmin, pmax, depth) -> (n, 3) float32 numpy array in octomap's push order."""
        return self._unknown(pmin, pmax, depth, False)

    def unknown_centers_device(self, pmin, pmax, depth=0):
        """The same as a torch CUDA float32 tensor."""
        return self._unknown(pmin, pmax, depth, True)

    def metric_min_max(self):
        """octomap's getMetricMin and getMetricMax -> (min, max), float64 arrays of three; six zeros for an empty tree."""
        lo, hi = np.zeros(3, np.float64), np.zeros(3, np.float64)
        _check(self._L.sbm_occ_metric(self._t, lo.ctypes.data, hi.ctypes.data), self._engine._h)
        return lo, hi

    def metric_size(self):
        """octomap's getMetricSize: max - min per axis."""
        lo, hi = self.metric_min_max()
        return np.array([hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]], np.float64)

    def volume(self):
        """octomap's volume(): x * y * z of the metric size."""
        x, y, z = (float(v) for v in self.metric_size())
        return x * y * z

    def binary(self):
        """The body of the .bt stream (a MAXLIKELIHOOD tree) as a torch CUDA uint8 tensor: two bytes per non-leaf node."""
        torch = _torch()
        i = self.info()
        n = 2 * (i["nodes"] - i["leaves"])
        out = torch.empty((n,), dtype=torch.uint8, device=torch.device("cuda", self._engine._device))
        got = ctypes.c_size_t()
        torch.cuda.current_stream(out.device).synchronize()
        _check(self._L.sbm_occ_tree_binary_device(self._t, out.data_ptr() if n else None, n, ctypes.byref(got)), self._engine._h)
        return out[:got.value]

    def write_binary(self, path):
        """tree.writeBinary(path) of a MAXLIKELIHOOD tree."""
        _check(self._L.sbm_occ_tree_write_binary(self._t, os.fsencode(path)), self._engine._h)

    def ot_body(self):
        """The body of the .ot stream (a LOGODDS tree) as a torch CUDA uint8 tensor: five bytes per node of the pruned tree."""
        torch = _torch()
        n = 5 * self.info()["nodes"]
        out = torch.empty((n,), dtype=torch.uint8, device=torch.device("cuda", self._engine._device))
        got = ctypes.c_size_t()
        torch.cuda.current_stream(out.device).synchronize()
        _check(self._L.sbm_occ_ot_body_device(self._t, out.data_ptr() if n else None, n, ctypes.byref(got)), self._engine._h)
        return out[:got.value]

    def ot(self):
        """The whole .ot stream of a LOGODDS tree as bytes: the file write_ot writes, read back."""
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "tree.ot")
            self.write_ot(path)
            with open(path, "rb") as f:
                return f.read()

    def write_ot(self, path):
        """tree.write(path) of a LOGODDS tree."""
        _check(self._L.sbm_occ_ot_write(self._t, os.fsencode(path)), self._engine._h)

    # ---- colours: the tree over a map that has them holds octomap's colour per node after prune(); updateInnerOccupancy() ----
    def leaves_colors(self, max_depth=0):
        """leaves(max_depth) with the colour word of every entry -> (centre keys uint64, depths int32, values float32, colour
        words uint32) as numpy arrays in octomap's iteration order. White for every node of a tree built over a colourless map."""
        n = self._leaf_count(max_depth)
        keys, depth, value, color = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.uint32)
        got = ctypes.c_size_t()
        _check(self._L.sbm_occ_color_leaves(self._t, int(max_depth), keys.ctypes.data if n else None, depth.ctypes.data if n else None,
                                            value.ctypes.data if n else None, color.ctypes.data if n else None, n, ctypes.byref(got)), self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value], color[:got.value]

    def leaves_colors_device(self, max_depth=0):
        """The same as torch CUDA tensors: keys int64, depths int32, values float32, colour words int32."""
        torch = _torch()
        n = self._leaf_count(max_depth)
        dev = torch.device("cuda", self._engine._device)
        keys, depth = torch.empty((n,), dtype=torch.int64, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        value, color = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_color_leaves_device(self._t, int(max_depth), keys.data_ptr() if n else None, depth.data_ptr() if n else None,
                                                   value.data_ptr() if n else None, color.data_ptr() if n else None, n, ctypes.byref(got)),
               self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value], color[:got.value]

    # ---- stamps: the tree over a map that has them is octomap's STAMPED pruned tree (siblings collapse only where the stamps agree) ----
    def leaves_stamps(self, max_depth=0):
        """leaves(max_depth) with the stamp of every entry -> (centre keys uint64, depths int32, values float32, stamps uint32) as
        numpy arrays in octomap's iteration order. 0 for every node of a tree built over a map without stamps."""
        n = self._leaf_count(max_depth)
        keys, depth, value, stamp = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.uint32)
        got = ctypes.c_size_t()
        _check(self._L.sbm_occ_stamp_leaves(self._t, int(max_depth), keys.ctypes.data if n else None, depth.ctypes.data if n else None,
                                            value.ctypes.data if n else None, stamp.ctypes.data if n else None, n, ctypes.byref(got)), self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value], stamp[:got.value]

    def leaves_stamps_device(self, max_depth=0):
        """The same as torch CUDA tensors: keys int64, depths int32, values float32, stamps int32."""
        torch = _torch()
        n = self._leaf_count(max_depth)
        dev = torch.device("cuda", self._engine._device)
        keys, depth = torch.empty((n,), dtype=torch.int64, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        value, stamp = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        got = ctypes.c_size_t()
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.sbm_occ_stamp_leaves_device(self._t, int(max_depth), keys.data_ptr() if n else None, depth.data_ptr() if n else None,
                                                   value.data_ptr() if n else None, stamp.data_ptr() if n else None, n, ctypes.byref(got)),
               self._engine._h)
        return keys[:got.value], depth[:got.value], value[:got.value], stamp[:got.value]

    def last_update_time(self):
        """octomap's getLastUpdateTime(): the root's stamp (the map's clock at build time unless the root itself collapsed)."""
        c = ctypes.c_uint32()
        _check(self._L.sbm_occ_stamp_root(self._t, ctypes.byref(c)), self._engine._h)
        return c.value

    def write_stamped_ot(self, path):
        """tree.write(path) of an OcTreeStamped: `id OcTreeStamped`, a LOGODDS tree built over a map with stamps."""
        _check(self._L.sbm_occ_stamp_ot_write(self._t, os.fsencode(path)), self._engine._h)

    def stamped_ot(self):
        """The whole OcTreeStamped stream as bytes: the file write_stamped_ot writes, read back."""
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "tree.ot")
            self.write_stamped_ot(path)
            with open(path, "rb") as f:
                return f.read()

    def color_ot_body(self):
        """The body of the ColorOcTree stream (a LOGODDS tree) as a torch CUDA uint8 tensor: eight bytes per node of the pruned tree."""
        torch = _torch()
        n = 8 * self.info()["nodes"]
        out = torch.empty((n,), dtype=torch.uint8, device=torch.device("cuda", self._engine._device))
        got = ctypes.c_size_t()
        torch.cuda.current_stream(out.device).synchronize()
        _check(self._L.sbm_occ_color_ot_body_device(self._t, out.data_ptr() if n else None, n, ctypes.byref(got)), self._engine._h)
        return out[:got.value]

    def color_ot(self):
        """The whole ColorOcTree stream of a LOGODDS tree as bytes: the file write_color_ot writes, read back."""
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "tree.ot")
            self.write_color_ot(path)
            with open(path, "rb") as f:
                return f.read()

    def write_color_ot(self, path):
        """tree.write(path) of a ColorOcTree: `id ColorOcTree`, a LOGODDS tree."""
        _check(self._L.sbm_occ_color_ot_write(self._t, os.fsencode(path)), self._engine._h)

    def profile(self):
        return self._engine._profile(("occ_tree_build", "occ_tree_query"))
