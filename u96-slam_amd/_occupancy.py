"""The occupancy voxel map of the reference's buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561): a device-side set of
octomap keys fed straight from disparity planes, and the octomap binary stream (.bt) written from its distinct keys."""
import ctypes
import os

import numpy as np

from ._abi import ERR_OCC_FULL, OccParams, StereoBMError, _check, _torch, load_library


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


def _poses(poses, n):
    p = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    if p.shape[0] != n:
        raise StereoBMError(-2, f"{p.shape[0]} poses for {n} planes")
    return p


class OccupancyMap:
    """A map for up to `capacity` voxels on the device of `engine` (a StereoBM or StereoSGBM), which must outlive it: the map
    uses the engine's handle, stream and scratch. Not thread-safe."""

    def __init__(self, engine, capacity, params=None, **kw):
        if params is not None and kw:
            raise TypeError("pass either an OccParams or keyword parameters")
        self._p = params if params is not None else occ_params(**kw)
        self._engine = engine
        self._L = engine._L
        self._m = ctypes.c_void_p()
        _check(self._L.sbm_occ_create(engine._h, ctypes.byref(self._p), int(capacity), ctypes.byref(self._m)), engine._h)

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

    def profile(self):
        return self._engine._profile(("occ_insert", "occ_fetch"))
