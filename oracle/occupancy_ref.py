"""The sequential CPU restatement of the reference's buildOccupancyGridMap (include/sbm.h, "occupancy map"):
oracle/liboccupancy_ref.so (from oracle/occupancy_ref.c) through ctypes. TEST INFRASTRUCTURE ONLY.

    params(resolution, range_max, tree_depth)      the reference's constants by default
    model(...) / pose_rows(poses)                   sbm_stereo_model; poses as float32 (n, 12)
    reproject(disp, scale, model, apply_local)      float32 (h, w, 3), NaN where skipped (= sbm_oracle.reproject)
    world(disp, scale, model, pose)                 float32 (h, w, 3): the point after both transforms
    point(pt, origin, p)                            -> (norm, gate, key_ok, key (3,) uint16) of one world point
    pixel_keys(disp, scale, model, poses, p)        uint64 (n, h, w): packed key per pixel, EMPTY where dropped
    insert(disp, scale, model, poses, p)            -> (sorted distinct keys uint64, hit counts uint32)
    write_binary(keys, resolution)                  -> (bytes of the .bt stream, node count, leaf count)
    pack(k) / unpack(keys)                          (m, 3) uint16 <-> packed uint64
"""
import ctypes

import numpy as np

import oracle_lib
from sbm_oracle import StereoModel

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GATE, KEY = 1, 2
_LIB = None


class Params(ctypes.Structure):
    _fields_ = [("resolution", ctypes.c_double), ("range_max", ctypes.c_float), ("tree_depth", ctypes.c_int32)]


def params(resolution=0.1, range_max=5.0, tree_depth=16):
    return Params(float(resolution), float(range_max), int(tree_depth))


def model(fx=400.0, fy=400.0, cx=320.0, cy=240.0, baseline=0.12, cx_r=None, local=None):
    m = StereoModel()
    m.fx_l, m.fy_l, m.cx_l, m.cy_l, m.Tx_l = fx, fy, cx, cy, 0.0
    m.fx_r, m.fy_r, m.cx_r, m.Tx_r = fx, fy, cx if cx_r is None else cx_r, -fx * baseline
    if local is not None:
        m.local[:] = [float(v) for v in np.asarray(local).reshape(-1)]
        m.has_local = 1
    return m


def model_from_array(a):
    """The 22 doubles a fixture stores: the nine intrinsics, the local transform, has_local."""
    a = np.asarray(a, np.float64)
    m = StereoModel()
    for k, v in zip(("fx_l", "fy_l", "cx_l", "cy_l", "Tx_l", "fx_r", "fy_r", "cx_r", "Tx_r"), a[:9]):
        setattr(m, k, float(v))
    m.local[:] = [float(np.float32(v)) for v in a[9:21]]
    m.has_local = int(a[21])
    return m


def model_to_array(m):
    return np.array([m.fx_l, m.fy_l, m.cx_l, m.cy_l, m.Tx_l, m.fx_r, m.fy_r, m.cx_r, m.Tx_r] + list(m.local) + [m.has_local],
                    np.float64)


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("liboccupancy_ref.so")
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        mp, pp = ctypes.POINTER(StereoModel), ctypes.POINTER(Params)
        L.occ_ref_reproject.argtypes = [vp, ci, ci, ci, mp, ci, vp]
        L.occ_ref_reproject.restype = None
        L.occ_ref_world.argtypes = [vp, ci, ci, ci, mp, vp, vp]
        L.occ_ref_world.restype = None
        L.occ_ref_point.argtypes = [vp, vp, pp, ctypes.POINTER(ctypes.c_double), vp]
        L.occ_ref_keys.argtypes = [ci, vp, ci, ci, ci, mp, vp, pp, vp]
        L.occ_ref_keys.restype = None
        L.occ_ref_write_binary.argtypes = [vp, sz, ctypes.c_double, vp, sz, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
        L.occ_ref_write_binary.restype = sz
        _LIB = L
    return _LIB


def pose_rows(poses):
    p = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
    return p


def _planes(disp):
    d = np.ascontiguousarray(disp, dtype=np.int16)
    return d[None] if d.ndim == 2 else d


def reproject(disp, scale, m, apply_local=True):
    d = np.ascontiguousarray(disp, dtype=np.int16)
    h, w = d.shape
    xyz = np.empty((h, w, 3), np.float32)
    lib().occ_ref_reproject(d.ctypes.data, w, h, scale, ctypes.byref(m), 1 if apply_local else 0, xyz.ctypes.data)
    return xyz


def world(disp, scale, m, pose):
    d = np.ascontiguousarray(disp, dtype=np.int16)
    h, w = d.shape
    pose = pose_rows(pose)
    assert pose.shape[0] == 1
    xyz = np.empty((h, w, 3), np.float32)
    lib().occ_ref_world(d.ctypes.data, w, h, scale, ctypes.byref(m), pose.ctypes.data, xyz.ctypes.data)
    return xyz


def point(pt, origin, p=None):
    p = p or params()
    pt = np.ascontiguousarray(pt, np.float32)
    origin = np.ascontiguousarray(origin, np.float32)
    norm = ctypes.c_double()
    key = np.zeros(3, np.uint16)
    bits = lib().occ_ref_point(pt.ctypes.data, origin.ctypes.data, ctypes.byref(p), ctypes.byref(norm), key.ctypes.data)
    return norm.value, bool(bits & GATE), bool(bits & KEY), key


def pixel_keys(disp, scale, m, poses, p=None):
    p = p or params()
    d = _planes(disp)
    n, h, w = d.shape
    poses = pose_rows(poses)
    assert poses.shape[0] == n, "one pose per plane"
    keys = np.empty((n, h, w), np.uint64)
    lib().occ_ref_keys(n, d.ctypes.data, w, h, scale, ctypes.byref(m), poses.ctypes.data, ctypes.byref(p), keys.ctypes.data)
    return keys


def distinct(pixel):
    """Sorted distinct keys and their hit counts of per-pixel keys."""
    k = np.asarray(pixel, np.uint64).reshape(-1)
    keys, hits = np.unique(k[k != EMPTY], return_counts=True)
    return keys.astype(np.uint64), hits.astype(np.uint32)


def insert(disp, scale, m, poses, p=None):
    return distinct(pixel_keys(disp, scale, m, poses, p))


def write_binary(keys, resolution=0.1):
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    nodes, leafs = ctypes.c_uint(), ctypes.c_uint()
    cap = 256 + 2 * (16 * len(keys) + 1)     # every key adds at most 16 inner nodes of 2 bytes
    out = np.empty(cap, np.uint8)
    n = lib().occ_ref_write_binary(keys.ctypes.data, len(keys), float(resolution), out.ctypes.data, cap, ctypes.byref(nodes),
                                   ctypes.byref(leafs))
    assert n <= cap
    return out[:n].tobytes(), nodes.value, leafs.value


def pack(k):
    k = np.asarray(k, np.uint64).reshape(-1, 3)
    return (k[:, 0] << np.uint64(32)) | (k[:, 1] << np.uint64(16)) | k[:, 2]


def unpack(keys):
    keys = np.asarray(keys, np.uint64).reshape(-1)
    m = np.uint64(0xFFFF)
    return np.stack([(keys >> np.uint64(32)) & m, (keys >> np.uint64(16)) & m, keys & m], axis=1).astype(np.uint16)
