"""The visual-word dictionary of the reference's loop-closure thread: VWDictionary::addNewWords (src/slam/src/core/
VWDictionary.cpp:40-115) with an exhaustive 2-NN search on the device, computeLikelihood and the choice of the highest hypothesis
(Mapper.cpp:536-677), and SensorData::limitKeypoints (SensorData.cpp:109-133)."""
import ctypes

import numpy as np

from ._abi import (ERR_VWD_FULL, VWD_L1, VWD_L2, VWD_NONE, StereoBMError, VwdParams, _check, _torch,  # noqa: F401
                   load_library)


def vwd_params(metric=VWD_L1, nndr=0.8, slices=0):
    """The reference's values by default: the L1 metric its index answers with, nndrRatio 0.8f; slices 0 = automatic."""
    return VwdParams(int(metric), float(nndr), int(slices))


def vwd_validate(params):
    """Status code of sbm_vwd_params_validate (0 = ok)."""
    return load_library().sbm_vwd_params_validate(ctypes.byref(params))


def limit_keypoints(responses, max_keypoints):
    """limitKeypoints' inliers as a bool array: the max_keypoints highest |response|, the higher index first among equal ones;
    everything when max_keypoints <= 0 or there are no more than that. Host code: needs no GPU."""
    r = np.ascontiguousarray(np.asarray(responses, np.float32).reshape(-1))
    keep = np.zeros(len(r), np.uint8)
    _check(load_library().sbm_vwd_limit_keypoints(r.ctypes.data if len(r) else None, len(r), int(max_keypoints),
                                                  keep.ctypes.data if len(r) else None))
    return keep.astype(bool)


class VWDictionary:
    """A dictionary for up to `capacity` words on the device of `engine` (a StereoBM or StereoSGBM), which must outlive it: the
    dictionary uses the engine's handle, stream and scratch. Not thread-safe."""

    def __init__(self, engine, capacity, params=None, **kw):
        if params is not None and kw:
            raise TypeError("pass either a VwdParams or keyword parameters")
        self._p = params if params is not None else vwd_params(**kw)
        self._engine = engine
        self._L = engine._L
        self._v = ctypes.c_void_p()
        _check(self._L.sbm_vwd_create(engine._h, int(capacity), ctypes.byref(self._p), ctypes.byref(self._v)), engine._h)

    def close(self):
        v = getattr(self, "_v", None)
        if v:
            self._L.sbm_vwd_destroy(v)
            self._v = None

    def __del__(self):
        self.close()

    def reset(self):
        """Forget every word, reference and node; the store is kept."""
        _check(self._L.sbm_vwd_reset(self._v), self._engine._h)

    def _device_rows(self, desc):
        torch = _torch()
        if not isinstance(desc, torch.Tensor) or desc.dtype != torch.uint8 or not desc.is_cuda or desc.dim() != 2 or \
                desc.shape[1] != 32 or not desc.is_contiguous() or desc.device.index != self._engine._device:
            raise StereoBMError(-2, "desc must be a contiguous uint8 CUDA tensor (n, 32) on the engine's device")
        torch.cuda.current_stream(desc.device).synchronize()
        return desc

    def add_words(self, desc, node_id, n_keypoints_total=None):
        """addNewWords(desc, node_id): desc a torch CUDA uint8 tensor (n, 32) (a frame's rows of orb_describe's output, used
        where they are) or a numpy uint8 array (n, 32) (the host form). n_keypoints_total: the node's keypoint count including
        the ones cut by limit_keypoints (default n). Returns the word id of every row (numpy int32). Raises
        StereoBMError(ERR_VWD_FULL), with nothing added, when the new words do not fit."""
        if isinstance(desc, np.ndarray):
            d = np.asarray(desc, np.uint8).reshape(-1, 32)
            if d.strides[1] != 1:
                d = np.ascontiguousarray(d)
            n = d.shape[0]
            ids = np.empty(max(n, 1), np.int32)
            _check(self._L.sbm_vwd_add_words(self._v, d.ctypes.data if n else None, d.strides[0] if n else 32, n, int(node_id),
                                             n if n_keypoints_total is None else int(n_keypoints_total), ids.ctypes.data),
                   self._engine._h)
            return ids[:n]
        d = self._device_rows(desc)
        n = d.shape[0]
        ids = np.empty(max(n, 1), np.int32)
        _check(self._L.sbm_vwd_add_words_device(self._v, d.data_ptr() if n else None, n, int(node_id),
                                                n if n_keypoints_total is None else int(n_keypoints_total), ids.ctypes.data),
               self._engine._h)
        return ids[:n]

    def search(self, desc):
        """The 2-NN records of a torch CUDA uint8 tensor (n, 32) against the dictionary as it is: int32 (n, 4) on the device,
        (i0, d0, i1, d1), -1 and VWD_NONE where there is no such neighbour. Nothing is added."""
        torch = _torch()
        d = self._device_rows(desc)
        n = d.shape[0]
        rec = torch.empty((n, 4), dtype=torch.int32, device=d.device)
        _check(self._L.sbm_vwd_search_device(self._v, d.data_ptr() if n else None, n, rec.data_ptr() if n else None, 1),
               self._engine._h)
        return rec

    def size(self):
        v = ctypes.c_size_t()
        _check(self._L.sbm_vwd_size(self._v, ctypes.byref(v)), self._engine._h)
        return v.value

    def overflow(self):
        v = ctypes.c_uint64()
        _check(self._L.sbm_vwd_overflow(self._v, ctypes.byref(v)), self._engine._h)
        return v.value

    def words(self, first=0, count=None):
        """Rows first .. first + count - 1 of the store (default: all) as numpy uint8 (count, 32)."""
        count = self.size() - first if count is None else count
        rows = np.empty((max(count, 1), 32), np.uint8)
        _check(self._L.sbm_vwd_fetch_words(self._v, int(first), int(count), rows.ctypes.data), self._engine._h)
        return rows[:count]

    def references(self, word_id):
        """{node id: count} of one word."""
        k = ctypes.c_int()
        st = self._L.sbm_vwd_references(self._v, int(word_id), None, None, 0, ctypes.byref(k))
        if st != 0 and not (st == -2 and k.value > 0):
            _check(st, self._engine._h)
        nodes, counts = np.empty(max(k.value, 1), np.int32), np.empty(max(k.value, 1), np.int32)
        _check(self._L.sbm_vwd_references(self._v, int(word_id), nodes.ctypes.data, counts.ctypes.data, k.value, ctypes.byref(k)),
               self._engine._h)
        return {int(a): int(b) for a, b in zip(nodes[:k.value], counts[:k.value])}

    def likelihood(self, node_id, candidates, n_nodes):
        """computeLikelihood of node_id against the candidate node ids, n_nodes the total node count. Returns (scores float32,
        one per candidate, best id, best score): the highest hypothesis of detectLoopClosure, (0, 0.0) when no score is positive."""
        c = np.ascontiguousarray(np.asarray(candidates, np.int32).reshape(-1))
        scores = np.zeros(max(len(c), 1), np.float32)
        best, score = ctypes.c_int(), ctypes.c_float()
        _check(self._L.sbm_vwd_likelihood(self._v, int(node_id), c.ctypes.data if len(c) else None, len(c), int(n_nodes),
                                          scores.ctypes.data if len(c) else None, ctypes.byref(best), ctypes.byref(score)),
               self._engine._h)
        return scores[:len(c)], best.value, np.float32(score.value)

    def profile(self):
        return self._engine._profile(("vwd_search", "vwd_append", "vwd_total"))
