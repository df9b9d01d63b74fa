"""The base of StereoBM and StereoSGBM: one `sbm_handle` (stream + scratch), the buffers its asynchronous calls still use,
and the one path every device entry point of the C-ABI is called through."""
import collections
import ctypes

import numpy as np

from ._abi import StereoBMError, _check, _torch


def _jobs_array(jobs):
    j = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 2))
    if j.shape[0] == 0:
        raise StereoBMError(-24, "no jobs")
    return j


def _count_values(count, n, message, dense=True):
    """`count` as a flat int32 CUDA tensor of n values; dense=False accepts a strided one and copies it."""
    c1 = count.reshape(-1)
    if c1.dtype != _torch().int32 or c1.numel() != n or not c1.is_cuda or (dense and not c1.is_contiguous()):
        raise StereoBMError(-2, message)
    return c1.contiguous()


class Engine:
    """Owner of one device handle. Not thread-safe."""

    def _open(self, L, bm_params, device):
        self._L = L
        self._h = ctypes.c_void_p()
        self._device = device
        self._inflight = []                         # buffers of asynchronous device calls, until the stream is drained
        self._host_inflight = collections.deque()   # (left, right, disparity) of StereoBM.submit_host, oldest first
        _check(L.sbm_create(ctypes.byref(self._h), ctypes.byref(bm_params), device))

    def close(self):
        """Release the engine. Whatever is in flight is drained first (sbm_synchronize) while its buffers are still referenced
        here, so every submitted `disparity` array is filled -- sbm_destroy on its own would let the queued copies finish and
        DROP the maps of the newest submission (include/sbm.h, "sbm_destroy() and the asynchronous feed")."""
        h = getattr(self, "_h", None)
        if h:
            if self._inflight or self._host_inflight:
                self._L.sbm_synchronize(h)
                self._inflight.clear()
                self._host_inflight.clear()
            self._L.sbm_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def synchronize(self):
        _check(self._L.sbm_synchronize(self._h), self._h)
        self._inflight.clear()        # buffers of asynchronous calls may be released now
        self._host_inflight.clear()

    def set_profiling(self, on):
        # 0 = off, 1 = sync after every call, 2 = stage events only (no host sync; up to 64 calls per profile() read),
        # 3 = as 2 on every 4th call only
        _check(self._L.sbm_set_profiling(self._h, int(on)), self._h)

    def _profile(self, keys):
        out = {}
        for k in keys:
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    def _device_call(self, fn, args, keep, sync=True):
        """Call the device entry point fn(handle, *args, sync). `keep` names every device buffer the call reads or writes, the
        first of them on the device whose current torch stream produced the inputs."""
        # the engine runs on its own (non-blocking) stream: order it behind whatever produced the inputs
        _torch().cuda.current_stream(keep[0].device).synchronize()
        _check(fn(self._h, *args, 1 if sync else 0), self._h)
        if sync:
            # the entry point has drained the engine's compute stream: earlier asynchronous DEVICE calls are done too
            # (host submissions keep their arrays: their maps may still be on the way home on the copy stream)
            self._inflight.clear()
        else:
            # torch's caching allocator only knows its own streams: without this the .contiguous() temporaries and a
            # freshly allocated output could be handed out again while the engine's kernels still use them
            # (a list: back-to-back asynchronous calls each keep their buffers until the next synchronize())
            self._inflight.append(keep)

    @staticmethod
    def _as3d(t):
        """(H,W) or (n,H,W) tensor -> (contiguous (n,H,W) tensor, n, h, w)."""
        t3 = (t if t.dim() == 3 else t[None]).contiguous()
        return (t3,) + tuple(t3.shape)

    def _check_device_images(self, *tensors):
        """Every image handed to the engine as a raw pointer: CUDA uint8, on the handle's device, (H,W) or (n,H,W)."""
        torch = _torch()
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
                raise StereoBMError(-2, "images must be CUDA uint8 tensors")
            if t.device.index != self._device:
                raise StereoBMError(-20, f"tensor on cuda:{t.device.index}, engine on device {self._device}")
            if t.dim() not in (2, 3):
                raise StereoBMError(-2, "expected (H,W) or (n,H,W) images")

    def _compute_device(self, fn, lead, left, right, disparity, sync):
        """The dense device call of both matchers, fn(handle, *lead, n, left, right, w, h, disparity, sync), on torch CUDA uint8
        tensors (n,H,W) or (H,W). Returns the torch int16 disparity tensor, of the images' shape."""
        torch = _torch()
        if left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        if left.dtype != torch.uint8 or right.dtype != torch.uint8 or not left.is_cuda or not right.is_cuda:
            raise StereoBMError(-2, "Both input images must be CUDA uint8 tensors")
        if left.device.index != self._device or right.device.index != self._device:
            raise StereoBMError(-20, f"tensor on cuda:{left.device.index}, engine on device {self._device}")
        if left.dim() not in (2, 3):
            raise StereoBMError(-2, "expected (H,W) or (n,H,W) images")
        shape = left.shape
        left, n, h, w = self._as3d(left)
        right = right.contiguous()
        if disparity is None:
            disparity = torch.empty(shape, dtype=torch.int16, device=left.device)
        elif (not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.int16 or disparity.device != left.device
              or tuple(disparity.shape) != tuple(shape) or not disparity.is_contiguous()):
            # the C-ABI writes n*h*w int16 through the raw pointer: anything else would be an out-of-bounds / strided-wrong write
            raise StereoBMError(-2, f"disparity must be a contiguous CUDA int16 tensor of shape {tuple(shape)} on {left.device}")
        self._device_call(fn, lead + (n, left.data_ptr(), right.data_ptr(), w, h, disparity.data_ptr()),
                          (left, right, disparity), sync)
        return disparity
