"""Producers in front of the dense path (fpga.c:303-366, rect_intp.v:285-404, xsbl2.v:661-874) and consumers of its map
(SensorData.cpp:50-58, Stereo.cpp:53-117,157-199, main.cpp:522-553), all on torch CUDA tensors."""
import ctypes

from ._abi import PREFILTER_FLAVOUR_CV, RectCam, StereoBMError, _torch


def make_rect_cam(f, c, f2inv, c2_f2, rot):
    cam = RectCam()
    cam.f[:] = [int(v) for v in f]
    cam.c[:] = [int(v) for v in c]
    cam.f2inv[:] = [int(v) for v in f2inv]
    cam.c2_f2[:] = [int(v) for v in c2_f2]
    for r in range(3):
        for k in range(3):
            cam.rot[r][k] = int(rot[r][k])
    return cam


class FrontEnd:
    def rect_map(self, cam, width, height):
        """Inverse rectification map of one camera: torch CUDA int16 (H, W, 2), (x, y) in 1/32 source pixels."""
        torch = _torch()
        m = torch.empty((height, width, 2), dtype=torch.int16, device=f"cuda:{self._device}")
        self._device_call(self._L.sbm_rect_map_device, (ctypes.byref(cam), width, height, m.data_ptr()), (m,))
        return m

    def rect_remap(self, src, rmap):
        """torch CUDA uint8 (n,H,W) or (H,W) raw frames + a map from rect_map -> rectified frames, on the device."""
        torch = _torch()
        s3, n, h, w = self._as3d(src)
        rmap = rmap.contiguous()
        if tuple(rmap.shape) != (h, w, 2) or rmap.dtype != torch.int16 or src.dtype != torch.uint8:
            raise StereoBMError(-2, "map must be int16 (H,W,2) and frames uint8 (..,H,W)")
        out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
        self._device_call(self._L.sbm_rect_remap_device, (n, s3.data_ptr(), rmap.data_ptr(), w, h, out.data_ptr()), (s3, rmap, out))
        return out

    def prefilter(self, src, flavour=PREFILTER_FLAVOUR_CV, cap=None):
        """Stand-alone x-Sobel prefilter of torch CUDA uint8 (n,H,W) or (H,W) frames, cv or RTL flavour."""
        self._check_device_images(src)
        s3, n, h, w = self._as3d(src)
        out = _torch().empty(src.shape, dtype=src.dtype, device=src.device)
        self._device_call(self._L.sbm_prefilter_device,
                          (n, s3.data_ptr(), w, h, flavour, self._p.prefilter_cap if cap is None else cap, out.data_ptr()), (s3, out))
        return out

    def to_float(self, disp):
        """CV_32F form of a torch CUDA int16 disparity tensor: disp / 16 as float32 (cv convertTo(CV_32F, 1/16))."""
        torch = _torch()
        d3, n, h, w = self._as3d(disp)
        out = torch.empty(disp.shape, dtype=torch.float32, device=disp.device)
        self._device_call(self._L.sbm_disparity_to_float_device, (n, d3.data_ptr(), w, h, out.data_ptr()), (d3, out))
        return out

    def decimate(self, disp, scale=4):
        """torch CUDA int16 (n,H,W) or (H,W) -> every scale-th pixel, on the device."""
        torch = _torch()
        d3, n, h, w = self._as3d(disp)
        out = torch.empty((n, h // scale, w // scale), dtype=torch.int16, device=d3.device)
        self._device_call(self._L.sbm_decimate_device, (n, d3.data_ptr(), w, h, scale, out.data_ptr()), (d3, out))
        return out if disp.dim() == 3 else out[0]

    def reproject(self, disp, model, scale=1, apply_local=True):
        """torch CUDA int16 map(s) -> float32 (..., H, W, 3) points, NaN where invalid."""
        torch = _torch()
        d3, n, h, w = self._as3d(disp)
        xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=d3.device)
        self._device_call(self._L.sbm_reproject_device,
                          (n, d3.data_ptr(), w, h, scale, ctypes.byref(model), 1 if apply_local else 0, xyz.data_ptr()), (d3, xyz))
        return xyz if disp.dim() == 3 else xyz[0]

    def keypoints3d(self, disp, kpts, model, min_depth=0.0, max_depth=0.0):
        """One full-resolution torch CUDA int16 map + float32 (nk,2) keypoints (x,y) -> float32 (nk,3)."""
        torch = _torch()
        disp, kpts = disp.contiguous(), kpts.contiguous()
        h, w = disp.shape
        xyz = torch.empty((kpts.shape[0], 3), dtype=torch.float32, device=disp.device)
        self._device_call(self._L.sbm_keypoints3d_device, (disp.data_ptr(), w, h, kpts.data_ptr(), kpts.shape[0], ctypes.byref(model),
                                                           min_depth, max_depth, xyz.data_ptr()), (disp, kpts, xyz))
        return xyz
