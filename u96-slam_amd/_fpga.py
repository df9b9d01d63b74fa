"""The reference's own matcher, FPGA flavour (src/dvp/rtl/bm*.v; FPGA.cpp:270-279 consumers), and the PL's GFTT
min-eigenvalue map (FPGA.cpp:283-291)."""
import ctypes

import numpy as np

from ._abi import FpgaParams, FpgaPlan, StereoBMError, _check, _torch, load_library


def fpga_params(width, height, block_size=21, num_disparities=64, uni_enable=0, uni_mode=0, uni_threshold=0):
    return FpgaParams(width, height, block_size, num_disparities, uni_enable, uni_mode, uni_threshold)


def fpga_params_from_regs(image_size, bm_setting, uni_filt_ctrl=0):
    """ImageSize [1708h], BmSetting [170Ch], UniFiltCtrl [1728h] -> FpgaParams (firmware: fpga.c:155,158)."""
    q = FpgaParams()
    _check(load_library().sbm_fpga_params_from_regs(image_size, bm_setting, uni_filt_ctrl, ctypes.byref(q)))
    return q


def fpga_sad_size_reg(params):
    """Read-back value of SAD_Size [1724h] (bm.v:208)."""
    return int(load_library().sbm_fpga_sad_size_reg(ctypes.byref(params)))


def fpga_validate(params):
    return int(load_library().sbm_fpga_params_validate(ctypes.byref(params)))


def fpga_plan(params, n=1):
    """The launch plan of fpga_bm for these parameters and n pairs (FpgaPlan; sbm_fpga_debug_plan: no handle, no device)."""
    pl = FpgaPlan()
    _check(load_library().sbm_fpga_debug_plan(ctypes.byref(params), n, ctypes.byref(pl), ctypes.sizeof(pl)))
    return pl


class FpgaMatcher:
    def _fpga(self, fn, a, b, params, sync=True):
        torch = _torch()
        self._check_device_images(a, b)
        if a.shape != b.shape:
            raise StereoBMError(-2, "both inputs must be CUDA uint8 tensors of the same shape")
        a3, n, h, w = self._as3d(a)
        b = b.contiguous()
        if (w, h) != (params.width, params.height):
            raise StereoBMError(-2, f"images are {w}x{h}, ImageSize says {params.width}x{params.height}")
        out = torch.empty(a.shape, dtype=torch.int16, device=a.device)
        self._device_call(fn, (n, a3.data_ptr(), b.data_ptr(), ctypes.byref(params), out.data_ptr()), (a3, b, out), sync)
        return out

    def fpga_bm(self, xsbl_l, xsbl_r, params, sync=True):
        """RTL block matcher on x-Sobel planes (torch CUDA uint8, (n,H,W) or (H,W)) -> int16 s11.4, -1 = none.
        sync=False leaves the call running on the engine's stream (call synchronize() before reading the result)."""
        return self._fpga(self._L.sbm_fpga_bm_device, xsbl_l, xsbl_r, params, sync)

    def fpga_compute(self, left, right, params, sync=True):
        """xsbl2.v prefilter + RTL block matcher on rectified frames: the PL pipeline behind Fpga::receiveDepthMap."""
        return self._fpga(self._L.sbm_fpga_compute_device, left, right, params, sync)

    def fpga_compute_host(self, left, right, params):
        """numpy uint8 (H,W) rectified pair -> numpy int16 (H,W): the frame Fpga::receiveDepthMap would hand out."""
        if left.shape != right.shape or left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2:
            raise StereoBMError(-2, "both inputs must be (H,W) uint8 arrays of the same shape")
        if left.strides[1] != 1 or right.strides[1] != 1 or left.strides[0] < left.shape[1] or right.strides[0] < right.shape[1]:
            raise StereoBMError(-2, "rows must be dense with a positive row stride")
        out = np.empty(left.shape, np.int16)
        _check(self._L.sbm_fpga_compute(self._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0],
                                        ctypes.byref(params), out.ctypes.data, out.strides[0]), self._h)
        return out

    def gftt_eig_host(self, img):
        """numpy uint8 (H,W) -> (numpy uint16 map, Max register value), as FPGA.cpp:283-291 assembles them."""
        if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            raise StereoBMError(-2, "image must be an (H,W) uint8 array with dense rows")
        out = np.empty(img.shape, np.uint16)
        mx = ctypes.c_uint32()
        _check(self._L.sbm_gftt_eig(self._h, img.ctypes.data, img.strides[0], img.shape[1], img.shape[0], out.ctypes.data,
                                    out.strides[0], ctypes.byref(mx)), self._h)
        return out, int(mx.value)

    def gftt_eig(self, img):
        """PL GFTT min-eigenvalue map of torch CUDA uint8 frames (n,H,W) or (H,W): (int16-viewed uint16 map as torch.int32,
        per-image maximum) -- the inputs of generateKeypoints2 (src/slam/src/core/GFTT.cpp:41)."""
        torch = _torch()
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        eig = torch.empty(img.shape, dtype=torch.int16, device=img.device)     # uint16 payload (torch has no uint16 math)
        mx = torch.empty((n,), dtype=torch.int32, device=img.device)
        self._device_call(self._L.sbm_gftt_eig_device, (n, i3.data_ptr(), w, h, eig.data_ptr(), mx.data_ptr()), (i3, eig, mx))
        return eig.to(torch.int32) & 0xffff, mx
