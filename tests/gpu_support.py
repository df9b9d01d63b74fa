"""What the test modules share: the call-site build (CPU and GPU modules alike), and for the GPU modules the torch_cuda and bm
fixtures (imported by name into the modules that use them) and the upload helper. TEST INFRASTRUCTURE ONLY."""
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def build_callsite(tmp_path, source, extra=(), *, flags=(), exe="cs", pkg=None, libs=()):
    """g++ over tests/cpp/<source> (or over source as it is where it is an absolute path, such as a file a test wrote into
    tmp_path) and the engine library -> (tmp_path / exe, the completed process). flags go in front of -I include, extra behind it. With pkg the library is linked by its path (pkg.library_path()), libs follow it, and ROCm's
    directory joins the rpath; without, it is linked as -L u96-slam_amd/lib -lsbm_hip."""
    exe = tmp_path / exe
    cmd = ["g++", "-std=c++17", "-O1", *flags, "-I", str(ROOT / "include"), *extra, str(ROOT / "tests" / "cpp" / source)]
    if pkg is not None:
        lib = pkg.library_path()
        cmd += ["-o", str(exe), str(lib), *libs, f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"]
    else:
        lib = ROOT / "u96-slam_amd" / "lib"
        cmd += ["-L", str(lib), "-lsbm_hip", f"-Wl,-rpath,{lib}", "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def bm(pkg):
    return pkg.StereoBM.create(64, 21)


def dev(a):
    """The array on cuda:0, same bytes and shape; uint16 (the response maps of gftt_select, the only caller that passes it)
    goes up viewed as int16, every other dtype as it is."""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to("cuda:0")
