"""The buffer-layout helper (u96-slam_amd/csrc/sbm_carve.h: Carve and pad16) compiled alone as host C++ under the address and
undefined-behaviour sanitizers and run as a child process (tests/cpp/carve_main.cpp): nothing of ROCm and nothing of the engine
library is linked. For every alignment a family uses, the counting pass and the placing pass of one layout end at the same
offset, every piece begins on the boundary, neighbours neither overlap nor leave a gap of the alignment or more, an empty piece
takes no room and moves nobody, and the default alignment gives the offsets that sums of pad16 give."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "u96-slam_amd" / "csrc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("carve_host") / "carve_main"
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                        str(ROOT / "tests" / "cpp" / "carve_main.cpp"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("align", [1, 4, 16, 256])
def test_layouts(exe, align):
    r = subprocess.run([str(exe), str(align)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr)
