"""sbm_debug_postfilter without a GPU: its argument checks come before any device work, in a fixed order (pointers, batch, size,
info_count, stages, and the handle last, so that everything else can be told apart without a device), and the Python mirror binds
it and names every info word."""
import ctypes

import numpy as np
import pytest

NULL, SIZE, UNSUPPORTED, BATCH = -1, -2, -23, -24
INFO = 18


@pytest.fixture(scope="module")
def call(pkg):
    L = pkg.load_library()
    pre = np.full((1, 6, 64), -16, np.int16)
    cost = np.zeros((1, 6, 64), np.int32)
    out = np.empty_like(pre)
    info = np.zeros(INFO, np.int32)
    good = dict(h=None, n=1, w=64, hh=6, pre=pre.ctypes.data, cost=cost.ctypes.data, stages=3, out=out.ctypes.data, info=info.ctypes.data,
                count=INFO)

    def run(**change):
        a = dict(good, **change)
        return L.sbm_debug_postfilter(a["h"], a["n"], a["w"], a["hh"], a["pre"], a["cost"], a["stages"], a["out"], a["info"], a["count"])

    run.keep = (pre, cost, out, info)
    return run


def test_it_is_exported_but_not_in_the_public_header(pkg):
    import pathlib

    assert hasattr(pkg.load_library(), "sbm_debug_postfilter")
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "sbm.h").read_text()
    assert "sbm_debug_postfilter" not in header and "sbm_debug_plan" not in header


@pytest.mark.parametrize("change,code", [
    ({}, NULL),                                     # everything but the handle is in order: the handle is looked at last
    ({"pre": None}, NULL), ({"out": None}, NULL), ({"info": None}, NULL),
    ({"cost": None}, NULL),                         # (a null cost plane is only judged with the handle's parameters)
    ({"n": 0}, BATCH), ({"n": -3}, BATCH),
    ({"w": 0}, SIZE), ({"hh": 0}, SIZE), ({"w": -64}, SIZE),
    ({"count": INFO - 1}, SIZE), ({"count": 0}, SIZE), ({"count": INFO + 5}, NULL),
    ({"stages": 0}, UNSUPPORTED), ({"stages": 4}, UNSUPPORTED), ({"stages": -1}, UNSUPPORTED),
    ({"n": 0, "w": 0, "stages": 0}, BATCH), ({"w": 0, "count": 0, "stages": 9}, SIZE), ({"count": 1, "stages": 9}, SIZE),
    ({"pre": None, "n": 0}, NULL),
])
def test_argument_checks(call, change, code):
    assert call(**change) == code
    assert not call.keep[3].any()   # and nothing was reported


def test_the_mirror_names_every_info_word(pkg):
    assert len(pkg.StereoBM.POSTFILTER_INFO) == INFO == len(set(pkg.StereoBM.POSTFILTER_INFO))
    assert (pkg.StereoBM.LR_COPY, pkg.StereoBM.LR_FAST16, pkg.StereoBM.LR_GENERIC_LDS, pkg.StereoBM.LR_GENERIC_GLOBAL) == (0, 1, 2, 3)
    assert pkg.load_library().sbm_debug_postfilter.argtypes[-1] is ctypes.c_size_t
