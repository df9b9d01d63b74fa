"""The visual-word dictionary's stage names through sbm_get_profile: zero on a fresh handle, positive after one profiled call, the
total the float sum of its parts. The names are written out from include/sbm.h, not read from the library."""
import ctypes

import numpy as np
import pytest

import vwd_cases as vc
from gpu_support import dev

pytestmark = pytest.mark.gpu
NAMES = ("vwd_search", "vwd_append", "vwd_total")


def read(bm, name):
    v = ctypes.c_float(-1.0)
    return bm._L.sbm_get_profile(bm._h, name.encode(), ctypes.byref(v)), v.value


def test_names_answer_zero_then_fill(pkg):
    bm = pkg.StereoBM.create(16, 9)
    try:
        for name in NAMES:
            assert read(bm, name) == (0, 0.0), name
        assert read(bm, "vwd_searchx")[0] == -23 and read(bm, "vwd")[0] == -23
        words, q = vc.make_case(3, 65, 129, vc.L1)
        d = pkg.VWDictionary(bm, 1024)
        try:
            d.add_words(words, 1)
            for name in NAMES:
                assert read(bm, name) == (0, 0.0), name        # not profiled: nothing recorded
            bm.set_profiling(1)
            d.add_words(dev(q), 2)
            t = {name: read(bm, name) for name in NAMES}
            print(t)
            assert all(st == 0 and ms > 0.0 for st, ms in t.values()), t
            assert np.float32(np.float32(t["vwd_search"][1]) + np.float32(t["vwd_append"][1])) == np.float32(t["vwd_total"][1])
            assert d.profile().keys() == set(NAMES)
            assert read(bm, "total") == (0, 0.0) and read(bm, "occ_insert") == (0, 0.0)   # no other family's
            bm.set_profiling(0)
            bm.set_profiling(1)
            for name in NAMES:
                assert read(bm, name) == (0, 0.0), name
        finally:
            d.close()
    finally:
        bm.close()
