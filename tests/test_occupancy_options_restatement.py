"""tests/occupancy_option_cases.py, the transcription of include/sbm.h's "occupancy map: insert options", against what the
reference's own octomap answered (tests/golden/occupancy_options.npz, tools/make_occupancy_option_fixtures.py): after every scan
of every case the leaf keys, the bits of the float log-odds, the changed keys and their flags. No GPU, no library."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_option_cases as oc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402

GOLDEN = oc.GOLDEN
FX, NAMES, case_of, recorded = oc.FX, oc.NAMES, oc.case_of, oc.recorded


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "keys", len(got[0]), len(want[0]))
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), (what, "log-odds")
    assert np.array_equal(got[2], want[2]), (what, "changed keys", len(got[2]), len(want[2]))
    assert np.array_equal(np.asarray(got[3], np.uint8), np.asarray(want[3], np.uint8)), (what, "created flags")


def test_the_fixture_is_the_committed_one():
    want = GOLDEN.with_suffix(".sha256").read_text().split()[0]
    assert hashlib.sha256(GOLDEN.read_bytes()).hexdigest() == want


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_octomap_after_every_scan(name):
    c = case_of(name)
    assert [float(v) for v in FX[f"{name}_constants"]] == [float(v) for v in rc.constants(c["params"])]
    got, want = oc.run_case(c, float(FX["resolution"])), recorded(name)
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        same(g, w, (name, s))


def test_the_cases_cover_what_the_header_states():
    assert {"box_inside", "box_exit", "origin_outside", "box_face", "box_range", "box_empty", "box_nokey_origin", "created", "toggle",
            "created_then_flipped", "clamp_noop", "enable_late", "disabled", "reset_between", "same_voxel", "wrap", "disc_range",
            "disc_duplicates_order", "scene_all"} <= set(NAMES)
    t = recorded("toggle")
    x = set(map(int, t[0][2])) & set(map(int, t[3][2]))            # created by the first hit; flipped by the third miss
    assert len(x) == 1 and not x & set(map(int, t[4][2])) and not x & set(map(int, t[2][2]))
    assert len(recorded("origin_outside")[0][0]) == 1 and len(recorded("box_empty")[0][0]) == 0
    assert oc.wrapped_key(3300.0, 10.0) == 232 and float(oc.key_coord(232, 0.1)) == float(np.float32(-3253.55))
    a, b = recorded("disc_duplicates_order")[0], recorded("disc_duplicates_order_perm")[0]
    same(a, b, "permuted")


def test_a_box_point_without_a_key_leaves_the_box_as_it_was():
    b = oc.Box()
    assert b.set((-1, -1, -1), (1, 1, 1)) and not b.set((0, 0, 0), (4000, 0, 0)) and not b.set((np.nan, 0, 0), (1, 1, 1))
    assert list(b.max) == [1, 1, 1] and b.min_key == (32758, 32758, 32758)
    assert b.set((1, 0, 0), (-1, 1, 1)) and not b.has_point((0, 0.5, 0.5)) and not b.has_key((32768, 32770, 32770))
