"""The CPU restatement of generateKeypoints2 (oracle/gftt_select_ref.c) against a literal Python transcription of GFTT.cpp:41-170: crafted
maps, every parameter edge, a seeded fuzz, strided maps and the prefix property of the cap."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import gftt_select_ref as ref  # noqa: E402
from gftt_select_cases import PARAM_EDGES, crafted_maps, literal_generate_keypoints2, random_case  # noqa: E402

MAPS = crafted_maps()


@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("mf,q,md", PARAM_EDGES)
def test_crafted_maps_and_edges(name, mf, q, md):
    m, mx = MAPS[name]
    got = ref.select(m, mx, mf, q, md)
    want = literal_generate_keypoints2(m, mx, mf, q, md)
    assert np.array_equal(got, want), (name, len(got), len(want))


def test_seeded_fuzz():
    rng = np.random.default_rng(20261015)
    for _ in range(120):
        m, mx, mf, q, md = random_case(rng)
        assert np.array_equal(ref.select(m, mx, mf, q, md), literal_generate_keypoints2(m, mx, mf, q, md)), (m.shape, mx, mf, q, md)


def test_reference_parameters_on_the_golden_frame(oracle, golden):
    eig, mx = oracle.gftt_eig(golden["rect_l"])
    got = ref.select(eig, mx)
    assert 0 < len(got) <= 1500
    assert np.array_equal(got, literal_generate_keypoints2(eig, mx))


@pytest.mark.parametrize("md", [0.0, 1.0, 2.5, 7.0, 7.4])
def test_prefix_property(md):
    rng = np.random.default_rng(5)
    m = rng.integers(0, 2000, (60, 70)).astype(np.uint16)
    full = ref.select(m, int(m.max()), -1, 0.05, md)
    assert len(full) > 40
    for cap in (1, 2, 17, 40, len(full), len(full) + 5):
        assert np.array_equal(ref.select(m, int(m.max()), cap, 0.05, md), full[:cap])


def test_strided_map_selects_as_dense():
    rng = np.random.default_rng(8)
    dense = rng.integers(0, 65536, (33, 41)).astype(np.uint16)
    big = np.zeros((33, 64), np.uint16)
    big[:, :41] = dense
    big[:, 41:] = 65535                      # padding past the row end must never be read as a candidate
    view = big[:, :41]
    for md in (0.0, 3.5, 7.0):
        assert np.array_equal(ref.select(view, 65535, -1, 0.01, md), ref.select(dense, 65535, -1, 0.01, md))


def test_threshold_compares_in_double():
    m = np.zeros((5, 5), np.uint16)
    m[1:4, 1:4] = [[99, 100, 101], [100, 100, 100], [98, 97, 102]]
    # max 10000 * 0.01 = 100.0 exactly; 0.01 is not a binary fraction, so the product is what the double multiply gives
    want = literal_generate_keypoints2(m, 10000, -1, 0.01, 0.0)
    assert np.array_equal(ref.select(m, 10000, -1, 0.01, 0.0), want)
    assert ref.candidates(m, 10000, 0.01) == len(want) == 6
