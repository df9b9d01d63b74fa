"""tests/occupancy_edit_cases.py, the transcription of include/sbm.h's "occupancy map: edit voxels by key", against what the
reference's own octomap recorded in tests/golden/occupancy_edit.npz: equal after every step, bit for bit, but for the two named
divergences, where octomap's record differs by exactly what the header states. No GPU, no library."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_edit_cases as ec  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402

DIVERGES = {(ec.LAST_VOXEL, 1), (ec.CHANGE_RECORD, 2), (ec.CHANGE_RECORD, 3)}
WANTED = {"clamps", "zero_update", "set_beyond", "set_update_order", "delete_then_update", "delete_depths", "delete_in_pruned",
          "delete_absent", "delete_last_voxel", "points", "nan", "box_delete", "detect", "delete_change_record", "bool", "scene_edits"}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_the_fixture_holds_the_cases_the_contract_names():
    assert WANTED <= set(ec.NAMES)
    kinds = {int(k) for n in ec.NAMES for k in ec.FX[f"{n}_steps"][:, 0]}
    assert kinds == {ec.SCAN, ec.EDIT, ec.DELETE_KEYS, ec.DELETE_BOX}
    assert {int(d) for d in ec.FX["delete_depths_steps"][1:, 4]} == {16, 13, 1}


@pytest.mark.parametrize("name", ec.NAMES)
def test_restatement_equals_octomap_after_every_step(name):
    mine, theirs = ec.run_case(ec.case_of(name)), ec.recorded(name)
    assert len(mine) == len(theirs) > 0
    for i, (m, t) in enumerate(zip(mine, theirs)):
        if (name, i) in DIVERGES:
            continue
        assert not t[4], (name, i, "a bare root")
        assert np.array_equal(m[0], t[0]) and np.array_equal(bits(m[1]), bits(t[1])), (name, i, "leaves")
        assert np.array_equal(m[2], t[2]) and np.array_equal(m[3], t[3]), (name, i, "changes")


def test_deleting_the_last_voxel_diverges_as_stated():
    """Here: an empty map. octomap: a root without children, which search returns for every key."""
    mine, theirs = ec.run_case(ec.case_of(ec.LAST_VOXEL)), ec.recorded(ec.LAST_VOXEL)
    assert len(mine[0][0]) == 1 and not theirs[0][4] and list(theirs[0][6]) == [1, 0]      # before: one voxel, found; the other key not
    assert len(mine[1][0]) == 0 and len(mine[1][2]) == 0
    keys, _, _, _, root_only, root_value, found, value = theirs[1]
    assert root_only and len(keys) == 0 and found.all() and (value == bits(root_value)).all()


def test_a_deleted_voxels_change_record_diverges_as_stated():
    """Here the record goes with the voxel. octomap keeps the key in changed_keys, and its insert does not overwrite the entry
    when the voxel is created again: a stays `flipped` there and is `created` here."""
    case = ec.case_of(ec.CHANGE_RECORD)
    mine, theirs = ec.run_case(case), ec.recorded(ec.CHANGE_RECORD)
    a, b = (int(k) for k in case["steps"][2]["keys"])
    for i in (2, 3):
        assert np.array_equal(mine[i][0], theirs[i][0]) and np.array_equal(bits(mine[i][1]), bits(theirs[i][1]))      # the leaves agree
        assert dict(zip(map(int, theirs[i][2]), theirs[i][3])) == {a: 0, b: 1}
    assert a not in map(int, mine[2][0]) and len(mine[2][2]) == 0
    assert dict(zip(map(int, mine[3][2]), mine[3][3])) == {a: 1, b: 1}


def test_order_matters_where_the_cases_say_so():
    case = ec.case_of("set_update_order")
    s = case["steps"][0]
    t = ec.Tree(case["params"])
    t.edit(s["keys"], s["ops"], s["values"])
    back = ec.Tree(case["params"])
    back.edit(s["keys"][::-1], s["ops"][::-1], s["values"][::-1])
    two = [int(k) for k in s["keys"][-4:]]
    assert two[0] == two[1] != two[2] == two[3]
    assert bits(t.v[two[0]]) == bits(t.cmax) and t.v[two[2]] == np.float32(3.0)             # set then update; update then set
    assert back.v[two[0]] == np.float32(3.0) and bits(back.v[two[2]]) == bits(back.cmax)    # the reverse order swaps them
    case = ec.case_of("delete_then_update")
    s = case["steps"][1]
    t = ec.run_case(case)[1]
    a = int(s["keys"][0])
    assert s["ops"][0] == ec.DELETE and s["ops"][1] == ec.UPDATE and bits(t[1][list(map(int, t[0])).index(a)]) == bits(rc.logodds(0.7))


def test_the_early_abort_changes_nothing_and_records_nothing():
    t = ec.Tree()
    t.detect = True
    k = rc.pack3((1, 2, 3))
    t.set_node_value(k, 9.0)
    t.reset_changes()
    assert bits(t.v[k]) == bits(t.cmax)
    t.update_node(k, t.hit), t.update_node(k, 0.0)
    assert bits(t.v[k]) == bits(t.cmax) and not t.changes
    t.update_node(k, np.float32("nan"))               # a NaN fails both comparisons of the abort and both of the clamp
    assert np.isnan(t.v[k])
    t.set_node_value(k, np.float32("nan"))
    assert np.isnan(t.v[k])


def test_update_node_bool_is_update_node_float_with_the_formed_logodds():
    case = ec.case_of("bool")
    s = case["steps"][0]
    assert {ec.HIT, ec.MISS} <= set(map(int, s["ops"]))
    t = ec.Tree(case["params"])
    ops, values = ec.floats_of(s["ops"], s["values"], t)
    assert set(map(int, ops)) <= {ec.UPDATE, ec.SET}
    hit, miss = rc.logodds(case["params"].prob_hit), rc.logodds(case["params"].prob_miss)
    assert all(bits(v) == bits(hit if o == ec.HIT else miss) for o, v in zip(s["ops"], values) if o in (ec.HIT, ec.MISS))
    t.edit(s["keys"], ops, values)
    theirs = ec.recorded("bool")[0]                  # octomap ran updateNode(key, bool)
    assert np.array_equal(t.leaves()[0], theirs[0]) and np.array_equal(bits(t.leaves()[1]), bits(theirs[1]))


def test_depth_masks_and_skips():
    assert ec.depth_mask(0) == ec.depth_mask(16) == ec.KEY_BITS and ec.depth_mask(1) == 0x8000_8000_8000
    assert ec.depth_mask(13) == 0xFFF8_FFF8_FFF8
    with pytest.raises(ValueError):
        ec.depth_mask(17)
    t = ec.Tree().edit([1 << 48, 5, 5], [ec.UPDATE, 7, ec.SET], np.float32([1, 1, 1]))
    assert t.last == dict(items=3, skipped=2, created=1, removed=0) and list(t.v) == [5]
    t.edit_points(np.float32([[4000, 0, 0], [0.05, 0.05, 0.05]]), None, np.float32([1, 1]))
    assert t.last["skipped"] == 1 and len(t.v) == 2
