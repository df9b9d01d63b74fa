"""The host half of the pose-graph optimiser (u96-slam_amd/csrc/sbm_pgo_plan.hip: the checks, the partition, getConnectedGraph and
the robust loop's link bookkeeping) compiled alone as host C++ under the address and undefined-behaviour sanitizers and run as a
child process (tests/cpp/pgo_plan_main.cpp): nothing of ROCm and nothing of the engine library is linked. Its plan must be the
built library's, its connected graph the numpy restatement's bit for bit, its refusals those of test_check_status_codes."""
import pathlib
import subprocess

import numpy as np
import pytest

import pgo_cases as pc
from test_pgo_cabi import REFUSALS

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "u96-slam_amd" / "csrc"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """run(c, run_max, coupling, fixed_id) -> what the program prints for graph c, as a dict of lists of words."""
    d = tmp_path_factory.mktemp("pgo_plan_host")
    exe = d / "pgo_plan"
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        str(CSRC), "-x", "c++", str(ROOT / "tests" / "cpp" / "pgo_plan_main.cpp"), str(CSRC / "sbm_pgo_plan.hip"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run_(c, run_max=64, coupling=pc.REFERENCE, fixed_id=1):
        ids, poses, frm, to, meas, _ = pc.args(c)
        with open(d / "graph.bin", "wb") as f:
            f.write(np.array([len(ids), len(frm), run_max, coupling, fixed_id], np.int32).tobytes())
            for a in (ids, frm, to):
                f.write(np.asarray(a, np.int32).tobytes())
            for a in (poses, meas):
                f.write(np.asarray(a, np.float64).tobytes())
        r = subprocess.run([str(exe), str(d / "graph.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
        return {w[0]: w[1:] for w in (line.split() for line in r.stdout.splitlines())}

    return run_


def ints(words):
    return np.array([int(w) for w in words], np.int64)


@pytest.mark.parametrize("coupling", [pc.REFERENCE, pc.SYMMETRIC], ids=["reference", "symmetric"])
@pytest.mark.parametrize("run_max", [1, 4, 64])
def test_plan_is_the_librarys(pkg, run, run_max, coupling):
    for name, c in pc.shape_cases(run_max).items():
        info, vrun, rc, couples = pkg.pgo_plan(pkg.pgo_params(coupling=coupling, run_max=run_max, fixed_id=pc.fixed(c)), *pc.args(c))
        out = run(c, run_max, coupling, pc.fixed(c))
        assert out["check"] == ["0"] and out["plan"] == ["0"], name
        assert ints(out["counts"]).tolist() == [info.n_free, info.n_runs, info.n_junctions, info.schur_size, info.n_coupling,
                                                info.longest_run, info.n_slots, info.max_junctions], name
        assert np.array_equal(ints(out["vrun"]), vrun), name
        assert np.array_equal(ints(out["slot_rc"]).reshape(-1, 2), rc), name
        assert np.array_equal(ints(out["couples"]).astype(bool), couples), name


def second_round(c):
    """robust_case() as the robust loop sees it in its second round: the outlier link (27, 41) removed."""
    keep = ~((c["frm"] == 27) & (c["to"] == 41))
    assert keep.sum() == len(keep) - 1
    return dict(c, frm=c["frm"][keep], to=c["to"][keep], meas=c["meas"][keep], info=c["info"][keep])


# name -> (graph, the vertex the walk starts from). The bidirectional graphs are what the reference's mapper stores: the walk
# keeps one link per vertex pair, in whichever direction it met first; started mid-chain most kept links run to a smaller id.
CONNECTED = {"robust60": (pc.robust_case(), 1), "unreachable": (pc.unreachable_case(), 1),
             "double_link": (pc.shape_cases()["double_link"], 1), "robust60_second_round": (second_round(pc.robust_case()), 1),
             "robust60_bidir": (pc.bidirectional(pc.robust_case()), 1),
             "multi48_bidir_gaps": (pc.relabel(pc.bidirectional(pc.multi_outlier_case()), pc.gapped), 1),
             "multi48_bidir_from_mid": (pc.bidirectional(pc.multi_outlier_case()), 23)}


@pytest.mark.parametrize("name", list(CONNECTED))
def test_connected_graph_bit_for_bit(run, name):
    c, start = CONNECTED[name]
    ids, poses, frm, to, meas, _ = pc.args(c)
    oid, oposes, kept = pc.connected_graph(start, ids, poses, frm, to, meas)
    out = run(c, fixed_id=start)
    assert np.array_equal(ints(out["reached"]), oid)
    assert np.array_equal(ints(out["kept"]), kept)
    got = np.array([float.fromhex(w) for w in out["poses"]], np.float64).reshape(-1, 3, 4)
    assert got.tobytes() == np.ascontiguousarray(oposes, np.float64).tobytes()
    if name == "unreachable":
        assert 9 not in oid and len(oid) == len(ids) - 1
    if "bidir" in name:                                       # one link per pair, and a good share of them towards the smaller id
        pairs = [frozenset(p) for p in zip(frm[kept].tolist(), to[kept].tolist())]
        assert len(set(pairs)) == len(pairs) == len(frm) // 2
        down = int((frm[kept] > to[kept]).sum())
        print(name, "kept", len(kept), "of them from the larger id to the smaller", down)
        assert down >= (len(kept) // 3 if start != 1 else 3)


TOPOLOGY = [r for r in REFUSALS if r[0] in ("ok", "duplicate_id", "fixed_absent", "edge_absent_from", "edge_absent_to", "self_edge")]


@pytest.mark.parametrize("name,change,c,code", TOPOLOGY, ids=[r[0] for r in TOPOLOGY])
def test_refusals_through_the_program(run, name, change, c, code):
    assert run(c, fixed_id=change.get("fixed_id", 1))["check"] == [str(code)]
