#!/usr/bin/env python3
"""What the generators tools/make_occupancy_*_fixtures.py share: the build of the reference's octomap and of a driver against
it, both sides of the record protocol between a generator and its driver (tools/octomap_drivers/driver.h describes it), the
deterministic .npz writer, and the small arithmetic of keys, voxels and floats.

The fixtures depend on each other in the order of FIXTURES, then of LATER_FIXTURES, then of MORE_FIXTURES: a generator reads
earlier fixtures from tests/golden (load()) and writes its own to --out. Run as a program, this file runs the whole chain in
that order:

    python tools/octomap_kit.py --reference /path/to/U96-SLAM [--out DIR]

FIXTURES is closed: tests/test_occupancy_fixture_kit.py pins its six names. A new fixture adds a driver
tools/octomap_drivers/<name>.cpp, a generator with its cases, and its line in MORE_FIXTURES, the open mapping: LATER_FIXTURES is
pinned as well (tests/test_occupancy_options_cabi.py), and no test pins what MORE_FIXTURES holds. load() takes every fixture of
LATER_FIXTURES as later than all of FIXTURES, and every fixture of MORE_FIXTURES as later than both.
"""
import argparse
import concurrent.futures
import hashlib
import io
import json
import os
import pathlib
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "oracle"), str(ROOT / "tests"), str(ROOT / "tools")]
import bench_occupancy_rays as bench  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
DRIVERS = ROOT / "tools" / "octomap_drivers"
BUILD = ROOT / "oracle" / "_ref" / "octomap_kit"        # untracked: the archive and the driver binaries
# fixture -> its generator, in the order in which they depend on each other
FIXTURES = {"octomap": "make_occupancy_fixtures.py", "rays": "make_occupancy_ray_fixtures.py", "query": "make_occupancy_query_fixtures.py",
            "tree": "make_occupancy_tree_fixtures.py", "load": "make_occupancy_load_fixtures.py", "ot": "make_occupancy_ot_fixtures.py"}
# fixtures added after that list was closed, in their own order of dependence; they may read every fixture above
LATER_FIXTURES = {"options": "make_occupancy_option_fixtures.py"}
# open: every later fixture goes here, in its order of dependence; they may read every fixture of the two mappings above
MORE_FIXTURES = {"edit": "make_occupancy_edit_fixtures.py", "planner": "make_occupancy_planner_fixtures.py", "color": "make_occupancy_color_fixtures.py",
                 "stamped": "make_occupancy_stamped_fixtures.py"}
RESOLUTION = 0.1
PROBS = ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres")
DEFAULT_PROBS = [getattr(rc.RayParams(), k) for k in PROBS]
BENCH_PLANES, BENCH_RANGE = 4, 25.0
CXX = ["g++", "-O1", "-std=c++11"]          # the recorded float bits and CPU times were made with these flags


# ---- build ----

def build(reference, driver, extra=()):
    """The reference's octomap sources, compiled once into a static archive (kept under a name made of the sources' and the
    flags' hash, so that every generator of a chain finds it), and tools/octomap_drivers/<driver>.cpp linked against it
    -> the binary's path. extra: flags added to CXX for the archive and the driver alike, which then have an archive of their own"""
    CXX = globals()["CXX"] + list(extra)
    ref = pathlib.Path(reference) / "src" / "slam"
    include = ["-I", str(ref / "include"), "-I", str(ref / "include" / "octomap")]
    srcs = sorted(str(p) for p in (ref / "src" / "octomap").glob("*.cpp"))
    h = hashlib.sha256(" ".join(CXX + include + srcs).encode())
    for s in srcs:
        h.update(pathlib.Path(s).read_bytes())
    work = BUILD / h.hexdigest()[:16]
    archive = work / "liboctomap.a"
    if not archive.exists():
        work.mkdir(parents=True, exist_ok=True)
        with tempfile.TemporaryDirectory(dir=work) as tmp:
            objs = [str(pathlib.Path(tmp) / (pathlib.Path(s).stem + ".o")) for s in srcs]
            with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
                list(pool.map(lambda so: subprocess.run(CXX + include + ["-c", so[0], "-o", so[1]], check=True), zip(srcs, objs)))
            subprocess.run(["ar", "rcs", str(pathlib.Path(tmp) / "liboctomap.a")] + objs, check=True)
            os.replace(pathlib.Path(tmp) / "liboctomap.a", archive)
    binary = work / driver
    # the whole archive: octomap's tree classes register themselves for AbstractOcTree::read from static initialisers, which a
    # link that takes only the referenced members would leave out
    subprocess.run(CXX + ["-Wall", "-Wextra"] + include + ["-o", str(binary), str(DRIVERS / f"{driver}.cpp"), "-Wl,--whole-archive",
                          str(archive), "-Wl,--no-whole-archive"], check=True)
    return binary


def run(driver, tag, write):
    """write(f) fills the driver's input -> (return code, the bytes it answered)"""
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        with open(tmp / f"{tag}.in", "wb") as f:
            write(f)
        r = subprocess.run([str(driver), str(tmp / f"{tag}.in"), str(tmp / f"{tag}.out")], stderr=subprocess.DEVNULL, timeout=600)
        return r.returncode, (tmp / f"{tag}.out").read_bytes()


# ---- the record protocol, writing side: each returns bytes ----

def head(probs=DEFAULT_PROBS, resolution=RESOLUTION):
    """probs: five probabilities, or a RayParams"""
    return struct.pack("<6d", *([getattr(probs, k) for k in PROBS] if isinstance(probs, rc.RayParams) else probs), resolution)


def ints(*values):
    return struct.pack(f"<{len(values)}i", *(int(v) for v in values))


def points(p):
    p = np.asarray(p, np.float32).reshape(-1, 3)
    return ints(len(p)) + p.tobytes()


def scan(origin, max_range, p):
    return np.asarray(origin, np.float32).tobytes() + struct.pack("<d", max_range) + points(p)


def scans(items):
    """items: [(origin, max_range, points)]"""
    return ints(len(items)) + b"".join(scan(*s) for s in items)


def hits(keys, counts=None):
    """keys: packed uint64; counts: how often each is hit (once, if not given)"""
    counts = np.ones(len(keys), np.uint32) if counts is None else np.asarray(counts, np.uint32)
    return ints(len(keys)) + occ.unpack(keys).tobytes() + counts.tobytes()


def stream(data):
    return struct.pack("<I", len(data)) + data


# ---- the record protocol, reading side ----

NODE = np.dtype([("k", "<u2", 3), ("depth", "<u2"), ("value", "<f4")])
FOUND_VALUE = np.dtype([("found", "<i4"), ("value", "<u4")])
FOUND_VALUE_DEPTH = np.dtype([("found", "<i4"), ("value", "<u4"), ("depth", "<i4")])


class Reader:
    def __init__(self, raw):
        self.raw, self.off = raw, 0

    def take(self, dtype, n=1):
        a = np.frombuffer(self.raw, dtype, n, self.off)
        self.off += a.nbytes
        return a

    def one(self, dtype):
        return self.take(dtype)[0].item()

    def nodes(self, n, depth_type):
        """-> packed keys, depths as depth_type, values"""
        rec = self.take(NODE, n)
        return occ.pack(rec["k"]), rec["depth"].astype(depth_type), rec["value"].copy()

    def leaves(self, depth_type=np.uint8):
        return self.nodes(self.one("<u4"), depth_type)

    def voxels(self, n):
        """n keys, then n values -> both sorted by packed key"""
        k, v = occ.pack(self.take("<u2", 3 * n)), self.take("<f4", n)
        order = np.argsort(k)
        return k[order], v[order]

    def stream(self):
        return self.take(np.uint8, self.one("<u4")).copy()

    def done(self):
        assert self.off == len(self.raw), (self.off, len(self.raw))


# ---- output ----

def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def numpy_npz(path, arrays):
    """The writer the bytes of occupancy_octomap.npz and occupancy_rays.npz came from"""
    np.savez_compressed(path, **arrays)


def write_sha256(path):
    path.with_suffix(".sha256").write_text(hashlib.sha256(path.read_bytes()).hexdigest() + "  " + path.name + "\n")


def save(out_dir, name, arrays, writer=write_npz, cpu=None):
    """occupancy_<name>.npz, its .sha256 and, where octomap was timed, occupancy_<name>_cpu.json -> the .npz's path"""
    path = pathlib.Path(out_dir) / f"occupancy_{name}.npz"
    path.parent.mkdir(parents=True, exist_ok=True)
    writer(path, arrays)
    write_sha256(path)
    if cpu is not None:
        (pathlib.Path(out_dir) / f"occupancy_{name}_cpu.json").write_text(json.dumps(cpu, indent=1) + "\n")
    return path


def load(name, by):
    """The committed fixture `name`, for the generator of fixture `by`, which has to come later in FIXTURES + LATER_FIXTURES +
    MORE_FIXTURES"""
    order = list(FIXTURES) + list(LATER_FIXTURES) + list(MORE_FIXTURES)
    assert order.index(name) < order.index(by), f"{by} cannot depend on {name}"
    return dict(np.load(GOLDEN / f"occupancy_{name}.npz"))


def arguments(doc):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--out", default=str(GOLDEN), help="where the fixture is written; earlier fixtures are read from tests/golden")
    return ap.parse_args()


# ---- small arithmetic ----

def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def f32(v):
    return np.float32(v)


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def voxel(j, dtype=np.float64):
    """centre of the voxel with key 32768 + j"""
    return ((np.asarray(j, np.float64) + 0.5) * RESOLUTION).astype(dtype)


def centres(keys):
    """keyToCoord of (n, 3) keys as float32 points"""
    return voxel(np.asarray(keys, np.float64) - 32768).astype(np.float32)


def scans_of(fixture, name):
    """[(origin, max_range, points)] of the scans a fixture stores under `name`, whether with one range or one per scan"""
    n = fixture[f"{name}_npoints"]
    ends = np.cumsum(n)
    ranges = fixture[f"{name}_scan_range"] if f"{name}_scan_range" in fixture else np.full(len(n), fixture[f"{name}_params"][5])
    return [(fixture[f"{name}_origins"][i], float(ranges[i]), fixture[f"{name}_points"][ends[i] - n[i]:ends[i]]) for i in range(len(n))]


def scene(by):
    """The three planes of tools/make_occupancy_fixtures.py, as its fixture keeps them -> (planes, poses, model)"""
    f = load("octomap", by)
    return f["scene_disp"], f["scene_poses"], occ.model_from_array(f["model"])


def bench_scans(planes=BENCH_PLANES, max_range=BENCH_RANGE):
    """The scans of the benchmarks' synthetic scene (tools/bench_occupancy_rays.py), which octomap is timed on"""
    disp, poses = bench.synth_planes(planes)
    m = bench.synth_model()
    return [(pose[[3, 7, 11]], max_range, rc.plane_points(d, bench.SCALE, m, pose)) for d, pose in zip(disp, poses)]


if __name__ == "__main__":
    args = arguments(__doc__)
    for tool in list(FIXTURES.values()) + list(LATER_FIXTURES.values()) + list(MORE_FIXTURES.values()):
        subprocess.run([sys.executable, str(ROOT / "tools" / tool), "--reference", args.reference, "--out", args.out], check=True)
