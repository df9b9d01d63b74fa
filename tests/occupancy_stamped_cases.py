"""A literal Python transcription of the occupancy map's time stamps (include/sbm.h, "occupancy map: time stamps per voxel"):
octomap's OcTreeStamped per depth-16 voxel on top of tests/occupancy_edit_cases.py (whose Tree holds the voxels, the switches and
the change states). TEST INFRASTRUCTURE ONLY, no GPU, no library.

    Map(params, resolution)                 ec.Tree with .clock (the map's clock, a uint32 the caller sets), a stamp per voxel,
                                            .degrade(time_thres) -> degraded, .forget(time_thres) -> removed,
                                            .stamped() -> (keys, log-odds, stamps), .search_stamps(points, thres)
    age(clock, stamp)                       (uint32)(clock - stamp): octomap's unsigned int subtraction
    SCAN, EDIT, DEGRADE, FORGET, SNAPSHOT, RESUME   the kinds of a step
    StampedTree(voxels, stamps, clock)      octomap's STAMPED pruned tree on top of tests/occupancy_tree_cases.py: collapsible is "all
                                            eight present, all leaves, equal value, equal stamp", bottom-up; .stamp[d][code];
                                            .nodes() pre-order with stamps; .root_stamp; .ot() the `id OcTreeStamped` stream
    parse(data, map_resolution)             occupancy_ot_cases.parse for the stamped id: any other id is UNSUPPORTED
    FX, NAMES, case_of(name), recorded(name), run_case(case)   tests/golden/occupancy_stamped.npz
"""
import pathlib

import numpy as np

import occupancy_edit_cases as ec
import occupancy_ot_cases as otc
import occupancy_ray_cases as rc
import occupancy_tree_cases as tc

F = np.float32
SCAN, EDIT, DEGRADE, FORGET, SNAPSHOT, RESUME = 0, 1, 2, 3, 4, 5
LOGODDS, MAXLIKELIHOOD = 0, 1                  # the two readings of a snapshot
OT_HEADER = otc.HEADER.replace("id OcTree\n", "id OcTreeStamped\n")
DISCRETIZE, USE_BOX, DETECT = 1, 2, 4          # the flags of a scan step
U32 = 0xFFFFFFFF


def age(clock, stamp):
    return (int(clock) - int(stamp)) & U32


class Map(ec.Tree):
    def __init__(self, rp=None, resolution=0.1):
        super().__init__(rp, resolution)
        self.clock = 0
        self.s = {}                                   # packed key -> stamp, of every voxel

    def _early(self, key, u):
        """updateNode's early return, which comes before updateNodeLogOdds: the voxel exists and sits at the clamp in the
        direction of the update. An update of exactly 0 tests both."""
        v = self.v.get(key)
        return v is not None and ((u >= 0 and v >= self.cmax) or (u <= 0 and v <= self.cmin))

    def update(self, key, u):
        """a scan's one update of a voxel"""
        early = self._early(key, F(u))
        super().update(key, u)
        if not early:
            self.s[key] = self.clock & U32            # OcTreeStamped::updateNodeLogOdds: updateTimestamp()

    def update_node(self, key, u):
        """an UPDATE item of an edit batch"""
        early = self._early(key, F(u))
        super().update_node(key, u)
        if not early:
            self.s[key] = self.clock & U32

    def set_node_value(self, key, x):
        """setNodeValue never stamps; a voxel it creates has stamp 0"""
        super().set_node_value(key, x)
        self.s.setdefault(key, 0)

    def delete_node(self, key, depth=0):
        n = super().delete_node(key, depth)
        for k in [k for k in self.s if k not in self.v]:
            del self.s[k]                             # a deleted voxel goes with its stamp: created again, it starts from 0
        return n

    def clear(self):
        super().clear()
        self.s = {}

    def degrade(self, time_thres):
        """degradeOutdatedNodes: isNodeOccupied and (clock - stamp) > time_thres in uint32 -> one miss update, clamped
        (integrateMissNoTime); the stamp and the change states stay"""
        n = 0
        for k, v in self.v.items():
            if v >= self.thres and age(self.clock, self.s[k]) > int(time_thres):
                w = F(v + self.miss)
                if w < self.cmin:
                    w = self.cmin
                elif w > self.cmax:
                    w = self.cmax
                self.v[k] = w
                n += 1
        return n

    def forget(self, time_thres):
        """every voxel with (clock - stamp) > time_thres in uint32 is deleted, whatever its value"""
        old = [k for k in self.v if age(self.clock, self.s[k]) > int(time_thres)]
        for k in old:
            self.delete_node(k)
        self.last = dict(items=0, skipped=0, created=0, removed=len(old))
        return len(old)

    def stamped(self):
        keys, lo = self.leaves()
        return keys, lo, np.array([self.s[int(k)] for k in keys], np.uint32)

    def search_stamps(self, points, thres=0.0):
        """-> (state int32, value bits uint32, stamps uint32) of search(point) per point"""
        factor = 1.0 / self.resolution
        st, val, stamp = [], [], []
        for p in np.asarray(points, np.float32).reshape(-1, 3):
            k = rc.key3(p, factor)
            key = None if k is None else rc.pack3(k)
            if key is None or key not in self.v:
                st.append(tc.CELL_OUT if key is None else tc.CELL_UNKNOWN), val.append(0x7FC00000), stamp.append(0)
            else:
                v = self.v[key]
                st.append(tc.CELL_OCCUPIED if v >= F(thres) else tc.CELL_FREE), val.append(int(F(v).view(np.uint32))), stamp.append(self.s[key])
        return np.array(st, np.int32), np.array(val, np.uint32), np.array(stamp, np.uint32)


class StampedTree(tc.Tree):
    """prune() and updateInnerOccupancy() of an OcTreeStamped. OcTreeNodeStamped's operator== compares value AND stamp, so eight
    siblings of equal value collapse only if their stamps are equal too; a collapsed node has the common stamp (copyData), every
    other inner node the clock at the time of updateInnerOccupancy()."""

    def __init__(self, voxels, stamps, clock, resolution=0.1):
        super().__init__(voxels, resolution)
        D = tc.DEPTH
        self.stamp = [dict() for _ in range(D + 1)]
        self.stamp[D] = {rc.morton(int(k)): int(stamps[int(k)]) for k in voxels}
        self.collapsed = [set() for _ in range(D + 1)]
        for d in range(D - 1, -1, -1):
            kids = {}
            for code, v in self.level[d + 1].items():
                kids.setdefault(code >> 3, []).append((code, v))
            for code, ch in kids.items():
                same = (len(ch) == 8 and all(v == ch[0][1] for _, v in ch) and all(self.stamp[d + 1][c] == self.stamp[d + 1][ch[0][0]] for c, _ in ch)
                        and (d + 1 == D or all(c in self.collapsed[d + 1] for c, _ in ch)))
                if same:
                    self.collapsed[d].add(code)
                self.stamp[d][code] = self.stamp[d + 1][ch[0][0]] if same else int(clock) & U32
        self.top = [dict() for _ in range(D + 1)]
        for d in range(D + 1):
            for code in self.level[d]:
                above = self.top[d - 1][code >> 3] if d else None
                self.top[d][code] = above if above is not None else (d if code in self.collapsed[d] else None)
        self.nodes_at = [sum(1 for c in self.level[d] if self.in_pruned(c, d)) for d in range(D + 1)]
        self.leaves_at = [sum(1 for c in self.level[d] if self.in_pruned(c, d) and self.is_leaf(c, d)) for d in range(D + 1)]
        self.size, self.num_leaves = sum(self.nodes_at), sum(self.leaves_at)
        self.root_stamp = self.stamp[0].get(0, 0)

    def nodes(self):
        """every node of the pruned tree in pre-order -> (centre keys, depths, values, stamps, leaf flags)"""
        rows = self._walk(tc.DEPTH, True)
        return self._arrays(rows) + (np.array([self.stamp[d][c] for c, d, _, _ in rows], np.uint32), np.array([leaf for _, _, _, leaf in rows], np.uint8))

    def leaves_stamps(self, max_depth=0):
        rows = self._walk(max_depth or tc.DEPTH, False)
        return self._arrays(rows) + (np.array([self.stamp[d][c] for c, d, _, _ in rows], np.uint32),)

    def ot(self):
        """AbstractOcTree::write: OcTreeNodeStamped does not override writeData, so the plain five-byte records under the other id"""
        return (OT_HEADER % (self.size, self.resolution)).encode() + otc.body(self)


def parse(data, map_resolution=None):
    """read() of an `id OcTreeStamped` stream: the plain parser behind the other id test"""
    b = bytes(data)
    if b"\nid OcTreeStamped\n" not in b[:b.find(b"\ndata\n") + 1]:
        p = otc.parse(b, map_resolution)
        if p.status == otc.OK:
            p.status = otc.UNSUPPORTED
        return p
    return otc.parse(b.replace(b"\nid OcTreeStamped\n", b"\nid OcTree\n", 1), map_resolution)


def snapshot(m):
    """What a snapshot step records: per reading (nodes, root stamp, stream), LOGODDS with the .ot, MAXLIKELIHOOD with the .bt"""
    lo = StampedTree(m.v, m.s, m.clock, m.resolution)
    consts = (m.hit, m.miss, m.cmin, m.cmax, m.thres)
    ml = StampedTree(tc.max_likelihood(m.v, tc.LOGODDS_MODE, consts), m.s, m.clock, m.resolution)
    return [(lo.nodes(), lo.root_stamp, lo.ot()), (ml.nodes(), ml.root_stamp, ml.stream(m.cmax).replace(b"\nid OcTree\n", b"\nid OcTreeStamped\n", 1))]   # writeBinary names the class too


def apply_step(m, s):
    """One step of a case on a Map, or on anything with the same methods -> the step's count (degraded, removed; else 0)"""
    m.clock = int(s["clock"])
    if s["kind"] == SCAN:
        if s["flags"] & USE_BOX:
            assert m.box.set(s["box"][:3], s["box"][3:])
        m.use_box, m.detect = bool(s["flags"] & USE_BOX), bool(s["flags"] & DETECT)
        m.insert(s["points"], s["origin"], bool(s["flags"] & DISCRETIZE))
    elif s["kind"] == EDIT:
        ops, values = ec.floats_of(s["ops"], s["values"], m)
        m.edit(s["keys"], ops, values)
    elif s["kind"] == DEGRADE:
        return m.degrade(s["thres"])
    elif s["kind"] == FORGET:
        return m.forget(s["thres"])
    elif s["kind"] == RESUME:
        leaves = otc.expand(parse(StampedTree(m.v, m.s, m.clock, m.resolution).ot(), m.resolution))
        m.v = {int(k): F(v) for k, v in zip(*leaves)}
        m.s = {k: 0 for k in m.v}                     # the stream carries no stamps
    return 0


def run_case(case, resolution=0.1):
    """-> per step (keys, log-odds, stamps, count) and, for a snapshot, a fifth entry: what snapshot() gives"""
    m = Map(case["params"], resolution)
    out = []
    for s in case["steps"]:
        n = apply_step(m, s)
        out.append(m.stamped() + (n,) + ((snapshot(m),) if s["kind"] == SNAPSHOT else ()))
    return out


def same_snapshot(mine, theirs):
    for (a, ra, da), (b, rb, db) in zip(mine, theirs):
        if not (all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else np.asarray(x),
                                   np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else np.asarray(y)) for x, y in zip(a, b))
                and int(ra) == int(rb) and bytes(da) == bytes(db)):
            return False
    return True


def same(mine, theirs):
    """A step of run_case against a step of recorded, exact in every integer and float bit"""
    if len(mine) > 4 and not same_snapshot(mine[4], theirs[4]):
        return False
    return (np.array_equal(mine[0], theirs[0]) and np.array_equal(np.asarray(mine[1], np.float32).view(np.uint32), np.asarray(theirs[1], np.float32).view(np.uint32))
            and np.array_equal(mine[2], theirs[2]) and int(mine[3]) == int(theirs[3]))


GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "occupancy_stamped.npz"
FX = dict(np.load(GOLDEN)) if GOLDEN.exists() else {}
NAMES = [str(n) for n in FX.get("names", [])]


def case_of(name):
    """A fixture case as tools/make_occupancy_stamped_fixtures.py describes one"""
    st = FX[f"{name}_steps"].astype(np.int64)       # per step: kind, clock, items, flags, thres
    ends = np.cumsum(st[:, 2])
    steps = []
    for i, (kind, clock, n, flags, thres) in enumerate(st):
        a = slice(ends[i] - n, ends[i])
        steps.append(dict(kind=int(kind), clock=int(clock), flags=int(flags), thres=int(thres), keys=FX[f"{name}_keys"][a], points=FX[f"{name}_points"][a],
                          values=FX[f"{name}_values"][a], ops=FX[f"{name}_ops"][a], origin=FX[f"{name}_origins"][i], box=FX[f"{name}_boxes"][i]))
    return dict(params=rc.RayParams(*[float(v) for v in FX[f"{name}_params"]]), steps=steps)


def recorded(name):
    """What octomap answered, in the shape of run_case"""
    nv = FX[f"{name}_nvoxels"].astype(np.int64)
    ends = np.cumsum(nv)
    out = [(FX[f"{name}_voxel_keys"][ends[i] - nv[i]:ends[i]], FX[f"{name}_voxel_values"][ends[i] - nv[i]:ends[i]],
            FX[f"{name}_voxel_stamps"][ends[i] - nv[i]:ends[i]], int(FX[f"{name}_counts"][i])) for i in range(len(nv))]
    kinds = FX[f"{name}_steps"][:, 0]
    nn, ns = FX[f"{name}_nnodes"].astype(np.int64), FX[f"{name}_nstream"].astype(np.int64)     # two per snapshot: LOGODDS, MAXLIKELIHOOD
    en, es = np.cumsum(nn), np.cumsum(ns)
    j = 0
    for i, k in enumerate(kinds):
        if k != SNAPSHOT:
            continue
        snap = []
        for _ in range(2):
            a, b = slice(en[j] - nn[j], en[j]), slice(es[j] - ns[j], es[j])
            snap.append(((FX[f"{name}_node_keys"][a], FX[f"{name}_node_depths"][a].astype(np.int32), FX[f"{name}_node_values"][a], FX[f"{name}_node_stamps"][a],
                          FX[f"{name}_node_leaf"][a]), int(FX[f"{name}_root_stamps"][j]), FX[f"{name}_streams"][b].tobytes()))
            j += 1
        out[i] = out[i] + (snap,)
    return out
