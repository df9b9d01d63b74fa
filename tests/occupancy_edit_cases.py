"""A literal Python transcription of the occupancy map's edits (include/sbm.h, "occupancy map: edit voxels by key"): octomap's
updateNode(key, float), setNodeValue and deleteNode, stated per depth-16 voxel on top of tests/occupancy_option_cases.py (whose
Tree holds the voxels, the switches and the change states). TEST INFRASTRUCTURE ONLY, no GPU, no library.

    UPDATE, SET, DELETE                     the ops of an item; HIT and MISS are updateNode(key, bool), which only fixtures hold:
                                            the adaptors form the float on the host (floats_of)
    Tree(params, resolution)                oc.Tree with .edit(keys, ops, values) in item order, .edit_points(points, ops, values),
                                            .delete(keys, depth), .delete_box(kmin, kmax, outside), .last (the counts of the last
                                            call: items, skipped, created, removed)
    depth_mask(depth)                       the bits of a packed key in which deleteNode(key, depth) compares
    floats_of(ops, values, tree)            HIT / MISS items as the UPDATE items the C-ABI takes
    FX, NAMES, case_of(name), recorded(name)   tests/golden/occupancy_edit.npz: a case's steps, and what octomap answered after
                                            every step
    run_case(case)                          a case through a Tree -> what recorded() holds
"""
import pathlib

import numpy as np

import occupancy_option_cases as oc
import occupancy_ray_cases as rc

F = np.float32
UPDATE, SET, DELETE, HIT, MISS = 0, 1, 2, 3, 4
SCAN, EDIT, DELETE_KEYS, DELETE_BOX = 0, 1, 2, 3          # the kinds of a step
KEY_BITS = (1 << 48) - 1


def depth_mask(depth):
    if not 0 <= depth <= 16:
        raise ValueError(f"depth {depth} is outside 0..16")
    m = (0xFFFF << (16 - (depth or 16))) & 0xFFFF
    return m << 32 | m << 16 | m


def in_box(key, kmin, kmax):
    k = ((key >> 32) & 0xFFFF, (key >> 16) & 0xFFFF, key & 0xFFFF)
    return all(int(kmin[i]) <= k[i] <= int(kmax[i]) for i in range(3))


class Tree(oc.Tree):
    def __init__(self, rp=None, resolution=0.1):
        super().__init__(rp, resolution)
        self.last = dict(items=0, skipped=0, created=0, removed=0)

    def _record(self, key, born, before):
        """updateNodeRecurs' / setNodeValueRecurs' leaf code. A deleted voxel's record went with the voxel, so a voxel that is
        created never has one."""
        if not self.detect:
            return
        if born:
            self.changes[key] = oc.CREATED
        elif (before >= self.thres) != (self.v[key] >= self.thres):
            if key not in self.changes:
                self.changes[key] = oc.FLIPPED
            elif self.changes[key] == oc.FLIPPED:
                del self.changes[key]

    def update_node(self, key, u):
        u, v = F(u), self.v.get(key)
        if v is not None and ((u >= 0 and v >= self.cmax) or (u <= 0 and v <= self.cmin)):
            return                                      # the early abort: nothing happens at all
        before = F(0) if v is None else v
        with np.errstate(invalid="ignore", over="ignore"):
            w = F(before + u)
        if w < self.cmin:
            w = self.cmin
        elif w > self.cmax:
            w = self.cmax
        self.v[key] = w
        self._record(key, v is None, before)

    def set_node_value(self, key, x):
        x = F(x)
        x = self.cmin if x < self.cmin else x           # std::max(x, cmin)
        x = self.cmax if self.cmax < x else x           # std::min(.., cmax)
        v = self.v.get(key)
        self.v[key] = x
        self._record(key, v is None, v)

    def delete_node(self, key, depth=0):
        m = depth_mask(depth)
        gone = [k for k in self.v if (k & m) == (key & m)] if m != KEY_BITS else [key] if key in self.v else []
        for k in gone:
            del self.v[k]
            self.changes.pop(k, None)
        return len(gone)

    def edit(self, keys, ops, values):
        """Items in item order; ops None: all updates. An item with a bit above 47 or an unknown op is skipped."""
        start = set(self.v)
        touched, skipped, removed = set(), 0, 0
        for i, key in enumerate(int(k) for k in keys):
            op = UPDATE if ops is None else int(ops[i])
            if key >> 48 or op not in (UPDATE, SET, DELETE):
                skipped += 1
            elif op == DELETE:
                self.delete_node(key)
            else:
                touched.add(key)
                (self.update_node if op == UPDATE else self.set_node_value)(key, values[i])
        removed = len(start - set(self.v))
        # created: absent when the call began and given a slot, whatever became of it later in the call
        self.last = dict(items=len(keys), skipped=skipped, created=len(touched - start), removed=removed + len(
            [k for k in touched - start if k not in self.v]))
        return self

    def edit_points(self, points, ops, values):
        """The key is coordToKeyChecked; an item whose point has none is skipped (as a key above bit 47 is)."""
        factor = 1.0 / self.resolution
        keys = []
        for p in np.asarray(points, np.float32).reshape(-1, 3):
            k = rc.key3(p, factor)
            keys.append(1 << 48 if k is None else rc.pack3(k))
        return self.edit(keys, ops, values)

    def delete(self, keys, depth=0):
        removed = skipped = 0
        for key in (int(k) for k in keys):
            if key >> 48:
                skipped += 1
            else:
                removed += self.delete_node(key, depth)
        self.last = dict(items=len(keys), skipped=skipped, created=0, removed=removed)
        return self

    def delete_box(self, kmin, kmax, outside=False):
        gone = [k for k in self.v if in_box(k, kmin, kmax) != bool(outside)]
        for k in gone:
            self.delete_node(k)
        self.last = dict(items=0, skipped=0, created=0, removed=len(gone))
        return self


def floats_of(ops, values, t):
    """updateNode(key, bool) as the adaptors form it: HIT / MISS become UPDATE with the hit / miss log-odds"""
    ops, values = np.array(ops, np.uint8), np.array(values, np.float32)
    values[ops == HIT], values[ops == MISS] = t.hit, t.miss
    ops[(ops == HIT) | (ops == MISS)] = UPDATE
    return ops, values


def apply_step(t, s):
    """One step of a case on a Tree, or on anything with the same methods"""
    t.detect = s["detect"]
    if s["reset_changes"]:
        t.reset_changes()
    if s["kind"] == SCAN:
        t.insert(s["points"], s["origin"])
    elif s["kind"] == EDIT:
        ops, values = floats_of(s["ops"], s["values"], t)
        if s["form"]:
            t.edit_points(s["points"], ops, values)
        else:
            t.edit(s["keys"], ops, values)
    elif s["kind"] == DELETE_KEYS:
        t.delete(s["keys"], s["depth"])
    else:
        t.delete_box(s["box"][:3], s["box"][3:], s["outside"])


def run_case(case, resolution=0.1):
    """-> after every step (leaf keys, log-odds, changed keys, created flags)"""
    t = Tree(case["params"], resolution)
    out = []
    for s in case["steps"]:
        apply_step(t, s)
        out.append(t.leaves() + t.changed())
    return out


GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "occupancy_edit.npz"
FX = dict(np.load(GOLDEN)) if GOLDEN.exists() else {}
NAMES = [str(n) for n in FX.get("names", [])]
# what the two divergences of the header are about: the cases that show octomap's side
LAST_VOXEL, CHANGE_RECORD = "delete_last_voxel", "delete_change_record"


def case_of(name):
    """A fixture case as tools/make_occupancy_edit_fixtures.py describes one"""
    st = FX[f"{name}_steps"].astype(np.int64)       # per step: kind, detect, reset_changes, items, depth or outside, form
    ends = np.cumsum(st[:, 3])
    steps = []
    for i, (kind, detect, reset, n, arg, form) in enumerate(st):
        a = slice(ends[i] - n, ends[i])
        steps.append(dict(kind=int(kind), detect=bool(detect), reset_changes=bool(reset), form=int(form), depth=int(arg), outside=bool(arg),
                          keys=FX[f"{name}_keys"][a], points=FX[f"{name}_points"][a], ops=FX[f"{name}_ops"][a],
                          values=FX[f"{name}_values"][a], origin=FX[f"{name}_origins"][i], box=FX[f"{name}_boxes"][i]))
    return dict(params=rc.RayParams(*[float(v) for v in FX[f"{name}_params"]]), steps=steps, probes=FX[f"{name}_probes"])


def recorded(name):
    """-> per step (leaf keys, log-odds, changed keys, created flags, root_only, root value, per probe (found, value))"""
    nl, nc = FX[f"{name}_nleaves"].astype(np.int64), FX[f"{name}_nchanges"].astype(np.int64)
    a, b = np.cumsum(nl), np.cumsum(nc)
    return [(FX[f"{name}_leaf_keys"][a[i] - nl[i]:a[i]], FX[f"{name}_leaf_values"][a[i] - nl[i]:a[i]],
             FX[f"{name}_changed_keys"][b[i] - nc[i]:b[i]], FX[f"{name}_changed_created"][b[i] - nc[i]:b[i]],
             bool(FX[f"{name}_root_only"][i]), FX[f"{name}_root_value"][i], FX[f"{name}_probe_found"][i], FX[f"{name}_probe_value"][i])
            for i in range(len(nl))]
