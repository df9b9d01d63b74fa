"""Designed inputs for the block matcher's two post-filters (sbm_lrcheck.hip, sbm_speckle.hip), pure numpy. TEST INFRASTRUCTURE ONLY.

Every case carries its map(s), its parameters and a closed-form statement of which pixels survive that uses neither reference:
the sizes of the components come from the arithmetic of the drawing (rows x columns, legs of a path), the survivors of an LR row
from the gadget that put the pixels there. tests/test_postfilter_cases.py holds the cases to the oracle, to the numpy restatements
below and to their own promises; tests/test_gpu_postfilter.py feeds them to the device filters through sbm_debug_postfilter.

The input contract of that entry (what the SAD kernels produce) is `contract_ok`: a pixel is (minDisparity - 1) * 16 or lies within
[minDisparity * 16, (minDisparity + numDisparities - 1) * 16]; costs are non-negative and at most 65534 where the cost plane has
16 bits."""
import numpy as np

# ---- independent numpy restatements of the two filters -----------------------------------------


def np_validate(disp, cost, mind, nd, tol_px):
    """Independent numpy restatement of SURVEY.md Appendix A.5."""
    disp = disp.copy()
    h, w = disp.shape
    inv = (mind - 1) * 16
    for y in range(h):
        d2 = np.full(w, inv, np.int64)
        c2 = np.full(w, np.iinfo(np.int64).max, np.int64)
        row = disp[y].astype(np.int64)
        for x in range(max(mind + nd, 0), w + min(mind, 0)):
            d = row[x]
            if d == inv:
                continue
            x2 = x - ((d + 8) >> 4)
            if c2[x2] > cost[y, x]:
                c2[x2], d2[x2] = cost[y, x], d
        for x in range(max(mind + nd, 0), w + min(mind, 0)):
            d = row[x]
            if d == inv:
                continue
            bad = []
            for xx in (x - (d >> 4), x - ((d + 15) >> 4)):
                bad.append(0 <= xx < w and d2[xx] > inv and abs(d2[xx] - d) > tol_px * 16)
            if all(bad):
                disp[y, x] = inv
    return disp


def np_components(img, new_val, max_diff):
    """Labels of the plain 4-connected components of "both valid and within max_diff" (scipy.sparse.csgraph), one per pixel;
    the labels of filtered pixels mean nothing."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    h, w = img.shape
    v = img.astype(np.int64)
    valid = v != new_val
    idx = np.arange(h * w).reshape(h, w)
    rows, cols = [], []
    m = valid[:, :-1] & valid[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= max_diff)
    rows.append(idx[:, :-1][m]); cols.append(idx[:, 1:][m])
    m = valid[:-1] & valid[1:] & (np.abs(v[:-1] - v[1:]) <= max_diff)
    rows.append(idx[:-1][m]); cols.append(idx[1:][m])
    r, c = np.concatenate(rows), np.concatenate(cols)
    g = coo_matrix((np.ones(r.size), (r, c)), shape=(h * w, h * w))
    _, lab = connected_components(g, directed=False)
    return lab.reshape(h, w)


def np_speckles(img, new_val, max_size, max_diff):
    """Independent restatement of Appendix A.6 as plain connected components (graph edges between
    4-neighbours that are both valid and within max_diff), via scipy.sparse.csgraph."""
    lab = np_components(img, new_val, max_diff).ravel()
    valid = img.astype(np.int64) != new_val
    sizes = np.bincount(lab)
    out = img.copy()
    kill = valid.ravel() & (sizes[lab] <= max_size)
    out.ravel()[kill] = new_val
    return out


def contract_ok(disp, mind, nd, cost=None, cost16=False):
    d = np.asarray(disp).astype(np.int64)
    inv = (mind - 1) * 16
    ok = bool(((d == inv) | ((d >= mind * 16) & (d <= (mind + nd - 1) * 16))).all())
    if cost is not None:
        c = np.asarray(cost).astype(np.int64)
        ok = ok and bool((c >= 0).all()) and (not cost16 or bool((c[d != inv] <= 65534).all()))
    return ok


def count_runs(row, new_val, max_diff):
    """Runs of one row: maximal stretches of valid pixels each within max_diff of its left neighbour."""
    v = row.astype(np.int64)
    valid = v != new_val
    joined = np.zeros(v.size, bool)
    joined[1:] = valid[1:] & valid[:-1] & (np.abs(v[1:] - v[:-1]) <= max_diff)
    return int((valid & ~joined).sum())


def count_contacts(up, dn, new_val, max_diff):
    """Contacts of two rows as the band walk lists them: stretches of columns where the same run above touches the same run below."""
    u, d = up.astype(np.int64), dn.astype(np.int64)
    touch = (u != new_val) & (d != new_val) & (np.abs(u - d) <= max_diff)

    def joined(v):
        j = np.zeros(v.size, bool)
        j[1:] = (v[1:] != new_val) & (v[:-1] != new_val) & (np.abs(v[1:] - v[:-1]) <= max_diff)
        return j

    same = np.zeros(u.size, bool)
    same[1:] = touch[1:] & touch[:-1] & joined(u)[1:] & joined(d)[1:]
    return int((touch & ~same).sum())


# ---- speckle cases -------------------------------------------------------------------------------------------------------------
# The matcher of every speckle case: minDisparity 0, 64 disparities, so newval = -16 and values within 0 .. 1008.
SPK_MIND, SPK_ND, SPK_NEWVAL = 0, 64, -16
SPK_DIFF = 32            # speckleRange of most cases
VAL_A, VAL_B = 320, 400  # two values more than SPK_DIFF apart


class Canvas:
    """A map under construction: img, and per pixel the id of the shape that drew it (0: filtered). size[id] is the shape's
    size as its drawing ARITHMETIC gives it, never a count of the pixels."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.img = np.full((H, W), SPK_NEWVAL, np.int16)
        self.ids = np.zeros((H, W), np.int32)
        self.size = {}

    def new(self):
        k = len(self.size) + 1
        self.size[k] = 0
        return k

    def rect(self, k, y0, x0, h, w, val, overlap=0):
        """h x w pixels of shape k; overlap: pixels of it the shape already had (a corner shared with the previous leg)."""
        assert 0 <= y0 and y0 + h <= self.H and 0 <= x0 and x0 + w <= self.W and h > 0 and w > 0, (y0, x0, h, w, self.H, self.W)
        own = self.ids[y0:y0 + h, x0:x0 + w]
        assert ((own == 0) | (own == k)).all(), "shapes must not be drawn over each other"
        assert int((own == k).sum()) == overlap
        self.img[y0:y0 + h, x0:x0 + w] = val
        own[...] = k
        self.size[k] += h * w - overlap

    def flipped(self):
        c = Canvas(self.H, self.W)
        c.img, c.ids, c.size = self.img[::-1].copy(), self.ids[::-1].copy(), dict(self.size)
        return c


def _spk_case(name, canvases, max_size, max_diff=SPK_DIFF, promises=None, one_sided=None):
    """keep: the closed form, a shape survives iff its arithmetic size exceeds max_size. one_sided: the case keeps everything or
    erases everything on purpose. promises: counts the CPU test verifies on the first map."""
    if isinstance(canvases, Canvas):
        canvases = [canvases]
    maps = np.stack([c.img for c in canvases])
    ids = np.stack([c.ids for c in canvases])
    keep = np.zeros(maps.shape, bool)
    for i, c in enumerate(canvases):
        big = np.array([False] + [c.size[k] > max_size for k in sorted(c.size)])
        keep[i] = big[c.ids]
    every = [s for c in canvases for s in c.size.values()]
    derived = not (any(s > max_size for s in every) and any(s <= max_size for s in every))
    assert one_sided is None or one_sided == derived, name
    one_sided = derived
    return dict(name=name, maps=maps, ids=ids, sizes=[dict(c.size) for c in canvases], keep=keep, max_size=int(max_size),
                max_diff=int(max_diff), newval=SPK_NEWVAL, promises=promises or {}, one_sided=one_sided)


def spk_expected(case):
    return np.where(case["keep"], case["maps"], np.int16(case["newval"])).astype(np.int16)


def stripes_canvas(H, W, dead_rows=0):
    """One-pixel vertical stripes of two values more than max_diff apart over the first H - dead_rows rows: W runs per row, W
    contacts per seam, every stripe a component of exactly H - dead_rows pixels."""
    c = Canvas(H, W)
    for x in range(W):
        c.rect(c.new(), 0, x, H - dead_rows, 1, VAL_A if x % 2 == 0 else VAL_B)
    return c


def stripes(H, W, keep, dead_rows=0):
    hs = H - dead_rows
    return _spk_case(f"stripes_{H}x{W}_{'keep' if keep else 'erase'}" + (f"_dead{dead_rows}" if dead_rows else ""),
                     stripes_canvas(H, W, dead_rows), hs - 1 if keep else hs, one_sided=True,
                     promises=dict(runs_per_row=W, contacts_per_seam=W, component_size=hs, components=W))


def snake_canvas(H, W, size):
    """A one-pixel serpentine: full rows 0, 2, 4, ... joined alternately at the right and the left end, the last row cut to
    reach `size` exactly: (r - 1) * (W + 1) + L pixels with r rows and L pixels of the last one. The rest of the connector rows
    holds the other value: stretches of W - 1 pixels that belong to nothing else."""
    c = Canvas(H, W)
    full = min((size - 1) // (W + 1), (H + 1) // 2 - 1)
    L = size - full * (W + 1)
    assert 1 <= L <= W, (H, W, size)
    k = c.new()
    for r in range(full):
        right = r % 2 == 0
        c.rect(k, 2 * r, 0, 1, W, VAL_A)
        c.rect(k, 2 * r + 1, W - 1 if right else 0, 1, 1, VAL_A)
        c.rect(c.new(), 2 * r + 1, 0 if right else 1, 1, W - 1, VAL_B)
    if full % 2 == 0:
        c.rect(k, 2 * full, 0, 1, L, VAL_A)          # entered from the left end (or it is the first row)
    else:
        c.rect(k, 2 * full, W - L, 1, L, VAL_A)      # entered from the right end
    assert c.size[k] == size
    return c


def snake(H, W, max_size, size):
    return _spk_case(f"snake_{H}x{W}_max{max_size}_size{size}", snake_canvas(H, W, size), max_size, promises=dict(component_size=size))


def comb_canvas(H, W, x0, bw, bh, flip=False, pitch=3):
    """A back of bh x bw pixels on the first rows with one-pixel teeth every `pitch` columns down to the last row, each tip with a
    one-pixel serif to its right: one component of bh * bw + teeth * (H - bh + 1) pixels. Beside it, free-standing teeth of the
    same shape that hang on nothing: H - bh + 1 pixels each. flip: upside down."""
    c = Canvas(H, W)
    k = c.new()
    c.rect(k, 0, x0, bh, bw, VAL_A)
    tl = H - bh
    teeth = 0
    for x in range(x0, x0 + bw - 1, pitch):
        c.rect(k, bh, x, tl, 1, VAL_A)
        c.rect(k, H - 1, x + 1, 1, 1, VAL_A)
        teeth += 1
    assert c.size[k] == bh * bw + teeth * (tl + 1)
    x = x0 + bw + 1
    while x + 2 <= min(W, x0 + bw + 1 + 8 * pitch):   # up to eight loose teeth
        f = c.new()
        c.rect(f, bh, x, tl, 1, VAL_A)
        c.rect(f, H - 1, x + 1, 1, 1, VAL_A)
        x += pitch
    return c.flipped() if flip else c


def comb(H, W, x0, bw, bh, max_size, flip=False, tag="comb"):
    """max_size <= 0: that much below the size of the whole comb (0: exactly the whole)"""
    c = comb_canvas(H, W, x0, bw, bh, flip)
    whole = c.size[1]
    rel = {0: "exact", -1: "minus1"}.get(max_size, f"max{max_size}")
    return _spk_case(f"{tag}_{H}x{W}_x{x0}_back{bh}x{bw}_{rel}{'_flipped' if flip else ''}", c, max_size if max_size > 0 else whole + max_size,
                     promises=dict(component_size=whole, loose=H - bh + 1))


def spiral_canvas(H, W):
    """A square spiral, corridors and gaps one pixel wide: legs right, down, left, up, ... each starting on the last pixel of the
    one before: sum of the legs - (legs - 1) pixels."""
    c = Canvas(H, W)
    k = c.new()
    top, left, bottom, right = 0, 0, H - 1, W - 1
    y, x = 0, 0
    legs, total = 0, 0
    direction = 0
    while True:
        if direction == 0:
            n = right - x + 1
            if n < 2 and legs: break
            c.rect(k, y, x, 1, n, VAL_A, overlap=1 if legs else 0); x = right; top += 2
        elif direction == 1:
            n = bottom - y + 1
            if n < 2: break
            c.rect(k, y, x, n, 1, VAL_A, overlap=1); y = bottom; right -= 2
        elif direction == 2:
            n = x - left + 1
            if n < 2: break
            c.rect(k, y, left, 1, n, VAL_A, overlap=1); x = left; bottom -= 2
        else:
            n = y - top + 1
            if n < 2: break
            c.rect(k, top, x, n, 1, VAL_A, overlap=1); y = top; left += 2
        total += n
        legs += 1
        direction = (direction + 1) % 4
    assert c.size[k] == total - (legs - 1)
    return c


def nested_u_canvas(H, W, count):
    """U shapes inside each other, one-pixel bars and gaps: U number j has its bars in columns 2j and W - 1 - 2j from row 0 down to
    its bottom in row H - 1 - 2j: 2 * (H - 2j) + (W - 4j) - 2 pixels. The bars of one U are separate pieces above its bottom row."""
    c = Canvas(H, W)
    for j in range(count):
        k = c.new()
        hh, ww = H - 2 * j, W - 4 * j
        assert hh >= 2 and ww >= 3
        c.rect(k, 0, 2 * j, hh, 1, VAL_A)
        c.rect(k, 0, W - 1 - 2 * j, hh, 1, VAL_A)
        c.rect(k, hh - 1, 2 * j + 1, 1, ww - 2, VAL_A)
        assert c.size[k] == 2 * hh + ww - 2
    return c


def seg_boundaries(W):
    """Columns c such that c - 1 | c is a boundary the band walk knows: the chunk pairs 63|64 and 255|256 and the first column of
    every segment but the first for 2 and 4 segments (SW = 64 * ceil(chunks / S))."""
    chunks = (W + 63) // 64
    cols = {64, 256}
    for S in (2, 4):
        if chunks >= S:
            sw = 64 * ((chunks + S - 1) // S)
            cols |= {k * sw for k in range(1, S)}
    return sorted(c for c in cols if 2 <= c <= W - 2)


def islands_canvas(H, W, max_size):
    """Islands of max_size - 1, max_size and max_size + 1 pixels, four columns wide and filled row by row (the last row from the
    left): in the four corners, and across every column of seg_boundaries(W) at rows 0, 5, 10, ... -- every row offset mod 4 where the map
    is tall enough."""
    c = Canvas(H, W)
    busy = np.zeros((H + 2, W + 2), bool)   # shapes and a one-pixel moat around them
    rows_of = lambda s: (s + 3) // 4
    turn = [0]

    def place(y0, x0, from_bottom=False):
        s = max_size - 1 + turn[0] % 3
        h = rows_of(s)
        if from_bottom:
            y0 = H - h
        if y0 < 0 or y0 + h > H or x0 < 0 or x0 + 4 > W or busy[y0:y0 + h + 2, x0:x0 + 6].any():
            return
        k = c.new()
        for r in range(h):
            c.rect(k, y0 + r, x0, 1, min(4, s - 4 * r), VAL_A)
        assert c.size[k] == s
        busy[y0:y0 + h + 2, x0:x0 + 6] = True
        turn[0] += 1

    place(0, 0); place(0, W - 4); place(0, 0, True); place(0, W - 4, True)
    for col in seg_boundaries(W):
        for y0 in range(0, H, 5):
            place(y0, col - 2)
    return c


def ramp_canvas(H, W, step):
    """value(y, x) = step * tri(x + y), tri a triangle wave of slope +-1 between 0 and P: every horizontal and every vertical
    neighbour pair differs by exactly `step`. One shape per pixel (the caller says whether they join)."""
    c = Canvas(H, W)
    P = max(1, min(1008 // max(step, 1), 60))
    yy, xx = np.mgrid[0:H, 0:W]
    c.img[...] = (step * (P - np.abs((xx + yy) % (2 * P) - P))).astype(np.int16)
    return c


def ramp(H, W, step, speckle_range, max_size):
    """step <= min(speckle_range, 1 << 17): the whole map is one component of H * W pixels; else one component per pixel."""
    c = ramp_canvas(H, W, step)
    joins = step <= speckle_range
    keep = np.full((1, H, W), (H * W if joins else 1) > max_size)
    return dict(name=f"ramp_{H}x{W}_step{step}_range{speckle_range}_max{max_size}", maps=c.img[None], ids=None, sizes=None, keep=keep,
                max_size=max_size, max_diff=speckle_range, newval=SPK_NEWVAL, one_sided=True,
                promises=dict(neighbour_step=step, components=1 if joins else H * W))


def beside_invalid_canvas(H, W, max_size):
    """Valid pixels of value newval + 16 beside filtered ones (they must not join them, whatever max_diff), as two blocks of at
    most max_size pixels with one filtered column between them; a checkerboard of valid and filtered pixels (diagonal neighbours
    never join); and a solid block of more than max_size pixels."""
    c = Canvas(H, W)
    v = SPK_NEWVAL + 16
    bw = max(1, min(max_size // H, 8))
    c.rect(c.new(), 0, 0, H, bw, v)
    c.rect(c.new(), 0, bw + 1, H, bw, v)
    x0 = 2 * bw + 3
    x1 = W - (max_size // H + 2) - 1
    for y in range(H):
        for x in range(x0 + (y % 2), x1, 2):
            c.rect(c.new(), y, x, 1, 1, v)
    c.rect(c.new(), 0, x1 + 1, H, W - x1 - 1, v)
    return c


def constant_canvas(H, W, val=VAL_A):
    c = Canvas(H, W)
    c.rect(c.new(), 0, 0, H, W, val)
    return c


def fuzz(seed, H, W):
    """The few-level, median-filtered maps with 25 % holes of test_filter_speckles_is_plain_connected_components: no closed form."""
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    img = (rng.integers(0, 6, (H, W)) * 40).astype(np.int16)
    img = ndimage.median_filter(img, 3).astype(np.int16)
    img[rng.random((H, W)) < 0.25] = SPK_NEWVAL
    ms, md = ((5, 0), (20, 40), (12, 32), (1, 100))[seed % 4]
    return dict(name=f"fuzz_{seed}_{H}x{W}_max{ms}_diff{md}", maps=img[None], ids=None, sizes=None, keep=None, max_size=ms, max_diff=md,
                newval=SPK_NEWVAL, one_sided=False, promises={})


def speckle_cases():
    cs = []
    # stripes: flush of the contact list, seam slots and records beyond the dense ones, the LDS run table's overflow (more than 128
    # / 256 runs per row of a segment needs W >= 257 at four rows per band and one segment, 1100 for every other variant), with
    # all-filtered rows whose bands do not overflow in the same workgroup
    for H, W, dead in ((5, 64, 0), (9, 65, 0), (10, 130, 0), (9, 256, 0), (11, 257, 0), (18, 320, 4), (10, 1100, 0), (18, 1100, 5)):
        cs += [stripes(H, W, True, dead), stripes(H, W, False, dead)]
    # snake: one long union chain; sizes at max_size and max_size + 1; the band walk's limit of 2048 and the first size beyond it
    cs += [snake(9, 65, 100, 100), snake(9, 65, 100, 101), snake(11, 130, 300, 300), snake(11, 130, 300, 301)]
    for H, W in ((5, 1100), (18, 257)):
        cs += [snake(H, W, 2048, 2048), snake(H, W, 2048, 2049), snake(H, W, 2049, 2049), snake(H, W, 2049, 2050)]
    # combs: the "touches something large" mark travels down (upright) and up (flipped) across at least three further seams
    for flip in (False, True):
        cs += [comb(18, 130, 40, 60, 4, 50, flip), comb(11, 65, 1, 55, 2, 40, flip), comb(18, 320, 100, 100, 4, 150, flip),
               comb(18, 1100, 280, 90, 4, 100, flip),
               # a back one row thin: 30 + 10 * 18 = 210 pixels, the piece inside the back's band at most 30 + 10 * 3
               comb(18, 130, 50, 30, 1, 100, flip, tag="thincomb"),
               comb(18, 130, 50, 30, 1, 0, flip, tag="thincomb"),       # the whole is exactly max_size
               comb(18, 130, 50, 30, 1, -1, flip, tag="thincomb")]
    # spirals and nested U shapes: pieces that are separate in the upper bands and join in the last one
    for H, W in ((9, 65), (18, 130), (11, 257)):
        c = spiral_canvas(H, W)
        s = c.size[1]
        cs += [_spk_case(f"spiral_{H}x{W}_erase", c, min(s, 2048), one_sided=True, promises=dict(component_size=s))]
        if s - 1 <= 2048:
            cs += [_spk_case(f"spiral_{H}x{W}_keep", c, s - 1, one_sided=True, promises=dict(component_size=s))]
    for H, W, count in ((10, 64, 4), (18, 130, 8), (9, 320, 4)):
        c = nested_u_canvas(H, W, count)
        mid = c.size[count // 2]          # U number count // 2 - 1 ... the outer ones are larger: kept; this one and the inner ones go
        cs += [_spk_case(f"nested_u_{H}x{W}", c, mid, promises=dict(components=count))]
    # islands at max_size - 1, max_size, max_size + 1 on every boundary the walk knows
    for H, W, ms in ((18, 320, 9), (18, 1100, 9), (18, 256, 9), (10, 257, 6), (5, 130, 5), (18, 320, 10), (18, 1100, 11)):
        cs += [_spk_case(f"islands_{H}x{W}_max{ms}", islands_canvas(H, W, ms), ms, promises=dict(sizes={ms - 1, ms, ms + 1}))]
    # ramps: neighbours exactly max_diff apart join, max_diff + 1 apart do not; max_diff 0; a range beyond the 1 << 17 clamp
    for H, W in ((9, 130), (10, 257)):
        cs += [ramp(H, W, 32, 32, 100), ramp(H, W, 33, 32, 1), ramp(H, W, 0, 0, 100), ramp(H, W, 1, 0, 1),
               ramp(H, W, 16, 200000, 100), ramp(H, W, 1, 200000, 100)]
    # valid beside filtered, checkerboard
    for H, W, ms, md in ((9, 65, 30, 16), (10, 130, 40, 1000), (11, 320, 50, 200000)):
        cs += [_spk_case(f"beside_invalid_{H}x{W}_diff{md}", beside_invalid_canvas(H, W, ms), ms, md)]
    # degenerate maps
    cs += [_spk_case("all_filtered_9x130", Canvas(9, 130), 50, one_sided=True),
           _spk_case("constant_5x64_kept", constant_canvas(5, 64), 319, one_sided=True),
           _spk_case("constant_5x64_erased", constant_canvas(5, 64), 320, one_sided=True),
           _spk_case("constant_18x1100_kept", constant_canvas(18, 1100), 2048, one_sided=True)]
    # batches of three different maps, one of them all filtered: plane offsets
    cs += [_spk_case("batch_18x320", [comb_canvas(18, 320, 100, 100, 4), Canvas(18, 320), islands_canvas(18, 320, 9)], 9),
           _spk_case("batch_11x257", [stripes_canvas(11, 257), Canvas(11, 257), spiral_canvas(11, 257)], 11),
           _spk_case("batch_9x1100", [Canvas(9, 1100), stripes_canvas(9, 1100, 2), islands_canvas(9, 1100, 7)], 7)]
    cs += [fuzz(0, 18, 130), fuzz(1, 11, 257), fuzz(2, 10, 320), fuzz(3, 9, 65), fuzz(5, 18, 1100)]
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), names
    return cs


# the cases whose size sums or seam unions race, and the pair of the stale-scratch test
RACE_CASES = ("stripes_18x1100_erase_dead5", "stripes_11x257_keep", "snake_18x257_max2048_size2048", "snake_18x257_max2048_size2049",
              "thincomb_18x130_x50_back1x30_minus1", "thincomb_18x130_x50_back1x30_exact_flipped")
STALE_PAIR = ("stripes_18x1100_erase_dead5", "islands_18x1100_max9")

# ---- LR cases ------------------------------------------------------------------------------------------------------------------
LR_H, LR_BLOCK = 6, 5    # the smallest map a 5 x 5 block fits: rows 2 and 3 are matched, the others are filled


class LrRow:
    """One row under construction. Gadgets put pixels and say which of them survive; every gadget owns the right-view columns its
    pixels claim or look at, and no two gadgets may own the same one, so each gadget's verdict holds whatever else is in the row."""

    def __init__(self, W, mind, nd, d12):
        self.W, self.mind, self.nd, self.d12 = W, mind, nd, d12
        self.inv = (mind - 1) * 16
        self.minX1, self.maxX1 = max(mind + nd, 0), W + min(mind, 0)
        self.d = np.full(W, self.inv, np.int64)
        self.c = np.zeros(W, np.int64)
        self.keep = np.zeros(W, bool)
        self.owned = {}
        self.gadget = 0

    def begin(self):
        self.gadget += 1

    def put(self, x, d, cost, keep, checked=True):
        assert 0 <= x < self.W and self.d[x] == self.inv, (x, self.W)
        assert self.mind * 16 <= d <= (self.mind + self.nd - 1) * 16, (d, self.mind, self.nd)
        assert (self.minX1 <= x < self.maxX1) == checked, (x, self.minX1, self.maxX1)
        self.d[x], self.c[x], self.keep[x] = d, cost, keep
        for t in {x - ((d + 8) >> 4), x - (d >> 4), x - ((d + 15) >> 4)}:
            assert self.owned.setdefault(t, self.gadget) == self.gadget, ("two gadgets share right-view column", t)

    def fits(self, xs, ds):
        """whether pixels at xs with disparities ds could be put: inside the checked columns, in range, targets not owned"""
        for x, d in zip(xs, ds):
            if not (self.minX1 <= x < self.maxX1) or self.d[x] != self.inv:
                return False
            if not (self.mind * 16 <= d <= (self.mind + self.nd - 1) * 16):
                return False
            if any(t in self.owned for t in (x - ((d + 8) >> 4), x - (d >> 4), x - ((d + 15) >> 4))):
                return False
        return True


def fan(row, t, k0, count, costs):
    """count pixels x = t + k, k = k0 .. k0 + count - 1, with d = 16 * k: all claim column t and all look at nothing else. The
    winner is the cheapest, then the lowest x; the survivors are whoever is within the tolerance of it."""
    ks = [k0 + i for i in range(count)]
    if not row.fits([t + k for k in ks], [16 * k for k in ks]):
        return False
    row.begin()
    win = min(range(count), key=lambda i: (costs[i], ks[i]))
    for i, k in enumerate(ks):
        row.put(t + k, 16 * k, costs[i], abs(16 * k - 16 * ks[win]) <= 16 * row.d12)
    return True


def subpixel(row, x, k, f, claim_a, claim_b):
    """P at x with d = 16 k + f. f != 0: it looks at column x - k (floor) and x - k - 1 (ceil); f == 0: at x - k alone. claim_a /
    claim_b: a cheaper pixel whose disparity is more than the tolerance away takes that column. P dies iff every column it looks at
    went to such a pixel."""
    oa = row.d12 + 2
    xs, ds = [x], [16 * k + f]
    if claim_a:
        xs.append(x + oa); ds.append(16 * (k + oa))              # claims x + oa - (k + oa) = x - k
    if claim_b and f:
        xs.append(x + oa + 1); ds.append(16 * (k + oa + 2))      # claims x + oa + 1 - (k + oa + 2) = x - k - 1
    if not row.fits(xs, ds):
        return False
    row.begin()
    dies = (claim_a and claim_b) if f else claim_a
    row.put(xs[0], ds[0], 10, not dies)
    for xq, dq in zip(xs[1:], ds[1:]):
        row.put(xq, dq, 5, True)
    return True


def tolerance_edge(row, x, k, sign, over):
    """P at x with d = 16 k and a cheaper Q that claims P's column x - k from d12 columns further on (sign +1) or back (-1), its
    disparity exactly disp12MaxDiff * 16 away (over = 0: P survives) or one more (over = 1: P dies). With disp12MaxDiff = 0 there is
    no second pixel at distance 0 or 1: Q sits one column on at the smallest distance there is, 8, and P dies."""
    tol = 16 * row.d12
    if row.d12 == 0:
        xq, dq, dies = x + 1, 16 * k + 8, True
    else:
        xq, dq, dies = x + sign * row.d12, 16 * k + sign * (tol + over), bool(over)
    if not row.fits([x, xq], [16 * k, dq]):
        return False
    assert xq - ((dq + 8) >> 4) == x - k
    row.begin()
    row.put(x, 16 * k, 7, not dies)
    row.put(xq, dq, 3, True)
    return True


def range_edges(row):
    """Valid pixels in the columns just outside [minX1, maxX1) are kept and neither claim nor check: U, outside, would take the column
    of V, inside, if it claimed (it is cheaper and far away), and looks at a column whose owner disagrees with it. Pixels at minX1 and
    maxX1 - 1 claim and check like any other: a cheap winner there, and the lowest and highest columns a claim can land on."""
    mind, nd = row.mind, row.nd
    dmax, dmin = mind + nd - 1, mind
    far = row.d12 + 2          # columns between U and V: their disparities are 16 * (far + 1) apart, beyond the tolerance
    # the lowest column a claim can land on (x >= minDisparity + numDisparities, d <= 16 * dmax: column 1; column 0 is out of
    # every claim's reach) and the highest (W - 1), claimed from minX1 and from maxX1 - 1
    row.begin()
    row.put(row.minX1, 16 * dmax, 9, True)
    row.begin()
    row.put(row.maxX1 - 1, 16 * dmin, 9, True)
    if far + 1 > nd - 1:
        return
    # left: V at minX1 + far and U at minX1 - 1 aim at the same column
    if row.minX1 - 1 >= 0:
        row.begin()
        t = row.minX1 + far - dmax
        row.put(row.minX1 + far, 16 * dmax, 9, True)
        row.put(row.minX1 - 1, 16 * (row.minX1 - 1 - t), 1, True, checked=False)
    # right: V at maxX1 - 1 - far and U at maxX1 (there is one where minDisparity < 0) aim at the same column
    if row.maxX1 < row.W:
        row.begin()
        t = row.maxX1 - 1 - far - dmin
        row.put(row.maxX1 - 1 - far, 16 * dmin, 9, True)
        row.put(row.maxX1, 16 * (row.maxX1 - t), 1, True, checked=False)


def _spread(row, count):
    """count anchor columns over the checked range, left edge, right edge and inner wavefronts alike"""
    lo, hi = row.minX1 + 1, row.maxX1 - 2
    return sorted({lo + (hi - lo) * i // max(count - 1, 1) for i in range(count)})


def lr_rows(W, mind, nd, d12, cost_hi=65534, seed=0):
    """The designed rows of one (W, minDisparity, numDisparities, disp12MaxDiff): each a dict(d, c, keep, designed) where designed
    says whether keep is a closed form (random rows have none)."""
    rows = []
    dmin, dmax = mind, mind + nd - 1
    span = min(nd, 12)

    def new():
        return LrRow(W, mind, nd, d12)

    def done(r, name):
        rows.append(dict(name=name, d=r.d.astype(np.int16), c=r.c.astype(np.int32), keep=r.keep.copy(), designed=True,
                         gadgets=r.gadget))

    # fans: the cost variants, each at several places of the row
    k0 = max(dmin, dmax - span + 1)
    variants = {
        "unique_min": lambda n, j: [20 + (i * 7) % 11 if i != j % n else 2 for i in range(n)],
        "tie_on_min": lambda n, j: [4 if i in ((j + 1) % n, (j + n // 2 + 1) % n) else 9 + i for i in range(n)],
        "all_equal": lambda n, j: [6] * n,
        "top_of_16_bits": lambda n, j: [cost_hi if i != (j + 2) % n else cost_hi - 1 for i in range(n)],
    }
    for vname, costs in variants.items():
        r = new()
        for j, t in enumerate(_spread(r, 9)):
            fan(r, t - k0, k0, span, costs(span, j))
        done(r, "fans_" + vname)
    # sub-pixel targets
    r = new()
    combos = [(f, a, b) for f in (1, 7, 8, 15) for a in (0, 1) for b in (0, 1)] + [(0, 0, 0), (0, 1, 0)]
    anchors = _spread(r, 4 * len(combos))
    kk = dmin + 1
    i = 0
    for x in anchors:
        f, a, b = combos[i % len(combos)]
        if kk + d12 + 4 <= dmax and subpixel(r, x, kk, f, a, b):
            i += 1
    done(r, "subpixel_targets")
    # tolerance edges, both signs
    r = new()
    combos = [(s, o) for s in (1, -1) for o in (0, 1)]
    i = 0
    for x in _spread(r, 24):
        s, o = combos[i % 4]
        k = dmin + 1 if s > 0 else dmax - 1
        if tolerance_edge(r, x, k, s, o):
            i += 1
    done(r, "tolerance_edges")
    # range edges
    r = new()
    range_edges(r)
    done(r, "range_edges")
    # tie-heavy random rows: costs 0 to 5, 30 % holes
    rng = np.random.default_rng(1000 * W + 10 * (mind + 50) + d12 + seed)
    for j in range(2):
        d = (rng.integers(0, (nd - 1) * 16 + 1, W) + mind * 16).astype(np.int16)
        d[rng.random(W) < 0.3] = (mind - 1) * 16
        rows.append(dict(name=f"random_{j}", d=d, c=rng.integers(0, 6, W).astype(np.int32), keep=None, designed=False, gadgets=0))
    return rows


def lr_case(W, mind, nd, d12, cost_hi=65534, tag=""):
    """The rows packed two per map into rows 2 and 3 of LR_H-row maps; the rows the matcher never computes hold copies of other
    designed rows (the device must overwrite them)."""
    rows = lr_rows(W, mind, nd, d12, cost_hi)
    n = (len(rows) + 1) // 2
    inv = (mind - 1) * 16
    pre = np.full((n, LR_H, W), inv, np.int16)
    cost = np.zeros((n, LR_H, W), np.int32)
    where = []
    for i, r in enumerate(rows):
        m, y = i // 2, 2 + i % 2
        pre[m, y], cost[m, y] = r["d"], r["c"]
        where.append((m, y))
        for yy in ((0, 4) if y == 2 else (1, 5)):
            pre[m, yy], cost[m, yy] = r["d"], r["c"]
    return dict(name=f"lr_W{W}_min{mind}_nd{nd}_d12_{d12}{tag}", W=W, mind=mind, nd=nd, d12=d12, rows=rows, where=where, pre=pre, cost=cost,
                cost_hi=cost_hi)


def lr_row_expected(r, mind):
    return np.where(r["keep"], r["d"], np.int16((mind - 1) * 16)).astype(np.int16)


def lr_device_expected(validate, case, info, block=LR_BLOCK):
    """What stage 1 of the entry must return, given a validate(disp, cost, mind, nd, d12) for whole rows: the columns the matcher
    never computes read as filtered, the check runs on the matched rows, and everything outside the valid ROI is filled."""
    pre, cost = case["pre"], case["cost"]
    inv = np.int16((case["mind"] - 1) * 16)
    out = np.full_like(pre, inv)
    r0, r1, c0, c1, lofs, xend = (info[k] for k in ("row0", "row1", "col0", "col1", "lofs", "xend"))
    for m in range(pre.shape[0]):
        live = pre[m, r0:r1].copy()
        live[:, :lofs] = inv
        live[:, lofs + xend:] = inv
        v = validate(live, cost[m, r0:r1], case["mind"], case["nd"], case["d12"])
        out[m, r0:r1, c0:c1] = v[:, c0:c1]
    return out


# (W, what launch_lrcheck picks on a 16-bit cost plane): every lrcheck16 instantiation and every remainder mod 2 and mod 4
LR_FAST_WIDTHS = [(100, (1, 2)), (127, (1, 2)), (128, (1, 2)), (129, (2, 2)), (255, (2, 2)), (383, (3, 2)), (386, (4, 2)), (640, (5, 2)),
                  (641, (3, 2)), (1023, (4, 2)), (1280, (5, 2)), (1281, (2, 4)), (2050, (3, 4)), (3075, (4, 4)), (4096, (4, 4))]
LR_PARAMS = [(0, 16, 1), (-8, 16, 0), (5, 32, 2), (0, 128, 64)]   # (minDisparity, numDisparities, disp12MaxDiff)


def lr_cases_fast():
    cs = []
    for i, (W, _) in enumerate(LR_FAST_WIDTHS):
        combos = LR_PARAMS if W in (386, 1281) else [LR_PARAMS[i % len(LR_PARAMS)]]
        for mind, nd, d12 in combos:
            cs.append(lr_case(W, *((mind, nd, d12) if W > nd + 100 else LR_PARAMS[0])))
    # at and beyond the 16384 clamp of the 16-bit verdict: everything passes (512 disparities are the most the 16-bit plane sees)
    cs += [lr_case(1100, 0, 512, 1024), lr_case(1100, 0, 512, 1025)]
    return cs


def lr_cases_generic():
    """Rows the generic kernel takes whatever the cost plane: 4097 (keys in LDS), 8193 (keys in global memory), and 1008 disparities
    (outside the interior SAD kernel's envelope, so the plane is int32) with tolerances around 16384."""
    return [lr_case(4097, -8, 16, 0), lr_case(8193, 5, 32, 2), lr_case(1100, 0, 1008, 1023), lr_case(1100, 0, 1008, 1025)]


def lr_cases_int32():
    """Costs beyond 16 bits, for the int32 plane alone."""
    return [lr_case(4097, 0, 16, 1, cost_hi=(1 << 31) - 2, tag="_big"), lr_case(8193, 0, 16, 1, cost_hi=(1 << 30) + 5, tag="_big"),
            lr_case(386, -8, 16, 0, cost_hi=(1 << 31) - 2, tag="_big")]
