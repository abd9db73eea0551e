"""The grid-stride loops of the voxel tools, and the cases that take each of them round again (tests/test_loop_passes.py on the CPU,
tests/test_loop_passes_gpu.py on the device).  Every kernel of the tools is launched under one of two rules of csrc/vr_api_tools.h:
tool_blocks(n), persistent, one wavefront per word / unit / item and `u += W` with W = 4 x blocks <= WORDS_PER_PASS; lane_blocks(n), one
lane per element and `i += stride` with stride <= LANE_CAP.  Below LANE_CAP a lane's loop body runs at most once; below WORDS_PER_PASS
the persistent rule launches n / 4 workgroups, so only the n % 4 words beyond 4 x (n / 4) send a wavefront round again (which is how
the tools' own tests notice an accumulator that is reset per pass, in at most three words).  What a pass hands to the next -- an
accumulator, the advanced index, a uniform trip count around a ballot -- is exercised in earnest only by the cases here.

ROWS is the inventory: one row per loop that `for \\(.*\\+= ?(W|stride)` finds in the nine tool headers and in vr_comp.h, with what the
loop carries and why a collective inside it is safe, both read from the code.  CHANNEL_ROWS, at the end, is the same for the ten loops
of the channel tools (vr_filter.h, vr_rank.h, vr_gamma.h), all launched with lane_blocks.  Harness only; the thresholds are
comp_cases'."""
import numpy as np

import raster_cases as rc
from comp_cases import LANE_CAP, SCAN_TILE, SPINE_CHUNK, TOOL_BLOCKS, WORDS_PER_PASS  # noqa: F401  (not restated here)

f32 = np.float32
HEADERS = ["vr_bitrows.h", "vr_morph.h", "vr_dist.h", "vr_raster.h", "vr_outline.h", "vr_mesh.h", "vr_hist.h", "vr_grow.h", "vr_resample.h"]
LOOP = r"for \(.*\+= ?(W|stride)"


# ---- the launch rules ----------------------------------------------------------------------------------------------------------------

def tool_blocks(n):
    return 1 if n < 4 else min(n // 4, TOOL_BLOCKS)


def lane_blocks(n):
    return min((n + 255) // 256, 4 * TOOL_BLOCKS)


def passes(rule, n):
    """(the passes of the busiest wavefront or lane, the elements of the last pass, the elements per pass) of a loop over n elements."""
    per = 4 * tool_blocks(n) if rule == "tool" else 256 * lane_blocks(n)
    return -(-n // per), n - (-(-n // per) - 1) * per, per


def box_words(box_lo, box_hi):
    return ((box_hi[0] + 63) // 64 - box_lo[0] // 64) * (box_hi[1] - box_lo[1]) * (box_hi[2] - box_lo[2])


def box_units(box_lo, box_hi):
    return int(np.prod([(h + 3) // 4 - l // 4 for l, h in zip(box_lo, box_hi)]))


def word_index(shape, box_lo, box_hi):
    """Per voxel of the (nz, ny, nx) volume: the box word it lies in, as the walk numbers them (bit_box_word: words, rows, slices), -1
    outside the box."""
    nz, ny, nx = shape
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    bw0, bw = x0 // 64, (x1 + 63) // 64 - x0 // 64
    z, y, x = np.indices(shape)
    u = ((z - z0) * (y1 - y0) + (y - y0)) * bw + (x // 64 - bw0)
    inside = (x >= x0) & (x < x1) & (y >= y0) & (y < y1) & (z >= z0) & (z < z1)
    return np.where(inside, u, -1)


def unit_index(shape, box_lo, box_hi):
    """Per voxel: the 4 x 4 x 4 unit of the box it lies in, as brick_unit numbers them (x fastest), -1 outside the box."""
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    un = [(h + 3) // 4 - l // 4 for l, h in zip(box_lo, box_hi)]
    z, y, x = np.indices(shape)
    u = ((z // 4 - z0 // 4) * un[1] + (y // 4 - y0 // 4)) * un[0] + (x // 4 - x0 // 4)
    inside = (x >= x0) & (x < x1) & (y >= y0) & (y < y1) & (z >= z0) & (z < z1)
    return np.where(inside, u, -1)


def later_density(a, index, per=WORDS_PER_PASS):
    """The density of the set `a` over the voxels whose word or unit is taken in the second or a later pass."""
    later = index >= per
    return float(a[later].mean()) if later.any() else 0.0


def seeded(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


# ---- persistent rule: boxes of words and of units ------------------------------------------------------------------------------------
# name -> (shape (nz, ny, nx), box_lo, box_hi); every box is off the volume's faces on at least one axis.  The restatements' times per
# call, on one CPU core: morph 0.01 s, the distance fields 0.06 s, raster 0.05 s, histogram 0.01 s, resample 0.05 s, grow
# 0.2 s (FACES) and 0.6 s (ALL: the voxel-by-voxel search visits 26 neighbours); nothing had to be cut.

WORD_BOXES = {
    "one_word": ((64, 65, 40), (1, 0, 0), (39, 65, 64)),        # 1 x 65 x 64 = 4160 words: two passes and 64 words
    "three_words": ((40, 37, 130), (2, 1, 0), (129, 37, 40)),   # 3 x 36 x 40 = 4320 words, the last of a row partial: two passes and 224
    "exact_words": ((243, 19, 40), (3, 1, 1), (40, 18, 242)),   # 1 x 17 x 241 = 4097 = 2 x WORDS_PER_PASS + 1: one wavefront's third pass
}
UNIT_BOXES = {
    "units": ((64, 64, 68), (1, 0, 0), (67, 64, 64)),           # 17 x 16 x 16 = 4352 units (and bricks): two passes and 256
    "exact_units": ((4, 964, 68), (1, 1, 0), (67, 963, 4)),     # 17 x 241 x 1 = 4097 units (and bricks)
}
DENSITY = 0.4


def word_case(name, seed=61):
    """(the set (nz, ny, nx) of density 0.4, box_lo, box_hi) of a box of words."""
    shape, lo, hi = WORD_BOXES[name]
    return seeded(shape, DENSITY, seed + len(name)), lo, hi


# ---- raster: more than WORDS_PER_PASS items ---------------------------------------------------------------------------------------------
ROWS_PER_ITEM = 8  # kRasterRowsPerItem (csrc/vr_api_raster.h): an item is a run of up to 8 rows of ONE polygon within the box


RASTER_PER_SLICE = {"one_word": 5, "three_words": 12}  # 64 and 40 slices: 320 and 480 polygons of 8 or 9 and 5 items each


def raster_polygons(name, grid=rc.GRIDS[1]):
    """Overlapping 11-gons on every slice of a box of words, each over most of the rows (the default form cuts a polygon's items to its
    rows, the plain form takes the box's), in contours 0 and 1 in turn: (points, polygons).  Items are numbered polygon by polygon, so
    the later passes take the later slices, as full as the first."""
    (nz, ny, nx), _, _ = WORD_BOXES[name]
    per_slice = RASTER_PER_SLICE[name]
    polys = []
    for z in range(nz):
        for k in range(per_slice):
            p = rc.ngon(11, nx * (0.2 + 0.6 * k / (per_slice - 1)) + z % 3, ny / 2 + (k % 5 - 2) * 0.7, nx * (0.15 + 0.03 * (k % 5)), ny * 0.49,
                        phase=0.1 * z + k)
            polys.append((rc.place(p, grid[1], grid[0]), z, k % 2))
    return rc.flatten(polys)


# Exactly 2 x WORDS_PER_PASS + 1 items: 17 polygons on each of 241 slices, in a box of seven rows, so that every polygon is one item in
# either form
RASTER_EXACT = ((241, 8, 40), (3, 1, 0), (40, 8, 241))


def raster_exact_polygons(grid=rc.GRIDS[1]):
    (nz, ny, nx), _, _ = RASTER_EXACT
    polys = []
    for z in range(nz):
        for k in range(17):
            p = rc.ngon(5 + k % 3, 4 + 2 * k + z % 2, 4 + (k % 2) * 0.5, 2.6 + 0.2 * (k % 4), 2.4, phase=0.3 * z + k)
            polys.append((rc.place(p, grid[1], grid[0]), z, k % 2))
    return rc.flatten(polys)


def raster_items(points, polygons, grid, box_lo, box_hi, plain):
    """The items of a vr_mask_polygons as raster_work (csrc/vr_api_raster.h) cuts them; per polygon the numbers of its first and last."""
    (sx, sy), (ox, oy) = grid
    n, spans = 0, []
    for first, count, z, _ in polygons:
        if not box_lo[2] <= z < box_hi[2]:
            spans.append(None)
            continue
        j0, j1 = box_lo[1], box_hi[1]
        if not plain:
            p = points[first:first + count].astype(np.int64)
            ceil_div = lambda a, b: -((-a) // b)
            s0, s1 = max(ceil_div(int(p[:, 0].min()) - ox, sx), box_lo[0]), min(ceil_div(int(p[:, 0].max()) - ox, sx), box_hi[0])
            j0, j1 = max(ceil_div(int(p[:, 1].min()) - oy, sy), box_lo[1]), min(ceil_div(int(p[:, 1].max()) - oy, sy), box_hi[1])
            if s0 >= s1 or j0 >= j1:
                spans.append(None)
                continue
        items = -(-(j1 - j0) // ROWS_PER_ITEM)
        spans.append((n, n + items))
        n += items
    return n, spans


# ---- units: grow, histogram, resample ----------------------------------------------------------------------------------------------------

GROW_QUANTILE = {6: 0.4, 26: 0.33}  # the density of Q: above the site-percolation thresholds (0.312, 0.098), so most of Q is reached
HOSTILE = np.array([np.nan, np.inf, -np.inf, -0.3, -0.0, -0.001, -1e-3 / 256, 1e30, -1e30, 3.0e9, 0.999999, 1.0, 15.99], f32)


def noise(shape, seed):
    """A vec4 volume, every channel different: .a in [0, 1) on a 1/4096 grid, a twentieth of all components hostile (NaN, infinities,
    negatives, -0, huge ones) -- the volume of the histogram's and the grow's own tests."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, 4096, size=shape + (4,)).astype(f32) / f32(4096.0)).astype(f32)
    v[..., 0] *= f32(16.0)
    v[..., 1] -= f32(0.5)
    k = rng.random(shape + (4,)) < 0.05
    v[k] = rng.choice(HOSTILE, size=int(k.sum()))
    return v


def grow_case(name, connectivity, seed=7):
    """(volume (nz, ny, nx, 4) with hostile values, lo, hi of the value window, 64 seeds from Q, box_lo, box_hi) of a box of units."""
    import grow_ref as gr
    shape, blo, bhi = UNIT_BOXES[name]
    v = noise(shape, seed)
    a = v[..., 3]
    hi = float(f32(np.quantile(a[np.isfinite(a)].astype(np.float64), GROW_QUANTILE[connectivity])))
    z, y, x = np.nonzero(gr.qualifies(a, -np.inf, hi, blo, bhi))
    pick = np.random.default_rng(3).choice(len(x), size=64, replace=False)
    return v, -float("inf"), hi, [(int(x[i]), int(y[i]), int(z[i])) for i in pick], blo, bhi


# The frontier form of grow_round_kernel walks the bricks QUEUED for a round, so its loop goes round only with more than
# WORDS_PER_PASS of them in ONE round, which no seeded noise in a box of 4352 bricks can be shown to give.  A lattice can: 128^3 voxels
# (32^3 bricks, 32 MiB a slot), Q = the three axis lines through every brick's first voxel (10 voxels a brick: the density rule of the
# other cases cannot hold here), FACES, 64 seeds on brick corners 8 bricks apart.  A brick reaches exactly its six face neighbours, each
# through one voxel, and a brick that no listed brick has reached yet has R = 0 and is queued by the first that does: round k + 1 lists at
# least the bricks at brick distance k from a seed, 64 disjoint octahedral shells of 4 k^2 + 2 bricks -- 64, 384, 1152 and, in round 4,
# 2432.  frontier_shells counts them from Q itself.  The voxel-by-voxel restatement takes 2 s for the 327 680 voxels of Q.
LATTICE_SHAPE = (128, 128, 128)
LATTICE_WINDOW = (0.5, 2.0)


def lattice_case():
    """(volume, seeds): .a is 1.0 on the lattice and +0.0 off it, the other channels zero."""
    v = np.zeros(LATTICE_SHAPE + (4,), f32)
    a = v[..., 3]
    a[::4, ::4, :] = 1.0
    a[::4, :, ::4] = 1.0
    a[:, ::4, ::4] = 1.0
    at = [16 + 32 * i for i in range(4)]  # brick 4 + 8 i
    return v, [(x, y, z) for z in at for y in at for x in at]


def frontier_shells(q, seeds, rounds):
    """Per round 1 .. rounds of the frontier form, FACES: the bricks first reached in it -- a lower bound of the round's queue, and the
    queue itself while no brick is reached twice.  Two face neighbours are joined where voxels of q touch across their face; every brick's
    own q is taken as connected (checked by the caller's shape of q)."""
    nz, ny, nx = (n // 4 for n in q.shape)
    reached = np.zeros((nz, ny, nx), bool)
    for x, y, z in seeds:
        reached[z // 4, y // 4, x // 4] = True
    joins = []  # per axis: brick b and its next along the axis touch through q
    for axis in range(3):
        t = np.moveaxis(q, axis, 0)
        touch = t[3:-1:4] & t[4::4]  # (bricks - 1, voxels, voxels) of the other two axes
        n, a, b = touch.shape
        joins.append(np.moveaxis(touch.reshape(n, a // 4, 4, b // 4, 4).any(axis=(2, 4)), 0, axis))
    counts, front = [int(reached.sum())], reached.copy()
    for _ in range(rounds - 1):
        new = np.zeros_like(reached)
        for axis in range(3):
            sl_lo = [slice(None)] * 3
            sl_hi = [slice(None)] * 3
            sl_lo[axis], sl_hi[axis] = slice(0, -1), slice(1, None)
            new[tuple(sl_hi)] |= front[tuple(sl_lo)] & joins[axis]
            new[tuple(sl_lo)] |= front[tuple(sl_hi)] & joins[axis]
        front = new & ~reached
        reached |= front
        counts.append(int(front.sum()))
    return counts


# a destination grid and the box written: 3 x 36 x 40 = 4320 units of 64 voxels with a tail (stride % ux = 2: the walk's carry from piece
# to row happens on most steps), and 1 x 17 x 241 = 4097 = 2 x WORDS_PER_PASS + 1
RESAMPLE_BOXES = {"three_pieces": ((40, 37, 130), (1, 1, 0), (130, 37, 40)), "exact_units": ((243, 19, 40), (3, 1, 1), (40, 18, 242))}


def resample_units(box_lo, box_hi):
    return ((box_hi[0] - box_lo[0] + 63) // 64) * (box_hi[1] - box_lo[1]) * (box_hi[2] - box_lo[2])


# ---- lane rule: the outlines ------------------------------------------------------------------------------------------------------------

# outline_ref.trace, on one CPU core: the vertex words 6.5 s (x is one voxel and cannot shrink; y and z are the smallest that pass
# LANE_CAP with y <= 65535), the checkerboard 0.3 s (SPLIT) and 0.5 s (JOIN), the fishbone 0.3 s
VWORDS_SHAPE = (9, 65535, 1)  # one vertex word a vertex row: 9 x 65535 rows of the box = 589 815 vertex words from 589 815 voxels
VWORDS_BOX = ((0, 1, 0), (1, 65535, 9))
BOARD_SHAPE = (1, 520, 520)   # a checkerboard: 2 x 519 x 519 + 2 x 2 x 519 + 4 = 540 800 nodes under either rule
FISH_SHAPE = (1, 600, 1021)


def vwords_members(seed=71):
    m = np.zeros((4,) + VWORDS_SHAPE, bool)
    m[0] = seeded(VWORDS_SHAPE, DENSITY, seed)
    return m


def board_members():
    m = np.zeros((4,) + BOARD_SHAPE, bool)
    m[0, 0] = (np.add.outer(np.arange(BOARD_SHAPE[1]), np.arange(BOARD_SHAPE[2])) & 1) == 0
    return m


def fishbone(ny=FISH_SHAPE[1], nx=FISH_SHAPE[2]):
    """One 4-connected set whose outline is ONE loop with about nx x ny corners: a spine along row 0, a rib on every fourth column, and
    one-voxel nubs on every other voxel of both sides of each rib (column 2 mod 4 stays empty: the nubs of two ribs never touch)."""
    s = np.zeros((ny, nx), bool)
    s[0, :] = True
    s[:, ::4] = True
    s[2::2, 1::4] = True
    s[2::2, 3::4] = True
    assert nx % 4 == 1  # (the last column is a rib: no nub hangs free)
    return s


def fishbone_members():
    m = np.zeros((4,) + FISH_SHAPE, bool)
    m[0, 0] = fishbone()
    return m


def member_counts(m, contours, box_lo, box_hi):
    """Per contour number: its members in the box (0 for a contour that is not traced)."""
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    return tuple(int(m[k, z0:z1, y0:y1, x0:x1].sum()) if (contours >> k) & 1 else 0 for k in range(4))


# ---- lane rule: the mesh count, and a reference for meshes whose content lies in bands of slices ----------------------------------------

# Boxes of lattice words for the persistent mesh kernels, cap 0: 1 x 65 x 64 = 4160 and 1 x 17 x 241 = 4097 words.  x is cut to two
# voxels (one cell a row): mesh_ref.extract is a Python loop over cells and takes a second for these 4032 and 3840.
MESH_BOXES = {"one_word": ((64, 66, 2), (0, 1, 0), (2, 66, 64)), "exact_words": ((241, 18, 2), (0, 1, 0), (2, 18, 241))}
MESH_LEVEL = 0.6  # of uniform noise in [0, 1): 0.4 of the voxels are inside


def mesh_values(name, seed=83):
    return np.random.default_rng(seed).random(MESH_BOXES[name][0]).astype(f32)


# Rows of three lattice words: 130 x 5 x 276 points of a 131-wide volume, 3 x 5 x 276 = 4140 words without the cap (two passes and 44)
# and 3 x 7 x 278 = 5838 with it.  Filled with noise its 142 000 cells would cost mesh_ref.extract half a minute, so the content is thinned
# to five bands of three or four slices -- both ends, and around the slices whose lattice words are numbers WORDS_PER_PASS and
# 2 x WORDS_PER_PASS without the cap (15 words a slice) and with it (21 a slice, one slice of cap first) -- and the reference is
# banded_extract's (2 s and 3 s).
WIDE_MESH = ((276, 5, 131), (1, 0, 0), (131, 5, 276))


def wide_mesh_bands():
    nz = WIDE_MESH[0][0]
    marks = sorted({k * WORDS_PER_PASS // 15 for k in (1, 2)} | {k * WORDS_PER_PASS // 21 - 1 for k in (1, 2)})
    bands = [(0, 3)] + [(z - 1, z + 2) for z in marks if z + 2 < nz - 4] + [(nz - 4, nz)]
    assert all(b[0] - a[1] >= 2 for a, b in zip(bands, bands[1:])) and len(bands) == 5
    return bands


def wide_mesh(seed=85):
    """(values float32 (nz, ny, nx), the bands): uniform noise in the bands (0.4 of it at or above MESH_LEVEL), 0.0 elsewhere."""
    rng = np.random.default_rng(seed)
    v = np.zeros(WIDE_MESH[0], f32)
    for z0, z1 in wide_mesh_bands():
        v[z0:z1] = rng.random((z1 - z0,) + WIDE_MESH[0][1:]).astype(f32)
    return v, wide_mesh_bands()


# the band-by-band reference of the rod: 0.2 s without the cap, 0.7 s with it; mesh_ref.counts over the whole rod 0.02 s and 0.2 s
ROD_SHAPE = (65535, 9, 2)  # (nz, ny, nx): keys are z-major; 1 x 9 x 65535 = 589 815 lattice words, 1 x 11 x 65537 with the cap
ROD_LEVEL = MESH_LEVEL


def rod_bands():
    """[z0, z1) of the bands of content, at most 40 slices each: both ends, and around the slices whose lattice words are numbers
    2 x WORDS_PER_PASS (the third pass of the persistent kernels) and LANE_CAP (the second pass of the count's lanes), without the cap
    (9 words a slice) and with it (11 words a slice, one slice of cap before slice 0)."""
    marks = sorted({2 * WORDS_PER_PASS // 9, 2 * WORDS_PER_PASS // 11 - 1, LANE_CAP // 9, LANE_CAP // 11 - 1})
    bands = [(0, 12)] + [(z - 14, z + 14) for z in marks] + [(ROD_SHAPE[0] - 12, ROD_SHAPE[0])]
    assert all(b[0] - a[1] >= 2 for a, b in zip(bands, bands[1:])) and all(b - a <= 40 for a, b in bands)
    return bands


def rod(seed=81):
    """(values float32 (nz, ny, nx), the bands): uniform noise in the bands (0.4 of it at or above the level), 0.0 elsewhere."""
    rng = np.random.default_rng(seed)
    v = np.zeros(ROD_SHAPE, f32)
    for z0, z1 in rod_bands():
        v[z0:z1] = rng.random((z1 - z0,) + ROD_SHAPE[1:]).astype(f32)
    return v, rod_bands()


def content_bands(v, level, box_lo, box_hi):
    """The maximal runs [z0, z1) of slices of the box that hold a voxel at or above the level (NaN is below)."""
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    if x1 <= x0 or y1 <= y0 or z1 <= z0:
        return []
    with np.errstate(invalid="ignore"):
        has = (np.asarray(v, f32)[z0:z1, y0:y1, x0:x1] >= f32(level)).any(axis=(1, 2))
    edges = np.flatnonzero(np.diff(np.concatenate([[False], has, [False]]).astype(np.int8)))
    return [(z0 + int(a), z0 + int(b)) for a, b in zip(edges[::2], edges[1::2])]


def banded_extract(v, level, cap, box_lo, box_hi, extract):
    """mesh_ref.extract (passed in as `extract`) of a call whose content lies in bands of slices, assembled from one extract per band:
    the band with one slice of margin on either side where the box has one (the margin holds nothing at or above the level, so no edge
    from it crosses; where the box ends instead, the band's box ends with it and the cap, if any, is the call's own).  Keys are z-major
    and the bands apart, so the vertices and the triangles of the bands, in turn, are those of the call; indices move by the vertices
    before.  tests/test_loop_passes.py pins it to extract itself."""
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    whole = extract(v[:0], level, cap, (x0, y0, 0), (x1, y1, 0))  # (the empty result)
    verts, tris, edges = [whole["vertices"]], [whole["triangles"]], []
    n_v = n_t = inside = cells = 0
    lo, hi = None, None
    lattice_ok = all(h - l + 2 * cap >= 2 for l, h in zip(box_lo, box_hi)) and all(h > l for l, h in zip(box_lo, box_hi))
    for a, b in content_bands(v, level, box_lo, box_hi):
        s, t = max(z0, a - 1), min(z1, b + 1)
        r = extract(v[s:t], level, cap, (x0, y0, s), (x1, y1, t), origin=(0, 0, s))
        inside += r["result"][2]
        if not lattice_ok or r["result"][3] == 0:
            continue
        verts.append(r["vertices"])
        tris.append(r["triangles"] + np.uint32(n_v))
        edges += r["edges"]
        n_v += r["result"][0]
        n_t += r["result"][1]
        cells += r["result"][3]
        lo = r["result"][4] if lo is None else tuple(min(p, q) for p, q in zip(lo, r["result"][4]))
        hi = r["result"][5] if hi is None else tuple(max(p, q) for p, q in zip(hi, r["result"][5]))
    return dict(vertices=np.concatenate(verts), triangles=np.concatenate(tris),
                result=(n_v, n_t, inside, cells, lo or (0, 0, 0), hi or (0, 0, 0)), edges=edges)


# ---- the inventory ----------------------------------------------------------------------------------------------------------------------

W3, W1, WX = box_words(*WORD_BOXES["three_words"][1:]), box_words(*WORD_BOXES["one_word"][1:]), box_words(*WORD_BOXES["exact_words"][1:])
U1, UX = box_units(*UNIT_BOXES["units"][1:]), box_units(*UNIT_BOXES["exact_units"][1:])
VWORDS = 9 * 65535                      # VWORDS_BOX: nc x slices x (rows of the box + 1) x vwx = 1 x 9 x 65535 x 1
BOARD_NODES = 540800                    # (pinned by tests/test_loop_passes.py, as FISH_NODES)
FISH_NODES = 610984
ROD_WORDS = (9 * 65535, 11 * 65537)     # lattice words without and with the cap
MESH_WORDS = (65 * 64, 17 * 241)        # MESH_BOXES, cap 0
WIDE_MESH_WORDS = (3 * 5 * 276, 3 * 7 * 278)  # WIDE_MESH without and with the cap
LATTICE_QUEUE = 64 * (4 * 3 * 3 + 2)    # the bricks queued for round 4 of the lattice case: 2432
RESAMPLE_UNITS = (resample_units(*RESAMPLE_BOXES["three_pieces"][1:]), resample_units(*RESAMPLE_BOXES["exact_units"][1:]))


def _row(header, kernel, rule, counts, case, n, carries, collective, existing=None):
    return dict(header=header, kernel=kernel, rule=rule, counts=counts, case=case, n=n, carries=carries, collective=collective, existing=existing)


UNIFORM_WAVE = ("u depends on blockIdx and the wavefront's number alone (readfirstlane of threadIdx.x >> 6): every lane of a wavefront "
                "makes the same trips")
WORDS_CASE = "test_loop_passes_gpu: one_word, three_words, exact_words"
# No rows: morph_dilate_kernel and dist_line_kernel take one lane per word or line of a grid that covers them all and return beyond it
# (no loop); grow_seed_kernel is one workgroup of 64 seeds.  `existing` names an older test that passes the threshold; under the
# persistent rule the n % 4 last words of any smaller box go round as well (see above).
ROWS = [
    _row("vr_bitrows.h", "bit_pack_kernel", "tool", "box words", WORDS_CASE, (W1, W3, WX),
         "the CountBox n (count, bounding box) of the wavefront's words, reported once behind the loop",
         "vr_ballot(in) packs a word: " + UNIFORM_WAVE,
         existing="test_morph_gpu.test_word_and_box_edges[130x37x21] reaches 2331 words (283 wavefronts go round once, over the specks "
                  "of the last slices); test_morph_gpu.test_random_sweep has boxes of up to 3 x 140 x 140 words"),
    _row("vr_morph.h", "morph_write_kernel", "tool", "box words", WORDS_CASE, (W1, W3, WX),
         "the CountBox n of the R words", "none (bit_fold is lane-local on a uniform word)",
         existing="as bit_pack_kernel"),
    _row("vr_dist.h", "dist_x_kernel", "tool", "words of the field's region (the box with dense content and no limit)", WORDS_CASE, (W1, W3, WX),
         "nothing but u", "none: the searches for the nearest word are uniform loads, no lane exchanges anything",
         existing="test_distance_gpu.test_word_and_line_edges[130x37x21]: 2331 words, dense"),
    _row("vr_dist.h", "dist_write_kernel", "tool", "box words", WORDS_CASE, (W1, W3, WX),
         "n_beyond and n_probe (uniform), p_min and p_max (per lane), folded once behind the loop",
         "vr_ballot(beyond) inside the loop, wave_min_u64 / wave_max_u64 behind it: " + UNIFORM_WAVE
         + "; the folds sit under P.probe, a kernel argument",
         existing="as dist_x_kernel; the probe's minimum and maximum at this size are new"),
    _row("vr_raster.h", "raster_rows_kernel", "tool", "items: runs of up to 8 rows of one polygon",
         "test_loop_passes_gpu: raster items, and exactly 4097 of them",
         None, "nothing across items (the toggle row in LDS is zeroed per row; `carry` lives within one row)",
         "vr_ballot over the word parities and wave_lds_fence, inside the loops over an item's rows and a row's chunks: the item, its polygon, "
         "nw and the chunk count are loaded uniformly (" + UNIFORM_WAVE + ")"),
    _row("vr_raster.h", "raster_write_kernel", "tool", "box words", WORDS_CASE, (W1, W3, WX),
         "the four CountBoxes n[k]", "none",
         existing="test_raster_gpu.test_word_and_box_edges[130x37x21]: 2331 words under a 17-gon per slice"),
    _row("vr_outline.h", "outline_corners_kernel", "lane", "vertex words", "test_loop_passes_gpu: outline vertex words", VWORDS,
         "nothing but u", "none"),
    _row("vr_outline.h", "outline_link_kernel", "lane", "nodes", "test_loop_passes_gpu: checkerboard, fishbone", (BOARD_NODES, FISH_NODES),
         "area[4], the shoelace sums per contour place, added up per lane over its nodes",
         "wave_sum_u64 BEHIND the loop, under k < G.nc (a kernel argument): lanes leave the loop at different trips (and `continue` inside it) "
         "and meet again before the sum; nothing collective inside"),
    _row("vr_outline.h", "outline_rank_init_kernel", "lane", "nodes", "as outline_link_kernel", (BOARD_NODES, FISH_NODES), "nothing but i", "none"),
    _row("vr_outline.h", "outline_rank_kernel", "lane", "nodes", "as outline_link_kernel; the fishbone runs all 20 rounds", (BOARD_NODES, FISH_NODES),
         "`any`: a change at any of the lane's nodes, stored behind the loop", "none (every writer of *changed stores 1)"),
    _row("vr_outline.h", "outline_leaders_kernel", "lane", "nodes", "as outline_link_kernel", (BOARD_NODES, FISH_NODES), "nothing but i", "none"),
    _row("vr_outline.h", "outline_counts_kernel", "lane", "nodes", "as outline_link_kernel", (BOARD_NODES, FISH_NODES), "nothing but i", "none"),
    _row("vr_outline.h", "outline_emit_kernel", "lane", "nodes", "as outline_link_kernel", (BOARD_NODES, FISH_NODES), "nothing but i", "none"),
    _row("vr_mesh.h", "mesh_pack_kernel", "tool", "lattice words", "test_loop_passes_gpu: mesh boxes, the rows of three words and the mesh rod",
         MESH_WORDS + WIDE_MESH_WORDS + ROD_WORDS,
         "n_box, n_load, n_settled per lane and n_in on lane 0, summed behind the loop",
         "vr_ballot(in) inside the loop (" + UNIFORM_WAVE + "); wave_sum_u64 behind it, unconditional",
         existing="test_mesh_index_edges_gpu.test_an_axis_of_65535 passes 2048 words, held to counts and closedness only"),
    _row("vr_mesh.h", "mesh_count_kernel", "lane", "lattice words", "test_loop_passes_gpu: the mesh rod", ROD_WORDS,
         "the CountBox n of the active cells, per lane", "wave_sum_u64, wave_min_i32, wave_max_i32 behind the loop, unconditional; none inside"),
    _row("vr_mesh.h", "mesh_vertex_kernel", "tool", "lattice words", "as mesh_pack_kernel", MESH_WORDS + WIDE_MESH_WORDS + ROD_WORDS, "nothing but u",
         "none: lanes without a crossing `continue`, and nothing in the body is collective", existing="as mesh_pack_kernel"),
    _row("vr_mesh.h", "mesh_triangle_kernel", "tool", "lattice words", "as mesh_pack_kernel", MESH_WORDS + WIDE_MESH_WORDS + ROD_WORDS,
         "nothing but u",
         "none: lanes without an active cell `continue`, and nothing in the body is collective", existing="as mesh_pack_kernel"),
    _row("vr_hist.h", "hist_kernel", "tool", "units", "test_loop_passes_gpu: units, exact_units, with a mask and all five rows", (U1, UX),
         "the workgroup's LDS copy of the counts; vox[], dropped[], n_box, n_load, n_settled per lane",
         "vr_ballot and readlane in the combining, under `H.rows >> r & 1` (a kernel argument); a settled unit `continue`s on its record, "
         "loaded uniformly; __syncthreads and wave_sum_u64 lie outside the loop: " + UNIFORM_WAVE,
         existing="test_histogram_gpu.test_large_volume_many_blocks: 65 536 units (32 passes) and a box of 63 504 (a partial 32nd), random "
                  "content, counts, rows and counters equal, both forms, LDS and global bins -- unmasked; test_index_edges_gpu's A1 "
                  "histograms 2^22 units"),
    _row("vr_grow.h", "grow_classify_kernel", "tool", "units", "test_loop_passes_gpu: units, exact_units", (U1, UX),
         "n_box, n_load, n_settled per lane", "vr_ballot(ok) packs Q; a settled unit `continue`s on its record, loaded uniformly: " + UNIFORM_WAVE,
         existing="test_grow_gpu.test_noise_large_many_workgroups: 2340 units and bricks (292 wavefronts go round once)"),
    _row("vr_grow.h", "grow_round_kernel", "tool", "items: every brick (sweep form) or the round's queued bricks (frontier form)",
         "test_loop_passes_gpu: units, exact_units (the sweep form walks all 4352 / 4097 bricks every round); the lattice (the frontier form's "
         "queue of 2432 bricks in round 4)", (U1, UX, LATTICE_QUEUE),
         "nothing but i",
         "grow_wave_or (shuffles) behind two `continue`s, on list_in[i] and on q[b]: both loaded at wave-uniform addresses: " + UNIFORM_WAVE
         + ".  The frontier form's n_in passes 2048 only with that many bricks queued for ONE round: the lattice case, whose queues "
         "frontier_shells counts on the CPU",
         existing="as grow_classify_kernel"),
    _row("vr_grow.h", "grow_write_kernel", "tool", "bricks of the volume", "test_loop_passes_gpu: units, exact_units", (U1, UX),
         "the CountBox n of the R words", "none", existing="as grow_classify_kernel"),
    _row("vr_resample.h", "resample_kernel", "tool", "units: 64-voxel pieces of a row of the box",
         "test_loop_passes_gpu: resample three_pieces, exact_units", RESAMPLE_UNITS,
         "row and xu, advanced by stride / ux and stride % ux with a carry; n_in, n_load, the y and z bounds (uniform), the x bounds per lane",
         "vr_ballot(in), vr_ballot(in && !settles), vr_ballot(load), under in_mask != 0 (itself a ballot) and R.bricks (an argument); the "
         "shuffles behind the loop are unconditional: " + UNIFORM_WAVE),
]
# vr_comp.h: every loop is taken round by the scale tests that exist (comp_cases.MIDDLE has more than LANE_CAP nodes and components, the
# scan boxes 262 144 and 262 145 words; the rods pass WORDS_PER_PASS): (kernel, rule, what n counts, the test)
MORE_NODES = "test_components_scale_gpu.test_more_nodes_than_lanes"
SCAN_BOXES = "test_components_scale_gpu.test_scan_of_one_spine_chunk_and_one_word_more"
COMP_ROWS = [
    ("comp_complement_kernel", "lane", "box words", "test_loop_passes_gpu.test_components_of_the_background (no scale test has a background "
     "over more than LANE_CAP words: the rods have 131 070, the limit's boxes take the set)"),
    ("comp_starts_kernel", "lane", "box words",
     "test_components_scale_gpu.test_label_limit_from_both_sides (its boxes of 129 slices: 528 384 words)"),
    ("comp_runs_kernel", "lane", "box words", "test_components_scale_gpu.test_label_limit_from_both_sides (as comp_starts_kernel)"),
    ("comp_merge_kernel", "lane", "nodes", MORE_NODES), ("comp_flatten_kernel", "lane", "nodes", MORE_NODES),
    ("comp_leaders_kernel", "lane", "nodes", MORE_NODES), ("comp_init_kernel", "lane", "nodes", MORE_NODES),
    ("comp_stats_kernel", "lane", "nodes", MORE_NODES + " (i0 is the workgroup's: every lane takes part in the votes)"),
    ("comp_pass_kernel", "lane", "components", MORE_NODES + "[checkerboard_faces]"),
    ("comp_result_kernel", "lane", "components", MORE_NODES + "[checkerboard_faces]"),
    ("comp_expand_kernel", "lane", "nodes", MORE_NODES),
    ("comp_write_kernel", "tool", "box words", SCAN_BOXES + " (262 144 and 262 145 words: 128 passes, and one word of a 129th)"),
]


# ---- the channel tools: filter, rank, gamma -------------------------------------------------------------------------------------------
# Their kernels are all launched with lane_blocks: the default forms with one workgroup per TILE up to 4 x TOOL_BLOCKS = 2048 workgroups
# (`u += gridDim.x` over the tiles), the plain forms and the writes with one lane per voxel of the box (`i += step`, step = 256 x
# gridDim.x <= LANE_CAP).  What a later trip of a tile loop needs is the barrier at the loop's tail (the next tile overwrites the LDS the
# last one read); what a write carries is its counts and its least and greatest key, folded once behind the loop.
CHANNEL_HEADERS = ["vr_filter.h", "vr_rank.h", "vr_gamma.h"]
CHANNEL_API = {"vr_filter.h": "vr_api_filter.h", "vr_rank.h": "vr_api_rank.h", "vr_gamma.h": "vr_api_gamma.h"}
TILE_LOOP = r"for \(unsigned long long u = blockIdx\.x; u < \w+\.tiles; u \+= gridDim\.x\)"
LANE_LOOP = r"for \(unsigned long long i = \(unsigned long long\)blockIdx\.x \* 256ull \+ threadIdx\.x; i < n; i \+= step\)"
LANE_STEP = r"step = \(unsigned long long\)gridDim\.x \* 256ull"
FILTER_ROUND = "test_filter_gpu.test_the_launch_loops_go_round"
RANK_ROUND = "test_rank_gpu.test_the_launch_loops_go_round"
GAMMA_ROUND = "test_gamma_gpu.test_the_launch_loops_go_round"
# (header, kernel, rule, what n counts, the GPU test that takes the loop past its first trip)
CHANNEL_ROWS = [
    ("vr_filter.h", "filter_x_kernel", "tile", "tiles: runs of 256 outputs of a row x groups of 8 rows of the pass' region", FILTER_ROUND),
    ("vr_filter.h", "filter_line_kernel", "tile", "tiles: 64 x by 64 outputs along the axis, for every line of the third axis", FILTER_ROUND),
    ("vr_filter.h", "filter_plain_kernel", "lane", "voxels of the pass' region", FILTER_ROUND),
    ("vr_filter.h", "filter_write_kernel", "lane", "box voxels", FILTER_ROUND),
    ("vr_rank.h", "rank_tile_kernel", "tile", "tiles: 32 x 8 x 4 outputs of the box", RANK_ROUND),
    ("vr_rank.h", "rank_plain_kernel", "lane", "box voxels", RANK_ROUND),
    ("vr_rank.h", "rank_write_kernel", "lane", "box voxels", RANK_ROUND),
    ("vr_gamma.h", "gamma_tile_kernel", "tile", "tiles: 32 x 8 x 4 outputs of the box", GAMMA_ROUND),
    ("vr_gamma.h", "gamma_plain_kernel", "lane", "box voxels", GAMMA_ROUND),
    ("vr_gamma.h", "gamma_write_kernel", "lane", "box voxels", GAMMA_ROUND),
]

# The filter's case: (nz, ny, nx) = (343, 343, 5) with r = 2 on every axis and the whole box.  x pass: 1 run x ceil(343 x 343 / 8)
# groups of rows; y pass: 1 x ceil(343 / 64) x 343; z pass the same; all against 2048 workgroups.  Voxels against LANE_CAP lanes.
FILTER_ROUND_SHAPE = (343, 343, 5)
FILTER_ROUND_TILES = (14707, 2058, 2058)
FILTER_ROUND_VOXELS = 588245
FILTER_ROUND_TAIL = 50000  # the last voxels, x fastest: all beyond LANE_CAP, the write's second trip


def filter_round_case(seed=73):
    """(src, the same with the tail's channel 3 zeroed): noise in every component; in channel 3 of the last FILTER_ROUND_TAIL voxels the
    source's greatest and least value by far and three NaN, each at least 8000 voxels (more than two slices) from the tail's start and
    from the volume's end, so that what the passes make of them stays in the tail."""
    src = np.random.default_rng(seed).normal(0.0, 1.0, FILTER_ROUND_SHAPE + (4,)).astype(f32)
    n = FILTER_ROUND_VOXELS
    for back, value in ((40000, 1000.0), (30000, -1000.0), (20000, np.nan), (15000, np.nan), (10000, np.nan)):
        src[np.unravel_index(n - back, FILTER_ROUND_SHAPE) + (3,)] = f32(value)
    zeroed = src.copy()
    zeroed[..., 3] = np.where(np.arange(n) >= n - FILTER_ROUND_TAIL, f32(0.0), src[..., 3].reshape(-1)).reshape(FILTER_ROUND_SHAPE)
    return src, zeroed
