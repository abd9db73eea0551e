"""The conditions tests/test_index_edges_gpu.py relies on, checked on the CPU: the content of the volumes around the 4 GiB line
cannot be read right through an offset truncated to 32 bits, the clipped views sample beyond the line, the shapes sit where the
text says, and the vectorised field restatement (skip_ref.py) equals the brute-force one it replaced."""
import numpy as np
import pytest

import index_edges_cases as ie
import skip_ref as sk

f32 = np.float32
GIB4 = 1 << 32


def slot_of(x, y, z, shape):
    """Slot of voxel (x, y, z) in the bricked copy (4^3 voxels per storage brick, bricks x-fastest, the volume padded to whole bricks)."""
    nbx, nby = (shape[0] + 3) // 4, (shape[1] + 3) // 4
    return (((z // 4) * nby + y // 4) * nbx + x // 4) * 64 + (z % 4) * 16 + (y % 4) * 4 + x % 4


def test_shapes_sit_on_either_side_of_the_line():
    nx, ny, nz = ie.A1
    assert nx * ny * nz * 16 > GIB4 and nx * ny * ie.LINE_Z * 16 == GIB4          # byte 2^32 = the start of slab 1024
    assert slot_of(0, 0, ie.LINE_Z, ie.A1) == 1 << 28
    nx, ny, nz = ie.A2
    assert nx * ny * nz * 16 == 4282090768 < GIB4                                  # the linear array: 32-bit offsets
    padded = [(n + 3) // 4 * 4 for n in ie.A2]
    assert padded == [512, 512, 1036] and padded[0] * padded[1] * padded[2] == 271581184 and 271581184 * 16 > GIB4
    assert slot_of(0, 0, ie.LINE_Z, ie.A2) == 1 << 28
    # one gather window of the lit shader's two-steps-ahead kernel (2^28 - 1 slots) plus a sliver
    for slots in (271581184, ie.A1[0] * ie.A1[1] * ie.A1[2]):
        assert 0 < slots - 0x0fffffff < 0.02 * 0x0fffffff
    # the in-place passes and refresh_bricks run over more than 2^28 voxels
    assert ie.A1[0] * ie.A1[1] * ie.A1[2] > 1 << 28


@pytest.mark.parametrize("shape", [ie.A1, ie.A2], ids=["A1", "A2"])
def test_content_beyond_the_line_differs_from_what_a_truncated_offset_reads(shape):
    """Voxel (x, y, z >= 1024) minus 2^28 voxels (A1's linear array) or slots (either bricked copy) is voxel (x, y, z - 1024).  The
    low band has odd values and no zero there, the high band even ones: the two differ at EVERY such voxel, so no offset that lost
    bit 32 reads the same number anywhere beyond the line."""
    nx, ny, nz = shape
    low, high = ie.bands(shape)
    beyond = nz - ie.LINE_Z
    assert 0 < beyond <= ie.SOLID <= ie.BAND
    z = np.arange(ie.LINE_Z, nz)
    # the aliases, from the layouts' own index arithmetic
    assert np.array_equal(slot_of(5, 7, z, shape) - (1 << 28), slot_of(5, 7, z - ie.LINE_Z, shape))
    if shape == ie.A1:
        assert np.array_equal((z * ny + 7) * nx + 5 - (1 << 28), ((z - ie.LINE_Z) * ny + 7) * nx + 5)
    top = high[ie.BAND - beyond:]      # z in [1024, nz)
    alias = low[:beyond]               # z in [0, nz - 1024)
    assert (alias != 0).all() and (alias % 2 == 1).all() and (top % 2 == 0).all()
    assert (top != alias).all()
    # skipping is live and an isosurface exists beyond the line: whole bricks of zeros beside values on both sides of mid-range
    assert 0.2 < float((top == 0).mean()) < 0.8 and (low[ie.SOLID:] == 0).any()
    peak = max(int(low.max()), int(high.max()))
    nonzero = top[top != 0]
    assert (nonzero > 0.6 * peak).any() and (nonzero < 0.4 * peak).any()
    # the two ends come from different seeds
    assert not np.array_equal(low[ie.SOLID:] == 0, high[ie.SOLID:] == 0)


def test_raw_volume_is_the_bands_around_zeros():
    shape = (24, 20, 80)
    raw = ie.raw_volume(shape)
    low, high = ie.bands(shape)
    assert raw.shape == (80, 20, 24) and not raw[ie.BAND:80 - ie.BAND].any()
    assert np.array_equal(raw[:ie.BAND], low) and np.array_equal(raw[80 - ie.BAND:], high)


@pytest.mark.parametrize("shape", [ie.A1, ie.A2], ids=["A1", "A2"])
def test_clipped_views_sample_beyond_the_line(shape):
    """Every sample of the clipped view lies in a cell at z >= 990, and at least half of them in cells with a corner at z >= 1024;
    the view along z crosses the line and reaches the low band."""
    nz = shape[2]
    cells = ie.sample_cells(ie.uniforms(ie.top_view(shape)), nz)
    assert cells.size > 5000 and cells.min() >= 990
    assert float((cells + 1 >= ie.LINE_Z).mean()) >= 0.5
    cells = ie.sample_cells(ie.uniforms(ie.through_view(shape)), nz)
    assert (cells >= ie.LINE_Z).any() and (cells < ie.BAND).any() and ((cells > 400) & (cells < 600)).any()


def test_sheets_put_content_in_the_top_two_brick_slabs():
    for shape in (ie.B1, ie.B2):
        nx, ny, nz = shape
        assert nx * ny * nz * 16 < GIB4
        # (only the ends are generated here: the whole sheet is 2 GiB of voxels)
        small = ie.sheet_raw((1, ny, 64))
        assert small[60:].any() and small[:8].any() and not small[8:56].any()
        assert (small[56:, :, 0] == 0).all(axis=0).reshape(-1, 4).all(axis=1).any()  # whole bricks of zeros along y
    bn = lambda s: [(n + 3) // 4 for n in s]  # noqa: E731
    assert bn(ie.B1)[1] * bn(ie.B1)[2] == 1 << 23 and bn(ie.B2)[1] * bn(ie.B2)[2] > 1 << 23


def test_lds_rule_shapes():
    s = ie.lds_rule_shapes(64)
    assert s[18] == (8184, 8185) and s[17] == (20343, 20344)
    for fl, (fits, over) in s.items():
        for nx, ok in ((fits, True), (over, False)):
            lds = (64 + 2) * 16 + (nx + 1 + 1 + 3) * 8 if fl == 17 else (nx + 1 + 1 + 6) * 4
            assert (lds <= (160 if fl == 17 else 32) * 1024) == ok, (fl, nx, lds)


def test_rods_have_runs_past_the_cap():
    for shape in ie.RODS:
        raw = ie.rod_raw(shape)
        v = np.zeros(raw.shape + (4,), f32)
        v[..., 3] = raw.astype(f32) / f32(4095.0)
        act = sk.numpy_active(v, ie.prefix_tf()[0])
        field = sk.linf_field(act)
        assert max(act.shape) == 16384 and act.any() and not act.all()
        assert field.max() == sk.CAP and field.min() == 0


# ---- skip_ref.py against the brute-force forms it replaced (tests/test_tf_edit_gpu.py before)

def brute_field(active):
    big = 1 << 20
    d = np.where(active, 0, big).astype(np.int64)
    for axis in (2, 1, 0):
        idx = np.arange(d.shape[axis])
        dist = np.abs(idx[:, None] - idx[None, :])
        moved = np.moveaxis(d, axis, -1)
        d = np.moveaxis(np.min(np.maximum(dist[None, :, :], moved[..., None, :]), axis=-1), -1, axis)
    return np.minimum(d, sk.CAP).astype(np.uint8)


def brute_records(vol):
    nz, ny, nx = vol.shape[:3]
    bn = [(n + 3) // 4 for n in (nx, ny, nz)]
    dens = np.empty((bn[2], bn[1], bn[0]), dtype=f32)
    rgb = np.empty_like(dens)
    for bz in range(bn[2]):
        for by in range(bn[1]):
            for bx in range(bn[0]):
                v = vol[4 * bz:min(4 * bz + 5, nz), 4 * by:min(4 * by + 5, ny), 4 * bx:min(4 * bx + 5, nx)]
                dens[bz, by, bx] = v[..., 3].max()
                rgb[bz, by, bx] = v[..., :3].max()
    return dens, rgb


@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 5, 9), (13, 8, 17), (3, 300, 2), (24, 24, 24)])
def test_vectorised_records_equal_brute_force(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(nx * 1000 + ny * 10 + nz)
    vol = rng.random((nz, ny, nx, 4)).astype(f32) - f32(0.3)
    vol[rng.random((nz, ny, nx)) < 0.5] = 0
    d, r = sk.brick_records(vol)
    bd, br = brute_records(vol)
    assert np.array_equal(d, bd) and np.array_equal(r, br)


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 3, 2), (2, 5, 300), (1, 290, 3), (20, 20, 20)])
@pytest.mark.parametrize("density", [0.0, 0.004, 0.2, 1.0])
def test_vectorised_field_equals_brute_force(shape, density):
    rng = np.random.default_rng(int(density * 1000) + sum(shape))
    active = rng.random(shape) < density
    assert np.array_equal(sk.linf_field(active), brute_field(active))
