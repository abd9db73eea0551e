"""Surface extraction (vr_volume_mesh) at the edges of its index ranges, in the pattern of tests/index_edges_cases.py: an axis of 65535
voxels in a thin volume (1024 words a lattice row, 1025 with the cap; 65535 rows; 65535 slices), and a small box in the far corner of a
volume of 4.03 GiB, whose voxels' byte offsets pass 2^32.  The box calls equal the restatement bit for bit; the whole rods, too long
for a Python loop over cells, are held to the vectorised counts of mesh_ref.counts and to closedness."""
import numpy as np
import pytest

import index_edges_cases as ie
import mesh_cases as mc
import mesh_ref as mr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 32, 24


def same(got, want, what):
    verts, tris, res = got
    assert res.as_tuple() == want["result"], (what, res.as_tuple(), want["result"])
    assert verts.shape == want["vertices"].shape and np.array_equal(vt.bits(verts), vt.bits(want["vertices"])), what
    assert np.array_equal(tris, want["triangles"]), what


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x65535", "y65535", "z65535"])
def test_an_axis_of_65535(axis):
    dims = [3, 2, 2]                      # (nx, ny, nz)
    dims[axis] = 65535
    nx, ny, nz = dims
    rng = np.random.default_rng(axis)
    i = np.arange(65535).reshape([65535 if a == 2 - axis else 1 for a in range(3)])
    v = (np.sin(0.37 * i) + 0.8 * rng.normal(size=(nz, ny, nx))).astype(f32)  # a crossing every few voxels
    far = [0, 0, 0]
    far[axis] = 65535 - 130
    with capi.Context(W, H, 0) as ctx:
        ctx.volume_upload(0, mc.vec4(v, 3, seed=4))
        for cap in (0, 1):
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                d = capi.MeshDesc().copy(src_slot=0, channel=3, level=0.25, cap=cap, box_lo=(0, 0, 0), box_hi=dims)
                verts, tris, res = ctx.volume_mesh(d)
                n_v, n_t, inside, cells = mr.counts(v, 0.25, cap, (0, 0, 0), dims)
                assert (res.n_vertices, res.n_triangles, res.inside, res.cells) == (n_v, n_t, inside, cells) and n_t > 65535, (cap, flavour)
                assert int(tris.max()) == n_v - 1 and len(np.unique(tris)) == n_v
                assert verts[:, axis].max() > 65533 and verts.min() >= 0 and (verts.max(0) <= np.array(dims) - 1).all()
                assert mr.is_closed(tris) == bool(cap)
                assert ctx.mesh_counters()[0] == nx * ny * nz
                # the far end as a box of its own
                d = d.copy(box_lo=far)
                same(ctx.volume_mesh(d), mr.extract(v, 0.25, cap, tuple(far), tuple(dims)), (axis, cap, flavour))


def test_a_box_beyond_4_gib():
    """A1 (512 x 512 x 1032, 4.03 GiB): the box lies in the last six slabs, every voxel offset of it beyond 2^32 bytes; what lies below the
    line differs, so an offset truncated to 32 bits reads other values."""
    nx, ny, nz = ie.A1
    raw = np.zeros((nz, ny, nx), np.uint16)
    rng = np.random.default_rng(11)
    raw[:40] = rng.integers(0, 4096, size=(40, ny, nx), dtype=np.uint16)       # (where truncated offsets land)
    crop = rng.integers(0, 4096, size=(6, 20, 70), dtype=np.uint16)
    crop[2:6, 0:13, 2:43] = 4000                                              # constant bricks among the noise
    raw[nz - 6:, ny - 20:, nx - 70:] = crop
    lo, hi = (nx - 70, ny - 20, nz - 6), (nx, ny, nz)
    assert (((lo[2] * ny + lo[1]) * nx + lo[0]) * 16) > 1 << 32
    v = crop.astype(f32)
    with capi.Context(W, H, 0) as ctx:
        ctx.volume_upload_raw(0, raw)
        del raw
        for channel in (3, 0):
            for cap in (0, 1):
                want = mr.extract(v, 2000.5, cap, lo, hi, origin=lo)
                assert want["result"][1] > 1000
                for flavour in (0, 1):
                    ctx.set_kernel_flavour(flavour)
                    d = capi.MeshDesc().copy(src_slot=0, channel=channel, level=2000.5, cap=cap, box_lo=lo, box_hi=hi)
                    same(ctx.volume_mesh(d), want, (channel, cap, flavour))
                    cnt = ctx.mesh_counters()
                    assert cnt[0] == 70 * 20 * 6 and (cnt[2] > 0) == (channel == 3 and flavour == 0), (channel, cap, flavour, cnt)
