"""Volumes, tables and views at the edges of the kernels' index ranges, shared by tests/test_index_edges.py (the conditions the
content and the views must meet, on the CPU) and tests/test_index_edges_gpu.py (the kernels against their references).

A1 and A2 straddle the 4 GiB line; B1 and B2 the brick-index limit (include/vr.h); the rods have one axis of up to 65535 voxels.
Everything is zero but two bands at the ends of z, so that the bulk costs the references nothing.  Harness only."""
import numpy as np

import host_ref as hr
import oracle_binding as ob

f32 = np.float32

A1 = (512, 512, 1032)   # (nx, ny, nz): 270 532 608 voxels = 4.03 GiB; byte 2^32 is voxel 2^28 = the start of slab z = 1024
A2 = (509, 509, 1033)   # 4 282 090 768 B linear (below the line); its bricked copy 512 x 512 x 1036 = 271 581 184 slots (above)
LINE_Z = 1024           # in both, and in both layouts: voxel / slot 2^28 is (0, 0, 1024)
BAND = 32               # slabs of content at either end of z
SOLID = 12              # slabs at z < SOLID have no zero runs (what the slabs beyond the line alias with under a truncated offset)
B1 = (1, 8192, 16384)   # 1 x 2048 x 4096 bricks: bny * bnz = 2^23, the last grid the skipping kernels index
B2 = (1, 8196, 16384)   # 1 x 2049 x 4096 bricks: refused
W, H = 32, 24           # the viewport of every view below


def band_raw(seed, nx, ny, depth, solid, odd):
    """uint16 [depth, ny, nx]: noise on a smooth blob, with runs of exact zeros (8^3 blocks, half of them) except in the first
    `solid` slabs.  Non-zero values are odd (`odd`) or even: two bands of different parity share no non-zero value."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(ny, dtype=f32), np.arange(nx, dtype=f32), indexing="ij")
    g = np.exp(-((x - f32(0.45 * nx)) ** 2 + (y - f32(0.55 * ny)) ** 2) / f32(2.0 * (0.22 * max(nx, ny, 8)) ** 2))
    raw = (f32(600.0) + f32(2800.0) * g)[None, :, :] + rng.integers(0, 600, size=(depth, ny, nx)).astype(f32)
    raw = raw.astype(np.uint16)
    raw = (raw | 1) if odd else (raw & ~np.uint16(1))
    holes = rng.random(((depth + 7) // 8, (ny + 7) // 8, (nx + 7) // 8)) < 0.5
    holes = np.repeat(np.repeat(np.repeat(holes, 8, 0), 8, 1), 8, 2)[:depth, :ny, :nx]
    holes[:solid] = False
    raw[holes] = 0
    return raw


def bands(shape, seed=1):
    """(low, high) raw bands of a volume (nx, ny, nz): z in [0, BAND) with odd values and no zero below SOLID, z in [nz - BAND, nz)
    with even ones."""
    nx, ny, nz = shape
    return band_raw(100 + seed, nx, ny, BAND, SOLID, True), band_raw(200 + seed, nx, ny, BAND, 0, False)


def raw_volume(shape, seed=1):
    nx, ny, nz = shape
    raw = np.zeros((nz, ny, nx), np.uint16)
    raw[:BAND], raw[nz - BAND:] = bands(shape, seed)
    return raw


def prepared(raw):
    """The reference's preparation on the host: broadcast, normalise, gradient."""
    v = ob.normalize_data(hr.raw_to_vec4(raw))
    return ob.precompute_gradient(v)


def sheet_raw(shape, seed=3):
    """B1 / B2: (1, ny, nz) with noise and zero runs along y in the top two brick slabs (z >= nz - 8) and at z < 8."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    raw = np.zeros((nz, ny, nx), np.uint16)
    for sl in (slice(0, 8), slice(nz - 8, nz)):
        part = rng.integers(1, 4096, size=(8, ny, nx)).astype(np.uint16)
        runs = np.repeat(rng.random((ny + 63) // 64) < 0.6, 64)[:ny]
        part[:, runs] = 0
        raw[sl] = part
    return raw


def rod_raw(shape, seed=7):
    """A rod with one long axis: noise with zero runs of 1 to 600 bricks along it (the field's distances reach the cap of 128)."""
    nx, ny, nz = shape
    rng = np.random.default_rng([seed, nx, ny, nz])
    raw = rng.integers(1, 4096, size=(nz, ny, nx)).astype(np.uint16)
    axis = int(np.argmax([nz, ny, nx]))
    n = raw.shape[axis]
    keep = np.ones(n, bool)
    pos = 0
    while pos < n:
        pos += 4 * int(rng.integers(1, 40))          # tissue
        run = 4 * int(rng.integers(1, 601))          # air
        keep[pos:pos + run] = False
        pos += run
    idx = [slice(None)] * 3
    idx[axis] = ~keep
    raw[tuple(idx)] = 0
    return raw


def prefix_tf(res=64, zeros=9, top=0.08):
    """A zero prefix (skipping is live) and a low ramp (no ray terminates early: the rays of a view along z reach both bands)."""
    o = np.zeros(res, dtype=f32)
    o[zeros:] = np.linspace(0.0, top, res - zeros + 1, dtype=f32)[1:]
    return o, hr.default_color_tf(res)


def top_view(shape, first_slab=1018, **over):
    """From the far end of z (a yaw of pi looks down the texture's z axis from z = 1), the clip box confined to z >= first_slab:
    one-voxel steps through the top of the volume."""
    nx, ny, nz = shape
    kw = dict(distance=1.1, yaw=3.26, pitch=0.08, steps_count=72, step_size=1.0 / nz, clip_z=(first_slab / nz, 0.0))
    kw.update(over)
    return kw


def through_view(shape, **over):
    """From z = 1 along z through the whole volume in four-voxel steps: every ray crosses the line and reaches the low band."""
    nx, ny, nz = shape
    kw = dict(distance=1.1, yaw=3.04, pitch=0.05, steps_count=300, step_size=4.0 / nz)
    kw.update(over)
    return kw


def uniforms(kw):
    return hr.make_uniforms(W, H, **kw)


def sample_cells(u, nz, w=W, h=H):
    """z of the base cell (floor(p.z * nz - 0.5)) of every in-box sample position of every ray of the frame: the positions every
    march restates (start + k * step by repeated rounded additions, proj_ref.march)."""
    lo = np.array([f32(0.0) + f32(u.clip_x[0]), f32(0.0) + f32(u.clip_y[0]), f32(0.0) + f32(u.clip_z[0])], f32)
    hi = np.array([f32(1.0) - f32(u.clip_x[1]), f32(1.0) - f32(u.clip_y[1]), f32(1.0) - f32(u.clip_z[1])], f32)
    rays = [ob.setup_ray(u, w, h, px, py) for py in range(h) for px in range(w)]
    hit = np.array([r[0] for r in rays])
    start = np.array([r[1] for r in rays], f32)[hit]
    end = np.array([r[2] for r in rays], f32)[hit]
    diff = end - start
    ln = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
    step = (diff * (f32(1.0) / ln)[:, None]) * f32(u.step_size)
    p, cells = start.copy(), []
    for _ in range(u.steps_count):
        inb = np.all((p >= lo) & (p <= hi), axis=1)
        cells.append(np.floor(p[inb, 2] * f32(nz) - f32(0.5)).astype(np.int64))
        p = p + step
    return np.concatenate(cells)


def lds_rule_shapes(tf_res=64):
    """The rods on either side of the two LDS rules of eligibility() (csrc/vr_api_render.h), solved for nx with ny = nz = 1:
    16 / 17 need (tf_res + 2) * 16 + (nx + ny + nz + 3) * 8 <= 160 KiB, 18 needs (nx + ny + nz + 6) * 4 <= 32 KiB.
    {flavour: (largest nx that fits, the next one)}."""
    p2 = (160 * 1024 - (tf_res + 2) * 16) // 8 - 3 - 2
    lut = (32 * 1024) // 4 - 6 - 2
    return {17: (p2, p2 + 1), 18: (lut, lut + 1)}


RODS = [(65535, 1, 1), (1, 65535, 1), (1, 1, 65535), (65535, 2, 3)]
