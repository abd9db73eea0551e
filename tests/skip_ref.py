"""numpy restatement of what exact empty-space skipping derives from a volume and an opacity table: the per-brick records
(brick_max_kernel), the active bricks (brick_active_kernel's rule) and the capped Chebyshev distance field (vr_skip_field).
Vectorised, so that grids of 16384 bricks along an axis and volumes of 2^28 voxels stay affordable.  Harness only."""
import numpy as np

f32 = np.float32
CAP = 128  # the field's cap (vr_skip_field)
BRICK = 4  # cells per brick edge


def linf_field(active):
    """min(L-infinity distance to the nearest active brick, CAP) of a boolean grid [bnz, bny, bnx], by the separable form:
    per axis out[i] = min over j of max(|i - j|, d[j]).  A j with |i - j| >= CAP cannot bring the result below CAP, and a
    d[j] above CAP acts like CAP there, so the offsets -CAP + 1 .. CAP - 1 on values capped at CAP give the same field."""
    d = np.where(np.asarray(active, dtype=bool), 0, CAP).astype(np.uint8)
    for axis in (2, 1, 0):
        m = np.ascontiguousarray(np.moveaxis(d, axis, -1))  # (the shifted slices below run along contiguous rows)
        out = m.copy()
        n = m.shape[-1]
        for k in range(1, min(CAP, n)):
            kk = np.uint8(k)
            np.minimum(out[..., k:], np.maximum(m[..., :-k], kk), out=out[..., k:])   # j = i - k
            np.minimum(out[..., :-k], np.maximum(m[..., k:], kk), out=out[..., :-k])  # j = i + k
        d = np.moveaxis(out, -1, axis)
    return np.ascontiguousarray(d)


def _brick_max_axis(a, axis):
    """max over the voxels [4 b, min(4 b + 4, n - 1)] of `axis`, for every brick b of it."""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    bn = (n + BRICK - 1) // BRICK
    pad = BRICK * bn + 1 - n  # (the last voxel once more: it belongs to every range the padding reaches into)
    p = np.concatenate([a, np.repeat(a[..., -1:], pad, axis=-1)], axis=-1)
    main = p[..., :BRICK * bn].reshape(a.shape[:-1] + (bn, BRICK)).max(axis=-1)
    out = np.maximum(main, p[..., BRICK:BRICK * bn + 1:BRICK])
    return np.moveaxis(out, -1, axis)


def brick_max(plane):
    """Per brick of 4^3 cells, the maximum of a plane [nz, ny, nx] over the voxels its cells can touch (finite values)."""
    out = np.asarray(plane, dtype=f32)
    for axis in (2, 1, 0):
        out = _brick_max_axis(out, axis)
    return np.ascontiguousarray(out)


def brick_records(vol):
    """Per brick of 4^3 cells (vr_prep.h brick_max_kernel): the maxima of .a and of max(r, g, b) over the voxels
    [4 b, min(4 b + 4, n - 1)] of each axis (finite volumes)."""
    return brick_max(vol[..., 3]), np.maximum(np.maximum(brick_max(vol[..., 0]), brick_max(vol[..., 1])), brick_max(vol[..., 2]))


def zero_prefix(opacity):
    """Index of the last entry of the table's run of leading exact zeros (-1: none)."""
    return int(np.argmax(opacity != 0.0)) - 1 if (opacity != 0.0).any() else opacity.size - 1


def numpy_active(density_vol, opacity, mask_vol=None):
    """The active bricks (brick_active_kernel's rule) from the volume and the opacity table, independently of the field."""
    z = zero_prefix(opacity)
    dens = brick_max(density_vol[..., 3])
    res = f32(opacity.size)
    inert = np.where(dens <= 0.0, z >= 0, np.floor(dens * res - f32(0.5)) + f32(2.0) <= f32(z))
    if mask_vol is not None:
        _, rgb = brick_records(mask_vol)
        inert &= rgb <= 0.0
    return ~inert


def check_field(ctx, variant, expect_active=None):
    """vr_skip_field of `variant` against the restatement: the field, the count and the box of the active bricks."""
    field, box, active = ctx.skip_field(variant)
    act = field == 0
    if expect_active is not None:
        assert np.array_equal(act, expect_active)
    assert np.array_equal(field, linf_field(act))
    assert active == int(act.sum())
    if active:
        zz, yy, xx = np.nonzero(act)
        assert box == (xx.min(), yy.min(), zz.min(), xx.max(), yy.max(), zz.max())
    else:
        assert box[3] < 0 and box[4] < 0 and box[5] < 0
    return field, box, active
