"""The brick-index limit of the skipping kernels (include/vr.h: THE BRICK-INDEX LIMIT), on the CPU.

brick_of (csrc/vr_kernels.h) and slice_record (csrc/vr_slice.h) compute mul24(mul24(bz, bny) + by, bnx) + bx.  On gfx950 that is
the SIGNED 24-bit multiply: each operand is sign-extended from its low 24 bits, the low 32 bits of the product are kept.  The
emulation below restates that; the host's rule (vr_skip_indexable, which every skipping launch goes through) must accept a grid
only where the emulated index is the true one, and the grid that the former rule -- bnx * bny < 2^23 -- let through shows why."""
import numpy as np
import pytest

from volumerendering_amd import capi


def sext24(x):
    x = np.asarray(x, dtype=np.int64) & 0xFFFFFF
    return np.where(x & 0x800000, x - 0x1000000, x)


def wrap32(x):
    x = np.asarray(x, dtype=np.int64) & 0xFFFFFFFF
    return np.where(x & 0x80000000, x - 0x100000000, x)


def mul24(a, b):
    return wrap32(sext24(a) * sext24(b))


def emulated_index(bx, by, bz, bnx, bny):
    return wrap32(mul24(wrap32(mul24(bz, bny) + by), bnx) + bx)


def true_index(bx, by, bz, bnx, bny):
    return (np.asarray(bz, np.int64) * bny + by) * bnx + bx


def probe_bricks(bnx, bny, bnz):
    """The eight corner bricks, and the bricks whose row index bz * bny + by is 2^23 - 1 (if the grid has such a row)."""
    out = [(x, y, z) for x in (0, bnx - 1) for y in (0, bny - 1) for z in (0, bnz - 1)]
    row = (1 << 23) - 1
    if row < bny * bnz:
        out += [(x, row % bny, row // bny) for x in (0, bnx - 1)]
    return out


def indexable(bnx, bny, bnz):
    """The host's rule, asked with the smallest volume of that many bricks per axis."""
    return capi.Context.skip_indexable(4 * bnx - 3, 4 * bny - 3, 4 * bnz - 3)


# (bnx, bny, bnz): the limits of each operand and of the byte offset from either side, and ordinary grids
GRIDS = [(1, 2048, 4096), (16384, 16, 1), (4096, 2048, 1), (2, 2, 2), (1, 4096, 2048), (64, 2048, 4096), (65, 2048, 4096),
         (16384, 1, 1), (1, 16384, 1), (1, 1, 16384), (16384, 16384, 1), (16384, 16384, 2), (16384, 16384, 3), (1, 2049, 4096),
         (1, 4096, 2049), (1, 16384, 16384), (16384, 2, 16384), (128, 128, 258), (812, 812, 812), (813, 813, 813), (256, 256, 256)]


def test_emulation_is_the_signed_24_bit_multiply():
    assert int(mul24(3, 5)) == 15
    assert int(mul24((1 << 23) - 1, 2)) == (1 << 24) - 2
    assert int(mul24(1 << 23, 1)) == -(1 << 23)            # bit 23 is the sign
    assert int(mul24((1 << 24) + 7, 3)) == 21              # bits above 23 are not read
    assert int(mul24((1 << 23) - 1, (1 << 23) - 1)) == int(wrap32(((1 << 23) - 1) ** 2))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_accepted_grids_index_exactly(grid):
    bnx, bny, bnz = grid
    ok = indexable(bnx, bny, bnz)
    assert ok == (bny * bnz <= 1 << 23 and bnx < 1 << 23 and bnx * bny * bnz <= 1 << 29), grid
    if not ok:
        return
    for bx, by, bz in probe_bricks(bnx, bny, bnz):
        e, t = int(emulated_index(bx, by, bz, bnx, bny)), int(true_index(bx, by, bz, bnx, bny))
        assert e == t, (grid, (bx, by, bz), e, t)
        assert 0 <= t << 3 < 1 << 32, (grid, t)  # (brick_record's 32-bit byte offset)


def test_every_brick_of_the_limit_grids_indexes_exactly():
    """All bricks of the two grids that sit on the row limit (2^23 rows exactly)."""
    for bnx, bny, bnz in [(1, 2048, 4096), (1, 4096, 2048)]:
        assert indexable(bnx, bny, bnz)
        bz, by = np.divmod(np.arange(bny * bnz, dtype=np.int64), bny)
        assert np.array_equal(emulated_index(0, by, bz, bnx, bny), true_index(0, by, bz, bnx, bny))


def test_the_grid_the_former_rule_admitted_is_refused():
    """(nx, ny, nz) = (1, 8196, 16384): 1 x 2049 x 4096 bricks.  bnx * bny = 2049 passed the former rule; the last brick's row index
    2049 * 4095 + 2048 = 8 392 703 has bit 23 set, so its index comes out negative -- an address far outside the records."""
    assert not capi.Context.skip_indexable(1, 8196, 16384)
    assert not indexable(1, 2049, 4096)
    assert capi.Context.skip_indexable(1, 8192, 16384)
    bnx, bny, bnz = 1, 2049, 4096
    assert bnx * bny < 1 << 23
    last = int(emulated_index(0, bny - 1, bnz - 1, bnx, bny))
    assert last < 0 and last != int(true_index(0, bny - 1, bnz - 1, bnx, bny))
    # ... and so do all the bricks of the top two brick slabs' upper rows: the first wrong one is row 2^23
    bz, by = np.divmod(np.arange(bny * bnz, dtype=np.int64), bny)
    wrong = emulated_index(0, by, bz, bnx, bny) != true_index(0, by, bz, bnx, bny)
    assert int(np.argmax(wrong)) == 1 << 23 and wrong[1 << 23:].all() and int(bz[1 << 23]) == bnz - 2


def test_every_cube_a_device_can_hold_is_inside():
    for n in (1, 4, 5, 1024, 2048, 3248):
        assert capi.Context.skip_indexable(n, n, n)
    assert not capi.Context.skip_indexable(3249, 3249, 3249)
