"""numpy restatement of the hull of the active bricks (csrc/vr_hull.h, vr_skip_hull): the 13 directions and the integer planes of
a brick set -- the smallest / largest n . b over its bricks b, per direction -- from a distance field (0 = active) or a mask."""
import numpy as np

DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1),
                 (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)], dtype=np.int64)
INT_MAX, INT_MIN = 2**31 - 1, -2**31


def planes_of_set(active):
    """active: bool[bnz, bny, bnx].  Returns (lo[13], hi[13]) as tuples of ints; INT_MAX / INT_MIN when the set is empty."""
    bz, by, bx = np.nonzero(active)
    if len(bx) == 0:
        return (INT_MAX,) * 13, (INT_MIN,) * 13
    proj = np.stack([bx, by, bz], 1).astype(np.int64) @ DIRS.T
    return tuple(int(v) for v in proj.min(0)), tuple(int(v) for v in proj.max(0))


def planes_of_field(field):
    """The planes of the active bricks of a distance field as Context.skip_field returns it (uint8[bnz, bny, bnx])."""
    return planes_of_set(np.asarray(field) == 0)
