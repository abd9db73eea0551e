"""CPU side of region growing (vr_segment_grow, include/vr.h): the restatement the GPU tests compare against (grow_ref.py) pinned on
hand-made cases and against scipy.ndimage.label, and the layouts of vr_grow_desc / vr_grow_result against the ctypes binding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grow_cases as gc
import grow_ref as gr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN, INF = float("nan"), float("inf")


def test_constants_match_the_binding():
    assert (gr.FACES, gr.ALL, gr.REPLACE, gr.ADD) == (capi.GROW_FACES, capi.GROW_ALL, capi.GROW_REPLACE, capi.GROW_ADD)
    assert len(gr.offsets(gr.FACES)) == 6 and len(gr.offsets(gr.ALL)) == 26
    assert (1, 1, 0) in gr.offsets(gr.ALL) and (1, 1, 0) not in gr.offsets(gr.FACES)


def test_hand_made_line_and_diagonal():
    a = np.zeros((3, 4, 5), f32)
    a[0, 0, 0:3] = 1.0          # a line along x
    a[1, 1, 3] = 1.0            # touches its end (2, 0, 0) at a corner only
    a[2, 3, 4] = 1.0            # isolated
    box = gc.whole(a.shape)
    out, n, bb, nbox, r, q = gr.grow(a, None, 2, 0.5, 1.5, gr.FACES, gr.REPLACE, *box, [(0, 0, 0)])
    assert n == 3 and bb == ((0, 0, 0), (3, 1, 1)) and nbox == 60 and int(q.sum()) == 5
    assert np.array_equal(out[..., 2], np.where(r, f32(1.0), f32(0.0))) and not out[..., [0, 1, 3]].any()
    out, n, bb, _, r, _ = gr.grow(a, None, 2, 0.5, 1.5, gr.ALL, gr.REPLACE, *box, [(0, 0, 0)])
    assert n == 4 and bb == ((0, 0, 0), (4, 2, 2)) and r[1, 1, 3] and not r[2, 3, 4]
    # two seeds, one of them not in Q, one outside the box, one a duplicate
    out, n, bb, _, r, _ = gr.grow(a, None, 0, 0.5, 1.5, gr.FACES, gr.REPLACE, *box, [(4, 3, 2), (1, 1, 1), (4, 3, 2)])
    assert n == 1 and bb == ((4, 3, 2), (5, 4, 3))
    _, n, bb, nbox, _, _ = gr.grow(a, None, 0, 0.5, 1.5, gr.FACES, gr.REPLACE, (0, 0, 0), (2, 4, 3), [(0, 0, 0), (4, 3, 2)])
    assert n == 2 and bb == ((0, 0, 0), (2, 1, 1)) and nbox == 24  # the box wall stops the line; the seed outside adds nothing


def test_hand_made_bounds_and_modes():
    a = np.array([[[0.0, 1.0, NAN, 1.0, -0.0, INF, -INF]]], f32)
    box = gc.whole(a.shape)
    assert gr.grow(a, None, 0, 1.0, 0.0, gr.FACES, gr.REPLACE, *box, [(1, 0, 0)])[1] == 0     # lo > hi
    assert gr.grow(a, None, 0, NAN, 2.0, gr.FACES, gr.REPLACE, *box, [(1, 0, 0)])[1] == 0     # a NaN bound
    assert gr.grow(a, None, 0, 0.0, NAN, gr.FACES, gr.REPLACE, *box, [(1, 0, 0)])[1] == 0
    r = gr.grow(a, None, 0, -INF, INF, gr.FACES, gr.REPLACE, *box, [(0, 0, 0), (6, 0, 0)])[4]   # NaN splits the row
    assert r[0, 0].tolist() == [True, True, False, True, True, True, True]
    assert gr.grow(a, None, 0, 0.0, 0.0, gr.FACES, gr.REPLACE, *box, [(4, 0, 0)])[1] == 1     # -0 >= +0
    # ADD keeps the other voxels' bits, REPLACE clears them; the other components keep theirs in both
    m = np.zeros(a.shape + (4,), f32)
    m[..., 1] = [2.0, NAN, -0.0, 5.0, 0.0, 1.0, -3.0]
    m[..., 0] = NAN
    m[..., 3] = f32(-0.0)
    add = gr.grow(a, m, 1, 1.0, 1.0, gr.FACES, gr.ADD, *box, [(1, 0, 0)])[0]
    want = m.copy()
    want[0, 0, 1, 1] = 1.0
    assert np.array_equal(add.view(np.uint32), want.view(np.uint32))
    rep = gr.grow(a, m, 1, 1.0, 1.0, gr.FACES, gr.REPLACE, *box, [(1, 0, 0)])[0]
    want[..., 1] = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(rep.view(np.uint32), want.view(np.uint32))


def test_snake_is_one_path():
    a, first, last, length = gc.snake(24)
    assert int((a != 0).sum()) == length
    for conn in (gr.FACES, gr.ALL):
        _, n, bb, _, r, q = gr.grow(a, None, 0, 0.5, 1.5, conn, gr.REPLACE, *gc.whole(a.shape), [first])
        assert n == length and r[last[2], last[1], last[0]] and np.array_equal(r, q)
    # it passes through every 4^3 brick
    assert (a.reshape(6, 4, 6, 4, 6, 4).max(axis=(1, 3, 5)) == 1.0).all()


@pytest.mark.parametrize("conn", [gr.FACES, gr.ALL])
@pytest.mark.parametrize("shape", [gc.SMALL, gc.LARGE])
def test_restatement_equals_scipy_label(shape, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    v, lo, hi = gc.noise_case(shape, conn)
    a = v[..., 3]
    structure = np.ones((3, 3, 3), int) if conn == gr.ALL else ndi.generate_binary_structure(3, 1)
    boxes = [gc.whole(shape)] + ([((1, 2, 3), (22, 17, 12)), ((4, 8, 4), (8, 12, 8))] if shape == gc.SMALL else [])
    for box in boxes:
        q = gr.qualifies(a, lo, hi, *box)
        labels, count = ndi.label(q, structure=structure)
        assert count > (10 if box == gc.whole(shape) else 1)
        for n_seeds in (1, 3, 64):
            seeds = gc.seeds_from(q, n_seeds, seed=n_seeds) + gc.seeds_from(q, 2, seed=5, want=False)
            hit = {int(labels[z, y, x]) for x, y, z in seeds} - {0}
            want = np.isin(labels, sorted(hit)) & (labels != 0)
            _, n, bb, nbox, r, q2 = gr.grow(a, None, 0, lo, hi, conn, gr.REPLACE, *box, seeds)
            assert np.array_equal(r, want) and np.array_equal(q, q2) and n == int(want.sum())
            z, y, x = np.nonzero(want)
            assert bb == ((x.min(), y.min(), z.min()), (x.max() + 1, y.max() + 1, z.max() + 1))


@pytest.mark.parametrize("conn", [gr.FACES, gr.ALL])
def test_noise_cases_have_one_large_component_among_many(conn):
    """What the GPU test relies on: at the connectivity's quantile the largest component is tortuous and far from all of Q."""
    v, lo, hi = gc.noise_case(gc.SMALL, conn)
    q = gr.qualifies(v[..., 3], lo, hi, *gc.whole(gc.SMALL))
    seed, n = gc.largest_component_seed(q, conn)
    assert 100 < n < int(q.sum()) and q[seed[2], seed[1], seed[0]]


def test_grow_struct_layouts_match_header(tmp_path):
    fields_d = ["volume_slot", "channel", "mask_slot", "contour", "lo", "hi", "connectivity", "mode", "box_lo", "box_hi", "n_seeds", "seeds"]
    fields_r = ["voxels", "lo", "hi", "rounds"]
    args = ["sizeof(vr_grow_desc)"] + [f"offsetof(vr_grow_desc, {f})" for f in fields_d]
    args += ["sizeof(vr_grow_result)"] + [f"offsetof(vr_grow_result, {f})" for f in fields_r]
    args += ["(size_t)VR_GROW_FACES", "(size_t)VR_GROW_ALL", "(size_t)VR_GROW_REPLACE", "(size_t)VR_GROW_ADD", "(size_t)VR_GROW_MAX_SEEDS",
             "(size_t)VR_GROW_BATCH", "(size_t)VR_ABI_VERSION"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' +
                   "".join(f'printf("%zu ", {a});' for a in args) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, R = capi.GrowDesc, capi.GrowResult
    want = [C.sizeof(D)] + [getattr(D, f).offset for f in fields_d] + [C.sizeof(R)] + [getattr(R, f).offset for f in fields_r]
    want += [capi.GROW_FACES, capi.GROW_ALL, capi.GROW_REPLACE, capi.GROW_ADD, capi.GROW_MAX_SEEDS, capi.GROW_BATCH, 1]
    assert out == want
    assert C.sizeof(D) == 4 * (8 + 6 + 1 + 3 * 64)


def test_grow_desc_copy():
    d = capi.GrowDesc()
    e = d.copy(volume_slot=2, lo=-1.5, box_hi=(3, 4, 5), seeds=[(1, 2, 3), (4, 5, 6)])
    assert (e.volume_slot, e.lo, list(e.box_hi), e.n_seeds) == (2, -1.5, [3, 4, 5], 2)
    assert list(e.seeds[1]) == [4, 5, 6] and list(e.seeds[2]) == [0, 0, 0] and d.n_seeds == 0
    assert e.copy(seeds=[(7, 8, 9)], n_seeds=5).n_seeds == 5
