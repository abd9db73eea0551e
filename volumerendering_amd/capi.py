"""ctypes binding of the C ABI in include/vr.h (libvr_hip.so).

Plumbing only: the product is the HIP library.  There is no CPU fallback -- if the shared library is missing
or no HIP device can be opened, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvr_hip.so")

VR_OK = 0
VR_ERR_INVALID_ARG = -1
VR_ERR_HIP = -2
VR_ERR_NOT_READY = -3
VR_ERR_UNSUPPORTED = -4
VR_ERR_OOM = -5
VR_ERR_INTERNAL = -6

BASIC, LIGHT, VOLUME_MASK, THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE, LIGHT_INSHADER = range(8)
MIP, MINIP, AVERAGE = 8, 9, 10  # intensity projections of volume slot 0 (include/vr.h)
ISO = 11  # shaded isosurface of volume slot 0 at the level of Context.set_iso_value (include/vr.h)
VARIANT_NAMES = ["BASIC", "LIGHT", "VOLUME_MASK", "THREE_FILES", "MULTI_CTRT", "TF_CALIB", "ILLUSTRATIVE", "LIGHT_INSHADER",
                 "MIP", "MINIP", "AVERAGE", "ISO"]
TILE = 64
ARITH_SEPARATE, ARITH_FUSED = 0, 1
OUTPUT_COLOR, OUTPUT_SURFACE = 0, 1  # Context.set_output (include/vr.h)
MAX_VOLUMES = 3
SLICE_MAX, SLICE_MIN, SLICE_AVERAGE = 0, 1, 2  # vr_slice_desc.reduce (include/vr.h)
SLICE_LINEAR, SLICE_NEAREST = 0, 1              # vr_slice_desc.filter
SLICE_RGBA32F, SLICE_BGRA8 = 0, 1               # vr_slice_desc.format
HIST_ROWS, HIST_MAX_BINS = 5, 65536              # vr_histogram (include/vr.h)
HIST_CLAMP, HIST_DROP = 0, 1                     # vr_hist_desc.out_of_range
GROW_FACES, GROW_ALL = 6, 26                     # vr_grow_desc.connectivity (include/vr.h)
GROW_REPLACE, GROW_ADD = 0, 1                    # vr_grow_desc.mode
GROW_MAX_SEEDS = 64
GROW_BATCH = 8                                   # propagation rounds enqueued between two looks at the outcome (VR_GROW_BATCH)
MORPH_MAX_RADIUS = 31                            # vr_morph_element (include/vr.h)
MORPH_NONE, MORPH_DILATE, MORPH_ERODE, MORPH_CLOSE, MORPH_OPEN = range(5)   # vr_morph_desc.op
MORPH_REPLACE, MORPH_OR, MORPH_AND, MORPH_ANDNOT = range(4)                 # vr_morph_desc.combine
DIST_OUTSIDE, DIST_INSIDE, DIST_SIGNED = range(3)                           # vr_dist_desc.mode (include/vr.h)
POLY_EVEN_ODD, POLY_UNION = 0, 1                                            # vr_polygons_desc.rule (include/vr.h)
POLY_MAX_COORD, POLY_MAX_SPACING = 1 << 29, 1 << 20                         # of a point coordinate or origin value (magnitude), a spacing
OUTLINE_SPLIT, OUTLINE_JOIN = 0, 1                                          # vr_outlines_desc.connect (include/vr.h)
COMP_FACES, COMP_ALL, COMP_PLANE_FACES, COMP_PLANE_ALL = 6, 26, 4, 8              # vr_components_desc.connectivity (include/vr.h)
COMP_MAX_KEEP, COMP_MAX_LABEL = 64, 1 << 24                                 # of keep_largest; of n_components with a label map
RESAMPLE_LINEAR, RESAMPLE_NEAREST = 0, 1                                    # vr_resample_desc.filter (include/vr.h)
FILTER_MAX_RADIUS = 32                                                      # of vr_filter_desc.radius (include/vr.h)
FILTER_CLAMP, FILTER_CONSTANT = 0, 1                                        # vr_filter_desc.border
RANK_MAX_RADIUS = 3                                                         # of vr_rank_desc.radius (include/vr.h)
RANK_MIN, RANK_MEDIAN, RANK_MAX = 0, -1, -2                                 # vr_rank_desc.rank: 0 .. N - 1, or N / 2, or N - 1
GAMMA_MAX_SUB, GAMMA_MAX_RADIUS = 4, 8                                      # of vr_gamma_desc.sub, of reach / spacing (include/vr.h)
GAMMA_GLOBAL, GAMMA_LOCAL = 0, 1                                            # vr_gamma_desc.mode
DIST_MAX_SPACING, DIST_MAX_LIMIT, DIST_MAX_EXTENT = 1 << 20, 1 << 31, 1 << 30  # of a spacing, the limit, (hi - lo) * spacing per axis

# every symbol include/vr.h declares (tests check that the library exports each of them)
ABI_SYMBOLS = [
    "vr_create", "vr_resize", "vr_destroy", "vr_last_error", "vr_abi_version", "vr_volume_upload",
    "vr_volume_upload_device", "vr_volume_upload_raw16", "vr_volume_upload_raw32", "vr_volume_normalize",
    "vr_volume_precompute_gradient", "vr_volume_download", "vr_tf_upload", "vr_tf_upload_opacity", "vr_tf_upload_color", "vr_set_uniforms", "vr_render", "vr_render_tiles", "vr_tile_count",
    "vr_render_async", "vr_render_tiles_async", "vr_unpack_tiles_async", "vr_download", "vr_download_tiles",
    "vr_render_batch_async", "vr_render_tiles_batch_async", "vr_unpack_tiles_strided_async",
    "vr_last_timing", "vr_kernel_times", "vr_reset_kernel_times", "vr_frame_device_ptr", "vr_last_covered_pixels", "vr_last_counters", "vr_set_kernel_flavour", "vr_last_block_trace", "vr_last_kernel_flavour",
    "vr_set_volume_layout", "vr_volume_layout", "vr_viewport", "vr_set_arithmetic", "vr_present_async", "vr_stream", "vr_hint_frames_in_flight",
    "vr_set_kernel_timing", "vr_present_tiles_async", "vr_kernel_choice",
    "vr_present_packed_async", "vr_unpack_tiles_bgra8_async",
    "vr_tf_upload_opacity_async", "vr_tf_upload_color_async", "vr_skip_field", "vr_skip_hull", "vr_skip_indexable", "vr_unbounded_box_launches",
    "vr_set_iso_value", "vr_set_shadows", "vr_shadow_volume",
    "vr_set_output", "vr_set_surface_threshold", "vr_surface_depth_async", "vr_pick",
    "vr_set_ray_bounds",
    "vr_slice_async", "vr_slice_render", "vr_slice_orthogonal", "vr_slice_counters",
    "vr_hist_whole", "vr_histogram_async", "vr_histogram", "vr_hist_counters",
    "vr_grow_whole", "vr_segment_grow", "vr_grow_counters", "vr_grow_timing",
    "vr_morph_ball", "vr_morph_box", "vr_morph_whole", "vr_mask_morph", "vr_morph_counters", "vr_morph_timing",
    "vr_dist_whole", "vr_mask_distance", "vr_dist_counters", "vr_dist_timing",
    "vr_polygons_whole", "vr_mask_polygons", "vr_polygons_counters", "vr_polygons_timing",
    "vr_outlines_whole", "vr_mask_outlines", "vr_outlines_counters", "vr_outlines_timing",
    "vr_components_whole", "vr_mask_components", "vr_components_counters", "vr_components_timing",
    "vr_resample_identity", "vr_resample_between", "vr_volume_resample", "vr_resample_counters", "vr_resample_timing",
    "vr_mesh_whole", "vr_volume_mesh", "vr_mesh_counters", "vr_mesh_timing",
    "vr_filter_whole", "vr_filter_gaussian", "vr_volume_filter", "vr_filter_counters", "vr_filter_timing",
    "vr_rank_whole", "vr_volume_rank", "vr_rank_counters", "vr_rank_timing",
    "vr_gamma_whole", "vr_volume_gamma", "vr_gamma_counters", "vr_gamma_timing",
]


class Uniforms(C.Structure):
    """struct vr_uniforms (include/vr.h)."""
    _fields_ = [
        ("model", C.c_float * 16), ("view", C.c_float * 16), ("proj", C.c_float * 16),
        ("view_inv", C.c_float * 16), ("proj_inv", C.c_float * 16),
        ("camera_pos", C.c_float * 3),
        ("fragment_mode", C.c_int32), ("steps_count", C.c_int32), ("step_size", C.c_float),
        ("clip_x", C.c_float * 2), ("clip_y", C.c_float * 2), ("clip_z", C.c_float * 2),
        ("toggles", C.c_int32 * 4),
        ("light_pos", C.c_float * 4), ("light_ambient", C.c_float * 4), ("light_diffuse", C.c_float * 4),
    ]


class PickResult(C.Structure):
    """struct vr_pick_result (include/vr.h)."""
    _fields_ = [
        ("hit", C.c_int32), ("uvw", C.c_float * 3), ("world", C.c_float * 3), ("depth", C.c_float), ("alpha", C.c_float),
        ("voxel", C.c_int32 * 3), ("value", (C.c_float * 4) * MAX_VOLUMES),
    ]

    def as_dict(self) -> dict:
        """The record as plain numpy values (float32 / int32), for comparisons."""
        return dict(hit=int(self.hit), uvw=np.array(self.uvw, np.float32), world=np.array(self.world, np.float32),
                    depth=np.float32(self.depth), alpha=np.float32(self.alpha), voxel=np.array(self.voxel, np.int32),
                    value=np.array([list(v) for v in self.value], np.float32))


class SliceDesc(C.Structure):
    """struct vr_slice_desc (include/vr.h): a plane in texture space, its output size, slab, reduction, filter and format."""
    _fields_ = [
        ("volume_slot", C.c_int32), ("tf_slot", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("dn", C.c_float * 3),
        ("slab_steps", C.c_int32), ("reduce", C.c_int32), ("filter", C.c_int32), ("format", C.c_int32),
    ]

    def copy(self, **over) -> "SliceDesc":
        """A copy with the given fields replaced (vectors from any sequence of three floats)."""
        d = SliceDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("origin", "du", "dv", "dn"):
                v = (C.c_float * 3)(*[float(x) for x in v])
            setattr(d, k, v)
        return d


class HistDesc(C.Structure):
    """struct vr_hist_desc (include/vr.h): the value slot and channel, the mask, the rows, the binning and the voxel box."""
    _fields_ = [
        ("volume_slot", C.c_int32), ("channel", C.c_int32), ("mask_slot", C.c_int32), ("rows", C.c_uint32), ("bins", C.c_uint32),
        ("scale", C.c_float), ("out_of_range", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
    ]

    def copy(self, **over) -> "HistDesc":
        """A copy with the given fields replaced (lo / hi from any sequence of three integers)."""
        d = HistDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("lo", "hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class HistRow(C.Structure):
    """struct vr_hist_row: voxels = counted + dropped."""
    _fields_ = [("voxels", C.c_uint64), ("dropped", C.c_uint64)]


class GrowDesc(C.Structure):
    """struct vr_grow_desc (include/vr.h): the value slot and channel, the mask slot and contour, the bounds, the connectivity, the
    mode, the voxel box and the seeds."""
    _fields_ = [
        ("volume_slot", C.c_int32), ("channel", C.c_int32), ("mask_slot", C.c_int32), ("contour", C.c_int32),
        ("lo", C.c_float), ("hi", C.c_float), ("connectivity", C.c_int32), ("mode", C.c_int32),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("n_seeds", C.c_uint32), ("seeds", (C.c_int32 * 3) * GROW_MAX_SEEDS),
    ]

    def copy(self, **over) -> "GrowDesc":
        """A copy with the given fields replaced (box_lo / box_hi from any sequence of three integers; seeds from a sequence of at
        most 64 (x, y, z), which sets n_seeds too unless that is given as well)."""
        d = GrowDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k == "seeds":
                v = [tuple(int(x) for x in p) for p in v]
                assert len(v) <= GROW_MAX_SEEDS
                if "n_seeds" not in over:
                    d.n_seeds = len(v)
                v = ((C.c_int32 * 3) * GROW_MAX_SEEDS)(*[(C.c_int32 * 3)(*p) for p in v])
            setattr(d, k, v)
        return d


class GrowResult(C.Structure):
    """struct vr_grow_result: |R|, its half-open bounding box (zeros when empty) and the propagation rounds."""
    _fields_ = [("voxels", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("rounds", C.c_uint32)]

    def as_tuple(self):
        return int(self.voxels), tuple(int(x) for x in self.lo), tuple(int(x) for x in self.hi)


class MorphElement(C.Structure):
    """struct vr_morph_element (include/vr.h): the radii (rx, ry, rz) and the half-chords along x, half[dz + rz][dy + ry]."""
    _fields_ = [("radius", C.c_int32 * 3), ("half", (C.c_int8 * (2 * MORPH_MAX_RADIUS + 1)) * (2 * MORPH_MAX_RADIUS + 1))]

    def table(self) -> np.ndarray:
        """The used window of the half-chords as an int8 array [2 rz + 1][2 ry + 1]."""
        rx, ry, rz = (int(r) for r in self.radius)
        return np.ctypeslib.as_array(self.half)[:2 * rz + 1, :2 * ry + 1].copy()


class MorphDesc(C.Structure):
    """struct vr_morph_desc (include/vr.h): the source slot and contour, the destination slot and contour, the operator, the way the
    result is stored, the voxel box and the structuring element."""
    _fields_ = [
        ("src_slot", C.c_int32), ("src_contour", C.c_int32), ("dst_slot", C.c_int32), ("dst_contour", C.c_int32),
        ("op", C.c_int32), ("combine", C.c_int32), ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("element", MorphElement),
    ]

    def copy(self, **over) -> "MorphDesc":
        """A copy with the given fields replaced (box_lo / box_hi from any sequence of three integers; element from a MorphElement,
        which is copied)."""
        d = MorphDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k == "element":
                v = MorphElement.from_buffer_copy(bytes(v))
            setattr(d, k, v)
        return d


class MorphResult(C.Structure):
    """struct vr_morph_result: |R|, |A'| and the half-open bounding box of R (zeros when empty)."""
    _fields_ = [("voxels", C.c_uint64), ("src_voxels", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]

    def as_tuple(self):
        return int(self.voxels), int(self.src_voxels), tuple(int(x) for x in self.lo), tuple(int(x) for x in self.hi)


class DistDesc(C.Structure):
    """struct vr_dist_desc (include/vr.h): the source slot and contour, the destination slot and channel, the mode, the probe, the limit,
    the voxel spacing, the scale and the voxel box."""
    _fields_ = [
        ("src_slot", C.c_int32), ("src_contour", C.c_int32), ("dst_slot", C.c_int32), ("dst_channel", C.c_int32), ("mode", C.c_int32),
        ("probe_slot", C.c_int32), ("probe_contour", C.c_int32), ("limit", C.c_uint32), ("spacing", C.c_uint32 * 3), ("scale", C.c_float),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
    ]

    def copy(self, **over) -> "DistDesc":
        """A copy with the given fields replaced (box_lo / box_hi / spacing from any sequence of three integers)."""
        d = DistDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k == "spacing":
                v = (C.c_uint32 * 3)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class DistResult(C.Structure):
    """struct vr_dist_result: |A'|, its half-open bounding box (zeros when empty), the voxels that store BEYOND's value, and the probe's
    voxel count and exact minimum / maximum of D2out (BEYOND = 2^64 - 1; zeros without a probe voxel)."""
    _fields_ = [("src_voxels", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("beyond", C.c_uint64),
                ("probe_voxels", C.c_uint64), ("probe_min_sq", C.c_uint64), ("probe_max_sq", C.c_uint64)]

    def as_tuple(self):
        return (int(self.src_voxels), tuple(int(x) for x in self.lo), tuple(int(x) for x in self.hi), int(self.beyond),
                int(self.probe_voxels), int(self.probe_min_sq), int(self.probe_max_sq))


class Polygon(C.Structure):
    """struct vr_polygon (include/vr.h): points[first .. first + count) on slice `slice`, for contour `contour`."""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("slice", C.c_int32), ("contour", C.c_int32)]


class PolygonsDesc(C.Structure):
    """struct vr_polygons_desc (include/vr.h): the grid and destination slots, the contours written, the rule, the way the result is
    stored, the voxel box, the grid's origin and spacing, and the points and polygons (set by Context.mask_polygons)."""
    _fields_ = [
        ("grid_slot", C.c_int32), ("dst_slot", C.c_int32), ("contours", C.c_int32), ("rule", C.c_int32), ("combine", C.c_int32),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("origin", C.c_int32 * 2), ("spacing", C.c_uint32 * 2),
        ("n_points", C.c_uint32), ("n_polygons", C.c_uint32), ("points", C.c_void_p), ("polygons", C.c_void_p),
    ]

    def copy(self, **over) -> "PolygonsDesc":
        """A copy with the given fields replaced (box_lo / box_hi from any sequence of three integers, origin / spacing of two)."""
        d = PolygonsDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k == "origin":
                v = (C.c_int32 * 2)(*[int(x) for x in v])
            if k == "spacing":
                v = (C.c_uint32 * 2)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class PolygonsResult(C.Structure):
    """struct vr_polygons_result: per contour |R_k| and its half-open bounding box (zeros when empty or not written)."""
    _fields_ = [("voxels", C.c_uint64 * 4), ("lo", (C.c_int32 * 3) * 4), ("hi", (C.c_int32 * 3) * 4)]

    def as_tuple(self):
        """((voxels, lo, hi) of contour 0, ... of contour 3)"""
        return tuple((int(self.voxels[k]), tuple(int(x) for x in self.lo[k]), tuple(int(x) for x in self.hi[k])) for k in range(4))


class OutlinesDesc(C.Structure):
    """struct vr_outlines_desc (include/vr.h): the source slot, the contours traced, the connect rule, the voxel box, the grid's origin,
    spacing and offset, and the capacities and arrays of the output (set by Context.mask_outlines)."""
    _fields_ = [
        ("src_slot", C.c_int32), ("contours", C.c_int32), ("connect", C.c_int32),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("origin", C.c_int32 * 2), ("spacing", C.c_uint32 * 2), ("offset", C.c_uint32 * 2),
        ("max_points", C.c_uint32), ("max_polygons", C.c_uint32), ("points", C.c_void_p), ("polygons", C.c_void_p),
    ]

    def copy(self, **over) -> "OutlinesDesc":
        """A copy with the given fields replaced (box_lo / box_hi from any sequence of three integers, origin / spacing / offset of two)."""
        d = OutlinesDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k == "origin":
                v = (C.c_int32 * 2)(*[int(x) for x in v])
            if k in ("spacing", "offset"):
                v = (C.c_uint32 * 2)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class OutlinesResult(C.Structure):
    """struct vr_outlines_result: the points and polygons the mask needs, and per contour its polygons, points and twice its area."""
    _fields_ = [("n_points", C.c_uint32), ("n_polygons", C.c_uint32), ("polygons_of", C.c_uint32 * 4), ("points_of", C.c_uint32 * 4),
                ("area2", C.c_int64 * 4)]

    def as_tuple(self):
        """(n_points, n_polygons, polygons_of, points_of, area2)"""
        return (int(self.n_points), int(self.n_polygons), tuple(int(x) for x in self.polygons_of), tuple(int(x) for x in self.points_of),
                tuple(int(x) for x in self.area2))


class MeshDesc(C.Structure):
    """struct vr_mesh_desc (include/vr.h): the source slot and its component, the level, the cap, the voxel box, and the capacities and
    arrays of the output (set by Context.volume_mesh)."""
    _fields_ = [
        ("src_slot", C.c_int32), ("channel", C.c_int32), ("level", C.c_float), ("cap", C.c_int32),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
        ("max_vertices", C.c_uint32), ("max_triangles", C.c_uint32), ("vertices", C.c_void_p), ("triangles", C.c_void_p),
    ]

    def copy(self, **over) -> "MeshDesc":
        """A copy with the given fields replaced (box_lo / box_hi from any sequence of three integers)."""
        d = MeshDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class MeshResult(C.Structure):
    """struct vr_mesh_result: the vertices and triangles the surface needs, the inside points of the box, the cells that emit and the
    half-open box of their origins (zeros when there are none)."""
    _fields_ = [("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("inside", C.c_uint64), ("cells", C.c_uint64),
                ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]

    def as_tuple(self):
        """(n_vertices, n_triangles, inside, cells, lo, hi)"""
        return (int(self.n_vertices), int(self.n_triangles), int(self.inside), int(self.cells), tuple(int(x) for x in self.lo),
                tuple(int(x) for x in self.hi))


class FilterDesc(C.Structure):
    """struct vr_filter_desc (include/vr.h): the source and destination slots and channels, per axis the radius and the weights (set by
    Context.volume_filter from its `taps`), the border rule and value, and the voxel box of the output."""
    _fields_ = [
        ("src_slot", C.c_int32), ("src_channel", C.c_int32), ("dst_slot", C.c_int32), ("dst_channel", C.c_int32),
        ("radius", C.c_int32 * 3), ("taps", C.c_void_p * 3), ("border", C.c_int32), ("border_value", C.c_float),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
    ]

    def copy(self, **over) -> "FilterDesc":
        """A copy with the given fields replaced (radius / box_lo / box_hi from any sequence of three integers, taps from three
        addresses or None)."""
        d = FilterDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("radius", "box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k == "taps":
                v = (C.c_void_p * 3)(*v)
            setattr(d, k, v)
        return d


class FilterResult(C.Structure):
    """struct vr_filter_result: the voxels of the box, those stored as NaN or +-inf, the least and greatest finite stored value."""
    _fields_ = [("stored", C.c_uint64), ("nonfinite", C.c_uint64), ("lo_value", C.c_float), ("hi_value", C.c_float)]

    def as_tuple(self):
        """(stored, nonfinite, the bits of lo_value, the bits of hi_value)"""
        lo, hi = np.array([self.lo_value, self.hi_value], np.float32).view(np.uint32)
        return int(self.stored), int(self.nonfinite), int(lo), int(hi)


class RankDesc(C.Structure):
    """struct vr_rank_desc (include/vr.h): the source and destination slots and channels, the radius per axis, the rank (0 .. N - 1 or
    RANK_MEDIAN / RANK_MAX), the border rule and value, and the voxel box of the output."""
    _fields_ = [
        ("src_slot", C.c_int32), ("src_channel", C.c_int32), ("dst_slot", C.c_int32), ("dst_channel", C.c_int32),
        ("radius", C.c_int32 * 3), ("rank", C.c_int32), ("border", C.c_int32), ("border_value", C.c_float),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
    ]

    def copy(self, **over) -> "RankDesc":
        """A copy with the given fields replaced (radius / box_lo / box_hi from any sequence of three integers)."""
        d = RankDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("radius", "box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class RankResult(C.Structure):
    """struct vr_rank_result: the voxels of the box, those stored as NaN or +-inf, those whose stored bits differ from the source's at
    the same voxel, the least and greatest finite stored value."""
    _fields_ = [("stored", C.c_uint64), ("nonfinite", C.c_uint64), ("changed", C.c_uint64), ("lo_value", C.c_float), ("hi_value", C.c_float)]

    def as_tuple(self):
        """(stored, nonfinite, changed, the bits of lo_value, the bits of hi_value)"""
        lo, hi = np.array([self.lo_value, self.hi_value], np.float32).view(np.uint32)
        return int(self.stored), int(self.nonfinite), int(self.changed), int(lo), int(hi)


class GammaDesc(C.Structure):
    """struct vr_gamma_desc (include/vr.h): the reference, evaluated and destination slots and channels, the ROI (roi_slot -1: none),
    the spacing, dta and reach in one integer unit, the sub-steps per voxel, the mode, the tolerance, the cutoff, what a skipped voxel
    stores, and the voxel box of the output."""
    _fields_ = [
        ("ref_slot", C.c_int32), ("ref_channel", C.c_int32), ("eval_slot", C.c_int32), ("eval_channel", C.c_int32),
        ("dst_slot", C.c_int32), ("dst_channel", C.c_int32), ("roi_slot", C.c_int32), ("roi_contour", C.c_int32),
        ("spacing", C.c_uint32 * 3), ("dta", C.c_uint32), ("reach", C.c_uint32), ("sub", C.c_int32), ("mode", C.c_int32),
        ("dose_tolerance", C.c_float), ("cutoff", C.c_float), ("skip_value", C.c_float),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
    ]

    def copy(self, **over) -> "GammaDesc":
        """A copy with the given fields replaced (spacing / box_lo / box_hi from any sequence of three integers; skip_bits sets the
        bits of skip_value, which a conversion through a Python float would not keep for a signalling NaN)."""
        d = GammaDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k == "skip_bits":
                C.c_uint32.from_address(C.addressof(d) + GammaDesc.skip_value.offset).value = int(v)
                continue
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            elif k == "spacing":
                v = (C.c_uint32 * 3)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class GammaResult(C.Structure):
    """struct vr_gamma_result: the voxels of the box, those evaluated, those that pass (G2 <= 1), those stored as NaN or +inf, the
    greatest finite stored value of an evaluated voxel."""
    _fields_ = [("stored", C.c_uint64), ("evaluated", C.c_uint64), ("passed", C.c_uint64), ("nonfinite", C.c_uint64),
                ("hi_value", C.c_float), ("reserved", C.c_uint32)]

    def as_tuple(self):
        """(stored, evaluated, passed, nonfinite, the bits of hi_value)"""
        hi = np.array([self.hi_value], np.float32).view(np.uint32)[0]
        return int(self.stored), int(self.evaluated), int(self.passed), int(self.nonfinite), int(hi)


class Component(C.Structure):
    """struct vr_component (include/vr.h): a component's voxels, half-open bounding box, first voxel (x, y, z) and the faces of the box
    it touches."""
    _fields_ = [("voxels", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("first", C.c_int32 * 3), ("faces", C.c_uint32)]

    def as_tuple(self):
        """(voxels, lo, hi, first, faces)"""
        return (int(self.voxels), tuple(int(x) for x in self.lo), tuple(int(x) for x in self.hi), tuple(int(x) for x in self.first),
                int(self.faces))


class ComponentsDesc(C.Structure):
    """struct vr_components_desc (include/vr.h): the set (slot, contour, background), the connectivity, the voxel box, the selection
    (size window, rejected faces, keep_largest), the contour and label-map destinations, and the table's capacity and array (set by
    Context.mask_components)."""
    _fields_ = [
        ("src_slot", C.c_int32), ("src_contour", C.c_int32), ("background", C.c_int32), ("connectivity", C.c_int32),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("min_voxels", C.c_uint64), ("max_voxels", C.c_uint64),
        ("reject_faces", C.c_uint32), ("keep_largest", C.c_uint32), ("dst_slot", C.c_int32), ("dst_contour", C.c_int32),
        ("combine", C.c_int32), ("label_slot", C.c_int32), ("label_channel", C.c_int32), ("max_components", C.c_uint32),
        ("components", C.c_void_p),
    ]

    def copy(self, **over) -> "ComponentsDesc":
        """A copy with the given fields replaced (box_lo / box_hi from any sequence of three integers)."""
        d = ComponentsDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            setattr(d, k, v)
        return d


class ComponentsResult(C.Structure):
    """struct vr_components_result: the components and how many are selected, |S|, |R|, the biggest component's voxels and the half-open
    bounding box of R (zeros when R is empty)."""
    _fields_ = [("n_components", C.c_uint64), ("n_selected", C.c_uint64), ("voxels", C.c_uint64), ("selected_voxels", C.c_uint64),
                ("largest", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]

    def as_tuple(self):
        """(n_components, n_selected, voxels, selected_voxels, largest, lo, hi)"""
        return (int(self.n_components), int(self.n_selected), int(self.voxels), int(self.selected_voxels), int(self.largest),
                tuple(int(x) for x in self.lo), tuple(int(x) for x in self.hi))


class ResampleDesc(C.Structure):
    """struct vr_resample_desc (include/vr.h): the source and destination slots, the components written, the filter, the destination
    grid, the affine map of its voxels into the source's texture space, the values stored outside the source and the voxel box."""
    _fields_ = [
        ("src_slot", C.c_int32), ("dst_slot", C.c_int32), ("channels", C.c_uint32), ("filter", C.c_int32), ("dst_n", C.c_int32 * 3),
        ("origin", C.c_float * 3), ("di", C.c_float * 3), ("dj", C.c_float * 3), ("dk", C.c_float * 3), ("outside", C.c_float * 4),
        ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3),
    ]

    def copy(self, **over) -> "ResampleDesc":
        """A copy with the given fields replaced (dst_n / box_lo / box_hi from any sequence of three integers, origin / di / dj / dk
        from three floats, outside from four)."""
        d = ResampleDesc.from_buffer_copy(bytes(self))
        for k, v in over.items():
            if k in ("dst_n", "box_lo", "box_hi"):
                v = (C.c_int32 * 3)(*[int(x) for x in v])
            if k in ("origin", "di", "dj", "dk"):
                v = (C.c_float * 3)(*[float(x) for x in v])
            if k == "outside":
                v = (C.c_float * 4)(*[float(x) for x in v])
            setattr(d, k, v)
        return d


class ResampleResult(C.Structure):
    """struct vr_resample_result: the inside and outside voxels of the box, the half-open bounding box of the inside ones (zeros
    when there are none)."""
    _fields_ = [("inside", C.c_uint64), ("outside", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]

    def as_tuple(self):
        return int(self.inside), int(self.outside), tuple(int(x) for x in self.lo), tuple(int(x) for x in self.hi)


class Grid(C.Structure):
    """struct vr_grid: n voxels per axis, the centre of voxel (0, 0, 0) and the pitch per axis in patient space, one unit."""
    _fields_ = [("n", C.c_int32 * 3), ("origin", C.c_double * 3), ("spacing", C.c_double * 3)]

    @classmethod
    def of(cls, n, origin, spacing) -> "Grid":
        return cls((C.c_int32 * 3)(*[int(x) for x in n]), (C.c_double * 3)(*[float(x) for x in origin]),
                   (C.c_double * 3)(*[float(x) for x in spacing]))


class VrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vr error {code}: {msg}")
        self.code = code


_lib = None


def load() -> C.CDLL:
    """Load libvr_hip.so; raises (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, u32, u16 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint16
    fp = C.POINTER(C.c_float)
    lib.vr_create.argtypes = [C.POINTER(vp), u32, u32, i32]
    lib.vr_resize.argtypes = [vp, u32, u32]
    lib.vr_destroy.argtypes = [vp]
    lib.vr_destroy.restype = None
    lib.vr_last_error.argtypes = [vp]
    lib.vr_last_error.restype = C.c_char_p
    lib.vr_abi_version.argtypes = []
    lib.vr_volume_upload.argtypes = [vp, i32, vp, u16, u16, u16]
    lib.vr_volume_upload_device.argtypes = [vp, i32, vp, u16, u16, u16]
    lib.vr_volume_upload_raw16.argtypes = [vp, i32, vp, u16, u16, u16]
    lib.vr_volume_upload_raw32.argtypes = [vp, i32, vp, u16, u16, u16]
    lib.vr_volume_normalize.argtypes = [vp, i32, i32, C.POINTER(C.c_int)]
    lib.vr_volume_precompute_gradient.argtypes = [vp, i32, i32]
    lib.vr_volume_download.argtypes = [vp, i32, vp]
    lib.vr_tf_upload.argtypes = [vp, i32, vp, vp, u32]
    lib.vr_tf_upload_opacity.argtypes = [vp, i32, vp, u32]
    lib.vr_tf_upload_color.argtypes = [vp, i32, vp, u32]
    lib.vr_tf_upload_opacity_async.argtypes = [vp, i32, vp, u32, vp]
    lib.vr_tf_upload_color_async.argtypes = [vp, i32, vp, u32, vp]
    lib.vr_skip_field.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_int * 3), C.POINTER(C.c_int * 6), C.POINTER(C.c_uint64)]
    lib.vr_skip_hull.argtypes = [vp, i32, C.POINTER(C.c_int * 13), C.POINTER(C.c_int * 13)]
    lib.vr_skip_indexable.argtypes = [u16, u16, u16]
    lib.vr_unbounded_box_launches.argtypes = [vp]
    lib.vr_unbounded_box_launches.restype = C.c_int64
    lib.vr_set_uniforms.argtypes = [vp, C.POINTER(Uniforms)]
    lib.vr_render.argtypes = [vp, i32]
    lib.vr_render_tiles.argtypes = [vp, i32, i32, i32]
    lib.vr_tile_count.argtypes = [vp, i32, i32]
    lib.vr_render_async.argtypes = [vp, i32, vp, vp]
    lib.vr_render_tiles_async.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.vr_unpack_tiles_async.argtypes = [vp, vp, i32, vp, vp]
    lib.vr_render_batch_async.argtypes = [vp, i32, i32, C.POINTER(Uniforms), C.POINTER(vp), vp]
    lib.vr_render_tiles_batch_async.argtypes = [vp, i32, i32, i32, i32, C.POINTER(Uniforms), C.POINTER(vp), vp]
    lib.vr_unpack_tiles_strided_async.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.vr_download.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64)]
    lib.vr_download_tiles.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    lib.vr_last_timing.argtypes = [vp, fp, fp]
    lib.vr_kernel_times.argtypes = [vp, vp, i32]
    lib.vr_reset_kernel_times.argtypes = [vp]
    lib.vr_set_kernel_timing.argtypes = [vp, i32]
    lib.vr_frame_device_ptr.argtypes = [vp]
    lib.vr_frame_device_ptr.restype = vp
    lib.vr_last_covered_pixels.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.vr_last_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_last_block_trace.argtypes = [vp, C.c_void_p, C.c_int]
    lib.vr_set_kernel_flavour.argtypes = [vp, i32]
    lib.vr_last_kernel_flavour.argtypes = [vp]
    lib.vr_set_volume_layout.argtypes = [vp, i32]
    lib.vr_set_arithmetic.argtypes = [vp, i32]
    lib.vr_set_iso_value.argtypes = [vp, C.c_float]
    lib.vr_set_shadows.argtypes = [vp, i32, C.c_float]
    lib.vr_shadow_volume.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int * 3)]
    lib.vr_set_output.argtypes = [vp, i32]
    lib.vr_set_surface_threshold.argtypes = [vp, C.c_float]
    lib.vr_surface_depth_async.argtypes = [vp, vp, vp, vp]
    lib.vr_pick.argtypes = [vp, i32, u32, u32, C.POINTER(PickResult)]
    lib.vr_set_ray_bounds.argtypes = [vp, vp, vp]
    lib.vr_slice_async.argtypes = [vp, C.POINTER(SliceDesc), vp, vp]
    lib.vr_slice_render.argtypes = [vp, C.POINTER(SliceDesc), vp]
    lib.vr_slice_orthogonal.argtypes = [vp, i32, i32, i32, i32, C.POINTER(SliceDesc)]
    lib.vr_slice_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_hist_whole.argtypes = [vp, i32, u32, C.c_float, C.POINTER(HistDesc)]
    lib.vr_histogram_async.argtypes = [vp, C.POINTER(HistDesc), vp, vp, vp]
    lib.vr_histogram.argtypes = [vp, C.POINTER(HistDesc), vp, vp]
    lib.vr_hist_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_grow_whole.argtypes = [vp, i32, i32, i32, C.c_float, C.c_float, C.POINTER(GrowDesc)]
    lib.vr_segment_grow.argtypes = [vp, C.POINTER(GrowDesc), C.POINTER(GrowResult)]
    lib.vr_grow_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_grow_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_morph_ball.argtypes = [C.POINTER(C.c_uint32 * 3), C.c_uint32, C.POINTER(MorphElement)]
    lib.vr_morph_box.argtypes = [i32, i32, i32, C.POINTER(MorphElement)]
    lib.vr_morph_whole.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(MorphDesc)]
    lib.vr_mask_morph.argtypes = [vp, C.POINTER(MorphDesc), C.POINTER(MorphResult)]
    lib.vr_morph_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_morph_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_dist_whole.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(DistDesc)]
    lib.vr_mask_distance.argtypes = [vp, C.POINTER(DistDesc), C.POINTER(DistResult)]
    lib.vr_dist_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_dist_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_polygons_whole.argtypes = [vp, i32, i32, C.POINTER(PolygonsDesc)]
    lib.vr_mask_polygons.argtypes = [vp, C.POINTER(PolygonsDesc), C.POINTER(PolygonsResult)]
    lib.vr_polygons_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_polygons_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_outlines_whole.argtypes = [vp, i32, C.POINTER(OutlinesDesc)]
    lib.vr_mask_outlines.argtypes = [vp, C.POINTER(OutlinesDesc), C.POINTER(OutlinesResult)]
    lib.vr_outlines_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_outlines_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_components_whole.argtypes = [vp, i32, i32, C.POINTER(ComponentsDesc)]
    lib.vr_mask_components.argtypes = [vp, C.POINTER(ComponentsDesc), C.POINTER(ComponentsResult)]
    lib.vr_components_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_components_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_resample_identity.argtypes = [vp, i32, i32, i32, C.POINTER(ResampleDesc)]
    lib.vr_resample_between.argtypes = [C.POINTER(Grid), C.POINTER(Grid), C.POINTER(C.c_double * 12), C.POINTER(ResampleDesc)]
    lib.vr_volume_resample.argtypes = [vp, C.POINTER(ResampleDesc), C.POINTER(ResampleResult)]
    lib.vr_resample_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_resample_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_mesh_whole.argtypes = [vp, i32, C.POINTER(MeshDesc)]
    lib.vr_volume_mesh.argtypes = [vp, C.POINTER(MeshDesc), C.POINTER(MeshResult)]
    lib.vr_mesh_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 4)]
    lib.vr_mesh_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_filter_whole.argtypes = [vp, i32, i32, i32, i32, C.POINTER(FilterDesc)]
    lib.vr_filter_gaussian.argtypes = [C.c_double, i32, C.c_double, fp, i32, C.POINTER(C.c_int)]
    lib.vr_volume_filter.argtypes = [vp, C.POINTER(FilterDesc), C.POINTER(FilterResult)]
    lib.vr_filter_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_filter_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_rank_whole.argtypes = [vp, i32, i32, i32, i32, C.POINTER(RankDesc)]
    lib.vr_volume_rank.argtypes = [vp, C.POINTER(RankDesc), C.POINTER(RankResult)]
    lib.vr_rank_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_rank_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_gamma_whole.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(GammaDesc)]
    lib.vr_volume_gamma.argtypes = [vp, C.POINTER(GammaDesc), C.POINTER(GammaResult)]
    lib.vr_gamma_counters.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.vr_gamma_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    lib.vr_present_async.argtypes = [vp, vp, vp, vp]
    lib.vr_present_tiles_async.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.vr_hint_frames_in_flight.argtypes = [vp, i32]
    lib.vr_present_packed_async.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.vr_unpack_tiles_bgra8_async.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.vr_kernel_choice.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.vr_stream.argtypes = [vp, i32]
    lib.vr_stream.restype = vp
    lib.vr_volume_layout.argtypes = [vp, i32, C.POINTER(C.c_int)]
    _lib = lib
    return lib


def _f32(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a


class Context:
    """Thin RAII wrapper over vr_ctx."""

    def __init__(self, width: int, height: int, device_id: int = 0):
        self.lib = load()
        self.h = C.c_void_p()
        rc = self.lib.vr_create(C.byref(self.h), width, height, device_id)
        if rc != VR_OK:
            raise VrError(rc, (self.lib.vr_last_error(None) or b"").decode())
        self.width, self.height = width, height

    def _chk(self, rc: int):
        if rc < 0:
            raise VrError(rc, (self.lib.vr_last_error(self.h) or b"").decode())
        return rc

    def close(self):
        if self.h:
            self.lib.vr_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resize(self, w: int, h: int):
        self._chk(self.lib.vr_resize(self.h, w, h))
        self.width, self.height = w, h

    def volume_upload(self, slot: int, vec4: np.ndarray):
        """vec4: float32 array of shape (nz, ny, nx, 4)."""
        v = _f32(vec4)
        assert v.ndim == 4 and v.shape[3] == 4, v.shape
        nz, ny, nx = v.shape[:3]
        self._chk(self.lib.vr_volume_upload(self.h, slot, v.ctypes.data, nx, ny, nz))

    def volume_upload_device(self, slot: int, dptr: int, nx: int, ny: int, nz: int):
        self._chk(self.lib.vr_volume_upload_device(self.h, slot, dptr, nx, ny, nz))

    def volume_upload_raw(self, slot: int, raw: np.ndarray):
        """raw: uint16 or uint32 array (nz, ny, nx); broadcast to vec4 on the device."""
        raw = np.ascontiguousarray(raw)
        nz, ny, nx = raw.shape
        fn = {np.dtype(np.uint16): self.lib.vr_volume_upload_raw16, np.dtype(np.uint32): self.lib.vr_volume_upload_raw32}[raw.dtype]
        self._chk(fn(self.h, slot, raw.ctypes.data, nx, ny, nz))
        self._shapes = getattr(self, "_shapes", {})
        self._shapes[slot] = (nz, ny, nx)

    def volume_normalize(self, slot: int, value: int = 0) -> int:
        used = C.c_int(0)
        self._chk(self.lib.vr_volume_normalize(self.h, slot, value, C.byref(used)))
        return int(used.value)

    def volume_precompute_gradient(self, slot: int, norm_to_zero_one: bool = False):
        self._chk(self.lib.vr_volume_precompute_gradient(self.h, slot, int(norm_to_zero_one)))

    def volume_download(self, slot: int, shape) -> np.ndarray:
        out = np.empty(tuple(shape) + (4,), dtype=np.float32)
        self._chk(self.lib.vr_volume_download(self.h, slot, out.ctypes.data))
        return out

    def tf_upload(self, slot: int, opacity: np.ndarray, color_rgba: np.ndarray):
        o, c = _f32(opacity), _f32(color_rgba)
        if c.size == 4 * o.size:
            self._chk(self.lib.vr_tf_upload(self.h, slot, o.ctypes.data, c.ctypes.data, o.size))
        else:  # the two textures of a pair may differ in resolution
            self._chk(self.lib.vr_tf_upload_opacity(self.h, slot, o.ctypes.data, o.size))
            self._chk(self.lib.vr_tf_upload_color(self.h, slot, c.ctypes.data, c.size // 4))

    def tf_upload_async(self, slot: int, opacity: np.ndarray | None = None, color: np.ndarray | None = None, stream: int = 0):
        """Stream-ordered table edit (vr_tf_upload_opacity_async / _color_async): copied on call, used by every render enqueued
        after it on any stream, drains nothing.  Either table may be left out."""
        if opacity is not None:
            o = _f32(opacity)
            self._chk(self.lib.vr_tf_upload_opacity_async(self.h, slot, o.ctypes.data, o.size, stream))
        if color is not None:
            c = _f32(color)
            self._chk(self.lib.vr_tf_upload_color_async(self.h, slot, c.ctypes.data, c.size // 4, stream))

    def skip_field(self, variant: int):
        """(field uint8[bnz, bny, bnx], box (lo xyz, hi xyz) in bricks, active bricks) a launch of `variant` would use now
        (vr_skip_field: built synchronously)."""
        dims, box, active = (C.c_int * 3)(), (C.c_int * 6)(), C.c_uint64(0)
        n = self._chk(self.lib.vr_skip_field(self.h, variant, None, 0, C.byref(dims), C.byref(box), C.byref(active)))
        out = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.vr_skip_field(self.h, variant, out.ctypes.data, n, C.byref(dims), C.byref(box), C.byref(active)))
        return out.reshape(dims[2], dims[1], dims[0]), tuple(int(x) for x in box), int(active.value)

    def skip_hull(self, variant: int):
        """(lo[13], hi[13]): the smallest / largest n . b over the active bricks of that field along the hull's 13 directions
        (vr_skip_hull: built synchronously; INT_MAX / INT_MIN when no brick is active)."""
        lo, hi = (C.c_int * 13)(), (C.c_int * 13)()
        self._chk(self.lib.vr_skip_hull(self.h, variant, C.byref(lo), C.byref(hi)))
        return tuple(int(x) for x in lo), tuple(int(x) for x in hi)

    @staticmethod
    def skip_indexable(nx: int, ny: int, nz: int) -> bool:
        """Whether launches on a volume of these dimensions may skip empty space (vr_skip_indexable; no device needed)."""
        return bool(load().vr_skip_indexable(nx, ny, nz))

    def unbounded_box_launches(self) -> int:
        """Skipping launches that ran without an active-brick box (an asynchronous rebuild's box still on its way)."""
        return self._chk(self.lib.vr_unbounded_box_launches(self.h))

    def set_uniforms(self, u: Uniforms):
        self._chk(self.lib.vr_set_uniforms(self.h, C.byref(u)))

    def render(self, variant: int):
        self._chk(self.lib.vr_render(self.h, variant))

    def render_tiles(self, variant: int, rank: int, world: int):
        self._chk(self.lib.vr_render_tiles(self.h, variant, rank, world))

    def tile_count(self, rank: int, world: int) -> int:
        return self._chk(self.lib.vr_tile_count(self.h, rank, world))

    def render_async(self, variant: int, d_frame: int = 0, stream: int = 0):
        self._chk(self.lib.vr_render_async(self.h, variant, d_frame, stream))

    def render_tiles_async(self, variant: int, rank: int, world: int, d_tiles: int, stream: int = 0):
        self._chk(self.lib.vr_render_tiles_async(self.h, variant, rank, world, d_tiles, stream))

    def unpack_tiles_async(self, d_gathered: int, world: int, d_frame: int = 0, stream: int = 0):
        self._chk(self.lib.vr_unpack_tiles_async(self.h, d_gathered, world, d_frame, stream))

    def unpack_tiles_strided_async(self, d_gathered: int, world: int, rank_stride_tiles: int, d_frame: int = 0, stream: int = 0):
        self._chk(self.lib.vr_unpack_tiles_strided_async(self.h, d_gathered, world, rank_stride_tiles, d_frame, stream))

    @staticmethod
    def _batch_args(uniforms, buffers):
        n = len(uniforms)
        assert n == len(buffers)
        return n, (Uniforms * n)(*uniforms), (C.c_void_p * n)(*buffers)

    def render_batch_async(self, variant: int, uniforms, d_frames, stream: int = 0):
        """One launch, len(uniforms) frames (1..4) of the bound scene: frame f with uniforms[f] into d_frames[f]."""
        n, us, bufs = self._batch_args(uniforms, d_frames)
        self._chk(self.lib.vr_render_batch_async(self.h, variant, n, us, bufs, stream))

    def render_tiles_batch_async(self, variant: int, rank: int, world: int, uniforms, d_tiles, stream: int = 0):
        n, us, bufs = self._batch_args(uniforms, d_tiles)
        self._chk(self.lib.vr_render_tiles_batch_async(self.h, variant, rank, world, n, us, bufs, stream))

    def download(self, present: bool = False):
        """Returns (frag[H,W,4] float32, bgra8[H,W,4] uint8 or None, composited_samples)."""
        frag = np.empty((self.height, self.width, 4), dtype=np.float32)
        bgra = np.empty((self.height, self.width, 4), dtype=np.uint8) if present else None
        n = C.c_uint64(0)
        self._chk(self.lib.vr_download(self.h, frag.ctypes.data, bgra.ctypes.data if present else None, C.byref(n)))
        return frag, bgra, int(n.value)

    def samples(self) -> int:
        n = C.c_uint64(0)
        self._chk(self.lib.vr_download(self.h, None, None, C.byref(n)))
        return int(n.value)

    def download_tiles(self, n_tiles: int):
        tiles = np.empty((n_tiles, TILE, TILE, 4), dtype=np.float32)
        n = C.c_uint64(0)
        self._chk(self.lib.vr_download_tiles(self.h, tiles.ctypes.data, C.byref(n)))
        return tiles, int(n.value)

    def last_timing(self):
        k, t = C.c_float(0), C.c_float(0)
        self._chk(self.lib.vr_last_timing(self.h, C.byref(k), C.byref(t)))
        return float(k.value), float(t.value)

    def kernel_times(self, capacity: int = 256) -> np.ndarray:
        out = np.zeros(capacity, dtype=np.float32)
        n = self._chk(self.lib.vr_kernel_times(self.h, out.ctypes.data, capacity))
        return out[:n].copy()

    def reset_kernel_times(self):
        self._chk(self.lib.vr_reset_kernel_times(self.h))

    def set_kernel_timing(self, events: bool):
        """vr_kernel_times from HIP events around every launch (True) or from the launches' own records (False, the default)."""
        self._chk(self.lib.vr_set_kernel_timing(self.h, 1 if events else 0))

    def covered_pixels(self) -> int:
        n = C.c_uint64(0)
        self._chk(self.lib.vr_last_covered_pixels(self.h, C.byref(n)))
        return int(n.value)

    def counters(self):
        """(composited samples, covered pixels, samples actually fetched) of the last render."""
        out = (C.c_uint64 * 3)()
        self._chk(self.lib.vr_last_counters(self.h, C.byref(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def block_trace(self):
        """(n, 6) uint64 array, one row per workgroup of the last march launch: composited, covered, fetched,
        start, end (100 MHz device clock), HW_ID | XCC_ID << 32."""
        n = self.lib.vr_last_block_trace(self.h, None, 0)
        if n < 0:
            self._chk(n)
        out = np.zeros((max(n, 0), 6), dtype=np.uint64)
        if n > 0:
            self._chk(min(0, self.lib.vr_last_block_trace(self.h, out.ctypes.data_as(C.c_void_p), n)))
        return out

    def frame_device_ptr(self) -> int:
        return int(self.lib.vr_frame_device_ptr(self.h) or 0)

    def last_kernel_flavour(self) -> int:
        return self._chk(self.lib.vr_last_kernel_flavour(self.h))

    def kernel_choice(self):
        """(candidate flavours, ms per launch measured for each, index of the one kept or -1) of the default's measured choice."""
        fl, ms, ch = (C.c_int * 6)(), (C.c_float * 6)(), C.c_int(-1)
        n = self.lib.vr_kernel_choice(self.h, fl, ms, C.byref(ch))
        if n < 0:
            self._chk(n)
        return [int(x) for x in fl[:n]], [float(x) for x in ms[:n]], int(ch.value)

    def hint_frames_in_flight(self, frames: int):
        """How many frames the caller keeps in flight on different streams (steers the default kernel choice only)."""
        self._chk(self.lib.vr_hint_frames_in_flight(self.h, frames))

    def stream(self, index: int) -> int:
        """Context-owned stream `index` (0..3) of a set probed to run side by side: use them in turn for frames in flight."""
        s = self.lib.vr_stream(self.h, index)
        if not s:
            raise VrError(VR_ERR_HIP, "vr_stream: no stream available")
        return int(s)

    def present_async(self, d_bgra8: int, d_frame: int = 0, stream: int = 0):
        """BGRA8Unorm present of a device frame into device memory (what a GL / Vulkan interop buffer would be)."""
        self._chk(self.lib.vr_present_async(self.h, d_frame, d_bgra8, stream))

    def present_tiles_async(self, d_gathered: int, world: int, d_bgra8: int, rank_stride_tiles: int = 0, stream: int = 0):
        """vr_present_tiles_async: BGRA8 frame straight from gathered tile-major segments (device pointers)."""
        self._chk(self.lib.vr_present_tiles_async(self.h, d_gathered, world, rank_stride_tiles, d_bgra8, stream))

    def set_arithmetic(self, mode: int):
        """ARITH_SEPARATE (0, default) or ARITH_FUSED (1): per-sample a * b + c with two roundings or one (include/vr.h)."""
        self._chk(self.lib.vr_set_arithmetic(self.h, mode))

    def set_iso_value(self, iso: float):
        """The level of ISO launches enqueued after this call (default 0.5; finite values only, include/vr.h)."""
        self._chk(self.lib.vr_set_iso_value(self.h, iso))

    def set_shadows(self, divisor: int, scale: float = 1.0):
        """Shadows of LIGHT launches enqueued after this call: divisor 0 = off (default), 1 / 2 / 4 / 8 = voxels per light-volume
        texel and axis; scale = the opacity scale (finite, >= 0).  include/vr.h vr_set_shadows."""
        self._chk(self.lib.vr_set_shadows(self.h, divisor, scale))

    def shadow_volume(self):
        """(transmittance float32[Gz, Gy, Gx], (Gx, Gy, Gz)): the light volume a LIGHT launch enqueued now would read
        (vr_shadow_volume: built synchronously, drains the device)."""
        dims = (C.c_int * 3)()
        n = self._chk(self.lib.vr_shadow_volume(self.h, None, 0, C.byref(dims)))
        out = np.zeros(n, dtype=np.float32)
        self._chk(self.lib.vr_shadow_volume(self.h, out.ctypes.data, n, C.byref(dims)))
        return out.reshape(dims[2], dims[1], dims[0]), (int(dims[0]), int(dims[1]), int(dims[2]))

    def set_output(self, mode: int):
        """OUTPUT_COLOR (0, default) or OUTPUT_SURFACE (1): launches of BASIC / LIGHT / ISO enqueued after this call write surface
        positions (q.x, q.y, q.z, alpha) instead of colour (include/vr.h vr_set_output)."""
        self._chk(self.lib.vr_set_output(self.h, mode))

    def set_surface_threshold(self, tau: float):
        """The alpha threshold of BASIC / LIGHT surface launches enqueued after this call (default 0.5; finite, 0 <= tau < 1)."""
        self._chk(self.lib.vr_set_surface_threshold(self.h, tau))

    def surface_depth(self, d_surface: int, d_depth: int, stream: int = 0):
        """vr_surface_depth_async: the depth (W*H floats, device) a rasteriser drawing at the points of the surface frame `d_surface`
        (device) would write, with the context's uniforms and threshold at this call; 1.0 where there is no hit."""
        self._chk(self.lib.vr_surface_depth_async(self.h, d_surface, d_depth, stream))

    def pick(self, variant: int, x: int, y: int) -> PickResult:
        """vr_pick: what is under pixel (x, y) of a BASIC / LIGHT / ISO frame with the context's uniforms (synchronous; the context's
        frame, counters and last flavour stay those of the render before it)."""
        out = PickResult()
        self._chk(self.lib.vr_pick(self.h, variant, x, y, C.byref(out)))
        return out

    def set_ray_bounds(self, d_near: int | None = None, d_far: int | None = None):
        """vr_set_ray_bounds: BASIC / LIGHT colour launches enqueued after this call march only between the two depth buffers (device
        pointers to W*H floats each, the depth convention of surface_depth; None = no bound on that side, both None = off)."""
        self._chk(self.lib.vr_set_ray_bounds(self.h, d_near or None, d_far or None))

    def slice_async(self, desc: SliceDesc, d_out: int, stream: int = 0):
        """vr_slice_async: the slice `desc` into device memory d_out (width * height float4, or 32-bit words for SLICE_BGRA8) on
        `stream`; nothing is synchronised."""
        self._chk(self.lib.vr_slice_async(self.h, C.byref(desc), d_out, stream))

    def slice(self, desc: SliceDesc) -> np.ndarray:
        """vr_slice_render: the slice as float32[height, width, 4], or uint8[height, width, 4] (B, G, R, A) for SLICE_BGRA8."""
        shape = (int(desc.height), int(desc.width), 4)
        out = np.empty(shape, dtype=np.uint8 if desc.format == SLICE_BGRA8 else np.float32)
        self._chk(self.lib.vr_slice_render(self.h, C.byref(desc), out.ctypes.data))
        return out

    def slice_orthogonal(self, slot: int, axis: int, index: int, thickness: int = 1) -> SliceDesc:
        """vr_slice_orthogonal: the descriptor of the axis-aligned plane `axis` (0 x, 1 y, 2 z) at voxel `index` of volume `slot`,
        one pixel per voxel, `thickness` voxels of slab centred on it (MAX, LINEAR, RGBA32F, TF slot 0: edit as needed)."""
        d = SliceDesc()
        self._chk(self.lib.vr_slice_orthogonal(self.h, slot, axis, index, thickness, C.byref(d)))
        return d

    def slice_counters(self):
        """(counted samples, pixels with a counted sample, samples whose voxels were loaded) of the last slice launch."""
        out = (C.c_uint64 * 3)()
        self._chk(self.lib.vr_slice_counters(self.h, C.byref(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def hist_whole(self, slot: int, bins: int, scale: float) -> HistDesc:
        """vr_hist_whole: the descriptor of the whole volume `slot` (channel 3, no mask, row 0, CLAMP: edit as needed)."""
        d = HistDesc()
        self._chk(self.lib.vr_hist_whole(self.h, slot, bins, scale, C.byref(d)))
        return d

    def histogram_async(self, desc: HistDesc, d_counts: int, d_rows: int, stream: int = 0):
        """vr_histogram_async: into device memory d_counts (uint64[5][bins]) and d_rows (5 x (voxels, dropped) uint64) on `stream`;
        nothing is synchronised."""
        self._chk(self.lib.vr_histogram_async(self.h, C.byref(desc), d_counts, d_rows, stream))

    def histogram(self, desc: HistDesc):
        """vr_histogram: (counts uint64[5, bins], rows = [(voxels, dropped)] * 5); rows that were not requested are zero."""
        counts = np.zeros((HIST_ROWS, int(desc.bins)), dtype=np.uint64)
        rows = (HistRow * HIST_ROWS)()
        self._chk(self.lib.vr_histogram(self.h, C.byref(desc), counts.ctypes.data, C.addressof(rows)))
        return counts, [(int(r.voxels), int(r.dropped)) for r in rows]

    def hist_counters(self):
        """(voxels of the box, voxels whose value was loaded, voxels settled from a brick record) of the last histogram launch."""
        out = (C.c_uint64 * 3)()
        self._chk(self.lib.vr_hist_counters(self.h, C.byref(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def _tool_counters(self, call):
        """The three counters of a mask tool's last call, as ints."""
        out = (C.c_uint64 * 3)()
        self._chk(call(self.h, C.byref(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def _tool_timing(self, call):
        """The four phases of a mask tool's last call in ms of device time."""
        out = (C.c_float * 4)()
        self._chk(call(self.h, C.byref(out)))
        return tuple(float(x) for x in out)

    def grow_whole(self, volume_slot: int, mask_slot: int, contour: int, lo: float, hi: float) -> GrowDesc:
        """vr_grow_whole: the descriptor of a grow over the whole volume (channel 3, FACES, REPLACE, no seeds: add them with copy)."""
        d = GrowDesc()
        self._chk(self.lib.vr_grow_whole(self.h, volume_slot, mask_slot, contour, lo, hi, C.byref(d)))
        return d

    def segment_grow(self, desc: GrowDesc) -> GrowResult:
        """vr_segment_grow: grows the region from desc's seeds and writes the contour into the mask slot (synchronous)."""
        out = GrowResult()
        self._chk(self.lib.vr_segment_grow(self.h, C.byref(desc), C.byref(out)))
        return out

    def grow_counters(self):
        """(voxels of the box, voxels whose value was loaded, voxels classified from a brick record) of the last segment_grow."""
        return self._tool_counters(self.lib.vr_grow_counters)

    def grow_timing(self):
        """(classify, propagate, write, refresh) of the last segment_grow in ms of device time (vr_grow_timing)."""
        return self._tool_timing(self.lib.vr_grow_timing)

    def morph_whole(self, src_slot: int, src_contour: int, dst_slot: int, dst_contour: int, op: int) -> MorphDesc:
        """vr_morph_whole: the descriptor of an operator over the whole volume (REPLACE, the radius-1 ball of unit spacing)."""
        d = MorphDesc()
        self._chk(self.lib.vr_morph_whole(self.h, src_slot, src_contour, dst_slot, dst_contour, op, C.byref(d)))
        return d

    def mask_morph(self, desc: MorphDesc) -> MorphResult:
        """vr_mask_morph: dilates, erodes, closes, opens or takes a contour and combines the result into a contour (synchronous)."""
        out = MorphResult()
        self._chk(self.lib.vr_mask_morph(self.h, C.byref(desc), C.byref(out)))
        return out

    def morph_counters(self):
        """(voxels of the box, voxels the last dilation launch computed, voxels settled without computing) of the last mask_morph."""
        return self._tool_counters(self.lib.vr_morph_counters)

    def morph_timing(self):
        """(pack, morphology, write, refresh) of the last mask_morph in ms of device time (vr_morph_timing)."""
        return self._tool_timing(self.lib.vr_morph_timing)

    def dist_whole(self, src_slot: int, src_contour: int, dst_slot: int, dst_channel: int, mode: int) -> DistDesc:
        """vr_dist_whole: the descriptor of a distance map over the whole volume (unit spacing, no limit, scale 1, no probe)."""
        return dist_whole(self, src_slot, src_contour, dst_slot, dst_channel, mode)

    def mask_distance(self, desc: DistDesc) -> DistResult:
        """vr_mask_distance: the exact Euclidean distance transform of a contour into one component of a volume slot (synchronous)."""
        out = DistResult()
        self._chk(self.lib.vr_mask_distance(self.h, C.byref(desc), C.byref(out)))
        return out

    def dist_counters(self):
        """(voxels of the box, voxels inside the region the envelope passes computed, the rest) of the last mask_distance."""
        return self._tool_counters(self.lib.vr_dist_counters)

    def dist_timing(self):
        """(pack, distance passes, write, refresh) of the last mask_distance in ms of device time (vr_dist_timing)."""
        return self._tool_timing(self.lib.vr_dist_timing)

    def polygons_whole(self, grid_slot: int, dst_slot: int) -> PolygonsDesc:
        """vr_polygons_whole: the descriptor of a raster over the whole grid (contour 0, EVEN_ODD, REPLACE, origin 0, unit spacing)."""
        d = PolygonsDesc()
        self._chk(self.lib.vr_polygons_whole(self.h, grid_slot, dst_slot, C.byref(d)))
        return d

    def mask_polygons(self, desc: PolygonsDesc, points, polygons) -> PolygonsResult:
        """vr_mask_polygons: rasterises closed polygons into contours of a mask slot (synchronous).  points: int32 (n, 2) pairs x, y in
        the descriptor's unit; polygons: a sequence of (first, count, slice, contour).  The descriptor's own points / polygons fields
        are ignored."""
        pts, polys = polygon_arrays(points, polygons)
        d = desc.copy(n_points=len(pts), n_polygons=len(polys), points=pts.ctypes.data if len(pts) else None,
                      polygons=C.cast(polys, C.c_void_p).value if len(polys) else None)
        out = PolygonsResult()
        self._chk(self.lib.vr_mask_polygons(self.h, C.byref(d), C.byref(out)))  # (pts and polys live until here)
        return out

    def polygons_counters(self):
        """(polygons given, polygons rasterised, polygons skipped) of the last mask_polygons."""
        return self._tool_counters(self.lib.vr_polygons_counters)

    def polygons_timing(self):
        """(upload, raster, write, refresh) of the last mask_polygons in ms of device time (vr_polygons_timing)."""
        return self._tool_timing(self.lib.vr_polygons_timing)

    def outlines_whole(self, src_slot: int) -> OutlinesDesc:
        """vr_outlines_whole: the descriptor of a trace over the whole volume (contour 0, SPLIT, origin 0, unit spacing, offset 0)."""
        d = OutlinesDesc()
        self._chk(self.lib.vr_outlines_whole(self.h, src_slot, C.byref(d)))
        return d

    def mask_outlines(self, desc: OutlinesDesc):
        """vr_mask_outlines: traces contours of a mask slot into closed polygons (synchronous): the counting call, then the call that
        stores.  Returns (points int32 (N, 2), polygons [(first, count, slice, contour)], OutlinesResult); the first two can be passed
        straight to mask_polygons.  The descriptor's own capacities and arrays are ignored."""
        out = OutlinesResult()
        self._chk(self.lib.vr_mask_outlines(self.h, C.byref(desc.copy(max_points=0, max_polygons=0, points=None, polygons=None)), C.byref(out)))
        pts = np.zeros((int(out.n_points), 2), np.int32)
        polys = (Polygon * int(out.n_polygons))()
        if out.n_points:
            d = desc.copy(max_points=len(pts), max_polygons=len(polys), points=pts.ctypes.data, polygons=C.cast(polys, C.c_void_p).value)
            self._chk(self.lib.vr_mask_outlines(self.h, C.byref(d), C.byref(out)))  # (pts and polys live until here)
        return pts, [(int(q.first), int(q.count), int(q.slice), int(q.contour)) for q in polys], out

    def outlines_counters(self):
        """(corner nodes, polygons, doubling rounds launched) of the last mask_outlines."""
        return self._tool_counters(self.lib.vr_outlines_counters)

    def outlines_timing(self):
        """(pack, corners + scan + link, doubling rounds, emit + copy back) of the last mask_outlines in ms of device time."""
        return self._tool_timing(self.lib.vr_outlines_timing)

    def components_whole(self, src_slot: int, src_contour: int) -> ComponentsDesc:
        """vr_components_whole: the descriptor of a labelling of contour src_contour over the whole volume (FACES, every component
        selected, no destination, no table)."""
        d = ComponentsDesc()
        self._chk(self.lib.vr_components_whole(self.h, src_slot, src_contour, C.byref(d)))
        return d

    def mask_components(self, desc: ComponentsDesc) -> dict:
        """vr_mask_components: the connected components of a contour (synchronous): the counting call, which writes nothing, then the
        call that stores.  Returns {"result": ComponentsResult, "components": [(voxels, lo, hi, first, faces)]}.  The descriptor's own
        capacity and array are ignored."""
        out = ComponentsResult()
        self._chk(self.lib.vr_mask_components(self.h, C.byref(desc.copy(dst_slot=-1, label_slot=-1, max_components=0, components=None)),
                                              C.byref(out)))
        n = int(out.n_components)
        table = (Component * n)()
        d = desc.copy(max_components=n, components=C.cast(table, C.c_void_p).value if n else None)
        if n or desc.dst_slot >= 0 or desc.label_slot >= 0:
            self._chk(self.lib.vr_mask_components(self.h, C.byref(d), C.byref(out)))  # (the table lives until here)
        return {"result": out, "components": [q.as_tuple() for q in table]}

    def components_counters(self):
        """(voxels of the box, run nodes, pairs of a node and a touching run examined) of the last mask_components."""
        return self._tool_counters(self.lib.vr_components_counters)

    def components_timing(self):
        """(pack, runs + scan + merge + flatten, numbering .. copy back, refresh) of the last mask_components in ms of device time."""
        return self._tool_timing(self.lib.vr_components_timing)

    def resample_identity(self, src_slot: int, dst_slot: int, filter: int = RESAMPLE_LINEAR) -> ResampleDesc:
        """vr_resample_identity: the descriptor that puts voxel centres on voxel centres of src_slot's own grid (all four components,
        outside = 0, the whole box)."""
        d = ResampleDesc()
        self._chk(self.lib.vr_resample_identity(self.h, src_slot, dst_slot, filter, C.byref(d)))
        return d

    def resample_between(self, src: Grid, dst: Grid, dst_to_src=None, **over) -> ResampleDesc:
        """vr_resample_between: the grid fields of a descriptor for `dst` sampled from `src` (resample_between below); needs no device."""
        return resample_between(src, dst, dst_to_src, **over)

    def volume_resample(self, desc: ResampleDesc) -> ResampleResult:
        """vr_volume_resample: writes components of the destination slot with values sampled from the source slot (synchronous)."""
        out = ResampleResult()
        self._chk(self.lib.vr_volume_resample(self.h, C.byref(desc), C.byref(out)))
        return out

    def resample_counters(self):
        """(voxels of the box, voxels whose source voxels were loaded, voxels stored without a load) of the last volume_resample."""
        return self._tool_counters(self.lib.vr_resample_counters)

    def resample_timing(self):
        """(range records, kernel, result words, refresh) of the last volume_resample in ms of device time (vr_resample_timing)."""
        return self._tool_timing(self.lib.vr_resample_timing)

    def mesh_whole(self, src_slot: int) -> MeshDesc:
        """vr_mesh_whole: the descriptor of an extraction over the whole volume (channel 3, level 0.5, no cap, no buffers)."""
        d = MeshDesc()
        self._chk(self.lib.vr_mesh_whole(self.h, src_slot, C.byref(d)))
        return d

    def volume_mesh(self, desc: MeshDesc):
        """vr_volume_mesh: the surface {value >= level} of a component inside a box as an indexed triangle mesh (synchronous): the
        counting call, then the call that stores.  Returns (vertices float32 (V, 3) in voxel-index units, triangles uint32 (T, 3),
        MeshResult).  The descriptor's own capacities and arrays are ignored."""
        out = MeshResult()
        self._chk(self.lib.vr_volume_mesh(self.h, C.byref(desc.copy(max_vertices=0, max_triangles=0, vertices=None, triangles=None)), C.byref(out)))
        verts = np.zeros((int(out.n_vertices), 3), np.float32)
        tris = np.zeros((int(out.n_triangles), 3), np.uint32)
        if out.n_vertices:
            d = desc.copy(max_vertices=len(verts), max_triangles=len(tris), vertices=verts.ctypes.data, triangles=tris.ctypes.data)
            self._chk(self.lib.vr_volume_mesh(self.h, C.byref(d), C.byref(out)))  # (verts and tris live until here)
        return verts, tris, out

    def mesh_counters(self):
        """(points of the box, voxels loaded, voxels settled from a range record, cells that emit) of the last volume_mesh."""
        out = (C.c_uint64 * 4)()
        self._chk(self.lib.vr_mesh_counters(self.h, C.byref(out)))
        return tuple(int(x) for x in out)

    def mesh_timing(self):
        """(classify / pack, counts + scans, vertex emit, triangle emit + copy back) of the last volume_mesh in ms of device time."""
        return self._tool_timing(self.lib.vr_mesh_timing)

    def filter_whole(self, src_slot: int, src_channel: int, dst_slot: int, dst_channel: int) -> FilterDesc:
        """vr_filter_whole: the descriptor of a filter of component src_channel of volume src_slot over its whole volume into component
        dst_channel of volume dst_slot: CLAMP, border_value 0, no pass (edit with copy; volume_filter takes the weights)."""
        d = FilterDesc()
        self._chk(self.lib.vr_filter_whole(self.h, src_slot, src_channel, dst_slot, dst_channel, C.byref(d)))
        return d

    def volume_filter(self, desc: FilterDesc, taps=(None, None, None)) -> FilterResult:
        """vr_volume_filter: up to three 1-D correlations along x, y, z of a component into a component (synchronous).  taps: per axis
        an odd number of float32 weights (filter_gaussian's, say) or None for no pass along it; they set the descriptor's radius and
        taps fields, whose own values are ignored."""
        arrays = [None if t is None else np.ascontiguousarray(t, dtype=np.float32).ravel() for t in taps]
        if len(arrays) != 3 or any(a is not None and a.size % 2 == 0 for a in arrays):
            raise ValueError("taps: three entries, each None or an odd number of weights")
        d = desc.copy(radius=[0 if a is None else a.size // 2 for a in arrays], taps=[None if a is None else a.ctypes.data for a in arrays])
        out = FilterResult()
        self._chk(self.lib.vr_volume_filter(self.h, C.byref(d), C.byref(out)))  # (arrays live until here)
        return out

    def filter_counters(self):
        """(voxels of the box, values the passes computed, passes) of the last volume_filter."""
        return self._tool_counters(self.lib.vr_filter_counters)

    def filter_timing(self):
        """(first pass, remaining passes, write + result words, refresh) of the last volume_filter in ms of device time."""
        return self._tool_timing(self.lib.vr_filter_timing)

    def rank_whole(self, src_slot: int, src_channel: int, dst_slot: int, dst_channel: int) -> RankDesc:
        """vr_rank_whole: the descriptor of a rank filter of component src_channel of volume src_slot over its whole volume into
        component dst_channel of volume dst_slot: radii 0, RANK_MEDIAN, CLAMP, border_value 0 (edit with copy)."""
        d = RankDesc()
        self._chk(self.lib.vr_rank_whole(self.h, src_slot, src_channel, dst_slot, dst_channel, C.byref(d)))
        return d

    def volume_rank(self, desc: RankDesc) -> RankResult:
        """vr_volume_rank: the value at position `rank` of the ascending order of the (2 rx + 1)(2 ry + 1)(2 rz + 1) values around every
        voxel of the box -- median, minimum, maximum -- of a component into a component (synchronous)."""
        out = RankResult()
        self._chk(self.lib.vr_volume_rank(self.h, C.byref(desc), C.byref(out)))
        return out

    def rank_counters(self):
        """(voxels of the box, voxels of the box grown by the radii and clipped to the volume, the resolved rank) of the last volume_rank."""
        return self._tool_counters(self.lib.vr_rank_counters)

    def rank_timing(self):
        """(the selection kernel, further ones: 0, write + result words, refresh) of the last volume_rank in ms of device time."""
        return self._tool_timing(self.lib.vr_rank_timing)

    def gamma_whole(self, ref_slot: int, ref_channel: int, eval_slot: int, eval_channel: int, dst_slot: int, dst_channel: int) -> GammaDesc:
        """vr_gamma_whole: the descriptor of a gamma comparison of component eval_channel of volume eval_slot against component
        ref_channel of volume ref_slot over the whole volume into component dst_channel of volume dst_slot: unit spacing,
        dta = reach = 1, sub 1, GAMMA_GLOBAL, tolerance 1, no cutoff, no ROI, skipped voxels NaN (edit with copy)."""
        d = GammaDesc()
        self._chk(self.lib.vr_gamma_whole(self.h, ref_slot, ref_channel, eval_slot, eval_channel, dst_slot, dst_channel, C.byref(d)))
        return d

    def volume_gamma(self, desc: GammaDesc) -> GammaResult:
        """vr_volume_gamma: for every voxel of the box the gamma index of the evaluated dose against the reference dose -- the least,
        over the candidate positions within reach, of dose difference and distance combined -- into a component (synchronous)."""
        out = GammaResult()
        self._chk(self.lib.vr_volume_gamma(self.h, C.byref(desc), C.byref(out)))
        return out

    def gamma_counters(self):
        """(voxels of the box, evaluated voxels, admitted offsets K) of the last volume_gamma."""
        return self._tool_counters(self.lib.vr_gamma_counters)

    def gamma_timing(self):
        """(the search kernel, further ones: 0, write + result words, refresh) of the last volume_gamma in ms of device time."""
        return self._tool_timing(self.lib.vr_gamma_timing)

    def set_volume_layout(self, mode: int):
        """0 bricked copy (default), 1 the reference's vec4 voxels only, 3 x-fastest voxels + density plane (2 was removed)."""
        self._chk(self.lib.vr_set_volume_layout(self.h, mode))

    def volume_layout(self, slot: int) -> int:
        """bit 0 density plane present, bit 1 .rgb verified as central difference of .a, bit 2 last render derived gradients."""
        f = C.c_int(0)
        self._chk(self.lib.vr_volume_layout(self.h, slot, C.byref(f)))
        return int(f.value)

    def set_kernel_flavour(self, flavour: int):
        self._chk(self.lib.vr_set_kernel_flavour(self.h, flavour))


def polygon_arrays(points, polygons):
    """(a contiguous int32 (n, 2) array, a ctypes array of Polygon) for vr_polygons_desc.points / .polygons."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.int32).reshape(-1, 2))
    polys = (Polygon * len(polygons))(*[Polygon(int(f), int(n), int(z), int(k)) for f, n, z, k in polygons])
    return pts, polys


def morph_ball(spacing, radius: int) -> MorphElement:
    """vr_morph_ball: the ball of `radius` on a grid of voxel spacing (sx, sy, sz), all in one integer unit (micrometres, say).  Host
    arithmetic: needs no context and no device."""
    e = MorphElement()
    sp = (C.c_uint32 * 3)(*[int(x) for x in spacing])
    rc = load().vr_morph_ball(C.byref(sp), int(radius), C.byref(e))
    if rc != VR_OK:
        raise VrError(rc, f"vr_morph_ball: spacing {tuple(spacing)}, radius {radius}")
    return e


def morph_box(rx: int, ry: int, rz: int) -> MorphElement:
    """vr_morph_box: the full box of radii (rx, ry, rz).  Host arithmetic: needs no context and no device."""
    e = MorphElement()
    rc = load().vr_morph_box(int(rx), int(ry), int(rz), C.byref(e))
    if rc != VR_OK:
        raise VrError(rc, f"vr_morph_box: radii {(rx, ry, rz)}")
    return e


def dist_whole(ctx: "Context", src_slot: int, src_contour: int, dst_slot: int, dst_channel: int, mode: int) -> DistDesc:
    """vr_dist_whole: the descriptor of a distance map of contour src_contour of volume src_slot over its whole volume into component
    dst_channel of volume dst_slot: unit spacing, no limit, scale 1.0, no probe (edit with copy)."""
    d = DistDesc()
    ctx._chk(ctx.lib.vr_dist_whole(ctx.h, src_slot, src_contour, dst_slot, dst_channel, mode, C.byref(d)))
    return d


def filter_gaussian(sigma: float, order: int = 0, truncate: float = 4.0) -> np.ndarray:
    """vr_filter_gaussian: the 2 r + 1 float32 weights of a Gaussian of standard deviation `sigma` voxels (order 0) or of its first
    derivative (order 1), r = int(truncate * sigma + 0.5): the counting call, then the call that stores.  Host arithmetic: needs no
    context and no device."""
    lib, r = load(), C.c_int(-1)
    lib.vr_filter_gaussian(float(sigma), int(order), float(truncate), None, 0, C.byref(r))
    if r.value < 0:
        raise VrError(VR_ERR_INVALID_ARG, f"vr_filter_gaussian: sigma {sigma}, order {order}, truncate {truncate} (radius at most {FILTER_MAX_RADIUS})")
    taps = np.zeros(2 * r.value + 1, np.float32)
    rc = lib.vr_filter_gaussian(float(sigma), int(order), float(truncate), taps.ctypes.data_as(C.POINTER(C.c_float)), taps.size, C.byref(r))
    if rc != VR_OK:
        raise VrError(rc, "vr_filter_gaussian")
    return taps


def resample_between(src: Grid, dst: Grid, dst_to_src=None, **over) -> ResampleDesc:
    """vr_resample_between: dst_n, origin, di, dj, dk and the whole box of a descriptor for destination grid `dst` sampled from source
    grid `src`; dst_to_src: twelve numbers, the row-major 3 x 4 map from destination to source patient coordinates (None = identity).
    The other fields are zero unless given in `over` (as ResampleDesc.copy takes them).  Host arithmetic: needs no context."""
    d = ResampleDesc()
    m = None if dst_to_src is None else (C.c_double * 12)(*[float(x) for x in np.asarray(dst_to_src, np.float64).ravel()])
    rc = load().vr_resample_between(C.byref(src), C.byref(dst), None if m is None else C.byref(m), C.byref(d))
    if rc != VR_OK:
        raise VrError(rc, "vr_resample_between: a grid size outside 1 .. 65535, a spacing that is not finite and > 0, or a matrix entry that is not finite")
    return d.copy(**over)
