// Application -- the render-call surface: owns the camera and the per-frame uniforms, hands them to the
// ray-marcher once per frame and asks the active scene to render.  Mirrors med::Application
// (App/src/Application.h / Application.cpp: OnStart :58-94, OnUpdate :96-119, OnRender :121-239,
// OnResize :299-323) without the window, the event queue and the ImGui layer.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "Camera.h"
#include "MiniApp.h"
#include "SurfaceMesh.h"
#include "dicom/StructureFileDcm.h"
#include "dicom/VolumeFileDcm.h"
#include "vr.h"

namespace med {

// What Application::Gamma takes beyond the tolerance and the distance to agreement.
struct GammaOptions {
    double reachMm = 0.0;            // how far the search goes; 0: 2 * dtaMm
    int sub = 1;                     // candidate positions per voxel step and axis, 1 .. VR_GAMMA_MAX_SUB
    int mode = VR_GAMMA_GLOBAL;      // VR_GAMMA_LOCAL: doseTolerance is a fraction of the reference dose at the voxel
    float cutoff = -HUGE_VALF;       // voxels whose reference dose is not >= cutoff are skipped
    int roiSlot = -1, roiContour = 0;  // voxels outside this contour are skipped; roiSlot -1: none
    float skipValue = NAN;           // what a skipped voxel stores
};

class Application {
public:
    Application(uint32_t width = 1280, uint32_t height = 720, int device = 0);  // Application.h:100-104
    ~Application();
    Application(const Application&) = delete;
    Application& operator=(const Application&) = delete;

    bool Ok() const { return p_Ctx != nullptr; }
    const std::string& LastError() const { return m_Error; }

    int OnStart(std::unique_ptr<MiniApp> app);   // scene selection + "use the MiniApp's step parameters" (:69-84)
    int OnUpdate();                              // rewrites every uniform (:96-119) and lets the scene re-upload TFs
    int OnRender();                              // ray end pass + volume pass
    int OnFrame() { int rc = OnUpdate(); return rc != VR_OK ? rc : OnRender(); }
    int OnResize(uint32_t width, uint32_t height);

    Camera& GetCamera() { return m_Camera; }
    MiniApp* GetApp() { return p_App.get(); }
    vr_ctx* GetContext() { return p_Ctx; }
    const vr_uniforms& GetUniforms() const { return m_Uniforms; }

    // what the ImGui sliders edit (Application.cpp:243-272)
    int m_FragmentMode = 0;
    int m_StepsCount = 200;
    float m_StepSize = 0.01f;
    vrm::vec2 m_ClipsX{}, m_ClipsY{}, m_ClipsZ{};
    bool m_BToggles[4] = {false, false, false, false};  // (variable step size, jitter, -, -)
    bool m_PrepareOnDevice = false;  // forwarded to the scene in OnStart (MiniApp::SetPrepareOnDevice)

    // What is under pixel (x, y) of the running scene's frame with the uniforms of the last OnUpdate (vr_pick: the surface position,
    // its depth, the voxel and the values of every volume there).  Scenes drawn as BASIC, LIGHT or ISO; any other returns
    // VR_ERR_UNSUPPORTED.  The frame of the last OnRender and its counters stay what they were.
    int Pick(uint32_t x, uint32_t y, vr_pick_result* out);
    // A slice view of one of the scene's volumes (vr_slice_render: a plane in texture space, any output size, any slot) into host
    // memory: desc.width * desc.height float4, or 32-bit words for VR_SLICE_BGRA8.  The frame of the last OnRender and its counters stay.
    int Slice(const vr_slice_desc& desc, void* out_host);
    // The axis-aligned plane `axis` (0 x, 1 y, 2 z) through the voxel under a picked pixel (pick.voxel of volume slot 0), `thickness`
    // voxels of maximum-intensity slab around it, through TF slot 0: rgba = *w x *h float4, one pixel per voxel.  A pick without a
    // hit returns VR_ERR_INVALID_ARG.
    int SliceThroughPick(const vr_pick_result& pick, int axis, int thickness, std::vector<float>& rgba, uint32_t* w, uint32_t* h);
    // A histogram of one of the scene's volumes (vr_histogram): counts = uint64[VR_HIST_ROWS * desc.bins], rows = vr_hist_row[VR_HIST_ROWS],
    // host memory.  The frame of the last OnRender and its counters stay.
    int Histogram(const vr_hist_desc& desc, uint64_t* counts, vr_hist_row* rows);
    // The cumulative dose-volume histogram of contour `contour` (0 .. 3) of volume maskSlot: .a of volume doseSlot binned as
    // (int)(dose * scale) into `bins` bins (CLAMP), then atLeast[b] = the sum of counts[k] over k >= b -- the voxels of the structure
    // that receive at least the dose of bin b; atLeast[0] is the structure's voxel count.
    int DoseVolumeHistogram(int doseSlot, int maskSlot, int contour, uint32_t bins, float scale, std::vector<uint64_t>& atLeast);
    // The structure under a picked pixel as contour `contour` (0 .. 3) of volume maskSlot: the voxels of volume valueSlot whose .a lies
    // in [lo, hi] and that are connected to pick.voxel (vr_segment_grow over the whole volume, VR_GROW_REPLACE; connectivity =
    // VR_GROW_FACES / VR_GROW_ALL).  `out` may be nullptr.  A pick without a hit returns VR_ERR_INVALID_ARG.
    int GrowFromPick(const vr_pick_result& pick, int valueSlot, int maskSlot, int contour, float lo, float hi, int connectivity, vr_grow_result* out);
    // Morphology and algebra of mask contours on the device (vr_mask_morph of include/vr.h): dilate, erode, close or open a contour by a
    // structuring element, or take it as it is, and combine the result into a contour.  `out` may be nullptr.
    int MorphContour(const vr_morph_desc& desc, vr_morph_result* out);
    // Contour srcContour of volume srcSlot grown by a margin of `mm` millimetres on the voxel grid of `grid` (its PixelSpacing and
    // SliceThickness), into contour dstContour of volume dstSlot: VR_MORPH_DILATE with VR_MORPH_REPLACE over the whole volume by
    // vr_morph_ball, the spacings and the radius each rounded to whole micrometres with lround.  VR_ERR_INVALID_ARG for a margin that
    // is negative or not finite, a spacing that is not positive, or a margin beyond VR_MORPH_MAX_RADIUS voxels on some axis.
    int MarginMm(int srcSlot, int srcContour, int dstSlot, int dstContour, float mm, const VolumeFileDcm& grid, vr_morph_result* out);
    // Exact distance maps of a mask contour on the device (vr_mask_distance of include/vr.h): a descriptor passed through.  `out` may be
    // nullptr.
    int DistanceMap(const vr_dist_desc& desc, vr_dist_result* out);
    // The distance in millimetres from contour srcContour of volume srcSlot, over the whole volume on the voxel grid of `grid` (its
    // PixelSpacing and SliceThickness), into component dstChannel of volume dstSlot: mode = VR_DIST_OUTSIDE / VR_DIST_INSIDE /
    // VR_DIST_SIGNED, limitMm = where the map saturates (0: nowhere).  The spacings and the limit are each rounded to whole micrometres
    // with lround, as MarginMm does, and scale = 0.001f.  VR_ERR_INVALID_ARG for a limit that is negative or not finite, a spacing that
    // is not positive, or a volume longer than 2^30 micrometres on some axis.
    int DistanceMm(int srcSlot, int srcContour, int dstSlot, int dstChannel, int mode, float limitMm, const VolumeFileDcm& grid,
                   vr_dist_result* out);
    // Volume srcSlot, which holds `src`, resampled onto the voxel grid of `grid` into volume dstSlot (vr_resample_between +
    // vr_volume_resample of include/vr.h): a dose onto the CT's grid, a second series onto the first's, a structure onto the dose grid.
    // Both grids in patient millimetres from GetVolumeParams() and GetSize(): ImagePositionPatient is the centre of voxel (0, 0, 0),
    // PixelSpacing x / y and SliceThickness the pitch -- the convention of Create3DMask and ContoursToMask.  channels: bit c =
    // component c is written; filter = VR_RESAMPLE_LINEAR / VR_RESAMPLE_NEAREST; outside[4] is stored where a voxel of `grid` lies
    // outside `src`.  dstToSrc: a row-major 3 x 4 map from `grid`'s patient coordinates to `src`'s (a rigid registration's result),
    // nullptr = the identity: one frame of reference.  An empty dstSlot is created on `grid`'s size.  `out` may be nullptr.
    // VR_ERR_INVALID_ARG when srcSlot does not hold a volume of `src`'s size or a filled dstSlot is not of `grid`'s size, and for a
    // spacing that is not positive.
    int ResampleOnto(const VolumeFileDcm& src, int srcSlot, const VolumeFileDcm& grid, int dstSlot, uint32_t channels, int filter,
                     const float outside[4], vr_resample_result* out, const double dstToSrc[12] = nullptr);
    // Closed planar polygons rasterised into contours of a mask volume on the device (vr_mask_polygons of include/vr.h): a descriptor
    // passed through.  `out` may be nullptr.
    int RasterPolygons(const vr_polygons_desc& desc, vr_polygons_result* out);
    // The structures contourIDs of an RTSTRUCT file as the contours of volume dstSlot, on the voxel grid of `grid` (a volume read from
    // DICOM in the same frame of reference; volume slot 0, the scene's first volume, holds it or one of its size): ONE vr_mask_polygons
    // with VR_MORPH_REPLACE over the whole grid, so one rebuild.  Channel l comes from the l-th accepted id as in StructureFileDcm::Create3DMask (ids are 1-based;
    // 0 and anything >= the number of structures are ignored).  Patient millimetres become whole micrometres by llround(v * 1000.0) in
    // double -- the points' x and y, ImagePositionPatient x / y and PixelSpacing -- and a polygon lies on the slice ContourSliceNumber gives
    // for its first point.  rule = VR_POLY_EVEN_ODD / VR_POLY_UNION.  VR_ERR_INVALID_ARG for another frame of reference, no accepted id,
    // a spacing that is not positive, a coordinate beyond 2^29 micrometres or a volume 0 of another size than `grid`.
    int ContoursToMask(const StructureFileDcm& structures, std::array<int, 4> contourIDs, const VolumeFileDcm& grid, int dstSlot, int rule,
                       vr_polygons_result* out);
    // The contours of a mask volume traced into closed planar polygons on the device (vr_mask_outlines of include/vr.h): a descriptor
    // passed through.  `out` may be nullptr.
    int MaskOutlines(const vr_outlines_desc& desc, vr_outlines_result* out);
    // The inverse of ContoursToMask: the contours `contours` (bit k: contour k) of volume srcSlot as structures in patient millimetres
    // on the voxel grid of `grid` (a volume read from DICOM, of srcSlot's size), the whole volume, connect = VR_OUTLINE_SPLIT /
    // VR_OUTLINE_JOIN.  The grid is taken in whole micrometres by the same llround(v * 1000.0) of ImagePositionPatient x / y and
    // PixelSpacing, the offset is half a spacing rounded down.  out[l] = the polygons of the l-th traced contour, each flat x y z floats
    // (the layout StructureFileDcm holds), z = that of the polygon's slice, the inverse of ContourSliceNumber.  VR_ERR_INVALID_ARG for a
    // spacing that is not positive, a coordinate beyond 2^29 micrometres or a volume of another size than `grid`.
    int MaskToContours(int srcSlot, int contours, int connect, const VolumeFileDcm& grid, std::vector<std::vector<std::vector<float>>>& out);
    // The surface {value >= level} of component `channel` of volume `slot` over the whole volume as a triangle mesh, extracted on the
    // device (vr_volume_mesh of include/vr.h: marching tetrahedra; cap = 1 closes the mesh at the volume's faces): the counting call and
    // the call that stores.  The positions are the voxel indices times `spacing` (x, y, z; nullptr = 1), multiplied in double on the
    // host; with `grid` its PixelSpacing and SliceThickness in millimetres.  VR_ERR_INVALID_ARG for a spacing that is not finite and
    // positive.
    int ExtractSurface(int slot, int channel, float level, int cap, SurfaceMesh& out, const double spacing[3] = nullptr);
    int ExtractSurface(int slot, int channel, float level, int cap, const VolumeFileDcm& grid, SurfaceMesh& out);
    // Component srcChannel of volume srcSlot smoothed by a Gaussian of sigmaMm millimetres over the whole volume into component dstChannel
    // of volume dstSlot, on the device (vr_filter_gaussian + vr_volume_filter of include/vr.h; VR_FILTER_CLAMP): per axis sigma in voxels =
    // sigmaMm / spacing[a] (x, y, z in millimetres; nullptr = 1), truncate 4; with `grid` its PixelSpacing and SliceThickness.  An axis
    // whose radius comes out 0 gets no pass; sigmaMm == 0 copies.  Source and destination may coincide.  `out` may be nullptr.
    // VR_ERR_INVALID_ARG for a sigma that is negative or not finite, a spacing that is not finite and positive, or a radius beyond
    // VR_FILTER_MAX_RADIUS voxels on some axis.
    int Smooth(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double sigmaMm, const double spacing[3] = nullptr,
               vr_filter_result* out = nullptr);
    int Smooth(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double sigmaMm, const VolumeFileDcm& grid, vr_filter_result* out = nullptr);
    // Gaussian derivatives of component 3 of volume `slot` into its components 0, 1, 2: three vr_volume_filter calls, each the first
    // derivative (order 1) along its own axis and the Gaussian (order 0) along the other two, sigma and spacing as Smooth takes them.  The values are
    // derivatives per VOXEL, unscaled: the caller normalises them (and divides by the spacing for a gradient in 1 / mm).  Component 3 is
    // left alone.  VR_ERR_INVALID_ARG as Smooth, and where the radius comes out 0 on some axis (a derivative needs neighbours).
    int GradientOfGaussian(int slot, double sigmaMm, const double spacing[3] = nullptr);
    int GradientOfGaussian(int slot, double sigmaMm, const VolumeFileDcm& grid);
    // The value at position `rank` (0 .. N - 1, VR_RANK_MEDIAN or VR_RANK_MAX) of the ascending order of the values in a box window of
    // radiusMm millimetres around every voxel of component srcChannel of volume srcSlot, over the whole volume into component dstChannel
    // of volume dstSlot, on the device (vr_volume_rank of include/vr.h; VR_FILTER_CLAMP): per axis the radius in voxels is
    // (int)(radiusMm / spacing[a] + 0.5) (x, y, z in millimetres; nullptr = 1); with `grid` its PixelSpacing and SliceThickness.  Source
    // and destination may coincide.  `out` may be nullptr.  VR_ERR_INVALID_ARG for a radiusMm that is negative or not finite, a spacing
    // that is not finite and positive, or a radius beyond VR_RANK_MAX_RADIUS voxels on some axis.  Median: the same with VR_RANK_MEDIAN.
    int RankFilter(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, int rank, const double spacing[3] = nullptr,
                   vr_rank_result* out = nullptr);
    int RankFilter(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, int rank, const VolumeFileDcm& grid,
                   vr_rank_result* out = nullptr);
    int Median(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, const double spacing[3] = nullptr,
               vr_rank_result* out = nullptr);
    int Median(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, const VolumeFileDcm& grid, vr_rank_result* out = nullptr);
    // The gamma index of component evalChannel of volume evalSlot against component refChannel of volume refSlot, over the whole volume
    // into component dstChannel of volume dstSlot, on the device (vr_volume_gamma of include/vr.h).  doseTolerance is in the doses' own
    // unit (3 % of the prescription, say: the library does not guess a normalisation dose), or a fraction under VR_GAMMA_LOCAL.
    // Millimetres become whole micrometres by llround(mm * 1000.0): dtaMm, the reach and the spacing (x, y, z; nullptr = 1 mm; with
    // `grid` its PixelSpacing and SliceThickness).  `out` may be nullptr.  VR_ERR_INVALID_ARG for a dtaMm, reach or spacing that is not
    // finite and positive or leaves vr_volume_gamma's ranges, and whatever else vr_volume_gamma refuses.
    int Gamma(int refSlot, int refChannel, int evalSlot, int evalChannel, int dstSlot, int dstChannel, float doseTolerance, double dtaMm,
              const double spacing[3] = nullptr, const GammaOptions& options = GammaOptions(), vr_gamma_result* out = nullptr);
    int Gamma(int refSlot, int refChannel, int evalSlot, int evalChannel, int dstSlot, int dstChannel, float doseTolerance, double dtaMm,
              const VolumeFileDcm& grid, const GammaOptions& options = GammaOptions(), vr_gamma_result* out = nullptr);
    // the accumulated opacity at which the unlit / lit scene's surface lies (vr_set_surface_threshold: finite, 0 <= tau < 1)
    int SetSurfaceThreshold(float tau);

    // read back the fragment output / the presented BGRA8 frame of the last OnRender
    int ReadFrame(float* frag_rgba, uint8_t* present_bgra8 = nullptr, uint64_t* samples = nullptr);

    uint32_t Width() const { return m_Width; }
    uint32_t Height() const { return m_Height; }

private:
    uint32_t m_Width, m_Height;
    Camera m_Camera;
    vr_ctx* p_Ctx = nullptr;
    std::unique_ptr<MiniApp> p_App;
    vr_uniforms m_Uniforms{};
    std::string m_Error;
};

}  // namespace med
