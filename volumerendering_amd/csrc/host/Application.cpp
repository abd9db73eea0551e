#include "Application.h"

#include <cmath>
#include <cstring>

namespace med {

Application::Application(uint32_t width, uint32_t height, int device)
    : m_Width(width), m_Height(height),
      m_Camera(Camera::CreatePerspective(vrm::radians(60.0f), static_cast<float>(width) / static_cast<float>(height), 0.01f, 100.0f))
{
    if (vr_create(&p_Ctx, width, height, device) != VR_OK) {
        m_Error = vr_last_error(nullptr);
        p_Ctx = nullptr;
    }
}

Application::~Application()
{
    if (p_App) p_App->OnEnd();
    p_App.reset();
    vr_destroy(p_Ctx);
}

int Application::OnStart(std::unique_ptr<MiniApp> app)
{
    p_App = std::move(app);
    if (!p_Ctx || !p_App) return VR_ERR_NOT_READY;
    p_App->SetPrepareOnDevice(m_PrepareOnDevice);
    p_App->OnStart(p_Ctx);
    if (p_App->StartStatus() != VR_OK) {  // an upload or a device-preparation call failed (out of memory, bad size ...)
        m_Error = vr_last_error(p_Ctx);
        if (m_Error.empty()) m_Error = "scene start failed: volume data does not match its declared size";
        return p_App->StartStatus();
    }
    // "Using MiniApp's required step size / count" (Application.cpp:74-84)
    if (p_App->GetStepSize() != 0.0f) m_StepSize = p_App->GetStepSize();
    if (p_App->GetStepsCount() != 0) m_StepsCount = p_App->GetStepsCount();
    return VR_OK;
}

int Application::OnUpdate()
{
    if (!p_Ctx) return VR_ERR_HIP;
    vr_uniforms& u = m_Uniforms;
    std::memset(&u, 0, sizeof u);
    const vrm::mat4 model(1.0f);  // dummy_model, never rewritten (Application.cpp:489-492)
    std::memcpy(u.model, model.data(), sizeof u.model);
    std::memcpy(u.view, m_Camera.GetViewMatrix().data(), sizeof u.view);
    std::memcpy(u.proj, m_Camera.GetProjectionMatrix().data(), sizeof u.proj);
    std::memcpy(u.view_inv, m_Camera.GetInverseViewMatrix().data(), sizeof u.view_inv);
    std::memcpy(u.proj_inv, m_Camera.GetInverseProjectionMatrix().data(), sizeof u.proj_inv);
    const vrm::vec3 pos = m_Camera.GetPosition();
    u.camera_pos[0] = pos.x; u.camera_pos[1] = pos.y; u.camera_pos[2] = pos.z;
    u.fragment_mode = m_FragmentMode;
    u.steps_count = m_StepsCount;
    u.step_size = m_StepSize;
    u.clip_x[0] = m_ClipsX.x; u.clip_x[1] = m_ClipsX.y;
    u.clip_y[0] = m_ClipsY.x; u.clip_y[1] = m_ClipsY.y;
    u.clip_z[0] = m_ClipsZ.x; u.clip_z[1] = m_ClipsZ.y;
    for (int i = 0; i < 4; ++i) u.toggles[i] = m_BToggles[i] ? 1 : 0;
    if (p_App && p_App->GetLight()) {
        const Light* l = p_App->GetLight();
        std::memcpy(u.light_pos, &l->Position.x, sizeof u.light_pos);
        std::memcpy(u.light_ambient, &l->Ambient.x, sizeof u.light_ambient);
        std::memcpy(u.light_diffuse, &l->Diffuse.x, sizeof u.light_diffuse);
    }
    int rc = vr_set_uniforms(p_Ctx, &u);
    if (rc != VR_OK) { m_Error = vr_last_error(p_Ctx); return rc; }
    if (p_App) p_App->OnUpdate();
    return VR_OK;
}

int Application::OnRender()
{
    if (!p_Ctx || !p_App) return VR_ERR_NOT_READY;
    int rc = p_App->OnRender(p_Ctx);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::OnResize(uint32_t width, uint32_t height)
{
    // like the reference, the camera's aspect ratio is NOT updated on resize (SetAspectRatio is never called,
    // Application.cpp:299-323); callers that want it call GetCamera().SetAspectRatio themselves
    m_Width = width;
    m_Height = height;
    int rc = vr_resize(p_Ctx, width, height);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::Slice(const vr_slice_desc& desc, void* out_host)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    int rc = vr_slice_render(p_Ctx, &desc, out_host);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::SliceThroughPick(const vr_pick_result& pick, int axis, int thickness, std::vector<float>& rgba, uint32_t* w, uint32_t* h)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    if (!pick.hit || axis < 0 || axis > 2) return VR_ERR_INVALID_ARG;
    vr_slice_desc d;
    int rc = vr_slice_orthogonal(p_Ctx, 0, axis, pick.voxel[axis], thickness, &d);
    if (rc != VR_OK) return rc;
    rgba.resize((size_t)d.width * d.height * 4);
    rc = Slice(d, rgba.data());
    if (rc != VR_OK) return rc;
    if (w) *w = d.width;
    if (h) *h = d.height;
    return VR_OK;
}

int Application::Histogram(const vr_hist_desc& desc, uint64_t* counts, vr_hist_row* rows)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    int rc = vr_histogram(p_Ctx, &desc, counts, rows);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::DoseVolumeHistogram(int doseSlot, int maskSlot, int contour, uint32_t bins, float scale, std::vector<uint64_t>& atLeast)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    if (contour < 0 || contour > 3) return VR_ERR_INVALID_ARG;
    vr_hist_desc d;
    int rc = vr_hist_whole(p_Ctx, doseSlot, bins, scale, &d);
    if (rc != VR_OK) return rc;
    d.mask_slot = maskSlot;
    d.rows = 2u << contour;
    std::vector<uint64_t> counts((size_t)VR_HIST_ROWS * bins);
    vr_hist_row rows[VR_HIST_ROWS];
    rc = Histogram(d, counts.data(), rows);
    if (rc != VR_OK) return rc;
    atLeast.assign(bins, 0);
    uint64_t sum = 0;
    for (size_t b = bins; b-- > 0;) {
        sum += counts[(size_t)(1 + contour) * bins + b];
        atLeast[b] = sum;
    }
    return VR_OK;
}

int Application::GrowFromPick(const vr_pick_result& pick, int valueSlot, int maskSlot, int contour, float lo, float hi, int connectivity,
                              vr_grow_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    if (!pick.hit) return VR_ERR_INVALID_ARG;
    vr_grow_desc d;
    int rc = vr_grow_whole(p_Ctx, valueSlot, maskSlot, contour, lo, hi, &d);
    if (rc != VR_OK) return rc;
    d.connectivity = connectivity;
    d.n_seeds = 1;
    for (int a = 0; a < 3; ++a) d.seeds[0][a] = pick.voxel[a];
    rc = vr_segment_grow(p_Ctx, &d, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::MorphContour(const vr_morph_desc& desc, vr_morph_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const int rc = vr_mask_morph(p_Ctx, &desc, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::MarginMm(int srcSlot, int srcContour, int dstSlot, int dstContour, float mm, const VolumeFileDcm& grid, vr_morph_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double mmOf[4] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness, (double)mm};
    uint32_t um[4];
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(mmOf[i]) || mmOf[i] < 0.0 || mmOf[i] > 4.0e6) return VR_ERR_INVALID_ARG;  // (micrometres fit 32 bits)
        um[i] = (uint32_t)std::lround(mmOf[i] * 1000.0);
    }
    vr_morph_desc d;
    int rc = vr_morph_whole(p_Ctx, srcSlot, srcContour, dstSlot, dstContour, VR_MORPH_DILATE, &d);
    if (rc != VR_OK) return rc;
    rc = vr_morph_ball(um, um[3], &d.element);
    if (rc != VR_OK) return rc;
    return MorphContour(d, out);
}

int Application::DistanceMap(const vr_dist_desc& desc, vr_dist_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const int rc = vr_mask_distance(p_Ctx, &desc, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::DistanceMm(int srcSlot, int srcContour, int dstSlot, int dstChannel, int mode, float limitMm, const VolumeFileDcm& grid,
                            vr_dist_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double mmOf[4] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness, (double)limitMm};
    uint32_t um[4];
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(mmOf[i]) || mmOf[i] < 0.0 || mmOf[i] > 4.0e6) return VR_ERR_INVALID_ARG;  // (micrometres fit 32 bits)
        um[i] = (uint32_t)std::lround(mmOf[i] * 1000.0);
    }
    vr_dist_desc d;
    const int rc = vr_dist_whole(p_Ctx, srcSlot, srcContour, dstSlot, dstChannel, mode, &d);
    if (rc != VR_OK) return rc;
    for (int a = 0; a < 3; ++a) d.spacing[a] = um[a];
    d.limit = um[3];
    d.scale = 0.001f;
    return DistanceMap(d, out);
}

int Application::ResampleOnto(const VolumeFileDcm& src, int srcSlot, const VolumeFileDcm& grid, int dstSlot, uint32_t channels, int filter,
                              const float outside[4], vr_resample_result* out, const double dstToSrc[12])
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    if (!outside) return VR_ERR_INVALID_ARG;
    auto gridOf = [](const VolumeFileDcm& f) {
        const DicomVolumeParams p = f.GetVolumeParams();
        const auto [x, y, z] = f.GetSize();
        vr_grid g;
        g.n[0] = (int32_t)x, g.n[1] = (int32_t)y, g.n[2] = (int32_t)z;
        for (int a = 0; a < 3; ++a) g.origin[a] = p.ImagePositionPatient[a];
        g.spacing[0] = p.PixelSpacing[0], g.spacing[1] = p.PixelSpacing[1], g.spacing[2] = p.SliceThickness;
        return g;
    };
    const vr_grid gs = gridOf(src), gd = gridOf(grid);
    vr_resample_desc d;
    int rc = vr_resample_identity(p_Ctx, srcSlot, dstSlot, filter, &d);  // (the slots, the filter, and the size srcSlot holds)
    if (rc != VR_OK) return rc;
    for (int a = 0; a < 3; ++a)
        if (d.dst_n[a] != gs.n[a]) return VR_ERR_INVALID_ARG;
    rc = vr_resample_between(&gs, &gd, dstToSrc, &d);
    if (rc != VR_OK) return rc;
    d.channels = channels;
    for (int k = 0; k < 4; ++k) d.outside[k] = outside[k];
    rc = vr_volume_resample(p_Ctx, &d, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::RasterPolygons(const vr_polygons_desc& desc, vr_polygons_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const int rc = vr_mask_polygons(p_Ctx, &desc, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::ContoursToMask(const StructureFileDcm& structures, std::array<int, 4> contourIDs, const VolumeFileDcm& grid, int dstSlot,
                                int rule, vr_polygons_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    if (!structures.CompareFrameOfReference(grid)) return VR_ERR_INVALID_ARG;
    const DicomVolumeParams p = grid.GetVolumeParams();
    // whole micrometres within the range of vr_mask_polygons, or false
    auto um = [](double mm, int32_t* v) {
        if (!std::isfinite(mm) || std::fabs(mm) * 1000.0 > (double)(1 << 29)) return false;
        *v = (int32_t)std::llround(mm * 1000.0);
        return true;
    };
    vr_polygons_desc d;
    int rc = vr_polygons_whole(p_Ctx, 0, dstSlot, &d);
    if (rc != VR_OK) return rc;
    const auto [xSize, ySize, zSize] = grid.GetSize();
    if ((int)xSize != d.box_hi[0] || (int)ySize != d.box_hi[1] || (int)zSize != d.box_hi[2]) return VR_ERR_INVALID_ARG;
    int32_t pitch[2];
    for (int a = 0; a < 2; ++a) {
        if (!um(p.ImagePositionPatient[a], &d.origin[a]) || !um(p.PixelSpacing[a], &pitch[a]) || pitch[a] <= 0) return VR_ERR_INVALID_ARG;
        d.spacing[a] = (uint32_t)pitch[a];
    }
    const auto& data = structures.GetContourData();
    std::vector<int32_t> points;
    std::vector<vr_polygon> polygons;
    int channels = 0;
    for (int id : contourIDs) {
        if (!(id > 0 && static_cast<size_t>(id) < data.size())) continue;
        for (const std::vector<float>& polygon : data[static_cast<size_t>(id - 1)]) {
            if (polygon.size() < 3) continue;
            vr_polygon g;
            g.first = (uint32_t)(points.size() / 2);
            g.count = (uint32_t)(polygon.size() / 3);
            g.slice = (int32_t)ContourSliceNumber(polygon[2], static_cast<float>(p.ImagePositionPatient[2]), static_cast<float>(p.SliceThickness));
            g.contour = channels;
            for (size_t j = 0; j + 3 <= polygon.size(); j += 3) {
                int32_t xy[2];
                if (!um((double)polygon[j], &xy[0]) || !um((double)polygon[j + 1], &xy[1])) return VR_ERR_INVALID_ARG;
                points.push_back(xy[0]);
                points.push_back(xy[1]);
            }
            polygons.push_back(g);
        }
        ++channels;
    }
    if (channels == 0) return VR_ERR_INVALID_ARG;
    d.contours = (1 << channels) - 1;
    d.rule = rule;
    d.n_points = (uint32_t)(points.size() / 2);
    d.n_polygons = (uint32_t)polygons.size();
    d.points = points.data();
    d.polygons = polygons.data();
    return RasterPolygons(d, out);
}

int Application::MaskOutlines(const vr_outlines_desc& desc, vr_outlines_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const int rc = vr_mask_outlines(p_Ctx, &desc, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::MaskToContours(int srcSlot, int contours, int connect, const VolumeFileDcm& grid, std::vector<std::vector<std::vector<float>>>& out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const DicomVolumeParams p = grid.GetVolumeParams();
    // whole micrometres within the range of vr_mask_outlines, or false
    auto um = [](double mm, int32_t* v) {
        if (!std::isfinite(mm) || std::fabs(mm) * 1000.0 > (double)(1 << 29)) return false;
        *v = (int32_t)std::llround(mm * 1000.0);
        return true;
    };
    vr_outlines_desc d;
    int rc = vr_outlines_whole(p_Ctx, srcSlot, &d);
    if (rc != VR_OK) return rc;
    const auto [xSize, ySize, zSize] = grid.GetSize();
    if ((int)xSize != d.box_hi[0] || (int)ySize != d.box_hi[1] || (int)zSize != d.box_hi[2]) return VR_ERR_INVALID_ARG;
    for (int a = 0; a < 2; ++a) {
        int32_t pitch;
        if (!um(p.ImagePositionPatient[a], &d.origin[a]) || !um(p.PixelSpacing[a], &pitch) || pitch <= 0) return VR_ERR_INVALID_ARG;
        d.spacing[a] = (uint32_t)pitch;
        d.offset[a] = (uint32_t)pitch / 2u;
    }
    d.contours = contours;
    d.connect = connect;
    vr_outlines_result r;
    rc = MaskOutlines(d, &r);  // the counting call
    if (rc != VR_OK) return rc;
    std::vector<int32_t> points((size_t)r.n_points * 2);
    std::vector<vr_polygon> polygons(r.n_polygons);
    if (r.n_points != 0) {
        d.max_points = r.n_points;
        d.max_polygons = r.n_polygons;
        d.points = points.data();
        d.polygons = polygons.data();
        rc = MaskOutlines(d, &r);
        if (rc != VR_OK) return rc;
    }
    int place[4] = {-1, -1, -1, -1}, traced = 0;
    for (int k = 0; k < 4; ++k)
        if ((contours >> k) & 1) place[k] = traced++;
    out.assign((size_t)traced, {});
    const float z0 = static_cast<float>(p.ImagePositionPatient[2]), dz = static_cast<float>(p.SliceThickness);
    for (const vr_polygon& g : polygons) {
        std::vector<float> flat;
        flat.reserve((size_t)g.count * 3);
        const float z = z0 + static_cast<float>(g.slice) * dz;
        for (uint32_t e = g.first; e < g.first + g.count; ++e) {
            flat.push_back(static_cast<float>(points[(size_t)e * 2] / 1000.0));
            flat.push_back(static_cast<float>(points[(size_t)e * 2 + 1] / 1000.0));
            flat.push_back(z);
        }
        out[(size_t)place[g.contour]].push_back(std::move(flat));
    }
    return VR_OK;
}

int Application::ExtractSurface(int slot, int channel, float level, int cap, SurfaceMesh& out, const double spacing[3])
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    const double unit[3] = {1.0, 1.0, 1.0};
    const double* const sp = spacing ? spacing : unit;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(sp[a]) || !(sp[a] > 0.0)) return VR_ERR_INVALID_ARG;
    vr_mesh_desc d;
    int rc = vr_mesh_whole(p_Ctx, slot, &d);
    if (rc != VR_OK) return rc;
    d.channel = channel;
    d.level = level;
    d.cap = cap;
    out = SurfaceMesh{};
    rc = vr_volume_mesh(p_Ctx, &d, &out.result);  // the counting call
    std::vector<float> verts((size_t)out.result.n_vertices * 3);
    out.triangles.assign((size_t)out.result.n_triangles * 3, 0u);
    if (rc == VR_OK && out.result.n_vertices != 0) {
        d.max_vertices = out.result.n_vertices;
        d.max_triangles = out.result.n_triangles;
        d.vertices = verts.data();
        d.triangles = out.triangles.data();
        rc = vr_volume_mesh(p_Ctx, &d, &out.result);
    }
    if (rc != VR_OK) {
        m_Error = vr_last_error(p_Ctx);
        return rc;
    }
    out.positions.resize(verts.size());
    for (size_t i = 0; i < verts.size(); ++i) out.positions[i] = static_cast<double>(verts[i]) * sp[i % 3];
    return VR_OK;
}

int Application::ExtractSurface(int slot, int channel, float level, int cap, const VolumeFileDcm& grid, SurfaceMesh& out)
{
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double spacing[3] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness};
    return ExtractSurface(slot, channel, level, cap, out, spacing);
}

namespace {

// The Gaussian weights of Smooth and GradientOfGaussian per axis and order ([order][axis]; truncate 4) and their radii: VR_OK, or
// VR_ERR_INVALID_ARG for a sigma that is negative or not finite, a spacing that is not finite and positive or a radius beyond the
// maximum.  An axis whose radius is 0 has no weights.
struct GaussianTaps {
    float w[2][3][2 * VR_FILTER_MAX_RADIUS + 1];
    int radius[3];
};
int gaussianTaps(double sigmaMm, const double spacing[3], GaussianTaps& g)
{
    if (!std::isfinite(sigmaMm) || sigmaMm < 0.0) return VR_ERR_INVALID_ARG;
    for (int a = 0; a < 3; ++a) {
        const double sp = spacing ? spacing[a] : 1.0;
        if (!std::isfinite(sp) || !(sp > 0.0)) return VR_ERR_INVALID_ARG;
        const double sigma = sigmaMm / sp;
        g.radius[a] = 0;
        if (!(4.0 * sigma + 0.5 >= 1.0)) continue;  // (radius 0, sigma 0 included: no pass)
        for (int order = 0; order < 2; ++order)
            if (const int rc = vr_filter_gaussian(sigma, order, 4.0, g.w[order][a], 2 * VR_FILTER_MAX_RADIUS + 1, &g.radius[a])) return rc;
    }
    return VR_OK;
}

}  // namespace

int Application::Smooth(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double sigmaMm, const double spacing[3], vr_filter_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    GaussianTaps g;
    int rc = gaussianTaps(sigmaMm, spacing, g);
    if (rc != VR_OK) return rc;
    vr_filter_desc d;
    rc = vr_filter_whole(p_Ctx, srcSlot, srcChannel, dstSlot, dstChannel, &d);
    if (rc != VR_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        d.radius[a] = g.radius[a];
        d.taps[a] = g.radius[a] != 0 ? g.w[0][a] : nullptr;
    }
    rc = vr_volume_filter(p_Ctx, &d, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::Smooth(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double sigmaMm, const VolumeFileDcm& grid, vr_filter_result* out)
{
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double spacing[3] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness};
    return Smooth(srcSlot, srcChannel, dstSlot, dstChannel, sigmaMm, spacing, out);
}

int Application::GradientOfGaussian(int slot, double sigmaMm, const double spacing[3])
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    GaussianTaps g;
    int rc = gaussianTaps(sigmaMm, spacing, g);
    if (rc != VR_OK) return rc;
    for (int a = 0; a < 3; ++a)
        if (g.radius[a] == 0) return VR_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) {  // component k: the derivative along axis k of the smoothed component 3
        vr_filter_desc d;
        rc = vr_filter_whole(p_Ctx, slot, 3, slot, k, &d);
        if (rc != VR_OK) return rc;
        for (int a = 0; a < 3; ++a) {
            d.radius[a] = g.radius[a];
            d.taps[a] = g.w[a == k ? 1 : 0][a];
        }
        rc = vr_volume_filter(p_Ctx, &d, nullptr);
        if (rc != VR_OK) {
            m_Error = vr_last_error(p_Ctx);
            return rc;
        }
    }
    return VR_OK;
}

int Application::GradientOfGaussian(int slot, double sigmaMm, const VolumeFileDcm& grid)
{
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double spacing[3] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness};
    return GradientOfGaussian(slot, sigmaMm, spacing);
}

int Application::RankFilter(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, int rank, const double spacing[3],
                            vr_rank_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    if (!std::isfinite(radiusMm) || radiusMm < 0.0) return VR_ERR_INVALID_ARG;
    int radius[3];
    for (int a = 0; a < 3; ++a) {
        const double sp = spacing ? spacing[a] : 1.0;
        if (!std::isfinite(sp) || !(sp > 0.0)) return VR_ERR_INVALID_ARG;
        const double reach = radiusMm / sp + 0.5;
        if (!(reach < (double)(VR_RANK_MAX_RADIUS + 1))) return VR_ERR_INVALID_ARG;
        radius[a] = (int)reach;
    }
    vr_rank_desc d;
    int rc = vr_rank_whole(p_Ctx, srcSlot, srcChannel, dstSlot, dstChannel, &d);
    if (rc != VR_OK) return rc;
    for (int a = 0; a < 3; ++a) d.radius[a] = radius[a];
    d.rank = rank;
    rc = vr_volume_rank(p_Ctx, &d, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::RankFilter(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, int rank, const VolumeFileDcm& grid,
                            vr_rank_result* out)
{
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double spacing[3] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness};
    return RankFilter(srcSlot, srcChannel, dstSlot, dstChannel, radiusMm, rank, spacing, out);
}

int Application::Median(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, const double spacing[3], vr_rank_result* out)
{
    return RankFilter(srcSlot, srcChannel, dstSlot, dstChannel, radiusMm, VR_RANK_MEDIAN, spacing, out);
}

int Application::Median(int srcSlot, int srcChannel, int dstSlot, int dstChannel, double radiusMm, const VolumeFileDcm& grid, vr_rank_result* out)
{
    return RankFilter(srcSlot, srcChannel, dstSlot, dstChannel, radiusMm, VR_RANK_MEDIAN, grid, out);
}

int Application::Gamma(int refSlot, int refChannel, int evalSlot, int evalChannel, int dstSlot, int dstChannel, float doseTolerance, double dtaMm,
                       const double spacing[3], const GammaOptions& options, vr_gamma_result* out)
{
    if (!p_Ctx) return VR_ERR_NOT_READY;
    // millimetres into whole micrometres; 0: not finite, not positive or beyond `most`
    const auto um = [](double mm, long long most) -> uint32_t {
        if (!std::isfinite(mm) || !(mm > 0.0) || mm * 1000.0 > (double)most) return 0u;
        const long long v = std::llround(mm * 1000.0);
        return v >= 1 && v <= most ? (uint32_t)v : 0u;
    };
    vr_gamma_desc d;
    int rc = vr_gamma_whole(p_Ctx, refSlot, refChannel, evalSlot, evalChannel, dstSlot, dstChannel, &d);
    if (rc != VR_OK) {
        m_Error = "Application::Gamma: a slot or channel is out of range, or the reference slot is empty";
        return rc;
    }
    for (int a = 0; a < 3; ++a) d.spacing[a] = um(spacing ? spacing[a] : 1.0, 1ll << 20);
    d.dta = um(dtaMm, 1ll << 24);
    d.reach = um(options.reachMm != 0.0 ? options.reachMm : 2.0 * dtaMm, 1ll << 24);
    if (d.spacing[0] == 0u || d.spacing[1] == 0u || d.spacing[2] == 0u || d.dta == 0u || d.reach == 0u) {
        m_Error = "Application::Gamma: dtaMm, the reach or a spacing is not finite and positive, or beyond vr_volume_gamma's range in micrometres";
        return VR_ERR_INVALID_ARG;
    }
    d.sub = options.sub;
    d.mode = options.mode;
    d.dose_tolerance = doseTolerance;
    d.cutoff = options.cutoff;
    d.roi_slot = options.roiSlot;
    d.roi_contour = options.roiContour;
    d.skip_value = options.skipValue;
    rc = vr_volume_gamma(p_Ctx, &d, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::Gamma(int refSlot, int refChannel, int evalSlot, int evalChannel, int dstSlot, int dstChannel, float doseTolerance, double dtaMm,
                       const VolumeFileDcm& grid, const GammaOptions& options, vr_gamma_result* out)
{
    const DicomVolumeParams p = grid.GetVolumeParams();
    const double spacing[3] = {p.PixelSpacing[0], p.PixelSpacing[1], p.SliceThickness};
    return Gamma(refSlot, refChannel, evalSlot, evalChannel, dstSlot, dstChannel, doseTolerance, dtaMm, spacing, options, out);
}

int Application::Pick(uint32_t x, uint32_t y, vr_pick_result* out)
{
    if (!p_Ctx || !p_App) return VR_ERR_NOT_READY;
    int rc = vr_pick(p_Ctx, p_App->Variant(), x, y, out);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::SetSurfaceThreshold(float tau)
{
    if (!p_Ctx) return VR_ERR_HIP;
    int rc = vr_set_surface_threshold(p_Ctx, tau);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

int Application::ReadFrame(float* frag_rgba, uint8_t* present_bgra8, uint64_t* samples)
{
    int rc = vr_download(p_Ctx, frag_rgba, present_bgra8, samples);
    if (rc != VR_OK) m_Error = vr_last_error(p_Ctx);
    return rc;
}

}  // namespace med
