// SurfaceMesh -- an indexed triangle mesh on the host: what Application::ExtractSurface returns (vr_volume_mesh of include/vr.h, its
// positions scaled by a voxel spacing), and its two file forms.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "vr.h"

namespace med {

struct SurfaceMesh {
    std::vector<double> positions;    // x y z per vertex: voxel index * spacing, in double
    std::vector<uint32_t> triangles;  // three vertex numbers per triangle, counter-clockwise seen from outside
    vr_mesh_result result{};          // what the extraction reported

    size_t VertexCount() const { return positions.size() / 3; }
    size_t TriangleCount() const { return triangles.size() / 3; }
    // Binary STL: 80 bytes of header, the triangle count, then per triangle its unit normal (from the triangle; zeros for one without
    // area), its three corners as float32 and two zero bytes.  false if the file cannot be written.
    bool WriteStl(const std::string& path) const;
    // Binary little-endian PLY, indexed: float x y z per vertex, then per face a uchar 3 and three uint vertex_indices.
    bool WritePly(const std::string& path) const;
};

}  // namespace med
