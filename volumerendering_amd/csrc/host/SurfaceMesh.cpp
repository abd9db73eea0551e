#include "SurfaceMesh.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace med {

namespace {

struct File {
    std::FILE* f;
    explicit File(const std::string& path) : f(std::fopen(path.c_str(), "wb")) {}
    ~File() { if (f) std::fclose(f); }
    bool put(const void* p, size_t n) { return f && std::fwrite(p, 1, n, f) == n; }
    bool close()
    {
        const bool ok = f && std::fclose(f) == 0;
        f = nullptr;
        return ok;
    }
};

}  // namespace

bool SurfaceMesh::WriteStl(const std::string& path) const
{
    File out(path);
    char header[80] = {};
    std::snprintf(header, sizeof header, "binary STL: marching tetrahedra, %zu triangles", TriangleCount());
    const uint32_t n = static_cast<uint32_t>(TriangleCount());
    if (!out.put(header, sizeof header) || !out.put(&n, 4)) return false;
    std::vector<unsigned char> rec((size_t)n * 50);
    for (size_t t = 0; t < n; ++t) {
        const double* p[3];
        for (int k = 0; k < 3; ++k) p[k] = &positions[(size_t)triangles[t * 3 + k] * 3];
        const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        double nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double len = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        float f[12];
        for (int a = 0; a < 3; ++a) f[a] = len > 0.0 ? static_cast<float>(nrm[a] / len) : 0.0f;
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) f[3 + k * 3 + a] = static_cast<float>(p[k][a]);
        std::memcpy(&rec[t * 50], f, 48);  // (the attribute byte count stays zero)
    }
    return out.put(rec.data(), rec.size()) && out.close();
}

bool SurfaceMesh::WritePly(const std::string& path) const
{
    File out(path);
    char header[256];
    const int len = std::snprintf(header, sizeof header,
                                  "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                                  "element face %zu\nproperty list uchar uint vertex_indices\nend_header\n",
                                  VertexCount(), TriangleCount());
    if (len <= 0 || !out.put(header, (size_t)len)) return false;
    std::vector<float> v(positions.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = static_cast<float>(positions[i]);
    std::vector<unsigned char> faces(TriangleCount() * 13);
    for (size_t t = 0; t < TriangleCount(); ++t) {
        faces[t * 13] = 3;
        std::memcpy(&faces[t * 13 + 1], &triangles[t * 3], 12);
    }
    return out.put(v.data(), v.size() * sizeof(float)) && out.put(faces.data(), faces.size()) && out.close();
}

}  // namespace med
