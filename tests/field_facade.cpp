// Test program for the C++ facade's distance-field queries: builds the three grid flavours of an OBJ file, takes distanceField() of each and
// writes, per flavour, sample()'s values (f32) and gradients (3 f32) of the points, then sphereTrace()'s t (f32) and status (u8) of the rays.
// usage: field_facade <obj> <voxel size> <points: raw f32 x y z> <rays: raw 6 f32> <radius> <out>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "VoxelBuilder.hpp"

static std::vector<float> read_floats(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> v(raw.size() / sizeof(float));
    std::memcpy(v.data(), raw.data(), v.size() * sizeof(float));
    return v;
}

template <class V> static void put(std::ofstream& f, const V& v) { f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(v[0]))); }

template <class T>
static void write_queries(const std::string& path, float vs, const std::vector<float>& pts, const std::vector<float>& rays, float radius, std::ofstream& f)
{
    VoxelBuilder<T> vb{std::filesystem::path(path)};
    const DistanceField field = vb.buildVoxelGrid(vs).distanceField();  // (the grid is gone when the queries run)
    std::vector<float> values, gradients, t;
    std::vector<uint8_t> status;
    field.sample(pts, values, &gradients);
    std::vector<float> again;
    field.sample(pts, again);
    if (again.size() != values.size() || (!values.empty() && std::memcmp(again.data(), values.data(), values.size() * sizeof(float))))
        throw std::runtime_error("sample without gradients differs");
    field.sphereTrace(rays, radius, 0.001f, 10000.0f, t, status);
    put(f, values); put(f, gradients); put(f, t); put(f, status);
}

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]), radius = std::stof(argv[5]);
    try {
        const std::vector<float> pts = read_floats(argv[3]), rays = read_floats(argv[4]);
        std::ofstream f(argv[6], std::ios::binary);
        write_queries<VoxelGridBool>(path, vs, pts, rays, radius, f);
        write_queries<VoxelGridAABBstruct>(path, vs, pts, rays, radius, f);
        write_queries<VoxelGridVec>(path, vs, pts, rays, radius, f);
        return f ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
