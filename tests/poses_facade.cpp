// Test program for the C++ facade's pose queries: builds the three grid flavours of an OBJ file, takes distanceField() of each and writes,
// per flavour, poses()'s clearance (f32), point (u32), count (u32), position (3 f32) and gradient (3 f32) of every pose.
// usage: poses_facade <obj> <voxel size> <points: raw f32 x y z> <radii: raw f32, may be empty> <transforms: raw 12 f32> <margin> <out>
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
static void write_queries(const std::string& path, float vs, const std::vector<float>& pts, const std::vector<float>& radii, const std::vector<float>& xf,
                          float margin, std::ofstream& f)
{
    VoxelBuilder<T> vb{std::filesystem::path(path)};
    const DistanceField field = vb.buildVoxelGrid(vs).distanceField();  // (the grid is gone when the queries run)
    std::vector<float> clearance, position, gradient, again;
    std::vector<uint32_t> point, count, point2, count2;
    field.poses(pts, radii, xf, margin, clearance, point, count, &position, &gradient);
    field.poses(pts, radii, xf, margin, again, point2, count2);
    if (again.size() != clearance.size() || (!again.empty() && std::memcmp(again.data(), clearance.data(), again.size() * sizeof(float))) || point2 != point ||
        count2 != count)
        throw std::runtime_error("poses without position and gradient differs");
    put(f, clearance); put(f, point); put(f, count); put(f, position); put(f, gradient);
}

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]), margin = std::stof(argv[6]);
    try {
        const std::vector<float> pts = read_floats(argv[3]), radii = read_floats(argv[4]), xf = read_floats(argv[5]);
        std::ofstream f(argv[7], std::ios::binary);
        write_queries<VoxelGridBool>(path, vs, pts, radii, xf, margin, f);
        write_queries<VoxelGridAABBstruct>(path, vs, pts, radii, xf, margin, f);
        write_queries<VoxelGridVec>(path, vs, pts, radii, xf, margin, f);
        return f ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
