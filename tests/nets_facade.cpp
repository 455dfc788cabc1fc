// Test program for the C++ facade's surface nets: builds the three grid flavours of an OBJ file and prints for each a line `nets V T checksum`
// (FNV-1a, 64 bits) over the bytes of smoothSurface's positions, triangles and normals.
//   usage: nets_facade <obj> <voxel size> <iterations> <lambda> <mu>
#include <cstdio>
#include <cstring>
#include <string>

#include "VoxelBuilder.hpp"

static uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

template <class T>
static void run(const std::string& path, float vs, const vx_smooth& sp)
{
    VoxelBuilder<T> vb{std::filesystem::path(path)};
    const T g = vb.buildVoxelGrid(vs);
    std::vector<float> xyz, normals;
    std::vector<int32_t> tris;
    g.smoothSurface(sp, xyz, tris, nullptr, &normals);
    uint64_t h = 14695981039346656037ull;
    h = fnv(h, xyz.data(), xyz.size() * 4);
    h = fnv(h, tris.data(), tris.size() * 4);
    h = fnv(h, normals.data(), normals.size() * 4);
    std::printf("nets %zu %zu %016llx\n", xyz.size() / 3, tris.size() / 3, (unsigned long long)h);
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]);
    const vx_smooth sp{(uint32_t)std::atoi(argv[3]), std::stof(argv[4]), std::stof(argv[5])};
    try {
        run<VoxelGridBool>(path, vs, sp);
        run<VoxelGridAABBstruct>(path, vs, sp);
        run<VoxelGridVec>(path, vs, sp);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
