// Test program for the C++ facade's distance fields: builds the three grid flavours of an OBJ file, surface or solid, and writes for each
// signedDistances() (f32) then squaredDistances(true) (u32) to the output file.   usage: distance_facade <obj> <voxel size> <out> [solid]
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "VoxelBuilder.hpp"

template <class T>
static void write_fields(const std::string& path, float vs, bool solid, std::ofstream& f)
{
    VoxelBuilder<T> vb{std::filesystem::path(path)};
    vb.withSolid(solid);
    const T g = vb.buildVoxelGrid(vs);
    const std::vector<float> s = g.signedDistances();
    const std::vector<uint32_t> d = g.squaredDistances(true);
    f.write(reinterpret_cast<const char*>(s.data()), (std::streamsize)(s.size() * sizeof(float)));
    f.write(reinterpret_cast<const char*>(d.data()), (std::streamsize)(d.size() * sizeof(uint32_t)));
    std::printf("%zu %zu %zu\n", g.dimX(), g.dimY(), g.dimZ());
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]);
    const bool solid = argc > 4 && !std::strcmp(argv[4], "solid");
    try {
        std::ofstream f(argv[3], std::ios::binary);
        write_fields<VoxelGridBool>(path, vs, solid, f);
        write_fields<VoxelGridAABBstruct>(path, vs, solid, f);
        write_fields<VoxelGridVec>(path, vs, solid, f);
        return f ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
