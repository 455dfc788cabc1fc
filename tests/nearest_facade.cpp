// Test program for the C++ facade's feature transform: builds the three grid flavours of an OBJ file, surface or solid, and writes for each
// nearestCells() (u32), nearestCells(true) (u32), then nearestLabels(6) (u32) and its K as one more u32 to the output file.
//   usage: nearest_facade <obj> <voxel size> <out> [solid]
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
    const std::vector<uint32_t> a = g.nearestCells();
    const std::vector<uint32_t> b = g.nearestCells(true);
    std::vector<uint32_t> lab;
    const uint32_t k = g.nearestLabels(6, lab);
    f.write(reinterpret_cast<const char*>(a.data()), (std::streamsize)(a.size() * sizeof(uint32_t)));
    f.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)(b.size() * sizeof(uint32_t)));
    f.write(reinterpret_cast<const char*>(lab.data()), (std::streamsize)(lab.size() * sizeof(uint32_t)));
    f.write(reinterpret_cast<const char*>(&k), sizeof(k));
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
