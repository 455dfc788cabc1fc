// Test program for the C++ facade's connected components: builds the three grid flavours of an OBJ file, surface or solid, and writes for
// each K (u32), components(connectivity) (u32 per cell) and componentStats(connectivity) (32 B per component) to the output file.
//   usage: components_facade <obj> <voxel size> <out> <6|26> [solid]
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "VoxelBuilder.hpp"

template <class T>
static void write_components(const std::string& path, float vs, int connectivity, bool solid, std::ofstream& f)
{
    VoxelBuilder<T> vb{std::filesystem::path(path)};
    vb.withSolid(solid);
    const T g = vb.buildVoxelGrid(vs);
    std::vector<uint32_t> labels;
    const uint32_t k = g.components(connectivity, labels);
    const std::vector<vx_component> s = g.componentStats(connectivity);
    f.write(reinterpret_cast<const char*>(&k), sizeof(k));
    f.write(reinterpret_cast<const char*>(labels.data()), (std::streamsize)(labels.size() * sizeof(uint32_t)));
    f.write(reinterpret_cast<const char*>(s.data()), (std::streamsize)(s.size() * sizeof(vx_component)));
    std::printf("%zu %zu %zu %u\n", g.dimX(), g.dimY(), g.dimZ(), k);
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]);
    const int connectivity = std::atoi(argv[4]);
    const bool solid = argc > 5 && !std::strcmp(argv[5], "solid");
    try {
        std::ofstream f(argv[3], std::ios::binary);
        write_components<VoxelGridBool>(path, vs, connectivity, solid, f);
        write_components<VoxelGridAABBstruct>(path, vs, connectivity, solid, f);
        write_components<VoxelGridVec>(path, vs, connectivity, solid, f);
        return f ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
