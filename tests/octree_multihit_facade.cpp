// Test program for the C++ facade's multi-hit query on the octree: builds the Octree of an OBJ file, traces the rays of a binary file
// (6 float32 each) with Octree::traceMulti and writes t, prim and count to the output file.
//   usage: octree_multihit_facade <obj> <voxel size> <rays.bin> <out> <max hits> <tmin> <tmax>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "octTree.hpp"

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]);
    const uint32_t k = (uint32_t)std::atoi(argv[5]);
    const float tmin = std::stof(argv[6]), tmax = std::stof(argv[7]);
    try {
        std::ifstream in(argv[3], std::ios::binary);
        const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::vector<float> rays(raw.size() / sizeof(float));
        std::memcpy(rays.data(), raw.data(), rays.size() * sizeof(float));
        Octree tree{std::filesystem::path(path), vs};
        std::vector<float> t;
        std::vector<uint32_t> prim, count;
        tree.traceMulti(rays, k, tmin, tmax, t, prim, count);
        std::ofstream f(argv[4], std::ios::binary);
        f.write(reinterpret_cast<const char*>(t.data()), (std::streamsize)(t.size() * sizeof(float)));
        f.write(reinterpret_cast<const char*>(prim.data()), (std::streamsize)(prim.size() * sizeof(uint32_t)));
        f.write(reinterpret_cast<const char*>(count.data()), (std::streamsize)(count.size() * sizeof(uint32_t)));
        std::printf("%zu rays, %zu slots, %zu items\n", count.size(), t.size(), tree.getAabbs().size());
        return f ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
