// Test program for the C++ facade's morphology: builds the three grid flavours of an OBJ file and prints, per flavour, the occupied counts of
// the grid and of dilated / eroded / opened / closed / sealed (r2), each result being a grid of the same class.
// usage: morph_facade <obj> <voxel size> <r2>
#include <cstdio>
#include <string>
#include <type_traits>

#include "VoxelBuilder.hpp"

template <class T>
static unsigned long long occupied(const T& g)
{
    vx_grid_desc d;
    vxdetail::check(vx_grid_describe(g.handle(), &d));
    return (unsigned long long)d.occupied;
}

template <class T>
static void run(const char* name, const std::string& path, float vs, uint32_t r2)
{
    VoxelBuilder<T> vb{std::filesystem::path(path)};
    const T g = vb.buildVoxelGrid(vs);
    static_assert(std::is_same_v<decltype(g.dilated(r2)), T> && std::is_same_v<decltype(g.sealed(r2)), T>, "a grid of the same class");
    const T d = g.dilated(r2), e = g.eroded(r2), o = g.opened(r2), c = g.closed(r2), s = g.sealed(r2);
    std::printf("%s %llu %llu %llu %llu %llu %llu %zu\n", name, occupied(g), occupied(d), occupied(e), occupied(o), occupied(c), occupied(s), s.getAabbs().size());
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const std::string path = argv[1];
    const float vs = std::stof(argv[2]);
    const uint32_t r2 = (uint32_t)std::stoul(argv[3]);
    try {
        run<VoxelGridBool>("bool", path, vs, r2);
        run<VoxelGridAABBstruct>("aabbstruct", path, vs, r2);
        run<VoxelGridVec>("vec", path, vs, r2);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
