// vxref: the reference's own voxelizer (VoxelBuilder.hpp, voxelgrid*.{hpp,cpp}, octTree.hpp), compiled unmodified from
// its checkout against the three stand-in headers in shim/, and driven from the command line so that tests can compare
// the CPU oracle (oracle/vx_oracle.c) with it.  Test infrastructure only; built by oracle/ref/Makefile.
//
//   vxref <obj> <voxelsize> <mode> <out>
//     mode: bool | aabbstruct | vec            VoxelBuilder<T, false> (serial driver, triBoxOverlap)
//           bool_par | aabbstruct_par | vec_par VoxelBuilder<T, true>  (std::thread driver, triBoxOverlapSchwarzSeidel)
//           octree[:maxItemsPerLeaf]            Octree(path, voxelsize, maxItemsPerLeaf) (default 16)
//   writes  <out>.aabbs  getAabbs() as raw 24-byte boxes (min xyz, max xyz; float32)
//           <out>.occ    grids only: occupancy read through the public getVoxel (uint32 words, voxel i -> bit i % 32 of
//                        word i / 32, i = x + W * (y + H * z)); empty when the grid has no cells
//           <out>.json   {"mode", "num_aabbs", "memory_bytes" (getMemoryUsageBytes()), "dims"}
// The reference's own stdout passes through unchanged.
#include "VoxelBuilder.hpp"
#include "octTree.hpp"
#include "voxelgridAABBstruct.hpp"
#include "voxelgridBool.hpp"
#include "voxelgridVecEncoding.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

namespace {

void write_file(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || (bytes && std::fwrite(data, 1, bytes, f) != bytes) || std::fclose(f) != 0) {
        throw std::runtime_error("cannot write " + path);
    }
}

void write_info(const std::string& out, const std::string& mode, size_t naabbs, size_t mem, const size_t* dims)
{
    std::string s = "{\"mode\": \"" + mode + "\", \"num_aabbs\": " + std::to_string(naabbs) + ", \"memory_bytes\": " + std::to_string(mem) +
                    ", \"dims\": ";
    s += dims ? "[" + std::to_string(dims[0]) + ", " + std::to_string(dims[1]) + ", " + std::to_string(dims[2]) + "]" : std::string("null");
    s += "}\n";
    write_file(out + ".json", s.data(), s.size());
}

template <typename G>
bool in_grid(const G& g, size_t x, size_t y, size_t z)
{
    try {
        (void)g.getCorrds(x, y, z);  // throws "Index out of bounds" outside [0, m_x) x [0, m_y) x [0, m_z)
        return true;
    } catch (const std::runtime_error&) {
        return false;
    }
}

// The grid's dimensions through its public interface: the first index on each axis at which getCorrds throws.
// false when the grid has no cells (some dimension is 0: every index throws).
template <typename G>
bool grid_dims(const G& g, size_t dims[3])
{
    if (!in_grid(g, 0, 0, 0)) return false;
    for (int a = 0; a < 3; ++a) {
        auto inside = [&](size_t k) { return in_grid(g, a == 0 ? k : 0, a == 1 ? k : 0, a == 2 ? k : 0); };
        size_t lo = 0, hi = 1;  // inside(lo), hi: first probe
        while (inside(hi)) {
            lo = hi;
            hi *= 2;
        }
        while (hi - lo > 1) {  // inside(lo) && !inside(hi)
            const size_t mid = lo + (hi - lo) / 2;
            (inside(mid) ? lo : hi) = mid;
        }
        dims[a] = hi;
    }
    return true;
}

template <typename T, bool Par>
void run_grid(const std::string& obj, float vs, const std::string& mode, const std::string& out)
{
    VoxelBuilder<T, Par> builder(obj);
    const T grid = builder.buildVoxelGrid(vs);
    const std::vector<Aabb> aabbs = grid.getAabbs();
    write_file(out + ".aabbs", aabbs.data(), aabbs.size() * sizeof(Aabb));

    size_t dims[3] = {0, 0, 0};
    const bool has_cells = grid_dims(grid, dims);
    std::vector<std::uint32_t> words;
    if (has_cells) {
        const size_t n = dims[0] * dims[1] * dims[2];
        words.assign((n + 31) / 32, 0u);
        if constexpr (std::is_same_v<T, VoxelGridBool>) {
            // VoxelGridBool::getVoxel(x, y, z) returns m_voxel[map3dto1d(x, y, z)] (voxelgrid.hpp): the bitmask WORD at that
            // linear index.  Word i is therefore read at the cell whose linear index is i (i < ceil(n / 32) <= n).
            for (size_t i = 0; i < words.size(); ++i) {
                words[i] = grid.getVoxel(i % dims[0], (i / dims[0]) % dims[1], i / (dims[0] * dims[1]));
            }
        } else if constexpr (std::is_same_v<T, VoxelGridAABBstruct>) {
            for (size_t z = 0, i = 0; z < dims[2]; ++z)
                for (size_t y = 0; y < dims[1]; ++y)
                    for (size_t x = 0; x < dims[0]; ++x, ++i)
                        if (grid.getVoxel(x, y, z).isUsed) words[i / 32] |= 1u << (i % 32);
        }
        // VoxelGridVec keeps the hit list in m_voxel, so its getVoxel(x, y, z) indexes that list: no occupancy to read
    }
    if (!std::is_same_v<T, VoxelGridVec>) write_file(out + ".occ", words.data(), words.size() * 4);
    write_info(out, mode, aabbs.size(), grid.getMemoryUsageBytes(), has_cells ? dims : nullptr);
}

void run_octree(const std::string& obj, float vs, size_t max_items, const std::string& mode, const std::string& out)
{
    const Octree oc(obj, vs, max_items);
    const std::vector<Aabb> aabbs = oc.getAabbs();
    write_file(out + ".aabbs", aabbs.data(), aabbs.size() * sizeof(Aabb));
    write_info(out, mode, aabbs.size(), oc.getMemoryUsageBytes(), nullptr);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: vxref <obj> <voxelsize> <bool|aabbstruct|vec>[_par]|octree[:maxItemsPerLeaf] <out>\n");
        return 2;
    }
    const std::string obj = argv[1], mode = argv[3], out = argv[4];
    const float vs = std::strtof(argv[2], nullptr);
    try {
        if (mode == "bool") run_grid<VoxelGridBool, false>(obj, vs, mode, out);
        else if (mode == "bool_par") run_grid<VoxelGridBool, true>(obj, vs, mode, out);
        else if (mode == "aabbstruct") run_grid<VoxelGridAABBstruct, false>(obj, vs, mode, out);
        else if (mode == "aabbstruct_par") run_grid<VoxelGridAABBstruct, true>(obj, vs, mode, out);
        else if (mode == "vec") run_grid<VoxelGridVec, false>(obj, vs, mode, out);
        else if (mode == "vec_par") run_grid<VoxelGridVec, true>(obj, vs, mode, out);
        else if (mode.rfind("octree", 0) == 0) {
            const size_t max_items = mode.size() > 7 && mode[6] == ':' ? std::strtoull(mode.c_str() + 7, nullptr, 10) : 16;
            run_octree(obj, vs, max_items, mode, out);
        } else {
            std::fprintf(stderr, "vxref: unknown mode %s\n", mode.c_str());
            return 2;
        }
    } catch (const std::exception& e) {
        std::fflush(stdout);
        std::fprintf(stderr, "vxref: %s\n", e.what());
        return 1;
    }
    std::fflush(stdout);
    return 0;
}
