// VoxelBuilder.hpp -- VoxelBuilder<T, inParaell> with the reference's interface (src/VoxelBuilder.hpp:24-42,338),
// running on an MI355X through libvoxhip.so.
//
//   VoxelBuilder<VoxelGridBool> b{path};          // parses the OBJ (VoxelBuilder.hpp:51-70)
//   VoxelGridBool g = b.buildVoxelGrid(0.1f);     // bbox, dims, SAT voxelization -- HIP kernels
//   std::vector<Aabb> a = g.getAabbs();
//
// inParaell selects which of the reference's two SAT routines is reproduced: false = triBoxOverlap (serial driver,
// :118-162), true = triBoxOverlapSchwarzSeidel (std::thread driver, :226-335).  Both run data-parallel on the GPU; the
// reference's stdout lines are kept.
#pragma once
#include <voxhip.h>

#include <charconv>
#include <concepts>
#include <cstdio>
#include <filesystem>
#include <string>
#include <type_traits>
#include <vector>

#include "voxelgrid.hpp"
#include "voxelgridAABBstruct.hpp"
#include "voxelgridBool.hpp"
#include "voxelgridVecEncoding.hpp"

template <typename Derived>
concept DerivedFromVoxelGrid = requires {
    typename Derived::VoxelType;
    requires std::is_base_of_v<VoxelGrid<typename Derived::VoxelType>, Derived>;
};

namespace vxdetail {
// std::format("{}", float): shortest representation that round-trips
inline std::string fmt(float v)
{
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), v);
    return std::string(buf, r.ptr);
}
template <class T> constexpr vx_grid_kind kind_of()
{
    if constexpr (std::is_same_v<T, VoxelGridBool>) return VX_GRID_BOOL;
    else if constexpr (std::is_same_v<T, VoxelGridAABBstruct>) return VX_GRID_AABBSTRUCT;
    else return VX_GRID_VEC;
}
struct MeshDeleter {
    void operator()(vx_mesh* m) const noexcept { vx_mesh_free(m); }
};
inline bool& quiet() { static bool q = false; return q; }
}  // namespace vxdetail

template <DerivedFromVoxelGrid T, bool inParaell = false>
class VoxelBuilder final
{
public:
    explicit VoxelBuilder(const std::filesystem::path& path) { readObjFile(path); }
    VoxelBuilder() = default;

    // de-facto extension for callers that already hold arrays (the post-parse boundary of the hot path)
    VoxelBuilder(const float* xyz, size_t numVertices, const int* triIndices, size_t numTriangles)
    {
        vx_mesh* m = nullptr;
        vxdetail::check(vx_mesh_from_arrays(xyz, numVertices, triIndices, numTriangles, &m));
        m_mesh.reset(m, vxdetail::MeshDeleter{});
    }

    // Switches on the material plumbing the reference keeps commented out (VoxelBuilder.hpp:375-395, voxelgridBool.cpp:64):
    // buildVoxelGrid then also fills the grid's getMatrials() / getMatIdx() from the OBJ's usemtl / mtllib.  Off by default, like
    // the reference today (every voxel MaterialObj{}, nothing recorded).
    VoxelBuilder& withMaterials(bool on = true) { m_materials = on; return *this; }

    // Solid voxelization (VX_VOXELIZE_SOLID): after the triangle loop every enclosed empty cell -- one that no path of 6-connected empty
    // cells joins to the grid's boundary -- is set as well (setVoxel with MaterialObj{}, ascending).  Off by default: the reference marks
    // the surface only.  A single-device build; with withDevices of more than one device buildVoxelGrid throws std::invalid_argument.
    VoxelBuilder& withSolid(bool on = true) { m_solid = on; return *this; }

    // Spreads buildVoxelGrid over several GPUs of this process (vx_voxelize_multi: word shards of the one grid, peer copies over
    // xGMI; the grid returned lives on the first device).  Empty = the current device only.  VoxelGridBool / VoxelGridAABBstruct.
    VoxelBuilder& withDevices(std::vector<int> devices) { m_devices = std::move(devices); return *this; }

private:
    std::shared_ptr<vx_mesh> m_mesh;
    bool m_materials = false;
    bool m_solid = false;
    std::vector<int> m_devices;

    void readObjFile(const std::filesystem::path& path)
    {
        if (!std::filesystem::exists(path)) { throw std::invalid_argument("Path does not exist!"); }  // VoxelBuilder.hpp:54-56
        vx_mesh* m = nullptr;
        vxdetail::check(vx_mesh_load_obj(path.string().c_str(), &m));  // VX_ERR_PARSE -> runtime_error("Colud not get valid reader! ...")
        m_mesh.reset(m, vxdetail::MeshDeleter{});
    }

public:
    T buildVoxelGrid(float voxelSize)
    {
        if (!m_mesh) {  // default-constructed builder: an empty attrib (the reference would produce inf bounds; we refuse)
            throw std::runtime_error("VoxelBuilder has no mesh");
        }
        vx_voxelize_opts opts{};
        opts.sat_variant = inParaell ? 1 : 0;
        opts.flags = (m_materials ? VX_VOXELIZE_MATERIALS : 0) | (m_solid ? VX_VOXELIZE_SOLID : 0);
        vx_grid* g = nullptr;
        if (m_devices.size() > 1) {
            // word shards on the listed devices, peer copies to the first; with materials the shards' first uses are combined and
            // the ids gathered in shard order (vx_multi_voxelize).  The grid handed back is the first device's.
            vx_multi* mc = nullptr;
            vxdetail::check(vx_multi_create(m_mesh.get(), m_devices.data(), (int)m_devices.size(), vxdetail::kind_of<T>(), &mc));
            const vx_status st = vx_multi_voxelize(mc, voxelSize, &opts, 0);
            if (st != VX_OK) {
                const std::string err = vx_last_error();
                vx_multi_free(mc);
                if (st == VX_ERR_INVALID_ARG) throw std::invalid_argument(err);
                throw std::runtime_error(err);
            }
            g = vx_multi_release_grid(mc, 0);
            vx_multi_free(mc);
        } else
            vxdetail::check(vx_voxelize(m_mesh.get(), voxelSize, vxdetail::kind_of<T>(), &opts, &g));
        vxdetail::GridHandle h = vxdetail::adopt(g);
        vx_grid_desc d;
        vxdetail::check(vx_grid_describe(g, &d));
        if (!vxdetail::quiet()) {
            using vxdetail::fmt;
            // VoxelBuilder.hpp:343-352, :417 (:464 for the threaded variant)
            std::printf("Bounding box: min(%s,%s,%s):\n", fmt(d.bbox_min[0]).c_str(), fmt(d.bbox_min[1]).c_str(), fmt(d.bbox_min[2]).c_str());
            std::printf("Bounding box: max(%s,%s,%s):\n", fmt(d.bbox_max[0]).c_str(), fmt(d.bbox_max[1]).c_str(), fmt(d.bbox_max[2]).c_str());
            std::printf("Bounding box: center(%s,%s,%s):\n", fmt(d.bbox_center[0]).c_str(), fmt(d.bbox_center[1]).c_str(),
                        fmt(d.bbox_center[2]).c_str());
            std::printf("Grid dimensions: %zux%zux%zu\n", (size_t)d.dim[0], (size_t)d.dim[1], (size_t)d.dim[2]);
            std::printf("Voxel size: %s\n", fmt(voxelSize).c_str());
            if constexpr (inParaell) {
                if (d.triangles == 0) std::printf("No triangles in OBJ, nothing to voxelize.\n");
                else std::printf("Using MI355X (device %d) for voxelization over %zu triangles.\n", d.device, (size_t)d.triangles);
            }
            if (!(inParaell && d.triangles == 0)) std::printf("Total triangles processed: %zu\n", (size_t)d.triangles);
        }
        return T(std::move(h), d);
    }
};
