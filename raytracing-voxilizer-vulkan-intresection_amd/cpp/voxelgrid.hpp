// voxelgrid.hpp -- VoxelGrid<T> with the reference's interface (src/voxelgrid.hpp:15-128), backed by a vx_grid handle
// of libvoxhip.so: the voxels live in HBM, not in std::vector members.
//
// Differences a caller can observe, all deliberate:
//   * no dense host allocations: the reference allocates m_matIdx = X*Y*Z int16 (voxelgrid.hpp:59; 2 B/voxel, never read
//     on this path) and, per subclass, m_voxel.  getMatIdx()/getMatrials() behave as in the reference (nothing is ever
//     added on this path because the material code is commented out upstream); addMatrialIfNeeded() keeps a sparse map.
//   * grids are cheap to copy (shared handle); like the reference they are not assignable.
//   * errors from the device library surface as the reference's exception types and messages.
#pragma once
#include <voxhip.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "obj_loader.h"
#include "shaders/host_device.h"

namespace vxdetail {
[[noreturn]] inline void throw_status(vx_status s)
{
    const std::string msg = vx_last_error();
    switch (s) {
        case VX_ERR_PATH: throw std::invalid_argument("Path does not exist!");          // VoxelBuilder.hpp:55
        case VX_ERR_OUT_OF_BOUNDS: throw std::runtime_error("Index out of bounds");     // voxelgrid.hpp:69
        case VX_ERR_INVALID_ARG: throw std::invalid_argument(msg);
        default: throw std::runtime_error(msg);                                         // incl. "Colud not get valid reader! ..."
    }
}
inline void check(vx_status s)
{
    if (s != VX_OK) throw_status(s);
}
struct GridDeleter {
    void operator()(vx_grid* g) const noexcept { vx_grid_free(g); }
};
using GridHandle = std::shared_ptr<vx_grid>;
inline GridHandle adopt(vx_grid* g) { return GridHandle(g, GridDeleter{}); }
}  // namespace vxdetail

// A snapshot of a grid's signed distance field that stays on the device (vx_field), queried at the caller's own points.  It does not
// depend on the grid it was taken from.
class DistanceField
{
    std::shared_ptr<vx_field> m_field;

public:
    explicit DistanceField(const vx_grid* grid)
    {
        vx_field* f = nullptr;
        vxdetail::check(vx_field_create(grid, nullptr, &f));
        m_field = std::shared_ptr<vx_field>(f, [](vx_field* p) noexcept { vx_field_free(p); });
    }
    vx_field* handle() const noexcept { return m_field.get(); }

    // Trilinear sample at points (x y z each): one value per point, and its gradient (3 per point) where asked for.
    void sample(const std::vector<float>& points, std::vector<float>& values, std::vector<float>* gradients = nullptr) const
    {
        const size_t n = points.size() / 3;
        values.assign(n, 0.0f);
        if (gradients) gradients->assign(3 * n, 0.0f);
        vx_field_sample_args a{};
        a.points = points.data(); a.num_points = n;
        a.value = values.data(); a.gradient = gradients ? gradients->data() : nullptr;
        vxdetail::check(vx_field_sample(m_field.get(), &a));
    }

    // Sphere cast: a sphere of `radius` (world units) along rays (origin, direction: 6 floats each) -> t (-1: no hit) and
    // VX_FIELD_MISS / VX_FIELD_HIT / VX_FIELD_STEP_LIMIT per ray, with the default step scale, hit tolerance and step limit.
    void sphereTrace(const std::vector<float>& rays, float radius, float tmin, float tmax, std::vector<float>& t, std::vector<uint8_t>& status) const
    {
        const size_t n = rays.size() / 6;
        t.assign(n, -1.0f);
        status.assign(n, (uint8_t)VX_FIELD_MISS);
        vx_field_trace_args a{};
        a.rays = rays.data(); a.num_rays = n;
        a.tmin = tmin; a.tmax = tmax; a.radius = radius;
        a.t = t.data(); a.status = status.data();
        vxdetail::check(vx_field_sphere_trace(m_field.get(), &a));
    }

    // Pose query: a body of points (x y z each) with radii (world units; empty: all 0) under transforms (body to world, row-major 3 x 4,
    // 12 floats each) -> per pose the smallest value - radius over the body, the point that has it (0xFFFFFFFF: none) and the number of
    // points with value - radius <= margin; where asked for, the contact position and the gradient there (3 per pose each).
    void poses(const std::vector<float>& points, const std::vector<float>& radii, const std::vector<float>& transforms, float margin,
               std::vector<float>& clearance, std::vector<uint32_t>& point, std::vector<uint32_t>& count, std::vector<float>* position = nullptr,
               std::vector<float>* gradient = nullptr) const
    {
        const size_t np = points.size() / 3, n = transforms.size() / 12;
        if (!radii.empty() && radii.size() != np) throw std::invalid_argument("poses: one radius per point, or none");
        clearance.assign(n, 0.0f);
        point.assign(n, 0u);
        count.assign(n, 0u);
        if (position) position->assign(3 * n, 0.0f);
        if (gradient) gradient->assign(3 * n, 0.0f);
        vx_field_pose_args a{};
        a.points = np ? points.data() : nullptr; a.num_points = np;
        a.radii = radii.empty() ? nullptr : radii.data();
        a.transforms = n ? transforms.data() : nullptr; a.num_poses = n;
        a.margin = margin;
        a.clearance = clearance.data(); a.point = point.data(); a.count = count.data();
        a.position = position ? position->data() : nullptr; a.gradient = gradient ? gradient->data() : nullptr;
        if (n) vxdetail::check(vx_field_poses(m_field.get(), &a));
    }
};

template <typename T>
class VoxelGrid
{
protected:
    const size_t m_x;
    const size_t m_y;
    const size_t m_z;
    const vec3 m_org;
    const float m_voxelSize;
    const float m_voxelDiameter;

    std::vector<MaterialObj> m_materials;
    std::map<size_t, int16_t> m_matIdx;  // sparse stand-in for the reference's dense int16 array
    std::unordered_map<MaterialObj, int16_t> m_materialMap;
    vxdetail::GridHandle m_grid;

    constexpr size_t map3dto1d(size_t x, size_t y, size_t z) const noexcept { return x + m_x * (y + m_y * z); }

    // grid of a given flavour with the reference constructor's arguments (voxelgrid.hpp:52-62)
    VoxelGrid(vx_grid_kind kind, size_t x, size_t y, size_t z, float voxelSize, vec3 org)
        : m_x(x), m_y(y), m_z(z), m_org(org), m_voxelSize(voxelSize), m_voxelDiameter(std::hypot(voxelSize, voxelSize, voxelSize))
    {
        m_materials.reserve(16);
        const float o[3] = {org.x, org.y, org.z};
        vx_grid* g = nullptr;
        vxdetail::check(vx_grid_create(kind, x, y, z, voxelSize, o, nullptr, &g));
        m_grid = vxdetail::adopt(g);
    }

    // adopt a grid the device voxelizer produced (VoxelBuilder::buildVoxelGrid)
    VoxelGrid(vxdetail::GridHandle h, const vx_grid_desc& d)
        : m_x(d.dim[0]), m_y(d.dim[1]), m_z(d.dim[2]), m_org(d.origin[0], d.origin[1], d.origin[2]), m_voxelSize(d.voxel_size),
          m_voxelDiameter(std::hypot(d.voxel_size, d.voxel_size, d.voxel_size)), m_grid(std::move(h))
    {
        m_materials.reserve(16);
    }

    std::vector<Aabb> fetchAabbs() const
    {
        uint64_t n = 0;
        vxdetail::check(vx_grid_aabbs(m_grid.get(), nullptr, 0, &n));
        std::vector<Aabb> ret(n);
        if (n) vxdetail::check(vx_grid_aabbs(m_grid.get(), reinterpret_cast<vx_aabb*>(ret.data()), n, &n));
        return ret;
    }

public:
    virtual ~VoxelGrid() = default;

    // VoxelGrid::getVoxel (voxelgrid.hpp:66-72) returns m_voxel[map3dto1d(x,y,z)]; what that means per flavour is defined
    // by the subclasses (see their headers).
    T getVoxel(size_t x, size_t y, size_t z) const
    {
        if (x >= m_x || y >= m_y || z >= m_z) [[unlikely]] { throw std::runtime_error("Index out of bounds"); }
        return voxelAt(map3dto1d(x, y, z));
    }

    // correct occupancy query (the reference has none for the Bool grid)
    bool isOccupied(size_t x, size_t y, size_t z) const
    {
        int occ = 0;
        vxdetail::check(vx_grid_test_voxel(m_grid.get(), x, y, z, &occ));
        return occ != 0;
    }

    // voxelgrid.hpp:74-89.  A grid voxelized with materials (VoxelBuilder::withMaterials) answers from the device: the distinct
    // MaterialObj in first-use order and the ids >= 0 in index order (one per occupied voxel, last setVoxel call wins; VoxelGridVec:
    // one per call).  Otherwise, as in the reference today, only what addMatrialIfNeeded was called with by hand.
    std::vector<MaterialObj> getMatrials() const noexcept
    {
        uint64_t n = 0;
        if (vx_grid_materials(m_grid.get(), nullptr, 0, &n) == VX_OK && n) {
            std::vector<vx_material> raw(n);
            if (vx_grid_materials(m_grid.get(), raw.data(), n, &n) == VX_OK) {
                std::vector<MaterialObj> ret(n);
                for (uint64_t i = 0; i < n; ++i) {
                    const vx_material& r = raw[i];
                    MaterialObj& m = ret[i];
                    m.ambient = vec3(r.ambient[0], r.ambient[1], r.ambient[2]);
                    m.diffuse = vec3(r.diffuse[0], r.diffuse[1], r.diffuse[2]);
                    m.specular = vec3(r.specular[0], r.specular[1], r.specular[2]);
                    m.transmittance = vec3(r.transmittance[0], r.transmittance[1], r.transmittance[2]);
                    m.emission = vec3(r.emission[0], r.emission[1], r.emission[2]);
                    m.shininess = r.shininess; m.ior = r.ior; m.dissolve = r.dissolve; m.illum = r.illum; m.textureID = r.texture_id;
                }
                return ret;
            }
        }
        return m_materials;
    }

    std::vector<int16_t> getMatIdx() const noexcept
    {
        uint64_t n = 0;
        if (vx_grid_material_ids(m_grid.get(), nullptr, 0, &n) == VX_OK && n) {
            std::vector<int16_t> ret(n);
            if (vx_grid_material_ids(m_grid.get(), ret.data(), n, &n) == VX_OK) return ret;
        }
        std::vector<int16_t> ret;
        ret.reserve(m_materials.size());
        for (const auto& kv : m_matIdx)
            if (kv.second >= 0) ret.push_back(kv.second);
        return ret;
    }

    vec3 getCorrds(size_t x, size_t y, size_t z) const
    {
        float c[3];
        vxdetail::check(vx_grid_coords(m_grid.get(), x, y, z, c));  // throws "Index out of bounds" like voxelgrid.hpp:93-95
        return vec3(c[0], c[1], c[2]);
    }

    void addMatrialIfNeeded(size_t idx, const MaterialObj& material)
    {
        const auto it = m_materialMap.find(material);
        if (it != m_materialMap.end()) [[likely]] {
            m_matIdx[idx] = it->second;
        } else {
            const int newIndex = static_cast<int>(m_materials.size());
            m_materials.push_back(material);
            m_materialMap[material] = static_cast<int16_t>(newIndex);
            m_matIdx[idx] = static_cast<int16_t>(newIndex);
        }
    }

    size_t getMemoryUsageBytes() const noexcept { return static_cast<size_t>(vx_grid_bytes(m_grid.get())); }

    // device-side handle, for callers that keep going on the GPU (ray queries, multi-GPU exchange)
    vx_grid* handle() const noexcept { return m_grid.get(); }
    size_t dimX() const noexcept { return m_x; }
    size_t dimY() const noexcept { return m_y; }
    size_t dimZ() const noexcept { return m_z; }
    float voxelSize() const noexcept { return m_voxelSize; }
    vec3 origin() const noexcept { return m_org; }

    // Exact distance fields of the occupancy (vx_grid_distance_sq / vx_grid_sdf), one value per cell at x + X*(y + Y*z).
    // squaredDistances: squared distance in cells to the nearest occupied cell (inside: to the nearest empty one), 0xFFFFFFFF when there is none.
    // signedDistances: voxelSize() * sqrt of the outside distance off the occupied cells, minus that of the inside distance on them.
    std::vector<uint32_t> squaredDistances(bool inside = false) const
    {
        std::vector<uint32_t> ret(m_x * m_y * m_z);
        vxdetail::check(vx_grid_distance_sq(m_grid.get(), inside ? VX_DISTANCE_INSIDE : 0u, ret.data(), ret.size()));
        return ret;
    }
    std::vector<float> signedDistances() const
    {
        std::vector<float> ret(m_x * m_y * m_z);
        vxdetail::check(vx_grid_sdf(m_grid.get(), ret.data(), ret.size()));
        return ret;
    }

    // The signed field kept on the device for queries at arbitrary points: trilinear samples and sphere casts (DistanceField above).
    DistanceField distanceField() const { return DistanceField(m_grid.get()); }

    // The boundary mesh of the occupancy (vx_grid_surface): one quad (two triangles) per exposed cell face over de-duplicated lattice
    // points.  xyz: 3 floats per vertex; tris: 3 vertex indices per triangle; mats (optional; a grid built with materials, not VoxelGridVec):
    // one index into getMatrials() per triangle.
    void surface(std::vector<float>& xyz, std::vector<int32_t>& tris, std::vector<int32_t>* mats = nullptr) const
    {
        uint64_t nv = 0, nt = 0;
        int32_t probe = 0;
        vxdetail::check(vx_grid_surface(m_grid.get(), nullptr, 0, nullptr, 0, mats ? &probe : nullptr, &nv, &nt));
        xyz.assign(nv * 3, 0.0f);
        tris.assign(nt * 3, 0);
        if (mats) mats->assign(nt, 0);
        if (nv || nt) vxdetail::check(vx_grid_surface(m_grid.get(), xyz.data(), nv, tris.data(), nt, mats ? mats->data() : nullptr, &nv, &nt));
    }

    // The surface-nets mesh of the occupancy (vx_grid_surface_smooth): surface()'s vertices and triangles, the positions relaxed inside
    // their dual cubes by params.iterations x (a step with lambda, a step with mu).  normals (optional): 3 floats per vertex.
    void smoothSurface(const vx_smooth& params, std::vector<float>& xyz, std::vector<int32_t>& tris, std::vector<int32_t>* mats = nullptr,
                       std::vector<float>* normals = nullptr) const
    {
        uint64_t nv = 0, nt = 0;
        int32_t probe = 0;
        vxdetail::check(vx_grid_surface_smooth(m_grid.get(), &params, nullptr, 0, nullptr, 0, mats ? &probe : nullptr, nullptr, &nv, &nt));
        xyz.assign(nv * 3, 0.0f);
        tris.assign(nt * 3, 0);
        if (mats) mats->assign(nt, 0);
        if (normals) normals->assign(nv * 3, 0.0f);
        if (nv || nt)
            vxdetail::check(vx_grid_surface_smooth(m_grid.get(), &params, xyz.data(), nv, tris.data(), nt, mats ? mats->data() : nullptr,
                                                   normals ? normals->data() : nullptr, &nv, &nt));
    }

    // Connected components of the occupancy (vx_grid_components): connectivity 6 (shared faces) or 26 (faces, edges, corners).  labels
    // gets one value per cell at x + X*(y + Y*z): 0 for empty cells, 1..K in ascending order of each component's smallest cell.  Returns K.
    uint32_t components(int connectivity, std::vector<uint32_t>& labels) const
    {
        labels.assign(m_x * m_y * m_z, 0u);
        uint64_t k = 0;
        vxdetail::check(vx_grid_components(m_grid.get(), (uint32_t)connectivity, labels.empty() ? nullptr : labels.data(), labels.size(), &k));
        return (uint32_t)k;
    }
    // componentStats: record k - 1 describes label k (cell count, inclusive cell bounds in x, y, z)
    std::vector<vx_component> componentStats(int connectivity) const
    {
        uint64_t k = 0;
        vxdetail::check(vx_grid_component_stats(m_grid.get(), (uint32_t)connectivity, nullptr, 0, &k));
        std::vector<vx_component> ret(k);
        if (k) vxdetail::check(vx_grid_component_stats(m_grid.get(), (uint32_t)connectivity, ret.data(), ret.size(), &k));
        return ret;
    }

    // The feature transform (vx_grid_nearest): per cell the index x + X*(y + Y*z) of its nearest occupied cell (inside: nearest empty cell),
    // the smallest index among equally near ones; 0xFFFFFFFF when there is none.
    std::vector<uint32_t> nearestCells(bool inside = false) const
    {
        std::vector<uint32_t> ret(m_x * m_y * m_z);
        vxdetail::check(vx_grid_nearest(m_grid.get(), inside ? VX_DISTANCE_INSIDE : 0u, ret.data(), ret.size()));
        return ret;
    }
    // nearestLabels: the Voronoi partition of the grid by part -- every cell gets the components(connectivity) label of its nearest occupied
    // cell (all 0 when nothing is occupied).  Returns K.
    uint32_t nearestLabels(int connectivity, std::vector<uint32_t>& labels) const
    {
        std::vector<uint32_t> own;
        const uint32_t k = components(connectivity, own);
        labels.assign(own.size(), 0u);
        if (!own.empty()) vxdetail::check(vx_grid_nearest_gather(m_grid.get(), 0u, own.data(), own.size(), 0u, labels.data(), labels.size()));
        return k;
    }

    // Multi-hit ray query (vx_trace_multi): for each ray (6 floats: origin, direction) the first maxHits (1..32) voxels it meets, ordered by
    // (t, index in getAabbs() order of the Bool grid), into t / prim (maxHits entries per ray, padded with -1 / 0xFFFFFFFF), and the number of
    // all voxels it meets within [tmin, tmax] into count.
    void traceMulti(const std::vector<float>& rays, uint32_t maxHits, float tmin, float tmax, std::vector<float>& t, std::vector<uint32_t>& prim,
                    std::vector<uint32_t>& count) const
    {
        const size_t n = rays.size() / 6;
        t.assign(n * maxHits, -1.0f);
        prim.assign(n * maxHits, 0xFFFFFFFFu);
        count.assign(n, 0u);
        vx_multihit_args a{};
        a.base.rays = rays.data(); a.base.num_rays = n; a.base.tmin = tmin; a.base.tmax = tmax;
        a.base.t = t.data(); a.base.prim = prim.data(); a.max_hits = maxHits; a.count = count.data();
        vxdetail::check(vx_trace_multi(m_grid.get(), &a));
    }

    // Abstract methods (voxelgrid.hpp:124-127)
    virtual std::vector<Aabb> getAabbs() const noexcept = 0;
    virtual void setVoxel(size_t x, size_t y, size_t z, const MaterialObj& material = MaterialObj{}) = 0;

protected:
    virtual T voxelAt(size_t linearIndex) const = 0;

    void deviceSetVoxel(size_t x, size_t y, size_t z)
    {
        if (x >= m_x || y >= m_y || z >= m_z) [[unlikely]] { throw std::runtime_error("Index out of bounds"); }
        vxdetail::check(vx_grid_set_voxel(m_grid.get(), x, y, z));
    }
};

// Morphology of the occupancy with the Euclidean ball of squared radius r2 in cells (vx_grid_morph / vx_grid_seal; r2 = 1, 2, 3: the 6-, 18-,
// 26-neighbourhood).  Every method returns a NEW grid of the same class -- dimensions, voxel size and origin kept, no materials; cells outside
// the grid count as empty.  dilated / eroded grow and shrink; opened drops specks; closed fills gaps narrower than the ball; sealed adds the
// interior that appears once holes up to the ball's size are closed (dilate, fill, erode) -- the solid grid of a mesh that is not watertight.
// The three grid classes derive from this layer.
template <class Derived, typename T>
class VoxelGridMorph : public VoxelGrid<T>
{
protected:
    using VoxelGrid<T>::VoxelGrid;

    Derived morphed(int op, uint32_t r2) const
    {
        vx_grid* g = nullptr;
        vxdetail::check(op < 0 ? vx_grid_seal(this->m_grid.get(), r2, &g) : vx_grid_morph(this->m_grid.get(), (uint32_t)op, r2, &g));
        vxdetail::GridHandle h = vxdetail::adopt(g);
        vx_grid_desc d;
        vxdetail::check(vx_grid_describe(g, &d));
        return Derived(std::move(h), d);
    }

public:
    Derived dilated(uint32_t r2) const { return morphed((int)VX_MORPH_DILATE, r2); }
    Derived eroded(uint32_t r2) const { return morphed((int)VX_MORPH_ERODE, r2); }
    Derived opened(uint32_t r2) const { return morphed((int)VX_MORPH_OPEN, r2); }
    Derived closed(uint32_t r2) const { return morphed((int)VX_MORPH_CLOSE, r2); }
    Derived sealed(uint32_t r2) const { return morphed(-1, r2); }
};
