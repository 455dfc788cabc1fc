// voxilizer.cpp -- the reference's command line for this path:  voxilizer <Path to obj file> <Voxlesize>
// (README.md:57, main.cpp:163 -> HelloVulkan::createAABB, hello_vulkan.cpp:669-699), without the Vulkan window.
// It performs exactly createAABB's call sequence -- VoxelBuilder<VoxelGridBool>{path}, buildVoxelGrid(vs) [timed],
// getAabbs() [timed] -- and prints the reference's three result lines, then throughput figures.
// Optional flags after the two positionals:
//   --grid bool|aabbstruct|vec|octree   grid flavour (default bool, the app's default: hello_vulkan.cpp:677)
//   --parallel                          reproduce the threaded driver's SAT (VoxelBuilder<T,true>)
//   --rays WxH                          also trace WxH primary rays from the reference camera (main.cpp:92, rgen:41-51)
//   --dump FILE                         write the AABB list as raw 24-byte records
//   --bench RUNS                        Benchmaker<T>{path, vs, RUNS} printout (hello_vulkan.h:172-241)
//   --render FILE.ppm [--size WxH]      the reference's picture of the voxels without Vulkan: primary rays from the reference
//                                       camera (main.cpp:92, raytrace.rgen:41-51), cube normals + Lambert + shadow ray as in
//                                       raytrace2.rchit:53-137 with the default material and light (hello_vulkan.h:84-90), miss
//                                       colour raytrace.rmiss:37, gamma post.frag:36.  Rays run on the GPU, the per-pixel shading
//                                       arithmetic (display, not the hot path) on the host.  --camera-dump FILE writes the two 4x4
//                                       matrices used (column-major float32), for comparisons.
//   --gpus N [--logical]                spread the build over N GPUs of this node (word shards + peer copies, vx_voxelize_multi);
//                                       --logical maps all N ranks onto device 0 (rehearsal on a box with fewer GPUs)
//   --grid octree --render FILE.ppm     the same picture from the octree's list (hello_vulkan.cpp:690-697), traced on the tree itself
//                                       (vx_octree_trace_ex) with the default material; --materials is refused there
//   --render FILE.ppm --mesh FILE.obj   the reference's full frame: the triangle model beside the voxels in one scene (hello_vulkan.cpp:596-635
//                                       triangle BLAS + the voxel AABB BLAS under one TLAS).  The model is read as loadModel does
//                                       (hello_vulkan.cpp:197) and traced on its BVH (vx_bvh_trace_ex).  A primary ray takes the closer of the
//                                       voxel hit and the triangle hit; on EQUAL t the voxel wins.  A voxel hit is shaded as without --mesh; a
//                                       triangle hit as raytrace.rchit:49-143 with the geometric normal turned toward the ray (the library has
//                                       no vertex normals), the triangle's OBJ material (MaterialObj{} without one), no textures.  Shadow rays
//                                       from both kinds of hit are any-hit queries against the voxels AND the mesh.  --grid bool or octree
//                                       (the grids that render); refused with --bench.
//   --render FILE.ppm --frames N        the same scene as a whole frame on the device (vx_render_frame_device: shading, shadow rays and the
//                                       merge of voxel and triangle hits in kernels, one asynchronous sequence per frame), N frames from the
//                                       reference camera; writes the last one and prints its hit counts and the device frame time (host wall
//                                       between device-synchronised points, first frame excluded).  Refused with --bench.
//   --render F.ppm --mesh M.obj --frames N --attributes
//                                       the frames shade the mesh's triangles in attribute mode (vx_render_set_shading): interpolated vertex
//                                       normals and the map_Kd textures of its materials (PPM / TGA, loaded by vx_mesh_load_textures), as
//                                       raytrace.rchit:73-74,99-104; with or without --instances.  Refused without --frames or --mesh.
//   --solid                             solid voxelization (VX_VOXELIZE_SOLID): the enclosed empty cells are filled after the triangle loop;
//                                       one more line gives their count.  bool / aabbstruct / vec with their options; not with --grid octree,
//                                       --gpus N > 1 or --bench
//   --morph OP:RADIUS                   the built grid is replaced by its morphology (vx_grid_morph) before every output that reads it (--dump,
//                                       --sdf, --surface, --components, --xray, --render): OP dilate|erode|open|close, RADIUS in cells (may be
//                                       fractional: radius_sq = floor(RADIUS^2)); one more line, morph: OP r2=.. occupied A -> B
//   --seal RADIUS                       the same with vx_grid_seal: the grid plus the interior behind holes up to the ball's size; bool /
//                                       aabbstruct / vec; neither with --grid octree, --bench or --materials (the result has none)
//   --sdf FILE                          the grid's signed distance field (vx_grid_sdf: voxel size x Euclidean distance to the nearest occupied
//                                       cell, negative inside by the distance to the nearest empty one) as raw little-endian f32, x fastest,
//                                       X*Y*Z values; one line gives the dims and the finite min / max.  bool / aabbstruct / vec, with or
//                                       without --solid; not with --grid octree, --gpus N > 1 or --bench
//   --probe POINTS.txt [--probe-out FILE]
//                                       the grid's distance field sampled at the file's points ("x y z" per line; vx_field_sample): per point a
//                                       line "x y z value gx gy gz occupied" (%.9g) to FILE or the standard output, and one summary line.
//                                       bool / aabbstruct / vec; not with --grid octree, --gpus N > 1 or --bench
//   --sphere-depth FILE.pgm --radius R [--size WxH]
//                                       a sphere of radius R (world units) cast along every camera ray of --xray's picture
//                                       (vx_field_sphere_trace) as a binary 16-bit PGM: 0 = no hit, else 1 + t in sixteenths of the voxel size,
//                                       at most 65535; same grids and refusals as --probe
//   --poses POSES.txt --body POINTS.txt [--pose-margin M] [--pose-out FILE]
//                                       a body of points or spheres ("x y z [radius]" per line, body frame, world units) under the file's poses
//                                       (12 floats per line: body to world, row-major 3 x 4) against the grid's distance field
//                                       (vx_field_poses): per pose a line "clearance point count px py pz gx gy gz" (%.9g) to FILE or the
//                                       standard output -- the smallest value - radius over the body, the point that has it, the number of
//                                       points within M (default 0), the contact position and the normal there -- and one summary line with
//                                       the number of colliding poses (count > 0); same grids and refusals as --probe
//   --nearest FILE [--nearest-inside]   the grid's feature transform (vx_grid_nearest: per cell the index x + X*(y + Y*z) of its nearest occupied
//                                       cell, the smallest index among equally near ones; --nearest-inside: of its nearest empty cell;
//                                       0xFFFFFFFF when there is none) as raw little-endian u32, x fastest, X*Y*Z values; one line gives the
//                                       dims and the largest squared distance to a nearest cell.  bool / aabbstruct / vec, with or without
//                                       --solid and --morph; not with --grid octree, --gpus N > 1 or --bench
//   --surface FILE.obj                  the boundary mesh of the grid (vx_grid_surface: two triangles per exposed cell face over shared lattice
//                                       points) as an OBJ: `v` lines in vertex order, then `f` lines (1-based) in triangle order.  With
//                                       --materials also FILE.mtl (one `newmtl m<id>` per grid material) and a `usemtl m<id>` before each run
//                                       of equal ids.  bool / aabbstruct / vec, with or without --solid; not with --grid octree, --gpus N > 1,
//                                       --bench, or --materials with --grid vec
//   --surface FILE.obj --smooth N[:LAMBDA:MU]
//                                       the surface-nets mesh instead (vx_grid_surface_smooth: the same vertices and triangles, positions
//                                       relaxed by N iterations of a step with LAMBDA, then one with MU; default 0.5:-0.53), with one `vn` line
//                                       per vertex after the `v` lines and faces written `f a//a b//b c//c`; the usemtl runs as above.
//                                       Refused without --surface
//   --xray FILE.pgm [--size WxH]        how many voxels each camera ray of --render meets (vx_trace_multi's count), as a binary 16-bit PGM
//                                       (big-endian, min(count, 65535) per pixel); --camera-dump FILE as for --render
//   --grid octree --octree-xray FILE.pgm [--size WxH]
//                                       the same picture from the octree (vx_octree_trace_multi's count: duplicate items are one voxel), same
//                                       file format, --camera-dump FILE as for --render; not with --gpus N > 1 or --bench
//   --mesh M.obj --mesh-xray FILE.pgm [--size WxH]
//                                       the same picture of the triangle model itself: how many triangles of M.obj each camera ray crosses
//                                       (vx_bvh_trace_multi's count), same file format; --mesh then needs no --render
//   --components FILE.csv [--connectivity 6|26]
//                                       the connected components of the grid's occupied cells (vx_grid_component_stats; 6: shared faces, the
//                                       default; 26: faces, edges and corners) as CSV: a header line, then label,cells,minx,miny,minz,maxx,
//                                       maxy,maxz per component in label order (bounds in cells, inclusive); one line gives K.  bool /
//                                       aabbstruct / vec, with or without --solid; not with --grid octree, --gpus N > 1 or --bench
//   --materials                         switch on the reference's commented-out material plumbing (usemtl / mtllib -> per-voxel
//                                       material ids; VoxelBuilder.hpp:375-395): --render shades with them, --dump-materials FILE writes
//                                       getMatIdx() as int16
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>

#include <hip/hip_runtime_api.h>

#include "Benchmaker.hpp"
#include "VoxelBuilder.hpp"
#include "octTree.hpp"

namespace {
using Clock = std::chrono::high_resolution_clock;

void dump(const std::string& file, const std::vector<Aabb>& a)
{
    if (file.empty()) return;
    std::ofstream f(file, std::ios::binary);
    f.write(reinterpret_cast<const char*>(a.data()), (std::streamsize)(a.size() * sizeof(Aabb)));
}

struct V3 { float x, y, z; };
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V3 norm(V3 a) { const float l = std::sqrt(dot(a, a)); return {a.x / l, a.y / l, a.z / l}; }

// viewInverse / projInverse as the reference uploads them (hello_vulkan.cpp:69-77): lookAt RH, perspectiveRH_ZO, [1][1] *= -1
void camera(float vi[16], float pi[16], float aspect)
{
    const V3 eye{6.16636f, 2.42256f, -3.15471f}, ctr{0.f, 1.f, 0.f}, up{0.f, 1.f, 0.f};  // main.cpp:92
    const V3 f = norm(ctr - eye), s = norm(cross(f, up)), u = cross(s, f);
    const float m[16] = {s.x, s.y, s.z, 0, u.x, u.y, u.z, 0, -f.x, -f.y, -f.z, 0, eye.x, eye.y, eye.z, 1};  // columns: s, u, -f, eye
    for (int i = 0; i < 16; ++i) vi[i] = m[i];
    const float fov = 60.0f * 3.14159265358979f / 180.0f;  // nvpro CameraManip default (third-party; unpinned in the tree)
    const float t = std::tan(fov * 0.5f), zn = 0.1f, zf = 1000.0f;
    const float a = 1.0f / (aspect * t), b = -1.0f / t, c = zf / (zn - zf), d = -(zf * zn) / (zf - zn);
    for (int i = 0; i < 16; ++i) pi[i] = 0.f;
    pi[0] = 1.0f / a; pi[5] = 1.0f / b; pi[11] = 1.0f / d; pi[14] = -1.0f; pi[15] = c / d;  // column-major inverse of the projection
}

// the triangle model of --mesh: its BVH and what raytrace.rchit reads besides the hit (vertices, per-triangle material)
struct MeshScene {
    vx_bvh* bvh = nullptr;
    const vx_mesh* model = nullptr;
    const float* verts = nullptr;
    const int32_t* idx = nullptr;
    std::vector<MaterialObj> materials;  // the OBJ's records
    const int32_t* matIds = nullptr;     // per triangle, -1 = none (null: the file has no materials)
    std::vector<vx_instance> instances;  // --instances: placements of the model (object-to-world, row-major 3x4); empty = the model once, as is
    bool attributes = false;             // --attributes: the frames shade its triangles with vertex normals and diffuse textures
};

struct RenderOpts { std::vector<MaterialObj> materials; std::vector<int16_t> matIdx; std::string cameraDump; const MeshScene* mesh = nullptr; long frames = 0; };

void hip_check(hipError_t e)
{
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP: ") + hipGetErrorString(e));
}

// --frames N: the picture of render() as device frames (vx_render_frame_device) on the default stream; the last one is written to `file`
int render_frames(const vx_grid* grid, const vx_octree* octree, const std::string& file, uint32_t W, uint32_t H, const RenderOpts& ro)
{
    float vi[16], pi[16];
    camera(vi, pi, (float)W / (float)H);
    if (!ro.cameraDump.empty()) {
        std::ofstream cf(ro.cameraDump, std::ios::binary);
        cf.write(reinterpret_cast<const char*>(vi), 64);
        cf.write(reinterpret_cast<const char*>(pi), 64);
    }
    vx_render_scene* scene = nullptr;
    std::unique_ptr<vx_tlas, void (*)(vx_tlas*)> tlas(nullptr, vx_tlas_free);
    if (ro.mesh && !ro.mesh->instances.empty()) {  // the model at every placement: a TLAS over its BVH (createTopLevelAS)
        const vx_bvh* bl[1] = {ro.mesh->bvh};
        vx_tlas* t = nullptr;
        vxdetail::check(vx_tlas_build(bl, 1, ro.mesh->instances.data(), ro.mesh->instances.size(), nullptr, &t));
        tlas.reset(t);
        const vx_mesh* ms[1] = {ro.mesh->model};
        vx_render_tlas_desc d{};
        d.grid = grid;
        d.octree = octree;
        d.tlas = t;
        d.meshes = ms;
        vxdetail::check(vx_render_create_tlas(&d, &scene));
        std::printf("[voxhip] %zu instances of the mesh, TLAS height %u\n", ro.mesh->instances.size(), vx_tlas_height(t));
    } else {
        vx_render_desc d{};
        d.grid = grid;
        d.octree = octree;
        if (ro.mesh) { d.bvh = ro.mesh->bvh; d.mesh = ro.mesh->model; }
        vxdetail::check(vx_render_create(&d, &scene));
    }
    std::unique_ptr<vx_render_scene, void (*)(vx_render_scene*)> keep(scene, vx_render_free);
    if (ro.mesh && ro.mesh->attributes) vxdetail::check(vx_render_set_shading(scene, VX_RENDER_ATTRIBUTES));  // --attributes: vertex normals and textures
    const size_t n = (size_t)W * H;
    void *drgba = nullptr, *dkind = nullptr;
    hip_check(hipMalloc(&drgba, n * 4));
    hip_check(hipMalloc(&dkind, n));
    vx_render_args a{};
    a.view_inverse = vi; a.proj_inverse = pi; a.width = W; a.height = H;
    a.rgba = static_cast<uint32_t*>(drgba);
    a.kind = static_cast<uint8_t*>(dkind);
    // frame 1 builds the traversal structure and sizes the scene's buffers; frames 2..N are timed as a block between two synchronisations
    vxdetail::check(vx_render_frame_device(scene, &a));
    hip_check(hipStreamSynchronize(nullptr));
    const auto t0 = Clock::now();
    for (long f = 1; f < ro.frames; ++f) vxdetail::check(vx_render_frame_device(scene, &a));
    hip_check(hipStreamSynchronize(nullptr));
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    std::vector<uint32_t> rgba(n);
    std::vector<uint8_t> kind(n);
    hip_check(hipMemcpy(rgba.data(), drgba, n * 4, hipMemcpyDeviceToHost));
    hip_check(hipMemcpy(kind.data(), dkind, n, hipMemcpyDeviceToHost));
    hip_check(hipFree(drgba));
    hip_check(hipFree(dkind));
    std::vector<unsigned char> img(3 * n);
    size_t hits = 0, thits = 0;
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) img[3 * i + k] = (unsigned char)(rgba[i] >> (8 * k));
        hits += kind[i] == 1;
        thits += kind[i] == 2;
    }
    std::ofstream f(file, std::ios::binary);
    f << "P6\n" << W << " " << H << "\n255\n";
    f.write(reinterpret_cast<const char*>(img.data()), (std::streamsize)img.size());
    if (ro.mesh) std::printf("[voxhip] rendered %ux%u to %s: %zu of %zu primary rays hit a voxel, %zu hit a triangle\n", W, H, file.c_str(), hits, n, thits);
    else std::printf("[voxhip] rendered %ux%u to %s: %zu of %zu primary rays hit a voxel\n", W, H, file.c_str(), hits, n);
    const long timed = ro.frames - 1;
    if (timed > 0) std::printf("[voxhip] device frame %ux%u: %.3f ms/frame (%.1f FPS) over %ld frames\n", W, H, ms / (double)timed, 1000.0 * (double)timed / ms, timed);
    else std::printf("[voxhip] device frame %ux%u: no timed frame (--frames 1)\n", W, H);
    return 0;
}

// computeSpecular, wavefront.glsl:32-48
void specular(const MaterialObj& mat, V3 dir, V3 N, V3 L, float spec[3])
{
    const float kPi = 3.14159265f, kSh = std::fmax(mat.shininess, 4.0f);
    const float kE = (2.0f + kSh) / (2.0f * kPi);
    const V3 V = norm(dir * -1.0f);
    const V3 I = L * -1.0f;                                     // reflect(-L, N) = I - 2 dot(N, I) N
    const V3 Rr = I - N * (2.0f * dot(N, I));
    const float sp = kE * std::pow(std::fmax(dot(V, Rr), 0.0f), kSh);
    spec[0] = mat.specular.x * sp; spec[1] = mat.specular.y * sp; spec[2] = mat.specular.z * sp;
}

// trace(const vx_trace_args*) -> vx_status runs one ray batch on whatever holds the boxes: vx_trace_ex on a grid, vx_octree_trace_ex on an octree
template <class Trace>
int render(Trace trace, const std::string& file, uint32_t W, uint32_t H, const RenderOpts& ro)
{
    float vi[16], pi[16];
    camera(vi, pi, (float)W / (float)H);
    if (!ro.cameraDump.empty()) {
        std::ofstream cf(ro.cameraDump, std::ios::binary);
        cf.write(reinterpret_cast<const char*>(vi), 64);
        cf.write(reinterpret_cast<const char*>(pi), 64);
    }
    const size_t n = (size_t)W * H;
    std::vector<float> t(n), nrm(3 * n), rays(6 * n), tmaxs(n);
    std::vector<uint32_t> prim(n);
    std::vector<uint8_t> shadowed(n);
    vx_trace_args a{};
    a.view_inverse = vi; a.proj_inverse = pi; a.width = W; a.height = H; a.tmin = 0.001f; a.tmax = 10000.0f;  // rgen:50-51
    a.t = t.data(); a.prim = prim.data(); a.normal = nrm.data();
    vxdetail::check(trace(&a));
    // --mesh: the same primary rays against the triangles; the closer hit wins, the voxel on equal t
    const MeshScene* ms = ro.mesh;
    std::vector<float> mt, mnrm, mbary;
    std::vector<uint32_t> mprim;
    std::vector<uint8_t> tri(n, 0);
    if (ms) {
        mt.resize(n); mnrm.resize(3 * n); mbary.resize(2 * n); mprim.resize(n);
        vx_bvh_trace_args ma{};
        ma.base = a;
        ma.base.t = mt.data(); ma.base.prim = mprim.data(); ma.base.normal = mnrm.data(); ma.bary = mbary.data();
        vxdetail::check(vx_bvh_trace_ex(ms->bvh, &ma));
        for (size_t i = 0; i < n; ++i) tri[i] = mt[i] > 0 && !(t[i] > 0 && t[i] <= mt[i]);
    }
    // shadow rays from the hit points toward the point light (rchit:76-122)
    const V3 light{10.f, 55.f, 8.f};  // hello_vulkan.h:86
    const float intensity = 1000.f;   // :88
    const V3 org{vi[12], vi[13], vi[14]};
    std::vector<V3> dirs(n);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t px = (uint32_t)(i % W), py = (uint32_t)(i / W);
        const float u = ((float)px + 0.5f) / (float)W, v = ((float)py + 0.5f) / (float)H, dx = u * 2.f - 1.f, dy = v * 2.f - 1.f;
        const V3 tg = norm(V3{pi[0] * dx + pi[4] * dy + pi[8] + pi[12], pi[1] * dx + pi[5] * dy + pi[9] + pi[13], pi[2] * dx + pi[6] * dy + pi[10] + pi[14]});
        dirs[i] = V3{vi[0] * tg.x + vi[4] * tg.y + vi[8] * tg.z, vi[1] * tg.x + vi[5] * tg.y + vi[9] * tg.z, vi[2] * tg.x + vi[6] * tg.y + vi[10] * tg.z};
        const V3 wp = org + dirs[i] * (tri[i] ? mt[i] : (t[i] > 0 ? t[i] : 0.f));
        V3 l = light - wp;
        if (tri[i]) {  // rchit:67-68,78-83: the light vector from the hit position interpolated with the barycentrics
            const int32_t* ti = ms->idx + 3 * (size_t)mprim[i];
            const float b1 = mbary[2 * i], b2 = mbary[2 * i + 1], b0 = 1.0f - b1 - b2;
            const float* p0 = ms->verts + 3 * (size_t)ti[0];
            const float* p1 = ms->verts + 3 * (size_t)ti[1];
            const float* p2 = ms->verts + 3 * (size_t)ti[2];
            const V3 pos{p0[0] * b0 + p1[0] * b1 + p2[0] * b2, p0[1] * b0 + p1[1] * b1 + p2[1] * b2, p0[2] * b0 + p1[2] * b1 + p2[2] * b2};
            l = light - pos;
        }
        const float dist = std::sqrt(dot(l, l));
        const V3 L = l * (1.0f / dist);
        rays[6 * i + 0] = wp.x; rays[6 * i + 1] = wp.y; rays[6 * i + 2] = wp.z;
        rays[6 * i + 3] = L.x; rays[6 * i + 4] = L.y; rays[6 * i + 5] = L.z;
        tmaxs[i] = dist;
    }
    vx_trace_args sa{};
    sa.rays = rays.data(); sa.num_rays = n; sa.tmin = 0.001f; sa.tmax = 10000.0f; sa.tmax_per_ray = tmaxs.data(); sa.any_hit = 1;
    sa.shadowed = shadowed.data();
    vxdetail::check(trace(&sa));
    if (ms) {  // the TLAS holds both BLAS kinds: a shadow ray is blocked by a voxel or a triangle
        std::vector<uint8_t> ms_shadowed(n);
        vx_bvh_trace_args mb{};
        mb.base = sa;
        mb.base.shadowed = ms_shadowed.data();
        vxdetail::check(vx_bvh_trace_ex(ms->bvh, &mb));
        for (size_t i = 0; i < n; ++i) shadowed[i] |= ms_shadowed[i];
    }
    const MaterialObj defmat{};  // the single default material createAABB uploads (hello_vulkan.cpp:701-702)
    std::vector<unsigned char> img(3 * n);
    size_t hits = 0, thits = 0;
    for (size_t i = 0; i < n; ++i) {
        float c[3] = {0.8f, 0.8f, 0.8f};  // rmiss:37 with the white clear colour of main.cpp:184
        if (tri[i]) {  // raytrace.rchit:49-143
            ++thits;
            V3 N{mnrm[3 * i], mnrm[3 * i + 1], mnrm[3 * i + 2]};
            if (dot(N, dirs[i]) > 0.0f) N = N * -1.0f;                          // the geometric normal, toward the ray
            const V3 L{rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
            const int32_t mi = ms->matIds ? ms->matIds[mprim[i]] : -1;           // rchit:92-93
            const MaterialObj& mat = (mi >= 0 && (size_t)mi < ms->materials.size()) ? ms->materials[(size_t)mi] : defmat;
            const float li = intensity / (tmaxs[i] * tmaxs[i]);                 // rchit:83
            const float dnl = std::fmax(dot(N, L), 0.0f);                       // computeDiffuse, wavefront.glsl:25
            float diff[3] = {mat.diffuse.x * dnl, mat.diffuse.y * dnl, mat.diffuse.z * dnl};
            if (mat.illum >= 1) { diff[0] += mat.ambient.x; diff[1] += mat.ambient.y; diff[2] += mat.ambient.z; }
            float att = 1.0f, spec[3] = {0.f, 0.f, 0.f};                        // rchit:106-140
            if (dot(N, L) > 0) {
                if (shadowed[i]) att = 0.3f;
                else if (mat.illum >= 2) specular(mat, dirs[i], N, L, spec);
            }
            for (int k = 0; k < 3; ++k) c[k] = li * att * (diff[k] + spec[k]);
        } else if (t[i] > 0) {
            ++hits;
            const V3 N{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]}, L{rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
            // matIndices.i[gl_PrimitiveID] -> materials.m[matIdx] (rchit:92-94); without --materials: index 0 of the one default material
            const MaterialObj& mat = (!ro.matIdx.empty() && prim[i] < ro.matIdx.size() && (size_t)ro.matIdx[prim[i]] < ro.materials.size())
                                         ? ro.materials[(size_t)ro.matIdx[prim[i]]] : defmat;
            const float li = intensity / (tmaxs[i] * tmaxs[i]);                 // rchit:85
            const float dnl = std::fmax(dot(N, L), 0.0f);                       // wavefront.glsl:25
            float diff[3] = {mat.diffuse.x * dnl, mat.diffuse.y * dnl, mat.diffuse.z * dnl};
            if (mat.illum >= 1) { diff[0] += mat.ambient.x; diff[1] += mat.ambient.y; diff[2] += mat.ambient.z; }
            float att = 0.3f, spec[3] = {0.f, 0.f, 0.f};                        // rchit:99-133
            if (dot(N, L) > 0 && !shadowed[i]) {
                att = 1.0f;
                if (mat.illum >= 2) specular(mat, dirs[i], N, L, spec);
            }
            for (int k = 0; k < 3; ++k) c[k] = li * att * (diff[k] + spec[k]);
        }
        for (int k = 0; k < 3; ++k) {
            const float g = std::pow(std::fmin(std::fmax(c[k], 0.f), 1.f), 1.0f / 2.2f);  // post.frag:36
            img[3 * i + k] = (unsigned char)std::lround(g * 255.0f);
        }
    }
    std::ofstream f(file, std::ios::binary);
    f << "P6\n" << W << " " << H << "\n255\n";
    f.write(reinterpret_cast<const char*>(img.data()), (std::streamsize)img.size());
    if (ms) std::printf("[voxhip] rendered %ux%u to %s: %zu of %zu primary rays hit a voxel, %zu hit a triangle\n", W, H, file.c_str(), hits, n, thits);
    else std::printf("[voxhip] rendered %ux%u to %s: %zu of %zu primary rays hit a voxel\n", W, H, file.c_str(), hits, n);
    return 0;
}

// --smooth N[:LAMBDA:MU]: the surface-nets parameters of --surface
struct SmoothOpt {
    bool on = false;
    vx_smooth p{0u, 0.5f, -0.53f};
};
SmoothOpt g_smooth;

bool parse_smooth(const char* s, SmoothOpt* o)
{
    unsigned n = 0;
    float lam = 0.5f, mu = -0.53f;
    char tail = 0;
    if (s[0] == '-' || (std::sscanf(s, "%u:%f:%f%c", &n, &lam, &mu, &tail) != 3 && std::sscanf(s, "%u%c", &n, &tail) != 1)) return false;
    if (n > 1024u || !(lam >= 0.0f && lam <= 1.0f) || !(mu >= -1.0f && mu <= 0.0f)) return false;
    o->on = true;
    o->p = vx_smooth{n, lam, mu};
    return true;
}

// --surface: the grid's boundary mesh as an OBJ (and, with materials, its MTL beside it)
template <class T>
void write_surface(const T& vox, const std::string& file, bool materials)
{
    std::vector<float> xyz;
    std::vector<int32_t> tris, mats;
    std::vector<float> normals;
    if (g_smooth.on) vox.smoothSurface(g_smooth.p, xyz, tris, materials ? &mats : nullptr, &normals);
    else vox.surface(xyz, tris, materials ? &mats : nullptr);
    std::FILE* f = std::fopen(file.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + file);
    if (materials) {
        std::string mtl = file;
        const size_t dot = mtl.find_last_of('.'), slash = mtl.find_last_of("/\\");
        if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) mtl.resize(dot);
        mtl += ".mtl";
        std::vector<vx_material> recs;
        uint64_t n = 0;
        vxdetail::check(vx_grid_materials(vox.handle(), nullptr, 0, &n));
        recs.resize(n);
        if (n) vxdetail::check(vx_grid_materials(vox.handle(), recs.data(), n, &n));
        std::FILE* m = std::fopen(mtl.c_str(), "w");
        if (!m) { std::fclose(f); throw std::runtime_error("cannot write " + mtl); }
        for (size_t i = 0; i < recs.size(); ++i) {
            const vx_material& r = recs[i];
            std::fprintf(m, "newmtl m%zu\n", i);
            const float* v3[5] = {r.ambient, r.diffuse, r.specular, r.transmittance, r.emission};
            const char* k3[5] = {"Ka", "Kd", "Ks", "Tf", "Ke"};
            for (int k = 0; k < 5; ++k) std::fprintf(m, "%s %.9g %.9g %.9g\n", k3[k], (double)v3[k][0], (double)v3[k][1], (double)v3[k][2]);
            std::fprintf(m, "Ns %.9g\nNi %.9g\nd %.9g\nillum %d\n", (double)r.shininess, (double)r.ior, (double)r.dissolve, (int)r.illum);
        }
        std::fclose(m);
        const size_t s2 = mtl.find_last_of("/\\");
        std::fprintf(f, "mtllib %s\n", s2 == std::string::npos ? mtl.c_str() : mtl.c_str() + s2 + 1);
    }
    for (size_t i = 0; i < xyz.size(); i += 3) std::fprintf(f, "v %.9g %.9g %.9g\n", (double)xyz[i], (double)xyz[i + 1], (double)xyz[i + 2]);
    for (size_t i = 0; i < normals.size(); i += 3) std::fprintf(f, "vn %.9g %.9g %.9g\n", (double)normals[i], (double)normals[i + 1], (double)normals[i + 2]);
    for (size_t t = 0; t < tris.size() / 3; ++t) {
        if (materials && (t == 0 || mats[t] != mats[t - 1])) std::fprintf(f, "usemtl m%d\n", (int)mats[t]);
        const int a = tris[3 * t] + 1, b = tris[3 * t + 1] + 1, c = tris[3 * t + 2] + 1;
        if (g_smooth.on) std::fprintf(f, "f %d//%d %d//%d %d//%d\n", a, a, b, b, c, c);
        else std::fprintf(f, "f %d %d %d\n", a, b, c);
    }
    const bool ok = std::ferror(f) == 0;
    if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + file);
    std::printf("[voxhip] surface: %zu vertices, %zu triangles\n", xyz.size() / 3, tris.size() / 3);
}

// the reference camera of a WxH picture, written to `cameraDump` when that is given
void xray_camera(float vi[16], float pi[16], uint32_t W, uint32_t H, const std::string& cameraDump)
{
    camera(vi, pi, (float)W / (float)H);
    if (!cameraDump.empty()) {
        std::ofstream cf(cameraDump, std::ios::binary);
        cf.write(reinterpret_cast<const char*>(vi), 64);
        cf.write(reinterpret_cast<const char*>(pi), 64);
    }
}

// per-pixel hit counts as a binary 16-bit PGM (min(count, 65535), most significant byte first) and the summary line; `what` names the hits
void write_counts_pgm(const std::vector<uint32_t>& count, const std::string& file, uint32_t W, uint32_t H, const char* what)
{
    const size_t n = (size_t)W * H;
    std::vector<unsigned char> px(2 * n);
    uint32_t most = 0;
    uint64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = count[i] < 65535u ? count[i] : 65535u;
        px[2 * i] = (unsigned char)(c >> 8);  // PGM samples above 255 are two bytes, most significant first
        px[2 * i + 1] = (unsigned char)(c & 255u);
        most = std::max(most, count[i]);
        sum += count[i];
    }
    std::ofstream f(file, std::ios::binary);
    f << "P5\n" << W << ' ' << H << "\n65535\n";
    f.write(reinterpret_cast<const char*>(px.data()), (std::streamsize)px.size());
    if (!f) throw std::runtime_error("cannot write " + file);
    std::printf("[voxhip] xray %ux%u: %llu %s crossings, at most %u on a ray\n", W, H, (unsigned long long)sum, what, most);
}

// --xray: the hit count of every primary ray of the reference camera as a 16-bit PGM
void write_xray(const vx_grid* grid, const std::string& file, uint32_t W, uint32_t H, const std::string& cameraDump)
{
    float vi[16], pi[16];
    xray_camera(vi, pi, W, H, cameraDump);
    std::vector<uint32_t> count((size_t)W * H);
    vx_multihit_args a{};
    a.base.view_inverse = vi; a.base.proj_inverse = pi; a.base.width = W; a.base.height = H; a.base.tmin = 0.001f; a.base.tmax = 10000.0f;  // rgen:50-51
    a.max_hits = 1;
    a.count = count.data();
    vxdetail::check(vx_trace_multi(grid, &a));
    write_counts_pgm(count, file, W, H, "voxel");
}

// --octree-xray: the same picture from the octree (vx_octree_trace_multi's count)
void write_octree_xray(const vx_octree* octree, const std::string& file, uint32_t W, uint32_t H, const std::string& cameraDump)
{
    float vi[16], pi[16];
    xray_camera(vi, pi, W, H, cameraDump);
    std::vector<uint32_t> count((size_t)W * H);
    vx_multihit_args a{};
    a.base.view_inverse = vi; a.base.proj_inverse = pi; a.base.width = W; a.base.height = H; a.base.tmin = 0.001f; a.base.tmax = 10000.0f;  // rgen:50-51
    a.max_hits = 1;
    a.count = count.data();
    vxdetail::check(vx_octree_trace_multi(octree, &a));
    write_counts_pgm(count, file, W, H, "voxel");
}

// --mesh-xray: the same picture of the --mesh model itself, the triangles every primary ray crosses (vx_bvh_trace_multi's count)
void write_mesh_xray(const vx_bvh* bvh, const std::string& file, uint32_t W, uint32_t H, const std::string& cameraDump)
{
    float vi[16], pi[16];
    xray_camera(vi, pi, W, H, cameraDump);
    std::vector<uint32_t> count((size_t)W * H);
    vx_bvh_multihit_args a{};
    a.m.base.view_inverse = vi; a.m.base.proj_inverse = pi; a.m.base.width = W; a.m.base.height = H; a.m.base.tmin = 0.001f; a.m.base.tmax = 10000.0f;  // rgen:50-51
    a.m.max_hits = 1;
    a.m.count = count.data();
    vxdetail::check(vx_bvh_trace_multi(bvh, &a));
    write_counts_pgm(count, file, W, H, "triangle");
}

// --nearest FILE [--nearest-inside]
struct NearestOpt {
    std::string file;
    bool inside = false;
};
NearestOpt g_nearest;

// --probe POINTS.txt [--probe-out FILE], --sphere-depth FILE.pgm --radius R: queries on the grid's distance field (DistanceField)
struct FieldOpt {
    std::string probe, probeOut, depth;
    float radius = 0.0f;
    bool radiusGiven = false;
    std::string poses, body, poseOut;  // --poses POSES.txt --body POINTS.txt [--pose-margin M] [--pose-out FILE]
    float poseMargin = 0.0f;
    bool poseMarginGiven = false;
};
FieldOpt g_field;

// --probe: "x y z" lines in, "x y z value gx gy gz occupied" lines out (%.9g: every float32 survives the round trip)
void write_probe(const DistanceField& field)
{
    std::ifstream in(g_field.probe);
    if (!in) throw std::runtime_error("cannot read " + g_field.probe);
    std::vector<float> pts;
    for (std::string a, b, c; in >> a >> b >> c;) {
        pts.push_back(std::strtof(a.c_str(), nullptr));  // (strtof reads nan and inf)
        pts.push_back(std::strtof(b.c_str(), nullptr));
        pts.push_back(std::strtof(c.c_str(), nullptr));
    }
    const size_t n = pts.size() / 3;
    std::vector<float> value(n), grad(3 * n);
    std::vector<uint8_t> occ(n);
    vx_field_sample_args a{};
    a.points = pts.data(); a.num_points = n; a.value = value.data(); a.gradient = grad.data(); a.occupied = occ.data();
    if (n) vxdetail::check(vx_field_sample(field.handle(), &a));
    std::FILE* f = g_field.probeOut.empty() ? stdout : std::fopen(g_field.probeOut.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + g_field.probeOut);
    size_t inside = 0;
    for (size_t i = 0; i < n; ++i) {
        std::fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", (double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], (double)value[i],
                     (double)grad[3 * i], (double)grad[3 * i + 1], (double)grad[3 * i + 2], (int)occ[i]);
        inside += occ[i];
    }
    const bool ok = std::ferror(f) == 0;
    if (f != stdout && (std::fclose(f) != 0 || !ok)) throw std::runtime_error("cannot write " + g_field.probeOut);
    std::printf("[voxhip] probe: %zu points, %zu in occupied cells\n", n, inside);
}

// the numbers of every non-empty line of a text file (strtof reads nan and inf)
std::vector<std::vector<float>> read_number_lines(const std::string& path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot read " + path);
    std::vector<std::vector<float>> rows;
    for (std::string line; std::getline(in, line);) {
        std::istringstream ls(line);
        std::vector<float> row;
        for (std::string tok; ls >> tok;) row.push_back(std::strtof(tok.c_str(), nullptr));
        if (!row.empty()) rows.push_back(row);
    }
    return rows;
}

// --poses: "clearance point count px py pz gx gy gz" per pose (%.9g: every float32 survives the round trip; point 4294967295: none)
void write_poses(const DistanceField& field)
{
    std::vector<float> pts, radii, xf;
    for (const std::vector<float>& r : read_number_lines(g_field.body)) {
        if (r.size() != 3 && r.size() != 4) throw std::runtime_error(g_field.body + ": a line is \"x y z\" or \"x y z radius\"");
        pts.insert(pts.end(), r.begin(), r.begin() + 3);
        radii.push_back(r.size() == 4 ? r[3] : 0.0f);
    }
    for (const std::vector<float>& r : read_number_lines(g_field.poses)) {
        if (r.size() != 12) throw std::runtime_error(g_field.poses + ": a line is 12 numbers, a row-major 3 x 4 transform");
        xf.insert(xf.end(), r.begin(), r.end());
    }
    const size_t n = xf.size() / 12;
    std::vector<float> clearance, position, gradient;
    std::vector<uint32_t> point, count;
    field.poses(pts, radii, xf, g_field.poseMargin, clearance, point, count, &position, &gradient);
    std::FILE* f = g_field.poseOut.empty() ? stdout : std::fopen(g_field.poseOut.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + g_field.poseOut);
    size_t colliding = 0;
    for (size_t i = 0; i < n; ++i) {
        std::fprintf(f, "%.9g %u %u %.9g %.9g %.9g %.9g %.9g %.9g\n", (double)clearance[i], point[i], count[i], (double)position[3 * i],
                     (double)position[3 * i + 1], (double)position[3 * i + 2], (double)gradient[3 * i], (double)gradient[3 * i + 1], (double)gradient[3 * i + 2]);
        colliding += count[i] > 0;
    }
    const bool ok = std::ferror(f) == 0;
    if (f != stdout && (std::fclose(f) != 0 || !ok)) throw std::runtime_error("cannot write " + g_field.poseOut);
    std::printf("[voxhip] poses: %zu poses of %zu points, margin %.9g: %zu colliding\n", n, pts.size() / 3, (double)g_field.poseMargin, colliding);
}

void xray_camera(float vi[16], float pi[16], uint32_t W, uint32_t H, const std::string& cameraDump);

// --sphere-depth: the sphere cast's t of every primary ray of the reference camera (the ray of pixel (px, py) as the ray kernels generate
// it) as a 16-bit PGM in --xray's form: 0 = no hit, else 1 + t in sixteenths of the voxel size, at most 65535
void write_sphere_depth(const DistanceField& field, float vs, uint32_t W, uint32_t H, const std::string& cameraDump)
{
    float vi[16], pi[16];
    xray_camera(vi, pi, W, H, cameraDump);
    const size_t n = (size_t)W * H;
    std::vector<float> rays(6 * n), t;
    std::vector<uint8_t> status;
    for (size_t r = 0; r < n; ++r) {
        const uint32_t px = (uint32_t)(r % W), py = (uint32_t)(r / W);
        const float u = ((float)px + 0.5f) / (float)W, v = ((float)py + 0.5f) / (float)H;
        const float ndx = u * 2.0f - 1.0f, ndy = v * 2.0f - 1.0f;
        float tg[3];
        for (int k = 0; k < 3; ++k) tg[k] = (pi[0 + k] * ndx + pi[4 + k] * ndy) + (pi[8 + k] * 1.0f + pi[12 + k] * 1.0f);
        const float il = 1.0f / std::sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2]);
        const float n0 = tg[0] * il, n1 = tg[1] * il, n2 = tg[2] * il;
        float* ray = &rays[6 * r];
        ray[0] = vi[12]; ray[1] = vi[13]; ray[2] = vi[14];
        for (int k = 0; k < 3; ++k) ray[3 + k] = (vi[0 + k] * n0 + vi[4 + k] * n1) + vi[8 + k] * n2;
    }
    field.sphereTrace(rays, g_field.radius, 0.001f, 10000.0f, t, status);
    std::vector<unsigned char> px(2 * n);
    size_t hits = 0, limited = 0;
    float far = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        uint32_t c = 0;
        if (status[i] == VX_FIELD_HIT) {
            const float q = t[i] / vs * 16.0f;
            c = q < 65534.0f ? (uint32_t)q + 1u : 65535u;
            ++hits;
            far = std::max(far, t[i]);
        }
        limited += status[i] == VX_FIELD_STEP_LIMIT;
        px[2 * i] = (unsigned char)(c >> 8);
        px[2 * i + 1] = (unsigned char)(c & 255u);
    }
    std::ofstream f(g_field.depth, std::ios::binary);
    f << "P5\n" << W << ' ' << H << "\n65535\n";
    f.write(reinterpret_cast<const char*>(px.data()), (std::streamsize)px.size());
    if (!f) throw std::runtime_error("cannot write " + g_field.depth);
    std::printf("[voxhip] sphere depth %ux%u: radius %g, %zu hits, farthest t %g, %zu rays at the step limit\n", W, H, (double)g_field.radius, hits, (double)far, limited);
}

// the feature transform of the grid as raw little-endian u32, and one line: the dims and the largest |c - N(c)|^2 over cells that have an N
template <class T>
void write_nearest(const T& vox)
{
    const std::vector<uint32_t> nn = vox.nearestCells(g_nearest.inside);
    const uint64_t X = vox.dimX(), Y = vox.dimY();
    uint64_t far = 0;
    for (uint64_t i = 0; i < nn.size(); ++i) {
        if (nn[i] == 0xFFFFFFFFu) continue;
        const uint64_t o = nn[i];
        const int64_t dx = (int64_t)(i % X) - (int64_t)(o % X), dy = (int64_t)(i / X % Y) - (int64_t)(o / X % Y), dz = (int64_t)(i / (X * Y)) - (int64_t)(o / (X * Y));
        far = std::max<uint64_t>(far, (uint64_t)(dx * dx + dy * dy + dz * dz));
    }
    std::ofstream f(g_nearest.file, std::ios::binary);
    f.write(reinterpret_cast<const char*>(nn.data()), (std::streamsize)(nn.size() * sizeof(uint32_t)));
    if (!f) throw std::runtime_error("cannot write " + g_nearest.file);
    std::printf("[voxhip] nearest: %zu x %zu x %zu cells, max squared distance %llu\n", vox.dimX(), vox.dimY(), vox.dimZ(), (unsigned long long)far);
}

// --morph OP:RADIUS / --seal RADIUS: op 0..3 = VX_MORPH_*, 4 = seal, -1 = none
struct MorphOpt {
    int op = -1;
    uint32_t r2 = 0;
};
MorphOpt g_morph;

bool parse_radius(const char* s, uint32_t* r2)
{
    char* end = nullptr;
    const double r = std::strtod(s, &end);
    if (end == s || *end || !(r >= 0.0) || !(r * r < 4294967295.0)) return false;
    *r2 = (uint32_t)std::floor(r * r);
    return true;
}

bool parse_morph(const char* s, MorphOpt* m)
{
    static const char* names[4] = {"dilate", "erode", "open", "close"};
    const char* colon = std::strchr(s, ':');
    if (!colon) return false;
    for (int k = 0; k < 4; ++k)
        if (std::string(s, colon) == names[k]) { m->op = k; return parse_radius(colon + 1, &m->r2); }
    return false;
}

template <class T>
T apply_morph(const T& g)
{
    static const char* names[5] = {"dilate", "erode", "open", "close", "seal"};
    vx_grid_desc a, b;
    vxdetail::check(vx_grid_describe(g.handle(), &a));
    T out = g_morph.op == 4 ? g.sealed(g_morph.r2)
            : g_morph.op == 0 ? g.dilated(g_morph.r2) : g_morph.op == 1 ? g.eroded(g_morph.r2) : g_morph.op == 2 ? g.opened(g_morph.r2) : g.closed(g_morph.r2);
    vxdetail::check(vx_grid_describe(out.handle(), &b));
    std::printf("[voxhip] morph: %s r2=%u occupied %llu -> %llu\n", names[g_morph.op], g_morph.r2, (unsigned long long)a.occupied, (unsigned long long)b.occupied);
    return out;
}

template <class T, bool P>
int run_grid(const std::string& path, float vs, const std::string& dumpFile, const char* label, const std::string& renderFile = "",
             uint32_t rw = 1280, uint32_t rh = 720, bool materials = false, const std::string& matDump = "", const std::string& cameraDump = "",
             const std::vector<int>& devices = {}, const MeshScene* mesh = nullptr, long frames = 0, bool solid = false, const std::string& sdfFile = "",
             const std::string& surfaceFile = "", const std::string& componentsFile = "", int connectivity = 6, const std::string& xrayFile = "")
{
    VoxelBuilder<T, P> voxelBuilder{std::filesystem::path(path)};
    voxelBuilder.withMaterials(materials);
    voxelBuilder.withSolid(solid);
    voxelBuilder.withDevices(devices);
    if (devices.size() > 1) std::printf("[voxhip] build sharded over %zu ranks (first device %d)\n", devices.size(), devices[0]);
    const auto t0 = Clock::now();
    T built = voxelBuilder.buildVoxelGrid(vs);
    const auto t1 = Clock::now();
    if (solid) {
        uint64_t interior = 0;
        vxdetail::check(vx_grid_interior(built.handle(), &interior));
        std::printf("[voxhip] solid: %llu interior voxels filled\n", (unsigned long long)interior);
    }
    T vox = g_morph.op < 0 ? built : apply_morph(built);  // (every output below reads the morphed grid)
    const std::vector<Aabb> aabbs = vox.getAabbs();
    const auto t2 = Clock::now();
    const auto msBuild = std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count();
    const auto msAabb = std::chrono::duration_cast<std::chrono::milliseconds>(t2 - t1).count();
    std::printf("Voxel build took %lldms\n", (long long)msBuild);                                   // hello_vulkan.cpp:686
    std::printf("Aabb build took %lldms\n", (long long)msAabb);                                     // :687
    std::printf("Total usage of the VoxelGridAABBstruct is %zu\n", vox.getMemoryUsageBytes());      // :688 (label as upstream)
    const double sb = std::chrono::duration<double>(t1 - t0).count(), sa = std::chrono::duration<double>(t2 - t1).count();
    const double cells = (double)vox.dimX() * vox.dimY() * vox.dimZ();
    std::printf("[voxhip] %s: %zu AABBs, %.1f Mvoxels/s build (host wall, incl. launch+sync), %.1f M AABBs/s getAabbs (incl. D2H copy)\n", label,
                aabbs.size(), cells / sb / 1e6, aabbs.size() / (sa > 0 ? sa : 1e-9) / 1e6);
    dump(dumpFile, aabbs);
    if (!sdfFile.empty()) {
        const std::vector<float> sdf = vox.signedDistances();
        float lo = std::numeric_limits<float>::infinity(), hi = -lo;
        for (const float v : sdf)
            if (std::isfinite(v)) { lo = std::min(lo, v); hi = std::max(hi, v); }
        std::ofstream f(sdfFile, std::ios::binary);
        f.write(reinterpret_cast<const char*>(sdf.data()), (std::streamsize)(sdf.size() * sizeof(float)));
        if (!f) throw std::runtime_error("cannot write " + sdfFile);
        std::printf("[voxhip] sdf: %zu x %zu x %zu cells, min %g max %g\n", vox.dimX(), vox.dimY(), vox.dimZ(), (double)lo, (double)hi);
    }
    if (!g_nearest.file.empty()) write_nearest(vox);
    if (!g_field.probe.empty() || !g_field.depth.empty() || !g_field.poses.empty()) {
        const DistanceField field = vox.distanceField();
        if (!g_field.probe.empty()) write_probe(field);
        if (!g_field.poses.empty()) write_poses(field);
        if (!g_field.depth.empty()) write_sphere_depth(field, vox.voxelSize(), rw, rh, cameraDump);
    }
    if (!surfaceFile.empty()) write_surface(vox, surfaceFile, materials);
    if (!componentsFile.empty()) {
        const std::vector<vx_component> cs = vox.componentStats(connectivity);
        std::ofstream f(componentsFile);
        f << "label,cells,minx,miny,minz,maxx,maxy,maxz\n";
        for (size_t k = 0; k < cs.size(); ++k)
            f << k + 1 << ',' << cs[k].cells << ',' << cs[k].min[0] << ',' << cs[k].min[1] << ',' << cs[k].min[2] << ',' << cs[k].max[0] << ','
              << cs[k].max[1] << ',' << cs[k].max[2] << '\n';
        if (!f) throw std::runtime_error("cannot write " + componentsFile);
        std::printf("[voxhip] components: %zu\n", cs.size());
    }
    if (!xrayFile.empty()) write_xray(vox.handle(), xrayFile, rw, rh, cameraDump);
    RenderOpts ro;
    ro.cameraDump = cameraDump;
    ro.mesh = mesh;
    if (materials) {
        ro.materials = vox.getMatrials();
        ro.matIdx = vox.getMatIdx();
        std::printf("[voxhip] materials: %zu distinct, %zu per-voxel ids\n", ro.materials.size(), ro.matIdx.size());
        if (!matDump.empty()) {
            std::ofstream f(matDump, std::ios::binary);
            f.write(reinterpret_cast<const char*>(ro.matIdx.data()), (std::streamsize)(ro.matIdx.size() * sizeof(int16_t)));
        }
    }
    ro.frames = frames;
    if (!renderFile.empty() && frames > 0) return render_frames(vox.handle(), nullptr, renderFile, rw, rh, ro);
    if (!renderFile.empty()) return render([g = vox.handle()](const vx_trace_args* a) { return vx_trace_ex(g, a); }, renderFile, rw, rh, ro);
    return 0;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {  // the reference reads argv[1], argv[2] unchecked (main.cpp:80,163)
        std::fprintf(stderr, "usage: %s <Path to obj file> <Voxlesize> [--grid bool|aabbstruct|vec|octree] [--parallel] [--dump FILE] [--bench RUNS] [--render FILE.ppm [--size WxH] [--camera-dump FILE] [--mesh FILE.obj [--instances FILE]] [--frames N [--attributes]]] [--materials [--dump-materials FILE]] (octree: --render, no --materials) [--gpus N [--logical]] [--solid] [--morph dilate|erode|open|close:RADIUS] [--seal RADIUS] [--sdf FILE] [--nearest FILE [--nearest-inside]] [--probe POINTS.txt [--probe-out FILE]] [--sphere-depth FILE.pgm --radius R [--size WxH]] [--poses POSES.txt --body POINTS.txt [--pose-margin M] [--pose-out FILE]] [--surface FILE.obj [--smooth N[:LAMBDA:MU]]] [--components FILE.csv [--connectivity 6|26]] [--xray FILE.pgm [--size WxH]] [--grid octree --octree-xray FILE.pgm [--size WxH]] [--mesh FILE.obj --mesh-xray FILE.pgm [--size WxH]]\n",
                     argv[0]);
        return 2;
    }
    const std::string path = argv[1];
    float vs = 0.f;
    try { vs = std::stof(argv[2]); } catch (const std::exception&) { std::fprintf(stderr, "invalid voxel size '%s'\n", argv[2]); return 2; }
    std::string grid = "bool", sdfFile, surfaceFile, componentsFile, xrayFile, octreeXrayFile, meshXrayFile, dumpFile, renderFile, matDump, cameraDump, meshFile, instFile;
    uint32_t rw = 1280, rh = 720;  // main.cpp:72-73
    bool parallel = false, materials = false, logical = false, attributes = false, solid = false;
    int gpus = 1, connectivity = 6;
    long benchRuns = 0, frames = 0;
    for (int i = 3; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--grid") && i + 1 < argc) grid = argv[++i];
        else if (!std::strcmp(argv[i], "--parallel")) parallel = true;
        else if (!std::strcmp(argv[i], "--dump") && i + 1 < argc) dumpFile = argv[++i];
        else if (!std::strcmp(argv[i], "--bench") && i + 1 < argc) benchRuns = std::atol(argv[++i]);
        else if (!std::strcmp(argv[i], "--render") && i + 1 < argc) renderFile = argv[++i];
        else if (!std::strcmp(argv[i], "--materials")) materials = true;
        else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--logical")) logical = true;
        else if (!std::strcmp(argv[i], "--dump-materials") && i + 1 < argc) matDump = argv[++i];
        else if (!std::strcmp(argv[i], "--camera-dump") && i + 1 < argc) cameraDump = argv[++i];
        else if (!std::strcmp(argv[i], "--mesh") && i + 1 < argc) meshFile = argv[++i];
        else if (!std::strcmp(argv[i], "--instances") && i + 1 < argc) instFile = argv[++i];
        else if (!std::strcmp(argv[i], "--attributes")) attributes = true;
        else if (!std::strcmp(argv[i], "--solid")) solid = true;
        else if (!std::strcmp(argv[i], "--morph") && i + 1 < argc) { if (!parse_morph(argv[++i], &g_morph)) { std::fprintf(stderr, "bad --morph '%s': OP:RADIUS with OP dilate|erode|open|close and RADIUS >= 0 in cells\n", argv[i]); return 2; } }
        else if (!std::strcmp(argv[i], "--seal") && i + 1 < argc) { g_morph.op = 4; if (!parse_radius(argv[++i], &g_morph.r2)) { std::fprintf(stderr, "bad --seal '%s': a radius >= 0 in cells\n", argv[i]); return 2; } }
        else if (!std::strcmp(argv[i], "--sdf") && i + 1 < argc) sdfFile = argv[++i];
        else if (!std::strcmp(argv[i], "--nearest") && i + 1 < argc) g_nearest.file = argv[++i];
        else if (!std::strcmp(argv[i], "--nearest-inside")) g_nearest.inside = true;
        else if (!std::strcmp(argv[i], "--probe") && i + 1 < argc) g_field.probe = argv[++i];
        else if (!std::strcmp(argv[i], "--probe-out") && i + 1 < argc) g_field.probeOut = argv[++i];
        else if (!std::strcmp(argv[i], "--sphere-depth") && i + 1 < argc) g_field.depth = argv[++i];
        else if (!std::strcmp(argv[i], "--poses") && i + 1 < argc) g_field.poses = argv[++i];
        else if (!std::strcmp(argv[i], "--body") && i + 1 < argc) g_field.body = argv[++i];
        else if (!std::strcmp(argv[i], "--pose-out") && i + 1 < argc) g_field.poseOut = argv[++i];
        else if (!std::strcmp(argv[i], "--pose-margin") && i + 1 < argc) { g_field.poseMargin = std::strtof(argv[++i], nullptr); g_field.poseMarginGiven = true; }
        else if (!std::strcmp(argv[i], "--radius") && i + 1 < argc) { g_field.radius = std::strtof(argv[++i], nullptr); g_field.radiusGiven = true; }
        else if (!std::strcmp(argv[i], "--surface") && i + 1 < argc) surfaceFile = argv[++i];
        else if (!std::strcmp(argv[i], "--smooth") && i + 1 < argc) { if (!parse_smooth(argv[++i], &g_smooth)) { std::fprintf(stderr, "bad --smooth '%s': N[:LAMBDA:MU] with N <= 1024, LAMBDA in [0, 1] and MU in [-1, 0]\n", argv[i]); return 2; } }
        else if (!std::strcmp(argv[i], "--components") && i + 1 < argc) componentsFile = argv[++i];
        else if (!std::strcmp(argv[i], "--xray") && i + 1 < argc) xrayFile = argv[++i];
        else if (!std::strcmp(argv[i], "--octree-xray") && i + 1 < argc) octreeXrayFile = argv[++i];
        else if (!std::strcmp(argv[i], "--mesh-xray") && i + 1 < argc) meshXrayFile = argv[++i];
        else if (!std::strcmp(argv[i], "--connectivity") && i + 1 < argc) connectivity = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--frames") && i + 1 < argc) { frames = std::atol(argv[++i]); if (frames < 1) { std::fprintf(stderr, "--frames needs N >= 1\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--size") && i + 1 < argc) { if (std::sscanf(argv[++i], "%ux%u", &rw, &rh) != 2) { std::fprintf(stderr, "bad --size\n"); return 2; } }
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (!meshXrayFile.empty() && meshFile.empty()) { std::fprintf(stderr, "--mesh-xray counts the triangles of the --mesh model: it needs --mesh\n"); return 2; }
    if (!meshFile.empty() && renderFile.empty() && meshXrayFile.empty()) { std::fprintf(stderr, "--mesh needs --render: the triangle model only takes part in the picture\n"); return 2; }
    if (!meshFile.empty() && (benchRuns > 0 || (grid != "bool" && grid != "octree"))) {
        std::fprintf(stderr, "--mesh renders with --grid bool or octree only, and not with --bench\n");
        return 2;
    }
    if (attributes && (renderFile.empty() || meshFile.empty() || frames < 1)) {
        std::fprintf(stderr, "--attributes shades the --mesh model in device frames: it needs --render, --mesh and --frames\n");
        return 2;
    }
    if (!instFile.empty() && (renderFile.empty() || meshFile.empty() || frames < 1)) {
        std::fprintf(stderr, "--instances places the --mesh model: it needs --render, --mesh and --frames\n");
        return 2;
    }
    if (frames > 0 && (renderFile.empty() || benchRuns > 0 || (grid != "bool" && grid != "octree"))) {
        std::fprintf(stderr, "--frames renders with --render and --grid bool or octree only, and not with --bench\n");
        return 2;
    }
    if (solid && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--solid fills the interior of one grid on one device: not with --grid octree, --gpus N > 1 or --bench\n");
        return 2;
    }
    if (g_morph.op >= 0 && (grid == "octree" || benchRuns > 0 || materials)) {
        std::fprintf(stderr, "--morph / --seal replace a bool, aabbstruct or vec grid by its morphology, which carries no materials: not with --grid octree, --bench or --materials\n");
        return 2;
    }
    if (!sdfFile.empty() && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--sdf writes the distance field of one grid on one device: not with --grid octree, --gpus N > 1 or --bench\n");
        return 2;
    }
    if (!g_nearest.file.empty() && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--nearest writes the nearest-cell field of one grid on one device: not with --grid octree, --gpus N > 1 or --bench\n");
        return 2;
    }
    if ((!g_field.probe.empty() || !g_field.depth.empty()) && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--probe / --sphere-depth query the distance field of one grid on one device: not with --grid octree, --gpus N > 1 or --bench\n");
        return 2;
    }
    if (!g_field.poses.empty() && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--poses queries the distance field of one grid on one device: not with --grid octree, --gpus N > 1 or --bench\n");
        return 2;
    }
    if (g_field.poses.empty() != g_field.body.empty()) {
        std::fprintf(stderr, "--poses POSES.txt and --body POINTS.txt go together: the poses of a body\n");
        return 2;
    }
    if ((!g_field.poseOut.empty() || g_field.poseMarginGiven) && g_field.poses.empty()) {
        std::fprintf(stderr, "--pose-out and --pose-margin belong to --poses POSES.txt --body POINTS.txt\n");
        return 2;
    }
    if (g_field.poseMargin != g_field.poseMargin) { std::fprintf(stderr, "--pose-margin must be a number (inf and -inf are allowed)\n"); return 2; }
    if (!g_field.probeOut.empty() && g_field.probe.empty()) { std::fprintf(stderr, "--probe-out names the file --probe writes: it needs --probe POINTS.txt\n"); return 2; }
    if (g_field.radiusGiven && g_field.depth.empty()) { std::fprintf(stderr, "--radius is the sphere of --sphere-depth: it needs --sphere-depth FILE.pgm\n"); return 2; }
    if (!g_field.depth.empty() && (!g_field.radiusGiven || !(g_field.radius >= 0.0f) || std::isinf(g_field.radius))) {
        std::fprintf(stderr, "--sphere-depth needs --radius R, finite and not negative (world units)\n");
        return 2;
    }
    if (g_nearest.inside && g_nearest.file.empty()) {
        std::fprintf(stderr, "--nearest-inside chooses the field that --nearest writes: it needs --nearest FILE\n");
        return 2;
    }
    if (!surfaceFile.empty() && (grid == "octree" || gpus > 1 || benchRuns > 0 || (materials && grid == "vec"))) {
        std::fprintf(stderr, "--surface writes the boundary mesh of one grid on one device: not with --grid octree, --gpus N > 1, --bench, or --materials with --grid vec\n");
        return 2;
    }
    if (g_smooth.on && surfaceFile.empty()) {
        std::fprintf(stderr, "--smooth relaxes the mesh that --surface writes: it needs --surface FILE.obj\n");
        return 2;
    }
    if (!componentsFile.empty() && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--components labels the occupied cells of one grid on one device: not with --grid octree, --gpus N > 1 or --bench\n");
        return 2;
    }
    if (!xrayFile.empty() && (grid == "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--xray counts the voxels of one grid on one device: not with --grid octree (use --octree-xray there), --gpus N > 1 or --bench\n");
        return 2;
    }
    if (!octreeXrayFile.empty() && (grid != "octree" || gpus > 1 || benchRuns > 0)) {
        std::fprintf(stderr, "--octree-xray counts the voxels of the octree on one device: it needs --grid octree, and not --gpus N > 1 or --bench\n");
        return 2;
    }
    if (connectivity != 6 && connectivity != 26) { std::fprintf(stderr, "--connectivity must be 6 or 26\n"); return 2; }
    std::vector<int> devices;
    if (gpus > 1) {
        const int have = vx_device_count();
        if (!logical && gpus > have) { std::fprintf(stderr, "--gpus %d but %d device(s) visible (add --logical to rehearse on one)\n", gpus, have); return 2; }
        for (int k = 0; k < gpus; ++k) devices.push_back(logical ? 0 : k);
    }
    // --mesh: the triangle model (loadModel, hello_vulkan.cpp:197) and its BVH, freed when main returns
    MeshScene meshScene;
    std::unique_ptr<vx_mesh, vxdetail::MeshDeleter> meshModel;
    std::unique_ptr<vx_bvh, void (*)(vx_bvh*)> meshBvh(nullptr, vx_bvh_free);
    try {
        if (!meshFile.empty()) {
            vx_mesh* m = nullptr;
            vxdetail::check(vx_mesh_load_obj(meshFile.c_str(), &m));
            meshModel.reset(m);
            if (attributes) vxdetail::check(vx_mesh_load_textures(m));  // the map_Kd images (PPM / TGA; 1x1 magenta where that fails)
            vx_bvh* b = nullptr;
            vxdetail::check(vx_bvh_build(m, 0, nullptr, &b));
            meshBvh.reset(b);
            meshScene.bvh = b;
            meshScene.model = m;
            meshScene.attributes = attributes;
            meshScene.verts = vx_mesh_host_vertices(m);
            meshScene.idx = vx_mesh_host_indices(m);
            std::vector<vx_material> recs(vx_mesh_num_materials(m));
            if (!recs.empty()) vxdetail::check(vx_mesh_materials(m, recs.data(), recs.size()));
            for (const vx_material& r : recs) {
                MaterialObj o;
                o.ambient = vec3(r.ambient[0], r.ambient[1], r.ambient[2]);
                o.diffuse = vec3(r.diffuse[0], r.diffuse[1], r.diffuse[2]);
                o.specular = vec3(r.specular[0], r.specular[1], r.specular[2]);
                o.shininess = r.shininess;
                o.illum = r.illum;
                meshScene.materials.push_back(o);
            }
            meshScene.matIds = vx_mesh_host_material_ids(m);
            if (!instFile.empty()) {  // one instance per line: 12 floats, the row-major 3x4 object-to-world transform
                std::ifstream in(instFile);
                if (!in) { std::fprintf(stderr, "cannot read %s\n", instFile.c_str()); return 2; }
                std::string line;
                while (std::getline(in, line)) {
                    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
                    std::istringstream ls(line);
                    vx_instance ins{};
                    int k = 0;
                    while (k < 12 && ls >> ins.transform[k]) ++k;
                    if (k != 12) { std::fprintf(stderr, "%s: a line needs 12 floats (row-major 3x4)\n", instFile.c_str()); return 2; }
                    ins.blas = 0;
                    ins.mask = 0xFF;
                    meshScene.instances.push_back(ins);
                }
                if (meshScene.instances.empty()) { std::fprintf(stderr, "%s: no instances\n", instFile.c_str()); return 2; }
            }
            std::printf("[voxhip] mesh %s: %zu triangles in the BVH\n", meshFile.c_str(), (size_t)vx_bvh_num_triangles(b));
            if (!meshXrayFile.empty()) write_mesh_xray(b, meshXrayFile, rw, rh, cameraDump);
        }
        const MeshScene* msp = meshFile.empty() ? nullptr : &meshScene;
        if (benchRuns > 0) {
            if (grid == "octree") Benchmaker<VoxelGridBool, true>{std::filesystem::path(path), vs, (size_t)benchRuns};
            else if (grid == "vec") Benchmaker<VoxelGridVec>{std::filesystem::path(path), vs, (size_t)benchRuns};
            else if (grid == "aabbstruct") Benchmaker<VoxelGridAABBstruct>{std::filesystem::path(path), vs, (size_t)benchRuns};
            else Benchmaker<VoxelGridBool>{std::filesystem::path(path), vs, (size_t)benchRuns};
            return 0;
        }
        if (grid == "octree") {
            if (materials) { std::fprintf(stderr, "--materials is not available with --grid octree: the octree has no material ids\n"); return 2; }
            // the commented-out alternative in createAABB (hello_vulkan.cpp:690-697)
            const auto t0 = Clock::now();
            Octree tree{std::filesystem::path(path), vs};
            const auto t1 = Clock::now();
            std::printf("Total usage of the Octree is %zu\n", tree.getMemoryUsageBytes());
            std::printf("Voxel build took %lldms\n", (long long)std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count());
            const std::vector<Aabb> aabbs = tree.getAabbs();
            std::printf("[voxhip] octree: %zu AABBs\n", aabbs.size());
            dump(dumpFile, aabbs);
            if (!octreeXrayFile.empty()) write_octree_xray(tree.handle(), octreeXrayFile, rw, rh, cameraDump);
            if (!renderFile.empty()) {  // the same picture of the octree's list, traced on the tree itself
                RenderOpts ro;
                ro.cameraDump = cameraDump;
                ro.mesh = msp;
                if (frames > 0) { ro.frames = frames; return render_frames(nullptr, tree.handle(), renderFile, rw, rh, ro); }
                return render([o = tree.handle()](const vx_trace_args* a) { return vx_octree_trace_ex(o, a); }, renderFile, rw, rh, ro);
            }
            return 0;
        }
        const bool surfMat = materials && !surfaceFile.empty();  // (--materials reaches an aabbstruct grid only for its surface's ids)
        if (grid == "bool") return parallel ? run_grid<VoxelGridBool, true>(path, vs, dumpFile, "VoxelGridBool", renderFile, rw, rh, materials, matDump, cameraDump, devices, msp, frames, solid, sdfFile, surfaceFile, componentsFile, connectivity, xrayFile)
                                               : run_grid<VoxelGridBool, false>(path, vs, dumpFile, "VoxelGridBool", renderFile, rw, rh, materials, matDump, cameraDump, devices, msp, frames, solid, sdfFile, surfaceFile, componentsFile, connectivity, xrayFile);
        if (grid == "aabbstruct") return parallel ? run_grid<VoxelGridAABBstruct, true>(path, vs, dumpFile, "VoxelGridAABBstruct", "", rw, rh, surfMat, "", cameraDump, {}, nullptr, 0, solid, sdfFile, surfaceFile, componentsFile, connectivity, xrayFile)
                                                  : run_grid<VoxelGridAABBstruct, false>(path, vs, dumpFile, "VoxelGridAABBstruct", "", rw, rh, surfMat, "", cameraDump, {}, nullptr, 0, solid, sdfFile, surfaceFile, componentsFile, connectivity, xrayFile);
        if (grid == "vec") return parallel ? run_grid<VoxelGridVec, true>(path, vs, dumpFile, "VoxelGridVec", "", rw, rh, false, "", cameraDump, {}, nullptr, 0, solid, sdfFile, surfaceFile, componentsFile, connectivity, xrayFile)
                                           : run_grid<VoxelGridVec, false>(path, vs, dumpFile, "VoxelGridVec", "", rw, rh, false, "", cameraDump, {}, nullptr, 0, solid, sdfFile, surfaceFile, componentsFile, connectivity, xrayFile);
        std::fprintf(stderr, "unknown grid flavour %s\n", grid.c_str());
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
