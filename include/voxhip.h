/*
 * voxhip.h -- C ABI of libvoxhip.so: MI355X (gfx950) implementation of the reference's voxelizer hot path.
 *
 * The reference (MatBayern/Raytracing-Voxilizer-Vulkan-Intresection) has no FFI layer; its boundary for this
 * path is the C++ template API  VoxelBuilder<T>{path}.buildVoxelGrid(vs) -> T,  T::getAabbs(),  Octree{path,vs}
 * and the GLSL intersection shader raytrace.rint.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).  The C++ facade in
 * raytracing-voxilizer-vulkan-intresection_amd/cpp/ re-creates the reference classes on top of this ABI.
 *
 * Conventions
 *   - plain pointers and sizes only; handles are opaque; every function returns vx_status (VX_OK == 0) unless
 *     stated otherwise; vx_last_error() gives the message of the calling thread's last failure.
 *   - "host" pointers are ordinary memory, "dev" pointers are HIP device memory on the handle's device.
 *   - `stream` arguments are hipStream_t passed as void* (NULL = the default stream).
 *   - handles are not thread-safe; distinct handles may be used from distinct threads.
 *   - all compute runs in HIP kernels; there is no CPU fallback: without a usable device the compute entry
 *     points fail with VX_ERR_NO_DEVICE.
 *
 * Data contracts (identical to the reference)
 *   - occupancy bitmask: uint32 words, LSB first, voxel index i = x + X*(y + Y*z)          (voxelgrid.hpp:37-40,
 *     voxelgridBool.cpp:54-68)
 *   - vx_aabb: 6 x float32, tightly packed, 24 B                                           (shaders/host_device.h:117-121)
 *   - AABB list order: VX_GRID_BOOL / VX_GRID_AABBSTRUCT ascending voxel index, no duplicates;
 *     VX_GRID_VEC triangle-major then z,y,x with duplicates; octree ascending Morton code with duplicates.
 */
#ifndef VOXHIP_H
#define VOXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vx_status {
    VX_OK = 0,
    VX_ERR_INVALID_ARG = 1,
    VX_ERR_PATH = 2,          /* "Path does not exist!"                  VoxelBuilder.hpp:54-56, octTree.hpp:300-302 */
    VX_ERR_PARSE = 3,         /* "Colud not get valid reader! ..."       VoxelBuilder.hpp:63-65 */
    VX_ERR_OUT_OF_BOUNDS = 4, /* "Index out of bounds"                   voxelgrid.hpp:68-70, voxelgridBool.cpp:57-59 */
    VX_ERR_MORTON_BITS = 5,   /* "We support up to 21 bits per axis ..." octTree.hpp:583-585 */
    VX_ERR_NO_DEVICE = 6,
    VX_ERR_HIP = 7,
    VX_ERR_CAPACITY = 8,      /* caller buffer too small, or an internal 32-bit counter would overflow */
    VX_ERR_UNSUPPORTED = 9
} vx_status;

typedef struct vx_aabb { float minimum[3]; float maximum[3]; } vx_aabb; /* shaders/host_device.h:117-121 */

typedef enum vx_grid_kind {
    VX_GRID_BOOL = 0,       /* VoxelGridBool        voxelgridBool.{hpp,cpp} */
    VX_GRID_AABBSTRUCT = 1, /* VoxelGridAABBstruct  voxelgridAABBstruct.{hpp,cpp} */
    VX_GRID_VEC = 2         /* VoxelGridVec         voxelgridVecEncoding.{hpp,cpp} */
} vx_grid_kind;

/* MaterialObj (common/obj_loader.h:32-52) as VoxelBuilder copies it out of tinyobj::material_t (VoxelBuilder.hpp:383-394) */
typedef struct vx_material {
    float ambient[3], diffuse[3], specular[3], transmittance[3], emission[3];
    float shininess, ior, dissolve;
    int32_t illum;
    int32_t texture_id;
} vx_material;

typedef struct vx_mesh vx_mesh;     /* parsed OBJ: what VoxelBuilder keeps in m_attribs / m_shapes / m_materials */
typedef struct vx_grid vx_grid;     /* a VoxelGrid<T> */
typedef struct vx_octree vx_octree; /* an Octree */

typedef struct vx_grid_desc {
    uint64_t dim[3];     /* m_x, m_y, m_z                                             voxelgrid.hpp:19-21 */
    float voxel_size;    /* m_voxelSize */
    float origin[3];     /* m_org (== bbox min for built grids) */
    float bbox_min[3], bbox_max[3], bbox_center[3]; /* VoxelBuilder.hpp:198-224 (zero for vx_grid_create) */
    uint64_t num_words;  /* ceil(X*Y*Z/32) */
    uint64_t set_calls;  /* m_voxelSet: number of setVoxel calls (duplicates counted)  voxelgridBool.cpp:67 */
    uint64_t occupied;   /* distinct occupied voxels (popcount of the bitmask) */
    uint64_t triangles;  /* "Total triangles processed"                                VoxelBuilder.hpp:417 */
    int32_t kind;        /* vx_grid_kind */
    int32_t device;
} vx_grid_desc;

typedef struct vx_voxelize_opts {
    int32_t sat_variant;  /* 0: triBoxOverlap (serial driver, VoxelBuilder.hpp:118-162, inParaell=false);
                             1: triBoxOverlapSchwarzSeidel (threaded driver, :226-335, inParaell=true) */
    int32_t flags;        /* VX_VOXELIZE_* bits (0 = the reference as it runs today) */
    uint64_t word_begin;  /* multi-GPU shard: only bitmask words [word_begin, word_end) are written by this    */
    uint64_t word_end;    /* call (both 0 = whole grid).  Triangle range for VX_GRID_VEC shards:               */
    uint64_t tri_begin;   /* only triangles [tri_begin, tri_end) are voxelized (both 0 = all).                 */
    uint64_t tri_end;
    void* stream;         /* hipStream_t the grid's kernels run on */
    int32_t shard_rank;   /* word shard BY RANK: with shard_world > 1 (and word_begin == word_end == 0) the build derives            */
    int32_t shard_world;  /* [word_begin, word_end) = vx_shard_words(num_words, shard_rank, shard_world) from its own bounding-box   */
                          /* pass -- the caller need not know the grid's word count beforehand (0 or 1: whole grid)                 */
} vx_voxelize_opts;

/* vx_voxelize_opts.flags */
#define VX_VOXELIZE_MATERIALS 1 /* also fill the per-voxel material ids: setVoxel -> addMatrialIfNeeded, the plumbing the reference keeps
                                   commented out (VoxelBuilder.hpp:375-395, voxelgridBool.cpp:64, voxelgridAABBstruct.cpp:31,
                                   voxelgridVecEncoding.cpp:27).  A word / triangle shard leaves the ids PENDING: the index a material
                                   gets is the order of its first use over the WHOLE build, so the shards' first uses are combined
                                   first (vx_grid_material_first_use -> element-wise minimum over the shards ->
                                   vx_grid_finish_materials); an unsharded build finishes by itself. */
#define VX_VOXELIZE_LIST_ASYNC 2 /* VX_GRID_VEC (ignored with VX_VOXELIZE_MATERIALS): the build returns with the list's LENGTH known but
                                   without having queued the kernel that writes its records.  Nothing the library queues after a build --
                                   traversal structure, word prefix, ray batches -- reads the list, and a ray batch ends with a long drain
                                   in which most of the GPU idles: the next vx_trace* call on the grid queues the emission on a
                                   low-priority side stream of the handle, beside its ray kernel.  vx_grid_aabbs_device on the BOUND
                                   buffer (vx_grid_bind_aabbs_device) then returns the count at once; the records are complete for work
                                   queued on the grid's stream after vx_grid_list_wait(g).  Every other reader of the list in this API
                                   (host copies, copies into another buffer, re-binding, setVoxel, the next build, free) waits by
                                   itself; without a ray batch in between the emission runs on the grid's stream when first asked for. */
#define VX_VOXELIZE_SOLID 4     /* solid voxelization: the inside of closed surfaces is filled.  S = the surface bitmask the build gives without the
                                   flag (bit for bit); an empty cell is EXTERIOR when a path of empty, 6-connected (face-neighbour) cells joins it to an
                                   empty cell of the grid's boundary (x in {0, X-1}, y in {0, Y-1} or z in {0, Z-1}); H = the empty cells that are not
                                   exterior (= binary_fill_holes(S) minus S).  The build then behaves as if, after the triangle loop, setVoxel(x, y, z,
                                   MaterialObj{}) ran once per cell of H in ascending voxel index:
                                     dim, origin, bbox, triangles   unchanged;  bitmask S | H, occupied its popcount;  set_calls + |H|
                                     Bool / AABBstruct list         ascending voxel index over S | H
                                     Vec list                       the triangles' records (duplicates included), then one cell_aabb record per cell
                                                                    of H in ascending index; vx_grid_bytes 24 x that length; a bound buffer receives
                                                                    the whole list when it fits
                                     materials                      surface voxels / calls keep their ids; interior ones get MaterialObj{}'s, appended
                                                                    to the table when no triangle used it and H is not empty
                                   An open mesh (or a hole wider than the conservative surface closes) gives H = {}, a grid with an axis of 1 or 2
                                   cells too.  Integer bit operations only: bit-exact.  VX_VOXELIZE_LIST_ASYNC is ignored together with this flag.
                                   With a word shard (word_begin / word_end, shard_world > 1), a triangle range or in vx_multi_voxelize:
                                   VX_ERR_INVALID_ARG before anything is queued (the fill is global).  More than 2^32 interior cells: VX_ERR_CAPACITY. */

/* ---- library ------------------------------------------------------------------------------------------- */
const char* vx_last_error(void);
const char* vx_status_string(vx_status s);
int vx_device_count(void);           /* HIP devices visible (0 when there is none / no driver) */
vx_status vx_set_device(int device); /* device used by handles created afterwards on this thread */
vx_status vx_release_cached_memory(void); /* return the library's pooled device blocks to HIP */

/* ---- mesh: replaces VoxelBuilder::readObjFile (VoxelBuilder.hpp:51-70) / Octree::readObjFile (octTree.hpp:298-316) */
vx_status vx_mesh_load_obj(const char* path, vx_mesh** out);
vx_status vx_mesh_from_arrays(const float* host_xyz, size_t num_vertices, const int32_t* host_tri_indices,
                              size_t num_triangles, vx_mesh** out);
/* borrow arrays already resident in HBM (no copy; they must outlive the mesh) */
vx_status vx_mesh_from_device(const float* dev_xyz, size_t num_vertices, const int32_t* dev_tri_indices,
                              size_t num_triangles, vx_mesh** out);
size_t vx_mesh_num_vertices(const vx_mesh* m);
size_t vx_mesh_num_triangles(const vx_mesh* m);
/* host copies (NULL for vx_mesh_from_device meshes) */
const float* vx_mesh_host_vertices(const vx_mesh* m);
const int32_t* vx_mesh_host_indices(const vx_mesh* m);
/* materials: what tinyobj hands VoxelBuilder as GetMaterials() and shape.mesh.material_ids (VoxelBuilder.hpp:69,375-381):
 * the records of the OBJ's mtllib files in file order and one id per triangle (-1 = none).  vx_mesh_set_materials attaches
 * the same to a mesh built from arrays (ids are copied; pass NULL ids for "no face has a material"). */
size_t vx_mesh_num_materials(const vx_mesh* m);
vx_status vx_mesh_materials(const vx_mesh* m, vx_material* out, size_t capacity);
const int32_t* vx_mesh_host_material_ids(const vx_mesh* m); /* num_triangles entries; NULL when the mesh has no materials */
vx_status vx_mesh_set_materials(vx_mesh* m, const vx_material* materials, size_t num_materials, const int32_t* tri_material_ids);
/* Corner attributes and textures: what attribute shading of frames reads (vx_render_set_shading; common/obj_loader.cpp:49-121).  Positions,
 * the BVH and the voxelizer never read them.
 *   Corner k of triangle t sits at 3t + k in the mesh's index order (OBJ polygons fan as (0, k-1, k)): 3 f32 normal, 2 f32 uv.
 *   vx_mesh_load_obj reads `vt u v` and `vn x y z` and the v/vt, v//vn, v/vt/vn corners (negative = relative): uv = (u, 1 - v); a corner
 *   without vt gets (0, 0), without vn (0, 0, 0); a vt / vn index that is 0 or out of range leaves that attribute absent (never an error:
 *   positions, triangles, materials and errors are those of the same file without attributes).  The mesh has corner normals when the file
 *   has at least one vn line, corner uvs when it has at least one vt line.
 *   Textures: one slot per material with a map_Kd, in material order (the file is its last token, options skipped, relative to the MTL's
 *   directory).  vx_material.texture_id stays -1; the slot of each material is a separate array.  vx_mesh_load_obj reads no image:
 *   vx_mesh_load_textures decodes every slot's file -- binary PPM (P6, maxval 255) and TGA (types 2 and 10, 24 or 32 bpp, origin bits
 *   honoured) -> RGBA8, top row first -- and gives a missing, unreadable, truncated or unsupported file the reference's 1x1 (255, 0, 255, 255)
 *   (hello_vulkan.cpp:318-327).  A slot without an image is shaded as that 1x1 magenta. */
const float* vx_mesh_host_corner_normals(const vx_mesh* m);  /* 9 f32 per triangle; NULL when the mesh has none */
const float* vx_mesh_host_corner_uvs(const vx_mesh* m);      /* 6 f32 per triangle; NULL when the mesh has none */
/* copies num_triangles*9 normals / *6 uvs from host arrays (any kind of mesh); NULL removes that attribute */
vx_status vx_mesh_set_attributes(vx_mesh* m, const float* corner_normals, const float* corner_uvs);
size_t vx_mesh_num_textures(const vx_mesh* m);                          /* texture slots */
const char* vx_mesh_texture_name(const vx_mesh* m, size_t slot);        /* the slot's file ("" when set by vx_mesh_set_texture); NULL out of range */
/* the slot's RGBA8 image (width*height*4 bytes, top row first) and its size; NULL (size 0) when the slot has no image */
const uint8_t* vx_mesh_host_texture(const vx_mesh* m, size_t slot, uint32_t* width, uint32_t* height);
const int32_t* vx_mesh_host_material_textures(const vx_mesh* m);       /* num_materials slots (-1 none); NULL without materials */
vx_status vx_mesh_set_material_textures(vx_mesh* m, const int32_t* slots, size_t num_materials); /* num_materials must match; any int32 */
/* sets slot `slot` (0..65535; the slot list grows to it) to a width x height RGBA8 image (copied); width and height 1..16384, else
 * VX_ERR_INVALID_ARG */
vx_status vx_mesh_set_texture(vx_mesh* m, int32_t slot, uint32_t width, uint32_t height, const uint8_t* rgba8);
vx_status vx_mesh_load_textures(vx_mesh* m);
void vx_mesh_free(vx_mesh* m);

/* ---- geometry at its extremes: what every builder does with vertices that are not ordinary numbers ----------
 * 1. Non-finite vertices.  A coordinate is non-finite when it is NaN (either sign, any payload), +Inf or -Inf.
 *    - vx_voxelize, vx_voxelize_into, vx_voxelize_multi, vx_multi_voxelize and vx_octree_build take the bounding box over ALL vertices
 *      of the mesh, referenced by a triangle or not, as the reference does.  A mesh with any non-finite coordinate is refused with
 *      VX_ERR_INVALID_ARG and a message that contains "non-finite".  The error is found on the device, from the bounding box, so it is
 *      of vx_voxelize_into's second class: the grid handle is left EMPTY and the next successful build equals a fresh one.
 *    - vx_bvh_build and vx_bvh_build_into refuse a mesh in which a vertex that some triangle REFERENCES has a non-finite coordinate:
 *      VX_ERR_INVALID_ARG, "non-finite"; host meshes and borrowed device meshes alike, found beside the index check.  A failed
 *      vx_bvh_build_into leaves the empty BVH.  Unreferenced vertices play no part in a BVH.
 * 2. Finite vertices of any magnitude are ordinary input and every contract holds as written: an outlying vertex at 2^100, vertices at
 *    +-FLT_MAX/2 whose extent overflows to +Inf.  The voxelizer refuses the latter with VX_ERR_CAPACITY and the octree with
 *    VX_ERR_MORTON_BITS (the extent divided by the voxel size is above 2^21); BVH and TLAS queries stay bit-equal to the brute force over
 *    all triangles, those that reach to the outlier included.  An instance whose world box overflows float32 is bounded by the whole
 *    space in the TLAS and is entered by every ray.
 * 3. Scale.  For the mesh times 2^k with the voxel size times 2^k the voxelizer is bit-identical to the reference on that same scaled
 *    input for every k at which no intermediate of the triangle/box test overflows -- downwards through gradual underflow, where the
 *    reference's own result changes with k (subnormal products, the 1e-8 thresholds of sat_variant 1).  Beyond that, once a product of
 *    the test is Inf and a NaN follows (from about 2^42 times a unit-sized mesh on), the result is unspecified.
 * 4. OBJ numerals (vx_mesh_load_obj: v, vt, vn and the reals of the MTL).  A numeral whose magnitude overflows double reads as +-Inf,
 *    one that underflows as +-0; a double beyond float's range converts to +-Inf (no undefined cast); `nan`, `inf` and their signed
 *    forms read as written; nothing consults the C locale.  Such a file LOADS; the builders then apply rule 1. */

/* ---- voxelize: replaces VoxelBuilder<T,inParaell>::buildVoxelGrid (VoxelBuilder.hpp:338-542) ---------------
 * Limits (the reference has none besides memory): at most 2^21 cells per axis, 2^21 itself included -- the bound the reference's
 * own Octree has (octTree.hpp:583-585); the per-triangle candidate ranges are 16 + 16 bits in the triangle record plus 5 + 6 high
 * bits (start, count) in an extension word read only by grids with an axis above 65535 cells, so a triangle may span a whole
 * 2^21-cell axis -- and 2^37 cells in total.  Beyond either vx_voxelize fails with VX_ERR_CAPACITY, vx_octree_build with
 * VX_ERR_MORTON_BITS and the reference's message.  Rays (vx_trace*) work on every grid the
 * builds accept (grids with an axis above 65535 cells are walked by variants of the ray kernel that keep 32-bit cell coordinates). */
vx_status vx_voxelize(const vx_mesh* mesh, float voxel_size, vx_grid_kind kind, const vx_voxelize_opts* opts /*NULL ok*/,
                      vx_grid** out);
/* same, re-using an existing grid handle's device buffers (steady-state loops; no allocation when sizes repeat).
 * A failed vx_voxelize_into leaves the grid in one of two defined states:
 *  - errors found from the arguments alone (a NULL mesh or grid, a voxel size that is not finite and positive, a mesh on another
 *    device, sat_variant, shard_rank / shard_world, a triangle range past the mesh, word_begin > word_end) or in the mesh itself
 *    (with VX_VOXELIZE_MATERIALS, more than 32767 distinct materials; a failed upload of the mesh): nothing has been queued on the
 *    grid and it still holds its previous build, unchanged through every reader;
 *  - every other error (a non-finite vertex coordinate, an axis above 2^21 cells, more than 2^37 cells, word_end past the new grid's word count, a counter
 *    overflow, a HIP error during the build): the grid is EMPTY -- 0 x 0 x 0 cells, no words, 0 occupied voxels and setVoxel calls, an empty list
 *    (a VX_VOXELIZE_LIST_ASYNC list of the previous build that was never written is dropped; a bound buffer holds 0 records), no
 *    materials, and every ray misses.
 * In both cases the next successful build on the handle gives what a build on a fresh handle gives. */
vx_status vx_voxelize_into(const vx_mesh* mesh, float voxel_size, const vx_voxelize_opts* opts, vx_grid* grid);

/* ---- the same build spread over several GPUs of one process (the call site on a multi-GPU node: hello_vulkan.cpp:677-683).
 * Device k of `devices` voxelizes the bitmask words vx_shard_words(num_words, k, num_devices) of the SAME grid -- contributions are
 * word-disjoint, so their OR is their concatenation -- and the shards travel over xGMI as peer copies (hipMemcpyPeerAsync: one
 * slab per peer link, no collective library needed inside one process; the one-process-per-GPU form of the same exchange is the
 * RCCL all-gather in vx_dist.py).  all_gather = 0: *out_grids receives ONE grid, on devices[0], holding the complete bitmask;
 * all_gather = 1: out_grids[k] receives a complete grid on devices[k] for every k (rays can then be split over the devices).
 * A device may appear more than once in `devices` (logical ranks: rehearsal on a box with fewer GPUs).  VX_GRID_BOOL and
 * VX_GRID_AABBSTRUCT only: VX_GRID_VEC's list order needs triangle shards (vx_voxelize_opts.tri_begin/tri_end). */
vx_status vx_voxelize_multi(const vx_mesh* mesh, float voxel_size, vx_grid_kind kind, int sat_variant, const int* devices, int num_devices, int all_gather,
                            vx_grid** out_grids);
/* The same as a STEADY-STATE entry: vx_multi_create uploads the mesh to every listed device once and starts one worker thread and
 * one grid handle per rank; every vx_multi_voxelize then rebuilds the grid (any voxel size) with no upload, no thread start and --
 * when sizes repeat -- no allocation: each rank derives its word shard from its own bounding-box pass (vx_voxelize_opts.shard_rank /
 * shard_world), the shards are exchanged as peer copies, the destination grids (rank 0, or every rank with all_gather) refresh word
 * prefix and traversal structure.  opts: sat_variant, flags (VX_VOXELIZE_MATERIALS: the shards' first uses are combined and the ids
 * gathered in shard order, see vx_grid_finish_materials) and stream are honoured; the shard fields must be 0.
 * vx_multi_grid: the context's grid of rank k (owned by the context, valid until the next vx_multi_voxelize / vx_multi_free);
 * vx_multi_release_grid hands it to the caller (vx_grid_free), the context then no longer rebuilds that rank. */
typedef struct vx_multi vx_multi;
vx_status vx_multi_create(const vx_mesh* mesh, const int* devices, int num_devices, vx_grid_kind kind, vx_multi** out);
vx_status vx_multi_voxelize(vx_multi* m, float voxel_size, const vx_voxelize_opts* opts /*NULL ok*/, int all_gather);
vx_grid* vx_multi_grid(vx_multi* m, int rank);
vx_grid* vx_multi_release_grid(vx_multi* m, int rank);
void vx_multi_free(vx_multi* m);

/* Materials of a SHARDED build (VX_VOXELIZE_MATERIALS with a word or triangle shard).  addMatrialIfNeeded (voxelgrid.hpp:102-114)
 * numbers materials in the order of their first setVoxel call over the whole build; a shard only sees its own calls.
 * vx_grid_material_first_use: per material VALUE of the mesh (value 0 = MaterialObj{}, then the mesh's records de-duplicated by
 * operator==, in record order) the index of the first triangle that carries it into a setVoxel call of this shard, -1 = none.
 * vx_grid_finish_materials: given the element-wise minimum of those arrays over all shards (-1 = unused everywhere) the grid fills
 * getMatrials() and the ids of ITS voxels / calls (ascending voxel order resp. call order: the shards' id arrays concatenated in
 * shard order are the unsharded build's).  Also callable on an unsharded build (a no-op: it has finished by itself). */
vx_status vx_grid_material_first_use(const vx_grid* g, int64_t* out, uint64_t capacity, uint64_t* count);
vx_status vx_grid_finish_materials(vx_grid* g, const int64_t* first_use_min, uint64_t count);

/* ---- grid: replaces VoxelGrid<T> and its three subclasses ------------------------------------------------ */
/* VoxelGrid ctor (voxelgrid.hpp:52-62): an empty grid of x*y*z voxels */
vx_status vx_grid_create(vx_grid_kind kind, uint64_t x, uint64_t y, uint64_t z, float voxel_size, const float origin[3],
                         void* stream, vx_grid** out);
vx_status vx_grid_describe(const vx_grid* g, vx_grid_desc* out);
/* setVoxel (voxelgridBool.cpp:54-68, voxelgridAABBstruct.cpp:23-47, voxelgridVecEncoding.cpp:19-39) */
vx_status vx_grid_set_voxel(vx_grid* g, uint64_t x, uint64_t y, uint64_t z);
/* occupancy test of one voxel (the reference's VoxelGrid::getVoxel is broken for the Bool grid, voxelgrid.hpp:66-72) */
vx_status vx_grid_test_voxel(const vx_grid* g, uint64_t x, uint64_t y, uint64_t z, int* occupied);
/* getCorrds (voxelgrid.hpp:91-100) */
vx_status vx_grid_coords(const vx_grid* g, uint64_t x, uint64_t y, uint64_t z, float out_xyz[3]);
/* getMemoryUsageBytes (voxelgrid.hpp:115-122): Bool 4*ceil(N/32); AABBstruct 28*N; Vec 24*set_calls */
uint64_t vx_grid_bytes(const vx_grid* g);
/* bitmask access */
vx_status vx_grid_bitmask(const vx_grid* g, uint32_t* host_words, uint64_t capacity_words);
const uint32_t* vx_grid_bitmask_device(const vx_grid* g);
/* for the multi-GPU exchange; call vx_grid_refresh afterwards.  Bits past X*Y*Z in the last word are not cells: a writer may set them
 * (a fill of the whole word array, for example), and vx_grid_refresh clears them, so that occupied, the AABB lists and the rays see
 * exactly the X*Y*Z cells. */
uint32_t* vx_grid_bitmask_device_mut(vx_grid* g);
vx_status vx_grid_refresh(vx_grid* g);            /* recount + rebuild derived data after the bitmask was written externally */
/* The fill of VX_VOXELIZE_SOLID on any grid (vx_grid_create + setVoxel, a mask written through vx_grid_bitmask_device_mut): exactly
 * vx_grid_set_voxel on every cell of the grid's interior H in ascending voxel index -- set_calls + |H|, a Vec list gets the records
 * appended (in the grid's own storage), materials are dropped when H is not empty -- then the derived data is refreshed. */
vx_status vx_grid_fill_interior(vx_grid* g);
/* |H| of the last VX_VOXELIZE_SOLID build or vx_grid_fill_interior on the handle; 0 after any other build and for a new grid */
vx_status vx_grid_interior(const vx_grid* g, uint64_t* count);
/* diagnostics: the flood-fill rounds that fill took, the final quiet round included (0: no fill, or a grid with an axis below 3 cells) */
uint32_t vx_grid_fill_rounds(const vx_grid* g);
/* Exact Euclidean distance fields of the bitmask.  A cell is c = (x, y, z); outputs hold one value per cell at x + X*(y + Y*z).  M = the
 * occupied cells of the bitmask as it stands when the call is queued (after the last build, setVoxel, fill_interior, or an external write
 * followed by vx_grid_refresh).  Only cells of the grid count: nothing outside it is empty or occupied.
 *   flags 0                D_out(c) = min over o in M of (cx-ox)^2 + (cy-oy)^2 + (cz-oz)^2, in cell units, exact: 0 on M;
 *                          0xFFFFFFFF everywhere when M is empty
 *   VX_DISTANCE_INSIDE     D_in(c) = the same minimum over the empty cells of the grid: 0 off M; 0xFFFFFFFF everywhere when every cell is
 *                          occupied
 *   vx_grid_sdf*           s(c) = vs * sqrtf((float)D_out(c)) off M, -(vs * sqrtf((float)D_in(c))) on M (vs = the voxel size; (float) rounds
 *                          to nearest even, sqrtf and * are correctly rounded f32); the sentinel gives +inf / -inf; no cell is 0.  Bit for
 *                          bit the float32 evaluation of that formula.
 * A grid with (X-1)^2 + (Y-1)^2 + (Z-1)^2 > 0xFFFFFFFE fails with VX_ERR_CAPACITY before anything is queued (65536 x 2 x 2 is accepted,
 * 65537 x 1 x 1 is not).  A NULL grid or buffer or unknown flag bits: VX_ERR_INVALID_ARG; capacity (in values) < X*Y*Z: VX_ERR_CAPACITY;
 * every failure writes nothing.  A grid of 0 cells (e.g. after a failed build): VX_OK, nothing written.
 * The _device variants queue on the grid's stream (the one its builds and ray batches use) and return without a host wait; the host variants
 * return once host_out is written.  Nothing a reader of the grid can see changes (bitmask, counts, lists, materials; a pending
 * VX_VOXELIZE_LIST_ASYNC emission is neither forced nor dropped; a bound list buffer is untouched).  Scratch comes from the library's pool:
 * a repeated call at the same dimensions allocates nothing. */
#define VX_DISTANCE_INSIDE 1
vx_status vx_grid_distance_sq_device(const vx_grid* g, uint32_t flags, uint32_t* dev_out, uint64_t capacity);
vx_status vx_grid_distance_sq(const vx_grid* g, uint32_t flags, uint32_t* host_out, uint64_t capacity);
vx_status vx_grid_sdf_device(const vx_grid* g, float* dev_out, uint64_t capacity);
vx_status vx_grid_sdf(const vx_grid* g, float* host_out, uint64_t capacity);
/* The feature transform: WHICH cell the distance fields' minimum belongs to.  i(c) = x + X*(y + Y*z) is the index of cell c; T is the target
 * set of vx_grid_distance_sq with the same flags (flags 0: the occupied cells M of the bitmask as it stands when the call is queued;
 * VX_DISTANCE_INSIDE: the empty cells of the grid).
 *   N(c) = min { i(o) : o in T, |c - o|^2 = min over p in T of |c - p|^2 }
 * -- the nearest target cell, and among several at the same exact squared distance the one of the smallest index (the smallest z, then the
 * smallest y, then the smallest x).  N(c) = i(c) on T; N(c) = 0xFFFFFFFF everywhere when T is empty.  One uint32 per cell at i(c).  The
 * squared distance is not returned: it is |c - N(c)|^2 and equals vx_grid_distance_sq(flags) on every cell.
 *   vx_grid_nearest_gather*   out[i(c)] = values[N(c)], `fill` where N(c) is the sentinel: values holds one uint32 per cell (nvalues of them).
 * Checks, in this order, every one before anything is queued, every failure writing nothing:
 *   1. a NULL grid or buffer: VX_ERR_INVALID_ARG
 *   2. unknown flag bits: VX_ERR_INVALID_ARG
 *   3. gather: nvalues < X*Y*Z, or values == out: VX_ERR_INVALID_ARG
 *   4. a grid of 0 cells (e.g. after a failed build): VX_OK, nothing written
 *   5. capacity (in values) < X*Y*Z: VX_ERR_CAPACITY
 *   6. the distance fields' limit, (X-1)^2 + (Y-1)^2 + (Z-1)^2 > 0xFFFFFFFE: VX_ERR_CAPACITY
 *   7. more than 0xFFFFFFFF cells (the last index would collide with the sentinel): VX_ERR_CAPACITY
 * (the distance fields run 1, 2, 4, 6, 5: the status of every call is the same either way.)  Everything else follows the distance fields'
 * rules: the calls only read the bitmask, nothing a reader of the grid can see changes, a pending VX_VOXELIZE_LIST_ASYNC emission stays
 * pending; the _device variants queue on the grid's stream and return without a host wait (values and out are device pointers), the host
 * variants return once host_out is written; scratch stays on the handle, so a repeated call at the same dimensions allocates nothing. */
vx_status vx_grid_nearest_device(const vx_grid* g, uint32_t flags, uint32_t* dev_out, uint64_t capacity);
vx_status vx_grid_nearest(const vx_grid* g, uint32_t flags, uint32_t* host_out, uint64_t capacity);
vx_status vx_grid_nearest_gather_device(const vx_grid* g, uint32_t flags, const uint32_t* dev_values, uint64_t nvalues, uint32_t fill,
                                        uint32_t* dev_out, uint64_t capacity);
vx_status vx_grid_nearest_gather(const vx_grid* g, uint32_t flags, const uint32_t* host_values, uint64_t nvalues, uint32_t fill,
                                 uint32_t* host_out, uint64_t capacity);
/* Binary morphology of the bitmask with the digital Euclidean ball (scipy.ndimage.binary_dilation / _erosion / _opening / _closing).
 * M = the occupied cells of the bitmask as it stands when the call is queued (after the last build, setVoxel, fill_interior, or an external
 * write followed by vx_grid_refresh).  radius_sq = r2 is a squared radius in cells, R = floor(sqrt(r2)), and the structuring element is
 *   B(r2) = {b in Z^3 : bx^2 + by^2 + bz^2 <= r2}:  B(0) the single cell, B(1) the 6-, B(2) the 18-, B(3) the 26-neighbourhood.
 * ONE rule for the border: every operation is the operation on the infinite lattice Z^3, in which every cell outside the grid is empty,
 * and its result is restricted to the grid.  There are no border flags.  c ranges over the cells of the grid:
 *   VX_MORPH_DILATE   {c : some b in B has c + b in M}  =  {c : D_out(c) <= r2}
 *   VX_MORPH_ERODE    {c : every b in B has c + b in M}  =  {c : D_in(c) > r2, and R <= x <= X-1-R, the same for y and z}: a cell nearer
 *                     than R to the border always loses, since B holds (+-R, 0, 0), (0, +-R, 0), (0, 0, +-R)
 *                     (= binary_erosion(M, B, border_value=0))
 *   VX_MORPH_OPEN     the dilation of the erosion; a subset of M
 *   VX_MORPH_CLOSE    {c : every b in B has c + b in D}, D = the dilation of M on Z^3 WITHOUT restriction (cells outside the grid included):
 *                     pad M with R empty cells on every side, dilate, erode, crop.  Extensive (M is a subset) and idempotent;
 *                     binary_closing on the unpadded array is neither at the border.
 * A plain CLOSE does not seal a hole in a thin wall -- the cap of a ball inside the hole pokes through the wall, so the hole's cells
 * survive the erosion.  vx_grid_seal is for that:
 *   seal(M, r2) = M | crop(erode(fill(dilate(pad(M, R + 1))))): pad with R + 1 empty cells on every side (the dilated body is then
 *                     surrounded by an empty shell), dilate, fill the interior exactly as VX_VOXELIZE_SOLID defines it
 *                     (binary_fill_holes) on the padded grid, erode, crop, OR with M.  r2 = 0 is M | H, the plain solid grid.
 * Integer bit operations only: every result is bit-exact.  R <= vx_morph_bit_radius() runs on mask words, 32 cells at a time; larger radii
 * threshold the distance fields above (and inherit their cost and their limit).
 * The mask variants return the result as a bitmask in the grid's own word layout (num_words words, padding bits past X*Y*Z zero) and follow
 * the distance fields' rules: they only read the bitmask; nothing a reader of g can see changes; a pending VX_VOXELIZE_LIST_ASYNC emission
 * is neither forced nor dropped; scratch stays on the handle, so a repeated call at the same dimensions and radius allocates nothing;
 * _device queues on the grid's stream and returns without a host wait.  Checks, in this order, every failure writing nothing:
 *   1. a NULL grid or buffer, an op above 3, radius_sq = 0xFFFFFFFF, or a dev_words range that overlaps the grid's own mask:
 *      VX_ERR_INVALID_ARG;
 *   2. a grid of 0 cells: VX_OK, nothing written;
 *   3. a working domain (the grid; for CLOSE the grid padded by R, for seal by R + 1) of more than 2^21 cells on an axis or more than
 *      2^37 cells, or, on the distance-field path, beyond the distance fields' limit on (X-1)^2 + (Y-1)^2 + (Z-1)^2: VX_ERR_CAPACITY
 *      before anything is queued;
 *   4. capacity_words < num_words: VX_ERR_CAPACITY.
 * The grid variants return a NEW handle with the kind, dimensions, voxel size, origin, device and stream of src, src's bbox fields and
 * triangles = 0; everything else is as if vx_grid_create were followed by vx_grid_set_voxel on every result cell in ascending voxel index:
 * set_calls = occupied = the popcount, Bool / AABBstruct lists ascend by voxel index, a Vec list holds one cell_aabb record per cell in
 * ascending index (vx_grid_bytes 24 x that), no materials.  Rays, frames, surface, components, distance fields, fill_interior and morph work
 * on it like on any grid.  vx_grid_interior(out) is 0 after vx_grid_morph and the number of cells the seal added to M after vx_grid_seal.
 * src is unchanged (bitmask, list, counts), also when it was built with VX_VOXELIZE_LIST_ASYNC. */
#define VX_MORPH_DILATE 0u
#define VX_MORPH_ERODE  1u
#define VX_MORPH_OPEN   2u
#define VX_MORPH_CLOSE  3u
vx_status vx_grid_morph_device(const vx_grid* g, uint32_t op, uint32_t radius_sq, uint32_t* dev_words, uint64_t capacity_words);
vx_status vx_grid_morph_mask(const vx_grid* g, uint32_t op, uint32_t radius_sq, uint32_t* host_words, uint64_t capacity_words);
vx_status vx_grid_morph(const vx_grid* src, uint32_t op, uint32_t radius_sq, vx_grid** out);
vx_status vx_grid_seal(const vx_grid* src, uint32_t radius_sq, vx_grid** out);
uint32_t vx_morph_bit_radius(void); /* the largest R the bit-level path takes; above it the distance-field path runs */
/* The boundary mesh of the bitmask M (as it stands when the call is queued, as for the distance fields).  Cell c = (x, y, z) in M has a face
 * in direction d = 0..5 (-X, +X, -Y, +Y, -Z, +Z) when c + e_d is outside the grid or not in M.  Lattice points (i, j, k), 0 <= i <= X,
 * 0 <= j <= Y, 0 <= k <= Z, index i + (X+1)*(j + (Y+1)*k), lie per axis at org + ((float)i + 0.5f)*vs - half (f32, no contraction: the minimum
 * corner of cell i's AABB, continued to i = X).  Vertices: the lattice points some face touches (equivalently: the 2x2x2 cells around them
 * are mixed), in ascending lattice index.  Triangles: faces in ascending cell index, then ascending d; each gives (c0, c1, c2), (c0, c2, c3)
 * with c0..c3 the points (x+dx, y+dy, z+dz), dx dy dz =
 *   -X 000 001 011 010   +X 100 110 111 101   -Y 000 100 101 001   +Y 010 011 111 110   -Z 000 010 110 100   +Z 001 101 111 011
 * (counter-clockwise seen from the empty side).  mat (optional): per triangle the cell's entry of vx_grid_material_ids, a VX_GRID_BOOL /
 * VX_GRID_AABBSTRUCT grid built with VX_VOXELIZE_MATERIALS only (VX_GRID_VEC: VX_ERR_UNSUPPORTED; any other grid: VX_ERR_INVALID_ARG).
 * Capacities in vertices (3 f32 each) and triangles (3 int32 each; mat: 1 int32 each).  Both capacities 0 = size query (buffers may be
 * NULL).  Either capacity short: VX_ERR_CAPACITY, counts reported, nothing written.  V or T above 2^31 - 1: VX_ERR_CAPACITY, counts
 * reported, nothing written.  A NULL grid or buffer: VX_ERR_INVALID_ARG.  A grid of 0 cells: VX_OK, V = T = 0.
 * The _device variant waits on the host for the two counts only and queues the emission on the grid's stream; the host variant returns once
 * the buffers are written.  No side effects, as for the distance fields; scratch stays on the handle. */
vx_status vx_grid_surface_device(const vx_grid* g, float* dev_xyz, uint64_t vertex_capacity, int32_t* dev_tri, uint64_t triangle_capacity,
                                 int32_t* dev_mat, uint64_t* num_vertices, uint64_t* num_triangles);
vx_status vx_grid_surface(const vx_grid* g, float* host_xyz, uint64_t vertex_capacity, int32_t* host_tri, uint64_t triangle_capacity,
                          int32_t* host_mat, uint64_t* num_vertices, uint64_t* num_triangles);
/* a mesh that owns its arrays, equal in everything observable to vx_mesh_from_arrays(the vx_grid_surface arrays) followed, with
 * with_materials, by vx_mesh_set_materials(vx_grid_materials records, the triangle ids); usable by vx_bvh_*, vx_render_*, vx_voxelize */
vx_status vx_grid_surface_mesh(const vx_grid* g, int with_materials, vx_mesh** out);
/* Surface nets: the mesh of vx_grid_surface with relaxed vertex positions and, optionally, vertex normals.  M, the lattice points, their
 * index and order, the faces, tri and mat are those of vx_grid_surface, word for word; a cell outside the grid is empty.  All float32, no
 * contraction; / and sqrtf correctly rounded.
 * Initial offset.  Vertex v is lattice point p = (i, j, k).  Its block is the eight cells (i-1+a, j-1+b, k-1+e), a, b, e in {0, 1}.  Each of
 * the block's twelve edges joins two cells that differ in one axis A; an edge crosses when exactly one of its two cells is in M.  n = the
 * number of crossing edges (3..12 for every vertex).  T_x = the sum, over crossing edges NOT along x, of (2a - 1), a the edge's x bit; T_y,
 * T_z likewise.  The offset in cells from p, per axis: u0 = (float)T / (float)(2*n), in [-1/3, 1/3].
 * Neighbours.  Directions in the order -X, +X, -Y, +Y, -Z, +Z.  q = p +- e_A is a neighbour when q is a lattice point of the grid and the
 * four cells around lattice edge pq are neither all in M nor all out; q is then always a vertex.  m = the number of neighbours (>= 3).
 * One step with weight w (Jacobi: every vertex reads the previous field).  s = (+0, +0, +0); for each neighbour q in direction d, in
 * direction order, s = s + r with r = u_q, except on d's axis, where r = (+-1.0f) + u_q.  mean = s / (float)m.  t = u + w*(mean - u),
 * evaluated as written.  u' = fminf(fmaxf(t, -0.5f), 0.5f) per axis (the vertex stays in its dual cube).
 * Parameters.  One iteration is a step with lambda, then a step with mu if mu != 0.  iterations <= 1024, lambda finite in [0, 1], mu finite
 * in [-1, 0]; anything else is VX_ERR_INVALID_ARG.  iterations = 0 gives u0.
 * World position, per axis: org + (((float)i + 0.5f) + u)*vs - half.  With u = +0 this is vx_grid_surface's position, bit for bit.
 * Normals (optional, 3 f32 per vertex), from the final world positions P.  Over the block's twelve internal faces in this order: axis
 * A = x, y, z, then the other two bits (b, e) = 00, 10, 01, 11 with the first of the other two axes fastest.  A face counts when its two
 * cells differ; it is then the face (c, d) of its occupied cell, corners c0..c3 from vx_grid_surface's table.  a = P(c2) - P(c0),
 * b = P(c3) - P(c1); N += (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), every product and difference rounded, N from +0.
 * l = sqrtf((N.x*N.x + N.y*N.y) + N.z*N.z); the normal is N/l per component when l > 0 and finite, else (0, 0, 0).
 * The size query, the capacity rule, the 2^31 - 1 limit, the NULL checks, the 0-cell grid, materials and "no side effects" are those of
 * vx_grid_surface; dev_mat and dev_normals may be NULL.  Order of checks: NULL arguments and a bad vx_smooth first, then everything else as
 * vx_grid_surface does.  Every failure writes nothing.  The _device variant waits on the host for V and T only; everything else, all
 * iterations included, is queued back to back on the grid's stream.  Scratch stays on the handle. */
typedef struct vx_smooth { uint32_t iterations; float lambda; float mu; } vx_smooth;
vx_status vx_grid_surface_smooth_device(const vx_grid* g, const vx_smooth* params, float* dev_xyz, uint64_t vertex_capacity, int32_t* dev_tri,
                                        uint64_t triangle_capacity, int32_t* dev_mat, float* dev_normals, uint64_t* num_vertices,
                                        uint64_t* num_triangles);
vx_status vx_grid_surface_smooth(const vx_grid* g, const vx_smooth* params, float* host_xyz, uint64_t vertex_capacity, int32_t* host_tri,
                                 uint64_t triangle_capacity, int32_t* host_mat, float* host_normals, uint64_t* num_vertices,
                                 uint64_t* num_triangles);
/* as vx_grid_surface_mesh; with_normals: vx_mesh_set_attributes with the three vertex normals of each triangle's corners, so that
 * VX_RENDER_ATTRIBUTES frames shade the mesh smoothly */
vx_status vx_grid_surface_smooth_mesh(const vx_grid* g, const vx_smooth* params, int with_materials, int with_normals, vx_mesh** out);
/* Connected components of the bitmask M (as it stands when the call is queued, as for the distance fields).  Two cells of M are adjacent
 * under VX_CONNECT_6 when they share a face, under VX_CONNECT_26 when they share a face, an edge or a corner; only cells of the grid count
 * (nothing wraps, no padding).  A component is a maximal set of cells of M that adjacency joins.  Labels: one uint32 per cell at
 * x + X*(y + Y*z); 0 for empty cells, 1..K for cells of M, the components numbered in ascending order of their smallest cell index (exactly
 * scipy.ndimage.label(cells[Z, Y, X], generate_binary_structure(3, 1 or 3))).  vx_component record k - 1 describes label k: its cell
 * count and its inclusive cell-coordinate bounds, x, y, z.
 * Checks, in this order; every failure writes nothing: a NULL grid or buffer, or a connectivity other than 6 or 26: VX_ERR_INVALID_ARG; a
 * grid of 0 cells: VX_OK, K = 0; X*Y*Z > 2^32 - 1: VX_ERR_CAPACITY before anything is queued (32-bit labels and union-find indices: 1024^3
 * is accepted, 2048 x 2048 x 1024 is not); label capacity < X*Y*Z or stats capacity < K: VX_ERR_CAPACITY, the count still reported where
 * the signature has one.  vx_grid_components: host_labels NULL with capacity 0 = K only.  vx_grid_component_stats: capacity 0 = size
 * query.  The _device variant queues on the grid's stream and returns without a host wait (dev_count: NULL, or K as one uint32 on the
 * device); the host variants return once their outputs are written.  No side effects, as for the distance fields; scratch stays on the
 * handle (the parent array of the union-find is the label buffer itself). */
#define VX_CONNECT_6 6u
#define VX_CONNECT_26 26u
typedef struct vx_component { uint64_t cells; uint32_t min[3]; uint32_t max[3]; } vx_component;
#ifdef __cplusplus
static_assert(sizeof(vx_component) == 32, "vx_component is 32 bytes");
#else
_Static_assert(sizeof(vx_component) == 32, "vx_component is 32 bytes");
#endif
vx_status vx_grid_components_device(const vx_grid* g, uint32_t connectivity, uint32_t* dev_labels, uint64_t capacity, uint32_t* dev_count);
vx_status vx_grid_components(const vx_grid* g, uint32_t connectivity, uint32_t* host_labels, uint64_t capacity, uint64_t* count);
vx_status vx_grid_component_stats(const vx_grid* g, uint32_t connectivity, vx_component* host_out, uint64_t capacity, uint64_t* count);
/* getAabbs (voxelgridBool.cpp:18-52, voxelgridAABBstruct.cpp:10-22, voxelgridVecEncoding.cpp:15-18).
 * *count receives the list length; at most `capacity` entries are written (capacity 0 = size query). */
vx_status vx_grid_aabbs(const vx_grid* g, vx_aabb* host_out, uint64_t capacity, uint64_t* count);
vx_status vx_grid_aabbs_device(const vx_grid* g, vx_aabb* dev_out, uint64_t capacity, uint64_t* count);
/* VX_GRID_VEC: hand the grid the device buffer its list should be built IN (VoxelGridVec::getAabbs returns a copy of m_voxel,
 * voxelgridVecEncoding.cpp:15-18; a caller that wants the list in its own HBM buffer saves that copy).  Later vx_voxelize_into
 * calls emit straight into dev_out when the list fits `capacity` entries (otherwise into the grid's own storage, as without a
 * binding), and vx_grid_aabbs_device(g, dev_out, ...) then has nothing left to copy.  The buffer must outlive the binding;
 * dev_out NULL / capacity 0 removes it.  No effect on the other flavours (their lists are emitted by vx_grid_aabbs_device). */
vx_status vx_grid_bind_aabbs_device(vx_grid* g, vx_aabb* dev_out, uint64_t capacity);
/* VX_VOXELIZE_LIST_ASYNC builds: makes the grid's stream wait for the list (queues the emission there if no ray batch has taken it
 * along yet).  Does not block the host.  A no-op for every other build. */
vx_status vx_grid_list_wait(vx_grid* g);
/* vx_grid_aabbs_device for the Bool / AABBstruct flavours with the same deferral: the word prefix is queued and *count returned as usual,
 * the kernel that writes the records into dev_out is left to the next vx_trace* call on the grid (low-priority side stream, beside its ray
 * kernel) -- or to vx_grid_list_wait / the next build / any call that changes or reads what it needs, which queue it on the grid's stream.
 * dev_out must stay valid until then.  VX_GRID_VEC: same as vx_grid_aabbs_device. */
vx_status vx_grid_aabbs_device_async(const vx_grid* g, vx_aabb* dev_out, uint64_t capacity, uint64_t* count);
/* getMatrials() / getMatIdx() (voxelgrid.hpp:74-89) of a grid built with VX_VOXELIZE_MATERIALS:
 *   materials     the distinct MaterialObj values in the order addMatrialIfNeeded first met them (equality = MaterialObj::operator==,
 *                 obj_loader.h:45-51: every field except ior and dissolve; a face without usemtl carries MaterialObj{});
 *   material ids  the entries >= 0 of m_matIdx in index order: for VX_GRID_BOOL / VX_GRID_AABBSTRUCT one int16 per occupied voxel in
 *                 ascending voxel order (entry i belongs to box i of vx_grid_aabbs; the value is the material of the LAST setVoxel
 *                 call on that voxel), for VX_GRID_VEC one per setVoxel call in call order (entry i belongs to box i of the list).
 * Without the flag both are empty, as in the reference today.  *count receives the length; capacity 0 = size query. */
vx_status vx_grid_materials(const vx_grid* g, vx_material* host_out, uint64_t capacity, uint64_t* count);
vx_status vx_grid_material_ids(const vx_grid* g, int16_t* host_out, uint64_t capacity, uint64_t* count);
const int16_t* vx_grid_material_ids_device(const vx_grid* g); /* NULL without materials */
void vx_grid_free(vx_grid* g);

/* ---- octree: replaces Octree (octTree.hpp:487-523) ------------------------------------------------------- */
typedef struct vx_octree_node { uint32_t children[8]; uint32_t start; uint32_t count; } vx_octree_node; /* octTree.hpp:251-277 */
vx_status vx_octree_build(const vx_mesh* mesh, float voxel_size, uint64_t max_items_per_leaf, void* stream, vx_octree** out);
uint64_t vx_octree_num_items(const vx_octree* o);
uint64_t vx_octree_num_nodes(const vx_octree* o);
uint64_t vx_octree_bytes(const vx_octree* o); /* getMemoryUsageBytes octTree.hpp:512-523: 8*items + 40*nodes */
vx_status vx_octree_items(const vx_octree* o, uint64_t* host_morton, uint64_t capacity);
vx_status vx_octree_nodes(const vx_octree* o, vx_octree_node* host_nodes, uint64_t capacity);
vx_status vx_octree_root_bounds(const vx_octree* o, float mn[3], float mx[3]);
vx_status vx_octree_aabbs(const vx_octree* o, vx_aabb* host_out, uint64_t capacity, uint64_t* count); /* getAabbs :502-510 */
vx_status vx_octree_aabbs_device(const vx_octree* o, vx_aabb* dev_out, uint64_t capacity, uint64_t* count);
void vx_octree_free(vx_octree* o);

/* ---- rays: replaces the procedural-hit stage  raytrace.rint:46-71 under traceRayEXT (raytrace.rgen:49-64) --
 * For every ray the closest accepted hit over all occupied voxels' AABBs:  t = hitAabb() of that box,
 * accepted iff t > 0 and tmin <= t <= tmax;  prim = index of the box in vx_grid_aabbs() order of the Bool grid
 * (== gl_PrimitiveID); miss: t = -1, prim = 0xFFFFFFFF.  Rays: 6 float32 each (origin xyz, direction xyz).
 * The reference's ray interval is tmin 0.001, tmax 10000 (raytrace.rgen:50-51).
 *
 * Non-finite rays.  A ray is non-finite when any of its six components is NaN (any sign, any payload), +Inf or -Inf, whether it was
 * read from a ray buffer or generated from the camera matrices.  EVERY ray query of this header -- vx_trace*, vx_trace_multi*,
 * vx_octree_trace*, vx_octree_trace_multi*, vx_bvh_trace*, vx_bvh_trace_multi*, vx_tlas_trace*, vx_tlas_trace_multi* and the frames of vx_render_* -- reports a
 * miss for it: t = -1, prim / instance = 0xFFFFFFFF, normal and bary zero, shadowed = 0, count = 0 with every list slot padded, no
 * entry in the compacted hit list and no part in num_hits; in a frame, the pixel a miss gives (kind 0).  This is a rule of its own, not
 * the brute force's answer: hitAabb's min / max drop a NaN, so a NaN on one axis (also 0 * inf, from o[a] = +-inf with d[a] = +-inf)
 * removes that axis from the slab test and the brute force HITS the boxes the other two axes select.  Finite
 * rays keep every promise of this header unchanged; an all-zero direction is a miss as before.
 * NaN in the interval: a NaN tmin, tmax or tmax_per_ray[r] accepts nothing (every comparison with NaN fails in the acceptance rule),
 * so those rays miss as well.  NaN in a multi-hit cursor (after_t) is not specified.                          */
typedef struct vx_hit { uint32_t ray; uint32_t prim; float t; } vx_hit;
vx_status vx_trace(const vx_grid* g, const float* host_rays, uint64_t num_rays, float tmin, float tmax,
                   float* host_t /*NULL ok*/, uint32_t* host_prim /*NULL ok*/, uint64_t* num_hits /*NULL ok*/);
/* device buffers; optional compacted hit list (ballot/prefix compaction) of capacity num_rays; *dev_num_hits is a
 * device uint64 counter the call zeroes first */
vx_status vx_trace_device(const vx_grid* g, const float* dev_rays, uint64_t num_rays, float tmin, float tmax,
                          float* dev_t /*NULL ok*/, uint32_t* dev_prim /*NULL ok*/, vx_hit* dev_hits /*NULL ok*/,
                          uint64_t* dev_num_hits /*NULL ok*/);
/* primary rays generated in-kernel from the reference camera model (raytrace.rgen:41-47): pixel (px,py) of a
 * width x height image, column-major 4x4 viewInverse / projInverse; outputs indexed py*width+px */
vx_status vx_trace_primary_device(const vx_grid* g, const float view_inverse[16], const float proj_inverse[16],
                                  uint32_t width, uint32_t height, float tmin, float tmax, float* dev_t,
                                  uint32_t* dev_prim /*NULL ok*/);

/* Extended query: one struct for every input/output of the ray stage, including the two consumers of the hit in
 * raytrace2.rchit: the cube-face normal (:60-73) and the shadow query (:103-122, gl_RayFlagsTerminateOnFirstHitEXT with
 * tMax = distance to the light).  Pointers are device pointers for vx_trace_ex_device and host pointers for vx_trace_ex;
 * every output is optional. */
typedef struct vx_trace_args {
    const float* rays;           /* 6 f32 per ray; NULL = primary rays from the camera below (raytrace.rgen:41-47) */
    const float* view_inverse;   /* column-major 4x4 (host pointers in both variants) */
    const float* proj_inverse;
    uint32_t width, height;
    uint64_t num_rays;           /* ignored for camera rays (= width*height) */
    float tmin, tmax;
    const float* tmax_per_ray;   /* optional: replaces tmax per ray */
    int32_t any_hit;             /* 1: terminate on the first accepted hit; only `shadowed` (and t) may be requested */
    int32_t reserved;
    float* t;                    /* closest accepted t, -1 on miss (any_hit: some accepted t) */
    uint32_t* prim;              /* gl_PrimitiveID of the closest hit, 0xFFFFFFFF on miss */
    float* normal;               /* 3 f32 per ray: (+-1,0,0)/(0,+-1,0)/(0,0,+-1), zeros on miss */
    uint8_t* shadowed;           /* 1 = an accepted hit exists */
    vx_hit* hits;                /* device variant only: compacted hit list */
    uint64_t* num_hits;
} vx_trace_args;
vx_status vx_trace_ex_device(const vx_grid* g, const vx_trace_args* args);
vx_status vx_trace_ex(const vx_grid* g, const vx_trace_args* args);

/* Multi-hit query: ALL the voxels a ray meets, in order -- X-ray and thickness images, depth peeling, counting wall crossings.
 * For ray r let A(r) be the set of occupied cells c whose t_c = hitAabb(box_c) is accepted by the rule above (t_c > 0 and
 * tmin <= t_c <= tmax, or tmax_per_ray[r] in place of tmax); box_c is the box vx_grid_aabbs emits for the cell and prim_c its index in
 * the Bool grid's list order.  A(r) is ordered by (t, prim) ascending: t compared as float, ties broken by the smaller prim.  With the
 * optional per-ray cursor (after_t[r], after_prim[r]) only the hits STRICTLY after the cursor in that order belong to A(r), for the
 * counts and the lists alike; a cursor of (-1, anything) is the same as no cursor.  Outputs per ray, K = max_hits:
 *   t[r*K + j], prim[r*K + j]   the j-th element of A(r) for j < min(K, |A(r)|); the remaining slots are -1.0f and 0xFFFFFFFF;
 *   count[r]                    |A(r)|, the full count even when it exceeds K.
 * Every output is bit-equal to the brute force over all occupied boxes; without a cursor slot 0 is what vx_trace_ex returns for t and
 * prim.  Lists longer than K are paged: call again with the cursor at the last hit of the previous page.
 * Checks, in this order, each writing nothing: NULL grid or args, K outside 1..VX_MULTIHIT_MAX, exactly one of the two cursor arrays,
 * any forbidden field of `base` set: VX_ERR_INVALID_ARG.  Zero rays: VX_OK.  A grid without occupied cells: every count 0, every slot
 * padded.  The traversal structure is built on demand as for vx_trace_ex; a list emission left pending by VX_VOXELIZE_LIST_ASYNC stays
 * pending; a repeated device call at the same ray count requests no device memory (vx_device_allocations unchanged). */
#define VX_MULTIHIT_MAX 32
typedef struct vx_multihit_args {
    vx_trace_args base;        /* rays / camera / num_rays / tmin / tmax / tmax_per_ray as for vx_trace_ex;
                                  base.t and base.prim hold max_hits entries PER RAY (ray-major), both optional;
                                  any_hit, normal, shadowed, hits, num_hits must be 0 / NULL -> else VX_ERR_INVALID_ARG */
    uint32_t max_hits;         /* K, 1..VX_MULTIHIT_MAX (32) */
    uint32_t reserved;
    uint32_t* count;           /* |A(r)|, the full count even when it exceeds K; optional */
    const float* after_t;      /* cursor, optional; both or neither */
    const uint32_t* after_prim;
} vx_multihit_args;
vx_status vx_trace_multi_device(const vx_grid* g, const vx_multihit_args* a);  /* device pointers, asynchronous on the grid's stream */
vx_status vx_trace_multi(const vx_grid* g, const vx_multihit_args* a);         /* host pointers, staged like vx_trace_ex */

/* ---- rays on the octree: the reference's second BLAS input (Octree{path, vs} -> getAabbs, hello_vulkan.cpp:690-697) under the
 * same raytrace.rint.  The contract of the grid trace above, applied to the list vx_octree_aabbs() returns (ascending Morton code,
 * duplicates included, octTree.hpp:502-510):
 *   t       the minimum of hitAabb over all list boxes, accepted iff t > 0 and tmin <= t <= tmax (or tmax_per_ray[r]); miss: -1;
 *   prim    the smallest list index among the boxes reaching that minimum (duplicate items have identical boxes, so prim is always the
 *           first index of its run of equal codes); miss: 0xFFFFFFFF;
 *   normal, shadowed (any_hit), camera rays and the compacted hit list exactly as vx_trace_ex / vx_trace_ex_device give them.
 * An octree without items (empty mesh) gives all misses.  Grids with an axis above 65535 cells: the traced boxes are the ones
 * vx_octree_aabbs emits, which carry the reference's low-16-bit Morton interleave (octTree.hpp:211-218): cell coordinates alias
 * modulo 65536 along such an axis.  Work runs on the octree's stream.  Argument rules as for vx_trace_ex*: any_hit together with
 * prim, normal or hits is VX_ERR_INVALID_ARG, hits on the host variant VX_ERR_UNSUPPORTED. */
vx_status vx_octree_trace_ex_device(const vx_octree* o, const vx_trace_args* args);  /* device pointers, incl. compacted hits */
vx_status vx_octree_trace_ex(const vx_octree* o, const vx_trace_args* args);         /* host pointers (staged), no `hits` */
vx_status vx_octree_trace(const vx_octree* o, const float* host_rays, uint64_t num_rays, float tmin, float tmax,
                          float* host_t /*NULL ok*/, uint32_t* host_prim /*NULL ok*/, uint64_t* num_hits /*NULL ok*/);

/* Multi-hit query on the octree: vx_trace_multi's query where the dense grid cannot exist (Grid voxelization refuses more than 2^37 cells
 * with VX_ERR_CAPACITY).  The struct is vx_multihit_args, unchanged.
 * List and runs.  The list is what vx_octree_aabbs returns: ascending Morton code, duplicates included.  A RUN is a maximal range of equal
 * codes; equal codes have identical boxes.  A run stands for ONE voxel, and its prim is the first list index of the run -- the index
 * vx_octree_trace_ex already reports.  Runs, not list entries, because a voxel touched by five triangles is one voxel to an X-ray:
 * counting entries would fill the K slots with copies of one box, paging by (t, prim) would need every copy ordered, and the first-hit
 * query already names a voxel by the first index of its run.
 * A(r) is the set of runs whose t = hitAabb(box) passes the first-hit query's own acceptance rule: t > 0 and tmin <= t <= tmax, with
 * tmax_per_ray[r] in place of tmax where given.  A(r) is ordered by (t, prim) ascending: t compared as float, ties to the smaller prim.
 * With the cursor (after_t[r], after_prim[r]) only the elements STRICTLY after it in that order belong to A(r), for the lists and the
 * counts alike; (-1, anything) means no cursor.  Outputs per ray, K = max_hits (1..VX_MULTIHIT_MAX):
 *   t[r*K + j], prim[r*K + j]   the j-th element of A(r) for j < min(K, |A(r)|); the remaining slots are -1.0f and 0xFFFFFFFF;
 *   count[r]                    |A(r)|, even above K.
 * Every output is bit-equal to the brute force over the de-duplicated list; without a cursor slot 0 is exactly what vx_octree_trace_ex
 * gives for t and prim.
 * Consequences.  On a scene with every axis at or below 65535 cells the distinct boxes are the Bool grid's boxes, so count and the
 * sequence of t values equal vx_trace_multi's on the same rays; the prim values differ (Morton order here, x-fastest there).  Above
 * 65535 cells on an axis, the cells that alias to one code (the reference's 16-bit interleave, see above) form one run and count once.
 * Checks, in this order, each writing nothing: NULL octree or args, K outside 1..VX_MULTIHIT_MAX, exactly one of the two cursor arrays,
 * any forbidden field of `base` set (any_hit, normal, shadowed, hits, num_hits): VX_ERR_INVALID_ARG.  Zero rays: VX_OK.  An octree without
 * items: every count 0, every slot padded.  Non-finite rays and NaN intervals: the rule above vx_trace.  Work runs on the octree's
 * stream; a repeated device call at the same ray count requests no device memory (vx_device_allocations unchanged). */
vx_status vx_octree_trace_multi_device(const vx_octree* o, const vx_multihit_args* a); /* device pointers, asynchronous on the octree's stream */
vx_status vx_octree_trace_multi(const vx_octree* o, const vx_multihit_args* a);        /* host pointers, staged like vx_octree_trace_ex */

/* ---- rays on the triangle mesh: the reference's triangle BLAS (hello_vulkan.cpp:596-635, objectToVkGeometryKHR over the model loadModel
 * reads at :197) under raytrace.rchit, as a BVH built on the device.  Rays, ray interval, camera rays and the compacted hit list are those
 * of vx_trace_ex.  Triangle k is the k-th index triple of the mesh (its gl_PrimitiveID in a single-geometry BLAS), vertices v0 v1 v2 as
 * stored.  Per (ray, triangle) Moeller-Trumbore in float32, exactly in this order, no contraction:
 *     e1 = v1 - v0;  e2 = v2 - v0;  cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x);  dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *     p = cross(d, e2);  det = dot(e1, p);  inv = 1.0f / det;  s = o - v0;  u = dot(s, p) * inv;  q = cross(s, e1);  v = dot(d, q) * inv;
 *     t = dot(e2, q) * inv;   accepted iff u >= 0 && u <= 1 && v >= 0 && u + v <= 1 && t > 0 && t >= tmin && t <= tmax
 * (a comparison with NaN fails; det == 0 needs no special case; edges and vertices are closed; triangles are two-sided, as the reference's
 * TRIANGLE_FACING_CULL_DISABLE makes them).
 *   t        the minimum accepted t over all triangles, -1 on a miss;
 *   prim     the smallest triangle index among those reaching it (a ray through a shared edge reports the lower index), 0xFFFFFFFF on a miss;
 *   bary     (u, v) of prim: raytrace.rchit's hitAttributeEXT vec2 attribs (:31,66); (0, 0) on a miss;
 *   normal   the unit geometric normal cross(e1, e2) / sqrt(dot(., .)) of prim, not flipped (rounding not pinned); zeros on a miss;
 *   shadowed (any_hit) 1 iff some triangle is accepted, t then some accepted t; tmax_per_ray honoured.
 * t, prim and bary are bit-equal to the brute force over all triangles: the BVH only accelerates.  (Every vertex a triangle references
 * is finite: the build refuses anything else.)
 * The BVH is a binary LBVH: vx_bvh_nodes returns its node array, vx_bvh_node records with the root at index 0:
 *   interior  a, b = the indices of its two children;
 *   leaf      b = 0x80000000 | count, a = the position of its first triangle in LEAF ORDER (the leaves' triangles, leaf after leaf);
 *   min, max  the exact float min / max of the vertices below the node.
 * vx_bvh_leaf_triangles returns the triangle index of every leaf-order position.  Once built the BVH holds its own copy of the vertices
 * (freeing the mesh is legal).  Work runs on the BVH's stream.  Argument rules as for vx_trace_ex*: any_hit together with prim, normal,
 * hits or bary is VX_ERR_INVALID_ARG, hits on the host variant VX_ERR_UNSUPPORTED.  A mesh without triangles gives all misses. */
typedef struct vx_bvh vx_bvh;
typedef struct vx_bvh_node { float min[3]; uint32_t a; float max[3]; uint32_t b; } vx_bvh_node;
#define VX_BVH_LEAF 0x80000000u
#define VX_BVH_DEFAULT_LEAF 4u
/* max_leaf_triangles: 0 = VX_BVH_DEFAULT_LEAF.  A borrowed device mesh whose indices leave [0, num_vertices) fails with VX_ERR_INVALID_ARG,
 * and so does any mesh with a non-finite coordinate in a referenced vertex ("geometry at its extremes", rule 1). */
vx_status vx_bvh_build(const vx_mesh* mesh, uint32_t max_leaf_triangles, void* stream, vx_bvh** out);
/* steady state: rebuild from the (refreshed) mesh into the same handle -- no allocation when the triangle count repeats */
vx_status vx_bvh_build_into(const vx_mesh* mesh, vx_bvh* bvh);
uint64_t vx_bvh_num_triangles(const vx_bvh* b);
uint64_t vx_bvh_num_nodes(const vx_bvh* b);
uint64_t vx_bvh_bytes(const vx_bvh* b);     /* device bytes of the node array + the triangle copies (32 B per node, 48 B per triangle) */
uint32_t vx_bvh_height(const vx_bvh* b);    /* an upper bound of the tree's height (<= 62 by construction) */
/* triangles whose angle at v0 has a sine below 2^-10 (slivers, collinear): their Moeller-Trumbore t is rounding noise that no box can
 * bound, so every ray tests them one by one before the descent -- a mesh made mostly of them traces at brute-force speed */
uint64_t vx_bvh_num_ill_conditioned(const vx_bvh* b);
vx_status vx_bvh_root_bounds(const vx_bvh* b, float mn[3], float mx[3]);
vx_status vx_bvh_nodes(const vx_bvh* b, void* host_out, uint64_t capacity_bytes, uint64_t* bytes);  /* vx_bvh_node array; capacity 0 = size query */
vx_status vx_bvh_leaf_triangles(const vx_bvh* b, uint32_t* host_out, uint64_t capacity);            /* num_triangles entries */
const void* vx_bvh_nodes_device(const vx_bvh* b);  /* the node array in device memory (stable across vx_bvh_build_into of the same size) */
typedef struct vx_bvh_trace_args {
    vx_trace_args base;  /* normal = the geometric normal above */
    float* bary;         /* 2 f32 per ray (u, v), optional */
} vx_bvh_trace_args;
vx_status vx_bvh_trace_ex_device(const vx_bvh* b, const vx_bvh_trace_args* args);  /* device pointers, incl. compacted hits */
vx_status vx_bvh_trace_ex(const vx_bvh* b, const vx_bvh_trace_args* args);         /* host pointers (staged), no `hits` */
vx_status vx_bvh_trace(const vx_bvh* b, const float* host_rays, uint64_t num_rays, float tmin, float tmax,
                       float* host_t /*NULL ok*/, uint32_t* host_prim /*NULL ok*/, uint64_t* num_hits /*NULL ok*/);
/* Multi-hit query on the mesh: ALL the triangles a ray crosses, in order -- X-ray and thickness images of the mesh itself, depth peeling,
 * counting wall crossings, the layers behind a transparent surface.  For ray r let A(r) be the set of triangles k that the pinned
 * Moeller-Trumbore above accepts (u >= 0 && u <= 1 && v >= 0 && u + v <= 1 && t > 0 && t >= tmin && t <= tmax, tmax_per_ray[r] in place of
 * tmax when given).  A(r) is ordered by (t, prim) ascending: t compared as float, prim the triangle's index in the mesh -- on a closed mesh
 * a ray through a shared edge meets two triangles at one t, so the prim part decides often.  With the optional per-ray cursor
 * (after_t[r], after_prim[r]) only the hits STRICTLY after the cursor in that order belong to A(r), for the counts and the lists alike; a
 * cursor of (-1, anything) is the same as no cursor.  Outputs per ray, K = m.max_hits in 1..VX_MULTIHIT_MAX:
 *   m.base.t[r*K + j], m.base.prim[r*K + j], bary[(r*K + j)*2 ..]   the j-th element of A(r) and its (u, v) for j < min(K, |A(r)|); the
 *                                remaining slots are -1.0f, 0xFFFFFFFF and (0, 0);
 *   m.count[r]                   |A(r)|, the full count even when it exceeds K.
 * Every output is bit-equal to the brute force over all triangles; without a cursor slot 0 is what vx_bvh_trace_ex returns for t, prim and
 * bary.  Lists longer than K are paged: call again with the cursor at the last hit of the previous page.
 * Checks, in this order, each writing nothing: NULL handle or args, K outside 1..VX_MULTIHIT_MAX, exactly one of the two cursor arrays, any
 * forbidden field of m.base set (any_hit, normal, shadowed, hits, num_hits): VX_ERR_INVALID_ARG.  Zero rays: VX_OK.  A mesh without
 * triangles: every count 0, every slot padded.  Camera rays (m.base.rays == NULL) as for vx_bvh_trace_ex.  Work runs on the BVH's stream;
 * a repeated device call requests no device memory (vx_device_allocations unchanged). */
typedef struct vx_bvh_multihit_args {
    vx_multihit_args m;  /* as for vx_trace_multi; m.base.t and m.base.prim hold max_hits entries PER RAY (ray-major) */
    float* bary;         /* 2 f32 per slot (u, v), optional */
} vx_bvh_multihit_args;
vx_status vx_bvh_trace_multi_device(const vx_bvh* b, const vx_bvh_multihit_args* a);  /* device pointers, asynchronous on the BVH's stream */
vx_status vx_bvh_trace_multi(const vx_bvh* b, const vx_bvh_multihit_args* a);         /* host pointers, staged like vx_bvh_trace_ex */
void vx_bvh_free(vx_bvh* b);

/* ---- instanced triangle scenes: the reference's top-level acceleration structure (createTopLevelAS, hello_vulkan.cpp:760-790) over the
 * models loadModel(filename, transform) appends (:197-240), as a TLAS built on the device over transformed instances of vx_bvh BLAS.
 * Instance i: object-to-world M = transform (row-major 3x4 as VkTransformMatrixKHR, hello_vulkan.cpp:771: rows (m0 m1 m2 | m3),
 * (m4 m5 m6 | m7), (m8 m9 m10 | m11)), blas = the index into the BLAS list given at build (gl_InstanceCustomIndexEXT -> objDesc),
 * mask 0 = never hit (the instance mask against the reference's cullMask 0xFF).
 * World-to-object W, computed on the device by the build and by every update, in float64 exactly in this order, then rounded to float32:
 *     C = cofactors of the 3x3 A = (m0 m1 m2; m4 m5 m6; m8 m9 m10):
 *         c00 = m5*m10 - m6*m9   c01 = m6*m8 - m4*m10   c02 = m4*m9 - m5*m8
 *         c10 = m2*m9 - m1*m10   c11 = m0*m10 - m2*m8   c12 = m1*m8 - m0*m9
 *         c20 = m1*m6 - m2*m5    c21 = m2*m4 - m0*m6    c22 = m0*m5 - m1*m4
 *     det = (m0*c00 + m1*c01) + m2*c02;   inv[r][c] = c{c}{r} / det;   w3(row r) = -((inv[r][0]*m3 + inv[r][1]*m7) + inv[r][2]*m11)
 *     W row r = (float)inv[r][0], (float)inv[r][1], (float)inv[r][2], (float)w3(row r)   (the inv used for w3 is the float64 one)
 * An instance is INACTIVE (never hit) when mask == 0, blas >= num_blas, its BLAS has no triangles, det is 0 or not finite, or an entry of
 * W is not finite.  vx_tlas_build / vx_tlas_update reject a blas index out of range and a non-finite transform with VX_ERR_INVALID_ARG;
 * vx_tlas_update_device cannot report them and marks such instances inactive.  vx_tlas_world_to_object returns the W actually used.
 * Per ray, for each active instance i and each triangle k of its BLAS, in float32, no contraction:
 *     o' = ((w0*ox + w1*oy) + w2*oz) + w3,  d' = (w0*dx + w1*dy) + w2*dz   per row of W;
 *     k tested on (o', d') with vx_bvh's pinned Moeller-Trumbore and the SAME tmin / tmax (t is parametric: the interval carries over).
 *   t         the minimum accepted t over all active (instance, triangle) pairs, -1 on a miss;
 *   instance  and prim: the lexicographically smallest (instance, triangle) pair reaching it; 0xFFFFFFFF / 0xFFFFFFFF on a miss;
 *   bary      (u, v) of that pair; (0, 0) on a miss;
 *   normal    the unit geometric normal of the WORLD-space triangle, vertices M*v = ((m0*x + m1*y) + m2*z) + m3 per row, then
 *             cross(e1, e2) / sqrt(dot(., .)) as vx_bvh computes it, not flipped (rounding not pinned); zeros on a miss;
 *   shadowed  (any_hit) and tmax_per_ray as for vx_bvh;
 *   hits      the compacted list as for vx_bvh: vx_hit carries the ray, prim and t but NOT the instance -- request `instance` as well to
 *             attribute a listed hit to its object.
 * t, instance, prim and bary are bit-equal to the brute force over every pair: the TLAS only accelerates.  One exception is not covered
 * by that argument: a BLAS's side list of ill-conditioned triangles (vx_bvh_num_ill_conditioned) is tested only when the ray
 * reaches the instance's TLAS leaf, so a rounding-noise hit on such a sliver far outside the instance's widened world box may be pruned.
 * vx_tlas_nodes returns the node array (vx_bvh_node records, root at 0, 2n-1 of them for n >= 1 instances): interior a, b = the children;
 * leaf b = VX_BVH_LEAF | 1, a = the instance; min / max the widened world boxes (empty boxes, min > max, for inactive instances; -Inf / +Inf for an instance whose world box
 * overflows float32).
 * Ownership: the TLAS BORROWS its BLAS handles; they must outlive it.  After a BLAS is rebuilt (vx_bvh_build_into) the caller calls
 * vx_tlas_update* (as in Vulkan): an update re-reads every BLAS's root box, node and triangle arrays, height and side list, and rebuilds the
 * TLAS over the given instances.  vx_tlas_update has copied the host array when it returns (the caller may reuse it at once) and does not
 * wait for the rebuild; it stages through two pinned buffers in turn and waits on the host only for the copy of the update before the
 * previous one; vx_tlas_update_device reads a DEVICE array of vx_instance on the TLAS's stream and neither synchronises nor copies
 * to or from the host.  An update with the same instance count requests no device memory (vx_device_allocations unchanged).
 * Streams: work runs on the TLAS's stream; build, update and trace make it wait for the work queued so far on the BLAS streams, and a
 * trace makes those streams wait for it (a later vx_bvh_build_into cannot overwrite what it reads).  Argument rules of the trace functions
 * as for vx_bvh_trace_ex*; any_hit together with instance is VX_ERR_INVALID_ARG too.  Zero instances give all misses. */
typedef struct vx_tlas vx_tlas;
typedef struct vx_instance {
    float transform[12];  /* object-to-world, row-major 3x4 */
    uint32_t blas;        /* index into the BLAS list given at build */
    uint32_t mask;        /* 0 = never hit */
} vx_instance;
vx_status vx_tlas_build(const vx_bvh* const* blas, uint32_t num_blas, const vx_instance* host_instances, uint64_t num_instances, void* stream,
                        vx_tlas** out);
vx_status vx_tlas_update(vx_tlas* t, const vx_instance* host_instances, uint64_t num_instances);
vx_status vx_tlas_update_device(vx_tlas* t, const vx_instance* dev_instances, uint64_t num_instances);  /* asynchronous, no host sync */
uint64_t vx_tlas_num_instances(const vx_tlas* t);
uint64_t vx_tlas_num_nodes(const vx_tlas* t);
uint32_t vx_tlas_height(const vx_tlas* t);   /* the built tree's height (reads it back: synchronises the TLAS's stream) */
uint64_t vx_tlas_bytes(const vx_tlas* t);    /* device bytes of the node array (32 B per node) and the per-instance records (100 B) */
vx_status vx_tlas_world_to_object(const vx_tlas* t, float* host_out /* 12 per instance */, uint64_t capacity /* floats */);
vx_status vx_tlas_nodes(const vx_tlas* t, void* host_out, uint64_t capacity_bytes, uint64_t* bytes);  /* capacity 0 = size query */
typedef struct vx_tlas_trace_args {
    vx_trace_args base;   /* normal = the world geometric normal above */
    float* bary;          /* 2 f32 per ray (u, v), optional */
    uint32_t* instance;   /* instance index, 0xFFFFFFFF on a miss, optional */
} vx_tlas_trace_args;
vx_status vx_tlas_trace_ex_device(const vx_tlas* t, const vx_tlas_trace_args* args);  /* device pointers, incl. compacted hits */
vx_status vx_tlas_trace_ex(const vx_tlas* t, const vx_tlas_trace_args* args);         /* host pointers (staged), no `hits` */
vx_status vx_tlas_trace(const vx_tlas* t, const float* host_rays, uint64_t num_rays, float tmin, float tmax, float* host_t /*NULL ok*/,
                        uint32_t* host_instance /*NULL ok*/, uint32_t* host_prim /*NULL ok*/, uint64_t* num_hits /*NULL ok*/);
/* Multi-hit query on the instances: the contract of vx_bvh_trace_multi over all active (instance, triangle) pairs.  Each pair is tested on
 * the instance's object-space ray above (o' = ((w0*ox + w1*oy) + w2*oz) + w3, d' = (w0*dx + w1*dy) + w2*dz per row of W) with the SAME
 * tmin / tmax.  A(r) is ordered by (t, instance, prim) ascending -- two instances of one BLAS under the same transform tie at every hit, and
 * the lower instance comes first.  `instance[r*K + j]` is one more output, padded with 0xFFFFFFFF.  The cursor is (after_t[r],
 * after_instance[r], after_prim[r]): all three arrays or none, else VX_ERR_INVALID_ARG (the third check).  Without a cursor slot 0 is what
 * vx_tlas_trace_ex returns for t, instance, prim and bary.  Every output is bit-equal to the brute force over every pair, with the one
 * exception of vx_tlas_trace_ex, verbatim: a BLAS's side list of ill-conditioned triangles is tested only when the ray reaches the
 * instance's TLAS leaf.  Zero instances, or none active: every count 0, every slot padded.  Streams as for vx_tlas_trace_ex: the call
 * waits for the work queued on the BLAS streams and makes them wait for it. */
typedef struct vx_tlas_multihit_args {
    vx_multihit_args m;
    float* bary;                     /* 2 f32 per slot (u, v), optional */
    uint32_t* instance;              /* max_hits entries per ray, optional */
    const uint32_t* after_instance;  /* the cursor's instance part: with m.after_t and m.after_prim, or none of the three */
} vx_tlas_multihit_args;
vx_status vx_tlas_trace_multi_device(const vx_tlas* t, const vx_tlas_multihit_args* a);  /* device pointers, asynchronous on the TLAS's stream */
vx_status vx_tlas_trace_multi(const vx_tlas* t, const vx_tlas_multihit_args* a);         /* host pointers, staged like vx_tlas_trace_ex */
void vx_tlas_free(vx_tlas* t);   /* waits for the TLAS's stream */

/* ---- frames: the reference's per-frame dispatch (raytrace.rgen -> raytrace.rint / raytrace2.rchit on the voxels, raytrace.rchit on the
 * triangles, a shadow ray into the TLAS, raytrace.rmiss, post.frag) as one asynchronous sequence of kernels that leaves a shaded RGBA8
 * image in device memory.  Per pixel r = py*width + px:
 *   primary ray   the camera ray of vx_trace_args (rgen:41-51, tmin 0.001, tmax 10000) against the voxels and, with a mesh, its BVH; the
 *                 closer hit wins, the voxel on equal t (kind 1 voxel, 2 triangle, 0 miss);
 *   shadow ray    from org + dir*t toward the light (a triangle hit: the light vector from the position its barycentrics interpolate),
 *                 tMax = the light distance, any-hit against the voxels and the mesh; dir is computed as voxilizer --render computes it
 *                 on the host, and origin, direction and tMax are bit-equal to that function's;
 *   shading       raytrace2.rchit:53-137 (voxels: cube normal, the grid's per-voxel material or MaterialObj{}) / raytrace.rchit:49-143
 *                 (triangles: the geometric normal turned toward the ray, the OBJ material of the triangle or MaterialObj{}, no textures -- see
 *                 vx_render_set_shading for vertex normals and textures):
 *                 diffuse + ambient (illum >= 1), specular (illum >= 2, lit and not shadowed), attenuation 0.3 when shadowed -- and for
 *                 a voxel facing away from the light, 1 for such a triangle; miss colour 0.8 (rmiss:37); gamma pow(clamp(c, 0, 1), 1/2.2)
 *                 rounded to nearest (post.frag:36); alpha 255.
 * The image equals voxilizer --render's within 1 LSB per channel (device powf against host powf); kind and shadowed are exact.
 * Light: position / intensity / type as the reference's push constants (hello_vulkan.h:84-90); NULL = its default, a point light at
 * {10, 55, 8} of intensity 1000.  Type 1 (directional, rchit:86-91): L = position * (1 / |position|), light distance 100000 (the shadow
 * ray's tMax), intensity not divided by the squared distance.
 * Shading at its extremes.  Every max / min of the shading is IEEE maxNum / minNum (fmaxf / fminf: the operand that is not NaN), and every
 * input below is a value the frame is defined for -- the stated float32 formula, evaluated as written:
 *   colour     a channel that is NaN before the gamma encodes as 0, +Inf as 255, -Inf and every negative as 0 (clamp = fminf(fmaxf(c, 0), 1));
 *   shininess  kSh = fmaxf(shininess, 4): a NaN shininess is 4;
 *   dot(N, L)  NaN is "not lit": shadowed = 0, the shadow ray gets the empty interval (tMax 0 below tMin), the diffuse factor
 *              fmaxf(dot, 0) is 0, and the attenuation is that of a hit facing away from the light -- 1 for a triangle, 0.3 for a voxel;
 *   light      position and intensity are any float32 values, non-finite ones included; kind never depends on the light.  With
 *              len = sqrtf(dot(l, l)) and L = l * (1 / len): a len of +Inf (dot overflows) gives 1 / len = 0 and L = 0, a non-finite l gives a
 *              NaN in L, and both are "not lit"; so are len = 0 with l = 0 (0 * Inf) and any L that has a NaN where N is not 0.  A lit pixel
 *              therefore has a finite shadow ray, with one exception: l != 0 so short that dot(l, l) underflows to 0 (|l| below about
 *              1e-23) has L = +-Inf in every component (NaN where l is 0), and a pixel whose N and l are non-zero in all three may be lit;
 *              its shadow ray is non-finite and, by the rule for non-finite rays above, hits nothing;
 *   material   ambient, diffuse, specular and shininess are any float32 values (negative, above 1, non-finite); illum is any int32
 *              (>= 1 adds the ambient term, >= 2 the specular one: 0 and negatives add neither, 3 and above both).  vx_mesh_set_materials
 *              refuses a triangle id below -1 or at or above the table size (-1: no material, MaterialObj{}); a texture slot may be any int32
 *              (negative or at or above vx_mesh_num_textures: no texture).
 * Everything before the two powf calls (the specular term, the gamma) is float32 with its association pinned, so a byte differs from
 * floor(255 * c^(1/2.2) + 0.5), evaluated with both powers in float64 from their float32 arguments, only where 255 * c^(1/2.2) lies within
 * 2^-12 of a rounding tie, and then by 1 (tests/shading_extremes.py).
 * Streams: a frame runs on the scene's stream.  It first makes that stream wait for the work queued so far on the voxel source's and the
 * BVH's streams, and at its end makes those streams wait for the frame -- a later vx_voxelize_into / vx_bvh_build_into on them cannot
 * overwrite what the frame still reads.  The grid's traversal structure is built lazily on the grid's own stream, as for vx_trace_ex.
 * The scene owns all its scratch (pooled): a frame of a size already rendered allocates nothing, and vx_render_frame_device neither
 * synchronises nor copies to the host -- it returns once the frame is enqueued.
 * The scene BORROWS its handles: grid or octree, BVH and mesh must outlive it.  Unlike vx_bvh alone, the mesh must stay alive too (the
 * frame reads its vertices, index triples and per-triangle materials).  A grid or BVH rebuilt in place is picked up by the next frame;
 * material tables (the grid's, the mesh's) are read at creation and by vx_render_refresh only.
 * Errors, checked before anything is enqueued: VX_ERR_INVALID_ARG for a null scene / args / camera / rgba, zero width or height, both or
 * neither voxel source, a grid other than VX_GRID_BOOL, bvh without mesh or the reverse, a mesh whose triangle count differs from the
 * BVH's, a light type other than 0 or 1; VX_ERR_CAPACITY above 2^32 pixels; VX_ERR_NO_DEVICE without a device (there is no CPU path). */
typedef struct vx_render_scene vx_render_scene;
typedef struct vx_render_light {
    float position[3];
    float intensity;
    int32_t type;           /* 0 point, 1 directional */
} vx_render_light;
typedef struct vx_render_desc {
    const vx_grid* grid;     /* exactly one of grid (VX_GRID_BOOL) and octree */
    const vx_octree* octree;
    const vx_bvh* bvh;       /* optional triangle model ... */
    const vx_mesh* mesh;     /* ... and the mesh it was built from (vertices, indices, per-triangle materials): both or neither */
    void* stream;            /* hipStream_t of the frames; NULL = the default stream */
} vx_render_desc;
typedef struct vx_render_args {
    const float* view_inverse;       /* host, column-major, as vx_trace_args */
    const float* proj_inverse;
    uint32_t width, height;
    const vx_render_light* light;    /* NULL = the reference's default */
    uint32_t* rgba;                  /* width*height RGBA8, R in the low byte (device pointer in _device, host pointer in vx_render_frame) */
    uint8_t* kind;                   /* optional: 0 miss, 1 voxel, 2 triangle */
    uint8_t* shadowed;               /* optional: the OR of both shadow queries where the shading reads it (a hit with dot(N, L) > 0), 0 elsewhere */
} vx_render_args;
vx_status vx_render_create(const vx_render_desc* desc, vx_render_scene** out);
/* Instanced scenes: the triangles come from a vx_tlas (its BLAS list gives one mesh each, in the same order: vertices, index triples,
 * per-triangle materials, objDesc[gl_InstanceCustomIndexEXT] of raytrace.rchit:52).  The frame is the sequence above with k_tlas_trace
 * in place of the BVH's traversal for the primary and the shadow rays; the primary merge is unchanged; the triangle hit point is
 * M * ((p0*b0 + p1*b1) + p2*b2) with M the instance's object-to-world rows in the pinned association ((m0*x + m1*y) + m2*z) + m3 (with M
 * the identity, the BVH scene's expression bit for bit); the shading normal is vx_tlas's world geometric normal turned toward the ray;
 * the material is the instance's mesh's.  At most one voxel source: a triangle-only scene (grid = octree = NULL) is allowed.  Streams:
 * a frame waits for the work queued so far on the voxel source's and the TLAS's streams, and at its end makes those streams and every
 * BLAS's stream wait for it -- an update enqueued after the frame cannot change what the frame reads, and a TLAS updated on its stream is
 * picked up by the next frame.  A frame of a size already rendered allocates nothing and never synchronises, with or without TLAS updates
 * of the same instance count between frames.  Errors: VX_ERR_INVALID_ARG for a null tlas or meshes, both voxel sources, a grid other than
 * VX_GRID_BOOL, a null mesh, a mesh whose triangle count differs from its BLAS's, or handles on different devices. */
typedef struct vx_render_tlas_desc {
    const vx_grid* grid;            /* at most one of grid (VX_GRID_BOOL) and octree; neither = triangles only */
    const vx_octree* octree;
    const vx_tlas* tlas;
    const vx_mesh* const* meshes;   /* one per BLAS of the TLAS, in its BLAS order */
    void* stream;
} vx_render_tlas_desc;
vx_status vx_render_create_tlas(const vx_render_tlas_desc* desc, vx_render_scene** out);
vx_status vx_render_refresh(vx_render_scene* s);                               /* re-read the material and attribute tables of the sources */
/* Attribute shading (flags = VX_RENDER_ATTRIBUTES; 0 = the shading above; other bits VX_ERR_INVALID_ARG), from the next frame, in BVH and
 * TLAS scenes.  Voxel hits are shaded as above.  A triangle hit, in float32 with every association pinned (b0 = (1 - b1) - b2):
 *   n   object space: the corner normals (n0*b0 + n1*b1) + n2*b2 when the mesh has them, else the face normal cross(p1 - p0, p2 - p0) =
 *       (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), e1 = p1 - p0, e2 = p2 - p0;
 *   N   world space: W^T n for an instance, W its world-to-object 3x3 (vx_tlas_world_to_object), component j = (w0j*n0 + w1j*n1) + w2j*n2;
 *       n itself in a BVH scene; then N = n / sqrtf((n0*n0 + n1*n1) + n2*n2), NOT turned toward the ray (raytrace.rchit:73-74: a back face is
 *       lit as the reference lights it).  N zero or not finite: the default normal (the geometric normal turned toward the ray).  N is the
 *       normal of the light test dot(N, L) > 0, of the shadow-ray compaction, of the diffuse and of the specular term.
 *   tex when the triangle's material (none: MaterialObj{}, no texture) has a slot with 0 <= slot < vx_mesh_num_textures: uv = (uv0*b0 +
 *       uv1*b1) + uv2*b2; per axis, w the width or height: x = u*w - 0.5, f = x - floorf(x), i0 = floorf(x) mod w (non-negative, repeat
 *       addressing), i1 = (i0 + 1) mod w, and for a non-finite x or |x| >= 2^62 i0 = i1 = 0, f = 0; texels decoded by a 256-entry table of
 *       the sRGB EOTF (c/12.92 for c <= 0.04045, else ((c + 0.055)/1.055)^2.4, computed in float64 and rounded to float32; R8G8B8A8_SRGB of
 *       hello_vulkan.cpp:286-350); tex = (t00*(1-fx) + t10*fx)*(1-fy) + (t01*(1-fx) + t11*fx)*fy per rgb channel (t10: texel (i1x, i0y)),
 *       1-f in float32, alpha ignored; the base level only, no mipmaps; float weights where a hardware sampler quantises them.  The diffuse
 *       term, ambient already added, is multiplied by tex (rchit:99-104); the specular term is not.
 * kind and shadowed are exact and rgba is within 1 LSB of a float32 restatement (powf of the specular term and of the gamma being the only
 * difference); with one identity instance a TLAS scene's frame equals the BVH scene's bit for bit.  Corner attributes, textures, material
 * slots and the table are uploaded at creation and by vx_render_refresh, never per frame; a frame in this mode allocates nothing at a size
 * already rendered and neither synchronises nor copies to the host. */
#define VX_RENDER_ATTRIBUTES 1u
vx_status vx_render_set_shading(vx_render_scene* s, uint32_t flags);
vx_status vx_render_frame_device(vx_render_scene* s, const vx_render_args* a);  /* asynchronous on the scene's stream */
vx_status vx_render_frame(vx_render_scene* s, const vx_render_args* a);         /* host buffers: returns when they are written */
void vx_render_free(vx_render_scene* s);                                        /* waits for the scene's stream */

/* ---- distance-field queries: a snapshot of the signed field that stays on the device, sampled at the caller's own points -------------
 * vx_field_create runs vx_grid_sdf_device's passes on the grid's stream into a buffer the field owns, copies dim, origin and voxel_size,
 * takes `state` from the grid's occupied count and returns once the field is complete (one host wait).  After that the field does not
 * depend on the grid, which may be rebuilt or freed.  `stream` is the stream of the field's queries (NULL: the default stream).  Nothing
 * a reader of the grid can see changes; a pending VX_VOXELIZE_LIST_ASYNC emission stays pending.  Checks, in this order, every failure
 * writing nothing and leaving *out NULL: NULL grid or out -> VX_ERR_INVALID_ARG; a grid of 0 cells -> VX_ERR_INVALID_ARG; the distance
 * fields' size limit -> VX_ERR_CAPACITY.  vx_field_update re-snapshots a grid of the SAME dimensions (else VX_ERR_INVALID_ARG) into the
 * same buffer and allocates nothing; origin, voxel_size and state are taken anew.  vx_field_values_device: X*Y*Z f32 at
 * x + X*(y + Y*z), exactly vx_grid_sdf's values.  vx_field_free waits for the field's stream and returns its blocks to the pool.
 *
 * THE SAMPLED FIELD (float32, in the order written, nothing fused; / and sqrtf correctly rounded; csrc/vx_field.h is this text as code).
 * Per axis a of point p:   u_raw = (p[a] - org[a]) / vs - 0.5f
 *                          out_a = (u_raw < 0) || (u_raw > (float)(dim[a]-1)) || dim[a] == 1
 *                          u = fminf(fmaxf(u_raw, 0.0f), (float)(dim[a]-1))
 *                          i0 = min((uint32_t)u, dim[a] >= 2 ? dim[a]-2 : 0);  i1 = min(i0+1, dim[a]-1);  f_a = u - (float)i0
 * With lerp(a,b,f) = a + f*(b - a) and cXYZ = S[i_X, i_Y, i_Z]:
 *   value = lerp(lerp(lerp(c000,c100,fx), lerp(c010,c110,fx), fy), lerp(lerp(c001,c101,fx), lerp(c011,c111,fx), fy), fz)
 *   gx = lerp(lerp(c100-c000, c110-c010, fy), lerp(c101-c001, c111-c011, fy), fz) / vs      (0 where out_x)
 *   gy = lerp(lerp(c010-c000, c110-c100, fx), lerp(c011-c001, c111-c101, fx), fz) / vs      (0 where out_y)
 *   gz = lerp(lerp(c001-c000, c101-c100, fx), lerp(c011-c010, c111-c110, fx), fy) / vs      (0 where out_z)
 *   occupied = every (p[a]-org[a])/vs lies in [0, dim[a])  &&  S at cell ((uint32_t)that per axis) < 0
 * The trilinear interpolant of the cell-centre values, clamped to the box of cell centres (constant across the half-cell rim and outside
 * the grid), and its exact gradient; the zero level lies on the shared face of an occupied and an empty cell.  State EMPTY: value +inf,
 * gradient 0, occupied 0.  State FULL: value -inf, gradient 0, occupied = the in-box test.  A point with a NaN or +-Inf component: value
 * 0x7FC00000, gradient 0, occupied 0.
 * vx_field_sample*: NULL f, a or points (num_points > 0), or all three outputs NULL -> VX_ERR_INVALID_ARG; zero points -> VX_OK.  The host
 * variant stages through blocks that stay on the handle: a repeated call of the same size allocates nothing.
 *
 * THE SPHERE CAST: a sphere of `radius` (world units) moved along origin + t * direction.  Per ray, float32, in this order:
 *  1. a miss (t = -1, clearance = +inf, steps = 0, status MISS) when the ray has a NaN or +-Inf component, its radius is NaN, infinite or
 *     negative, or dn = sqrtf((dx*dx + dy*dy) + dz*dz) is not > 0 or is infinite;
 *  2. [tmin, tmax] (tmax_per_ray[r] in place of tmax where given) is clipped to the grid's own box [org, org + (float)dim*vs], not grown:
 *     per axis inv = 1.0f/d[a]; isinf(inv): a miss unless lo <= o[a] <= hi; else ta = (lo-o[a])*inv, tb = (hi-o[a])*inv,
 *     t0 = fmaxf(t0, fminf(ta,tb)), t1 = fminf(t1, fmaxf(ta,tb)); !(t0 <= t1) is a miss;
 *  3. t = t0; clearance = +inf; for k in 0 .. max_steps-1:
 *         p[a] = o[a] + t*d[a];  f = value(p);  steps = k+1;  clearance = fminf(clearance, f);  g = f - radius
 *         if (g <= hit_eps*vs) { t_out = t; status = HIT; stop }
 *         t = t + (g*step_scale)/dn
 *         if (t > t1) { t_out = -1; status = MISS; stop }
 *     after the loop: t_out = -1, status = STEP_LIMIT.
 * Every partial derivative of the interpolant is at most 2 in magnitude, so |grad| <= 2 sqrt 3: with step_scale <= 1/(2 sqrt 3) ~ 0.2887
 * the march never steps over a point of the clipped segment where the field is <= radius.
 * Checks before anything is queued: NULL handle, args or rays (num_rays > 0); all outputs NULL; step_scale outside {0} U (0, 1]; hit_eps
 * negative or non-finite; max_steps > 65535; a global radius that is NaN, infinite or negative while radius_per_ray is NULL ->
 * VX_ERR_INVALID_ARG.  Zero rays -> VX_OK.  The _device variants take device pointers and are asynchronous on the field's stream. */
typedef struct vx_field vx_field;
typedef struct vx_field_desc { uint64_t dim[3]; float voxel_size; float origin[3]; uint32_t state; uint64_t bytes; } vx_field_desc;
#define VX_FIELD_FINITE 0   /* some cells occupied, some empty: every value finite   */
#define VX_FIELD_EMPTY  1   /* no occupied cell: every value +inf                    */
#define VX_FIELD_FULL   2   /* every cell occupied: every value -inf                 */
vx_status vx_field_create(const vx_grid* g, void* stream, vx_field** out);
vx_status vx_field_update(vx_field* f, const vx_grid* g);
vx_status vx_field_describe(const vx_field* f, vx_field_desc* out);
const float* vx_field_values_device(const vx_field* f);
void vx_field_free(vx_field* f);

typedef struct vx_field_sample_args {
    const float* points; uint64_t num_points;   /* 3 f32 each */
    float* value; float* gradient /*3 each*/; uint8_t* occupied;   /* outputs: NULL ok, not all */
} vx_field_sample_args;
vx_status vx_field_sample_device(const vx_field* f, const vx_field_sample_args* a);
vx_status vx_field_sample(const vx_field* f, const vx_field_sample_args* a);

#define VX_FIELD_MISS 0
#define VX_FIELD_HIT 1
#define VX_FIELD_STEP_LIMIT 2
typedef struct vx_field_trace_args {
    const float* rays; uint64_t num_rays;            /* 6 f32: origin, direction, as vx_trace */
    float tmin, tmax; const float* tmax_per_ray;     /* NULL ok */
    float radius; const float* radius_per_ray;       /* NULL ok; world units */
    float step_scale;                                /* 0 = default 0.25; else in (0, 1] */
    float hit_eps;                                   /* in cells; 0 = default 1/64; else > 0, finite */
    uint32_t max_steps;                              /* 0 = default 256; at most 65535 */
    float* t; float* clearance; uint32_t* steps; uint8_t* status;   /* each NULL ok, not all */
} vx_field_trace_args;
vx_status vx_field_sphere_trace_device(const vx_field* f, const vx_field_trace_args* a);
vx_status vx_field_sphere_trace(const vx_field* f, const vx_field_trace_args* a);

/* ---- pose queries: a body of points or spheres under many candidate poses, against the sampled field ---------------------------------
 * A body is num_points points p in its own frame (3 f32 each) with optional radii (world units; NULL: 0).  A pose is a body-to-world
 * transform m: row-major 3 x 4, 12 f32, the layout of vx_tlas_instance.transform.  THE CONTRACT (float32, in the order written, nothing
 * fused; csrc/vx_poses.h is this text as code).  For pose n and point i:
 *     q[a] = ((m[4a]*p[0] + m[4a+1]*p[1]) + m[4a+2]*p[2]) + m[4a+3]      a = 0, 1, 2
 *     v    = value(q)              the sampled field above: 0x7FC00000 for a non-finite q, +-inf on an EMPTY / FULL field
 *     g    = (v - radius[i]) + 0.0f          (the + 0.0f turns -0 into +0: equal values have equal bits)
 * A point whose g is NaN is skipped (a non-finite point, transform entry or radius, an overflowing product, inf - inf); nothing else is:
 * g = +-inf takes part.  Per pose, each output optional but not all NULL:
 *     clearance f32      the smallest g over the points not skipped; +inf when there is none
 *     point     u32      the lowest i among the points whose g equals clearance; 0xFFFFFFFF when there is none
 *     count     u32      the number of points not skipped with g <= margin
 *     position  3 f32    q of `point`, by the formula above; 0 0 0 when there is none
 *     gradient  3 f32    vx_field_sample's gradient at position: the contact normal, pointing out of the solid; 0 0 0 when there is none
 * Every output is the same bits whatever the launch shape: the reduction is an integer minimum over orderable(g) << 32 | i and an integer
 * sum.  Checks, before anything is queued, a failure writing nothing: NULL f or a, num_poses > 0 with NULL transforms, num_points > 0
 * with NULL points, all outputs NULL, a NaN margin (+-inf is allowed) -> VX_ERR_INVALID_ARG; num_points > 0xFFFFFFFE -> VX_ERR_CAPACITY.
 * Zero poses -> VX_OK, nothing written.  Zero points: every pose gets the answer of "none".
 * vx_field_poses_device takes device pointers, is asynchronous on the field's stream and does not wait on the host; vx_field_poses takes
 * host arrays and returns when they are written.  Its staging blocks and the reduction's scratch (12 bytes per pose) stay on the handle:
 * a repeated call of the same sizes allocates nothing; vx_field_free returns them.
 * VX_FIELD_POSE_CHUNK / _TILE: how a body of more than 64 points is cut (points per workgroup, poses a workgroup walks).  They do not show
 * in any result; tests place their sizes around them. */
#define VX_FIELD_POSE_CHUNK 256
#define VX_FIELD_POSE_TILE 32
typedef struct vx_field_pose_args {
    const float* points; uint64_t num_points;        /* the body: 3 f32 each */
    const float* radii;                              /* NULL ok: every radius 0 */
    const float* transforms; uint64_t num_poses;     /* 12 f32 each */
    float margin;                                    /* world units; not NaN */
    float* clearance; uint32_t* point; uint32_t* count; float* position /*3 each*/; float* gradient /*3 each*/;   /* each NULL ok, not all */
} vx_field_pose_args;
vx_status vx_field_poses_device(const vx_field* f, const vx_field_pose_args* a);
vx_status vx_field_poses(const vx_field* f, const vx_field_pose_args* a);

/* ---- test aid: the device radix sort the Octree uses for its Morton items (octTree.hpp:363 -> vx_sort.hip), applied to a host array.
 * Keys must have no bit set at or above `bits` (1..64); sorted in place. */
vx_status vx_sort_u64(uint64_t* host_keys, uint64_t n, int bits);

/* ---- test aid: the device-wide exclusive prefix scan every feature runs on (vx_kernels.hip, launch_scan_u32 / launch_scan_u8), applied
 * to host arrays, scan after scan on ONE scratch block that keeps its generation counter between scans.
 * mode: VX_SCAN_VALUES (uint32 elements), VX_SCAN_POPCOUNT (the popcounts of uint32 words), VX_SCAN_BYTES (uint8 elements).
 * Scan k reads sizes[k] elements from `in` (the inputs one after another) and writes out[0..n] = the exclusive prefix mod 2^32
 * (n + 1 entries) followed by VX_SCAN_CANARY words that must still read VX_SCAN_CANARY_VALUE; `out` holds the scans one after
 * another, sizes[k] + 1 + VX_SCAN_CANARY words each.  totals[k] is the 64-bit total as the scan wrote it: the true total T while
 * T < 2^40 - 1, else at least 2^40 - 1 and below 2^48 (values, and the three-pass path: exactly 2^40 - 1), OR-ed with total_tag
 * (bits 48..63) by the single-pass paths.  out[i] is exact for every 16384-element tile whose exclusive prefix is below 2^40 - 1.
 * paths[k]: VX_SCAN_PATH_GEN (single pass, the block's next generation number; ticket mode past 512 tiles of 16384, as for the
 * library's callers), VX_SCAN_PATH_TICKET (single pass without a generation number), VX_SCAN_PATH_THREE (three passes),
 * VX_SCAN_PATH_AUTO (what the library's own callers do: the block's next generation number).  in_offset / out_offset
 * (elements) move the device arrays off their 16-byte alignment: a uint32 scan then takes the three-pass path whatever paths[k]
 * asks.  taken[k] (optional) is the path the scan took.  sel / group16 (optional; VX_SCAN_POPCOUNT / VX_SCAN_VALUES): sel_cap /
 * group16_cap words per scan (at least ceil(32 n / 1024) / n / 16 + 1; sel in popcount mode only), filled with VX_SCAN_CANARY_VALUE before the scan; the single-pass paths write sel[c] = the element
 * whose range [pre, pre + v) holds c * 1024 (values of at most 1024) and group16[i] = out[16 i]; the three-pass path writes neither.
 * gen_start: the block's generation counter before the first scan (< 2^22; the counter wraps to 1 at 2^22 and clears the block).
 * clean[k] (optional): 1 when, after scan k, the block is in the state the next scan relies on -- all zero after a scan without a
 * generation number; after one with a generation number, the ticket words zero and every state word of that or an older
 * generation. */
#define VX_SCAN_VALUES 0u
#define VX_SCAN_POPCOUNT 1u
#define VX_SCAN_BYTES 2u
#define VX_SCAN_PATH_GEN 0u
#define VX_SCAN_PATH_TICKET 1u
#define VX_SCAN_PATH_THREE 2u
#define VX_SCAN_PATH_AUTO 3u
#define VX_SCAN_CANARY 16u
#define VX_SCAN_CANARY_VALUE 0xA5A5A5A5u
typedef struct vx_scan_args {
    uint32_t mode;
    uint32_t nscans;
    const uint64_t* sizes;   /* nscans */
    const uint32_t* paths;   /* nscans */
    const void* in;
    uint32_t* out;
    uint64_t* totals;        /* nscans */
    uint32_t* taken;         /* nscans, optional */
    uint32_t* clean;         /* nscans, optional */
    uint32_t* sel;           /* nscans * sel_cap, optional */
    uint32_t* group16;       /* nscans * group16_cap, optional */
    uint64_t sel_cap, group16_cap;
    uint64_t in_offset, out_offset;
    uint64_t total_tag;
    uint32_t gen_start;
    uint32_t pad;
} vx_scan_args;
vx_status vx_scan_u32(const vx_scan_args* a);

/* ---- test aid: poisoned pool blocks.  Every kernel works on blocks of the library's stream-ordered pool, and a block handed out holds
 * whatever its previous owner left in it: another handle, another feature, an earlier and larger call.  While the mode is on
 * (on != 0), every block the pool hands out -- recycled or new from hipMalloc -- is first filled with the 32-bit `pattern` over its whole
 * rounded size.  The fill is queued on the stream the request names and waited for before the block is returned, so the mode serialises
 * the host with that stream at every allocation: it is for tests, not for timing.  Process-wide and atomic (the worker threads of
 * vx_multi allocate too); off when the library is loaded, where it costs one relaxed atomic load per request.  Nothing else changes:
 * vx_device_allocations, vx_device_live_blocks, the same-stream / event rule of reuse and vx_release_cached_memory behave as without it.
 * A library that computes the same outputs under 0xFFFFFFFF, 0xA5A5A5A5 and 0x00000001 as on clean blocks reads no word it has not
 * written ("Who defines every block").
 * vx_pool_poisoned_blocks: blocks filled since the library was loaded; over any interval with the mode on it rises by exactly what
 * vx_device_allocations rises by. */
vx_status vx_pool_poison(int on, uint32_t pattern);
uint64_t vx_pool_poisoned_blocks(void);

/* ---- measurement aid: per-kernel durations from HIP events recorded on the launch stream (off by default).
 * slot = 0,1,... until VX_ERR_INVALID_ARG; name is the kernel symbol as launched. */
vx_status vx_profile_enable(int on);
/* time only launches of this kernel (bare name, e.g. "k_trace"); NULL or "" = every kernel.  Two event records per
 * launch are not free, so a throughput measurement selects the one kernel it prices. */
vx_status vx_profile_select(const char* kernel_name);
vx_status vx_profile_reset(void);
vx_status vx_profile_read(int slot, char* name, size_t name_capacity, double* total_ms, uint64_t* launches);
/* the number of device blocks the library's handles have requested from its memory pool since the library was loaded (pool hits
 * included): a steady-state call that allocates nothing leaves it unchanged */
uint64_t vx_device_allocations(void);
/* the number of pool blocks the library's handles and calls in progress hold right now, summed over the devices: back to its earlier
 * value once everything created in between is freed */
uint64_t vx_device_live_blocks(void);

/* ---- multi-GPU helpers (host arithmetic only) ----------------------------------------------------------------
 * Word-aligned shard of the bitmask for rank r of n: contributions of different ranks are word-disjoint, so an
 * all-gather of the shards (or a sum/max all-reduce of zero-padded buffers) equals the OR of the full masks. */
void vx_shard_words(uint64_t num_words, int rank, int world, uint64_t* word_begin, uint64_t* word_end,
                    uint64_t* padded_shard_words);
void vx_shard_range(uint64_t count, int rank, int world, uint64_t* begin, uint64_t* end);

#ifdef __cplusplus
}
#endif
#endif /* VOXHIP_H */
