// vx_internal.h -- launch interface between the C ABI (vx_api.cpp) and the gfx950 kernels (vx_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vx_math.h"
#include "../../include/voxhip.h"

namespace vx {

// De-indexed triangle + its candidate voxel box, written once by k_tri_setup and read by every later pass.
// 48 B, 16-B aligned: three dwordx4 loads.
struct __attribute__((aligned(16))) TriRec {
    float v[9];     // v0.xyz v1.xyz v2.xyz                      loadPos, VoxelBuilder.hpp:356-362
    uint32_t xr;    // start | count << 16 along x               candidate range, VoxelBuilder.hpp:175-184
    uint32_t yr;
    uint32_t zr;
};
static_assert(sizeof(TriRec) == 48, "TriRec must be 48 bytes");

// Cells per axis: the reference's grids are bounded by memory only, its Octree by 21 Morton bits per axis (octTree.hpp:583-585);
// candidate ranges are kept as 16 + 16 bits per axis in TriRec plus 5 + 6 high bits in a per-triangle extension word (vx_math.h,
// range_ext).  The limit is inclusive: a triangle may span all 2^21 cells of an axis.
constexpr uint32_t kMaxDim = 1u << 21;
constexpr uint32_t kCoarse = 8;        // cells per brick edge (ray traversal structure)
constexpr uint32_t kCoarseShift = 3;
// the traversal structure's block level (level-2 mip, k_walk's and k_multihit's block slabs): 4^3 bricks = 32^3 cells per block
constexpr uint32_t kBlockBricks = 4;   // bricks per block edge
constexpr uint32_t kBlockBricksShift = 2;
constexpr uint32_t kBlockCells = kBlockBricks * kCoarse;   // cells per block edge
constexpr uint32_t kBlockCellsShift = kBlockBricksShift + kCoarseShift;
static_assert(kBlockBricks == 1u << kBlockBricksShift && kCoarse == 1u << kCoarseShift && kBlockCells == 32u, "block and brick edges are powers of two");
constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;          // elements per thread in the scan kernels
constexpr int kScanTile = kScanBlock * kScanItems;

struct Camera { float viewInv[16]; float projInv[16]; uint32_t width, height; };

// ---- optional per-kernel event timing (vx_prof.cpp) ----------------------------------------------------------
void prof_enable(bool on);
void prof_select(const char* name);  // nullptr/"" = all kernels
bool prof_enabled();
void prof_reset();
int prof_read(int slot, char* name, size_t cap, double* ms, uint64_t* n);
struct ProfScope {
    ProfScope(const char* name, hipStream_t s);
    ~ProfScope();
    const char* name_;
    hipStream_t s_;
    hipEvent_t a_;
};
// every kernel launch goes through here so that the optional event profiler sees it
#define VX_KL(kern, grid, block, shmem, stream, ...)                         \
    do {                                                                     \
        ProfScope ps_(#kern, stream);                                        \
        hipLaunchKernelGGL(kern, grid, block, shmem, stream, __VA_ARGS__);   \
    } while (0)

// ---- launchers (all asynchronous on `s`) ------------------------------------------------------------------
// K1: bbox of all vertices with the reference's first-occurrence tie rule; out6 = min xyz, max xyz (device).
// state7: self-cleaning reduction state (initialise ONCE with bbox_state_init); out6 may point to pinned host memory;
// zero64 (optional): the per-build setVoxel-call counters (kCallCounters of them, one per 64-byte line), cleared by the kernel.
constexpr unsigned long long kScanTotalSat = (1ull << 40) - 1ull;  // where a posted total saturates (vx_kernels.hip, THE TOTAL)
constexpr uint32_t kCallCounters = 64;  // k_voxelize's waves add to counter (wave index % 64): entry [8 * i] of the array
// dgrid (optional, device memory): origin = bbox min and dims = ceil((max - min) / vs) as the host will derive them, for kernels
// queued behind K1 before the host has read the bbox.
struct DevGrid {
    float org[3];
    uint32_t dim[3];
    uint32_t pad[2];
};
void bbox_state_init(unsigned long long state7[7]);
void launch_bbox(const float* verts, uint64_t nverts, unsigned long long* state7, float* out6, unsigned long long* zero64, hipStream_t s,
                 float vs = 1.0f, DevGrid* dgrid = nullptr,
                 unsigned long long* tag_out = nullptr /*optional, host mailbox word: receives `tag` once out6 is complete, for a host that polls*/,
                 unsigned long long tag = 0);

// K2a: per-triangle record + number of row-segment work units; zlo/zhi clamp the candidate box to a z slab.
void launch_tri_setup(const float* verts, const int32_t* idx, uint64_t tri_begin, uint32_t ntri, const GridParams& g,
                      int sat_variant, uint32_t zlo, uint32_t zhi, TriRec* recs, uint32_t* units, hipStream_t s, const DevGrid* dgrid = nullptr,
                      void* clear = nullptr /*optional: a 16-byte aligned buffer the kernel zeroes beside its own work*/, uint64_t clear_bytes = 0,
                      uint64_t shard_wb = 0, uint64_t shard_we = 0 /*with dgrid: derive zlo / zhi on the device from the word shard (0, 0: whole grid)*/,
                      uint32_t* ext = nullptr /*optional, ntri words: bits 16..20 of the range values, for grids with an axis above 65535 cells*/,
                      uint32_t shard_rank = 0, uint32_t shard_world = 0 /*with dgrid and world > 1: the word shard vx_shard_words gives that rank*/);

// exclusive scan of n uint32 (or of their popcounts) into out[0..n] (out[n] = total mod 2^32, saturating check via *total64)
// *total64: exact below 2^40 - 1, then at least 2^40 - 1 and below 2^48 (vx_kernels.hip, THE TOTAL): a caller refuses a total >= 0xFFFFFFFF.
size_t scan_tmp_bytes(uint64_t n);
// path: kScanPathAuto = single-pass; the other two choose in the call (test aid).
// Unaligned in / out take the three-pass path whatever `path` says.
constexpr int kScanPathAuto = 0, kScanPathOne = 1, kScanPathThree = 2;
// launch_scan_u32's optional arguments
struct ScanArgs {
    bool tmp_is_zero = false;          // the caller guarantees tmp (scan_tmp_bytes(n)) is all zero; the scan leaves it all zero again
    // (bits 48..63 only) OR-ed into *total64 by the single-pass kernel, so that a host polling a pinned mailbox word can tell this scan's
    // total from an older one (the three-pass path applies no tag: *total64 is the bare total)
    unsigned long long total_tag = 0;
    uint32_t* sel1024 = nullptr;       // optional (single-pass kernel only, values <= 1024): sel1024[c] = the element whose range holds c * 1024
    uint32_t gen = 0;                  // generation mode (vx_kernels.hip): the number of this scan on `tmp`, 1, 2, 3 ... < 2^22; 0 = tickets + self-cleaning state
    uint32_t* group16 = nullptr;       // optional (single-pass kernel only): group16[i] = out[16 i], n / 16 + 1 entries -- a dense array small
                                       // enough to stay in L2 for readers that gather (k_rank)
    int path = kScanPathAuto;
};
// what a launcher answers: the path the scan took (three_pass: no tag in *total64, no sel1024 / group16 output)
enum class ScanTaken { three_pass, ticket, generation };
ScanTaken launch_scan_u32(const uint32_t* in, uint32_t* out, uint64_t n, bool popcount_input, void* tmp, unsigned long long* total64, hipStream_t s,
                          const ScanArgs& a = ScanArgs());

// clears the bits past nvox in the last word of a bitmask of nvox cells (nothing to do when nvox is a multiple of 32)
void launch_mask_tail(uint32_t* words, uint64_t nvox, hipStream_t s);

ScanTaken launch_scan_u8(const uint8_t* in, uint32_t* out, uint64_t n, void* tmp /*scan_tmp_bytes(n), all zero*/, unsigned long long* total64, hipStream_t s,
                         unsigned long long total_tag = 0, uint32_t gen = 0);

// The unit pipeline as its readers see it: k_tri_setup's records, the exclusive scan of the unit counts (ntri + 1 entries), per 256-unit
// block the triangle of its first unit (launch_unit_blocks; enables LDS staging) and the extension words of the candidate ranges (null
// unless an axis has more than 65535 cells).  The first argument of every launcher that walks the units.
struct Units {
    const TriRec* recs = nullptr;
    const uint32_t* unit_base = nullptr;
    const uint32_t* block_tri = nullptr;
    uint32_t ntri = 0;
    const uint32_t* ext = nullptr;
};
// launch_unit_blocks' optional arguments
struct UnitBlockArgs {
    uint32_t cap_blocks = 0xFFFFFFFFu;              // the kernel never writes at or beyond this entry of block_tri
    const unsigned long long* fwd_src = nullptr;    // optional: *fwd_dst = *fwd_src, the unit scan's total on its way from device memory to
    unsigned long long* fwd_dst = nullptr;          // the host's mailbox
    uint32_t* zero_hits = nullptr;                  // optional: entries [nUB, zero_n) of the voxelizer's block_hits are zeroed (zero_n at most
    uint32_t zero_n = 0;                            // the blocks this launch covers)
};
// block_tri (u.block_tri is not read): the table to write
void launch_unit_blocks(const Units& u, uint32_t total_units, uint32_t* block_tri, hipStream_t s, const UnitBlockArgs& a = UnitBlockArgs());
// K2: triangle/voxel overlap over all work units; ORs hits into `words` (only words in [wb,we)), optionally
// stores each unit's 32-bit hit mask (unit_mask) for the ordered emitters; adds the hit count to *set_calls.
struct VoxelizeArgs {
    uint32_t* block_hits = nullptr;                    // with unit_mask: hits per block of 64 units, (U + 63) / 64 entries -- what
                                                       // launch_emit_units' block_base is the exclusive scan of
    bool tiled = false;                                // `words` is the tiled build mask (tiled_mask_words(dim) words, dim[0] % 32 == 0, whole
                                                       // grid): launch_untile then writes the reference's bitmask
    const unsigned long long* units_total = nullptr;   // a launch queued before the host knows the unit total: the scan's 64-bit total in
                                                       // device memory; the kernel does nothing when it exceeds unit_cap
    uint32_t unit_cap = 0;                             // the units unit_mask / block_hits / block_tri were sized for
};
void launch_voxelize(const Units& u, const GridParams& g, int sat_variant, uint32_t* words, uint64_t wb, uint64_t we, uint32_t* unit_mask,
                     unsigned long long* set_calls, hipStream_t s, const VoxelizeArgs& a = VoxelizeArgs());
uint64_t tiled_mask_words(const uint32_t dim[3]);
void launch_untile(const uint32_t* tiled, uint32_t* words, const uint32_t dim[3], hipStream_t s, uint64_t wb = 0, uint64_t we = ~0ull /*the words the build owns: the others are written as zero*/);

// K3: VoxelGridVec / Octree emitters: one output per set bit of unit_mask, in unit order (== reference order).  block_base[b] = position of
// the first hit of units [64 b, 64 b + 64): the exclusive scan of launch_voxelize's block_hits.
void launch_emit_units(const Units& u, const GridParams& g, const uint32_t* unit_mask, const uint32_t* block_base, vx_aabb* aabbs, uint64_t* morton,
                       hipStream_t s, uint64_t cap = ~0ull);

// Per-voxel material ids (the reference's commented-out addMatrialIfNeeded plumbing): pass 1 = last triangle per occupied voxel
// (last_tri[rank], zeroed by the caller; may be null for the Vec flavour) + tri_hit[t] = 1 for triangles that set a voxel (zeroed by
// the caller); pass 2 = triangle -> material value -> index of first use.
void launch_mat_last(const Units& u, const GridParams& g, const uint32_t* unit_mask, const uint32_t* words, const uint32_t* word_prefix, uint32_t* last_tri,
                     uint8_t* tri_hit, hipStream_t s);
void launch_mat_ids(const uint32_t* last_tri, uint64_t n, const int32_t* tri_value, const int16_t* value_index, int16_t* out, hipStream_t s);
void launch_mat_ids_calls(const Units& u, const uint32_t* unit_mask, const uint32_t* block_base, const int32_t* tri_value, const int16_t* value_index,
                          int16_t* out, hipStream_t s);

// K4: bitmask -> ordered AABB list (word_prefix = exclusive scan of popcounts, nwords+1 entries)
void launch_emit_bool_aabbs(const uint32_t* words, const uint32_t* word_prefix, const GridParams& g, vx_aabb* out,
                            uint64_t capacity, hipStream_t s, const uint32_t* sel1024 = nullptr /*from the prefix scan: the word of every 1024th record*/);
// AABBs from sorted Morton items (Octree::getAabbs)
void launch_emit_morton_aabbs(const uint64_t* items, uint64_t n, const float root_min[3], float vs, vx_aabb* out, hipStream_t s);

// ---- K6: first hit per ray (vx_walk.hip) and the structure it walks --------------------------------------------------------
// Traversal structure = the analogue of the reference's BLAS build (hello_vulkan.cpp:737-760), three levels:
//   bricks3  the bitmask re-tiled brick-major (8^3 cells) in three orientations, one per possible major axis of a ray:
//            bricks3[ori][brick][slab along ori], ori 0 x / 1 y / 2 z; orientation 2 holds bit y*8+x per z slab, orientation 0
//            bit z*8+y per x slab, orientation 1 bit x*8+z per y slab
//   w1       one bit per brick (dims d1), x-fastest;   w2: one bit per block of kBlockBricks^3 bricks (dims d2)
// (m1 given and bdim[0] % 64 == 0: the brick kernel writes the level-1 mip itself, leaves empty bricks unwritten and returns true)
struct BricksArgs {
    const uint32_t* tiled = nullptr;                   // the voxelizer's tiled build mask (dim[0] % 32 == 0): the source instead of `words`, and
                                                       // `words` is WRITTEN from it -- launch_untile's job done on the way
    uint32_t* line_cnt = nullptr;                      // with `tiled`, dim[0] % 512 == 0 (so every 16-word line of the bitmask lies in one row): the
                                                       // set bits per line, nwords / 16 counts; their exclusive scan is word_prefix[16 i]
    const unsigned long long* hit_counters = nullptr;  // optional: k_voxelize's kCallCounters spread counters, complete on `s`
    unsigned long long* hits_out = nullptr;            // with hit_counters: receives hits_tag | their sum (THE TOTAL's contract) as the kernel starts
    unsigned long long hits_tag = 0;
};
bool launch_build_bricks3(const uint32_t* words, const uint32_t dim[3], const uint32_t bdim[3], unsigned long long* bricks3, uint32_t* m1, hipStream_t s,
                          const BricksArgs& a = BricksArgs());
void launch_brick_mip1(const unsigned long long* bricks_z /*orientation 2*/, uint64_t nbricks, uint32_t* m1, hipStream_t s);
void launch_build_mip2(const uint32_t* m1, const uint32_t d1[3], const uint32_t d2[3], uint32_t* m2, hipStream_t s);
// the level-2 mip and the exclusive scan of n uint32 (launch_scan_u32 on a generation-managed, zero-between-scans tmp) in one launch
ScanTaken launch_mip2_scan(const uint32_t* m1, const uint32_t d1[3], const uint32_t d2[3], uint32_t* m2, const uint32_t* in, uint32_t* out, uint64_t n, void* tmp,
                           unsigned long long* total64, hipStream_t s, unsigned long long total_tag, uint32_t gen);
struct TraceMips {
    const unsigned long long* bricks3;
    const uint32_t* w0;                // the reference-layout bitmask (primitive rank only)
    const uint32_t* w1;
    const uint32_t* w2;
    uint32_t d1[3];
    uint32_t d2[3];
};
struct TraceIO {
    const float* rays = nullptr;         // 6 f32 per ray, or null with cam
    const Camera* cam = nullptr;         // primary rays generated in-kernel (host copy)
    const Camera* cam_dev = nullptr;     // the same camera in device memory (filled in by the API layer)
    uint64_t nrays = 0;
    float tmin = 0.001f, tmax = 10000.0f;
    const float* tmax_per_ray = nullptr; // optional per-ray tMax
    bool any_hit = false;                // terminate on the first accepted hit (shadow query)
    float* t_out = nullptr;
    uint32_t* prim_out = nullptr;
    float* normal_out = nullptr;         // 3 f32 per ray: cube-face normal (zero for misses)
    uint8_t* shadowed_out = nullptr;     // 1 = some accepted hit
    vx_hit* hits = nullptr;
    unsigned long long* nhits = nullptr;
};
// voxel indices of the hits travel from the walk to the rank pass as 32-bit words when they fit (all ones = miss)
inline bool trace_idx32(const GridParams& g) { return g.nvox < 0xFFFFFFFFull; }
inline size_t trace_idx_bytes(const GridParams& g, uint64_t nrays) { return (size_t)nrays * (trace_idx32(g) ? 4 : 8) + 8; }
// The ray kernel's work queue, for whoever wants to start something when it runs dry (hipStreamWaitValue64 on another stream): the device
// word the kernel's waves draw their chunks of rays from and the value it has reached when the last chunk is out -- from then on the launch
// only drains (0: the static first chunks cover the batch).  Batches of more than 2^31 rays: the last launch's.
struct WalkQueue {
    unsigned long long* counter = nullptr;
    unsigned long long dry_at = 0;
};
void launch_queue_gate(const WalkQueue& q, hipStream_t s);  // vx_trace.hip: holds `s` until the kernel's first wave has drawn from q (300 us bound)
// The chunk ring of the ray kernel's rank epilogue: a batch that wants t + prim and nothing else, on a grid with 32-bit voxel indices, is
// ranked by the waves of k_walk themselves as they leave (no k_rank launch).  Every wave remembers the chunks of rays it drew from the work
// queue in `cap` words of its own.  walk_ring_cap decides ONCE per batch (the API layer calls it and carries the answer in WalkRing): the
// entries per wave for a batch of nrays and, in *waves, the waves of its launch; 0: the batch keeps k_rank (more than one launch, or no ring
// of a sane size holds its chunks).  VOXHIP_TRACE_RING=<entries> overrides the choice (0: k_rank); whether waves * cap chunks cover the
// batch still decides.
uint32_t walk_ring_cap(uint64_t nrays, uint32_t* waves);
struct WalkRing {
    uint32_t* words = nullptr;   // waves * cap words of device memory; contents are scratch
    uint32_t cap = 0;            // walk_ring_cap's answer for this batch ...
    uint32_t waves = 0;          // ... and the waves it counted on
};
struct WalkRank {  // what launch_walk's epilogue ranks with and where to
    const uint32_t* words = nullptr;        // the reference-layout bitmask
    const uint32_t* word_prefix = nullptr;  // its word prefix, and / or ...
    const uint32_t* prefix16 = nullptr;     // ... every 16th entry of it, dense (nwords % 16 == 0)
    uint32_t* prim_out = nullptr;
    WalkRing ring;
};
// Returns false when an output that was asked for could not be queued: a ring was given (so the caller kept no t for k_rank) and the ray
// kernel declined the epilogue -- the caller's sizing and the launch disagree, an internal error.
bool launch_trace(const GridParams& g, const TraceMips& mips, const uint32_t* word_prefix, const TraceIO& io, unsigned long long* counters /*2 device words, zero before the first trace; they alternate*/, int* phase /*host*/,
                  void* idx_tmp /*trace_idx_bytes when ranks / normals / the hit list are wanted*/, hipStream_t s,
                  const uint32_t* prefix16 = nullptr /*optional: launch_scan_u32's group16 of word_prefix*/, WalkQueue* queue = nullptr,
                  const WalkRing* ring = nullptr /*walk_ring_cap's ring for this batch: t + prim batches are ranked inside k_walk*/);

// Multi-hit queries (vx_hitlist.h; the grid in vx_multihit.hip, the octree in vx_octmulti.hip, the mesh in vx_meshmulti.hip): per ray the
// first K (1..32) accepted primitives in (t, prim) order -- (t, instance, prim) on a TLAS -- into io.t_out / io.prim_out / bary / instance (K
// entries per ray, ray-major, padded with -1 / all ones / (0, 0); all optional) and the number of all accepted primitives into count
// (optional); after_*: the optional per-ray cursor.  bary: the mesh only; instance, after_instance: the TLAS only.  io's other outputs are
// not written.
struct MultiIO {
    uint32_t K = 0;
    uint32_t* count = nullptr;
    float* bary = nullptr;
    uint32_t* instance = nullptr;
    const float* after_t = nullptr;
    const uint32_t* after_instance = nullptr;
    const uint32_t* after_prim = nullptr;
};
// On the grid: io as for launch_octree_trace (cam_dev, not cam).  mips.bricks3 or word_prefix null: every ray misses.
void launch_multihit(const GridParams& g, const TraceMips& mips, const uint32_t* word_prefix, const TraceIO& io, const MultiIO& m, hipStream_t s);

// First hit per ray against the octree's AABB list by descending its node array (vx_octrace.hip).  io as for launch_trace (cam_dev, not cam;
// prim = index in vx_octree_aabbs order); nodes may be null / nitems 0: every ray misses.
void launch_octree_trace(const vx_octree_node* nodes, const uint64_t* items, uint64_t nitems, uint32_t bits, const float root_min[3], float vs, const TraceIO& io,
                         hipStream_t s);
// Multi-hit query on the octree, over the runs of equal codes of the item list (a run is one voxel, prim = its first list index).  nodes /
// items / nitems as for launch_octree_trace.
void launch_octree_multihit(const vx_octree_node* nodes, const uint64_t* items, uint64_t nitems, uint32_t bits, const float root_min[3], float vs, const TraceIO& io,
                            const MultiIO& m, hipStream_t s);

// Triangle BVH (vx_bvh.hip).  Build, all on `s`: launch_bvh_prep (box6 = ordered-uint bounds of all triangles, initialised to ~0 x3 / 0 x3;
// *err |= 1 when an index leaves [0, nv); keys = Morton code << 32 | triangle), launch_sort_u64 over 62 bits, launch_bvh_tree (radix tree,
// bottom-up bounds + heights into kbox (2n-1 records of 32 B), the de-indexed triangles in leaf order into tris (48 B each: (v0, triangle
// index), (v1, 1 when the triangle is on the side list `ill`, else 0), (v2, 0)), the survivors of
// the collapse into alive[2n-1]), an exclusive scan of alive into newidx, launch_bvh_emit (the node array, 32 B per node, root at 0).
void launch_bvh_prep(const float* v, const int32_t* idx, uint64_t nv, uint32_t ntri, uint32_t* box6, uint32_t* err, uint64_t* keys, hipStream_t s);
void launch_bvh_tree(const float* v, const int32_t* idx, uint64_t nv, uint32_t n, const uint64_t* keys, uint32_t max_leaf, uint32_t* child,
                     uint32_t* parent, uint32_t* range, uint32_t* arrived, float* kbox, float* tris, uint32_t* alive,
                     uint32_t* ill /*n entries: the ill-conditioned triangles' leaf-order positions*/, uint32_t* nill /*zeroed by the caller*/, hipStream_t s);
void launch_bvh_emit(uint32_t n, const uint32_t* alive, const uint32_t* newidx, const uint32_t* child, const uint32_t* range, uint32_t max_leaf,
                     const float* kbox, float* nodes, hipStream_t s);
// First hit per ray on the BVH: io as for launch_octree_trace (cam_dev, not cam; prim = triangle index); bary_out optional (2 f32 per ray).
// height: the tree's height (LDS stack entries); extent (the largest side of the root box) and coord_max (the largest |coordinate| of the
// mesh) size the traversal's box widening.
void launch_bvh_trace(const float* nodes, const float* tris, const uint32_t* ill, uint32_t nill, uint32_t ntri, uint32_t height, float extent,
                      float coord_max, const TraceIO& io, float* bary_out, hipStream_t s);

// Instanced scenes (vx_tlas.hip).  One record per BLAS of a TLAS, re-read from its vx_bvh at every build / update: node and triangle arrays,
// side list, triangle count (0: instances of it are inactive), the box widening of its traversal and its root box.
struct TlasBlas {
    const float* nodes;
    const float* tris;
    const uint32_t* ill;
    uint32_t nill;
    uint32_t ntri;
    float pad;
    float rmin[3], rmax[3];
    uint32_t height;
};
// Build / update, all on `s`: launch_tlas_prep (xf / w2o: 12 f32 per instance, iblas, ibox: 2 float4 per instance, small[0..6] initialised
// to ~0 x3 / 0 x4, keys), launch_sort_u64 over 62 bits, launch_tlas_tree (nodes: 2n-1 vx_bvh_node records, hgt: 2n-1 heights, small[7] =
// the root's height).  n >= 1.
void launch_tlas_prep(const vx_instance* in, uint32_t n, const TlasBlas* tab, uint32_t nb, float* xf, float* w2o, uint32_t* iblas, float* ibox,
                      uint32_t* small, uint64_t* keys, hipStream_t s);
void launch_tlas_tree(uint32_t n, const uint64_t* keys, const float* ibox, uint32_t* child, uint32_t* parent, uint32_t* range, uint32_t* arrived,
                      float* nodes, uint32_t* hgt, uint32_t* small, hipStream_t s);
void launch_bvh_karras(const uint64_t* keys, uint32_t n, uint32_t* child, uint32_t* parent, uint32_t* range, hipStream_t s);  // vx_bvh.hip
// the upper bound of a TLAS's height over n instances that the trace's stack is sized to: min(n - 1, 30 + ceil(log2 n))
uint32_t tlas_height_bound(uint64_t n);
float bvh_pad(float extent, float coord_max);  // vx_bvh.hip: the box widening launch_bvh_trace applies
// the BLAS table (nb records) written on `s` from kernel arguments
void launch_tlas_table(const TlasBlas* host, uint32_t nb, TlasBlas* dev, hipStream_t s);
struct TlasDev {
    const float* nodes = nullptr;
    const float* w2o = nullptr;
    const float* xf = nullptr;
    const uint32_t* iblas = nullptr;
    const TlasBlas* tab = nullptr;
    const uint32_t* small = nullptr;
    uint32_t ninst = 0;
    uint32_t levels = 1;
};
// First hit per ray on the instances: io as for launch_bvh_trace (prim = triangle index in its mesh, normal = the world geometric normal);
// bary_out (2 f32 per ray) and inst_out (instance, kNone on a miss) optional.
void launch_tlas_trace(const TlasDev& T, const TraceIO& io, float* bary_out, uint32_t* inst_out, hipStream_t s);
float tlas_ray_pad();  // vx_tlas.hip: the per-ray widening of every TLAS box test, per unit of cond_max |o|

// Multi-hit queries on the mesh: io as for launch_bvh_trace, the remaining arguments launch_bvh_trace's / launch_tlas_trace's.
void launch_bvh_multihit(const float* nodes, const float* tris, const uint32_t* ill, uint32_t nill, uint32_t ntri, uint32_t height, float extent,
                         float coord_max, const TraceIO& io, const MultiIO& m, hipStream_t s);
void launch_tlas_multihit(const TlasDev& T, const TraceIO& io, const MultiIO& m, hipStream_t s);

#if defined(__HIPCC__)
// The unit geometric normal of triangle k (leaf-order position in its BLAS) of instance inst in WORLD space: vertices M*v in the pinned
// association ((m0*x + m1*y) + m2*z) + m3 per row, then e1, e2, cross(e1, e2) / sqrt(dot) as vx_bvh computes it.
__device__ __forceinline__ void tlas_world_normal(const TlasBlas* tab, const uint32_t* iblas, const float* xf, uint32_t inst, uint32_t k, float& n0,
                                                  float& n1, float& n2)
{
    const float4* t = reinterpret_cast<const float4*>(tab[iblas[inst]].tris) + 3ull * k;
    const float* m = xf + 12ull * inst;
    float p[9];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const float4 q = t[v];
#pragma unroll
        for (int r = 0; r < 3; ++r) p[3 * v + r] = ((m[4 * r] * q.x + m[4 * r + 1] * q.y) + m[4 * r + 2] * q.z) + m[4 * r + 3];
    }
    const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
    const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float il = 1.0f / sqrtf((cx * cx + cy * cy) + cz * cz);
    n0 = cx * il; n1 = cy * il; n2 = cz * il;
}
#endif

// Frames (vx_render.hip): the per-pixel stages of vx_render_frame_device around the traversals.  n = width * height pixels, pixel
// r = py * width + px.  Hit arrays as the traversals write them (mt / mprim / mnrm / mbary null without a mesh); srays (6 f32 per pixel),
// sdist (the light distance, for the shading's 1/d^2) and stmax (the shadow ray's tMax: sdist, with 0 where no shading reads the shadow
// flag) are written by the shadow-ray stage; sv / sm (optional) are the two shadow queries.
// the mesh of each BLAS of an instanced scene (vx_render_create_tlas): vertices, index triples, per-triangle material ids (null: none)
// and its material table
struct InstMesh {
    const float* verts;
    const int32_t* idx;
    const int32_t* mids;
    const vx_material* mat;
    uint64_t nmat;
};
struct RenderParams {
    uint64_t n = 0;
    const Camera* cam = nullptr;
    const float* vt = nullptr;
    const uint32_t* vprim = nullptr;
    const float* vnrm = nullptr;
    const float* mt = nullptr;
    const uint32_t* mprim = nullptr;
    const float* mnrm = nullptr;
    const float* mbary = nullptr;
    const float* verts = nullptr;   // the mesh (device): vertices and index triples
    const int32_t* idx = nullptr;
    float light[3] = {0, 0, 0};
    float intensity = 0.f;
    int light_type = 0;             // 0 point, 1 directional
    float* srays = nullptr;
    float* sdist = nullptr;
    float* stmax = nullptr;
    const uint8_t* sv = nullptr;
    const uint8_t* sm = nullptr;
    const int16_t* vids = nullptr;  // per-voxel material ids (vx_grid_material_ids_device), nvids of them; null: MaterialObj{}
    uint64_t nvids = 0;
    const vx_material* vmat = nullptr;
    uint64_t nvmat = 0;
    const int32_t* mids = nullptr;  // per-triangle material ids (-1 none); null: MaterialObj{}
    const vx_material* mmat = nullptr;
    uint64_t nmmat = 0;
    // instanced scenes (inst: the _tlas kernels): the hit's instance per pixel, the instances' object-to-world rows (12 f32 each), their BLAS,
    // and the mesh of each BLAS; vt may be null (no voxel source: every voxel query misses)
    const uint32_t* minst = nullptr;
    const float* ixf = nullptr;
    const uint32_t* iblas = nullptr;
    const InstMesh* imesh = nullptr;
    uint32_t* rgba = nullptr;
    uint8_t* kind_out = nullptr;
    uint8_t* shadowed_out = nullptr;
};
void launch_render_camera(const Camera& cam, Camera* dev, hipStream_t s);  // one thread: the camera block, from a kernel argument
// Attribute shading (vx_render_set_shading(VX_RENDER_ATTRIBUTES)): what a triangle hit reads besides RenderParams, per mesh (one record for a
// BVH scene, one per BLAS of an instanced scene): corner normals (9 f32 per triangle, null: the face normal), corner uvs (6 f32 per triangle,
// null: (0, 0)), the texture slot of every material (nslot of them) and the mesh's textures (ntex records into the scene's texel pool).
struct TexRec {
    uint64_t offset;  // first texel (RGBA8 as uint32, R in the low byte) in the pool, rows top first
    uint32_t w, h;
};
struct AttrMesh {
    const float* nrm;
    const float* uv;
    const int32_t* slot;
    uint64_t nslot;
    const TexRec* tex;
    uint32_t ntex;
    uint32_t pad;
};
struct AttrParams {
    const AttrMesh* mesh = nullptr;  // [0] in a BVH scene, [iblas[inst]] in an instanced one
    const uint32_t* texels = nullptr;
    const float* srgb = nullptr;     // 256 f32: the sRGB EOTF of c / 255, computed in float64 and rounded
    const float* w2o = nullptr;      // instanced scenes: the TLAS's world-to-object rows (12 f32 per instance)
    float* nbuf = nullptr;           // 3 f32 per pixel: the normal of a triangle hit, written by the shadow-ray stage, read by the shading
};
// The two per-pixel stages, each one of four kernels.  A: attribute shading's tables, null for the default shading; inst: an instanced scene,
// whose triangle hit point is M * ((p0*b0 + p1*b1) + p2*b2) and whose materials are the instance's mesh's.
void launch_render_shadow_rays(const RenderParams& P, const AttrParams* A, bool inst, hipStream_t s);
void launch_render_shade(const RenderParams& P, const AttrParams* A, bool inst, hipStream_t s);

// single-voxel helpers
void launch_set_bit(uint32_t* words, uint64_t idx, hipStream_t s);

// Solid voxelization (vx_solid.hip): the exterior of the mask grown from the boundary's empty cells in rounds, then H = empty & ~exterior.
// Padded layout: W words per (y, z) row, pwords in all; `padded` is false when X % 32 == 0 (the reference's bitmask is that layout).
struct SolidPlan {
    uint32_t W = 0;
    bool padded = false;
    uint64_t pwords = 0;
};
SolidPlan solid_plan(const uint32_t dim[3]);
// mp (padded only, pwords): the padded mask; ext (pwords): the exterior's seed; *flag = 1 (the flag the first round reads)
void launch_solid_seed(const uint32_t* words, uint32_t* mp, uint32_t* ext, const uint32_t dim[3], uint32_t* flag, hipStream_t s);
// one round (x, y, z sweeps) over the padded mask m (mp, or the bitmask when not padded); every kernel exits at once when *prev_flag == 0 and
// sets *flag = 1 when it grows the exterior; agg: solid_agg_words(dim) words of scratch (the column scans' per-chunk words)
uint64_t solid_agg_words(const uint32_t dim[3]);
void launch_solid_round(const uint32_t* m, uint32_t* ext, uint32_t* agg, const uint32_t dim[3], const uint32_t* prev_flag, uint32_t* flag, hipStream_t s);
// *out = tag | (number of the nrounds flags that are set)
void launch_solid_report(const uint32_t* flags, uint32_t nrounds, unsigned long long* out, unsigned long long tag, hipStream_t s);
// words |= H; H in the reference's layout into h (padded) or over ext (not padded: h unused)
void launch_solid_finish(uint32_t* words, const uint32_t* mp, uint32_t* ext, uint32_t* h, const uint32_t dim[3], uint64_t nwords, hipStream_t s);
// ids[i] = v for i < n (only_unset: only where ids[i] < 0)
void launch_solid_ids(int16_t* ids, uint64_t n, int16_t v, bool only_unset, hipStream_t s);

// Distance fields (vx_distance.hip): x pass from the bitmask, then an exact lower envelope per y and per z column, in place in buf (N = X*Y*Z
// values).  mode 0: D_out, 1: D_in, 2: the signed field (buf ends as f32, vs the voxel size).  stk: distance_stack_entries(dim, mode == 2)
// entries of scratch (the envelopes' stacks, [k][column]).
uint64_t distance_stack_entries(const uint32_t dim[3], bool is_signed);
void launch_distance(const uint32_t* words, const uint32_t dim[3], int mode, float vs, uint32_t* buf, uint2* stk, hipStream_t s);
// The feature transform (vx_distance.hip): the same passes carrying the nearest target itself; buf (N values, in place) ends as the cell
// index of the nearest occupied (inside: empty) cell, 0xFFFFFFFF when there is none -- or, with values (N entries, not buf), as values[that
// index], `fill` when there is none.  N <= 0xFFFFFFFF and the distance fields' limit hold.  stk: distance_stack_entries(dim, false) entries.
void launch_nearest(const uint32_t* words, const uint32_t dim[3], bool inside, const uint32_t* values, uint32_t fill, uint32_t* buf, uint2* stk,
                    hipStream_t s);

// Queries on a snapshot S of the signed field (vx_field.hip; the arithmetic is vx_field.h's): the trilinear sample of n points (each output
// optional) and the sphere cast of a ray batch (device pointers; step_scale, hit_eps and max_steps with their defaults filled in).
struct FieldGeom;
struct FieldTraceIO {
    const float* rays;
    uint64_t nrays;
    float tmin, tmax;
    const float* tmax_per_ray;
    float radius;
    const float* radius_per_ray;
    float step_scale, hit_eps;
    uint32_t max_steps;
    float* t;
    float* clearance;
    uint32_t* steps;
    uint8_t* status;
};
void launch_field_sample(const float* S, const FieldGeom& G, const float* points, uint64_t n, float* value, float* gradient, uint8_t* occupied,
                         hipStream_t s);
void launch_field_trace(const float* S, const FieldGeom& G, const FieldTraceIO& io, hipStream_t s);

// Pose queries on the snapshot (vx_poses.hip; the arithmetic is vx_poses.h's).  Device pointers; keys / counts: nposes entries of scratch
// each, which the launch initialises itself where it merges into them; each output optional.  A body of more than 64 points is cut into
// chunks of kPoseChunk points that walk tiles of kPoseTile poses; a smaller one takes a group of lanes per pose, kPoseNarrowRounds poses
// per group and workgroup.  The shape does not show in the results.
constexpr uint32_t kPoseChunk = VX_FIELD_POSE_CHUNK, kPoseTile = VX_FIELD_POSE_TILE, kPoseNarrowRounds = 8;
struct FieldPoseIO {
    const float* points;
    uint32_t npoints;
    const float* radii;
    const float* transforms;
    uint64_t nposes;
    float margin;
    unsigned long long* keys;
    uint32_t* counts;
    float* clearance;
    uint32_t* point;
    uint32_t* count;
    float* position;
    float* gradient;
};
hipError_t launch_field_poses(const float* S, const FieldGeom& G, const FieldPoseIO& io, hipStream_t s);

// Morphology with the digital Euclidean ball (vx_morph.hip).  A domain: its cells and the bits from one (y, z) row to the next -- X for the
// reference's bitmask, 32 * ceil(X / 32) for a ROW-ALIGNED mask (morph_aligned_words(dim) words, padding bits zero).
struct MorphDom {
    uint32_t dim[3];
    uint64_t stride;
};
constexpr uint32_t kMorphInvIn = 1u;   // the source is complemented over the whole lattice (cells outside its domain become targets)
constexpr uint32_t kMorphInvOut = 2u;  // the result is complemented (inside the output domain)
// vx_morph_bit_radius(): the largest R the bit-level kernel takes; at most 32, so that a shift reaches only the neighbouring word.  Measured
// (tools/morph_time.py); -DVX_MORPH_BIT_RADIUS=n builds the library for that measurement.
#ifndef VX_MORPH_BIT_RADIUS
#define VX_MORPH_BIT_RADIUS 16
#endif
constexpr uint32_t kMorphBitRadius = VX_MORPH_BIT_RADIUS;
static_assert(kMorphBitRadius <= 32u, "the bit-level kernel stages one word of halo");
uint64_t morph_aligned_words(const uint32_t dim[3]);
// dst (row-aligned, odim) = the dilation by B(r2), R = isqrt(r2) <= 32, of src; output cell c reads the input around c + (shift, shift, shift).
// r2 = 0: a bit copy with an offset (pad / crop).  Both flags: the erosion.
void launch_morph_ball(const uint32_t* src, const MorphDom& in, uint32_t* dst, const uint32_t odim[3], int32_t shift, uint32_t r2, uint32_t flags, hipStream_t s);
// dst (the reference's layout, ceil(X*Y*Z / 32) words, tail bits zero) = aligned | orw (orw optional, the reference's layout)
void launch_morph_pack(const uint32_t* aligned, const uint32_t dim[3], const uint32_t* orw, uint32_t* dst, hipStream_t s);
// dst (the reference's layout) = field <= r2, or with erode: field > r2 and at least R cells from every border
void launch_morph_thresh(const uint32_t* field, const uint32_t dim[3], uint32_t r2, bool erode, uint32_t* dst, hipStream_t s);

// Surface mesh (vx_surface.hip): npts = (X+1)(Y+1)(Z+1) lattice points, nlw = ceil(npts / 32) corner words.
struct SurfacePlan {
    uint64_t npts = 0, nlw = 0;
};
SurfacePlan surface_plan(const GridParams& g);
// tcount (nwords): triangles of every mask word; cmask (nlw): the used lattice points, one bit each
void launch_surface_count(const uint32_t* words, const GridParams& g, const SurfacePlan& p, uint32_t* tcount, uint32_t* cmask, hipStream_t s);
// tpre / vpre: exclusive scans of tcount / of cmask's popcounts.  Positions (3 f32 per vertex), triangles (3 int32) and, with cell_mat
// (the per-occupied-cell ids, indexed through wprefix = the word prefix of the mask) and mat non-null, one id per triangle.
void launch_surface_emit(const uint32_t* words, const GridParams& g, const SurfacePlan& p, const uint32_t* tpre, const uint32_t* cmask,
                         const uint32_t* vpre, const uint32_t* wprefix, const int16_t* cell_mat, float* xyz, int32_t* tri, int32_t* mat,
                         hipStream_t s);
// the triangles and ids alone (k_surf_emit)
void launch_surface_tris(const uint32_t* words, const GridParams& g, const uint32_t* tpre, const uint32_t* cmask, const uint32_t* vpre,
                         const uint32_t* wprefix, const int16_t* cell_mat, int32_t* tri, int32_t* mat, hipStream_t s);
// Surface nets (vx_grid_surface_smooth*): per-vertex scratch carved from one block.  lat: lattice index; nb: the six neighbours' vertex
// indices, nb[d * V + v], -1 = none; u[2]: the offsets in cells, ping-pong; cfg: the 2x2x2 block configuration.
struct NetsBufs {
    void* base = nullptr;
    uint64_t* lat = nullptr;
    int32_t* nb = nullptr;
    float* u[2] = {nullptr, nullptr};
    uint8_t* cfg = nullptr;
};
// bytes of the block for V vertices; with b->base set, also the pointers into it
size_t nets_bytes(uint64_t V, NetsBufs* b);
// after the count and both scans (cmask, vpre, V known to the host): configuration and u0, `iterations` x (a step with lambda, a step with
// mu when mu != 0), the positions into xyz and, when normals is non-null, the vertex normals; all queued back to back on s
void launch_surface_nets(const uint32_t* words, const GridParams& g, const SurfacePlan& p, const uint32_t* cmask, const uint32_t* vpre,
                         uint64_t V, const NetsBufs& b, uint32_t iterations, float lambda, float mu, float* xyz, float* normals, hipStream_t s);

// Connected components (vx_components.hip), X*Y*Z <= 2^32 - 1.  launch_components: labels (X*Y*Z) receives parent = the smallest cell of
// the component for the occupied cells (empty slots untouched), roots (nwords) the root bitmask.  launch_components_label: rpre = the
// exclusive scan of the roots' popcounts; labels in place (0 for empty cells), and K into dev_count when non-null.
void launch_components(const uint32_t* words, const GridParams& g, bool conn26, uint32_t* labels, uint32_t* roots, hipStream_t s);
void launch_components_label(const uint32_t* words, const GridParams& g, uint32_t* labels, const uint32_t* roots, const uint32_t* rpre,
                             uint32_t* dev_count, hipStream_t s);
// rec: k records of vx_component (8 words each) from the labels
void launch_component_stats(const uint32_t* labels, const GridParams& g, uint64_t k, uint32_t* rec, hipStream_t s);

// device radix sort of uint64 keys (octree items; vx_sort.hip); tmp sized by sort_tmp_bytes.  The two key buffers ping-pong:
// returns 0 when the sorted keys end up in keys_a, 1 for keys_b (the other buffer is scratch afterwards).
size_t sort_tmp_bytes(uint64_t n);
int launch_sort_u64(uint64_t* keys_a /*in*/, uint64_t* keys_b, uint64_t n, int bits, void* tmp, size_t tmp_bytes, hipStream_t s);

// Octree node array, direct form (max_items <= kOctDirectMaxItems): per item position the number of nodes that START there
// (launch_oct_depths, bytes), an exclusive scan of those = the pre-order index of the first of them, then start / count / child links
// (launch_oct_nodes) into a node array the caller has filled with 0xFF bytes.
constexpr uint64_t kOctDirectMaxItems = 64;
void launch_oct_depths(const uint64_t* items, uint32_t nitems, uint32_t bits, uint32_t max_items, uint8_t* ncount, hipStream_t s);
void launch_oct_nodes(const uint64_t* items, uint32_t nitems, uint32_t bits, const uint32_t* base, vx_octree_node* nodes, hipStream_t s);

// Octree node array (pre-order, octTree.hpp:319-358), level by level (any max_items): per level launch_oct_count (children per node), an
// exclusive scan, launch_oct_emit (the next level's start / count, 8 child links per node in breadth-first ids, the depth); then
// launch_oct_keys, the sort of (key, id) pairs on 40 key bits (tmp: oct_sort_tmp_bytes), launch_oct_inverse and launch_oct_finalize,
// which writes the nodes in pre-order.  Sequenced by vx_api.cpp (octree_nodes_by_level).
void launch_oct_count(const uint64_t* items, const uint32_t* start, const uint32_t* count, uint32_t nnodes, uint32_t depth, uint32_t max_depth, uint32_t max_items,
                      uint32_t* nchild, hipStream_t s);
void launch_oct_emit(const uint64_t* items, uint32_t* start, uint32_t* count, uint32_t* children, uint8_t* depth_of, uint32_t level_off, uint32_t nnodes,
                     uint32_t depth, uint32_t max_depth, uint32_t max_items, const uint32_t* child_base, uint32_t next_off, hipStream_t s);
void launch_oct_keys(const uint32_t* start, const uint8_t* depth_of, uint32_t n, uint64_t* keys, uint32_t* ids, hipStream_t s);
size_t oct_sort_tmp_bytes(uint32_t n);
hipError_t launch_oct_sort(const uint64_t* keys, uint64_t* keys_out, const uint32_t* ids, uint32_t* order, uint32_t n, void* tmp, size_t tmp_bytes, hipStream_t s);
void launch_oct_inverse(const uint32_t* order, uint32_t n, uint32_t* newidx, hipStream_t s);
void launch_oct_finalize(const uint32_t* order, const uint32_t* newidx, const uint32_t* start, const uint32_t* count, const uint32_t* children, uint32_t n,
                         vx_octree_node* out, hipStream_t s);

}  // namespace vx
