// vx_api.cpp -- the C ABI declared in include/voxhip.h: handles, device-memory pool, launch sequencing.
// All compute happens in the kernels of vx_kernels.hip; there is no CPU compute path in this library.
#include "vx_internal.h"
#include "vx_field.h"

#include <cctype>
#include <cmath>
#include <limits>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#pragma clang fp contract(off)

#include "vx_obj.h"

namespace {

thread_local std::string g_err;
thread_local int g_device = 0;

vx_status fail(vx_status s, const std::string& m)
{
    g_err = m;
    return s;
}

#define VX_HIP(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e__ = (expr);                                                                           \
        if (e__ != hipSuccess) return fail(VX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
#define VX_TRY(expr)                 \
    do {                             \
        vx_status s__ = (expr);      \
        if (s__ != VX_OK) return s__; \
    } while (0)

// ---- pooled device memory: hipMalloc/hipFree are slow and synchronising, steady-state loops must not call them ----
// The pool is STREAM-ORDERED: a block goes back on the free list together with the stream its owner queued work on and an
// event recorded on that stream at the moment of the release.  It is handed out again at once to a request from the SAME
// stream (work queued later on that stream runs after the old owner's kernels), and to any other stream only once the
// event has completed -- so a block that kernels in flight still read or write is never given to a different handle
// (distinct handles on distinct threads with per-handle streams are allowed by voxhip.h).
constexpr int kMaxDev = 16;
struct FreeBlock {
    void* p;
    hipStream_t stream;
    hipEvent_t ev;  // null: nothing was in flight (never used, or released after a synchronize)
};
struct Pool {
    std::mutex mu;
    std::multimap<size_t, FreeBlock> free_blocks;
    std::unordered_map<void*, size_t> live;
    std::vector<hipEvent_t> spare_events;
};
Pool g_pool[kMaxDev];

size_t round_size(size_t b)
{
    if (b < 256) b = 256;
    if (b >= (1u << 20)) return (b + (2u << 20) - 1) / (2u << 20) * (2u << 20);
    size_t p = 256;
    while (p < b) p <<= 1;
    return p;
}

std::atomic<uint64_t> g_pool_requests{0};  // vx_device_allocations

// Poison mode (vx_pool_poison, a test aid): bit 32 = on, bits 0..31 = the pattern.  One word, so a worker thread of vx_multi never sees
// the switch without its pattern.
std::atomic<uint64_t> g_pool_poison{0};
std::atomic<uint64_t> g_pool_poisoned{0};  // vx_pool_poisoned_blocks

// A block about to be handed out, filled over its whole rounded size.  The fill is queued on the requesting stream and waited for: an owner
// that initialises its block with a synchronous copy (ensure_small) must not find a fill still queued on a non-blocking stream behind it.
hipError_t pool_poison_fill(void* p, size_t sz, uint32_t pattern, hipStream_t stream)
{
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)pattern, sz / 4, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) g_pool_poisoned.fetch_add(1, std::memory_order_relaxed);
    return e;
}

hipError_t pool_alloc(int dev, size_t bytes, void** out, hipStream_t stream)
{
    g_pool_requests.fetch_add(1, std::memory_order_relaxed);
    const uint64_t poison = g_pool_poison.load(std::memory_order_relaxed);
    const size_t sz = round_size(bytes);
    Pool& P = g_pool[dev];
    void* hit = nullptr;
    size_t hit_size = 0;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        for (auto it = P.free_blocks.lower_bound(sz); it != P.free_blocks.end() && it->first <= sz * 2; ++it) {
            FreeBlock& fb = it->second;
            if (fb.ev && fb.stream != stream && hipEventQuery(fb.ev) != hipSuccess) continue;  // still in flight on another stream
            if (fb.ev) P.spare_events.push_back(fb.ev);
            hit = fb.p;
            hit_size = it->first;
            P.live[hit] = hit_size;
            P.free_blocks.erase(it);
            break;
        }
    }
    if (hit) {
        *out = hit;
        return poison ? pool_poison_fill(hit, hit_size, (uint32_t)poison, stream) : hipSuccess;  // (outside the pool's lock: the fill waits)
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, sz);
    if (e != hipSuccess) {
        // drop the cache and retry once
        vx_release_cached_memory();
        e = hipMalloc(&p, sz);
        if (e != hipSuccess) return e;
    }
    {
        std::lock_guard<std::mutex> lk(P.mu);
        P.live[p] = sz;
    }
    *out = p;
    return poison ? pool_poison_fill(p, sz, (uint32_t)poison, stream) : hipSuccess;
}

// `in_flight`: work that touches the block may still be queued on `stream` (false: the caller has synchronized)
void pool_free(int dev, void* p, hipStream_t stream, bool in_flight)
{
    if (!p) return;
    Pool& P = g_pool[dev];
    hipEvent_t ev = nullptr;
    if (in_flight) {
        {
            std::lock_guard<std::mutex> lk(P.mu);
            if (!P.spare_events.empty()) { ev = P.spare_events.back(); P.spare_events.pop_back(); }
        }
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
        if (!ev || hipEventRecord(ev, stream) != hipSuccess) {
            // no event to order the reuse by: fall back to waiting for the stream
            (void)hipStreamSynchronize(stream);
            if (ev) { std::lock_guard<std::mutex> lk(P.mu); P.spare_events.push_back(ev); }
            ev = nullptr;
        }
    }
    std::lock_guard<std::mutex> lk(P.mu);
    auto it = P.live.find(p);
    if (it == P.live.end()) { if (ev) P.spare_events.push_back(ev); return; }
    P.free_blocks.emplace(it->second, FreeBlock{p, stream, ev});
    P.live.erase(it);
}

// Where a buffer lives: the device of its blocks and the stream its owner queues their work on (the pool orders reuse by it).  Every handle
// IS a Home (g->device, g->stream), a function's temporaries share a local one.  `drained`: the owner has synchronised the stream and queues
// nothing more -- its blocks go back without an event each (handle_free).  Not copyable: buffers point at it.
struct Home {
    int device;
    hipStream_t stream;
    bool drained;
    explicit Home(int d = 0, hipStream_t s = nullptr, bool is_drained = false) : device(d), stream(s), drained(is_drained) {}
    void before_free() {}  // handle_free's hook: what a handle type must settle before its stream is waited for (vx_grid)
    Home(const Home&) = delete;
    Home& operator=(const Home&) = delete;
};

// One pool block and its owner: a buffer is named once, where it is declared -- bound there to its Home, released by its destructor.  A
// move hands the block over and leaves the source empty; the target keeps its own Home.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    const Home* const home;
    bool fresh = false;  // set when ensure() handed out a new block (contents undefined); the owner clears it
    explicit DevBuf(const Home* h) : home(h) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), home(o.home), fresh(o.fresh) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap; fresh = o.fresh;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        release();
        hipError_t e = pool_alloc(home->device, bytes, &p, home->stream);
        if (e == hipSuccess) { cap = round_size(bytes); fresh = true; }
        return e;
    }
    // ensure() for an array that keeps its first `keep` bytes: a larger block (at least twice the old one) from the same Home, a copy on its
    // stream, and the old block goes back in flight -- the pool hands it to nobody else before the copy has run.  No host wait.
    hipError_t grow(size_t keep, size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        DevBuf larger{home};
        hipError_t e = larger.ensure(std::max(bytes, 2 * cap));
        if (e == hipSuccess && keep) e = hipMemcpyAsync(larger.p, p, keep, hipMemcpyDeviceToDevice, home->stream);
        if (e == hipSuccess) *this = std::move(larger);
        return e;
    }
    // `in_flight`: see pool_free; a drained Home's blocks never are
    void release(bool in_flight = true)
    {
        if (p) pool_free(home->device, p, home->stream, in_flight && !home->drained);
        p = nullptr;
        cap = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a block has one owner");

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; }
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The one way a handle goes (every vx_*_free of a stream-owning Home): its device current, the type's hook, one wait for its stream -- an
// asynchronous call may still be in flight -- and then its blocks go back without an event each.
template <class H> void handle_free(H* h)
{
    if (!h) return;
    DeviceGuard dg(h->device);
    h->before_free();
    (void)hipStreamSynchronize(h->stream);
    h->drained = true;
    delete h;
}
// The one way a create function holds a handle it has not handed out yet: a failure on the way frees it like any other handle, and the
// failure's message stays the last error.
template <class H> struct FreshFree {
    void operator()(H* h) const
    {
        const std::string e = g_err;
        handle_free(h);
        g_err = e;
    }
};
template <class H> using Fresh = std::unique_ptr<H, FreshFree<H>>;

// The host variants' arrays, through device memory of `home` (the handle: its device and stream), one block each: a pooled one that goes
// back when the call ends, or `kept`, a block the handle keeps so that a repeated call of the same size asks the pool for nothing.  in()
// queues an upload, out() notes a download, finish() queues the downloads and waits once.  A null host array is no array: null comes back
// and its kept block is not touched.  The first failure is kept (status()) and turns every later call into a no-op.  From the first
// queued upload on the stream reads the caller's arrays, so a Staging that goes out of scope before finish() has waited -- a failed run,
// a failed ensure or copy -- waits first.
class Staging {
    struct Block {
        DevBuf pooled;  // empty where the array goes through a kept block
        void* dev;
        void* host;     // where finish() copies `bytes` back to; null: an input
        size_t bytes;
    };
    const Home& home;
    std::vector<Block> blocks;
    vx_status st = VX_OK;
    bool queued = false;

    void* add(const void* src, void* dst, size_t bytes, size_t spare, DevBuf* kept)
    {
        if (st != VX_OK || !(src || dst)) return nullptr;
        blocks.reserve(10);  // (here, not in the constructor: a Staging that a _device call never uses costs nothing)
        blocks.push_back(Block{DevBuf{&home}, nullptr, dst, bytes});
        DevBuf& b = kept ? *kept : blocks.back().pooled;
        hipError_t e = b.ensure(bytes + spare);
        if (e == hipSuccess && src) {
            e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, home.stream);
            queued = queued || e == hipSuccess;
        }
        if (e != hipSuccess) st = fail(VX_ERR_HIP, std::string("staging a host array: ") + hipGetErrorString(e));
        return blocks.back().dev = st == VX_OK ? b.p : nullptr;  // (the address of the memory, never of the Block: `blocks` may grow)
    }

public:
    explicit Staging(const Home& h) : home(h) {}
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() { if (queued) (void)hipStreamSynchronize(home.stream); }
    template <class T> T* in(const T* host, size_t bytes, DevBuf* kept = nullptr) { return static_cast<T*>(add(host, nullptr, bytes, 0, kept)); }
    // `spare`: bytes of the block behind the array, which the kernel may touch and nobody reads
    template <class T> T* out(T* host, size_t bytes, size_t spare = 0, DevBuf* kept = nullptr) { return static_cast<T*>(add(nullptr, host, bytes, spare, kept)); }
    vx_status status() const { return st; }
    vx_status finish()
    {
        VX_TRY(st);
        for (const Block& b : blocks)
            if (b.host) VX_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, home.stream));
        VX_HIP(hipStreamSynchronize(home.stream));
        queued = false;
        return VX_OK;
    }
};

vx_status need_device(int dev)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(VX_ERR_NO_DEVICE, "no HIP device available: libvoxhip has no CPU path");
    if (dev < 0 || dev >= n || dev >= kMaxDev) return fail(VX_ERR_INVALID_ARG, "device index out of range");
    return VX_OK;
}

// small per-handle scratch in device memory
struct Small {
    unsigned long long bbox_state[8];  // K1's self-cleaning reduction state (initialised once, see ensure_small)
    vx::DevGrid dgrid;                 // origin + dims as K1 derives them, for kernels queued before the host has seen the bbox
    unsigned long long set_calls[vx::kCallCounters * 8];  // 64 counters on lines of their own (k_voxelize), summed by sync_counts
    unsigned long long units64;        // the unit scan's tagged total where the voxelizer is queued before the host has seen it (voxelize_build)
    unsigned long long nhits;
    unsigned long long trace_counters[4];
    uint32_t solid_flags[2 * 32];      // one word per round of a solid fill: two halves, batches alternate between them
};

// The few values the HOST waits for (bbox -> grid dims, unit / hit / occupied counts -> buffer sizes).  Kernels write them
// straight into pinned host memory; the host reads them after a stream synchronize.  No device-to-host copy kernel, no
// staging through pageable memory.
struct Mail {
    float bbox[8];
    unsigned long long units, hits, occupied, pad;
    unsigned long long solid_rounds, interior;  // solid fill: changed rounds of the last batch, |H|
    unsigned long long surf_tris, surf_verts;   // surface mesh: T and V
    unsigned long long cc_count;                // connected components: K
    unsigned long long bbox_tag;                // the build's tag once bbox is complete (k_bbox), for a host that polls for the bbox alone
};

// Totals may arrive tagged with the build's sequence number in bits 48..63 (see launch_scan_u32): the host then polls the word
// instead of draining the stream -- the totals are written by scans that finish long before the build's last kernel.
constexpr unsigned long long kMailValue = (1ull << 48) - 1ull;
inline bool mail_wait(const volatile unsigned long long* a, const volatile unsigned long long* b /*optional*/, unsigned long long tag, double timeout_ms)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        if ((*a & ~kMailValue) == tag && (!b || (*b & ~kMailValue) == tag)) return true;
        if ((spin & 255u) == 255u && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > timeout_ms) return false;
        __builtin_ia32_pause();
    }
}

struct MailFree {
    void operator()(Mail* m) const { (void)hipHostFree(m); }
};
using MailPtr = std::unique_ptr<Mail, MailFree>;

hipError_t mail_alloc(MailPtr& out)
{
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, sizeof(Mail), hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    std::memset(p, 0, sizeof(Mail));
    out.reset(reinterpret_cast<Mail*>(p));
    return hipSuccess;
}

// What a handle owns besides pool blocks and its mailbox, each destroyed by its destructor: an event (created on first use, with its flags),
// a pinned host block, the grid's low-priority side stream.  Not copyable.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t bytes)  // (contents are not kept)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
};
struct SideStream {
    hipStream_t s = nullptr;
    SideStream() = default;
    SideStream(const SideStream&) = delete;
    SideStream& operator=(const SideStream&) = delete;
    ~SideStream()  // (waits: what it still runs reads its owner's blocks)
    {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    hipError_t create()
    {
        if (s) return hipSuccess;
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);  // (lo: numerically greatest = lowest priority)
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, lo);
        return e;
    }
    operator hipStream_t() const { return s; }
};

// (re)allocated Small: the bbox reduction state needs its initial values once; everything else starts at zero
hipError_t ensure_small(DevBuf& small)
{
    hipError_t e = small.ensure(sizeof(Small));
    if (e != hipSuccess || !small.fresh) return e;
    Small h;
    std::memset(&h, 0, sizeof(h));
    vx::bbox_state_init(h.bbox_state);
    e = hipMemcpy(small.p, &h, sizeof(h), hipMemcpyHostToDevice);
    if (e == hipSuccess) small.fresh = false;
    return e;
}

struct ScanOpts {  // what the callers of a handle scan vary (the rest of vx::ScanArgs is ScanScratch's business)
    unsigned long long total_tag = 0;
    uint32_t *sel1024 = nullptr, *group16 = nullptr;
};

// The scratch of the scans queued on a handle: the single-pass scan's status block and the number of the last scan on it.  The block is
// cleared once when it comes from the pool, and every scan on it is the next generation (state words of older scans read as "not there
// yet"; the numbers wrap at 2^22, where the block is cleared again).  in / out are whole blocks, hence 16-byte aligned: a scan queued
// here always runs single-pass, so its total carries the caller's tag and sel1024 / group16 are written.
struct ScanScratch {
    DevBuf block;
    uint32_t gen = 0;  // the number of the last scan on the block
    vx::ScanTaken took = vx::ScanTaken::ticket;  // the path of the last scan (test aid)
    explicit ScanScratch(const Home* h) : block(h) {}
    // the block sized for a scan of n elements: for callers that must size it ahead of an earlier kernel of theirs (the scans do it themselves)
    hipError_t reserve(uint64_t n, hipStream_t s)
    {
        hipError_t e = block.ensure(vx::scan_tmp_bytes(n));
        if (e != hipSuccess || !block.fresh) return e;
        e = hipMemsetAsync(block.p, 0, block.cap, s);
        if (e == hipSuccess) { block.fresh = false; gen = 0; }
        return e;
    }
    uint32_t next_gen(hipStream_t s)
    {
        if (gen + 1u >= (1u << 22)) { (void)hipMemsetAsync(block.p, 0, block.cap, s); gen = 0; }
        return ++gen;
    }
    void start_at(uint32_t g) { gen = g; }  // (test aid: the next scan is generation g + 1)
    vx_status u32(const DevBuf& in, const DevBuf& out, uint64_t n, bool popcount_input, unsigned long long* total64, hipStream_t s, const ScanOpts& o = ScanOpts())
    {
        VX_HIP(reserve(n, s));
        vx::ScanArgs a;
        a.tmp_is_zero = true;
        a.total_tag = o.total_tag;
        a.sel1024 = o.sel1024;
        a.group16 = o.group16;
        a.gen = next_gen(s);
        return done(vx::launch_scan_u32(in.as<uint32_t>(), out.as<uint32_t>(), n, popcount_input, block.p, total64, s, a));
    }
    vx_status u8(const DevBuf& in, const DevBuf& out, uint64_t n, unsigned long long* total64, hipStream_t s, unsigned long long total_tag = 0)
    {
        VX_HIP(reserve(n, s));
        return done(vx::launch_scan_u8(in.as<uint8_t>(), out.as<uint32_t>(), n, block.p, total64, s, total_tag, next_gen(s)));
    }
    // the scan of n uint32 values and the level-2 mip in one launch (launch_mip2_scan)
    vx_status mip2(const uint32_t* m1, const uint32_t d1[3], const uint32_t d2[3], uint32_t* m2, const DevBuf& in, const DevBuf& out, uint64_t n,
                   unsigned long long* total64, hipStream_t s, unsigned long long total_tag)
    {
        VX_HIP(reserve(n, s));
        return done(vx::launch_mip2_scan(m1, d1, d2, m2, in.as<uint32_t>(), out.as<uint32_t>(), n, block.p, total64, s, total_tag, next_gen(s)));
    }
    vx_status done(vx::ScanTaken t)
    {
        took = t;
        return t != vx::ScanTaken::three_pass ? VX_OK : fail(VX_ERR_UNSUPPORTED, "internal: a scan on a handle's scratch took the three-pass path");
    }
};

// A total that has arrived in the mailbox: the tag bits masked off, refused with the caller's message at 2^32 - 1 and above.
vx_status mail_value(const volatile unsigned long long* word, const char* limit_message, uint64_t* out)
{
    const unsigned long long tot = *word & kMailValue;
    if (tot >= 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, limit_message);
    *out = tot;
    return VX_OK;
}

// A total the host waits for: under its tag it is polled for (5 ms at most); tag 0 -- or a total that does not come -- waits for the stream.
vx_status mail_total(const volatile unsigned long long* word, unsigned long long tag, hipStream_t s, const char* limit_message, uint64_t* out)
{
    if (!(tag && mail_wait(word, nullptr, tag, 5.0))) VX_HIP(hipStreamSynchronize(s));
    return mail_value(word, limit_message, out);
}

// what is left of the record kernel's and the unit scan's optional arguments (UnitPipe::setup_launch)
struct SetupOpts {
    const vx::DevGrid* dgrid = nullptr;   // origin and dims as K1 left them on the device: a launch queued before the host has read the bbox
    unsigned long long tag = 0;           // of the unit total in the mailbox
    void* clear = nullptr;                // a buffer the record kernel zeroes beside its own work ...
    uint64_t clear_bytes = 0;             // ... and its size
    uint64_t shard_wb = 0, shard_we = 0;  // with dgrid: the word shard whose z slab the kernel derives (0, 0: whole grid)
    uint32_t shard_rank = 0, shard_world = 0;  // with dgrid and world > 1: the word shard vx_shard_words gives that rank
    unsigned long long* units_total = nullptr;  // where the unit total goes instead of the mailbox (device memory)
};

// The unit pipeline of a build (grids and the octree): triangle records, high bits of the candidate ranges, units per triangle and their
// scan, the block table, per unit its hit mask, hits per block of 64 units and their exclusive scan, and the scratch of the scans.
struct UnitPipe {
    DevBuf recs, ext, units, ubase, btri, umask, bhits, hbase;
    ScanScratch scantmp;
    explicit UnitPipe(const Home* h) : recs(h), ext(h), units(h), ubase(h), btri(h), umask(h), bhits(h), hbase(h), scantmp(h) {}
    // what the launchers read; wide: an axis above 65535 cells, the unit kernels also read the extension words
    vx::Units view(uint32_t ntri, bool wide) const
    {
        vx::Units u;
        u.recs = recs.as<vx::TriRec>();
        u.unit_base = ubase.as<uint32_t>();
        u.block_tri = btri.as<uint32_t>();
        u.ntri = ntri;
        u.ext = wide ? ext.as<uint32_t>() : nullptr;
        return u;
    }
    // The front half of buildVoxelGrid that grids and the octree share: records, unit counts, unit bases.  In two parts so that
    // the caller can queue work that does not depend on the unit count (clearing the bitmask) before the host waits for it.
    vx_status setup_launch(const vx_mesh* m, const vx::GridParams& g, int sat, uint64_t tb, uint32_t ntri, uint32_t zlo, uint32_t zhi, Mail* mail, hipStream_t s,
                           const SetupOpts& o = SetupOpts());
    // btri_entries: entries of the block table a launch queued before the host knew the total has already filled (0: none)
    vx_status setup_finish(uint32_t ntri, Mail* mail, hipStream_t s, uint64_t* total_units, bool stream_is_drained = false, uint64_t btri_entries = 0);
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------
struct vx_mesh : Home {  // (no stream of its own: uploads are synchronous)
    std::vector<float> hv;
    std::vector<int32_t> hi;
    std::vector<int32_t> tri_mat;        // material id per triangle (-1 = none); empty: the mesh has no materials
    std::vector<vx_material> materials;  // m_materials of the reference builder (VoxelBuilder.hpp:69)
    // material VALUES for the voxelizer: the mesh's records de-duplicated by MaterialObj::operator== (value 0 is always the default
    // MaterialObj{} that faces without usemtl carry, VoxelBuilder.hpp:383) and the value id of every triangle
    std::vector<vx_material> values;
    std::vector<int32_t> tri_value;
    bool values_ready = false;
    DevBuf btv{this};  // tri_value on the device
    size_t nv = 0, nt = 0;
    const float* dv = nullptr;
    const int32_t* di = nullptr;
    DevBuf bv{this}, bi{this};
    bool borrowed = false;
    bool uploaded = false;
    // attribute shading (vx_render_set_shading): corner normals / uvs (9 / 6 f32 per triangle, empty: none), texture slots (file name, RGBA8
    // image top row first; w = 0: no image yet) and the slot of every material (-1 none).  Host only; scenes upload them.
    std::vector<float> cnrm, cuv;
    struct Texture { std::string name; uint32_t w = 0, h = 0; std::vector<uint8_t> rgba; };
    std::vector<Texture> tex;
    std::vector<int32_t> mat_slot;
};

namespace {
constexpr int32_t kMaxTextureSlots = 1 << 16;
constexpr uint32_t kMaxTextureSide = 16384;

// Texture files of vx_mesh_load_textures: binary PPM (P6, maxval 255) and TGA (types 2 and 10: uncompressed / RLE true colour, 24 or 32 bpp,
// the origin bits honoured) -> RGBA8, top row first, as stbi_load returns an image.  false: missing, unreadable, truncated or unsupported.
bool decode_ppm(const std::string& d, uint32_t& w, uint32_t& h, std::vector<uint8_t>& out)
{
    size_t i = 2;
    uint64_t v[3];
    for (int k = 0; k < 3; ++k) {
        for (;;) {  // whitespace and comments between the header fields
            while (i < d.size() && std::isspace((unsigned char)d[i])) ++i;
            if (i < d.size() && d[i] == '#') { while (i < d.size() && d[i] != '\n') ++i; continue; }
            break;
        }
        if (i >= d.size() || !std::isdigit((unsigned char)d[i])) return false;
        v[k] = 0;
        while (i < d.size() && std::isdigit((unsigned char)d[i]) && v[k] < 1000000) v[k] = v[k] * 10 + (uint64_t)(d[i++] - '0');
    }
    if (i >= d.size() || !std::isspace((unsigned char)d[i])) return false;
    ++i;  // the single whitespace before the raster
    if (v[2] != 255 || v[0] < 1 || v[0] > kMaxTextureSide || v[1] < 1 || v[1] > kMaxTextureSide) return false;
    const size_t n = (size_t)v[0] * v[1];
    if (d.size() - i < n * 3) return false;
    w = (uint32_t)v[0];
    h = (uint32_t)v[1];
    out.resize(n * 4);
    for (size_t p = 0; p < n; ++p) {
        for (int c = 0; c < 3; ++c) out[4 * p + c] = (uint8_t)d[i + 3 * p + c];
        out[4 * p + 3] = 255;
    }
    return true;
}

bool decode_tga(const std::string& d, uint32_t& w, uint32_t& h, std::vector<uint8_t>& out)
{
    if (d.size() < 18) return false;
    const uint8_t* b = reinterpret_cast<const uint8_t*>(d.data());
    const uint32_t idlen = b[0], cmap = b[1], type = b[2], bpp = b[16], desc = b[17];
    const uint32_t tw = b[12] | (b[13] << 8), th = b[14] | (b[15] << 8);
    if (cmap != 0 || (type != 2 && type != 10) || (bpp != 24 && bpp != 32)) return false;
    if (tw < 1 || th < 1 || tw > kMaxTextureSide || th > kMaxTextureSide) return false;
    const size_t bytes = bpp / 8, n = (size_t)tw * th;
    size_t i = 18 + idlen;
    std::vector<uint8_t> px(n * 4);  // file order
    auto put = [&](size_t p, const uint8_t* src) {
        px[4 * p] = src[2]; px[4 * p + 1] = src[1]; px[4 * p + 2] = src[0];  // BGR(A)
        px[4 * p + 3] = bytes == 4 ? src[3] : 255;
    };
    if (type == 2) {
        if (i > d.size() || d.size() - i < n * bytes) return false;
        for (size_t p = 0; p < n; ++p) put(p, b + i + p * bytes);
    } else {
        size_t p = 0;
        while (p < n) {
            if (i >= d.size()) return false;
            const uint32_t hdr = b[i++], cnt = (hdr & 0x7F) + 1;
            if (p + cnt > n) return false;
            if (hdr & 0x80) {
                if (d.size() - i < bytes) return false;
                for (uint32_t k = 0; k < cnt; ++k) put(p++, b + i);
                i += bytes;
            } else {
                if (d.size() - i < cnt * bytes) return false;
                for (uint32_t k = 0; k < cnt; ++k) put(p++, b + i + k * bytes);
                i += cnt * bytes;
            }
        }
    }
    const bool top = (desc & 0x20) != 0, right = (desc & 0x10) != 0;  // origin: bottom-left unless bit 5 (top) / bit 4 (right) is set
    w = tw;
    h = th;
    out.resize(n * 4);
    for (uint32_t y = 0; y < th; ++y)
        for (uint32_t x = 0; x < tw; ++x) {
            const size_t sy = top ? y : th - 1 - y, sx = right ? tw - 1 - x : x;
            std::memcpy(&out[4 * ((size_t)y * tw + x)], &px[4 * (sy * tw + sx)], 4);
        }
    return true;
}

bool decode_image(const std::string& path, uint32_t& w, uint32_t& h, std::vector<uint8_t>& out)
{
    if (path.empty()) return false;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string d;
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) d.append(buf, k);
    std::fclose(f);
    if (d.size() >= 2 && d[0] == 'P' && d[1] == '6') return decode_ppm(d, w, h, out);
    return decode_tga(d, w, h, out);
}

vx_material default_material()  // MaterialObj{} (common/obj_loader.h:32-43)
{
    vx_material m;
    std::memset(&m, 0, sizeof(m));
    m.ambient[0] = m.ambient[1] = m.ambient[2] = 0.1f;
    m.diffuse[0] = m.diffuse[1] = 1.0f;
    m.specular[0] = m.specular[1] = m.specular[2] = 1.0f;
    m.emission[2] = 0.10f;
    m.shininess = 0.f;
    m.ior = 1.0f;
    m.dissolve = 1.f;
    m.illum = 0;
    m.texture_id = -1;
    return m;
}
bool same_material(const vx_material& a, const vx_material& b)  // MaterialObj::operator== (obj_loader.h:45-51): ior and dissolve are not compared
{
    for (int k = 0; k < 3; ++k)
        if (a.ambient[k] != b.ambient[k] || a.diffuse[k] != b.diffuse[k] || a.specular[k] != b.specular[k] || a.transmittance[k] != b.transmittance[k] ||
            a.emission[k] != b.emission[k])
            return false;
    return a.shininess == b.shininess && a.illum == b.illum && a.texture_id == b.texture_id;
}
}  // namespace

struct vx_grid : Home {
    int kind = VX_GRID_BOOL;
    vx::GridParams g{};
    float bbmin[3] = {0, 0, 0}, bbmax[3] = {0, 0, 0}, bbc[3] = {0, 0, 0};
    uint64_t triangles = 0;
    uint32_t cdim[3] = {0, 0, 0}, c2dim[3] = {0, 0, 0};
    MailPtr mail;  // (ahead of the buffers: freed after them)
    DevBuf words{this}, twords{this} /*tiled build mask (launch_voxelize)*/, cwords{this}, c2words{this}, bricks{this}, idxtmp{this}, ttmp{this}, camera{this}, wprefix{this};
    DevBuf wsel{this} /*word of every 1024th occupied voxel (prefix scan)*/, wp16{this} /*every 16th entry of wprefix, dense (prefix scan)*/;
    DevBuf lcnt{this} /*set bits per 16-word line of the bitmask (the brick kernel of a whole Vec build): wp16 is their scan*/;
    DevBuf wring{this} /*k_walk's rank epilogue: per wave the chunks of rays it drew (walk_ring_cap words each); scratch of one ray batch*/;
    UnitPipe up{this};  // (its scantmp serves every scan on the main stream, the queries' too)
    ScanScratch hscantmp{this};  // of a block-hit scan queued with the list (list_scan)
    DevBuf small{this}, vec{this}, matids{this}, mattmp{this};
    // solid voxelization (vx_solid.hip): padded mask, exterior, H in the reference's layout (padded rows only) and the word prefix over H
    DevBuf solid_m{this}, solid_e{this}, solid_h{this}, solid_pre{this}, solid_agg{this} /*the column scans' per-chunk words*/;
    // distance fields (vx_distance.hip): the envelopes' stacks, and the field itself for the host variants
    DevBuf dist_stk{this}, dist_out{this};
    DevBuf near_val{this};  // the feature transform's host gather: the values on the device (its stacks and result share dist_stk / dist_out)
    // morphology (vx_morph.hip): two row-aligned masks (a stage's output, the next one's input), a padded or intermediate mask in the
    // reference's layout, the distance-field path's field and the host variant's result
    DevBuf morph_a{this}, morph_b{this}, morph_p{this}, morph_d{this}, morph_out{this};
    // surface mesh (vx_surface.hip): triangles per mask word and their scan, the used lattice points and their scan, the host variant's arrays
    DevBuf surf_cnt{this}, surf_tpre{this}, surf_cm{this}, surf_vpre{this}, surf_out{this};
    DevBuf nets_buf{this};  // surface nets: lattice index, neighbour table, two offset fields, configuration per vertex
    // connected components (vx_components.hip): the root bitmask and its scan, the host variants' labels, the statistics
    DevBuf cc_roots{this}, cc_rpre{this}, cc_lab{this}, cc_stat{this};
    uint64_t interior = 0;        // |H| of the last build or fill on the handle (vx_grid_interior)
    uint32_t solid_rounds = 0;    // rounds of that fill, the quiet one included (vx_grid_fill_rounds)
    uint64_t mat_interior = 0;    // a solid VX_VOXELIZE_MATERIALS build: ids of interior voxels / calls still to be given MaterialObj{}'s index
    uint64_t mat_surface = 0;     // ... Vec: they follow the triangles' mat_surface calls
    std::vector<vx_material> materials;  // m_materials: distinct values in first-use order (VX_VOXELIZE_MATERIALS builds only)
    uint64_t mat_count = 0;              // entries of matids
    bool has_materials = false;
    // a VX_VOXELIZE_MATERIALS build in two halves: what the build itself knows (per value the first triangle of this shard that uses
    // it; the last triangle per voxel resp. the unit masks stay in mattmp / umask / hbase) and the finish (finish_materials)
    bool mat_pending = false;
    std::vector<long long> mat_first_use;
    std::vector<vx_material> mat_values;   // the mesh's material values at build time
    const int32_t* mat_dtv = nullptr;      // per-triangle value ids of this build's triangle range (device, owned by the mesh)
    uint32_t mat_ntri = 0;
    uint64_t mat_nids = 0;
    bool mat_gathered = false;             // multi-GPU build: the ids of ALL shards, gathered in shard order, live in mattmp
    uint64_t mat_gather_count = 0;
    bool coarse_valid = false, prefix_valid = false /*word_prefix queued or done*/, occupied_known = false, counts_valid = true;
    // wp16 and the occupied count queued or done WITHOUT the word prefix: scanned from the brick kernel's line counts (p16_launch).  All a ray
    // batch's rank pass reads; whoever indexes wprefix itself builds it on demand (prefix_launch / ensure_prefix)
    bool p16_valid = false;
    bool last_tiled = false;  // the previous build on this handle went through the tiled build mask (twords)
    uint64_t occupied = 0, set_calls = 0, host_set_calls = 0;
    uint64_t vec_count = 0;
    uint32_t mail_seq = 0;  // sequence tag of the totals the current build writes to the mailbox
    bool sel_valid = false;  // wsel belongs to the current word prefix
    unsigned long long occ_tag = 0;  // tag of the scan whose total (the occupied count) is in flight; 0: none
    int trace_phase = 0;  // which of Small::trace_counters[0..1] the next ray launch draws its work from (the launch clears the other)
    // VX_GRID_VEC: the caller's own list buffer (vx_grid_bind_aabbs_device); builds emit straight into it when it is large enough
    vx_aabb* bound = nullptr;
    uint64_t bound_cap = 0;
    bool vec_in_bound = false;  // the current list lives in `bound`, not in `vec`
    vx_aabb* vec_ptr() const { return vec_in_bound ? bound : reinterpret_cast<vx_aabb*>(vec.p); }
    // VX_VOXELIZE_LIST_ASYNC (VX_GRID_VEC): the ordered emission of the list is not queued by the build.  Nothing that follows a build on the
    // handle's stream -- traversal structure, word prefix, a ray batch -- reads the list; the ray kernel keeps a set of persistent workgroups
    // on every CU and ends with a long drain in which most of the machine idles, and the emission (store-bound, 40 us on the bench scene) fits
    // into that: the next ray batch queues it on a low-priority SIDE stream of the handle, behind an event recorded on the main stream in front
    // of the ray kernel, so that its workgroups fill the slots the ray kernel's leave.  Whatever reads the list or overwrites what the emission
    // reads (host / device copies of the list, re-binding, setVoxel, the next build, free) goes through list_resolve() first.
    // (behind every DevBuf, the stream last: it is destroyed first, drained, before the events it waits on and the blocks its work touches)
    Event ev_ready, ev_list;
    SideStream side;
    bool list_deferred = false;  // the emission has not been queued yet (its arguments: ld)
    bool list_pending = false;   // it has been queued on `side`; the main stream has not waited for ev_list yet
    // from_mask: vx_grid_aabbs_device_async (K4).  scan_blocks: hbase has not been written by the build -- the host took the hit count from the
    // voxelizer's counters (k_build_bricks3) -- and the scan of the build's scan_blocks block-hit counts goes in front of the emission
    struct { uint32_t ntri = 0; bool ext = false; vx_aabb* tgt = nullptr; uint64_t cap = 0; bool from_mask = false; uint64_t scan_blocks = 0; } ld;
    hipError_t side_init()
    {
        // (both events order streams of ONE device: no system-scope fence -- its cache write-back would stand in front of the ray kernel)
        const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
        hipError_t e = side.create();
        if (e == hipSuccess) e = ev_ready.create(evf);
        if (e == hipSuccess) e = ev_list.create(evf);
        return e;
    }
    // the hit bases the emission reads, where the build left their scan to the list: queued once, on the stream the emission follows on
    // (a status block of its own, hscantmp, sized by the build: the main stream's scans use scantmp at the same time)
    void list_scan(hipStream_t st)
    {
        if (ld.from_mask || !ld.scan_blocks) return;
        (void)hscantmp.u32(up.bhits, up.hbase, ld.scan_blocks, false, nullptr, st);
        ld.scan_blocks = 0;
    }
    void list_emit(hipStream_t st)
    {
        list_scan(st);
        if (ld.from_mask) {  // Bool / AABBstruct: the ascending list from the bitmask and its word prefix (both complete on the main stream)
            vx::launch_emit_bool_aabbs(words.as<uint32_t>(), wprefix.as<uint32_t>(), g, ld.tgt, ld.cap, st, sel_valid ? wsel.as<uint32_t>() : nullptr);
            return;
        }
        vx::launch_emit_units(up.view(ld.ntri, ld.ext), g, up.umask.as<uint32_t>(), up.hbase.as<uint32_t>(), ld.tgt, nullptr, st, ld.cap);
    }
    // first half, BEFORE the caller queues the work the emission is to run beside; second half after it
    hipError_t list_side_begin()
    {
        hipError_t e = side_init();
        if (e == hipSuccess) e = hipEventRecord(ev_ready, stream);
        return e;
    }
    // `counter`, `dry_at`: the ray kernel's work queue (vx::WalkQueue), for the gate in front of the emission.  Holding the emission until the
    // queue is DRY was measured and dropped: the drain frees registers wave by wave but LDS only workgroup by workgroup, the emission then
    // needs the whole drain (155 us) and ends about when the ray kernel does -- 0.504-0.510 ms per step.
    hipError_t list_side_launch(unsigned long long* counter, unsigned long long dry_at)
    {
        hipError_t e = hipStreamWaitEvent(side, ev_ready, 0);
        if (e != hipSuccess) return e;
        // (the hit scan, a handful of 1024-thread workgroups, in front of the gate: it runs as the ray kernel starts, not in its drain, where a
        // workgroup of that size finds no room until most of a CU's ray workgroups have left)
        list_scan(side);
        // The emission is held until the first wave of the ray kernel has come back to the queue for more rays -- the kernel's persistent
        // workgroups are all placed by then, the emission cannot take their slots first (without the hold the step varies 0.497-0.535 ms
        // from run to run, with it 0.489-0.494).  The hold is a one-wave gate kernel with a time bound (vx_trace.hip: a stream-level wait
        // on the counter hangs under serialising profilers).
        if (counter && dry_at) {  // (dry_at == 0: the static first chunks cover the batch, the counter never moves)
            vx::WalkQueue q;
            q.counter = counter;
            q.dry_at = dry_at;
            vx::launch_queue_gate(q, side);
        }
        list_emit(side);
        e = hipEventRecord(ev_list, side);
        list_deferred = false;
        list_pending = true;
        return e;
    }
    // work queued on the main stream after this call sees the complete list (and may overwrite what the emission read)
    hipError_t list_resolve(bool drop_unqueued = false)
    {
        if (list_deferred) {
            list_deferred = false;
            // nobody asked for rays in between: the emission runs where it always did (a caller's buffer is always filled; the grid's own
            // Vec list may be dropped when it is about to be replaced)
            if (!drop_unqueued || ld.from_mask) list_emit(stream);
            ld.scan_blocks = 0;  // (a dropped list drops its scan)
        }
        if (list_pending) {
            list_pending = false;
            return hipStreamWaitEvent(stream, ev_list, 0);
        }
        return hipSuccess;
    }
    void before_free() { (void)list_resolve(/*drop_unqueued=*/true); }  // (the main stream then waits for the side stream's emission)
    // ---- what a build (or a failed one) resets, one place per kind of state
    void reset_materials()
    {
        has_materials = mat_pending = mat_gathered = false;
        materials.clear();
        mat_count = 0;
        mat_interior = mat_surface = 0;
    }
    void reset_solid() { interior = 0; solid_rounds = 0; }
    // what is derived from the mask: traversal structure, prefixes, counts, the list's length.  counts_known: an EMPTY grid's occupied count
    // is known (0); a fresh grid's is whatever the build that follows leaves
    void reset_derived(bool counts_known)
    {
        coarse_valid = prefix_valid = p16_valid = false;
        occupied_known = counts_known;
        counts_valid = true;
        occupied = set_calls = host_set_calls = vec_count = 0;
    }
    // the stream this handle queues work on; the pool orders the reuse of released blocks by it
    void set_stream(hipStream_t st)
    {
        if (st != stream && words.p) {  // work queued on the old stream (and beside it) must not outlive the switch
            (void)list_resolve();
            (void)hipStreamSynchronize(stream);
        }
        stream = st;
    }
};

struct vx_octree : Home {
    float vs = 0.f;
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};
    uint64_t dim[3] = {0, 0, 0};
    uint32_t bits = 0;
    uint64_t max_items = 16;
    uint64_t nitems = 0;
    DevBuf items{this};  // sorted Morton codes
    DevBuf nodebuf{this};  // pre-order node array, from either form of the node build
    uint64_t nnodes = 0;
    DevBuf camera{this};  // vx_octree_trace*: the camera block of primary-ray batches
};

namespace {

vx_status mesh_to_device(vx_mesh* m)
{
    if (m->uploaded || m->borrowed) return VX_OK;
    VX_TRY(need_device(m->device));
    VX_HIP(m->bv.ensure(m->nv * 12 + 16));
    VX_HIP(m->bi.ensure(m->nt * 12 + 16));
    if (m->nv) VX_HIP(hipMemcpy(m->bv.p, m->hv.data(), m->nv * 12, hipMemcpyHostToDevice));
    if (m->nt) VX_HIP(hipMemcpy(m->bi.p, m->hi.data(), m->nt * 12, hipMemcpyHostToDevice));
    m->dv = m->bv.as<float>();
    m->di = m->bi.as<int32_t>();
    m->uploaded = true;
    return VX_OK;
}

// material values of a mesh (host) and their per-triangle ids on the device
vx_status mesh_material_values(vx_mesh* m)
{
    if (!m->values_ready) {
        if (m->borrowed && !m->tri_mat.empty() && m->tri_mat.size() != m->nt) return fail(VX_ERR_INVALID_ARG, "material ids do not match the triangle count");
        m->values.clear();
        m->values.push_back(default_material());
        std::vector<int32_t> rec_value(m->materials.size(), 0);
        for (size_t i = 0; i < m->materials.size(); ++i) {
            // VoxelBuilder copies the record into a fresh MaterialObj (VoxelBuilder.hpp:383-394): textureID stays -1
            vx_material v = m->materials[i];
            v.texture_id = -1;
            int32_t id = -1;
            for (size_t k = 0; k < m->values.size(); ++k)
                if (same_material(m->values[k], v)) { id = (int32_t)k; break; }
            if (id < 0) { m->values.push_back(v); id = (int32_t)m->values.size() - 1; }
            rec_value[i] = id;
        }
        if (m->values.size() > 32767) return fail(VX_ERR_CAPACITY, "more than 32767 distinct materials: per-voxel ids are int16 (voxelgrid.hpp:29)");
        m->tri_value.assign(m->nt, 0);
        if (!m->tri_mat.empty())
            for (size_t t = 0; t < m->nt; ++t) {
                const int32_t id = m->tri_mat[t];
                m->tri_value[t] = (id >= 0 && (size_t)id < rec_value.size()) ? rec_value[(size_t)id] : 0;  // VoxelBuilder.hpp:384: out-of-range ids keep the default
            }
        m->values_ready = true;
        m->btv.release();
    }
    if (!m->btv.p && m->nt) {
        VX_HIP(m->btv.ensure(m->nt * 4 + 16));
        VX_HIP(hipMemcpy(m->btv.p, m->tri_value.data(), m->nt * 4, hipMemcpyHostToDevice));
    }
    return VX_OK;
}

// bbox + dims: computeBboxFromAttrib (VoxelBuilder.hpp:198-224) on the device, dims on the host (:347-349)
struct Extent {
    float mn[3], mx[3], ctr[3];
    uint64_t dim[3];
};

// morton_error: the caller is the Octree, whose limit of 2^21 cells per axis carries the reference's own message (octTree.hpp:583-585)
vx_status extent_from_bbox(const float* bb, size_t nv, float vs, Extent* e, bool morton_error = false)
{
    // a NaN or infinite coordinate of any vertex is the minimum or the maximum of its axis (k_bbox orders +NaN above +Inf and -NaN below -Inf)
    for (int a = 0; a < 6 && nv; ++a)
        if (!std::isfinite(bb[a])) return fail(VX_ERR_INVALID_ARG, "mesh has a non-finite vertex coordinate (NaN or Inf)");
    for (int a = 0; a < 3; ++a) {
        e->mn[a] = bb[a];
        e->mx[a] = bb[3 + a];
        e->ctr[a] = (bb[a] + bb[3 + a]) * 0.5f;  // VoxelBuilder.hpp:221
        if (nv == 0) { e->dim[a] = 0; continue; }
        const float q = std::ceil((e->mx[a] - e->mn[a]) / vs);  // :347-349
        if (!(q >= 0.0f) || q > (float)vx::kMaxDim) {
            if (morton_error && q > (float)vx::kMaxDim) return fail(VX_ERR_MORTON_BITS, "We support up to 21 bits per axis (max 2^21 voxels per dimension)!");
            return fail(VX_ERR_CAPACITY, "grid dimension outside [0, 2^21]: voxel size too small for this mesh");
        }
        e->dim[a] = (uint64_t)q;
    }
    return VX_OK;
}

vx_status compute_extent(const vx_mesh* m, float vs, Small* dsmall, Mail* mail, hipStream_t s, Extent* e, bool morton_error = false)
{
    // one kernel: reduction, result into the host mailbox, state restored, per-build setVoxel counter cleared
    vx::launch_bbox(m->dv, m->nv, dsmall->bbox_state, mail->bbox, dsmall->set_calls, s);
    VX_HIP(hipStreamSynchronize(s));
    return extent_from_bbox(mail->bbox, m->nv, vs, e, morton_error);
}

vx_status check_voxel_size(float vs)
{
    if (!(vs > 0.0f) || !std::isfinite(vs)) return fail(VX_ERR_INVALID_ARG, "voxel size must be a finite positive float");
    return VX_OK;
}

void fill_params(vx::GridParams& g, const float org[3], float vs, const uint64_t dim[3])
{
    for (int a = 0; a < 3; ++a) { g.org[a] = org[a]; g.dim[a] = (uint32_t)dim[a]; }
    g.vs = vs;
    g.half = vs * 0.5f;
    g.nvox = dim[0] * dim[1] * dim[2];
    g.nwords = (g.nvox + 31) / 32;
}

constexpr uint64_t kMaxVoxels = 1ull << 37;  // 16 GiB of bitmask

vx_status UnitPipe::setup_launch(const vx_mesh* m, const vx::GridParams& g, int sat, uint64_t tb, uint32_t ntri, uint32_t zlo, uint32_t zhi, Mail* mail, hipStream_t s,
                                 const SetupOpts& o)
{
    VX_HIP(recs.ensure((size_t)ntri * sizeof(vx::TriRec) + 64));
    VX_HIP(ext.ensure(((size_t)ntri + 1) * 4));  // high bits of the candidate ranges (read only when an axis has more than 65535 cells)
    VX_HIP(units.ensure(((size_t)ntri + 1) * 4));
    VX_HIP(ubase.ensure(((size_t)ntri + 2) * 4));
    VX_HIP(scantmp.reserve(ntri, s));  // (ahead of the record kernel, as ever)
    vx::launch_tri_setup(m->dv, m->di, tb, ntri, g, sat, zlo, zhi, recs.as<vx::TriRec>(), units.as<uint32_t>(), s, o.dgrid, o.clear, o.clear_bytes, o.shard_wb, o.shard_we,
                         ext.as<uint32_t>(), o.shard_rank, o.shard_world);
    // (o.tag == 0: the total carries no tag, its reader waits for the stream -- setup_finish)
    return scantmp.u32(units, ubase, ntri, false, o.units_total ? o.units_total : &mail->units, s, {o.tag});
}

vx_status UnitPipe::setup_finish(uint32_t ntri, Mail* mail, hipStream_t s, uint64_t* total_units, bool stream_is_drained, uint64_t btri_entries)
{
    const char* limit = "more than 2^32 candidate row segments: shard the mesh or the grid";
    uint64_t tot = 0;
    if (stream_is_drained) VX_TRY(mail_value(&mail->units, limit, &tot));
    else VX_TRY(mail_total(&mail->units, 0, s, limit, &tot));
    *total_units = tot;
    if (tot && btri_entries < tot / 64 + 2) {
        VX_HIP(btri.ensure((size_t)(tot / 64 + 2) * 4));
        vx::launch_unit_blocks(view(ntri, false), (uint32_t)tot, btri.as<uint32_t>(), s);
    }
    return VX_OK;
}

// the sequence tag of the next total the handle's kernels post to its mailbox (bits 48..63, never 0: an untagged word never matches)
unsigned long long next_tag(vx_grid* g)
{
    g->mail_seq = (g->mail_seq % 0xFFFFu) + 1u;
    return (unsigned long long)g->mail_seq << 48;
}

// word_prefix + occupied count.  Split in two so that callers can queue dependent kernels before the host waits for the
// count (a host sync in front of a kernel leaves the GPU idle and the clocks down for its start).
vx_status prefix_launch(vx_grid* g, bool* pending, unsigned long long tag = 0)
{
    *pending = !g->occupied_known;
    if (g->prefix_valid) return VX_OK;
    const bool count_known = g->p16_valid && g->occupied_known;  // (the line counts' scan gave the count already: nobody has to wait for this one's)
    if (!tag) tag = next_tag(g);  // a scan outside a build: its own sequence tag
    VX_HIP(g->wprefix.ensure((size_t)(g->g.nwords + 2) * 4));
    VX_HIP(g->wsel.ensure((size_t)(g->g.nwords / 32 + 4) * 4));  // at most 32 nwords / 1024 chunks of 1024 records
    VX_HIP(g->wp16.ensure((size_t)(g->g.nwords / 16 + 4) * 4));
    VX_TRY(g->up.scantmp.u32(g->words, g->wprefix, g->g.nwords, true, &g->mail->occupied, g->stream, {tag, g->wsel.as<uint32_t>(), g->wp16.as<uint32_t>()}));
    g->prefix_valid = g->sel_valid = true;
    if (count_known) return VX_OK;
    g->occ_tag = tag;  // what the host polls the mailbox for instead of draining the stream (prefix_finish)
    g->occupied_known = false;
    *pending = true;
    return VX_OK;
}

// A whole Vec build on the tiled build mask whose rows are multiples of 512 voxels: the brick kernel, which has every word of the bitmask
// in its hands, also left the set bits of every 16-word line (g->lcnt).  Their exclusive scan IS word_prefix[16 i] -- the table the rank pass
// of a ray batch reads beside the voxel's own line of the mask -- and its total the occupied count, posted to the same mailbox word: a scan
// over nwords / 16 values instead of a pass that reads the mask again and writes nwords prefixes nobody on this path reads.
// The level-2 mip, which like this scan reads only what the brick kernel wrote, shares the scan's launch (ensure_coarse calls this in place of
// its own last kernel).
vx_status p16_launch(vx_grid* g, unsigned long long tag)
{
    const uint64_t nl = g->g.nwords / 16;
    VX_HIP(g->wp16.ensure((size_t)(nl + 4) * 4));
    VX_TRY(g->up.scantmp.mip2(g->cwords.as<uint32_t>(), g->cdim, g->c2dim, g->c2words.as<uint32_t>(), g->lcnt, g->wp16, nl, &g->mail->occupied, g->stream, tag));
    g->p16_valid = true;
    g->prefix_valid = g->sel_valid = false;  // (wprefix and wsel still describe an older mask)
    g->occ_tag = tag;
    g->occupied_known = false;
    return VX_OK;
}

// what the rank pass of a ray batch needs on the stream: wp16 where the build left it, the word prefix (which brings wp16 along) otherwise
vx_status rank_launch(vx_grid* g, bool* pending)
{
    if (g->p16_valid) { *pending = !g->occupied_known; return VX_OK; }
    return prefix_launch(g, pending);
}

vx_status prefix_finish(vx_grid* g, bool pending)
{
    if (!pending || g->occupied_known) return VX_OK;
    VX_TRY(mail_total(&g->mail->occupied, g->occ_tag, g->stream, "more than 2^32 occupied voxels", &g->occupied));
    g->occupied_known = true;
    return VX_OK;
}

vx_status ensure_prefix(vx_grid* g)
{
    DeviceGuard dg(g->device);
    bool pending = false;
    VX_TRY(prefix_launch(g, &pending));
    return prefix_finish(g, pending);
}

// the occupied count on the host (no word prefix is built for it where the line counts' scan delivers it)
vx_status ensure_occupied(vx_grid* g)
{
    if (!g->p16_valid) return ensure_prefix(g);
    DeviceGuard dg(g->device);
    return prefix_finish(g, !g->occupied_known);
}

// What a build asks of the traversal structure beyond the lazy form (ensure_coarse):
struct CoarseBuild {
    bool from_tiled = false;     // the reference's bitmask has not been written yet -- the brick kernel reads the tiled build mask (g->twords) and writes it on the way
    bool line_counts = false;    // (with from_tiled) it also leaves the set bits per 16-word line in g->lcnt, and their scan (p16_launch: wp16, the occupied
                                 // count under `tag`) is queued in one launch with the level-2 mip
    unsigned long long tag = 0;  // of the totals it posts
    bool post_hits = false;      // (with from_tiled) the brick kernel posts the voxelizer's hit count to mail->hits under `tag`
};
vx_status build_coarse(vx_grid* g, const CoarseBuild& c)
{
    if (g->coarse_valid && !c.from_tiled) return VX_OK;
    DeviceGuard dg(g->device);
    for (int a = 0; a < 3; ++a) {
        g->cdim[a] = (g->g.dim[a] + vx::kCoarse - 1) / vx::kCoarse;
        g->c2dim[a] = (g->cdim[a] + vx::kBlockBricks - 1) / vx::kBlockBricks;
    }
    const uint64_t nc = (uint64_t)g->cdim[0] * g->cdim[1] * g->cdim[2];
    const uint64_t nc2 = (uint64_t)g->c2dim[0] * g->c2dim[1] * g->c2dim[2];
    VX_HIP(g->cwords.ensure((size_t)((nc + 63) / 64 * 2 + 2) * 4));
    VX_HIP(g->c2words.ensure((size_t)((nc2 + 31) / 32 + 2) * 4));
    VX_HIP(g->bricks.ensure((size_t)(nc * 8 * 3 + 8) * 8));  // three orientations (x, y, z slabs)
    // bitmask -> brick-major slabs in three orientations -> level-1 mip (from the z orientation) -> level-2 mip
    const bool fuse_mip1 = !(getenv("VOXHIP_FUSE_MIP1") && atoi(getenv("VOXHIP_FUSE_MIP1")) == 0);  // 0: the separate kernel, every brick stored (tests)
    vx::BricksArgs ba;
    if (c.from_tiled) {
        ba.tiled = g->twords.as<uint32_t>();
        if (c.line_counts) ba.line_cnt = g->lcnt.as<uint32_t>();
        if (c.post_hits) {
            ba.hit_counters = g->small.as<Small>()->set_calls;
            ba.hits_out = &g->mail->hits;
        }
    }
    ba.hits_tag = c.tag;
    const bool fused = vx::launch_build_bricks3(g->words.as<uint32_t>(), g->g.dim, g->cdim, g->bricks.as<unsigned long long>(),
                                                fuse_mip1 ? g->cwords.as<uint32_t>() : nullptr, g->stream, ba);
    if (!fused) vx::launch_brick_mip1(g->bricks.as<unsigned long long>() + 2ull * nc * 8ull, nc, g->cwords.as<uint32_t>(), g->stream);
    if (c.from_tiled && c.line_counts) VX_TRY(p16_launch(g, c.tag));
    else vx::launch_build_mip2(g->cwords.as<uint32_t>(), g->cdim, g->c2dim, g->c2words.as<uint32_t>(), g->stream);
    g->coarse_valid = true;
    return VX_OK;
}

// the traversal structure of the grid's mask as it stands, built in front of the first query that needs it
vx_status ensure_coarse(vx_grid* g) { return build_coarse(g, CoarseBuild()); }

vx_status sync_counts(vx_grid* g)
{
    if (g->counts_valid) return VX_OK;
    DeviceGuard dg(g->device);
    unsigned long long part[vx::kCallCounters * 8];
    VX_HIP(hipMemcpyAsync(part, g->small.as<Small>()->set_calls, sizeof(part), hipMemcpyDeviceToHost, g->stream));
    VX_HIP(hipStreamSynchronize(g->stream));
    unsigned long long sc = 0;
    for (uint32_t i = 0; i < vx::kCallCounters; ++i) sc += part[8 * i];
    g->set_calls = sc + g->host_set_calls;
    g->counts_valid = true;
    return VX_OK;
}

// `clear`: zero the bitmask and the call counter now (false: the caller queues that itself)
vx_status init_grid_storage(vx_grid* g, bool clear = true)
{
    VX_HIP(ensure_small(g->small));
    if (!g->mail) VX_HIP(mail_alloc(g->mail));
    VX_HIP(g->words.ensure((size_t)(g->g.nwords + 2) * 4));
    if (clear) {
        VX_HIP(hipMemsetAsync(g->words.p, 0, (size_t)(g->g.nwords + 2) * 4, g->stream));
        VX_HIP(hipMemsetAsync(g->small.as<Small>()->set_calls, 0, sizeof(Small::set_calls), g->stream));
    }
    g->reset_derived(/*counts_known=*/false);  // (a fresh grid: the build or the caller's writes decide what it holds)
    return VX_OK;
}

// Second half of a VX_VOXELIZE_MATERIALS build: addMatrialIfNeeded (voxelgrid.hpp:102-114) gives a material the next index when the
// first setVoxel call carrying it arrives, i.e. values are numbered by the first triangle that uses them; then triangle -> value ->
// index for every voxel (Bool / AABBstruct: the last triangle per voxel) or call (Vec).
vx_status finish_materials(vx_grid* g, const long long* first_use, size_t nvalues)
{
    if (!g->mat_pending) return VX_OK;
    if (nvalues != g->mat_values.size()) return fail(VX_ERR_INVALID_ARG, "first-use array does not match the mesh's material values");
    DeviceGuard dg(g->device);
    hipStream_t s = g->stream;
    std::vector<size_t> used;
    for (size_t v = 0; v < nvalues; ++v)
        if (first_use[v] >= 0) used.push_back(v);
    std::sort(used.begin(), used.end(), [&](size_t a, size_t b) { return first_use[a] < first_use[b]; });
    std::vector<int16_t> vindex(nvalues, (int16_t)-1);
    g->materials.clear();
    for (size_t k = 0; k < used.size(); ++k) {
        vindex[used[k]] = (int16_t)k;
        g->materials.push_back(g->mat_values[used[k]]);
    }
    const uint32_t ntri = g->mat_ntri;
    const bool vec = g->kind == VX_GRID_VEC;
    uint8_t* base = g->mattmp.as<uint8_t>();
    uint32_t* last_tri = vec ? nullptr : reinterpret_cast<uint32_t*>(base);
    uint8_t* tri_hit = base + (vec ? 0 : (size_t)g->mat_nids * 4);
    int16_t* value_index = reinterpret_cast<int16_t*>(tri_hit + (((size_t)ntri + 63) & ~(size_t)63));
    VX_HIP(hipMemcpyAsync(value_index, vindex.data(), vindex.size() * 2, hipMemcpyHostToDevice, s));
    VX_HIP(g->matids.ensure((size_t)g->mat_nids * 2 + 16));
    if (g->mat_nids) {
        if (vec)
            vx::launch_mat_ids_calls(g->up.view(ntri, false), g->up.umask.as<uint32_t>(), g->up.hbase.as<uint32_t>(), g->mat_dtv, value_index, g->matids.as<int16_t>(), s);
        else
            vx::launch_mat_ids(last_tri, g->mat_nids, g->mat_dtv, value_index, g->matids.as<int16_t>(), s);
    }
    if (g->mat_interior && g->mat_first_use.size() && vindex[0] >= 0)  // solid build: the second loop's setVoxel calls carry MaterialObj{} (value 0)
        vx::launch_solid_ids(g->matids.as<int16_t>() + (vec ? g->mat_surface : 0), vec ? g->mat_interior : g->mat_nids, vindex[0], /*only_unset=*/!vec, s);
    VX_HIP(hipStreamSynchronize(s));  // vindex lives on this stack frame
    g->mat_count = g->mat_nids;
    g->has_materials = true;
    g->mat_pending = false;
    return VX_OK;
}

// Solid voxelization (vx_solid.hip): the interior H of the grid's complete bitmask is OR-ed into it; H in the reference's layout stays in
// *h_words with its word prefix in g->solid_pre (nwords + 1 entries) for the Vec list.  The host reads one mailbox word per batch of rounds
// and queues batches until a round is quiet: no cap on the rounds.  Grids with an axis of 1 or 2 cells have no interior (nothing queued).
vx_status solid_fill(vx_grid* g, uint64_t* n_interior, const uint32_t** h_words)
{
    *n_interior = 0;
    *h_words = nullptr;
    g->solid_rounds = 0;
    const uint32_t* dim = g->g.dim;
    if (dim[0] < 3 || dim[1] < 3 || dim[2] < 3) return VX_OK;
    hipStream_t s = g->stream;
    const vx::SolidPlan plan = vx::solid_plan(dim);
    VX_HIP(g->solid_e.ensure((size_t)plan.pwords * 4 + 16));
    if (plan.padded) {
        VX_HIP(g->solid_m.ensure((size_t)plan.pwords * 4 + 16));
        VX_HIP(g->solid_h.ensure((size_t)g->g.nwords * 4 + 16));
    }
    VX_HIP(g->solid_pre.ensure((size_t)(g->g.nwords + 2) * 4));
    VX_HIP(g->solid_agg.ensure((size_t)vx::solid_agg_words(dim) * 4 + 16));
    VX_HIP(g->up.scantmp.reserve(g->g.nwords, s));  // (ahead of the seed)
    uint32_t* flags = g->small.as<Small>()->solid_flags;
    uint32_t* words = g->words.as<uint32_t>();
    const uint32_t* m = plan.padded ? g->solid_m.as<uint32_t>() : words;
    uint32_t* ext = g->solid_e.as<uint32_t>();
    uint32_t prev = 2 * 32 - 1;  // the flag the first round reads: set by the seed (the other half of what batch 0 clears)
    vx::launch_solid_seed(words, g->solid_m.as<uint32_t>(), ext, dim, flags + prev, s);
    uint32_t batch = 4, rounds = 0;
    for (uint32_t k = 0;; ++k) {
        const uint32_t first = (k & 1u) * 32u;
        VX_HIP(hipMemsetAsync(flags + first, 0, batch * 4, s));
        for (uint32_t r = 0; r < batch; ++r) {
            vx::launch_solid_round(m, ext, g->solid_agg.as<uint32_t>(), dim, flags + prev, flags + first + r, s);
            prev = first + r;
        }
        const unsigned long long tag = next_tag(g);
        vx::launch_solid_report(flags + first, batch, &g->mail->solid_rounds, tag, s);
        uint64_t changed = 0;  // (at most `batch`)
        VX_TRY(mail_total(&g->mail->solid_rounds, tag, s, "solid fill: round count out of range", &changed));
        rounds += (uint32_t)changed;
        if (changed < batch) break;  // a quiet round: every round after it exited at once
        if (batch < 32) batch *= 2;
    }
    g->solid_rounds = rounds + 1;
    const DevBuf& h = plan.padded ? g->solid_h : g->solid_e;
    vx::launch_solid_finish(words, g->solid_m.as<uint32_t>(), ext, h.as<uint32_t>(), dim, g->g.nwords, s);
    const unsigned long long tag = next_tag(g);
    VX_TRY(g->up.scantmp.u32(h, g->solid_pre, g->g.nwords, true, &g->mail->interior, s, {tag}));
    VX_TRY(mail_total(&g->mail->interior, tag, s, "more than 2^32 interior voxels", n_interior));
    *h_words = h.as<uint32_t>();
    return VX_OK;
}

}  // namespace

// ============================================================================================================
extern "C" {

const char* vx_last_error(void) { return g_err.c_str(); }

const char* vx_status_string(vx_status s)
{
    switch (s) {
        case VX_OK: return "ok";
        case VX_ERR_INVALID_ARG: return "invalid argument";
        case VX_ERR_PATH: return "Path does not exist!";
        case VX_ERR_PARSE: return "Colud not get valid reader!";
        case VX_ERR_OUT_OF_BOUNDS: return "Index out of bounds";
        case VX_ERR_MORTON_BITS: return "We support up to 21 bits per axis (max 2^21 voxels per dimension)!";
        case VX_ERR_NO_DEVICE: return "no HIP device";
        case VX_ERR_HIP: return "HIP runtime error";
        case VX_ERR_CAPACITY: return "capacity exceeded";
        case VX_ERR_UNSUPPORTED: return "unsupported";
    }
    return "unknown";
}

int vx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

vx_status vx_set_device(int device)
{
    VX_TRY(need_device(device));
    g_device = device;
    return VX_OK;
}

vx_status vx_release_cached_memory(void)
{
    int n = vx_device_count();
    for (int d = 0; d < n && d < kMaxDev; ++d) {
        std::vector<FreeBlock> blocks;
        {
            std::lock_guard<std::mutex> lk(g_pool[d].mu);
            for (auto& kv : g_pool[d].free_blocks) blocks.push_back(kv.second);
            g_pool[d].free_blocks.clear();
        }
        if (blocks.empty()) continue;
        DeviceGuard dg(d);
        for (FreeBlock& fb : blocks) {
            if (fb.ev) (void)hipEventSynchronize(fb.ev);  // hipFree of a block that queued kernels still use would be the same race
            (void)hipFree(fb.p);
            if (fb.ev) { std::lock_guard<std::mutex> lk(g_pool[d].mu); g_pool[d].spare_events.push_back(fb.ev); }
        }
    }
    return VX_OK;
}

// ---- mesh ---------------------------------------------------------------------------------------------------
vx_status vx_mesh_load_obj(const char* path, vx_mesh** out)
{
    if (!path || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_mesh* m = new vx_mesh();
    std::string msg;
    vx::ObjAttributes attr;
    const int rc = vx::load_obj(path, m->hv, m->hi, m->tri_mat, m->materials, msg, &attr);
    if (rc == 1) { delete m; return fail(VX_ERR_PATH, "Path does not exist!"); }                                    // VoxelBuilder.hpp:54-56
    if (rc == 2) { delete m; return fail(VX_ERR_PARSE, "Colud not get valid reader! Error message " + msg); }        // :63-65
    m->nv = m->hv.size() / 3;
    m->nt = m->hi.size() / 3;
    if (m->materials.empty()) m->tri_mat.clear();  // no mtllib: every id is -1
    m->cnrm = std::move(attr.nrm);
    m->cuv = std::move(attr.uv);
    for (std::string& n : attr.tex_names) { m->tex.emplace_back(); m->tex.back().name = std::move(n); }
    m->mat_slot = std::move(attr.mat_slot);
    m->device = g_device;
    *out = m;
    return VX_OK;
}

vx_status vx_mesh_from_arrays(const float* xyz, size_t nv, const int32_t* idx, size_t nt, vx_mesh** out)
{
    if (!out || (nv && !xyz) || (nt && !idx)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (nv >= 0xFFFFFFFFull || nt >= 0xFFFFFFFEull) return fail(VX_ERR_CAPACITY, "mesh too large for 32-bit indices");
    for (size_t i = 0; i < nt * 3; ++i)
        if (idx[i] < 0 || (size_t)idx[i] >= nv) return fail(VX_ERR_INVALID_ARG, "triangle index out of range");
    vx_mesh* m = new vx_mesh();
    m->hv.assign(xyz, xyz + nv * 3);
    m->hi.assign(idx, idx + nt * 3);
    m->nv = nv;
    m->nt = nt;
    m->device = g_device;
    *out = m;
    return VX_OK;
}

vx_status vx_mesh_from_device(const float* dxyz, size_t nv, const int32_t* didx, size_t nt, vx_mesh** out)
{
    if (!out || (nv && !dxyz) || (nt && !didx)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (nv >= 0xFFFFFFFFull || nt >= 0xFFFFFFFEull) return fail(VX_ERR_CAPACITY, "mesh too large for 32-bit indices");
    VX_TRY(need_device(g_device));
    vx_mesh* m = new vx_mesh();
    m->nv = nv;
    m->nt = nt;
    m->dv = dxyz;
    m->di = didx;
    m->borrowed = true;
    m->device = g_device;
    *out = m;
    return VX_OK;
}

size_t vx_mesh_num_vertices(const vx_mesh* m) { return m ? m->nv : 0; }
size_t vx_mesh_num_triangles(const vx_mesh* m) { return m ? m->nt : 0; }
const float* vx_mesh_host_vertices(const vx_mesh* m) { return (m && !m->borrowed) ? m->hv.data() : nullptr; }
const int32_t* vx_mesh_host_indices(const vx_mesh* m) { return (m && !m->borrowed) ? m->hi.data() : nullptr; }
size_t vx_mesh_num_materials(const vx_mesh* m) { return m ? m->materials.size() : 0; }
vx_status vx_mesh_materials(const vx_mesh* m, vx_material* out, size_t cap)
{
    if (!m || (!out && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (cap < m->materials.size()) return fail(VX_ERR_CAPACITY, "material buffer too small");
    if (!m->materials.empty()) std::memcpy(out, m->materials.data(), m->materials.size() * sizeof(vx_material));
    return VX_OK;
}
const int32_t* vx_mesh_host_material_ids(const vx_mesh* m) { return (m && !m->tri_mat.empty()) ? m->tri_mat.data() : nullptr; }
vx_status vx_mesh_set_materials(vx_mesh* m, const vx_material* mats, size_t n, const int32_t* ids)
{
    if (!m || (n && !mats)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (n > 32767) return fail(VX_ERR_CAPACITY, "more than 32767 materials: per-voxel ids are int16 (voxelgrid.hpp:29)");
    if (ids)
        for (size_t t = 0; t < m->nt; ++t)
            if (ids[t] < -1 || (ids[t] >= 0 && (size_t)ids[t] >= n)) return fail(VX_ERR_INVALID_ARG, "material id out of range");
    m->materials.assign(mats, mats + n);
    if (ids && n) m->tri_mat.assign(ids, ids + m->nt); else m->tri_mat.clear();
    m->mat_slot.assign(n, -1);
    m->values_ready = false;
    return VX_OK;
}

// ---- corner attributes and textures (attribute shading of frames) ----------------------------------------------
const float* vx_mesh_host_corner_normals(const vx_mesh* m) { return (m && !m->cnrm.empty()) ? m->cnrm.data() : nullptr; }
const float* vx_mesh_host_corner_uvs(const vx_mesh* m) { return (m && !m->cuv.empty()) ? m->cuv.data() : nullptr; }
vx_status vx_mesh_set_attributes(vx_mesh* m, const float* corner_normals, const float* corner_uvs)
{
    if (!m) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (corner_normals) m->cnrm.assign(corner_normals, corner_normals + m->nt * 9); else m->cnrm.clear();
    if (corner_uvs) m->cuv.assign(corner_uvs, corner_uvs + m->nt * 6); else m->cuv.clear();
    return VX_OK;
}
size_t vx_mesh_num_textures(const vx_mesh* m) { return m ? m->tex.size() : 0; }
const char* vx_mesh_texture_name(const vx_mesh* m, size_t slot) { return (m && slot < m->tex.size()) ? m->tex[slot].name.c_str() : nullptr; }
const uint8_t* vx_mesh_host_texture(const vx_mesh* m, size_t slot, uint32_t* width, uint32_t* height)
{
    const bool ok = m && slot < m->tex.size() && m->tex[slot].w;
    if (width) *width = ok ? m->tex[slot].w : 0;
    if (height) *height = ok ? m->tex[slot].h : 0;
    return ok ? m->tex[slot].rgba.data() : nullptr;
}
const int32_t* vx_mesh_host_material_textures(const vx_mesh* m) { return (m && !m->mat_slot.empty()) ? m->mat_slot.data() : nullptr; }
vx_status vx_mesh_set_material_textures(vx_mesh* m, const int32_t* slots, size_t n)
{
    if (!m || (n && !slots)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (n != m->materials.size()) return fail(VX_ERR_INVALID_ARG, "one texture slot per material");
    m->mat_slot.assign(slots, slots + n);
    return VX_OK;
}
vx_status vx_mesh_set_texture(vx_mesh* m, int32_t slot, uint32_t width, uint32_t height, const uint8_t* rgba8)
{
    if (!m || !rgba8) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (slot < 0 || slot >= kMaxTextureSlots) return fail(VX_ERR_INVALID_ARG, "texture slot out of range");
    if (width < 1 || width > kMaxTextureSide || height < 1 || height > kMaxTextureSide) return fail(VX_ERR_INVALID_ARG, "texture width and height must be 1..16384");
    if ((size_t)slot >= m->tex.size()) m->tex.resize((size_t)slot + 1);
    vx_mesh::Texture& t = m->tex[(size_t)slot];
    t.w = width;
    t.h = height;
    t.rgba.assign(rgba8, rgba8 + (size_t)width * height * 4);
    return VX_OK;
}
vx_status vx_mesh_load_textures(vx_mesh* m)
{
    if (!m) return fail(VX_ERR_INVALID_ARG, "null argument");
    for (vx_mesh::Texture& t : m->tex) {
        if (!decode_image(t.name, t.w, t.h, t.rgba)) {  // hello_vulkan.cpp:318-327: a 1x1 magenta image stands in
            t.w = t.h = 1;
            t.rgba = {255, 0, 255, 255};
        }
    }
    return VX_OK;
}

void vx_mesh_free(vx_mesh* m)
{
    if (!m) return;
    if (m->uploaded || m->btv.p) {
        // grids on any stream may still be reading the vertex / index arrays: wait for the device before the blocks go back
        DeviceGuard dg(m->device);
        (void)hipDeviceSynchronize();
    }
    m->drained = true;  // (or nothing was ever queued on its blocks)
    delete m;
}

// ---- voxelize -------------------------------------------------------------------------------------------------
// What a build that failed after it queued work leaves (voxhip.h, vx_voxelize_into): a grid of 0 x 0 x 0 cells -- no words, no
// voxels, no setVoxel calls, an empty list and no materials; every ray misses.  Host state only: the error may be the device's.
static void grid_set_empty(vx_grid* g, float vs)
{
    const float zero3[3] = {0.f, 0.f, 0.f};
    const uint64_t zdim[3] = {0, 0, 0};
    fill_params(g->g, zero3, vs, zdim);
    for (int a = 0; a < 3; ++a) g->bbmin[a] = g->bbmax[a] = g->bbc[a] = 0.f;
    g->triangles = 0;
    g->reset_derived(/*counts_known=*/true);  // (an empty grid's counts are known: 0)
    g->vec_in_bound = false;
    g->list_deferred = false;  // (here only: a list of the previous build that was never emitted -- its records are gone with it)
    g->reset_materials();
    g->reset_solid();
}

// ---- the build: one record, named phases ("The build, phase by phase") ----------------------------------------------
// Everything one pass of a build decides and queues, handed from phase to phase.  A phase is an ordinary function of (grid, mesh, Build&);
// build_pass calls them in order.  The ORDER of what they queue -- kernels, memsets, waits -- is what the voxelize stage's time is made of.
struct Build {
    enum Next { kGoOn, kDone /*nothing (more) to voxelize: the build is complete*/, kAgain /*run the pass again without the early launch*/ };
    Next next = kGoOn;
    const vx_voxelize_opts* o = nullptr;
    float vs = 0.f;
    bool allow_early = true;
    hipStream_t s = nullptr;
    // plan_args: the decoded options
    bool want_mat = false, solid = false, list_async = false, by_rank = false, sharded_words = false;
    uint64_t tb = 0, te = 0;  // the triangle range ...
    uint32_t ntri = 0;        // ... and its length
    unsigned long long mtag = 0;  // sequence tag of this pass's totals in the mailbox
    // the early launch: the voxelizer queued before the host knows the unit total, sized by the previous build's buffers
    bool early = false;
    uint64_t unit_cap = 0;      // the units those buffers hold
    uint64_t btri_entries = 0;  // entries of the block table filled by the launch queued ahead of the unit total
    bool setup_queued = false;  // records and unit scan went out in front of the extent
    // cleared ahead of the host wait
    size_t cleared = 0;          // bytes of the build's mask ...
    bool cleared_tiled = false;  // ... of the tiled build mask, that is
    bool mask_is_clear = false;  // nothing is left to clear in g->words
    size_t mask_bytes = 0;
    Extent ex;
    uint64_t nvox = 0;
    // plan_grid
    uint64_t wb = 0, we = 0;  // the words this build owns
    bool whole_words = false, whole_build = false, tiled = false, untile_in_bricks = false, defer_scan = false, lines = false;
    bool wide = false;  // an axis above 65535 cells: the unit kernels also read the extension words of the candidate ranges
    // queued
    uint64_t U = 0, nUB = 0;  // units, blocks of 64 units
    uint32_t* umask = nullptr;
    uint32_t* bhits = nullptr;
    bool occ_queued = false;  // this build queued the scan that posts the occupied count under mtag
    uint64_t n_interior = 0;
    const uint32_t* h_words = nullptr;
};

// 1. plan from the arguments: pure host work
static void build_plan_args(vx_grid* g, const vx_mesh* mesh, Build& b)
{
    const vx_voxelize_opts& o = *b.o;
    b.want_mat = (o.flags & VX_VOXELIZE_MATERIALS) != 0;
    b.solid = (o.flags & VX_VOXELIZE_SOLID) != 0;
    // (the material ids need the hit bases on the main stream; a solid build appends the interior's records behind the triangles')
    b.list_async = (o.flags & VX_VOXELIZE_LIST_ASYNC) != 0 && g->kind == VX_GRID_VEC && !b.want_mat && !b.solid;
    g->reset_solid();
    g->reset_materials();
    b.by_rank = o.shard_world > 1 && !(o.word_begin || o.word_end);
    b.tb = 0;
    b.te = mesh->nt;
    if (o.tri_begin || o.tri_end) {
        b.tb = o.tri_begin;
        b.te = o.tri_end;
    }
    b.ntri = (uint32_t)(b.te - b.tb);
    b.sharded_words = o.word_begin || o.word_end || b.by_rank;
    b.mtag = next_tag(g);
    // A VX_VOXELIZE_LIST_ASYNC rebuild (nothing queued inside the build but the voxelizer reads a buffer sized by the unit total U): the host
    // waits for the BBOX only -- k_bbox posts a tag of its own -- and queues the voxelizer and everything behind it while the record kernel
    // and the unit scan still run, instead of leaving the GPU idle for a mailbox round trip plus a launch (8-12 us) behind the scan.  The
    // voxelizer finds U in device memory (the scan's total goes there, and on to the mailbox with k_unit_blocks) and does nothing when U
    // exceeds what the handle's buffers from the previous build hold; the host reads U in the wait for the hit count and only then, or with
    // 2^32 units or more, goes the way of a first build: U first, buffers, the same kernels again.
    const UnitPipe& up = g->up;
    b.early = b.allow_early && b.ntri > 0 && !b.sharded_words && b.list_async && up.umask.cap >= 64 && up.bhits.cap >= 64 && up.hbase.cap >= 64 && up.btri.cap >= 64;
}

// 2a. front, the queue: bbox, triangle records and unit scan, the block table ahead of the total, the early clear
// Unsharded build: K1 leaves origin + dims in device memory, so the triangle records and the unit scan are queued right
// behind it and the host waits ONCE for the bbox and the unit count (every host round trip costs ~20 us of idle GPU: the
// wake-up plus the launch latency of an empty queue).  The bitmask of the previous build is cleared in the same window.
// (a word shard's z slab is derived from the device-side dims by the record kernel itself)
static vx_status build_front_queue(vx_grid* g, vx_mesh* mesh, Build& b)
{
    const vx_voxelize_opts& o = *b.o;
    Small* ds = g->small.as<Small>();
    UnitPipe& up = g->up;
    vx::GridParams gp{};
    const float zero3[3] = {0.f, 0.f, 0.f};
    const uint64_t zdim[3] = {0, 0, 0};
    fill_params(gp, zero3, b.vs, zdim);
    vx::launch_bbox(mesh->dv, mesh->nv, ds->bbox_state, g->mail->bbox, ds->set_calls, b.s, b.vs, &ds->dgrid, b.early ? &g->mail->bbox_tag : nullptr, b.mtag);
    // the previous build's bitmask is cleared in the same window -- by the record kernel's own threads when there are enough of
    // them (at most 256 bytes each), by a memset behind the block table otherwise
    // (a handle whose previous build went through the tiled build mask is expected to do so again: that is the buffer to clear)
    DevBuf& cb = (g->last_tiled && g->twords.p) ? g->twords : g->words;
    b.cleared_tiled = &cb == &g->twords;
    const bool clear_in_setup = cb.p && (cb.cap % 16) == 0 && cb.cap / 256 <= (size_t)b.ntri;
    SetupOpts so;
    so.dgrid = &ds->dgrid;
    so.tag = b.mtag;
    if (clear_in_setup) {
        so.clear = cb.p;
        so.clear_bytes = cb.cap;
    }
    if (b.sharded_words) {
        so.shard_wb = o.word_begin;
        so.shard_we = o.word_end;
    }
    if (b.by_rank) {
        so.shard_rank = (uint32_t)o.shard_rank;
        so.shard_world = (uint32_t)o.shard_world;
    }
    if (b.early) so.units_total = &ds->units64;
    VX_TRY(up.setup_launch(mesh, gp, o.sat_variant, b.tb, b.ntri, 0, 0, g->mail.get(), b.s, so));
    if (clear_in_setup) b.cleared = cb.cap;
    // the block table of the units: queued now, for as many blocks as the handle's table from the previous build holds, so that
    // it runs while the host waits for the unit total (redone by setup_finish should the table turn out too small)
    if (up.btri.p && up.btri.cap >= 64) {
        b.btri_entries = up.btri.cap / 4;
        if (b.btri_entries > 0x3FFFFFFull) b.btri_entries = 0x3FFFFFFull;
        vx::UnitBlockArgs ua;
        ua.cap_blocks = (uint32_t)b.btri_entries;
        if (b.early) {
            // the units the buffers of the previous build hold; the hit scan runs over the blocks of that many units, so the entries
            // behind this build's last block are zeroed on the way
            b.unit_cap = std::min(std::min((uint64_t)up.umask.cap / 4 - 1, ((uint64_t)up.bhits.cap / 4 - 4) * 64),
                                  std::min(((uint64_t)up.hbase.cap / 4 - 4) * 64, (b.btri_entries - 2) * 64));
            ua.fwd_src = &ds->units64;
            ua.fwd_dst = &g->mail->units;
            ua.zero_hits = up.bhits.as<uint32_t>();
        }
        ua.zero_n = (uint32_t)((b.unit_cap + 63) / 64);
        vx::launch_unit_blocks(up.view(b.ntri, false), (uint32_t)((b.btri_entries - 2) * 64), up.btri.as<uint32_t>(), b.s, ua);
    }
    if (cb.p && !clear_in_setup) {
        VX_HIP(hipMemsetAsync(cb.p, 0, cb.cap, b.s));
        b.cleared = cb.cap;
    }
    return VX_OK;
}

// 2. front: what goes out ahead of the extent, the build's single host wait, the extent, the grid's storage
static vx_status build_front(vx_grid* g, vx_mesh* mesh, Build& b)
{
    if (b.ntri > 0) {
        VX_TRY(build_front_queue(g, mesh, b));
        if (b.early) {
            if (!mail_wait(&g->mail->bbox_tag, nullptr, b.mtag, 5.0)) VX_HIP(hipStreamSynchronize(b.s));
            std::atomic_thread_fence(std::memory_order_acquire);
        } else {
            // the bbox (written by k_bbox, two kernels earlier) and the unit total: polled from the mailbox, see the hit count below
            if (!mail_wait(&g->mail->units, nullptr, b.mtag, 5.0)) VX_HIP(hipStreamSynchronize(b.s));
        }
        VX_TRY(extent_from_bbox(g->mail->bbox, mesh->nv, b.vs, &b.ex));
        b.setup_queued = true;
    } else {
        b.early = false;
        VX_TRY(compute_extent(mesh, b.vs, g->small.as<Small>(), g->mail.get(), b.s, &b.ex));  // also clears the per-build call counter
    }
    b.nvox = b.ex.dim[0] * b.ex.dim[1] * b.ex.dim[2];
    if (b.nvox > kMaxVoxels) return fail(VX_ERR_CAPACITY, "grid exceeds 2^37 voxels");
    fill_params(g->g, b.ex.mn, b.vs, b.ex.dim);
    for (int a = 0; a < 3; ++a) { g->bbmin[a] = b.ex.mn[a]; g->bbmax[a] = b.ex.mx[a]; g->bbc[a] = b.ex.ctr[a]; }
    VX_TRY(init_grid_storage(g, /*clear=*/false));
    b.mask_bytes = (size_t)(g->g.nwords + 2) * 4;
    if (g->words.fresh) { if (!b.cleared_tiled) b.cleared = 0; g->words.fresh = false; }  // a new block: the early clear hit the old one
    b.mask_is_clear = !b.cleared_tiled && b.cleared >= b.mask_bytes;
    return VX_OK;
}

// 3. plan from the grid: pure host work -- the words this build owns and the form its mask takes
static vx_status build_plan_grid(vx_grid* g, const vx_mesh* mesh, Build& b)
{
    const vx_voxelize_opts& o = *b.o;
    b.wb = 0;
    b.we = g->g.nwords;
    if (b.by_rank) {
        vx_shard_words(g->g.nwords, o.shard_rank, o.shard_world, &b.wb, &b.we, nullptr);
    } else if (b.sharded_words) {
        if (o.word_end > g->g.nwords) return fail(VX_ERR_INVALID_ARG, "word shard out of range");
        b.wb = o.word_begin;
        b.we = o.word_end;
    }
    b.whole_build = b.wb == 0 && b.we == g->g.nwords && b.tb == 0 && b.te == mesh->nt;
    g->triangles = b.te - b.tb;
    // Unsharded words, rows of whole words: the voxelizer ORs into the tiled build mask (one atomic request per 4 x 4 rows instead of one per
    // row, launch_voxelize) and launch_untile writes every word of the reference's bitmask from it.  Ragged rows take the direct form.
    b.whole_words = b.wb == 0 && b.we == g->g.nwords;
    // (a word shard goes the same way: the voxelizer keeps to the rows whose words it owns, launch_untile writes those and zeroes the rest --
    // a second pass over the WHOLE mask per rank, so only where the mask is small against the mesh: the size rule of the clear that rides in
    // the record kernel's threads.  atrium262k, two logical ranks on one GPU: 512^3 voxelize stage 121 -> 95 us; 1024^3 392 -> 426, hence the rule)
    // ... and only for shards of a fifth of the mask or more: shard 0 of 2 / 4 / 8 at 512^3 (tools/shard_time.py, kernels of a rebuild)
    // 119.7 -> 97.9 / 90.6 -> 73.3 / 55.1 -> 64.0 us -- at an eighth the un-tiling pass costs what the voxelizer no longer has to gain
    const bool shard_small = (size_t)vx::tiled_mask_words(g->g.dim) * 4 / 256 <= (size_t)b.ntri && (b.we - b.wb) * 5 >= g->g.nwords;
    b.tiled = (b.whole_words || shard_small) && (b.ex.dim[0] % 32) == 0;
    // (the tiled mask -> the reference's bitmask: by the brick kernel on its way when the traversal structure is built right away)
    // (VX_VOXELIZE_SOLID: the fill reads and extends the reference's bitmask, the traversal structure is built from the final one)
    b.untile_in_bricks = b.tiled && b.whole_words && !b.solid;
    // A list_async rebuild whose brick kernel follows at once: nothing queued in the build reads the hit bases -- the block-hit scan stood
    // there for its total, the list's length -- so the brick kernel posts that total from the voxelizer's own counters and the scan goes in
    // front of the emission (list_scan).  Everything else keeps the scan in the build.
    b.defer_scan = b.early && b.untile_in_bricks;
    // (a Vec build's consumers -- the ray batch's rank pass -- read wp16 only: from the brick kernel's line counts where a line lies in
    // one row, i.e. X % 512 == 0, which makes nwords a multiple of 16 as the rank pass's 16-word path needs it.  The Bool flavours emit
    // their list from the word prefix right away, materials index it: the word-prefix scan)
    b.lines = b.untile_in_bricks && g->kind == VX_GRID_VEC && !b.want_mat && (b.ex.dim[0] % 512) == 0;
    b.wide = b.ex.dim[0] > 65535 || b.ex.dim[1] > 65535 || b.ex.dim[2] > 65535;
    return VX_OK;
}

// a build without a setVoxel call: no material is ever used
static vx_status build_no_calls(vx_grid* g, const vx_mesh* mesh, Build& b)
{
    b.next = Build::kDone;
    if (!b.want_mat) return VX_OK;
    g->mat_pending = true;
    g->mat_values = mesh->values;
    g->mat_first_use.assign(mesh->values.size(), -1);
    g->mat_dtv = nullptr; g->mat_ntri = 0; g->mat_nids = 0;
    VX_HIP(g->mattmp.ensure(mesh->values.size() * 2 + 256));
    if (b.whole_build) return finish_materials(g, g->mat_first_use.data(), g->mat_first_use.size());
    return VX_OK;
}

// 4. masks and unit total: what is left to clear, and U the early way, from the setup queued in the front, or behind a word shard's own setup
static vx_status build_masks_units(vx_grid* g, vx_mesh* mesh, Build& b)
{
    const vx_voxelize_opts& o = *b.o;
    hipStream_t s = b.s;
    if (b.ntri == 0 || b.nvox == 0 || b.wb == b.we) {
        if (!b.mask_is_clear) VX_HIP(hipMemsetAsync(g->words.p, 0, b.mask_bytes, s));
        return build_no_calls(g, mesh, b);
    }
    g->last_tiled = b.tiled;
    if (b.tiled) {
        const size_t tbytes = (size_t)vx::tiled_mask_words(g->g.dim) * 4;
        VX_HIP(g->twords.ensure(tbytes));
        const bool tw_clear = b.cleared_tiled && b.cleared >= tbytes && !g->twords.fresh;
        g->twords.fresh = false;
        if (!tw_clear) VX_HIP(hipMemsetAsync(g->twords.p, 0, tbytes, s));
        b.mask_is_clear = true;  // every word of the mask and the two spare words behind it are written by launch_untile (or the brick kernel) --
                                 // or, when there is no unit to run, by the memset below
    }
    if (b.early) {
        if (!b.mask_is_clear) VX_HIP(hipMemsetAsync(g->words.p, 0, b.mask_bytes, s));
        b.U = b.unit_cap;  // (what the buffers below are sized for: they are the previous build's)
    } else if (b.setup_queued) {
        if (!b.mask_is_clear) VX_HIP(hipMemsetAsync(g->words.p, 0, b.mask_bytes, s));
        VX_TRY(g->up.setup_finish(b.ntri, g->mail.get(), s, &b.U, /*stream_is_drained=*/true, b.btri_entries));
    } else {
        // z slab that contains the voxels of words [wb, we)
        const uint64_t XY = b.ex.dim[0] * b.ex.dim[1];
        const uint32_t zlo = (uint32_t)((b.wb * 32) / XY);
        uint64_t zh = (b.we * 32 + XY - 1) / XY;
        if (zh > b.ex.dim[2]) zh = b.ex.dim[2];
        // records + unit scan are queued, THEN the bitmask is cleared (it does not depend on the unit count), then the host waits
        VX_TRY(g->up.setup_launch(mesh, g->g, o.sat_variant, b.tb, b.ntri, zlo, (uint32_t)zh, g->mail.get(), s));
        VX_HIP(hipMemsetAsync(g->words.p, 0, b.mask_bytes, s));
        VX_TRY(g->up.setup_finish(b.ntri, g->mail.get(), s, &b.U));
    }
    if (b.U == 0) {  // (e.g. a word shard whose z slab holds no triangle): nothing will write the mask
        if (b.tiled) VX_HIP(hipMemsetAsync(g->words.p, 0, b.mask_bytes, s));
        return build_no_calls(g, mesh, b);
    }
    return VX_OK;
}

// 5. the voxelizer, the un-tiling pass where the brick kernel does not do it, the block-hit scan or its deferral, the solid fill
static vx_status build_voxelize(vx_grid* g, vx_mesh*, Build& b)
{
    hipStream_t s = b.s;
    UnitPipe& up = g->up;
    Small* ds = g->small.as<Small>();
    if (g->kind == VX_GRID_VEC || b.want_mat) {
        VX_HIP(up.umask.ensure((size_t)(b.U + 1) * 4));
        b.umask = up.umask.as<uint32_t>();
    }
    // VoxelGridVec::setVoxel appends one Aabb per call (voxelgridVecEncoding.cpp:19-39): ordered emission, at the exclusive scan of the
    // hit counts -- two-level: the voxelizer leaves the hits of every block of 64 units, the device scan runs over those
    b.nUB = (b.U + 63) / 64;
    if (g->kind == VX_GRID_VEC) {
        VX_HIP(up.bhits.ensure((size_t)(b.nUB + 4) * 4));
        VX_HIP(up.hbase.ensure((size_t)(b.nUB + 4) * 4));
        b.bhits = up.bhits.as<uint32_t>();
    }
    vx::VoxelizeArgs va;
    va.block_hits = b.bhits;
    va.tiled = b.tiled;
    va.units_total = b.early ? &ds->units64 : nullptr;
    va.unit_cap = (uint32_t)b.unit_cap;
    vx::launch_voxelize(up.view(b.ntri, b.wide), g->g, b.o->sat_variant, b.tiled ? g->twords.as<uint32_t>() : g->words.as<uint32_t>(), b.wb, b.we, b.umask, ds->set_calls, s, va);
    if (b.tiled && !b.untile_in_bricks) vx::launch_untile(g->twords.as<uint32_t>(), g->words.as<uint32_t>(), g->g.dim, s, b.wb, b.we);
    g->counts_valid = false;
    if (b.defer_scan) {
        VX_HIP(g->hscantmp.reserve(b.nUB, s));  // (the scan itself: list_scan)
    } else if (g->kind == VX_GRID_VEC) {
        VX_TRY(up.scantmp.u32(up.bhits, up.hbase, b.nUB, false, &g->mail->hits, s, {b.mtag}));
    }
    // VX_VOXELIZE_SOLID: the second loop -- setVoxel on every interior cell in ascending order -- once the surface mask is complete
    if (b.solid) {
        VX_TRY(solid_fill(g, &b.n_interior, &b.h_words));
        g->interior = b.n_interior;
        g->host_set_calls += b.n_interior;
    }
    return VX_OK;
}

// 6. A complete (unsharded) bitmask: queue what every consumer of the grid needs next -- the traversal structure (bricks,
// bounds, mips = the reference's acceleration-structure build, hello_vulkan.cpp:700-703) and the word prefix (getAabbs /
// primitive ids), or the line counts' scan in its place -- behind the voxelizer instead of lazily in front of the first query.  For the
// Vec flavour this work runs while the host waits for the hit count.  A word shard's stay lazy (ensure_coarse / ensure_prefix in the
// query paths).
static vx_status build_structure(vx_grid* g, vx_mesh*, Build& b)
{
    if (!b.whole_words) return VX_OK;
    if (b.lines) VX_HIP(g->lcnt.ensure((size_t)(g->g.nwords / 16 + 4) * 4));
    CoarseBuild c;
    c.from_tiled = b.untile_in_bricks;
    c.line_counts = b.lines;
    c.tag = b.mtag;
    c.post_hits = b.defer_scan;
    VX_TRY(build_coarse(g, c));
    if (b.lines) {
        b.occ_queued = true;
    } else {
        bool pending = false;
        b.occ_queued = !g->prefix_valid;
        VX_TRY(prefix_launch(g, &pending, b.mtag));
    }
    return VX_OK;
}

// 7a. The host needs the hit count (and takes the occupied count along).  Both are written by scans -- the hit count of a build that
// left its block-hit scan to the list (defer_scan) by the brick kernel, from the voxelizer's counters -- that run BEFORE the
// emission: the host polls the mailbox words for the build's tag and goes on queueing work (the caller's next call: a trace) while
// the emission still runs; a stream synchronize would wake it ~15 us after the last kernel.  5 ms without an answer: the synchronize.
// VX_VOXELIZE_LIST_ASYNC: only the hit count -- its scan runs in front of the traversal structure and the word prefix, so the host
// is back in the caller ~40 us of GPU work before the build ends and the caller's ray batch is queued in time; the occupied count
// (the LAST kernel's total) is fetched when somebody asks for it (prefix_finish).
// *units_known: the true unit total.  An early launch whose buffers it outgrew: they grow, and next = kAgain.
static vx_status build_list_wait(vx_grid* g, Build& b, uint64_t* hits, uint64_t* units_known)
{
    hipStream_t s = b.s;
    const bool occ_in_flight = (g->prefix_valid || g->p16_valid) && !g->occupied_known;
    const bool occ_along = occ_in_flight && !(b.list_async && b.occ_queued);
    bool got = false;  // (an occupied count in flight that this build did not queue carries another tag: the stream is drained for it)
    if (!occ_along || b.occ_queued) got = mail_wait(&g->mail->hits, occ_along ? &g->mail->occupied : nullptr, b.mtag, 5.0);
    if (!got) VX_HIP(hipStreamSynchronize(s));
    *units_known = b.U;
    if (b.early) {
        // the unit total, in the mailbox since k_unit_blocks: checked as setup_finish checks it.  More units than the early launch's
        // buffers hold: the voxelizer did nothing -- the buffers grow and the build runs again the way of a first build
        if ((g->mail->units & ~kMailValue) != b.mtag) VX_HIP(hipStreamSynchronize(s));
        uint64_t tot = 0;
        VX_TRY(mail_value(&g->mail->units, "more than 2^32 candidate row segments: shard the mesh or the grid", &tot));
        if (tot > b.unit_cap) {
            VX_HIP(hipStreamSynchronize(s));  // (the kernels of this pass read the blocks that are about to be replaced)
            VX_HIP(g->up.umask.ensure((size_t)(tot + 1) * 4));
            VX_HIP(g->up.bhits.ensure((size_t)(tot / 64 + 5) * 4));
            VX_HIP(g->up.hbase.ensure((size_t)(tot / 64 + 5) * 4));
            VX_HIP(g->up.btri.ensure((size_t)(tot / 64 + 2) * 4));
            b.next = Build::kAgain;
            return VX_OK;
        }
        *units_known = tot;
    }
    VX_TRY(mail_value(&g->mail->hits, "more than 2^32 voxel hits", hits));
    if ((g->prefix_valid || g->p16_valid) && (occ_along || !got)) {  // the same wait covered the occupied count
        VX_TRY(mail_value(&g->mail->occupied, "more than 2^32 occupied voxels", &g->occupied));
        g->occupied_known = true;
    }
    return VX_OK;
}

// 7. the Vec list: emitted into the handle's existing buffer before the host knows the hit count (writes beyond the buffer's
// capacity are dropped by the kernel); only a list that outgrew it is emitted again after the wait -- or, VX_VOXELIZE_LIST_ASYNC, recorded
// for whoever queues it (g->ld)
static vx_status build_list(vx_grid* g, vx_mesh*, Build& b)
{
    hipStream_t s = b.s;
    UnitPipe& up = g->up;
    const vx::Units units = up.view(b.ntri, b.wide);
    const bool to_bound = g->bound != nullptr && g->bound_cap > 0;
    vx_aabb* tgt = to_bound ? g->bound : g->vec.as<vx_aabb>();
    const uint64_t cap_rec = to_bound ? g->bound_cap + 1 : (g->vec.p ? g->vec.cap / sizeof(vx_aabb) : 0);
    g->vec_in_bound = false;
    if (cap_rec && !b.list_async) vx::launch_emit_units(units, g->g, b.umask, up.hbase.as<uint32_t>(), tgt, nullptr, s, to_bound ? g->bound_cap : cap_rec);
    uint64_t hits = 0, units_known = 0;
    VX_TRY(build_list_wait(g, b, &hits, &units_known));
    if (b.next == Build::kAgain) return VX_OK;
    const uint64_t total = hits + b.n_interior;  // (a solid build: the interior's records follow the triangles')
    if (total >= 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^32 voxel records");
    if (total + 1 <= cap_rec) g->vec_in_bound = to_bound;
    if (total + 1 > cap_rec) VX_HIP(g->vec.ensure((size_t)(total + 1) * sizeof(vx_aabb)));
    if (b.list_async) {
        // VX_VOXELIZE_LIST_ASYNC: the count is known, the records are written later -- beside the next ray batch (trace_common), or
        // on this stream by whatever asks for them first (list_resolve)
        g->ld.from_mask = false;
        g->ld.ntri = b.ntri;
        g->ld.ext = b.wide;
        g->ld.tgt = g->vec_ptr();
        g->ld.cap = g->vec_in_bound ? g->bound_cap : ~0ull;
        g->list_deferred = hits != 0;
        g->ld.scan_blocks = b.defer_scan && hits ? (units_known + 63) / 64 : 0;  // (the true unit total: the build's own blocks, not the buffers')
    } else if (total + 1 > cap_rec) {
        vx::launch_emit_units(units, g->g, b.umask, up.hbase.as<uint32_t>(), g->vec.as<vx_aabb>(), nullptr, s);
    }
    if (b.n_interior)  // cell_aabb of every interior cell in ascending order, at offset `hits`
        vx::launch_emit_bool_aabbs(b.h_words, g->solid_pre.as<uint32_t>(), g->g, g->vec_ptr() + hits, b.n_interior, s);
    g->vec_count = total;
    g->mat_surface = hits;
    return VX_OK;
}

// 8. per-voxel material ids (see k_mat_last): needs the word prefix (queued above for an unsharded build) and, for the Vec
// flavour, the hit bases.  First half here: the last triangle per voxel of this shard and, per material value, the first
// triangle of this shard that uses it; second half (finish_materials) once the first uses of ALL shards are known -- at once
// for a whole build.
static vx_status build_materials(vx_grid* g, vx_mesh* mesh, Build& b)
{
    hipStream_t s = b.s;
    const uint32_t ntri = b.ntri;
    bool pending = false;
    VX_TRY(prefix_launch(g, &pending));
    VX_TRY(prefix_finish(g, pending));
    const uint64_t nids = g->kind == VX_GRID_VEC ? g->vec_count : g->occupied;
    const size_t tmp_bytes = (g->kind == VX_GRID_VEC ? 0 : (size_t)nids * 4) + (size_t)ntri + 64 + mesh->values.size() * 2 + 64;
    VX_HIP(g->mattmp.ensure(tmp_bytes));
    uint8_t* base = g->mattmp.as<uint8_t>();
    uint32_t* last_tri = g->kind == VX_GRID_VEC ? nullptr : reinterpret_cast<uint32_t*>(base);
    uint8_t* tri_hit = base + (g->kind == VX_GRID_VEC ? 0 : (size_t)nids * 4);
    VX_HIP(hipMemsetAsync(base, 0, (size_t)(tri_hit - base) + ntri, s));
    vx::launch_mat_last(g->up.view(ntri, b.wide), g->g, b.umask, g->words.as<uint32_t>(), g->wprefix.as<uint32_t>(), last_tri, tri_hit, s);
    std::vector<uint8_t> hit(ntri);
    VX_HIP(hipMemcpyAsync(hit.data(), tri_hit, ntri, hipMemcpyDeviceToHost, s));
    VX_HIP(hipStreamSynchronize(s));
    g->mat_values = mesh->values;
    g->mat_first_use.assign(mesh->values.size(), -1);
    const int32_t* tv = mesh->tri_value.data() + b.tb;
    for (uint32_t t = 0; t < ntri; ++t)
        if (hit[t] && g->mat_first_use[(size_t)tv[t]] < 0) g->mat_first_use[(size_t)tv[t]] = (long long)(b.tb + t);
    // the interior's calls come after every triangle's and carry MaterialObj{} (value 0): addMatrialIfNeeded appends it if no triangle used it
    g->mat_interior = b.n_interior;
    if (b.n_interior && g->mat_first_use[0] < 0) g->mat_first_use[0] = (long long)(b.tb + ntri);
    g->mat_dtv = mesh->btv.as<int32_t>() + b.tb;
    g->mat_ntri = ntri;
    g->mat_nids = nids;
    g->mat_pending = true;
    if (b.whole_build) VX_TRY(finish_materials(g, g->mat_first_use.data(), g->mat_first_use.size()));
    return VX_OK;
}

// one pass over the phases
static vx_status build_pass(vx_grid* g, vx_mesh* mesh, Build& b)
{
    g->set_stream((hipStream_t)b.o->stream);
    b.s = g->stream;
    // a list emission of the previous build that is still to come reads the unit masks, hit bases and records this build overwrites (one
    // that was never queued is dropped: its list is about to be replaced)
    VX_HIP(g->list_resolve(/*drop_unqueued=*/true));
    VX_HIP(ensure_small(g->small));
    if (!g->mail) VX_HIP(mail_alloc(g->mail));
    build_plan_args(g, mesh, b);
    VX_TRY(build_front(g, mesh, b));
    VX_TRY(build_plan_grid(g, mesh, b));
    VX_TRY(build_masks_units(g, mesh, b));
    if (b.next == Build::kDone) return VX_OK;
    VX_TRY(build_voxelize(g, mesh, b));
    VX_TRY(build_structure(g, mesh, b));
    if (g->kind == VX_GRID_VEC) {
        VX_TRY(build_list(g, mesh, b));
        if (b.next == Build::kAgain) return VX_OK;
    }
    if (b.want_mat) VX_TRY(build_materials(g, mesh, b));
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// At most two passes: a list-async rebuild that outgrew the buffers its early launch was sized by runs again with the total known.
static vx_status voxelize_build(vx_mesh* mesh, float vs, const vx_voxelize_opts& o, vx_grid* g)
{
    for (int pass = 0;; ++pass) {
        Build b;
        b.o = &o;
        b.vs = vs;
        b.allow_early = pass == 0;
        VX_TRY(build_pass(g, mesh, b));
        if (b.next != Build::kAgain) return VX_OK;
    }
}

vx_status vx_voxelize_into(const vx_mesh* mesh_c, float vs, const vx_voxelize_opts* opts, vx_grid* g)
{
    if (!mesh_c || !g) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(check_voxel_size(vs));
    vx_mesh* mesh = const_cast<vx_mesh*>(mesh_c);
    VX_TRY(need_device(g->device));
    if (mesh->device != g->device) return fail(VX_ERR_INVALID_ARG, "mesh and grid live on different devices");
    vx_voxelize_opts o{};
    if (opts) o = *opts;
    // Errors the arguments alone tell (and the mesh's own: its upload, its material table): found before anything touches the
    // handle, which keeps its previous build (voxhip.h)
    if (o.sat_variant != 0 && o.sat_variant != 1) return fail(VX_ERR_INVALID_ARG, "sat_variant must be 0 or 1");
    if (o.shard_world < 0 || (o.shard_world > 0 && (o.shard_rank < 0 || o.shard_rank >= o.shard_world))) return fail(VX_ERR_INVALID_ARG, "shard_rank / shard_world out of range");
    if ((o.tri_begin || o.tri_end) && (o.tri_begin > o.tri_end || o.tri_end > mesh->nt)) return fail(VX_ERR_INVALID_ARG, "triangle shard out of range");
    if (o.word_begin > o.word_end) return fail(VX_ERR_INVALID_ARG, "word shard out of range");
    if ((o.flags & VX_VOXELIZE_SOLID) && (o.word_begin || o.word_end || o.shard_world > 1 || o.tri_begin || o.tri_end))
        return fail(VX_ERR_INVALID_ARG, "VX_VOXELIZE_SOLID needs the whole grid: no word shard, no triangle range");
    DeviceGuard dg(g->device);
    VX_TRY(mesh_to_device(mesh));
    if (o.flags & VX_VOXELIZE_MATERIALS) VX_TRY(mesh_material_values(mesh));
    // ... every later error: the handle is left empty, whatever the build had queued or changed by then
    const vx_status st = voxelize_build(mesh, vs, o, g);
    if (st != VX_OK) grid_set_empty(g, vs);
    return st;
}

vx_status vx_voxelize(const vx_mesh* mesh, float vs, vx_grid_kind kind, const vx_voxelize_opts* opts, vx_grid** out)
{
    if (!mesh || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (kind != VX_GRID_BOOL && kind != VX_GRID_AABBSTRUCT && kind != VX_GRID_VEC) return fail(VX_ERR_INVALID_ARG, "unknown grid kind");
    Fresh<vx_grid> g(new vx_grid());
    g->kind = kind;
    g->device = mesh->device;
    VX_TRY(vx_voxelize_into(mesh, vs, opts, g.get()));
    *out = g.release();
    return VX_OK;
}

// ---- multi-GPU build inside one process -----------------------------------------------------------------------------
// vx_multi: the persistent form.  Created once per (mesh, device list): the mesh is uploaded to every device, every rank gets a
// grid handle and a worker thread that lives as long as the context.  vx_multi_voxelize then runs with no upload, no allocation
// (the grids' buffers are reused when sizes repeat) and no thread start: rank k voxelizes the word shard vx_shard_words(.., k, n)
// that it derives from its own bounding-box pass (vx_voxelize_opts.shard_rank / shard_world: nobody needs the grid's word count
// beforehand), the shards travel as peer copies, the destination grids rebuild word prefix and traversal structure.
struct vx_multi {
    int nd = 0;
    vx_grid_kind kind = VX_GRID_BOOL;
    std::vector<int> devices;
    std::vector<vx_mesh*> meshes;
    std::vector<vx_grid*> grids;
    // workers
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    uint64_t epoch = 0;       // bumped by vx_multi_voxelize: the workers' signal
    int remaining = 0;        // workers still busy with the current epoch
    bool quit = false;
    float vs = 0.f;
    vx_voxelize_opts opts{};
    std::vector<vx_status> st;
    std::vector<std::string> msg;
};

namespace {
void multi_worker(vx_multi* m, int k)
{
    g_device = m->devices[(size_t)k];  // thread-local
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv_go.wait(lk, [&] { return m->quit || m->epoch != seen; });
            if (m->quit) return;
            seen = m->epoch;
        }
        vx_voxelize_opts o = m->opts;
        o.shard_rank = k;
        o.shard_world = m->nd;
        o.word_begin = o.word_end = o.tri_begin = o.tri_end = 0;
        const vx_status s = vx_voxelize_into(m->meshes[(size_t)k], m->vs, &o, m->grids[(size_t)k]);
        m->st[(size_t)k] = s;
        if (s != VX_OK) m->msg[(size_t)k] = g_err;
        else {  // the shard must be complete before another device copies it
            DeviceGuard dg(m->grids[(size_t)k]->device);
            (void)hipStreamSynchronize(m->grids[(size_t)k]->stream);
        }
        {
            std::lock_guard<std::mutex> lk(m->mu);
            if (--m->remaining == 0) m->cv_done.notify_all();
        }
    }
}
}  // namespace

vx_status vx_multi_create(const vx_mesh* mesh, const int* devices, int nd, vx_grid_kind kind, vx_multi** out)
{
    if (!mesh || !devices || !out || nd < 1) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (kind != VX_GRID_BOOL && kind != VX_GRID_AABBSTRUCT)
        return fail(VX_ERR_UNSUPPORTED, "multi-GPU builds are VX_GRID_BOOL / VX_GRID_AABBSTRUCT (VX_GRID_VEC's list order needs triangle shards)");
    if (mesh->borrowed) return fail(VX_ERR_UNSUPPORTED, "multi-GPU builds need a mesh with host arrays (vx_mesh_load_obj / vx_mesh_from_arrays)");
    for (int k = 0; k < nd; ++k) VX_TRY(need_device(devices[k]));
    vx_multi* m = new vx_multi();
    m->nd = nd;
    m->kind = kind;
    m->devices.assign(devices, devices + nd);
    m->meshes.assign((size_t)nd, nullptr);
    m->grids.assign((size_t)nd, nullptr);
    m->st.assign((size_t)nd, VX_OK);
    m->msg.assign((size_t)nd, std::string());
    const int prev_device = g_device;
    vx_status s = VX_OK;
    for (int k = 0; k < nd && s == VX_OK; ++k) {
        g_device = devices[k];
        s = vx_mesh_from_arrays(mesh->hv.data(), mesh->nv, mesh->hi.data(), mesh->nt, &m->meshes[(size_t)k]);
        if (s == VX_OK && !mesh->materials.empty())
            s = vx_mesh_set_materials(m->meshes[(size_t)k], mesh->materials.data(), mesh->materials.size(), mesh->tri_mat.empty() ? nullptr : mesh->tri_mat.data());
        if (s == VX_OK) s = mesh_to_device(m->meshes[(size_t)k]);
        if (s == VX_OK) {
            vx_grid* g = new vx_grid();
            g->kind = kind;
            g->device = devices[k];
            m->grids[(size_t)k] = g;
        }
    }
    g_device = prev_device;
    if (s != VX_OK) { const std::string e = g_err; vx_multi_free(m); return fail(s, e); }
    for (int k = 0; k < nd; ++k) m->threads.emplace_back(multi_worker, m, k);
    *out = m;
    return VX_OK;
}

vx_status vx_multi_voxelize(vx_multi* m, float vs, const vx_voxelize_opts* opts, int all_gather)
{
    if (!m) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(check_voxel_size(vs));
    vx_voxelize_opts o{};
    if (opts) o = *opts;
    if (o.word_begin || o.word_end || o.tri_begin || o.tri_end || o.shard_world) return fail(VX_ERR_INVALID_ARG, "vx_multi_voxelize shards the build itself");
    if (o.flags & VX_VOXELIZE_SOLID) return fail(VX_ERR_INVALID_ARG, "VX_VOXELIZE_SOLID needs the whole grid on one device: vx_multi_voxelize shards it");
    const bool want_mat = (o.flags & VX_VOXELIZE_MATERIALS) != 0;
    const int nd = m->nd;
    for (int k = 0; k < nd; ++k)
        if (!m->grids[(size_t)k]) return fail(VX_ERR_INVALID_ARG, "a grid of this context was handed to the caller (vx_multi_release_grid): create a new context");
    {   // ---- every rank builds its shard, side by side
        std::unique_lock<std::mutex> lk(m->mu);
        m->vs = vs;
        m->opts = o;
        m->remaining = nd;
        ++m->epoch;
        m->cv_go.notify_all();
        m->cv_done.wait(lk, [&] { return m->remaining == 0; });
    }
    for (int k = 0; k < nd; ++k)
        if (m->st[(size_t)k] != VX_OK) return fail(m->st[(size_t)k], m->msg[(size_t)k]);
    const uint64_t nwords = m->grids[0]->g.nwords;
    for (int k = 1; k < nd; ++k)
        if (m->grids[(size_t)k]->g.nwords != nwords) return fail(VX_ERR_HIP, "ranks disagree about the grid (different devices gave different bounding boxes?)");
    // ---- exchange: every destination pulls the other ranks' word ranges as peer copies (one slab per source device)
    const int ndst = all_gather ? nd : 1;
    hipError_t e = hipSuccess;
    for (int d = 0; d < ndst && e == hipSuccess; ++d) {
        vx_grid* gd = m->grids[(size_t)d];
        DeviceGuard dg(gd->device);
        for (int k = 0; k < nd && e == hipSuccess; ++k) {
            if (k == d) continue;
            vx_grid* gk = m->grids[(size_t)k];
            if (gk->device != gd->device) {  // direct xGMI copies instead of staging through the host
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, gd->device, gk->device) == hipSuccess && can) {
                    (void)hipDeviceEnablePeerAccess(gk->device, 0);
                    (void)hipGetLastError();  // (already enabled is not an error)
                }
            }
            uint64_t wb = 0, we = 0;
            vx_shard_words(nwords, k, nd, &wb, &we, nullptr);
            if (we <= wb) continue;
            e = hipMemcpyPeerAsync(gd->words.as<uint32_t>() + wb, gd->device, gk->words.as<uint32_t>() + wb, gk->device, (size_t)(we - wb) * 4, gd->stream);
        }
    }
    for (int d = 0; d < ndst && e == hipSuccess; ++d) {
        DeviceGuard dg(m->grids[(size_t)d]->device);
        e = hipStreamSynchronize(m->grids[(size_t)d]->stream);
    }
    if (e != hipSuccess) return fail(VX_ERR_HIP, std::string("peer exchange: ") + hipGetErrorString(e));
    // ---- materials: the index of a material is the order of its first use over ALL shards (vx_grid_finish_materials); the ids of the
    // voxels in ascending order are the shards' id arrays one after the other
    std::vector<uint64_t> shard_ids((size_t)nd, 0);
    if (want_mat) {
        const size_t nv = m->grids[0]->mat_first_use.size();
        std::vector<long long> fu(nv, -1);
        for (int k = 0; k < nd; ++k) {
            const std::vector<long long>& a = m->grids[(size_t)k]->mat_first_use;
            if (a.size() != nv) return fail(VX_ERR_HIP, "ranks disagree about the mesh's materials");
            for (size_t v = 0; v < nv; ++v)
                if (a[v] >= 0 && (fu[v] < 0 || a[v] < fu[v])) fu[v] = a[v];
        }
        for (int k = 0; k < nd; ++k) {
            VX_TRY(finish_materials(m->grids[(size_t)k], fu.data(), fu.size()));
            shard_ids[(size_t)k] = m->grids[(size_t)k]->mat_count;
        }
    }
    // ---- the complete masks: counts, word prefix and traversal structure; setVoxel calls of all shards add up
    uint64_t calls = 0, total_ids = 0;
    for (int k = 0; k < nd; ++k) {
        VX_TRY(sync_counts(m->grids[(size_t)k]));
        calls += m->grids[(size_t)k]->set_calls;
        total_ids += shard_ids[(size_t)k];
    }
    const uint64_t ntri_all = m->meshes[0]->nt;
    for (int d = 0; d < ndst; ++d) {
        vx_grid* gd = m->grids[(size_t)d];
        DeviceGuard dg(gd->device);
        if (want_mat && nd > 1) {
            // gather the shards' ids in shard order (a destination's own ids move to their place first: a copy within the device)
            DevBuf all{gd};
            VX_HIP(all.ensure((size_t)total_ids * 2 + 16));
            uint64_t off = 0;
            for (int k = 0; k < nd; ++k) {
                vx_grid* gk = m->grids[(size_t)k];
                if (shard_ids[(size_t)k]) {
                    if (gk->device == gd->device) VX_HIP(hipMemcpyAsync(all.as<int16_t>() + off, gk->matids.p, (size_t)shard_ids[(size_t)k] * 2, hipMemcpyDeviceToDevice, gd->stream));
                    else VX_HIP(hipMemcpyPeerAsync(all.as<int16_t>() + off, gd->device, gk->matids.p, gk->device, (size_t)shard_ids[(size_t)k] * 2, gd->stream));
                }
                off += shard_ids[(size_t)k];
            }
            VX_HIP(hipStreamSynchronize(gd->stream));
            gd->mattmp.release();   // (its first-half scratch is spent; every rank's own ids stay in its matids for the other destinations)
            gd->mattmp = std::move(all);  // (kept so that the next build finds a block of this size)
            gd->mat_gathered = true;
            gd->mat_gather_count = total_ids;
        }
        gd->set_calls = calls;
        gd->counts_valid = true;
        gd->triangles = ntri_all;
        VX_TRY(vx_grid_refresh(gd));
    }
    return VX_OK;
}

vx_grid* vx_multi_grid(vx_multi* m, int k) { return (m && k >= 0 && k < m->nd) ? m->grids[(size_t)k] : nullptr; }

vx_grid* vx_multi_release_grid(vx_multi* m, int k)
{
    if (!m || k < 0 || k >= m->nd) return nullptr;
    vx_grid* g = m->grids[(size_t)k];
    m->grids[(size_t)k] = nullptr;
    return g;
}

void vx_multi_free(vx_multi* m)
{
    if (!m) return;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->quit = true;
        m->cv_go.notify_all();
    }
    for (auto& t : m->threads) t.join();
    const int prev_device = g_device;
    for (int k = 0; k < m->nd; ++k) {
        if (m->grids[(size_t)k]) vx_grid_free(m->grids[(size_t)k]);
        if (m->meshes[(size_t)k]) vx_mesh_free(m->meshes[(size_t)k]);
    }
    g_device = prev_device;
    delete m;
}

// one-shot form: create the context, build once, hand the destination grids to the caller
vx_status vx_voxelize_multi(const vx_mesh* mesh, float vs, vx_grid_kind kind, int sat_variant, const int* devices, int nd, int all_gather, vx_grid** out)
{
    if (!out) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_multi* m = nullptr;
    VX_TRY(vx_multi_create(mesh, devices, nd, kind, &m));
    vx_voxelize_opts o{};
    o.sat_variant = sat_variant;
    const vx_status s = vx_multi_voxelize(m, vs, &o, all_gather);
    if (s != VX_OK) { const std::string e = g_err; vx_multi_free(m); return fail(s, e); }
    const int ndst = all_gather ? nd : 1;
    for (int d = 0; d < ndst; ++d) out[d] = vx_multi_release_grid(m, d);
    vx_multi_free(m);
    return VX_OK;
}

// ---- grid -----------------------------------------------------------------------------------------------------
vx_status vx_grid_create(vx_grid_kind kind, uint64_t x, uint64_t y, uint64_t z, float vs, const float origin[3], void* stream, vx_grid** out)
{
    if (!out) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (kind != VX_GRID_BOOL && kind != VX_GRID_AABBSTRUCT && kind != VX_GRID_VEC) return fail(VX_ERR_INVALID_ARG, "unknown grid kind");
    if (x > vx::kMaxDim || y > vx::kMaxDim || z > vx::kMaxDim || x * y * z > kMaxVoxels) return fail(VX_ERR_CAPACITY, "grid too large");
    VX_TRY(need_device(g_device));
    Fresh<vx_grid> g(new vx_grid());
    g->kind = kind;
    g->device = g_device;
    g->set_stream((hipStream_t)stream);
    const float zero[3] = {0.f, 0.f, 0.f};
    const uint64_t dim[3] = {x, y, z};
    fill_params(g->g, origin ? origin : zero, vs, dim);
    DeviceGuard dg(g->device);
    VX_TRY(init_grid_storage(g.get()));
    *out = g.release();
    return VX_OK;
}

vx_status vx_grid_describe(const vx_grid* gc, vx_grid_desc* d)
{
    if (!gc || !d) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_grid* g = const_cast<vx_grid*>(gc);
    VX_TRY(sync_counts(g));
    VX_TRY(ensure_occupied(g));
    std::memset(d, 0, sizeof(*d));
    for (int a = 0; a < 3; ++a) {
        d->dim[a] = g->g.dim[a];
        d->origin[a] = g->g.org[a];
        d->bbox_min[a] = g->bbmin[a];
        d->bbox_max[a] = g->bbmax[a];
        d->bbox_center[a] = g->bbc[a];
    }
    d->voxel_size = g->g.vs;
    d->num_words = g->g.nwords;
    d->set_calls = g->set_calls;
    d->occupied = g->occupied;
    d->triangles = g->triangles;
    d->kind = g->kind;
    d->device = g->device;
    return VX_OK;
}

vx_status vx_grid_set_voxel(vx_grid* g, uint64_t x, uint64_t y, uint64_t z)
{
    if (!g) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (x >= g->g.dim[0] || y >= g->g.dim[1] || z >= g->g.dim[2]) return fail(VX_ERR_OUT_OF_BOUNDS, "Index out of bounds");
    DeviceGuard dg(g->device);
    const uint64_t i = x + (uint64_t)g->g.dim[0] * (y + (uint64_t)g->g.dim[1] * z);
    VX_HIP(g->list_resolve());  // (a list emission still to come reads the mask / appends to the list this call changes)
    vx::launch_set_bit(g->words.as<uint32_t>(), i, g->stream);
    if (g->kind == VX_GRID_VEC) {
        // append {c - half, c + half} (voxelgridVecEncoding.cpp:27-36); the float recipe is shared with the kernels
        vx_aabb b;
        vx::cell_aabb(g->g, (uint32_t)x, (uint32_t)y, (uint32_t)z, b.minimum);
        const size_t need = (size_t)(g->vec_count + 1) * sizeof(vx_aabb);
        if (g->vec_in_bound) {  // the list lives in the caller's buffer: appending continues in the grid's own storage
            VX_HIP(g->vec.ensure(need * 2));
            if (g->vec_count) VX_HIP(hipMemcpyAsync(g->vec.p, g->bound, (size_t)g->vec_count * sizeof(vx_aabb), hipMemcpyDeviceToDevice, g->stream));
            g->vec_in_bound = false;
        }
        if (need > g->vec.cap) {
            DevBuf nb{g};
            VX_HIP(nb.ensure(need * 2));
            if (g->vec_count) VX_HIP(hipMemcpyAsync(nb.p, g->vec.p, (size_t)g->vec_count * sizeof(vx_aabb), hipMemcpyDeviceToDevice, g->stream));
            VX_HIP(hipStreamSynchronize(g->stream));
            g->vec.release();
            g->vec = std::move(nb);
        }
        VX_HIP(hipMemcpyAsync(g->vec.as<vx_aabb>() + g->vec_count, &b, sizeof(b), hipMemcpyHostToDevice, g->stream));
        VX_HIP(hipStreamSynchronize(g->stream));
        g->vec_count++;
    }
    g->host_set_calls++;
    g->set_calls++;
    g->coarse_valid = g->prefix_valid = g->p16_valid = g->occupied_known = false;
    g->has_materials = false;  // ids are per box of the list: a host-side setVoxel (default material, not recorded) invalidates them
    return VX_OK;
}

vx_status vx_grid_test_voxel(const vx_grid* g, uint64_t x, uint64_t y, uint64_t z, int* occ)
{
    if (!g || !occ) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (x >= g->g.dim[0] || y >= g->g.dim[1] || z >= g->g.dim[2]) return fail(VX_ERR_OUT_OF_BOUNDS, "Index out of bounds");
    DeviceGuard dg(g->device);
    const uint64_t i = x + (uint64_t)g->g.dim[0] * (y + (uint64_t)g->g.dim[1] * z);
    uint32_t w = 0;
    VX_HIP(hipMemcpyAsync(&w, g->words.as<uint32_t>() + (i >> 5), 4, hipMemcpyDeviceToHost, g->stream));
    VX_HIP(hipStreamSynchronize(g->stream));
    *occ = (int)((w >> (i & 31)) & 1u);
    return VX_OK;
}

vx_status vx_grid_coords(const vx_grid* g, uint64_t x, uint64_t y, uint64_t z, float out[3])
{
    if (!g || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (x >= g->g.dim[0] || y >= g->g.dim[1] || z >= g->g.dim[2]) return fail(VX_ERR_OUT_OF_BOUNDS, "Index out of bounds");  // voxelgrid.hpp:93-95
    out[0] = vx::cell_centre(g->g.org[0], g->g.vs, (uint32_t)x);
    out[1] = vx::cell_centre(g->g.org[1], g->g.vs, (uint32_t)y);
    out[2] = vx::cell_centre(g->g.org[2], g->g.vs, (uint32_t)z);
    return VX_OK;
}

uint64_t vx_grid_bytes(const vx_grid* gc)
{
    if (!gc) return 0;
    vx_grid* g = const_cast<vx_grid*>(gc);
    switch (g->kind) {
        case VX_GRID_BOOL: return g->g.nwords * 4;     // m_voxel.size() * sizeof(unsigned)
        case VX_GRID_AABBSTRUCT: return g->g.nvox * 28;  // sizeof(AabbInternal) == 28
        case VX_GRID_VEC: return g->vec_count * 24;      // one Aabb per setVoxel call
    }
    return 0;
}

vx_status vx_grid_bitmask(const vx_grid* g, uint32_t* host_words, uint64_t cap)
{
    if (!g || (!host_words && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (cap < g->g.nwords) return fail(VX_ERR_CAPACITY, "bitmask buffer too small");
    DeviceGuard dg(g->device);
    if (g->g.nwords) VX_HIP(hipMemcpyAsync(host_words, g->words.p, (size_t)g->g.nwords * 4, hipMemcpyDeviceToHost, g->stream));
    VX_HIP(hipStreamSynchronize(g->stream));
    return VX_OK;
}

const uint32_t* vx_grid_bitmask_device(const vx_grid* g) { return g ? g->words.as<uint32_t>() : nullptr; }
uint32_t* vx_grid_bitmask_device_mut(vx_grid* g)
{
    if (!g) return nullptr;
    { DeviceGuard dg(g->device); (void)g->list_resolve(); }  // (an emission still to come reads the mask the caller is about to write)
    g->coarse_valid = g->prefix_valid = g->p16_valid = g->occupied_known = false;
    return g->words.as<uint32_t>();
}
vx_status vx_grid_refresh(vx_grid* g)
{
    if (!g) return fail(VX_ERR_INVALID_ARG, "null argument");
    {
        DeviceGuard dg(g->device);
        VX_HIP(g->list_resolve());
        if (g->g.nwords) vx::launch_mask_tail(g->words.as<uint32_t>(), g->g.nvox, g->stream);  // (padding bits are not cells)
    }
    g->coarse_valid = g->prefix_valid = g->p16_valid = g->occupied_known = false;
    VX_TRY(ensure_prefix(g));
    return ensure_coarse(g);
}

vx_status vx_grid_fill_interior(vx_grid* g)
{
    if (!g) return fail(VX_ERR_INVALID_ARG, "null argument");
    DeviceGuard dg(g->device);
    VX_HIP(g->list_resolve());  // (an emission still to come reads the mask / writes the list this call extends)
    if (!g->mail) VX_HIP(mail_alloc(g->mail));
    VX_HIP(ensure_small(g->small));
    uint64_t n = 0;
    const uint32_t* h = nullptr;
    const vx_status st = solid_fill(g, &n, &h);
    g->coarse_valid = g->prefix_valid = g->p16_valid = g->occupied_known = false;  // (the mask may have changed even when the fill failed)
    VX_TRY(st);
    if (g->kind == VX_GRID_VEC && n) {
        // setVoxel appends one record per call: the list continues in the grid's own storage, as after vx_grid_set_voxel
        const size_t need = (size_t)(g->vec_count + n + 1) * sizeof(vx_aabb);
        if (g->vec_in_bound || need > g->vec.cap) {
            DevBuf nb{g};
            VX_HIP(nb.ensure(need));
            if (g->vec_count) VX_HIP(hipMemcpyAsync(nb.p, g->vec_ptr(), (size_t)g->vec_count * sizeof(vx_aabb), hipMemcpyDeviceToDevice, g->stream));
            g->vec.release();
            g->vec = std::move(nb);
            g->vec_in_bound = false;
        }
        vx::launch_emit_bool_aabbs(h, g->solid_pre.as<uint32_t>(), g->g, g->vec.as<vx_aabb>() + g->vec_count, n, g->stream);
        g->vec_count += n;
    }
    g->host_set_calls += n;
    g->set_calls += n;
    g->interior = n;
    if (n) g->has_materials = false;  // (setVoxel from the host drops the per-voxel ids)
    VX_TRY(ensure_prefix(g));
    VX_TRY(ensure_coarse(g));
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_grid_interior(const vx_grid* g, uint64_t* count)
{
    if (!g || !count) return fail(VX_ERR_INVALID_ARG, "null argument");
    *count = g->interior;
    return VX_OK;
}

uint32_t vx_grid_fill_rounds(const vx_grid* g) { return g ? g->solid_rounds : 0; }

// Distance fields: the argument checks in the order the header lists them, then the three passes on the grid's stream (vx_distance.hip).
// Nothing the grid's readers see is touched: the passes only read the bitmask, and a pending list emission (which reads it too) stays pending.
static vx_status distance_check(const vx_grid* g, uint64_t cap, uint64_t* n)
{
    *n = 0;
    if (!g->g.nvox) return VX_OK;  // (a grid of 0 cells: nothing to write)
    const uint64_t d0 = g->g.dim[0] - 1ull, d1 = g->g.dim[1] - 1ull, d2 = g->g.dim[2] - 1ull;
    if (d0 * d0 + d1 * d1 + d2 * d2 > 0xFFFFFFFEull) return fail(VX_ERR_CAPACITY, "distance fields need (X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 0xFFFFFFFE");
    if (cap < g->g.nvox) return fail(VX_ERR_CAPACITY, "distance field buffer too small");
    *n = g->g.nvox;
    return VX_OK;
}

static vx_status distance_queue(vx_grid* g, int mode, void* dev_out)
{
    VX_HIP(g->dist_stk.ensure((size_t)vx::distance_stack_entries(g->g.dim, mode == 2) * 8));
    vx::launch_distance(g->words.as<uint32_t>(), g->g.dim, mode, g->g.vs, static_cast<uint32_t*>(dev_out), g->dist_stk.as<uint2>(), g->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// The ten field entry points (distance_sq / sdf / nearest / nearest_gather / morph, each with its _device variant) in one order: null checks;
// check(&bytes), the feature's own checks in the header's order -> the bytes the call writes (0: a grid of 0 cells, nothing to do); the
// guard; queue(g, in, out) on the caller's device pointers, or (host) on a Staging over blocks the grid keeps: `in` through near_val, the
// result through g->*stage (`spare` bytes behind it).
extern "C++" {
template <class Check, class Queue>
static vx_status field_entry(const vx_grid* gc, const void* in, bool needs_in, void* out, bool host, DevBuf vx_grid::*stage, size_t spare, Check check,
                             Queue queue)
{
    if (!gc || !out || (needs_in && !in)) return fail(VX_ERR_INVALID_ARG, "null argument");
    size_t bytes = 0;
    VX_TRY(check(&bytes));
    if (!bytes) return VX_OK;
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    if (!host) return queue(g, in, out);
    Staging s(*g);
    out = s.out(out, bytes, spare, &(g->*stage));
    in = s.in(in, bytes, &g->near_val);
    VX_TRY(s.status());
    VX_TRY(queue(g, in, out));
    return s.finish();
}
}  // extern "C++"

// mode: 0 distance_sq, 1 distance_sq inside, 2 sdf
static vx_status distance_entry(const vx_grid* gc, uint32_t flags, int mode, void* out, uint64_t capacity, bool host)
{
    return field_entry(gc, nullptr, false, out, host, &vx_grid::dist_out, 0,
        [&](size_t* bytes) {
            if (flags & ~(uint32_t)VX_DISTANCE_INSIDE) return fail(VX_ERR_INVALID_ARG, "unknown distance flags");
            uint64_t n = 0;
            const vx_status st = distance_check(gc, capacity, &n);
            *bytes = (size_t)n * 4;
            return st;
        },
        [&](vx_grid* g, const void*, void* dev_out) { return distance_queue(g, mode, dev_out); });
}

vx_status vx_grid_distance_sq_device(const vx_grid* g, uint32_t flags, uint32_t* dev_out, uint64_t capacity)
{
    return distance_entry(g, flags, (flags & VX_DISTANCE_INSIDE) ? 1 : 0, dev_out, capacity, false);
}

vx_status vx_grid_distance_sq(const vx_grid* g, uint32_t flags, uint32_t* host_out, uint64_t capacity)
{
    return distance_entry(g, flags, (flags & VX_DISTANCE_INSIDE) ? 1 : 0, host_out, capacity, true);
}

vx_status vx_grid_sdf_device(const vx_grid* g, float* dev_out, uint64_t capacity) { return distance_entry(g, 0u, 2, dev_out, capacity, false); }
vx_status vx_grid_sdf(const vx_grid* g, float* host_out, uint64_t capacity) { return distance_entry(g, 0u, 2, host_out, capacity, true); }

// The feature transform (vx_grid_nearest*): the checks in the order the header lists them, then the three passes of launch_nearest.  The
// stacks and the host variants' result share the distance fields' buffers (one stream: the calls are ordered).
static vx_status nearest_check(const vx_grid* g, uint32_t flags, const uint32_t* values, uint64_t nvalues, bool gather, const uint32_t* out,
                               uint64_t cap, uint64_t* n)
{
    *n = 0;
    if (flags & ~(uint32_t)VX_DISTANCE_INSIDE) return fail(VX_ERR_INVALID_ARG, "unknown nearest flags");
    if (gather && nvalues < g->g.nvox) return fail(VX_ERR_INVALID_ARG, "nearest gather: fewer values than cells");
    if (gather && values == out) return fail(VX_ERR_INVALID_ARG, "nearest gather: values and out must differ");
    if (!g->g.nvox) return VX_OK;  // (a grid of 0 cells: nothing to write)
    if (cap < g->g.nvox) return fail(VX_ERR_CAPACITY, "nearest buffer too small");
    const uint64_t d0 = g->g.dim[0] - 1ull, d1 = g->g.dim[1] - 1ull, d2 = g->g.dim[2] - 1ull;
    if (d0 * d0 + d1 * d1 + d2 * d2 > 0xFFFFFFFEull) return fail(VX_ERR_CAPACITY, "nearest needs (X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 0xFFFFFFFE");
    if (g->g.nvox > 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, "nearest needs at most 0xFFFFFFFF cells");
    *n = g->g.nvox;
    return VX_OK;
}

static vx_status nearest_queue(vx_grid* g, uint32_t flags, const uint32_t* dev_values, uint32_t fill, uint32_t* dev_out)
{
    VX_HIP(g->dist_stk.ensure((size_t)vx::distance_stack_entries(g->g.dim, false) * 8));
    vx::launch_nearest(g->words.as<uint32_t>(), g->g.dim, (flags & VX_DISTANCE_INSIDE) != 0, dev_values, fill, dev_out, g->dist_stk.as<uint2>(),
                       g->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// gather: `values` (one per cell) are what the result holds; otherwise the nearest cell's index
static vx_status nearest_entry(const vx_grid* gc, uint32_t flags, bool gather, const uint32_t* values, uint64_t nvalues, uint32_t fill, uint32_t* out,
                               uint64_t capacity, bool host)
{
    return field_entry(gc, values, gather, out, host, &vx_grid::dist_out, 0,
        [&](size_t* bytes) {
            uint64_t n = 0;
            const vx_status st = nearest_check(gc, flags, values, nvalues, gather, out, capacity, &n);
            *bytes = (size_t)n * 4;
            return st;
        },
        [&](vx_grid* g, const void* dev_values, void* dev_out) {
            return nearest_queue(g, flags, static_cast<const uint32_t*>(dev_values), fill, static_cast<uint32_t*>(dev_out));
        });
}

vx_status vx_grid_nearest_device(const vx_grid* g, uint32_t flags, uint32_t* dev_out, uint64_t capacity)
{
    return nearest_entry(g, flags, false, nullptr, 0, 0u, dev_out, capacity, false);
}

vx_status vx_grid_nearest(const vx_grid* g, uint32_t flags, uint32_t* host_out, uint64_t capacity)
{
    return nearest_entry(g, flags, false, nullptr, 0, 0u, host_out, capacity, true);
}

vx_status vx_grid_nearest_gather_device(const vx_grid* g, uint32_t flags, const uint32_t* dev_values, uint64_t nvalues, uint32_t fill,
                                        uint32_t* dev_out, uint64_t capacity)
{
    return nearest_entry(g, flags, true, dev_values, nvalues, fill, dev_out, capacity, false);
}

vx_status vx_grid_nearest_gather(const vx_grid* g, uint32_t flags, const uint32_t* host_values, uint64_t nvalues, uint32_t fill,
                                 uint32_t* host_out, uint64_t capacity)
{
    return nearest_entry(g, flags, true, host_values, nvalues, fill, host_out, capacity, true);
}

// Morphology (vx_morph.hip).  Every operation is a chain of stages on the grid's stream; the scratch of all of them lives on the handle
// whose mask is read.  Bit path (R <= vx_morph_bit_radius()): k_morph_ball stages, row-aligned in between, packed at the end.  Distance-field
// path: launch_distance on a mask in the reference's layout (padded physically where the operation pads), thresholded into a mask again.
constexpr uint32_t kMorphSeal = 4u;  // (internal: vx_grid_seal's plan)

struct MorphPlan {
    uint32_t R = 0, pad = 0;
    bool bit = true;
    uint32_t wdim[3] = {0, 0, 0};  // the working domain: the grid, padded for CLOSE (R) and seal (R + 1)
};

static uint32_t morph_isqrt(uint32_t v)
{
    uint32_t r = (uint32_t)std::sqrt((double)v);
    while ((uint64_t)r * r > v) --r;
    while ((uint64_t)(r + 1) * (r + 1) <= v) ++r;
    return r;
}

static vx_status morph_plan(const vx_grid* g, uint32_t op, uint32_t r2, MorphPlan* p)
{
    p->R = morph_isqrt(r2);
    p->bit = p->R <= vx::kMorphBitRadius;
    p->pad = op == VX_MORPH_CLOSE ? p->R : (op == kMorphSeal ? p->R + 1u : 0u);
    uint64_t cells = 1, dsq = 0;
    for (int a = 0; a < 3; ++a) {
        const uint64_t d = (uint64_t)g->g.dim[a] + 2ull * p->pad;
        if (d > vx::kMaxDim) return fail(VX_ERR_CAPACITY, "morphology: the working domain exceeds 2^21 cells on an axis");
        p->wdim[a] = (uint32_t)d;
        cells *= d;
        dsq += (d - 1) * (d - 1);
    }
    if (cells > kMaxVoxels) return fail(VX_ERR_CAPACITY, "morphology: the working domain exceeds 2^37 cells");
    if (!p->bit && dsq > 0xFFFFFFFEull) return fail(VX_ERR_CAPACITY, "morphology: the distance-field path needs (X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 0xFFFFFFFE");
    return VX_OK;
}

static vx::MorphDom morph_dom(const uint32_t d[3], bool aligned)
{
    vx::MorphDom m;
    for (int a = 0; a < 3; ++a) m.dim[a] = d[a];
    m.stride = aligned ? 32ull * ((d[0] + 31u) / 32u) : d[0];
    return m;
}

static uint64_t morph_words(const uint32_t d[3]) { return ((uint64_t)d[0] * d[1] * d[2] + 31u) / 32u; }

// one ball stage whose result is wanted in the reference's layout (odim cells, in dst): straight into dst where the two layouts coincide and
// nothing is OR-ed in, through `stage` and the pack kernel otherwise
static vx_status morph_ball_ref(vx_grid* sc, DevBuf& stage, const uint32_t* src, const vx::MorphDom& in, const uint32_t odim[3], int32_t shift, uint32_t r2,
                                uint32_t flags, const uint32_t* orw, uint32_t* dst)
{
    if (odim[0] % 32u == 0u && !orw) {
        vx::launch_morph_ball(src, in, dst, odim, shift, r2, flags, sc->stream);
        return VX_OK;
    }
    VX_HIP(stage.ensure((size_t)vx::morph_aligned_words(odim) * 4 + 16));
    vx::launch_morph_ball(src, in, stage.as<uint32_t>(), odim, shift, r2, flags, sc->stream);
    vx::launch_morph_pack(stage.as<uint32_t>(), odim, orw, dst, sc->stream);
    return VX_OK;
}

// the squared distance field (mode 0: to the occupied cells, 1: to the empty ones) of a mask in the reference's layout -- two spare words
// behind it, as the grid's own has -- into sc->morph_d
static vx_status morph_field(vx_grid* sc, const uint32_t* mask, const uint32_t d[3], int mode)
{
    VX_HIP(sc->morph_d.ensure((size_t)d[0] * d[1] * d[2] * 4 + 16));
    VX_HIP(sc->dist_stk.ensure((size_t)vx::distance_stack_entries(d, false) * 8));
    vx::launch_distance(mask, d, mode, 1.0f, sc->morph_d.as<uint32_t>(), sc->dist_stk.as<uint2>(), sc->stream);
    return VX_OK;
}

// op 0..3 of the mask src (the reference's layout, dim cells, two spare words behind it) into dst (the same layout); scratch and stream: sc
static vx_status morph_run(vx_grid* sc, const uint32_t* src, const uint32_t dim[3], uint32_t op, uint32_t r2, const MorphPlan& p, uint32_t* dst)
{
    hipStream_t s = sc->stream;
    const vx::MorphDom gd = morph_dom(dim, false);
    const uint32_t both = vx::kMorphInvIn | vx::kMorphInvOut;
    const int32_t R = (int32_t)p.R;
    if (p.bit) {
        switch (op) {
        case VX_MORPH_DILATE: return morph_ball_ref(sc, sc->morph_b, src, gd, dim, 0, r2, 0u, nullptr, dst);
        case VX_MORPH_ERODE: return morph_ball_ref(sc, sc->morph_b, src, gd, dim, 0, r2, both, nullptr, dst);
        case VX_MORPH_OPEN:
            VX_HIP(sc->morph_a.ensure((size_t)vx::morph_aligned_words(dim) * 4 + 16));
            vx::launch_morph_ball(src, gd, sc->morph_a.as<uint32_t>(), dim, 0, r2, both, s);
            return morph_ball_ref(sc, sc->morph_b, sc->morph_a.as<uint32_t>(), morph_dom(dim, true), dim, 0, r2, 0u, nullptr, dst);
        default:  // CLOSE: dilate into the padded domain, erode back out of it
            VX_HIP(sc->morph_a.ensure((size_t)vx::morph_aligned_words(p.wdim) * 4 + 16));
            vx::launch_morph_ball(src, gd, sc->morph_a.as<uint32_t>(), p.wdim, -R, r2, 0u, s);
            return morph_ball_ref(sc, sc->morph_b, sc->morph_a.as<uint32_t>(), morph_dom(p.wdim, true), dim, R, r2, both, nullptr, dst);
        }
    }
    switch (op) {
    case VX_MORPH_DILATE:
        VX_TRY(morph_field(sc, src, dim, 0));
        vx::launch_morph_thresh(sc->morph_d.as<uint32_t>(), dim, r2, false, dst, s);
        return VX_OK;
    case VX_MORPH_ERODE:
        VX_TRY(morph_field(sc, src, dim, 1));
        vx::launch_morph_thresh(sc->morph_d.as<uint32_t>(), dim, r2, true, dst, s);
        return VX_OK;
    case VX_MORPH_OPEN: {
        VX_HIP(sc->morph_p.ensure((size_t)(morph_words(dim) + 2) * 4));
        uint32_t* e = sc->morph_p.as<uint32_t>();
        VX_TRY(morph_field(sc, src, dim, 1));
        vx::launch_morph_thresh(sc->morph_d.as<uint32_t>(), dim, r2, true, e, s);
        VX_TRY(morph_field(sc, e, dim, 0));
        vx::launch_morph_thresh(sc->morph_d.as<uint32_t>(), dim, r2, false, dst, s);
        return VX_OK;
    }
    default: {  // CLOSE on a physically padded copy; every stage is complete on the stream before the next overwrites what it read
        VX_HIP(sc->morph_p.ensure((size_t)(morph_words(p.wdim) + 2) * 4));
        uint32_t* pm = sc->morph_p.as<uint32_t>();
        VX_TRY(morph_ball_ref(sc, sc->morph_a, src, gd, p.wdim, -R, 0u, 0u, nullptr, pm));
        VX_TRY(morph_field(sc, pm, p.wdim, 0));
        vx::launch_morph_thresh(sc->morph_d.as<uint32_t>(), p.wdim, r2, false, pm, s);
        VX_TRY(morph_field(sc, pm, p.wdim, 1));
        vx::launch_morph_thresh(sc->morph_d.as<uint32_t>(), p.wdim, r2, true, pm, s);
        return morph_ball_ref(sc, sc->morph_a, pm, morph_dom(p.wdim, false), dim, R, 0u, 0u, nullptr, dst);
    }
    }
}

// a new grid like src (kind, cells, voxel size, origin, device, stream) with an all-zero mask
static vx_status morph_new_grid(const vx_grid* src, int kind, const uint32_t dim[3], vx_grid** out)
{
    VX_TRY(need_device(src->device));
    Fresh<vx_grid> g(new vx_grid());
    g->kind = kind;
    g->device = src->device;
    g->set_stream(src->stream);
    const uint64_t d[3] = {dim[0], dim[1], dim[2]};
    fill_params(g->g, src->g.org, src->g.vs, d);
    DeviceGuard dg(g->device);
    VX_TRY(init_grid_storage(g.get()));
    *out = g.release();
    return VX_OK;
}

// seal(M, r2) = M | crop(erode(fill(dilate(pad(M, R + 1))))) into dst; the fill runs on an internal grid handle of the padded domain
static vx_status morph_seal_run(vx_grid* g, uint32_t r2, const MorphPlan& p, uint32_t* dst)
{
    vx_grid* t = nullptr;
    VX_TRY(morph_new_grid(g, VX_GRID_BOOL, p.wdim, &t));
    hipStream_t s = g->stream;
    const uint32_t* dim = g->g.dim;
    const vx::MorphDom gd = morph_dom(dim, false), pd = morph_dom(p.wdim, false);
    const uint32_t both = vx::kMorphInvIn | vx::kMorphInvOut;
    const int32_t P = (int32_t)p.pad;
    uint32_t* tw = t->words.as<uint32_t>();
    vx_status st = VX_OK;
    auto run = [&]() -> vx_status {
        if (p.bit) {
            VX_TRY(morph_ball_ref(g, g->morph_a, g->words.as<uint32_t>(), gd, p.wdim, -P, r2, 0u, nullptr, tw));
        } else {
            VX_TRY(morph_ball_ref(g, g->morph_a, g->words.as<uint32_t>(), gd, p.wdim, -P, 0u, 0u, nullptr, tw));
            VX_TRY(morph_field(g, tw, p.wdim, 0));
            vx::launch_morph_thresh(g->morph_d.as<uint32_t>(), p.wdim, r2, false, tw, s);
        }
        uint64_t n = 0;
        const uint32_t* h = nullptr;
        VX_TRY(solid_fill(t, &n, &h));
        if (p.bit) return morph_ball_ref(g, g->morph_a, tw, pd, dim, P, r2, both, g->words.as<uint32_t>(), dst);
        VX_TRY(morph_field(g, tw, p.wdim, 1));
        vx::launch_morph_thresh(g->morph_d.as<uint32_t>(), p.wdim, r2, true, tw, s);
        return morph_ball_ref(g, g->morph_a, tw, pd, dim, P, 0u, 0u, g->words.as<uint32_t>(), dst);
    };
    st = run();
    const std::string e = g_err;
    vx_grid_free(t);  // (waits for the stream: everything that read the padded mask is done)
    return st == VX_OK ? VX_OK : fail(st, e);
}

static vx_status morph_args(const vx_grid* g, uint32_t op, uint32_t r2, const void* buf)
{
    if (!g || !buf) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (op > VX_MORPH_CLOSE) return fail(VX_ERR_INVALID_ARG, "unknown morphology operation");
    if (r2 == 0xFFFFFFFFu) return fail(VX_ERR_INVALID_ARG, "radius_sq 0xFFFFFFFF is the distance fields' sentinel");
    return VX_OK;
}

// vx_grid_morph_device / vx_grid_morph_mask; only the device variant's output can overlap the grid's own mask
static vx_status morph_entry(const vx_grid* gc, uint32_t op, uint32_t r2, uint32_t* words, uint64_t capacity_words, bool host)
{
    MorphPlan p;
    return field_entry(gc, nullptr, false, words, host, &vx_grid::morph_out, 8,
        [&](size_t* bytes) {
            VX_TRY(morph_args(gc, op, r2, words));
            const uintptr_t a = (uintptr_t)words, b = (uintptr_t)gc->words.p, n = (uintptr_t)gc->g.nwords * 4u;
            if (!host && n && a < b + n && b < a + n) return fail(VX_ERR_INVALID_ARG, "the output overlaps the grid's own bitmask");
            if (!gc->g.nvox) return VX_OK;
            VX_TRY(morph_plan(gc, op, r2, &p));
            if (capacity_words < gc->g.nwords) return fail(VX_ERR_CAPACITY, "morphology: mask buffer too small");
            *bytes = (size_t)gc->g.nwords * 4;
            return VX_OK;
        },
        [&](vx_grid* g, const void*, void* dev_words) {
            VX_TRY(morph_run(g, g->words.as<uint32_t>(), g->g.dim, op, r2, p, static_cast<uint32_t*>(dev_words)));
            VX_HIP(hipGetLastError());
            return VX_OK;
        });
}

vx_status vx_grid_morph_device(const vx_grid* g, uint32_t op, uint32_t radius_sq, uint32_t* dev_words, uint64_t capacity_words)
{
    return morph_entry(g, op, radius_sq, dev_words, capacity_words, false);
}

vx_status vx_grid_morph_mask(const vx_grid* g, uint32_t op, uint32_t radius_sq, uint32_t* host_words, uint64_t capacity_words)
{
    return morph_entry(g, op, radius_sq, host_words, capacity_words, true);
}

// the result grid's counts, list and derived data from its mask: as if vx_grid_set_voxel had run on every cell in ascending index
static vx_status morph_finish_grid(vx_grid* out, const vx_grid* src)
{
    for (int a = 0; a < 3; ++a) { out->bbmin[a] = src->bbmin[a]; out->bbmax[a] = src->bbmax[a]; out->bbc[a] = src->bbc[a]; }
    out->triangles = 0;
    out->coarse_valid = out->prefix_valid = out->p16_valid = out->occupied_known = false;
    if (!out->g.nvox) { out->occupied_known = true; return VX_OK; }
    VX_TRY(ensure_prefix(out));
    out->host_set_calls = out->set_calls = out->occupied;
    out->counts_valid = true;
    if (out->kind == VX_GRID_VEC && out->occupied) {
        VX_HIP(out->vec.ensure((size_t)(out->occupied + 1) * sizeof(vx_aabb)));
        vx::launch_emit_bool_aabbs(out->words.as<uint32_t>(), out->wprefix.as<uint32_t>(), out->g, out->vec.as<vx_aabb>(), out->occupied, out->stream,
                                   out->sel_valid ? out->wsel.as<uint32_t>() : nullptr);
        out->vec_count = out->occupied;
    }
    VX_TRY(ensure_coarse(out));
    VX_HIP(hipGetLastError());
    return VX_OK;
}

static vx_status morph_grid(const vx_grid* src_c, uint32_t op, uint32_t r2, vx_grid** out)
{
    vx_grid* src = const_cast<vx_grid*>(src_c);
    MorphPlan p;
    if (src->g.nvox) VX_TRY(morph_plan(src, op, r2, &p));
    vx_grid* g = nullptr;
    VX_TRY(morph_new_grid(src, src->kind, src->g.dim, &g));
    DeviceGuard dg(src->device);
    vx_status st = VX_OK;
    uint64_t before = 0;
    if (src->g.nvox) {
        if (op == kMorphSeal) {
            st = ensure_occupied(src);
            before = src->occupied;
            if (st == VX_OK) st = morph_seal_run(src, r2, p, g->words.as<uint32_t>());
        } else {
            st = morph_run(src, src->words.as<uint32_t>(), src->g.dim, op, r2, p, g->words.as<uint32_t>());
        }
    }
    if (st == VX_OK) st = morph_finish_grid(g, src);
    if (st != VX_OK) { const std::string e = g_err; vx_grid_free(g); return fail(st, e); }
    if (op == kMorphSeal) g->interior = g->occupied - before;
    *out = g;
    return VX_OK;
}

vx_status vx_grid_morph(const vx_grid* src, uint32_t op, uint32_t radius_sq, vx_grid** out)
{
    VX_TRY(morph_args(src, op, radius_sq, out));
    return morph_grid(src, op, radius_sq, out);
}

vx_status vx_grid_seal(const vx_grid* src, uint32_t radius_sq, vx_grid** out)
{
    VX_TRY(morph_args(src, VX_MORPH_DILATE, radius_sq, out));
    return morph_grid(src, kMorphSeal, radius_sq, out);
}

uint32_t vx_morph_bit_radius(void) { return vx::kMorphBitRadius; }

// Surface mesh: the argument checks in the header's order, the counting pass and both scans on the grid's stream, one host wait for the
// totals, then the emission (vx_surface.hip).  The passes only read the bitmask (and, with materials, the word prefix and the ids); a
// pending list emission stays pending.
static vx_status surface_materials(const vx_grid* g, const int16_t** ids)
{
    if (g->kind == VX_GRID_VEC) return fail(VX_ERR_UNSUPPORTED, "surface materials: a Vec grid's cell may carry several records");
    if (!g->has_materials) return fail(VX_ERR_INVALID_ARG, "surface materials: the grid was not built with VX_VOXELIZE_MATERIALS");
    *ids = vx_grid_material_ids_device(g);
    return VX_OK;
}

// counts -> *nv / *nt; the emission's inputs stay in the handle's scratch.  *mat_ids: the per-cell ids when want_mat (word prefix queued).
static vx_status surface_count(vx_grid* g, bool want_mat, uint64_t* nv, uint64_t* nt, const int16_t** mat_ids)
{
    *nv = *nt = 0;
    const int16_t* ids = nullptr;
    if (want_mat) VX_TRY(surface_materials(g, &ids));
    *mat_ids = ids;
    if (!g->g.nvox) return VX_OK;
    const vx::SurfacePlan p = vx::surface_plan(g->g);
    const uint64_t nmax = g->g.nwords > p.nlw ? g->g.nwords : p.nlw;
    VX_HIP(g->surf_cnt.ensure((size_t)(g->g.nwords + 4) * 4));
    VX_HIP(g->surf_tpre.ensure((size_t)(g->g.nwords + 4) * 4));
    VX_HIP(g->surf_cm.ensure((size_t)(p.nlw + 4) * 4));
    VX_HIP(g->surf_vpre.ensure((size_t)(p.nlw + 4) * 4));
    VX_HIP(g->up.scantmp.reserve(nmax, g->stream));  // (one scratch block for both scans, sized ahead of the count kernel)
    bool pending = false;
    if (want_mat) VX_TRY(prefix_launch(g, &pending));
    vx::launch_surface_count(g->words.as<uint32_t>(), g->g, p, g->surf_cnt.as<uint32_t>(), g->surf_cm.as<uint32_t>(), g->stream);
    VX_TRY(g->up.scantmp.u32(g->surf_cnt, g->surf_tpre, g->g.nwords, false, &g->mail->surf_tris, g->stream));
    VX_TRY(g->up.scantmp.u32(g->surf_cm, g->surf_vpre, p.nlw, true, &g->mail->surf_verts, g->stream));
    VX_HIP(hipGetLastError());
    // (one wait for both totals; beyond 2^32 - 1 they are refused as surface_check refuses them)
    const char* limit = "surface mesh above 2^31 - 1 vertices or triangles (int32 indices)";
    uint64_t tris = 0, verts = 0;
    VX_TRY(mail_total(&g->mail->surf_tris, 0, g->stream, limit, &tris));
    VX_TRY(mail_value(&g->mail->surf_verts, limit, &verts));
    VX_TRY(prefix_finish(g, pending));
    if (want_mat && g->occupied > (g->mat_gathered ? g->mat_gather_count : g->mat_count))
        return fail(VX_ERR_INVALID_ARG, "surface materials: the grid's material ids do not cover its occupied cells");
    *nt = tris;
    *nv = verts;
    return VX_OK;
}

static vx_status surface_check(uint64_t nv, uint64_t nt, uint64_t vcap, uint64_t tcap)
{
    if (nv > 0x7FFFFFFFull || nt > 0x7FFFFFFFull) return fail(VX_ERR_CAPACITY, "surface mesh above 2^31 - 1 vertices or triangles (int32 indices)");
    if (!vcap && !tcap) return VX_OK;  // (size query)
    if (vcap < nv || tcap < nt) return fail(VX_ERR_CAPACITY, "surface mesh buffer too small");
    return VX_OK;
}

// Surface nets (sp != null): vx_grid_surface's count, scans, wait and triangles; the positions from the relaxation instead of k_surf_verts,
// and optionally the vertex normals (vx_surface.hip).  Everything after the wait for V and T is queued back to back.
static vx_status smooth_params(const vx_smooth* sp)
{
    if (!sp) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (sp->iterations > 1024u) return fail(VX_ERR_INVALID_ARG, "vx_smooth: iterations above 1024");
    if (!(sp->lambda >= 0.0f && sp->lambda <= 1.0f)) return fail(VX_ERR_INVALID_ARG, "vx_smooth: lambda must be finite in [0, 1]");
    if (!(sp->mu >= -1.0f && sp->mu <= 0.0f)) return fail(VX_ERR_INVALID_ARG, "vx_smooth: mu must be finite in [-1, 0]");
    return VX_OK;
}

// sp null: the faces' mesh (normals null).  sp non-null: the surface nets, sp already through smooth_params.
static vx_status surface_run(vx_grid* g, const vx_smooth* sp, bool host, float* xyz, uint64_t vcap, int32_t* tri, uint64_t tcap, int32_t* mat,
                             float* normals, uint64_t* num_vertices, uint64_t* num_triangles)
{
    if ((vcap || tcap) && (!xyz || !tri)) return fail(VX_ERR_INVALID_ARG, "null argument");
    DeviceGuard dg(g->device);
    uint64_t nv = 0, nt = 0;
    const int16_t* ids = nullptr;
    VX_TRY(surface_count(g, mat != nullptr, &nv, &nt, &ids));
    if (num_vertices) *num_vertices = nv;
    if (num_triangles) *num_triangles = nt;
    VX_TRY(surface_check(nv, nt, vcap, tcap));
    if ((!vcap && !tcap) || (!nv && !nt)) return VX_OK;
    const vx::SurfacePlan p = vx::surface_plan(g->g);
    float* dx = xyz;
    int32_t* dt = tri;
    int32_t* dm = mat;
    float* dn = normals;
    if (host) {  // one staging block: positions, normals, triangles, ids
        VX_HIP(g->surf_out.ensure((size_t)nv * 12 + (normals ? (size_t)nv * 12 : 0) + (size_t)nt * 12 + (mat ? (size_t)nt * 4 : 0) + 16));
        dx = g->surf_out.as<float>();
        dn = normals ? dx + 3 * nv : nullptr;
        dt = reinterpret_cast<int32_t*>(dx + (normals ? 6 : 3) * nv);
        dm = mat ? dt + 3 * nt : nullptr;
    }
    const uint32_t* wprefix = mat ? g->wprefix.as<uint32_t>() : nullptr;
    if (sp) {
        vx::NetsBufs nb;
        VX_HIP(g->nets_buf.ensure(vx::nets_bytes(nv, nullptr)));
        nb.base = g->nets_buf.p;
        vx::nets_bytes(nv, &nb);
        vx::launch_surface_nets(g->words.as<uint32_t>(), g->g, p, g->surf_cm.as<uint32_t>(), g->surf_vpre.as<uint32_t>(), nv, nb, sp->iterations,
                                sp->lambda, sp->mu, dx, dn, g->stream);
        vx::launch_surface_tris(g->words.as<uint32_t>(), g->g, g->surf_tpre.as<uint32_t>(), g->surf_cm.as<uint32_t>(), g->surf_vpre.as<uint32_t>(),
                                wprefix, ids, dt, dm, g->stream);
    } else {
        vx::launch_surface_emit(g->words.as<uint32_t>(), g->g, p, g->surf_tpre.as<uint32_t>(), g->surf_cm.as<uint32_t>(),
                                g->surf_vpre.as<uint32_t>(), wprefix, ids, dx, dt, dm, g->stream);
    }
    VX_HIP(hipGetLastError());
    if (host) {
        VX_HIP(hipMemcpyAsync(xyz, dx, (size_t)nv * 12, hipMemcpyDeviceToHost, g->stream));
        VX_HIP(hipMemcpyAsync(tri, dt, (size_t)nt * 12, hipMemcpyDeviceToHost, g->stream));
        if (mat) VX_HIP(hipMemcpyAsync(mat, dm, (size_t)nt * 4, hipMemcpyDeviceToHost, g->stream));
        if (normals) VX_HIP(hipMemcpyAsync(normals, dn, (size_t)nv * 12, hipMemcpyDeviceToHost, g->stream));
        VX_HIP(hipStreamSynchronize(g->stream));
    }
    return VX_OK;
}

vx_status vx_grid_surface_device(const vx_grid* gc, float* dev_xyz, uint64_t vertex_capacity, int32_t* dev_tri, uint64_t triangle_capacity,
                                 int32_t* dev_mat, uint64_t* num_vertices, uint64_t* num_triangles)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    return surface_run(const_cast<vx_grid*>(gc), nullptr, false, dev_xyz, vertex_capacity, dev_tri, triangle_capacity, dev_mat, nullptr,
                       num_vertices, num_triangles);
}

vx_status vx_grid_surface(const vx_grid* gc, float* host_xyz, uint64_t vertex_capacity, int32_t* host_tri, uint64_t triangle_capacity,
                          int32_t* host_mat, uint64_t* num_vertices, uint64_t* num_triangles)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    return surface_run(const_cast<vx_grid*>(gc), nullptr, true, host_xyz, vertex_capacity, host_tri, triangle_capacity, host_mat, nullptr,
                       num_vertices, num_triangles);
}

vx_status vx_grid_surface_smooth_device(const vx_grid* gc, const vx_smooth* params, float* dev_xyz, uint64_t vertex_capacity, int32_t* dev_tri,
                                        uint64_t triangle_capacity, int32_t* dev_mat, float* dev_normals, uint64_t* num_vertices,
                                        uint64_t* num_triangles)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(smooth_params(params));
    return surface_run(const_cast<vx_grid*>(gc), params, false, dev_xyz, vertex_capacity, dev_tri, triangle_capacity, dev_mat, dev_normals,
                       num_vertices, num_triangles);
}

vx_status vx_grid_surface_smooth(const vx_grid* gc, const vx_smooth* params, float* host_xyz, uint64_t vertex_capacity, int32_t* host_tri,
                                 uint64_t triangle_capacity, int32_t* host_mat, float* host_normals, uint64_t* num_vertices,
                                 uint64_t* num_triangles)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(smooth_params(params));
    return surface_run(const_cast<vx_grid*>(gc), params, true, host_xyz, vertex_capacity, host_tri, triangle_capacity, host_mat, host_normals,
                       num_vertices, num_triangles);
}

// The mesh of either surface as a vx_mesh (sp as for surface_run, already checked): the size query is vx_grid_surface's for both.
static vx_status surface_mesh(const vx_grid* gc, const vx_smooth* sp, int with_materials, int with_normals, vx_mesh** out)
{
    if (with_materials) {
        const int16_t* ids = nullptr;
        VX_TRY(surface_materials(gc, &ids));
    }
    uint64_t nv = 0, nt = 0;
    VX_TRY(vx_grid_surface(gc, nullptr, 0, nullptr, 0, nullptr, &nv, &nt));
    std::vector<float> xyz((size_t)nv * 3 + 1), nrm(with_normals ? (size_t)nv * 3 + 1 : 0);
    std::vector<int32_t> tri((size_t)nt * 3 + 1), mat(with_materials ? (size_t)nt + 1 : 0);
    if (nv || nt)
        VX_TRY(surface_run(const_cast<vx_grid*>(gc), sp, true, xyz.data(), nv, tri.data(), nt, with_materials ? mat.data() : nullptr,
                           with_normals ? nrm.data() : nullptr, &nv, &nt));
    vx_mesh* m = nullptr;
    VX_TRY(vx_mesh_from_arrays(xyz.data(), (size_t)nv, tri.data(), (size_t)nt, &m));
    vx_status st = VX_OK;
    if (with_materials) st = vx_mesh_set_materials(m, gc->materials.data(), gc->materials.size(), mat.data());
    if (st == VX_OK && with_normals) {  // per triangle, its three corners' vertex normals
        std::vector<float> cn((size_t)nt * 9 + 1);
        for (size_t c = 0; c < (size_t)nt * 3; ++c)
            for (int a = 0; a < 3; ++a) cn[c * 3 + a] = nrm[(size_t)tri[c] * 3 + a];
        st = vx_mesh_set_attributes(m, cn.data(), nullptr);
    }
    if (st != VX_OK) { vx_mesh_free(m); return st; }
    *out = m;
    return VX_OK;
}

vx_status vx_grid_surface_mesh(const vx_grid* gc, int with_materials, vx_mesh** out)
{
    if (!gc || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    return surface_mesh(gc, nullptr, with_materials, 0, out);
}

vx_status vx_grid_surface_smooth_mesh(const vx_grid* gc, const vx_smooth* params, int with_materials, int with_normals, vx_mesh** out)
{
    if (!gc || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(smooth_params(params));
    return surface_mesh(gc, params, with_materials, with_normals, out);
}

// Connected components: the argument checks in the header's order, then the labelling passes and one scan on the grid's stream
// (vx_components.hip).  The passes only read the bitmask; the union-find's parent array is the label buffer itself.  *empty: a grid of
// 0 cells (VX_OK, nothing to write).
static vx_status components_check(const vx_grid* g, uint32_t connectivity, bool* empty)
{
    if (connectivity != VX_CONNECT_6 && connectivity != VX_CONNECT_26) return fail(VX_ERR_INVALID_ARG, "connectivity must be VX_CONNECT_6 or VX_CONNECT_26");
    *empty = !g->g.nvox;
    if (*empty) return VX_OK;
    if (g->g.nvox > 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, "components need X*Y*Z <= 2^32 - 1 (32-bit labels and union-find indices)");
    return VX_OK;
}

// labels (X*Y*Z, device) <- the labels; K lands in the mailbox and, when dev_count is non-null, in *dev_count on the device
static vx_status components_queue(vx_grid* g, uint32_t connectivity, uint32_t* labels, uint32_t* dev_count)
{
    VX_HIP(g->cc_roots.ensure((size_t)(g->g.nwords + 4) * 4));
    VX_HIP(g->cc_rpre.ensure((size_t)(g->g.nwords + 4) * 4));
    VX_HIP(g->up.scantmp.reserve(g->g.nwords, g->stream));  // (ahead of the union-find kernel)
    vx::launch_components(g->words.as<uint32_t>(), g->g, connectivity == VX_CONNECT_26, labels, g->cc_roots.as<uint32_t>(), g->stream);
    VX_TRY(g->up.scantmp.u32(g->cc_roots, g->cc_rpre, g->g.nwords, true, &g->mail->cc_count, g->stream));
    vx::launch_components_label(g->words.as<uint32_t>(), g->g, labels, g->cc_roots.as<uint32_t>(), g->cc_rpre.as<uint32_t>(), dev_count, g->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// the labels into the handle's staging buffer (and on to host_labels, when non-null), one host wait, K
static vx_status components_host(vx_grid* g, uint32_t connectivity, uint32_t* host_labels, uint64_t* k)
{
    VX_HIP(g->cc_lab.ensure((size_t)g->g.nvox * 4));
    VX_TRY(components_queue(g, connectivity, g->cc_lab.as<uint32_t>(), nullptr));
    if (host_labels) VX_HIP(hipMemcpyAsync(host_labels, g->cc_lab.p, (size_t)g->g.nvox * 4, hipMemcpyDeviceToHost, g->stream));
    return mail_total(&g->mail->cc_count, 0, g->stream, "components need X*Y*Z <= 2^32 - 1 (32-bit labels and union-find indices)", k);
}

vx_status vx_grid_components_device(const vx_grid* gc, uint32_t connectivity, uint32_t* dev_labels, uint64_t capacity, uint32_t* dev_count)
{
    if (!gc || !dev_labels) return fail(VX_ERR_INVALID_ARG, "null argument");
    bool empty = false;
    VX_TRY(components_check(gc, connectivity, &empty));
    if (empty) return VX_OK;
    if (capacity < gc->g.nvox) return fail(VX_ERR_CAPACITY, "component label buffer too small");
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    return components_queue(g, connectivity, dev_labels, dev_count);
}

vx_status vx_grid_components(const vx_grid* gc, uint32_t connectivity, uint32_t* host_labels, uint64_t capacity, uint64_t* count)
{
    if (!gc || (capacity && !host_labels)) return fail(VX_ERR_INVALID_ARG, "null argument");
    bool empty = false;
    VX_TRY(components_check(gc, connectivity, &empty));
    if (count) *count = 0;
    if (empty) return VX_OK;
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    const bool write = host_labels && capacity >= g->g.nvox;
    uint64_t k = 0;
    VX_TRY(components_host(g, connectivity, write ? host_labels : nullptr, &k));
    if (count) *count = k;
    if (host_labels && !write) return fail(VX_ERR_CAPACITY, "component label buffer too small");
    return VX_OK;
}

vx_status vx_grid_component_stats(const vx_grid* gc, uint32_t connectivity, vx_component* host_out, uint64_t capacity, uint64_t* count)
{
    if (!gc || (capacity && !host_out)) return fail(VX_ERR_INVALID_ARG, "null argument");
    bool empty = false;
    VX_TRY(components_check(gc, connectivity, &empty));
    if (count) *count = 0;
    if (empty) return VX_OK;
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    uint64_t k = 0;
    VX_TRY(components_host(g, connectivity, nullptr, &k));
    if (count) *count = k;
    if (!capacity) return VX_OK;  // (size query)
    if (capacity < k) return fail(VX_ERR_CAPACITY, "component statistics buffer too small");
    if (!k) return VX_OK;
    VX_HIP(g->cc_stat.ensure((size_t)k * sizeof(vx_component)));
    vx::launch_component_stats(g->cc_lab.as<uint32_t>(), g->g, k, g->cc_stat.as<uint32_t>(), g->stream);
    VX_HIP(hipGetLastError());
    VX_HIP(hipMemcpyAsync(host_out, g->cc_stat.p, (size_t)k * sizeof(vx_component), hipMemcpyDeviceToHost, g->stream));
    VX_HIP(hipStreamSynchronize(g->stream));
    return VX_OK;
}

vx_status vx_grid_aabbs_device(const vx_grid* gc, vx_aabb* dev_out, uint64_t cap, uint64_t* count)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    if (g->kind == VX_GRID_VEC) {
        if (count) *count = g->vec_count;
        const uint64_t n = cap < g->vec_count ? cap : g->vec_count;
        if (n && dev_out && dev_out != g->vec_ptr()) {  // (a bound buffer already holds the list: nothing to copy)
            VX_HIP(g->list_resolve());
            VX_HIP(hipMemcpyAsync(dev_out, g->vec_ptr(), (size_t)n * sizeof(vx_aabb), hipMemcpyDeviceToDevice, g->stream));
        }
        // (a VX_VOXELIZE_LIST_ASYNC build's list in its bound buffer: the count now, the records after vx_grid_list_wait)
        return VX_OK;
    }
    // queue the prefix scan and the emission back to back, then wait once for the count
    VX_HIP(g->list_resolve());
    bool pending = false;
    VX_TRY(prefix_launch(g, &pending));
    if (cap && dev_out && (pending || g->occupied))
        vx::launch_emit_bool_aabbs(g->words.as<uint32_t>(), g->wprefix.as<uint32_t>(), g->g, dev_out, cap, g->stream, g->sel_valid ? g->wsel.as<uint32_t>() : nullptr);
    if (pending) VX_TRY(ensure_coarse(g));  // (as in vx_grid_aabbs_device_async: the traversal structure of an externally written mask, built while the host waits)
    VX_TRY(prefix_finish(g, pending));
    if (count) *count = g->occupied;
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_grid_aabbs_device_async(const vx_grid* gc, vx_aabb* dev_out, uint64_t cap, uint64_t* count)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_grid* g = const_cast<vx_grid*>(gc);
    if (g->kind == VX_GRID_VEC) return vx_grid_aabbs_device(gc, dev_out, cap, count);  // (a Vec list is deferred by its build: VX_VOXELIZE_LIST_ASYNC)
    DeviceGuard dg(g->device);
    VX_HIP(g->list_resolve());
    // the word prefix on the grid's stream (the ray batch's primitive ids need it there anyway) and its total = the list's length; the
    // emission itself waits for the next ray batch (trace_common) or for whoever reads the list first (list_resolve)
    bool pending = false;
    VX_TRY(prefix_launch(g, &pending));
    // a mask written from outside (the multi-rank exchange) has no traversal structure yet: queued here, it is built while the host waits
    // for the count instead of after it, in front of the caller's ray batch
    if (pending) VX_TRY(ensure_coarse(g));
    VX_TRY(prefix_finish(g, pending));
    if (count) *count = g->occupied;
    if (cap && dev_out && g->occupied) {
        g->ld.from_mask = true;
        g->ld.tgt = dev_out;
        g->ld.cap = cap;
        g->list_deferred = true;
    }
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_grid_aabbs(const vx_grid* gc, vx_aabb* host_out, uint64_t cap, uint64_t* count)
{
    if (!gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    uint64_t n = 0;
    if (g->kind == VX_GRID_VEC) n = g->vec_count;
    else { VX_TRY(ensure_prefix(g)); n = g->occupied; }
    if (count) *count = n;
    const uint64_t m = cap < n ? cap : n;
    if (!m || !host_out) return VX_OK;
    if (g->kind == VX_GRID_VEC) {
        VX_HIP(g->list_resolve());
        VX_HIP(hipMemcpyAsync(host_out, g->vec_ptr(), (size_t)m * sizeof(vx_aabb), hipMemcpyDeviceToHost, g->stream));
        VX_HIP(hipStreamSynchronize(g->stream));
        return VX_OK;
    }
    Staging s(*g);
    vx_aabb* list = s.out(host_out, (size_t)m * sizeof(vx_aabb));
    VX_TRY(s.status());
    vx::launch_emit_bool_aabbs(g->words.as<uint32_t>(), g->wprefix.as<uint32_t>(), g->g, list, m, g->stream, g->sel_valid ? g->wsel.as<uint32_t>() : nullptr);
    return s.finish();
}

vx_status vx_grid_list_wait(vx_grid* g)
{
    if (!g) return fail(VX_ERR_INVALID_ARG, "null argument");
    DeviceGuard dg(g->device);
    VX_HIP(g->list_resolve());
    return VX_OK;
}

vx_status vx_grid_bind_aabbs_device(vx_grid* g, vx_aabb* dev_out, uint64_t capacity)
{
    if (!g) return fail(VX_ERR_INVALID_ARG, "null argument");
    { DeviceGuard dg0(g->device); VX_HIP(g->list_resolve()); }
    if (g->vec_in_bound && g->vec_count) {  // keep the current list reachable: move it into the grid's own storage first
        DeviceGuard dg(g->device);
        VX_HIP(g->vec.ensure((size_t)(g->vec_count + 1) * sizeof(vx_aabb)));
        VX_HIP(hipMemcpyAsync(g->vec.p, g->bound, (size_t)g->vec_count * sizeof(vx_aabb), hipMemcpyDeviceToDevice, g->stream));
        VX_HIP(hipStreamSynchronize(g->stream));
    }
    g->vec_in_bound = false;
    g->bound = capacity ? dev_out : nullptr;
    g->bound_cap = dev_out ? capacity : 0;
    return VX_OK;
}

vx_status vx_grid_materials(const vx_grid* g, vx_material* out, uint64_t cap, uint64_t* count)
{
    if (!g || (!out && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    const uint64_t n = g->has_materials ? g->materials.size() : 0;
    if (count) *count = n;
    const uint64_t m = cap < n ? cap : n;
    if (m) std::memcpy(out, g->materials.data(), (size_t)m * sizeof(vx_material));
    return VX_OK;
}

vx_status vx_grid_material_ids(const vx_grid* g, int16_t* out, uint64_t cap, uint64_t* count)
{
    if (!g || (!out && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    const uint64_t n = g->has_materials ? (g->mat_gathered ? g->mat_gather_count : g->mat_count) : 0;
    if (count) *count = n;
    const uint64_t m = cap < n ? cap : n;
    if (!m) return VX_OK;
    DeviceGuard dg(g->device);
    VX_HIP(hipMemcpyAsync(out, g->mat_gathered ? g->mattmp.p : g->matids.p, (size_t)m * 2, hipMemcpyDeviceToHost, g->stream));
    VX_HIP(hipStreamSynchronize(g->stream));
    return VX_OK;
}

vx_status vx_grid_material_first_use(const vx_grid* g, int64_t* out, uint64_t cap, uint64_t* count)
{
    if (!g || (!out && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (!g->mat_pending && !g->has_materials) return fail(VX_ERR_INVALID_ARG, "the grid was not built with VX_VOXELIZE_MATERIALS");
    const uint64_t n = g->mat_first_use.size();
    if (count) *count = n;
    const uint64_t m = cap < n ? cap : n;
    for (uint64_t i = 0; i < m; ++i) out[i] = (int64_t)g->mat_first_use[i];
    return VX_OK;
}

vx_status vx_grid_finish_materials(vx_grid* g, const int64_t* first_use_min, uint64_t count)
{
    if (!g || (!first_use_min && count)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (!g->mat_pending) return g->has_materials ? VX_OK : fail(VX_ERR_INVALID_ARG, "the grid was not built with VX_VOXELIZE_MATERIALS");
    std::vector<long long> fu(first_use_min, first_use_min + count);
    return finish_materials(g, fu.data(), fu.size());
}

const int16_t* vx_grid_material_ids_device(const vx_grid* g)
{
    if (!g || !g->has_materials) return nullptr;
    if (g->mat_gathered) return g->mat_gather_count ? g->mattmp.as<int16_t>() : nullptr;
    return g->mat_count ? g->matids.as<int16_t>() : nullptr;
}

void vx_grid_free(vx_grid* g) { handle_free(g); }

// ---- distance-field queries (vx_field.hip) ----------------------------------------------------------------------
// A snapshot of the signed field in a block of its own, and the blocks the host variants stage through: they stay on the handle, so a
// repeated call of the same size asks the pool for nothing.
struct vx_field : Home {
    vx::FieldGeom G{};
    uint64_t nvox = 0;
    DevBuf values{this};
    DevBuf st_in{this}, st_tmax{this}, st_radius{this};            // points or rays, tmax_per_ray, radius_per_ray
    DevBuf st_a{this}, st_b{this}, st_c{this}, st_d{this};         // value / t, gradient / clearance, steps, occupied / status
    DevBuf st_xf{this}, st_e{this};                                // pose queries: transforms, position (the rest goes through the blocks above)
    DevBuf pose_keys{this}, pose_counts{this};                     // pose queries: the reduction's scratch, 8 + 4 bytes per pose
};

// The snapshot: the signed field's passes on the GRID's stream into the field's block (which no query reads meanwhile: the field's stream
// is drained first), the state from the occupied count, one wait.  The grid's readers see no change (distance_queue).
static vx_status field_snapshot(vx_field* f, vx_grid* g)
{
    DeviceGuard dg(g->device);
    VX_HIP(hipStreamSynchronize(f->stream));
    VX_TRY(ensure_occupied(g));
    VX_TRY(distance_queue(g, 2, f->values.p));
    VX_HIP(hipStreamSynchronize(g->stream));
    for (int a = 0; a < 3; ++a) { f->G.org[a] = g->g.org[a]; f->G.dim[a] = g->g.dim[a]; }
    f->G.vs = g->g.vs;
    f->G.state = g->occupied == 0 ? VX_FIELD_EMPTY : (g->occupied == g->g.nvox ? VX_FIELD_FULL : VX_FIELD_FINITE);
    return VX_OK;
}

vx_status vx_field_create(const vx_grid* gc, void* stream, vx_field** out)
{
    if (out) *out = nullptr;
    if (!gc || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (!gc->g.nvox) return fail(VX_ERR_INVALID_ARG, "a field needs a grid of at least one cell");
    uint64_t n = 0;
    VX_TRY(distance_check(gc, ~0ull, &n));
    vx_grid* g = const_cast<vx_grid*>(gc);
    Fresh<vx_field> f(new vx_field());
    f->device = g->device;
    f->stream = (hipStream_t)stream;
    f->nvox = n;
    DeviceGuard dg(g->device);
    const hipError_t e = f->values.ensure((size_t)n * 4);
    if (e != hipSuccess) return fail(VX_ERR_HIP, std::string("the field's block: ") + hipGetErrorString(e));
    VX_TRY(field_snapshot(f.get(), g));
    *out = f.release();
    return VX_OK;
}

vx_status vx_field_update(vx_field* f, const vx_grid* gc)
{
    if (!f || !gc) return fail(VX_ERR_INVALID_ARG, "null argument");
    for (int a = 0; a < 3; ++a)
        if (gc->g.dim[a] != f->G.dim[a]) return fail(VX_ERR_INVALID_ARG, "vx_field_update needs a grid of the field's dimensions");
    if (gc->device != f->device) return fail(VX_ERR_INVALID_ARG, "vx_field_update needs a grid on the field's device");
    return field_snapshot(f, const_cast<vx_grid*>(gc));
}

vx_status vx_field_describe(const vx_field* f, vx_field_desc* d)
{
    if (!f || !d) return fail(VX_ERR_INVALID_ARG, "null argument");
    std::memset(d, 0, sizeof(*d));
    for (int a = 0; a < 3; ++a) { d->dim[a] = f->G.dim[a]; d->origin[a] = f->G.org[a]; }
    d->voxel_size = f->G.vs;
    d->state = f->G.state;
    d->bytes = f->nvox * 4;
    return VX_OK;
}

const float* vx_field_values_device(const vx_field* f) { return f ? f->values.as<float>() : nullptr; }

void vx_field_free(vx_field* f) { handle_free(f); }

// The three queries in trace_entry's order: the checks, the zero-count return, the guard, then one launch on the caller's device arrays or
// (host) on a Staging over the handle's st_* blocks.
static vx_status field_sample_entry(const vx_field* fc, const vx_field_sample_args* a, bool host)
{
    if (!fc || !a) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (a->num_points && !a->points) return fail(VX_ERR_INVALID_ARG, "null points");
    if (!a->value && !a->gradient && !a->occupied) return fail(VX_ERR_INVALID_ARG, "the sample needs at least one output");
    const size_t n = (size_t)a->num_points;
    if (!n) return VX_OK;
    vx_field* f = const_cast<vx_field*>(fc);
    DeviceGuard dg(f->device);
    vx_field_sample_args io = *a;
    Staging s(*f);
    if (host) {
        io.value = s.out(a->value, n * 4, 0, &f->st_a);
        io.gradient = s.out(a->gradient, n * 12, 0, &f->st_b);
        io.occupied = s.out(a->occupied, n, 0, &f->st_d);
        io.points = s.in(a->points, n * 12, &f->st_in);
        VX_TRY(s.status());
    }
    vx::launch_field_sample(f->values.as<float>(), f->G, io.points, n, io.value, io.gradient, io.occupied, f->stream);
    VX_HIP(hipGetLastError());
    return host ? s.finish() : VX_OK;
}

vx_status vx_field_sample_device(const vx_field* f, const vx_field_sample_args* a) { return field_sample_entry(f, a, false); }
vx_status vx_field_sample(const vx_field* f, const vx_field_sample_args* a) { return field_sample_entry(f, a, true); }

static vx_status field_trace_entry(const vx_field* fc, const vx_field_trace_args* a, bool host)
{
    if (!fc || !a) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (a->num_rays && !a->rays) return fail(VX_ERR_INVALID_ARG, "null rays");
    if (!a->t && !a->clearance && !a->steps && !a->status) return fail(VX_ERR_INVALID_ARG, "the sphere cast needs at least one output");
    if (!(a->step_scale == 0.0f || (a->step_scale > 0.0f && a->step_scale <= 1.0f))) return fail(VX_ERR_INVALID_ARG, "step_scale must be 0 or in (0, 1]");
    if (!(a->hit_eps >= 0.0f) || std::isinf(a->hit_eps)) return fail(VX_ERR_INVALID_ARG, "hit_eps must be finite and not negative");
    if (a->max_steps > 65535u) return fail(VX_ERR_INVALID_ARG, "max_steps must be at most 65535");
    if (!a->radius_per_ray && (!(a->radius >= 0.0f) || std::isinf(a->radius))) return fail(VX_ERR_INVALID_ARG, "radius must be finite and not negative");
    const size_t n = (size_t)a->num_rays;
    if (!n) return VX_OK;
    vx_field* f = const_cast<vx_field*>(fc);
    DeviceGuard dg(f->device);
    vx::FieldTraceIO io{};
    io.rays = a->rays; io.nrays = n;
    io.tmin = a->tmin; io.tmax = a->tmax; io.tmax_per_ray = a->tmax_per_ray;
    io.radius = a->radius; io.radius_per_ray = a->radius_per_ray;
    io.step_scale = a->step_scale == 0.0f ? 0.25f : a->step_scale;
    io.hit_eps = a->hit_eps == 0.0f ? 0.015625f : a->hit_eps;
    io.max_steps = a->max_steps ? a->max_steps : 256u;
    io.t = a->t; io.clearance = a->clearance; io.steps = a->steps; io.status = a->status;
    Staging s(*f);
    if (host) {
        io.t = s.out(io.t, n * 4, 0, &f->st_a);
        io.clearance = s.out(io.clearance, n * 4, 0, &f->st_b);
        io.steps = s.out(io.steps, n * 4, 0, &f->st_c);
        io.status = s.out(io.status, n, 0, &f->st_d);
        io.rays = s.in(io.rays, n * 24, &f->st_in);
        io.tmax_per_ray = s.in(io.tmax_per_ray, n * 4, &f->st_tmax);
        io.radius_per_ray = s.in(io.radius_per_ray, n * 4, &f->st_radius);
        VX_TRY(s.status());
    }
    vx::launch_field_trace(f->values.as<float>(), f->G, io, f->stream);
    VX_HIP(hipGetLastError());
    return host ? s.finish() : VX_OK;
}

vx_status vx_field_sphere_trace_device(const vx_field* f, const vx_field_trace_args* a) { return field_trace_entry(f, a, false); }
vx_status vx_field_sphere_trace(const vx_field* f, const vx_field_trace_args* a) { return field_trace_entry(f, a, true); }

// Pose queries (vx_poses.hip).  Every check before a block is asked for; the reduction's scratch before the arrays.
static vx_status field_poses_entry(const vx_field* fc, const vx_field_pose_args* a, bool host)
{
    if (!fc || !a) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (a->num_poses && !a->transforms) return fail(VX_ERR_INVALID_ARG, "null transforms");
    if (a->num_points && !a->points) return fail(VX_ERR_INVALID_ARG, "null points");
    if (!a->clearance && !a->point && !a->count && !a->position && !a->gradient) return fail(VX_ERR_INVALID_ARG, "the pose query needs at least one output");
    if (a->margin != a->margin) return fail(VX_ERR_INVALID_ARG, "margin must not be NaN");
    if (a->num_points > 0xFFFFFFFEull) return fail(VX_ERR_CAPACITY, "a body has at most 0xFFFFFFFE points");
    const size_t n = (size_t)a->num_poses, np = (size_t)a->num_points;
    if (!n) return VX_OK;
    vx_field* f = const_cast<vx_field*>(fc);
    DeviceGuard dg(f->device);
    VX_HIP(f->pose_keys.ensure(n * 8));
    VX_HIP(f->pose_counts.ensure(n * 4));
    vx::FieldPoseIO io{};
    io.points = a->points; io.npoints = (uint32_t)np; io.radii = np ? a->radii : nullptr;
    io.transforms = a->transforms; io.nposes = n; io.margin = a->margin;
    io.keys = f->pose_keys.as<unsigned long long>(); io.counts = f->pose_counts.as<uint32_t>();
    io.clearance = a->clearance; io.point = a->point; io.count = a->count; io.position = a->position; io.gradient = a->gradient;
    Staging s(*f);
    if (host) {
        io.clearance = s.out(io.clearance, n * 4, 0, &f->st_a);
        io.gradient = s.out(io.gradient, n * 12, 0, &f->st_b);
        io.point = s.out(io.point, n * 4, 0, &f->st_c);
        io.count = s.out(io.count, n * 4, 0, &f->st_d);
        io.position = s.out(io.position, n * 12, 0, &f->st_e);
        io.points = s.in(np ? io.points : nullptr, np * 12, &f->st_in);  // (a body of no points: no array)
        io.radii = s.in(io.radii, np * 4, &f->st_radius);
        io.transforms = s.in(io.transforms, n * 48, &f->st_xf);
        VX_TRY(s.status());
    }
    VX_HIP(vx::launch_field_poses(f->values.as<float>(), f->G, io, f->stream));
    return host ? s.finish() : VX_OK;
}

vx_status vx_field_poses_device(const vx_field* f, const vx_field_pose_args* a) { return field_poses_entry(f, a, false); }
vx_status vx_field_poses(const vx_field* f, const vx_field_pose_args* a) { return field_poses_entry(f, a, true); }

// ---- rays -----------------------------------------------------------------------------------------------------
// the grid's traversal structure as launch_trace takes it; *p16: the 16th-prefix table of the word prefix for the rank pass, null where it
// cannot be used (no scan on the stream has written it; the mask is allocated with two spare words, so a rank may read its voxel's whole
// 16-word group only when that lies inside: nwords % 16 == 0)
static vx::TraceMips grid_mips(const vx_grid* g, const uint32_t** p16)
{
    vx::TraceMips mips;
    mips.bricks3 = g->bricks.as<unsigned long long>();
    mips.w0 = g->words.as<uint32_t>();
    mips.w1 = g->cwords.as<uint32_t>();
    mips.w2 = g->c2words.as<uint32_t>();
    for (int a = 0; a < 3; ++a) { mips.d1[a] = g->cdim[a]; mips.d2[a] = g->c2dim[a]; }
    *p16 = ((g->sel_valid || g->p16_valid) && (g->g.nwords % 16) == 0) ? g->wp16.as<uint32_t>() : nullptr;
    return mips;
}

// primary rays: the batch's camera (io.cam, on the caller's stack) into the handle's device copy, for the kernels to read as io.cam_dev
static vx_status upload_camera(DevBuf& buf, hipStream_t stream, vx::TraceIO& io)
{
    if (!io.cam) return VX_OK;
    VX_HIP(buf.ensure(sizeof(vx::Camera)));
    VX_HIP(hipMemcpyAsync(buf.p, io.cam, sizeof(vx::Camera), hipMemcpyHostToDevice, stream));
    VX_HIP(hipStreamSynchronize(stream));  // the host copy lives on the caller's stack
    io.cam_dev = buf.as<vx::Camera>();
    return VX_OK;
}

// The first-hit query on device arrays.  The four structures' *_trace_common share one signature, (handle, io, bary, instance), so that
// trace_entry can call any of them; the grid and the octree have neither output.
static vx_status trace_common(vx_grid* g, vx::TraceIO io, float* = nullptr, uint32_t* = nullptr)
{
    VX_TRY(ensure_coarse(g));
    const uint32_t* prefix = nullptr;
    void* idx_tmp = nullptr;
    vx::WalkRing ring;
    if (io.prim_out || io.hits || io.normal_out) {
        bool pending = false;
        VX_TRY(rank_launch(g, &pending));  // the ranks need wp16 or the prefix array on the stream, not the count on the host
        prefix = g->prefix_valid ? g->wprefix.as<uint32_t>() : nullptr;
        VX_HIP(g->idxtmp.ensure(vx::trace_idx_bytes(g->g, io.nrays)));
        idx_tmp = g->idxtmp.p;
        // prim alone: the ray kernel's waves rank their own rays as they leave, from the chunk ring, where one launch and a ring of a sane
        // size cover the batch (walk_ring_cap); that rank does not read t
        uint32_t waves = 0;
        const uint32_t cap = (io.prim_out && !io.hits && !io.normal_out && vx::trace_idx32(g->g)) ? vx::walk_ring_cap(io.nrays, &waves) : 0u;
        if (cap) {
            VX_HIP(g->wring.ensure((size_t)waves * cap * 4));
            ring.words = g->wring.as<uint32_t>();
            ring.cap = cap;
            ring.waves = waves;
        } else if (!io.t_out) {  // the rank / normal / compaction pass reads t
            VX_HIP(g->ttmp.ensure((size_t)io.nrays * 4 + 8));
            io.t_out = g->ttmp.as<float>();
        }
    }
    const uint32_t* p16 = nullptr;  // (read by the rank pass only, which runs with `prefix`)
    const vx::TraceMips mips = grid_mips(g, &p16);
    VX_TRY(upload_camera(g->camera, g->stream, io));
    const bool list_beside = g->list_deferred;  // VX_VOXELIZE_LIST_ASYNC: the list's emission goes beside this ray batch
    if (list_beside) VX_HIP(g->list_side_begin());
    vx::WalkQueue wq;
    const bool queued = vx::launch_trace(g->g, mips, prefix, io, g->small.as<Small>()->trace_counters, &g->trace_phase, idx_tmp, g->stream, p16, list_beside ? &wq : nullptr,
                                         ring.words ? &ring : nullptr);
    if (list_beside) VX_HIP(g->list_side_launch(wq.counter, wq.dry_at));
    VX_HIP(hipGetLastError());
    if (!queued) return fail(VX_ERR_UNSUPPORTED, "internal: the ray kernel declined the rank epilogue its ring was sized for");
    return VX_OK;
}

vx_status vx_trace_device(const vx_grid* gc, const float* dev_rays, uint64_t nrays, float tmin, float tmax, float* dev_t, uint32_t* dev_prim,
                          vx_hit* dev_hits, uint64_t* dev_nhits)
{
    if (!gc || (nrays && !dev_rays)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (dev_hits && !dev_nhits) return fail(VX_ERR_INVALID_ARG, "dev_hits needs dev_num_hits");
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    vx::TraceIO io;
    io.rays = dev_rays; io.nrays = nrays; io.tmin = tmin; io.tmax = tmax;
    io.t_out = dev_t; io.prim_out = dev_prim; io.hits = dev_hits; io.nhits = (unsigned long long*)dev_nhits;
    return trace_common(g, io);
}

vx_status vx_trace_primary_device(const vx_grid* gc, const float vi[16], const float pi[16], uint32_t w, uint32_t h, float tmin, float tmax,
                                  float* dev_t, uint32_t* dev_prim)
{
    if (!gc || !vi || !pi || !dev_t) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx_grid* g = const_cast<vx_grid*>(gc);
    DeviceGuard dg(g->device);
    vx::Camera cam;
    std::memcpy(cam.viewInv, vi, 64);
    std::memcpy(cam.projInv, pi, 64);
    cam.width = w;
    cam.height = h;
    vx::TraceIO io;
    io.cam = &cam; io.nrays = (uint64_t)w * h; io.tmin = tmin; io.tmax = tmax; io.t_out = dev_t; io.prim_out = dev_prim;
    return trace_common(g, io);
}

// The four structures share one argument form inside the library: vx_tlas_trace_args, of which vx_trace_args (grid, octree) and
// vx_bvh_trace_args are leading parts.
static vx_tlas_trace_args from_trace_args(const vx_trace_args* a)
{
    vx_tlas_trace_args x{};
    if (a) x.base = *a;
    return x;
}

static vx_tlas_trace_args from_bvh_trace_args(const vx_bvh_trace_args* a)
{
    vx_tlas_trace_args x{};
    if (a) { x.base = a->base; x.bary = a->bary; }
    return x;
}

// The argument checks of the ray queries, in the header's order; *io receives the batch, and points at *cam for camera rays
static vx_status args_to_io(const vx_tlas_trace_args& x, vx::Camera* cam, vx::TraceIO* io)
{
    const vx_trace_args* a = &x.base;
    if (!a->rays && !(a->view_inverse && a->proj_inverse && a->width && a->height)) return fail(VX_ERR_INVALID_ARG, "no rays and no camera");
    if (a->hits && !a->num_hits) return fail(VX_ERR_INVALID_ARG, "hits needs num_hits");
    io->rays = a->rays;
    io->nrays = a->num_rays;
    if (!a->rays) {
        std::memcpy(cam->viewInv, a->view_inverse, 64);
        std::memcpy(cam->projInv, a->proj_inverse, 64);
        cam->width = a->width;
        cam->height = a->height;
        io->cam = cam;
        io->nrays = (uint64_t)a->width * a->height;
    }
    io->tmin = a->tmin; io->tmax = a->tmax; io->tmax_per_ray = a->tmax_per_ray; io->any_hit = a->any_hit != 0;
    io->t_out = a->t; io->prim_out = a->prim; io->normal_out = a->normal; io->shadowed_out = a->shadowed;
    io->hits = a->hits; io->nhits = (unsigned long long*)a->num_hits;
    if (io->any_hit && (io->prim_out || io->normal_out || io->hits || x.bary || x.instance))
        return fail(VX_ERR_INVALID_ARG, "any_hit reports only `shadowed` (and an arbitrary accepted t)");
    return VX_OK;
}

// The eight vx_*_trace_ex* entry points: the null checks, the argument checks, (host) the refusal of `hits` and the zero-ray return, the
// guard, then common(handle, io, bary, instance) on the caller's device arrays or on staged copies of the host arrays.  `given`: the
// caller's args pointer, `a` its conversion.
extern "C++" {
template <class H, class Common>
static vx_status trace_entry(const H* hc, const void* given, const vx_tlas_trace_args& a, bool host, Common common)
{
    if (!hc || !given) return fail(VX_ERR_INVALID_ARG, "null argument");
    vx::Camera cam{};
    vx::TraceIO io;
    VX_TRY(args_to_io(a, &cam, &io));
    H* h = const_cast<H*>(hc);
    if (!host) {
        DeviceGuard dg(h->device);
        return common(h, io, a.bary, a.instance);
    }
    if (io.hits) return fail(VX_ERR_UNSUPPORTED, "the compacted hit list is a device-side output: use the _device variant");
    const size_t n = (size_t)io.nrays;
    if (!n) return VX_OK;
    DeviceGuard dg(h->device);
    Staging s(*h);
    io.rays = s.in(io.rays, n * 24);
    io.tmax_per_ray = s.in(io.tmax_per_ray, n * 4);
    io.t_out = s.out(io.t_out, n * 4);
    io.prim_out = s.out(io.prim_out, n * 4);
    io.normal_out = s.out(io.normal_out, n * 12);
    io.shadowed_out = s.out(io.shadowed_out, n);
    float* bary = s.out(a.bary, n * 8, 16);
    uint32_t* inst = s.out(a.instance, n * 4, 16);
    VX_TRY(s.status());
    VX_TRY(common(h, io, bary, inst));
    return s.finish();
}
}  // extern "C++"

vx_status vx_trace_ex_device(const vx_grid* g, const vx_trace_args* args) { return trace_entry(g, args, from_trace_args(args), false, trace_common); }
vx_status vx_trace_ex(const vx_grid* g, const vx_trace_args* args) { return trace_entry(g, args, from_trace_args(args), true, trace_common); }

// ---- multi-hit query (vx_multihit.hip) -----------------------------------------------------------------------------
// The four structures share one argument form inside the library: vx_tlas_multihit_args, of which vx_multihit_args (grid, octree) and
// vx_bvh_multihit_args are leading parts.
static vx_tlas_multihit_args from_grid_args(const vx_multihit_args* a)
{
    vx_tlas_multihit_args x{};
    if (a) x.m = *a;
    return x;
}

static vx_tlas_multihit_args from_bvh_args(const vx_bvh_multihit_args* a)
{
    vx_tlas_multihit_args x{};
    if (a) { x.m = a->m; x.bary = a->bary; }
    return x;
}

// The checks of the eight vx_*_trace_multi* entry points, in the header's order (tlas: the cursor has an instance part); *io receives the ray
// batch (nrays == 0: nothing to do)
static vx_status multihit_args_to_io(const void* handle, const vx_tlas_multihit_args* a, bool tlas, vx::Camera* cam, vx::TraceIO* io)
{
    if (!handle || !a) return fail(VX_ERR_INVALID_ARG, "null argument");
    const vx_multihit_args& m = a->m;
    if (m.max_hits < 1 || m.max_hits > VX_MULTIHIT_MAX) return fail(VX_ERR_INVALID_ARG, "max_hits must be 1..VX_MULTIHIT_MAX");
    const bool cursor = m.after_t != nullptr;
    if (cursor != (m.after_prim != nullptr) || (tlas && cursor != (a->after_instance != nullptr)))
        return fail(VX_ERR_INVALID_ARG, tlas ? "the cursor needs after_t, after_instance and after_prim" : "the cursor needs both after_t and after_prim");
    const vx_trace_args& b = m.base;
    if (b.any_hit || b.normal || b.shadowed || b.hits || b.num_hits)
        return fail(VX_ERR_INVALID_ARG, "any_hit, normal, shadowed, hits and num_hits are not part of the multi-hit query");
    const bool camera = b.view_inverse && b.proj_inverse && b.width && b.height;
    if (!b.rays && !camera && !b.num_rays) { io->nrays = 0; return VX_OK; }  // zero rays
    return args_to_io(from_trace_args(&b), cam, io);
}

static vx::MultiIO multi_io(const vx_tlas_multihit_args& a)
{
    vx::MultiIO m;
    m.K = a.m.max_hits;
    m.count = a.m.count;
    m.bary = a.bary;
    m.instance = a.instance;
    m.after_t = a.m.after_t;
    m.after_instance = a.after_instance;
    m.after_prim = a.m.after_prim;
    return m;
}

// The eight vx_*_trace_multi* entry points: the checks, the zero-ray return, the guard, then common(handle, io, args) on the caller's device
// arrays or on staged copies of the host arrays.  `given`: the caller's args pointer, `a` its conversion; tlas: see multihit_args_to_io.
extern "C++" {
template <class H, class Common>
static vx_status multihit_entry(const H* hc, const void* given, const vx_tlas_multihit_args& a, bool tlas, bool host, Common common)
{
    vx::Camera cam{};
    vx::TraceIO io;
    VX_TRY(multihit_args_to_io(hc, given ? &a : nullptr, tlas, &cam, &io));
    if (!io.nrays) return VX_OK;
    H* h = const_cast<H*>(hc);
    DeviceGuard dg(h->device);
    if (!host) return common(h, io, a);
    const size_t n = (size_t)io.nrays, K = a.m.max_hits;
    Staging s(*h);
    vx_tlas_multihit_args d = a;
    io.rays = s.in(io.rays, n * 24);
    io.tmax_per_ray = s.in(io.tmax_per_ray, n * 4);
    d.m.after_t = s.in(a.m.after_t, n * 4);
    d.after_instance = s.in(a.after_instance, n * 4);
    d.m.after_prim = s.in(a.m.after_prim, n * 4);
    io.t_out = s.out(io.t_out, n * K * 4);
    io.prim_out = s.out(io.prim_out, n * K * 4);
    d.bary = s.out(a.bary, n * K * 8);
    d.instance = s.out(a.instance, n * K * 4);
    d.m.count = s.out(a.m.count, n * 4);
    VX_TRY(s.status());
    VX_TRY(common(h, io, d));
    return s.finish();
}
}  // extern "C++"

// the query on device arrays: io's pointers and those of `a` are device memory
static vx_status multihit_common(vx_grid* g, vx::TraceIO io, const vx_tlas_multihit_args& a)
{
    vx::TraceMips mips{};
    const uint32_t* prefix = nullptr;
    if (g->g.nvox) {  // (a grid of 0 cells has nothing to build or to walk: every slot is padded)
        VX_TRY(ensure_coarse(g));
        bool pending = false;
        VX_TRY(prefix_launch(g, &pending));  // prim needs the prefix array on the stream, not the count on the host
        prefix = g->wprefix.as<uint32_t>();
        const uint32_t* p16 = nullptr;
        mips = grid_mips(g, &p16);
    }
    VX_TRY(upload_camera(g->camera, g->stream, io));
    // (read-only: a deferred list emission is neither queued nor waited for here)
    vx::launch_multihit(g->g, mips, prefix, io, multi_io(a), g->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_trace_multi_device(const vx_grid* g, const vx_multihit_args* args)
{
    return multihit_entry(g, args, from_grid_args(args), false, false, multihit_common);
}

vx_status vx_trace_multi(const vx_grid* g, const vx_multihit_args* args)
{
    return multihit_entry(g, args, from_grid_args(args), false, true, multihit_common);
}

// vx_trace / vx_octree_trace: t and prim of a host ray buffer through the handle's host-buffer extended query, hits counted on the host
extern "C++" {
template <class Ex>
static vx_status trace_simple(const float* host_rays, uint64_t nrays, float tmin, float tmax, float* host_t, uint32_t* host_prim, uint64_t* num_hits, Ex ex)
{
    if (num_hits) *num_hits = 0;
    if (!nrays) return VX_OK;
    std::vector<float> tbuf;
    float* tdst = host_t;
    if (!tdst) { tbuf.resize(nrays); tdst = tbuf.data(); }
    vx_trace_args a{};
    a.rays = host_rays; a.num_rays = nrays; a.tmin = tmin; a.tmax = tmax; a.t = tdst; a.prim = host_prim;
    VX_TRY(ex(&a));
    if (num_hits) {
        uint64_t n = 0;
        for (uint64_t i = 0; i < nrays; ++i) n += tdst[i] > 0.0f;
        *num_hits = n;
    }
    return VX_OK;
}
}  // extern "C++"

vx_status vx_trace(const vx_grid* gc, const float* host_rays, uint64_t nrays, float tmin, float tmax, float* host_t, uint32_t* host_prim,
                   uint64_t* num_hits)
{
    if (!gc || (nrays && !host_rays)) return fail(VX_ERR_INVALID_ARG, "null argument");
    return trace_simple(host_rays, nrays, tmin, tmax, host_t, host_prim, num_hits, [&](const vx_trace_args* a) { return vx_trace_ex(gc, a); });
}

// ---- octree ---------------------------------------------------------------------------------------------------
// The node array level by level (vx_octree.hip, LEVEL-BY-LEVEL FORM) from o's sorted items into o->nodebuf: breadth-first expansion with one
// host wait per level (the size of the next one), then the pre-order renumbering.  Scratch on the build's Home; the four arrays indexed by
// breadth-first id grow as the levels arrive and keep their contents.
static vx_status octree_nodes_by_level(vx_octree* o, const Home& here, ScanScratch& scan, Mail* mail)
{
    hipStream_t s = here.stream;
    const uint64_t* items = o->items.as<uint64_t>();
    const uint32_t max_items = o->max_items > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)o->max_items;
    DevBuf start{&here}, count{&here}, children{&here}, depth_of{&here}, nchild{&here}, cbase{&here};
    const size_t first = 1024;  // nodes of the first blocks
    VX_HIP(start.ensure(first * 4));
    VX_HIP(count.ensure(first * 4));
    VX_HIP(children.ensure(first * 32));
    VX_HIP(depth_of.ensure(first));
    const uint32_t root[2] = {0u, (uint32_t)o->nitems};
    VX_HIP(hipMemcpyAsync(start.p, &root[0], 4, hipMemcpyHostToDevice, s));
    VX_HIP(hipMemcpyAsync(count.p, &root[1], 4, hipMemcpyHostToDevice, s));
    uint32_t total = 1, level_off = 0, level_n = 1;
    for (uint32_t depth = 0;; ++depth) {
        VX_HIP(nchild.ensure(((size_t)level_n + 1) * 4));
        VX_HIP(cbase.ensure(((size_t)level_n + 2) * 4));
        vx::launch_oct_count(items, start.as<uint32_t>() + level_off, count.as<uint32_t>() + level_off, level_n, depth, o->bits, max_items, nchild.as<uint32_t>(), s);
        VX_TRY(scan.u32(nchild, cbase, level_n, false, &mail->occupied, s));
        uint64_t next_n = 0;
        VX_TRY(mail_total(&mail->occupied, 0, s, "more than 2^32 octree nodes", &next_n));
        const size_t need = (size_t)total + next_n;
        if (need >= 0xFFFFFFFFull) return fail(VX_ERR_HIP, "2^32 - 1 octree nodes or more");
        VX_HIP(start.grow((size_t)total * 4, need * 4));
        VX_HIP(count.grow((size_t)total * 4, need * 4));
        VX_HIP(children.grow((size_t)total * 32, need * 32));
        VX_HIP(depth_of.grow(total, need));
        vx::launch_oct_emit(items, start.as<uint32_t>(), count.as<uint32_t>(), children.as<uint32_t>(), depth_of.as<uint8_t>(), level_off, level_n, depth, o->bits,
                            max_items, cbase.as<uint32_t>(), /*next_off=*/total, s);
        if (next_n == 0) break;
        level_off = total;
        level_n = (uint32_t)next_n;
        total += level_n;
    }
    // pre-order numbering: rank of (start << 8 | depth)
    DevBuf keys{&here}, keys2{&here}, ids{&here}, order{&here}, newidx{&here}, sorttmp{&here};
    const size_t tb = vx::oct_sort_tmp_bytes(total);
    VX_HIP(keys.ensure((size_t)total * 8));
    VX_HIP(keys2.ensure((size_t)total * 8));
    VX_HIP(ids.ensure((size_t)total * 4));
    VX_HIP(order.ensure((size_t)total * 4));
    VX_HIP(newidx.ensure((size_t)total * 4));
    VX_HIP(sorttmp.ensure(tb));
    VX_HIP(o->nodebuf.ensure((size_t)total * sizeof(vx_octree_node)));
    vx::launch_oct_keys(start.as<uint32_t>(), depth_of.as<uint8_t>(), total, keys.as<uint64_t>(), ids.as<uint32_t>(), s);
    VX_HIP(vx::launch_oct_sort(keys.as<uint64_t>(), keys2.as<uint64_t>(), ids.as<uint32_t>(), order.as<uint32_t>(), total, sorttmp.p, tb, s));
    vx::launch_oct_inverse(order.as<uint32_t>(), total, newidx.as<uint32_t>(), s);
    vx::launch_oct_finalize(order.as<uint32_t>(), newidx.as<uint32_t>(), start.as<uint32_t>(), count.as<uint32_t>(), children.as<uint32_t>(), total,
                            o->nodebuf.as<vx_octree_node>(), s);
    VX_HIP(hipStreamSynchronize(s));
    o->nnodes = total;
    return VX_OK;
}

vx_status vx_octree_build(const vx_mesh* mesh_c, float vs, uint64_t max_items, void* stream, vx_octree** out)
{
    if (!mesh_c || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(check_voxel_size(vs));
    vx_mesh* mesh = const_cast<vx_mesh*>(mesh_c);
    VX_TRY(need_device(mesh->device));
    DeviceGuard dg(mesh->device);
    VX_TRY(mesh_to_device(mesh));
    hipStream_t s = (hipStream_t)stream;
    const Home here(mesh->device, s);  // of the build's scratch: it outlives the octree, which a failed build frees on its way out
    Fresh<vx_octree> o(new vx_octree());
    o->device = mesh->device;
    o->stream = s;
    o->vs = vs;
    o->max_items = max_items;
    MailPtr mail;
    DevBuf small{&here}, unsorted{&here}, sorttmp{&here}, ncount{&here}, nbase{&here};
    UnitPipe up{&here};
    VX_HIP(ensure_small(small));
    Small* ds = small.as<Small>();
    VX_HIP(mail_alloc(mail));
    Extent ex;
    VX_TRY(compute_extent(mesh, vs, ds, mail.get(), s, &ex, /*morton_error=*/true));
    for (int a = 0; a < 3; ++a) { o->root_min[a] = ex.mn[a]; o->root_max[a] = ex.mx[a]; o->dim[a] = ex.dim[a]; }
    uint64_t maxDim = ex.dim[0] > ex.dim[1] ? ex.dim[0] : ex.dim[1];
    if (ex.dim[2] > maxDim) maxDim = ex.dim[2];
    if (maxDim == 0) { *out = o.release(); return VX_OK; }  // octTree.hpp:571-574
    o->bits = (uint32_t)std::ceil(std::log2((double)maxDim));  // :577-578
    if (o->bits > 21) return fail(VX_ERR_MORTON_BITS, "We support up to 21 bits per axis (max 2^21 voxels per dimension)!");
    const float root_ext = vs * (float)(1u << o->bits);  // :592
    for (int a = 0; a < 3; ++a) o->root_max[a] = ex.mn[a] + root_ext;
    const uint32_t ntri = (uint32_t)mesh->nt;
    if (ntri == 0) { *out = o.release(); return VX_OK; }  // :696-699 (returns before buildTree)
    vx::GridParams g;
    fill_params(g, ex.mn, vs, ex.dim);
    uint64_t U = 0;
    const bool wide = ex.dim[0] > 65535 || ex.dim[1] > 65535 || ex.dim[2] > 65535;  // the unit kernels also read the extension words
    VX_TRY(up.setup_launch(mesh, g, /*sat a7: octTree.hpp:762*/ 0, 0, ntri, 0, (uint32_t)ex.dim[2], mail.get(), s));
    VX_TRY(up.setup_finish(ntri, mail.get(), s, &U));
    uint64_t hits = 0;
    if (U) {
        VX_HIP(up.umask.ensure((size_t)(U + 1) * 4));
        const uint64_t nUB = (U + 63) / 64;  // hits per block of 64 units from the voxelizer, scanned: the items' positions (as for the Vec grid)
        VX_HIP(up.bhits.ensure((size_t)(nUB + 4) * 4));
        VX_HIP(up.hbase.ensure((size_t)(nUB + 4) * 4));
        VX_HIP(up.scantmp.reserve(nUB, s));  // (ahead of the voxelizer)
        vx::VoxelizeArgs va;
        va.block_hits = up.bhits.as<uint32_t>();
        vx::launch_voxelize(up.view(ntri, wide), g, 0, nullptr, 0, 0, up.umask.as<uint32_t>(), ds->set_calls, s, va);
        VX_TRY(up.scantmp.u32(up.bhits, up.hbase, nUB, false, &mail->hits, s));
        VX_TRY(mail_total(&mail->hits, 0, s, "more than 2^32 octree items", &hits));
    }
    o->nitems = hits;
    if (hits) {
        VX_HIP(unsorted.ensure((size_t)hits * 8));
        VX_HIP(o->items.ensure((size_t)hits * 8));
        vx::launch_emit_units(up.view(ntri, wide), g, up.umask.as<uint32_t>(), up.hbase.as<uint32_t>(), nullptr, unsorted.as<uint64_t>(), s);
        const size_t tb = vx::sort_tmp_bytes(hits);
        VX_HIP(sorttmp.ensure(tb));
        // octTree.hpp:363; the sort ping-pongs between the two buffers: whichever holds the result becomes the octree's item list
        if (vx::launch_sort_u64(unsorted.as<uint64_t>(), o->items.as<uint64_t>(), hits, o->bits ? (int)(3 * o->bits) : 1, sorttmp.p, tb, s) == 0)
            std::swap(unsorted, o->items);
    }
    // node array (octTree.hpp:319-358, :371)
    if (hits && max_items <= vx::kOctDirectMaxItems) {
        // direct form (vx_octree.hip): nodes starting at every item position -> scan -> start / count / links; one wait for the node count
        const uint32_t ni = (uint32_t)hits;
        VX_HIP(ncount.ensure((size_t)ni + 16));
        VX_HIP(nbase.ensure(((size_t)ni + 2) * 4));
        VX_HIP(up.scantmp.reserve(ni, s));  // (ahead of the depth kernel)
        vx::launch_oct_depths(o->items.as<uint64_t>(), ni, o->bits, (uint32_t)max_items, ncount.as<uint8_t>(), s);
        VX_TRY(up.scantmp.u8(ncount, nbase, ni, &mail->occupied, s));
        uint64_t nn = 0;
        VX_TRY(mail_total(&mail->occupied, 0, s, "more than 2^32 octree nodes", &nn));
        if (nn == 0) return fail(VX_ERR_CAPACITY, "more than 2^32 octree nodes");
        VX_HIP(o->nodebuf.ensure((size_t)nn * sizeof(vx_octree_node)));
        VX_HIP(hipMemsetAsync(o->nodebuf.p, 0xFF, (size_t)nn * sizeof(vx_octree_node), s));  // children = 0xFFFFFFFF (none)
        vx::launch_oct_nodes(o->items.as<uint64_t>(), ni, o->bits, nbase.as<uint32_t>(), o->nodebuf.as<vx_octree_node>(), s);
        VX_HIP(hipStreamSynchronize(s));
        o->nnodes = nn;
    } else {
        VX_TRY(octree_nodes_by_level(o.get(), here, up.scantmp, mail.get()));  // (any max_items; also the empty item list's lone root)
    }
    *out = o.release();
    return VX_OK;
}

uint64_t vx_octree_num_items(const vx_octree* o) { return o ? o->nitems : 0; }
uint64_t vx_octree_num_nodes(const vx_octree* o) { return o ? o->nnodes : 0; }
uint64_t vx_octree_bytes(const vx_octree* o) { return o ? o->nitems * 8 + o->nnodes * 40 : 0; }

vx_status vx_octree_items(const vx_octree* o, uint64_t* host, uint64_t cap)
{
    if (!o || (!host && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (cap < o->nitems) return fail(VX_ERR_CAPACITY, "item buffer too small");
    if (!o->nitems) return VX_OK;
    DeviceGuard dg(o->device);
    VX_HIP(hipMemcpyAsync(host, o->items.p, (size_t)o->nitems * 8, hipMemcpyDeviceToHost, o->stream));
    VX_HIP(hipStreamSynchronize(o->stream));
    return VX_OK;
}

vx_status vx_octree_nodes(const vx_octree* o, vx_octree_node* host, uint64_t cap)
{
    if (!o || (!host && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (cap < o->nnodes) return fail(VX_ERR_CAPACITY, "node buffer too small");
    if (!o->nnodes) return VX_OK;
    DeviceGuard dg(o->device);
    VX_HIP(hipMemcpyAsync(host, o->nodebuf.as<vx_octree_node>(), (size_t)o->nnodes * sizeof(vx_octree_node), hipMemcpyDeviceToHost, o->stream));
    VX_HIP(hipStreamSynchronize(o->stream));
    return VX_OK;
}

vx_status vx_octree_root_bounds(const vx_octree* o, float mn[3], float mx[3])
{
    if (!o || !mn || !mx) return fail(VX_ERR_INVALID_ARG, "null argument");
    std::memcpy(mn, o->root_min, 12);
    std::memcpy(mx, o->root_max, 12);
    return VX_OK;
}

vx_status vx_octree_aabbs_device(const vx_octree* o, vx_aabb* dev_out, uint64_t cap, uint64_t* count)
{
    if (!o) return fail(VX_ERR_INVALID_ARG, "null argument");
    const uint64_t n = o->nnodes == 0 ? 0 : o->nitems;  // octTree.hpp:505-507
    if (count) *count = n;
    const uint64_t m = cap < n ? cap : n;
    if (!m || !dev_out) return VX_OK;
    DeviceGuard dg(o->device);
    vx::launch_emit_morton_aabbs(o->items.as<uint64_t>(), m, o->root_min, o->vs, dev_out, o->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_octree_aabbs(const vx_octree* o, vx_aabb* host_out, uint64_t cap, uint64_t* count)
{
    if (!o) return fail(VX_ERR_INVALID_ARG, "null argument");
    const uint64_t n = o->nnodes == 0 ? 0 : o->nitems;
    if (count) *count = n;
    const uint64_t m = cap < n ? cap : n;
    if (!m || !host_out) return VX_OK;
    DeviceGuard dg(o->device);
    Staging s(*o);
    vx_aabb* list = s.out(host_out, (size_t)m * sizeof(vx_aabb));
    VX_TRY(s.status());
    vx::launch_emit_morton_aabbs(o->items.as<uint64_t>(), m, o->root_min, o->vs, list, o->stream);
    return s.finish();
}

// ---- rays on the octree: the grid trace's contract over the vx_octree_aabbs list (vx_octrace.hip) ----------------------------------
// the traversal of the octree's current build, queued on st: the octree's own stream, or a frame's (render_enqueue)
static void octree_launch(const vx_octree* o, const vx::TraceIO& io, hipStream_t st)
{
    const uint64_t nitems = o->nnodes == 0 ? 0 : o->nitems;  // the list vx_octree_aabbs returns
    vx::launch_octree_trace(o->nodebuf.as<vx_octree_node>(), o->items.as<uint64_t>(), nitems, o->bits, o->root_min, o->vs, io, st);
}

static vx_status octree_trace_common(vx_octree* o, vx::TraceIO io, float*, uint32_t*)
{
    if (!io.nrays) return VX_OK;
    VX_TRY(upload_camera(o->camera, o->stream, io));
    octree_launch(o, io, o->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_octree_trace_ex_device(const vx_octree* o, const vx_trace_args* args)
{
    return trace_entry(o, args, from_trace_args(args), false, octree_trace_common);
}

vx_status vx_octree_trace_ex(const vx_octree* o, const vx_trace_args* args)
{
    return trace_entry(o, args, from_trace_args(args), true, octree_trace_common);
}

vx_status vx_octree_trace(const vx_octree* oc, const float* host_rays, uint64_t nrays, float tmin, float tmax, float* host_t, uint32_t* host_prim,
                          uint64_t* num_hits)
{
    if (!oc || (nrays && !host_rays)) return fail(VX_ERR_INVALID_ARG, "null argument");
    return trace_simple(host_rays, nrays, tmin, tmax, host_t, host_prim, num_hits, [&](const vx_trace_args* a) { return vx_octree_trace_ex(oc, a); });
}

// ---- multi-hit query on the octree (vx_octmulti.hip): vx_trace_multi's contract over the runs of equal codes of the list
static vx_status octree_multihit_common(vx_octree* o, vx::TraceIO io, const vx_tlas_multihit_args& a)
{
    VX_TRY(upload_camera(o->camera, o->stream, io));
    const uint64_t nitems = o->nnodes == 0 ? 0 : o->nitems;  // the list vx_octree_aabbs returns
    vx::launch_octree_multihit(o->nodebuf.as<vx_octree_node>(), o->items.as<uint64_t>(), nitems, o->bits, o->root_min, o->vs, io, multi_io(a), o->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_octree_trace_multi_device(const vx_octree* o, const vx_multihit_args* args)
{
    return multihit_entry(o, args, from_grid_args(args), false, false, octree_multihit_common);
}

vx_status vx_octree_trace_multi(const vx_octree* o, const vx_multihit_args* args)
{
    return multihit_entry(o, args, from_grid_args(args), false, true, octree_multihit_common);
}

void vx_octree_free(vx_octree* o) { handle_free(o); }

// ---- triangle BVH: the reference's triangle BLAS (hello_vulkan.cpp:596-635) under raytrace.rchit (vx_bvh.hip) -------------------------
struct vx_bvh : Home {
    uint32_t max_leaf = VX_BVH_DEFAULT_LEAF;
    uint64_t ntri = 0, nnodes = 0;
    uint32_t height = 0;
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};
    float coord_max = 0.f;  // the largest |coordinate| below the root and ...
    float extent = 0.f;     // ... the root box's largest side: the traversal's box widening is relative to these
    uint32_t nill = 0;      // ill-conditioned triangles (vx_bvh.hip): tested by every ray
    DevBuf nodes{this}, tris{this}, ill{this};  // the BVH itself
    // build scratch, kept for rebuilds
    DevBuf keys_a{this}, keys_b{this}, sorttmp{this}, child{this}, parent{this}, range{this}, arrived{this}, kbox{this}, alive{this}, newidx{this}, scantmp{this}, small{this},
        camera{this};
};

namespace {
struct BvhSmall {
    uint32_t box6[6];
    uint32_t err;
    uint32_t nill;
    unsigned long long total;
};

vx_status bvh_build_impl(vx_mesh* mesh, vx_bvh* b)
{
    VX_TRY(need_device(mesh->device));
    if (mesh->device != b->device) return fail(VX_ERR_INVALID_ARG, "mesh and BVH live on different devices");
    DeviceGuard dg(b->device);
    VX_TRY(mesh_to_device(mesh));
    hipStream_t s = b->stream;
    const uint64_t n = mesh->nt;
    if (n >= 0x7FFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^31 triangles");
    b->ntri = 0; b->nnodes = 0; b->height = 0; b->coord_max = 0.f; b->extent = 0.f; b->nill = 0;
    for (int a = 0; a < 3; ++a) b->root_min[a] = b->root_max[a] = 0.f;
    if (n == 0) return VX_OK;
    const uint32_t nt = (uint32_t)n, nall = 2 * nt - 1;
    VX_HIP(b->small.ensure(sizeof(BvhSmall)));
    VX_HIP(b->keys_a.ensure(n * 8));
    VX_HIP(b->keys_b.ensure(n * 8));
    const size_t tb = vx::sort_tmp_bytes(n);
    VX_HIP(b->sorttmp.ensure(tb));
    VX_HIP(b->child.ensure((size_t)n * 8));
    VX_HIP(b->range.ensure((size_t)n * 8));
    VX_HIP(b->parent.ensure((size_t)nall * 4));
    VX_HIP(b->arrived.ensure((size_t)n * 4));
    VX_HIP(b->kbox.ensure((size_t)nall * 32));
    VX_HIP(b->alive.ensure(((size_t)nall + 16) * 4));
    VX_HIP(b->newidx.ensure(((size_t)nall + 16) * 4));
    VX_HIP(b->scantmp.ensure(vx::scan_tmp_bytes(nall)));
    VX_HIP(b->nodes.ensure((size_t)nall * 32));
    VX_HIP(b->tris.ensure((size_t)n * 48));
    VX_HIP(b->ill.ensure((size_t)n * 4));
    BvhSmall* ds = b->small.as<BvhSmall>();
    VX_HIP(hipMemsetAsync(ds->box6, 0xFF, 12, s));  // min: the largest ordered value
    VX_HIP(hipMemsetAsync(ds->box6 + 3, 0, 20, s)); // max: the smallest; err = nill = 0
    vx::launch_bvh_prep(mesh->dv, mesh->di, mesh->nv, nt, ds->box6, &ds->err, b->keys_a.as<uint64_t>(), s);
    const uint64_t* keys =
        vx::launch_sort_u64(b->keys_a.as<uint64_t>(), b->keys_b.as<uint64_t>(), n, 62, b->sorttmp.p, tb, s) == 0 ? b->keys_a.as<uint64_t>() : b->keys_b.as<uint64_t>();
    vx::launch_bvh_tree(mesh->dv, mesh->di, mesh->nv, nt, keys, b->max_leaf, b->child.as<uint32_t>(), b->parent.as<uint32_t>(), b->range.as<uint32_t>(),
                        b->arrived.as<uint32_t>(), b->kbox.as<float>(), b->tris.as<float>(), b->alive.as<uint32_t>(), b->ill.as<uint32_t>(), &ds->nill, s);
    vx::launch_scan_u32(b->alive.as<uint32_t>(), b->newidx.as<uint32_t>(), nall, false, b->scantmp.p, &ds->total, s);
    vx::launch_bvh_emit(nt, b->alive.as<uint32_t>(), b->newidx.as<uint32_t>(), b->child.as<uint32_t>(), b->range.as<uint32_t>(), b->max_leaf,
                        b->kbox.as<float>(), b->nodes.as<float>(), s);
    VX_HIP(hipGetLastError());
    float root[8];
    uint32_t nn = 0, err = 0, nill = 0;
    VX_HIP(hipMemcpyAsync(root, b->kbox.p, 32, hipMemcpyDeviceToHost, s));  // the radix tree's root (unified index 0) and its height
    VX_HIP(hipMemcpyAsync(&nn, b->newidx.as<uint32_t>() + nall, 4, hipMemcpyDeviceToHost, s));
    VX_HIP(hipMemcpyAsync(&err, &ds->err, 4, hipMemcpyDeviceToHost, s));
    VX_HIP(hipMemcpyAsync(&nill, &ds->nill, 4, hipMemcpyDeviceToHost, s));
    VX_HIP(hipStreamSynchronize(s));
    if (err & 1u) return fail(VX_ERR_INVALID_ARG, "triangle index out of range");
    if (err & 2u) return fail(VX_ERR_INVALID_ARG, "a triangle has a non-finite vertex coordinate (NaN or Inf)");
    std::memcpy(&b->height, &root[3], 4);
    for (int a = 0; a < 3; ++a) {
        b->root_min[a] = root[a];
        b->root_max[a] = root[4 + a];
        b->coord_max = std::max(b->coord_max, std::max(std::fabs(root[a]), std::fabs(root[4 + a])));
        b->extent = std::max(b->extent, root[4 + a] - root[a]);
    }
    // every referenced vertex is finite (k_bvh_prep), so coord_max is; max - min of vertices beyond +-FLT_MAX/2 overflows: the widening
    // then takes the largest finite extent (2^-10 of it stays finite), not 0, which would leave 2^-18 of coord_max alone
    if (!std::isfinite(b->extent)) b->extent = std::numeric_limits<float>::max();
    b->ntri = n;
    b->nnodes = nn;
    b->nill = nill;
    return VX_OK;
}
}  // namespace

vx_status vx_bvh_build(const vx_mesh* mesh_c, uint32_t max_leaf, void* stream, vx_bvh** out)
{
    if (!mesh_c || !out) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (max_leaf >= 0x80000000u) return fail(VX_ERR_INVALID_ARG, "max_leaf_triangles must be below 2^31");
    vx_mesh* mesh = const_cast<vx_mesh*>(mesh_c);
    VX_TRY(need_device(mesh->device));
    Fresh<vx_bvh> b(new vx_bvh());
    b->device = mesh->device;
    b->stream = (hipStream_t)stream;
    b->max_leaf = max_leaf ? max_leaf : VX_BVH_DEFAULT_LEAF;
    VX_TRY(bvh_build_impl(mesh, b.get()));
    *out = b.release();
    return VX_OK;
}

vx_status vx_bvh_build_into(const vx_mesh* mesh_c, vx_bvh* b)
{
    if (!mesh_c || !b) return fail(VX_ERR_INVALID_ARG, "null argument");
    return bvh_build_impl(const_cast<vx_mesh*>(mesh_c), b);
}

uint64_t vx_bvh_num_triangles(const vx_bvh* b) { return b ? b->ntri : 0; }
uint64_t vx_bvh_num_nodes(const vx_bvh* b) { return b ? b->nnodes : 0; }
uint64_t vx_bvh_bytes(const vx_bvh* b) { return b ? b->nnodes * 32 + b->ntri * 48 : 0; }
uint32_t vx_bvh_height(const vx_bvh* b) { return b ? b->height : 0; }
uint64_t vx_bvh_num_ill_conditioned(const vx_bvh* b) { return b ? b->nill : 0; }
const void* vx_bvh_nodes_device(const vx_bvh* b) { return b ? b->nodes.p : nullptr; }

vx_status vx_bvh_root_bounds(const vx_bvh* b, float mn[3], float mx[3])
{
    if (!b || !mn || !mx) return fail(VX_ERR_INVALID_ARG, "null argument");
    std::memcpy(mn, b->root_min, 12);
    std::memcpy(mx, b->root_max, 12);
    return VX_OK;
}

vx_status vx_bvh_nodes(const vx_bvh* b, void* host, uint64_t cap, uint64_t* bytes)
{
    if (!b || (!host && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    const uint64_t nb = b->nnodes * sizeof(vx_bvh_node);
    if (bytes) *bytes = nb;
    if (!cap || !nb) return VX_OK;
    if (cap < nb) return fail(VX_ERR_CAPACITY, "node buffer too small");
    DeviceGuard dg(b->device);
    VX_HIP(hipMemcpyAsync(host, b->nodes.p, (size_t)nb, hipMemcpyDeviceToHost, b->stream));
    VX_HIP(hipStreamSynchronize(b->stream));
    return VX_OK;
}

vx_status vx_bvh_leaf_triangles(const vx_bvh* b, uint32_t* host, uint64_t cap)
{
    if (!b || (!host && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (cap < b->ntri) return fail(VX_ERR_CAPACITY, "triangle buffer too small");
    if (!b->ntri) return VX_OK;
    DeviceGuard dg(b->device);
    std::vector<float> t((size_t)b->ntri * 12);  // the triangle copies: the index rides in the w of the first vertex
    VX_HIP(hipMemcpyAsync(t.data(), b->tris.p, t.size() * 4, hipMemcpyDeviceToHost, b->stream));
    VX_HIP(hipStreamSynchronize(b->stream));
    for (uint64_t i = 0; i < b->ntri; ++i) std::memcpy(&host[i], &t[(size_t)i * 12 + 3], 4);
    return VX_OK;
}

// the traversal of the BVH's current build, queued on st: the BVH's own stream, or a frame's (render_enqueue)
static void bvh_launch(const vx_bvh* b, const vx::TraceIO& io, float* bary, hipStream_t st)
{
    vx::launch_bvh_trace(b->ntri ? b->nodes.as<float>() : nullptr, b->tris.as<float>(), b->ill.as<uint32_t>(), b->nill, (uint32_t)b->ntri, b->height, b->extent, b->coord_max, io, bary,
                         st);
}

static vx_status bvh_trace_common(vx_bvh* b, vx::TraceIO io, float* bary, uint32_t*)
{
    if (!io.nrays) return VX_OK;
    VX_TRY(upload_camera(b->camera, b->stream, io));
    bvh_launch(b, io, bary, b->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_bvh_trace_ex_device(const vx_bvh* b, const vx_bvh_trace_args* args)
{
    return trace_entry(b, args, from_bvh_trace_args(args), false, bvh_trace_common);
}

vx_status vx_bvh_trace_ex(const vx_bvh* b, const vx_bvh_trace_args* args)
{
    return trace_entry(b, args, from_bvh_trace_args(args), true, bvh_trace_common);
}

vx_status vx_bvh_trace(const vx_bvh* bc, const float* host_rays, uint64_t nrays, float tmin, float tmax, float* host_t, uint32_t* host_prim,
                       uint64_t* num_hits)
{
    if (!bc || (nrays && !host_rays)) return fail(VX_ERR_INVALID_ARG, "null argument");
    return trace_simple(host_rays, nrays, tmin, tmax, host_t, host_prim, num_hits, [&](const vx_trace_args* a) {
        vx_bvh_trace_args ba{};
        ba.base = *a;
        return vx_bvh_trace_ex(bc, &ba);
    });
}

// ---- multi-hit queries on the mesh (vx_meshmulti.hip): the argument form, checks and staging of vx_trace_multi above
// the query on device arrays: io's pointers and those of `a` are device memory
static vx_status bvh_multihit_common(vx_bvh* b, vx::TraceIO io, const vx_tlas_multihit_args& a)
{
    VX_TRY(upload_camera(b->camera, b->stream, io));
    vx::launch_bvh_multihit(b->ntri ? b->nodes.as<float>() : nullptr, b->tris.as<float>(), b->ill.as<uint32_t>(), b->nill, (uint32_t)b->ntri, b->height,
                            b->extent, b->coord_max, io, multi_io(a), b->stream);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

vx_status vx_bvh_trace_multi_device(const vx_bvh* b, const vx_bvh_multihit_args* args)
{
    return multihit_entry(b, args, from_bvh_args(args), false, false, bvh_multihit_common);
}

vx_status vx_bvh_trace_multi(const vx_bvh* b, const vx_bvh_multihit_args* args)
{
    return multihit_entry(b, args, from_bvh_args(args), false, true, bvh_multihit_common);
}

void vx_bvh_free(vx_bvh* b) { handle_free(b); }

// ---- instanced scenes: the reference's TLAS (createTopLevelAS, hello_vulkan.cpp:760-790) over vx_bvh BLAS (vx_tlas.hip) --------------
struct vx_tlas : Home {
    std::vector<vx_bvh*> blas;            // borrowed
    std::vector<vx::TlasBlas> tab;        // the table as last written to the device
    uint64_t n = 0;
    uint32_t levels = 1;                  // LDS stack entries of k_tlas_trace
    DevBuf dinst{this}, xf{this}, w2o{this}, iblas{this}, ibox{this}, keys_a{this}, keys_b{this}, sorttmp{this}, child{this}, parent{this}, range{this}, arrived{this},
        nodes{this}, hgt{this}, small{this}, dtab{this}, camera{this};
    // host staging of vx_tlas_update: two pinned buffers used in turn, so that an update waits (on the host) only for the copy out of
    // the buffer it reuses, the one of the update before the previous one
    PinnedBuf pinned[2];
    bool staged[2] = {false, false};      // ev_staged[k] marks the end of the last copy out of pinned[k]
    int stage = 0;                        // the buffer the next host update fills
    // (behind the DevBufs: the events and pinned blocks are destroyed ahead of the device blocks that the copies they order fill)
    Event ev_src, ev_end, ev_staged[2];   // created by vx_tlas_build
};

namespace {
vx::TlasDev tlas_dev(const vx_tlas* t)
{
    vx::TlasDev d;
    d.nodes = t->nodes.as<float>();
    d.w2o = t->w2o.as<float>();
    d.xf = t->xf.as<float>();
    d.iblas = t->iblas.as<uint32_t>();
    d.tab = t->dtab.as<vx::TlasBlas>();
    d.small = t->small.as<uint32_t>();
    d.ninst = (uint32_t)t->n;
    d.levels = t->levels;
    return d;
}

// the BLAS streams wait for / are waited on by the TLAS's stream
vx_status tlas_wait_blas(vx_tlas* t)
{
    for (vx_bvh* b : t->blas) {
        if (b->stream == t->stream) continue;
        VX_HIP(hipEventRecord(t->ev_src, b->stream));
        VX_HIP(hipStreamWaitEvent(t->stream, t->ev_src, 0));
    }
    return VX_OK;
}
vx_status tlas_fence_blas(vx_tlas* t)
{
    VX_HIP(hipEventRecord(t->ev_end, t->stream));
    for (vx_bvh* b : t->blas)
        if (b->stream != t->stream) VX_HIP(hipStreamWaitEvent(b->stream, t->ev_end, 0));
    return VX_OK;
}

vx_status tlas_check_host(const vx_instance* in, uint64_t n, uint32_t nb)
{
    if (n && !in) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (n >= 0x7FFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^31 instances");
    for (uint64_t i = 0; i < n; ++i) {
        if (in[i].blas >= nb) return fail(VX_ERR_INVALID_ARG, "instance " + std::to_string(i) + ": blas index out of range");
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(in[i].transform[k])) return fail(VX_ERR_INVALID_ARG, "instance " + std::to_string(i) + ": non-finite transform");
    }
    return VX_OK;
}

// rebuild from `in` (device pointer, n instances) on t->stream: no host synchronisation, no copy
vx_status tlas_build_impl(vx_tlas* t, const vx_instance* in, uint64_t n)
{
    DeviceGuard dg(t->device);
    hipStream_t s = t->stream;
    VX_TRY(tlas_wait_blas(t));
    // the BLAS table, re-read from the handles; written to the device (from kernel arguments) only when it changed
    std::vector<vx::TlasBlas> tab(t->blas.size());
    uint32_t hmax = 0;
    for (size_t k = 0; k < t->blas.size(); ++k) {
        const vx_bvh* b = t->blas[k];
        vx::TlasBlas& e = tab[k];
        std::memset(&e, 0, sizeof(e));
        e.nodes = b->ntri ? b->nodes.as<float>() : nullptr;
        e.tris = b->tris.as<float>();
        e.ill = b->ill.as<uint32_t>();
        e.nill = b->ntri ? b->nill : 0;
        e.ntri = (uint32_t)b->ntri;
        e.pad = vx::bvh_pad(b->extent, b->coord_max);
        for (int a = 0; a < 3; ++a) { e.rmin[a] = b->root_min[a]; e.rmax[a] = b->root_max[a]; }
        e.height = b->height;
        hmax = std::max(hmax, b->ntri ? b->height : 0u);
    }
    if (!tab.empty()) {
        VX_HIP(t->dtab.ensure(tab.size() * sizeof(vx::TlasBlas)));
        if (t->dtab.fresh || tab.size() != t->tab.size() || std::memcmp(tab.data(), t->tab.data(), tab.size() * sizeof(vx::TlasBlas)) != 0) {
            vx::launch_tlas_table(tab.data(), (uint32_t)tab.size(), t->dtab.as<vx::TlasBlas>(), s);
            t->dtab.fresh = false;
            t->tab = tab;
        }
    }
    t->n = n;
    t->levels = std::max(1u, vx::tlas_height_bound(n) + hmax);
    if (n == 0) return VX_OK;
    const uint32_t nn = (uint32_t)n, nall = 2 * nn - 1;
    VX_HIP(t->xf.ensure((size_t)n * 48));
    VX_HIP(t->w2o.ensure((size_t)n * 48));
    VX_HIP(t->iblas.ensure((size_t)n * 4));
    VX_HIP(t->ibox.ensure((size_t)n * 32));
    VX_HIP(t->keys_a.ensure((size_t)n * 8));
    VX_HIP(t->keys_b.ensure((size_t)n * 8));
    const size_t tb = vx::sort_tmp_bytes(n);
    VX_HIP(t->sorttmp.ensure(tb));
    VX_HIP(t->child.ensure((size_t)n * 8));
    VX_HIP(t->range.ensure((size_t)n * 8));
    VX_HIP(t->parent.ensure((size_t)nall * 4));
    VX_HIP(t->arrived.ensure((size_t)n * 4));
    VX_HIP(t->nodes.ensure((size_t)nall * 32));
    VX_HIP(t->hgt.ensure((size_t)nall * 4));
    VX_HIP(t->small.ensure(8 * 4));
    uint32_t* sm = t->small.as<uint32_t>();
    VX_HIP(hipMemsetAsync(sm, 0xFF, 12, s));     // box min: the largest ordered value
    VX_HIP(hipMemsetAsync(sm + 3, 0, 20, s));    // box max, the condition number, the height
    vx::launch_tlas_prep(in, nn, t->dtab.as<vx::TlasBlas>(), (uint32_t)t->blas.size(), t->xf.as<float>(), t->w2o.as<float>(), t->iblas.as<uint32_t>(),
                         t->ibox.as<float>(), sm, t->keys_a.as<uint64_t>(), s);
    const uint64_t* keys =
        vx::launch_sort_u64(t->keys_a.as<uint64_t>(), t->keys_b.as<uint64_t>(), n, 62, t->sorttmp.p, tb, s) == 0 ? t->keys_a.as<uint64_t>() : t->keys_b.as<uint64_t>();
    vx::launch_tlas_tree(nn, keys, t->ibox.as<float>(), t->child.as<uint32_t>(), t->parent.as<uint32_t>(), t->range.as<uint32_t>(), t->arrived.as<uint32_t>(),
                         t->nodes.as<float>(), t->hgt.as<uint32_t>(), sm, s);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// host instances: staged through the TLAS's pinned buffer (free for the caller on return), then the device build
vx_status tlas_update_host(vx_tlas* t, const vx_instance* in, uint64_t n)
{
    VX_TRY(tlas_check_host(in, n, (uint32_t)t->blas.size()));
    DeviceGuard dg(t->device);
    if (n) {
        const int k = t->stage;
        if (t->staged[k]) { VX_HIP(hipEventSynchronize(t->ev_staged[k])); t->staged[k] = false; }  // the copy out of this buffer is done
        VX_HIP(t->pinned[k].ensure((size_t)n * sizeof(vx_instance)));
        std::memcpy(t->pinned[k].p, in, (size_t)n * sizeof(vx_instance));
        VX_HIP(t->dinst.ensure((size_t)n * sizeof(vx_instance)));
        VX_HIP(hipMemcpyAsync(t->dinst.p, t->pinned[k].p, (size_t)n * sizeof(vx_instance), hipMemcpyHostToDevice, t->stream));
        VX_HIP(hipEventRecord(t->ev_staged[k], t->stream));
        t->staged[k] = true;
        t->stage = 1 - k;
    }
    return tlas_build_impl(t, t->dinst.as<vx_instance>(), n);
}

vx_status tlas_trace_common(vx_tlas* t, vx::TraceIO io, float* bary, uint32_t* inst)
{
    if (!io.nrays) return VX_OK;
    VX_TRY(upload_camera(t->camera, t->stream, io));
    VX_TRY(tlas_wait_blas(t));
    vx::launch_tlas_trace(tlas_dev(t), io, bary, inst, t->stream);
    VX_HIP(hipGetLastError());
    return tlas_fence_blas(t);
}

}  // namespace

vx_status vx_tlas_build(const vx_bvh* const* blas, uint32_t num_blas, const vx_instance* host_instances, uint64_t num_instances, void* stream,
                        vx_tlas** out)
{
    if (!out || (num_blas && !blas)) return fail(VX_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    for (uint32_t k = 0; k < num_blas; ++k)
        if (!blas[k]) return fail(VX_ERR_INVALID_ARG, "null BLAS handle");
    if (num_instances && !num_blas) return fail(VX_ERR_INVALID_ARG, "instances need at least one BLAS");
    VX_TRY(tlas_check_host(host_instances, num_instances, num_blas));
    const int dev = num_blas ? blas[0]->device : g_device;
    VX_TRY(need_device(dev));
    for (uint32_t k = 0; k < num_blas; ++k)
        if (blas[k]->device != dev) return fail(VX_ERR_INVALID_ARG, "the BLAS handles live on different devices");
    Fresh<vx_tlas> t(new vx_tlas());
    t->device = dev;
    t->stream = (hipStream_t)stream;
    for (uint32_t k = 0; k < num_blas; ++k) t->blas.push_back(const_cast<vx_bvh*>(blas[k]));
    DeviceGuard dg(t->device);
    hipError_t e = hipSuccess;
    for (Event* ev : {&t->ev_src, &t->ev_end, &t->ev_staged[0], &t->ev_staged[1]})
        if (e == hipSuccess) e = ev->create();
    if (e != hipSuccess) return fail(VX_ERR_HIP, std::string("vx_tlas_build: ") + hipGetErrorString(e));
    VX_TRY(tlas_update_host(t.get(), host_instances, num_instances));
    e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return fail(VX_ERR_HIP, hipGetErrorString(e));
    *out = t.release();
    return VX_OK;
}

vx_status vx_tlas_update(vx_tlas* t, const vx_instance* host_instances, uint64_t num_instances)
{
    if (!t) return fail(VX_ERR_INVALID_ARG, "null argument");
    return tlas_update_host(t, host_instances, num_instances);
}

vx_status vx_tlas_update_device(vx_tlas* t, const vx_instance* dev_instances, uint64_t num_instances)
{
    if (!t || (num_instances && !dev_instances)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (num_instances >= 0x7FFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^31 instances");
    return tlas_build_impl(t, dev_instances, num_instances);
}

uint64_t vx_tlas_num_instances(const vx_tlas* t) { return t ? t->n : 0; }
uint64_t vx_tlas_num_nodes(const vx_tlas* t) { return t && t->n ? 2 * t->n - 1 : 0; }
uint64_t vx_tlas_bytes(const vx_tlas* t) { return t ? vx_tlas_num_nodes(t) * 32 + t->n * 100 : 0; }

uint32_t vx_tlas_height(const vx_tlas* t)
{
    if (!t || !t->n) return 0;
    DeviceGuard dg(t->device);
    uint32_t h = 0;
    if (hipMemcpyAsync(&h, t->small.as<uint32_t>() + 7, 4, hipMemcpyDeviceToHost, t->stream) != hipSuccess) return 0;
    if (hipStreamSynchronize(t->stream) != hipSuccess) return 0;
    return h;
}

vx_status vx_tlas_world_to_object(const vx_tlas* t, float* host, uint64_t cap)
{
    if (!t || (!host && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (cap < t->n * 12) return fail(VX_ERR_CAPACITY, "matrix buffer too small (12 floats per instance)");
    if (!t->n) return VX_OK;
    DeviceGuard dg(t->device);
    VX_HIP(hipMemcpyAsync(host, t->w2o.p, (size_t)t->n * 48, hipMemcpyDeviceToHost, t->stream));
    VX_HIP(hipStreamSynchronize(t->stream));
    return VX_OK;
}

vx_status vx_tlas_nodes(const vx_tlas* t, void* host, uint64_t cap, uint64_t* bytes)
{
    if (!t || (!host && cap)) return fail(VX_ERR_INVALID_ARG, "null argument");
    const uint64_t nb = vx_tlas_num_nodes(t) * sizeof(vx_bvh_node);
    if (bytes) *bytes = nb;
    if (!cap || !nb) return VX_OK;
    if (cap < nb) return fail(VX_ERR_CAPACITY, "node buffer too small");
    DeviceGuard dg(t->device);
    VX_HIP(hipMemcpyAsync(host, t->nodes.p, (size_t)nb, hipMemcpyDeviceToHost, t->stream));
    VX_HIP(hipStreamSynchronize(t->stream));
    return VX_OK;
}

vx_status vx_tlas_trace_ex_device(const vx_tlas* t, const vx_tlas_trace_args* args)
{
    return trace_entry(t, args, args ? *args : vx_tlas_trace_args{}, false, tlas_trace_common);
}

vx_status vx_tlas_trace_ex(const vx_tlas* t, const vx_tlas_trace_args* args)
{
    return trace_entry(t, args, args ? *args : vx_tlas_trace_args{}, true, tlas_trace_common);
}

vx_status vx_tlas_trace(const vx_tlas* tc, const float* host_rays, uint64_t nrays, float tmin, float tmax, float* host_t, uint32_t* host_instance,
                        uint32_t* host_prim, uint64_t* num_hits)
{
    if (!tc || (nrays && !host_rays)) return fail(VX_ERR_INVALID_ARG, "null argument");
    return trace_simple(host_rays, nrays, tmin, tmax, host_t, host_prim, num_hits, [&](const vx_trace_args* a) {
        vx_tlas_trace_args ta{};
        ta.base = *a;
        ta.instance = host_instance;
        return vx_tlas_trace_ex(tc, &ta);
    });
}

// the multi-hit query on device arrays, under the stream rules of tlas_trace_common
static vx_status tlas_multihit_common(vx_tlas* t, vx::TraceIO io, const vx_tlas_multihit_args& a)
{
    VX_TRY(upload_camera(t->camera, t->stream, io));
    VX_TRY(tlas_wait_blas(t));
    vx::launch_tlas_multihit(tlas_dev(t), io, multi_io(a), t->stream);
    VX_HIP(hipGetLastError());
    return tlas_fence_blas(t);
}

vx_status vx_tlas_trace_multi_device(const vx_tlas* t, const vx_tlas_multihit_args* a)
{
    return multihit_entry(t, a, a ? *a : vx_tlas_multihit_args{}, true, false, tlas_multihit_common);
}

vx_status vx_tlas_trace_multi(const vx_tlas* t, const vx_tlas_multihit_args* a)
{
    return multihit_entry(t, a, a ? *a : vx_tlas_multihit_args{}, true, true, tlas_multihit_common);
}

void vx_tlas_free(vx_tlas* t) { handle_free(t); }

// ---- frames: the reference's per-frame raytrace dispatch as one asynchronous sequence on the scene's stream (vx_render.hip) ------------
// camera block -> primary traversals (voxels, mesh) -> launch_render_shadow_rays -> shadow traversals (voxels, mesh) -> launch_render_shade,
// each of the two one of four kernels (k_render_shadow_rays / k_render_shade, _tlas, _attr, _attr_tlas).  The scene owns every buffer the
// sequence touches, the walk's work counters included, so a frame never shares scratch with a trace the user runs on a source's own stream.
struct vx_render_scene : Home {
    vx_grid* grid = nullptr;
    vx_octree* octree = nullptr;
    vx_bvh* bvh = nullptr;
    vx_tlas* tlas = nullptr;              // instanced scenes (vx_render_create_tlas)
    std::vector<vx_mesh*> meshes;         // the BVH's mesh, or one per BLAS of the TLAS; none without triangles
    std::vector<vx::InstMesh> imeshes;    // a record per mesh (render_upload_materials); instanced scenes read the table from `imesh`
    DevBuf camera{this}, counters{this}, idxtmp{this}, vt{this}, vprim{this}, vnrm{this}, mt{this}, mprim{this}, mnrm{this}, mbary{this}, srays{this}, sdist{this},
        stmax{this}, sv{this}, sm{this}, vmat{this}, mmat{this}, mids{this}, rgba{this}, kind{this}, shad{this}, minst{this}, imesh{this};
    // attribute shading: per-mesh records, corner normals / uvs, material slots, texture records and texels of every mesh (concatenated), the
    // sRGB table, and the per-pixel normal scratch
    DevBuf amesh{this}, anrm{this}, auv{this}, aslot{this}, atex{this}, texels{this}, srgb{this}, nbuf{this};
    uint32_t shading = 0;       // vx_render_set_shading flags
    int phase = 0;              // which of the two walk counters the next k_walk launch draws from (launch_trace)
    uint64_t nvmat = 0;
    // (behind the DevBufs: destroyed ahead of the blocks of the frames they order)
    Event ev_src[2];  // recorded on the voxel source's and the BVH's stream at the start of a frame
    Event ev_end;     // recorded on the scene's stream at its end
};

namespace {
vx_status render_desc_check(const vx_render_desc* d)
{
    if (!d) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (!d->grid == !d->octree) return fail(VX_ERR_INVALID_ARG, "exactly one voxel source: grid or octree");
    if (!d->bvh != !d->mesh) return fail(VX_ERR_INVALID_ARG, "bvh and mesh go together: both or neither");
    return VX_OK;
}

vx_status render_light(const vx_render_light* l, vx_render_light* out)
{
    if (!l) {  // hello_vulkan.h:84-90: point light at {10, 55, 8}, intensity 1000
        out->position[0] = 10.f; out->position[1] = 55.f; out->position[2] = 8.f;
        out->intensity = 1000.f;
        out->type = 0;
        return VX_OK;
    }
    if (l->type != 0 && l->type != 1) return fail(VX_ERR_INVALID_ARG, "light type must be 0 (point) or 1 (directional)");
    *out = *l;
    return VX_OK;
}

vx_status render_args_check(const vx_render_args* a, vx_render_light* light)
{
    if (!a || !a->view_inverse || !a->proj_inverse || !a->rgba) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (!a->width || !a->height) return fail(VX_ERR_INVALID_ARG, "zero width or height");
    if ((uint64_t)a->width * a->height >= 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^32 pixels");
    return render_light(a->light, light);
}

// the handles' state that a frame reads (checked at creation and before every frame: sources may be rebuilt in between)
vx_status render_sources_check(const vx_render_scene* s)
{
    if (s->grid && s->grid->kind != VX_GRID_BOOL) return fail(VX_ERR_INVALID_ARG, "the grid must be a VX_GRID_BOOL grid");
    const int dev = s->grid ? s->grid->device : (s->octree ? s->octree->device : s->tlas->device);
    const char* const devices = "the scene's handles live on different devices";
    if (s->bvh) {  // (its one mesh: render_desc_check)
        if (s->bvh->ntri != s->meshes[0]->nt) return fail(VX_ERR_INVALID_ARG, "the mesh's triangle count differs from the BVH's");
        if (s->bvh->device != dev) return fail(VX_ERR_INVALID_ARG, devices);
    }
    if (s->tlas) {
        if (s->tlas->device != dev) return fail(VX_ERR_INVALID_ARG, devices);
        if (s->meshes.size() != s->tlas->blas.size()) return fail(VX_ERR_INVALID_ARG, "one mesh per BLAS of the TLAS");
    }
    for (size_t k = 0; k < s->meshes.size(); ++k) {
        const vx_mesh* m = s->meshes[k];
        if (!m) return fail(VX_ERR_INVALID_ARG, "null mesh");
        if (s->tlas && m->nt != s->tlas->blas[k]->ntri) return fail(VX_ERR_INVALID_ARG, "mesh " + std::to_string(k) + ": its triangle count differs from its BLAS's");
        if (m->device != dev) return fail(VX_ERR_INVALID_ARG, devices);
    }
    return VX_OK;
}

// the voxel source's stream (k = 0) and the triangles' (k = 1: the BVH's or the TLAS's); null when the scene has no such source
bool has_source(const vx_render_scene* s, int k) { return k == 0 ? (s->grid || s->octree) : (s->bvh || s->tlas); }
hipStream_t source_stream(const vx_render_scene* s, int k)
{
    if (k == 0) return s->grid ? s->grid->stream : s->octree->stream;
    return s->bvh ? s->bvh->stream : s->tlas->stream;
}

// one table of a scene: `bytes` from host memory into b, on st; nothing to upload leaves b alone
hipError_t render_upload(DevBuf& b, const void* src, size_t bytes, hipStream_t st)
{
    if (!bytes) return hipSuccess;
    hipError_t e = b.ensure(bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st);
    return e;
}

// the grid's material table (getMatrials), and every mesh's OBJ records and per-triangle ids, concatenated, with a record per mesh (ids
// only where there is one per triangle: a hit of a mesh without them shades with MaterialObj{}); staged once, not per frame
vx_status render_upload_materials(vx_render_scene* s)
{
    s->nvmat = 0;
    if (s->grid && s->grid->has_materials) {
        const std::vector<vx_material>& vm = s->grid->materials;
        VX_HIP(render_upload(s->vmat, vm.data(), vm.size() * sizeof(vx_material), s->stream));
        s->nvmat = vm.size();
    }
    std::vector<vx_material> tm;
    std::vector<int32_t> ti;
    std::vector<std::pair<int64_t, int64_t>> off(s->meshes.size(), {-1, 0});
    for (size_t k = 0; k < s->meshes.size(); ++k) {
        const vx_mesh* m = s->meshes[k];
        off[k].second = (int64_t)tm.size();
        tm.insert(tm.end(), m->materials.begin(), m->materials.end());
        if (!m->tri_mat.empty() && m->tri_mat.size() == m->nt) {
            off[k].first = (int64_t)ti.size();
            ti.insert(ti.end(), m->tri_mat.begin(), m->tri_mat.end());
        }
    }
    VX_HIP(render_upload(s->mmat, tm.data(), tm.size() * sizeof(vx_material), s->stream));
    VX_HIP(render_upload(s->mids, ti.data(), ti.size() * 4, s->stream));
    s->imeshes.resize(s->meshes.size());
    for (size_t k = 0; k < s->meshes.size(); ++k) {
        const vx_mesh* m = s->meshes[k];
        vx::InstMesh& im = s->imeshes[k];
        im.verts = m->dv;
        im.idx = m->di;
        im.mids = off[k].first >= 0 ? s->mids.as<int32_t>() + off[k].first : nullptr;
        im.mat = m->materials.empty() ? nullptr : s->mmat.as<vx_material>() + off[k].second;
        im.nmat = m->materials.size();
    }
    // the table on the device is what the _tlas kernels read; a BVH scene's one record travels in RenderParams (render_enqueue)
    if (s->tlas) VX_HIP(render_upload(s->imesh, s->imeshes.data(), s->imeshes.size() * sizeof(vx::InstMesh), s->stream));
    VX_HIP(hipStreamSynchronize(s->stream));  // the host vectors may change after this call
    return VX_OK;
}

// the sRGB EOTF of c / 255 for every byte c, in float64, rounded to float32 (include/voxhip.h)
void srgb_table(float out[256])
{
    for (int c = 0; c < 256; ++c) {
        const double x = c / 255.0;
        out[c] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4));
    }
}

// attribute shading's tables: every mesh's corner attributes, material slots and textures (the texel pool with an {offset, w, h} record per
// slot; a slot without an image gets the 1x1 magenta of a file that failed to load), one AttrMesh per mesh, and the sRGB table.  Staged once
// at creation and by vx_render_refresh, never per frame.
vx_status render_upload_attributes(vx_render_scene* s)
{
    const std::vector<vx_mesh*>& ms = s->meshes;
    std::vector<float> nrm, uv;
    std::vector<int32_t> slot;
    std::vector<vx::TexRec> tex;
    std::vector<uint32_t> texels;
    struct Off { int64_t nrm, uv; size_t slot, tex; };
    std::vector<Off> off(ms.size());
    for (size_t k = 0; k < ms.size(); ++k) {
        const vx_mesh* m = ms[k];
        off[k].nrm = m->cnrm.size() == m->nt * 9 && m->nt ? (int64_t)nrm.size() : -1;
        if (off[k].nrm >= 0) nrm.insert(nrm.end(), m->cnrm.begin(), m->cnrm.end());
        off[k].uv = m->cuv.size() == m->nt * 6 && m->nt ? (int64_t)uv.size() : -1;
        if (off[k].uv >= 0) uv.insert(uv.end(), m->cuv.begin(), m->cuv.end());
        off[k].slot = slot.size();
        for (size_t i = 0; i < m->materials.size(); ++i) slot.push_back(i < m->mat_slot.size() ? m->mat_slot[i] : -1);
        off[k].tex = tex.size();
        for (const vx_mesh::Texture& t : m->tex) {
            vx::TexRec r;
            r.offset = texels.size();
            if (t.w) {
                r.w = t.w;
                r.h = t.h;
                const size_t cnt = (size_t)t.w * t.h;
                texels.resize(texels.size() + cnt);
                std::memcpy(texels.data() + r.offset, t.rgba.data(), cnt * 4);
            } else {
                r.w = r.h = 1;
                texels.push_back(0xFFFF00FFu);  // (255, 0, 255, 255), R in the low byte
            }
            tex.push_back(r);
        }
    }
    float lut[256];
    srgb_table(lut);
    VX_HIP(render_upload(s->srgb, lut, sizeof(lut), s->stream));
    VX_HIP(render_upload(s->anrm, nrm.data(), nrm.size() * 4, s->stream));
    VX_HIP(render_upload(s->auv, uv.data(), uv.size() * 4, s->stream));
    VX_HIP(render_upload(s->aslot, slot.data(), slot.size() * 4, s->stream));
    VX_HIP(render_upload(s->atex, tex.data(), tex.size() * sizeof(vx::TexRec), s->stream));
    VX_HIP(render_upload(s->texels, texels.data(), texels.size() * 4, s->stream));
    std::vector<vx::AttrMesh> am(ms.size());
    for (size_t k = 0; k < ms.size(); ++k) {
        const vx_mesh* m = ms[k];
        am[k].nrm = off[k].nrm >= 0 ? s->anrm.as<float>() + off[k].nrm : nullptr;
        am[k].uv = off[k].uv >= 0 ? s->auv.as<float>() + off[k].uv : nullptr;
        am[k].nslot = m->materials.size();
        am[k].slot = am[k].nslot ? s->aslot.as<int32_t>() + off[k].slot : nullptr;
        am[k].ntex = (uint32_t)m->tex.size();
        am[k].tex = am[k].ntex ? s->atex.as<vx::TexRec>() + off[k].tex : nullptr;
        am[k].pad = 0;
    }
    VX_HIP(render_upload(s->amesh, am.data(), am.size() * sizeof(vx::AttrMesh), s->stream));
    VX_HIP(hipStreamSynchronize(s->stream));  // the host vectors go out of scope
    return VX_OK;
}

// size the per-pixel buffers (pooled: a size already rendered requests nothing)
vx_status render_buffers(vx_render_scene* s, uint64_t n)
{
    if (has_source(s, 0)) {
        VX_HIP(s->vt.ensure(n * 4 + 8));
        VX_HIP(s->vprim.ensure(n * 4 + 8));
        VX_HIP(s->vnrm.ensure(n * 12 + 8));
        VX_HIP(s->sv.ensure(n + 8));
    }
    if (s->grid) VX_HIP(s->idxtmp.ensure(vx::trace_idx_bytes(s->grid->g, n)));
    if (s->tlas) VX_HIP(s->minst.ensure(n * 4 + 8));
    if (has_source(s, 1)) {
        VX_HIP(s->mt.ensure(n * 4 + 8));
        VX_HIP(s->mprim.ensure(n * 4 + 8));
        VX_HIP(s->mnrm.ensure(n * 12 + 8));
        VX_HIP(s->mbary.ensure(n * 8 + 8));
        VX_HIP(s->sm.ensure(n + 8));
    }
    VX_HIP(s->srays.ensure(n * 24 + 8));
    VX_HIP(s->sdist.ensure(n * 4 + 8));
    VX_HIP(s->stmax.ensure(n * 4 + 8));
    if ((s->shading & VX_RENDER_ATTRIBUTES) && has_source(s, 1)) VX_HIP(s->nbuf.ensure(n * 12 + 8));
    return VX_OK;
}

// one frame, enqueued on s->stream; rgba / kind / shadowed are device pointers
vx_status render_enqueue(vx_render_scene* s, const vx_render_args* a, const vx_render_light& light, uint32_t* rgba, uint8_t* kind, uint8_t* shadowed)
{
    const uint64_t n = (uint64_t)a->width * a->height;
    hipStream_t st = s->stream;
    vx_grid* g = s->grid;
    if (g) {  // the traversal structure and the word prefix, built once per grid build on the grid's own stream (no-ops when current)
        VX_TRY(ensure_coarse(g));
        bool pending = false;
        VX_TRY(prefix_launch(g, &pending));
    }
    VX_TRY(render_buffers(s, n));
    // start: the frame's stream waits for everything queued so far on the sources' streams
    for (int k = 0; k < 2; ++k) {
        if (!has_source(s, k)) continue;
        const hipStream_t ss = source_stream(s, k);
        if (ss == st) continue;
        VX_HIP(hipEventRecord(s->ev_src[k], ss));
        VX_HIP(hipStreamWaitEvent(st, s->ev_src[k], 0));
    }
    vx::Camera cam;
    std::memcpy(cam.viewInv, a->view_inverse, 64);
    std::memcpy(cam.projInv, a->proj_inverse, 64);
    cam.width = a->width;
    cam.height = a->height;
    vx::launch_render_camera(cam, s->camera.as<vx::Camera>(), st);
    // primary rays, rgen:50-51
    vx::TraceIO io;
    io.cam_dev = s->camera.as<vx::Camera>();
    io.nrays = n;
    io.tmin = 0.001f;
    io.tmax = 10000.0f;
    io.t_out = s->vt.as<float>();
    io.prim_out = s->vprim.as<uint32_t>();
    io.normal_out = s->vnrm.as<float>();
    vx::TraceMips mips{};
    const uint32_t* p16 = nullptr;
    if (g) mips = grid_mips(g, &p16);
    vx_octree* o = s->octree;
    auto voxels = [&](const vx::TraceIO& q) {
        if (g) vx::launch_trace(g->g, mips, g->wprefix.as<uint32_t>(), q, s->counters.as<unsigned long long>(), &s->phase, s->idxtmp.p, st, p16, nullptr);
        else octree_launch(o, q, st);
    };
    vx_bvh* b = s->bvh;
    vx_tlas* tl = s->tlas;
    auto triangles = [&](const vx::TraceIO& q, float* bary, uint32_t* inst) {
        if (tl) vx::launch_tlas_trace(tlas_dev(tl), q, bary, inst, st);
        else bvh_launch(b, q, bary, st);
    };
    const bool vox = has_source(s, 0);
    if (vox) voxels(io);
    if (b || tl) {
        vx::TraceIO mio = io;
        mio.t_out = s->mt.as<float>();
        mio.prim_out = s->mprim.as<uint32_t>();
        mio.normal_out = s->mnrm.as<float>();
        triangles(mio, s->mbary.as<float>(), tl ? s->minst.as<uint32_t>() : nullptr);
    }
    vx::RenderParams P;
    P.n = n;
    P.cam = s->camera.as<vx::Camera>();
    P.vt = vox ? s->vt.as<float>() : nullptr;
    P.vprim = vox ? s->vprim.as<uint32_t>() : nullptr;
    P.vnrm = vox ? s->vnrm.as<float>() : nullptr;
    if (b || tl) {
        P.mt = s->mt.as<float>();
        P.mprim = s->mprim.as<uint32_t>();
        P.mnrm = s->mnrm.as<float>();
        P.mbary = s->mbary.as<float>();
        P.sm = s->sm.as<uint8_t>();
    }
    if (tl) {
        P.minst = s->minst.as<uint32_t>();
        P.ixf = tl->xf.as<float>();
        P.iblas = tl->iblas.as<uint32_t>();
        P.imesh = s->imesh.as<vx::InstMesh>();
    }
    if (b) {  // its one mesh's record, by value
        const vx::InstMesh& im = s->imeshes[0];
        P.verts = im.verts;
        P.idx = im.idx;
        P.mids = im.mids;
        P.mmat = im.mat;
        P.nmmat = im.nmat;
    }
    for (int k = 0; k < 3; ++k) P.light[k] = light.position[k];
    P.intensity = light.intensity;
    P.light_type = light.type;
    P.srays = s->srays.as<float>();
    P.sdist = s->sdist.as<float>();
    P.stmax = s->stmax.as<float>();
    P.sv = vox ? s->sv.as<uint8_t>() : nullptr;
    const int16_t* vids = g ? vx_grid_material_ids_device(g) : nullptr;
    if (vids && s->nvmat) {
        P.vids = vids;
        P.nvids = g->mat_gathered ? g->mat_gather_count : g->mat_count;
        P.vmat = s->vmat.as<vx_material>();
        P.nvmat = s->nvmat;
    }
    P.rgba = rgba;
    P.kind_out = kind;
    P.shadowed_out = shadowed;
    const bool attr = (s->shading & VX_RENDER_ATTRIBUTES) && (b || tl);  // voxel hits are shaded as by default: only triangles change
    vx::AttrParams A;
    if (attr) {
        A.mesh = s->amesh.as<vx::AttrMesh>();
        A.texels = s->texels.as<uint32_t>();
        A.srgb = s->srgb.as<float>();
        A.w2o = tl ? tl->w2o.as<float>() : nullptr;
        A.nbuf = s->nbuf.as<float>();
    }
    vx::launch_render_shadow_rays(P, attr ? &A : nullptr, tl != nullptr, st);
    // shadow rays: any-hit against the voxels and the mesh (rchit:108-122), tMax = the light distance -- or 0, the empty interval
    // (0 < tmin) that the traversals leave at once, for pixels whose shading cannot read the flag: misses, hits facing away from the
    // light (5-12 % of the frame)
    vx::TraceIO sio;
    sio.rays = s->srays.as<float>();
    sio.nrays = n;
    sio.tmin = 0.001f;
    sio.tmax = 10000.0f;
    sio.tmax_per_ray = s->stmax.as<float>();
    sio.any_hit = true;
    sio.shadowed_out = s->sv.as<uint8_t>();
    if (vox) voxels(sio);
    if (b || tl) {
        sio.shadowed_out = s->sm.as<uint8_t>();
        triangles(sio, nullptr, nullptr);
    }
    vx::launch_render_shade(P, attr ? &A : nullptr, tl != nullptr, st);
    VX_HIP(hipGetLastError());
    // end: later work on the sources' streams (a rebuild) waits for the frame's reads
    VX_HIP(hipEventRecord(s->ev_end, st));
    for (int k = 0; k < 2; ++k) {
        if (!has_source(s, k)) continue;
        const hipStream_t ss = source_stream(s, k);
        if (ss != st) VX_HIP(hipStreamWaitEvent(ss, s->ev_end, 0));
    }
    if (tl)  // the BLAS a frame reads: a later vx_bvh_build_into waits for it too
        for (vx_bvh* bb : tl->blas)
            if (bb->stream != st && bb->stream != tl->stream) VX_HIP(hipStreamWaitEvent(bb->stream, s->ev_end, 0));
    return VX_OK;
}
}  // namespace

namespace {
vx_status render_create_common(Fresh<vx_render_scene> s, vx_render_scene** out);
}

vx_status vx_render_create(const vx_render_desc* desc, vx_render_scene** out)
{
    if (!out) return fail(VX_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    VX_TRY(render_desc_check(desc));
    VX_TRY(need_device(g_device));
    Fresh<vx_render_scene> s(new vx_render_scene());
    s->grid = const_cast<vx_grid*>(desc->grid);
    s->octree = const_cast<vx_octree*>(desc->octree);
    s->bvh = const_cast<vx_bvh*>(desc->bvh);
    if (desc->mesh) s->meshes.push_back(const_cast<vx_mesh*>(desc->mesh));
    s->stream = (hipStream_t)desc->stream;
    return render_create_common(std::move(s), out);
}

vx_status vx_render_create_tlas(const vx_render_tlas_desc* desc, vx_render_scene** out)
{
    if (!out) return fail(VX_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!desc || !desc->tlas || (!desc->meshes && desc->tlas->blas.size())) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (desc->grid && desc->octree) return fail(VX_ERR_INVALID_ARG, "at most one voxel source: grid or octree");
    VX_TRY(need_device(desc->tlas->device));
    Fresh<vx_render_scene> s(new vx_render_scene());
    s->grid = const_cast<vx_grid*>(desc->grid);
    s->octree = const_cast<vx_octree*>(desc->octree);
    s->tlas = const_cast<vx_tlas*>(desc->tlas);
    for (size_t k = 0; k < s->tlas->blas.size(); ++k) s->meshes.push_back(const_cast<vx_mesh*>(desc->meshes[k]));
    s->stream = (hipStream_t)desc->stream;
    return render_create_common(std::move(s), out);
}

namespace {
vx_status render_create_common(Fresh<vx_render_scene> s, vx_render_scene** out)
{
    s->device = s->grid ? s->grid->device : (s->octree ? s->octree->device : s->tlas->device);
    VX_TRY(render_sources_check(s.get()));
    DeviceGuard dg(s->device);
    for (vx_mesh* m : s->meshes) VX_TRY(mesh_to_device(m));
    VX_HIP(s->camera.ensure(sizeof(vx::Camera)));
    VX_HIP(s->counters.ensure(4 * sizeof(unsigned long long)));
    VX_HIP(hipMemsetAsync(s->counters.p, 0, 4 * sizeof(unsigned long long), s->stream));  // the walk's counters start at zero
    for (Event* ev : {&s->ev_src[0], &s->ev_src[1], &s->ev_end}) VX_HIP(ev->create());
    VX_TRY(render_upload_materials(s.get()));
    VX_TRY(render_upload_attributes(s.get()));
    *out = s.release();
    return VX_OK;
}
}  // namespace

vx_status vx_render_refresh(vx_render_scene* s)
{
    if (!s) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(render_sources_check(s));
    DeviceGuard dg(s->device);
    // the old tables may still be read by a frame in flight: queue the refresh behind it on the scene's stream (upload is stream-ordered)
    VX_TRY(render_upload_materials(s));
    return render_upload_attributes(s);
}

vx_status vx_render_set_shading(vx_render_scene* s, uint32_t flags)
{
    if (!s) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (flags & ~(uint32_t)VX_RENDER_ATTRIBUTES) return fail(VX_ERR_INVALID_ARG, "unknown shading flag");
    s->shading = flags;
    return VX_OK;
}

// The two frame entry points: the argument and light checks, the device count, the null scene, the sources' state, the guard, then one
// frame into the caller's device arrays or (host) into the blocks the scene keeps, through a Staging.
static vx_status render_frame_entry(vx_render_scene* s, const vx_render_args* a, bool host)
{
    vx_render_light light;
    VX_TRY(render_args_check(a, &light));
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return fail(VX_ERR_NO_DEVICE, "no HIP device available: libvoxhip has no CPU path");
    if (!s) return fail(VX_ERR_INVALID_ARG, "null argument");
    VX_TRY(render_sources_check(s));
    DeviceGuard dg(s->device);
    if (!host) return render_enqueue(s, a, light, a->rgba, a->kind, a->shadowed);
    const size_t n = (size_t)a->width * a->height;
    Staging st(*s);
    uint32_t* rgba = st.out(a->rgba, n * 4, 0, &s->rgba);
    uint8_t* kind = st.out(a->kind, n, 0, &s->kind);
    uint8_t* shadowed = st.out(a->shadowed, n, 0, &s->shad);
    VX_TRY(st.status());
    VX_TRY(render_enqueue(s, a, light, rgba, kind, shadowed));
    return st.finish();
}

vx_status vx_render_frame_device(vx_render_scene* s, const vx_render_args* a) { return render_frame_entry(s, a, false); }
vx_status vx_render_frame(vx_render_scene* s, const vx_render_args* a) { return render_frame_entry(s, a, true); }

void vx_render_free(vx_render_scene* s) { handle_free(s); }

// ---- test aid: the octree's item sort on a host array ----------------------------------------------------------
vx_status vx_sort_u64(uint64_t* host_keys, uint64_t n, int bits)
{
    if (!host_keys && n) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (bits < 1 || bits > 64) return fail(VX_ERR_INVALID_ARG, "bits must be in 1..64");
    if (n >= 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^32 keys");
    if (!n) return VX_OK;
    VX_TRY(need_device(g_device));
    DeviceGuard dg(g_device);
    const Home here(g_device, nullptr, /*drained=*/true);  // (every step below waits for the device)
    DevBuf a{&here}, b{&here}, tmp{&here};
    VX_HIP(a.ensure((size_t)n * 8));
    VX_HIP(b.ensure((size_t)n * 8));
    const size_t tb = vx::sort_tmp_bytes(n);
    VX_HIP(tmp.ensure(tb));
    VX_HIP(hipMemcpy(a.p, host_keys, (size_t)n * 8, hipMemcpyHostToDevice));
    const int where = vx::launch_sort_u64(a.as<uint64_t>(), b.as<uint64_t>(), n, bits, tmp.p, tb, nullptr);
    VX_HIP(hipStreamSynchronize(nullptr));
    VX_HIP(hipMemcpy(host_keys, where == 0 ? a.p : b.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return VX_OK;
}

// ---- test aid: the device prefix scan on host arrays, scan after scan on one scratch block --------------------------
vx_status vx_scan_u32(const vx_scan_args* a)
{
    if (!a || (a->nscans && (!a->sizes || !a->paths || !a->totals))) return fail(VX_ERR_INVALID_ARG, "null argument");
    if (a->mode > VX_SCAN_BYTES) return fail(VX_ERR_INVALID_ARG, "mode must be VX_SCAN_VALUES, VX_SCAN_POPCOUNT or VX_SCAN_BYTES");
    if (a->total_tag & kMailValue) return fail(VX_ERR_INVALID_ARG, "total_tag must only have bits 48..63");
    if (a->gen_start >= (1u << 22)) return fail(VX_ERR_INVALID_ARG, "gen_start must be below 2^22");
    if (a->mode == VX_SCAN_BYTES && ((a->sel && a->sel_cap) || (a->group16 && a->group16_cap)))
        return fail(VX_ERR_INVALID_ARG, "the byte scan has no sel / group16 outputs");
    if (a->mode != VX_SCAN_POPCOUNT && a->sel && a->sel_cap) return fail(VX_ERR_INVALID_ARG, "sel needs values of at most 1024: popcount mode only");
    const size_t esz = a->mode == VX_SCAN_BYTES ? 1 : 4;
    uint64_t nmax = 0, nin = 0, nout = 0;
    for (uint32_t k = 0; k < a->nscans; ++k) {
        if (a->paths[k] > VX_SCAN_PATH_AUTO) return fail(VX_ERR_INVALID_ARG, "unknown scan path");
        if (a->sizes[k] >= 0xFFFFFFFFull) return fail(VX_ERR_CAPACITY, "more than 2^32 elements");
        nmax = std::max(nmax, a->sizes[k]);
        nin += a->sizes[k];
        nout += a->sizes[k] + 1 + VX_SCAN_CANARY;
    }
    if ((nin && !a->in) || (nout && !a->out)) return fail(VX_ERR_INVALID_ARG, "null argument");
    // what the kernel writes: sel[c] for c * 1024 below the total (at most 32 per word), group16[0..n / 16]
    if (a->sel && a->sel_cap && a->sel_cap < (32 * nmax + 1023) / 1024) return fail(VX_ERR_INVALID_ARG, "sel_cap below ceil(32 n / 1024)");
    if (a->group16 && a->group16_cap && a->group16_cap < nmax / 16 + 1) return fail(VX_ERR_INVALID_ARG, "group16_cap below n / 16 + 1");
    if (!a->nscans) return VX_OK;
    VX_TRY(need_device(g_device));
    DeviceGuard dg(g_device);
    hipStream_t s = nullptr;
    const Home here(g_device, s, /*drained=*/true);  // (every scan below is waited for before the next step)
    DevBuf din{&here}, dout{&here}, dsel{&here}, dg16{&here}, dtot{&here};
    ScanScratch tmp{&here};
    const uint64_t out_words = a->out_offset + nmax + 1 + VX_SCAN_CANARY;
    const uint64_t sel_cap = a->sel ? a->sel_cap : 0, g16_cap = a->group16 ? a->group16_cap : 0;
    std::vector<uint32_t> canary(std::max<uint64_t>(std::max(out_words, sel_cap), g16_cap), VX_SCAN_CANARY_VALUE);
    VX_HIP(din.ensure((size_t)(a->in_offset + nmax) * esz + 16));
    VX_HIP(dout.ensure((size_t)out_words * 4));
    VX_HIP(dsel.ensure((size_t)sel_cap * 4 + 4));
    VX_HIP(dg16.ensure((size_t)g16_cap * 4 + 4));
    VX_HIP(dtot.ensure(8));
    VX_HIP(tmp.reserve(nmax, s));
    std::vector<unsigned long long> state(tmp.block.cap / sizeof(unsigned long long));
    tmp.start_at(a->gen_start);
    bool zero = true;  // the scratch block is known to be all zero (what ticket-mode and three-pass scans require and leave behind)
    uint64_t ioff = 0, ooff = 0;
    for (uint32_t k = 0; k < a->nscans; ++k) {
        const uint64_t n = a->sizes[k];
        uint32_t* out = dout.as<uint32_t>() + a->out_offset;
        uint32_t* sel = sel_cap ? dsel.as<uint32_t>() : nullptr;
        uint32_t* g16 = g16_cap ? dg16.as<uint32_t>() : nullptr;
        VX_HIP(hipMemcpy(dout.p, canary.data(), (size_t)out_words * 4, hipMemcpyHostToDevice));
        if (sel) VX_HIP(hipMemcpy(sel, canary.data(), (size_t)sel_cap * 4, hipMemcpyHostToDevice));
        if (g16) VX_HIP(hipMemcpy(g16, canary.data(), (size_t)g16_cap * 4, hipMemcpyHostToDevice));
        if (n) VX_HIP(hipMemcpy((char*)din.p + a->in_offset * esz, (const char*)a->in + ioff * esz, (size_t)n * esz, hipMemcpyHostToDevice));
        VX_HIP(hipMemset(dtot.p, 0, 8));
        // the path: GEN / AUTO = what the library's own callers do, the next generation of the block (ticket mode above kScanGenTiles tiles):
        // through ScanScratch where in and out start their blocks, as theirs do;
        // TICKET / THREE = no generation, on a block that is all zero (cleared first when an older generation-mode scan left words);
        // those and offset starts go to the launchers directly
        const uint32_t p = a->paths[k];
        const bool numbered = p == VX_SCAN_PATH_GEN || p == VX_SCAN_PATH_AUTO;
        vx::ScanTaken took;
        if (numbered && !a->in_offset && !a->out_offset) {
            if (a->mode == VX_SCAN_BYTES) VX_TRY(tmp.u8(din, dout, n, dtot.as<unsigned long long>(), s, a->total_tag));
            else VX_TRY(tmp.u32(din, dout, n, a->mode == VX_SCAN_POPCOUNT, dtot.as<unsigned long long>(), s, {a->total_tag, sel, g16}));
            took = tmp.took;
        } else {
            const uint32_t gen = numbered ? tmp.next_gen(s) : 0u;
            if (!gen && !zero) (void)hipMemsetAsync(tmp.block.p, 0, tmp.block.cap, s);
            if (a->mode == VX_SCAN_BYTES) {
                took = vx::launch_scan_u8((const uint8_t*)din.p + a->in_offset, out, n, tmp.block.p, dtot.as<unsigned long long>(), s, a->total_tag, gen);
            } else {
                vx::ScanArgs sa;
                sa.tmp_is_zero = true;
                sa.total_tag = a->total_tag;
                sa.sel1024 = sel;
                sa.gen = gen;
                sa.group16 = g16;
                sa.path = p == VX_SCAN_PATH_THREE ? vx::kScanPathThree : p == VX_SCAN_PATH_AUTO ? vx::kScanPathAuto : vx::kScanPathOne;
                took = vx::launch_scan_u32(din.as<uint32_t>() + a->in_offset, out, n, a->mode == VX_SCAN_POPCOUNT, tmp.block.p, dtot.as<unsigned long long>(), s, sa);
            }
        }
        VX_HIP(hipStreamSynchronize(s));
        VX_HIP(hipMemcpy(a->out + ooff, out, (size_t)(n + 1 + VX_SCAN_CANARY) * 4, hipMemcpyDeviceToHost));
        VX_HIP(hipMemcpy(&a->totals[k], dtot.p, 8, hipMemcpyDeviceToHost));
        if (sel) VX_HIP(hipMemcpy(a->sel + (size_t)k * sel_cap, sel, (size_t)sel_cap * 4, hipMemcpyDeviceToHost));
        if (g16) VX_HIP(hipMemcpy(a->group16 + (size_t)k * g16_cap, g16, (size_t)g16_cap * 4, hipMemcpyDeviceToHost));
        VX_HIP(hipMemcpy(state.data(), tmp.block.p, state.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        // clean: a scan without a generation number leaves the block all zero; one with a generation number leaves the ticket and the
        // finished-tiles words zero and state words of its own or an older generation only, never of a later one (which a later scan
        // would take for its own)
        bool all_zero = true, ok = true;
        for (size_t i = 0; i < state.size(); ++i) {
            const unsigned long long w = state[i];
            if (!w) continue;
            all_zero = false;
            const unsigned long long wg = (w >> 40) & ((1ull << 22) - 1ull);
            if (i < 2 || (w >> 62) == 0 || wg == 0 || wg > tmp.gen) ok = false;
        }
        if (!numbered && !all_zero) ok = false;
        if (a->clean) a->clean[k] = ok ? 1u : 0u;
        if (a->taken) a->taken[k] = took == vx::ScanTaken::three_pass ? VX_SCAN_PATH_THREE : took == vx::ScanTaken::generation ? VX_SCAN_PATH_GEN : VX_SCAN_PATH_TICKET;
        zero = all_zero;
        ioff += n;
        ooff += n + 1 + VX_SCAN_CANARY;
    }
    return VX_OK;
}

uint64_t vx_device_allocations(void) { return g_pool_requests.load(std::memory_order_relaxed); }

uint64_t vx_device_live_blocks(void)
{
    uint64_t n = 0;
    for (Pool& P : g_pool) {
        std::lock_guard<std::mutex> lk(P.mu);
        n += P.live.size();
    }
    return n;
}

// ---- test aid: poisoned pool blocks ---------------------------------------------------------------------------
vx_status vx_pool_poison(int on, uint32_t pattern)
{
    g_pool_poison.store(on ? ((1ull << 32) | (uint64_t)pattern) : 0ull, std::memory_order_relaxed);
    return VX_OK;
}

uint64_t vx_pool_poisoned_blocks(void) { return g_pool_poisoned.load(std::memory_order_relaxed); }

// ---- per-kernel timing (bench / profiling aid) ----------------------------------------------------------------
vx_status vx_profile_enable(int on)
{
    vx::prof_enable(on != 0);
    return VX_OK;
}
vx_status vx_profile_select(const char* kernel_name)
{
    vx::prof_select(kernel_name);
    return VX_OK;
}
vx_status vx_profile_reset(void)
{
    vx::prof_reset();
    return VX_OK;
}
vx_status vx_profile_read(int slot, char* name, size_t name_capacity, double* total_ms, uint64_t* launches)
{
    if (vx::prof_read(slot, name, name_capacity, total_ms, launches) != 0) return fail(VX_ERR_INVALID_ARG, "no such profile slot");
    return VX_OK;
}

// ---- sharding helpers -----------------------------------------------------------------------------------------
void vx_shard_words(uint64_t num_words, int rank, int world, uint64_t* wb, uint64_t* we, uint64_t* padded)
{
    if (world < 1) world = 1;
    const uint64_t chunk = (num_words + (uint64_t)world - 1) / (uint64_t)world;
    uint64_t b = (uint64_t)rank * chunk;
    if (b > num_words) b = num_words;
    uint64_t e = b + chunk;
    if (e > num_words) e = num_words;
    if (wb) *wb = b;
    if (we) *we = e;
    if (padded) *padded = chunk;
}

void vx_shard_range(uint64_t count, int rank, int world, uint64_t* begin, uint64_t* end)
{
    if (world < 1) world = 1;
    const uint64_t chunk = (count + (uint64_t)world - 1) / (uint64_t)world;
    uint64_t b = (uint64_t)rank * chunk;
    if (b > count) b = count;
    uint64_t e = b + chunk;
    if (e > count) e = count;
    if (begin) *begin = b;
    if (end) *end = e;
}

}  // extern "C"
