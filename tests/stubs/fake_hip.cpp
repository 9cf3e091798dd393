// fake_hip.cpp -- a recording stand-in for the HIP runtime (tests/test_launch_trace.py).  hiprt.cpp binds whatever HARE_HIP_RUNTIME names, so a
// process that has not loaded libamdhip64 runs the whole unmodified library against this: one device (FAKE_HIP_CUS compute units, default
// 256), allocations in host memory, uploads copied for real, module functions as interned name strings, streams and events as counters.
// hipModuleLaunchKernel runs nothing: it appends one line to a log -- kernel, grid, block, dynamic LDS, and for the hare_voxel_* /
// hare_octree_* / hare_kdtree_* kernels the two argument structs decoded with the tree's own hare_device.h.  A scalar field that is zero and a
// pointer that is null are left out of the line (absent = 0 / null); every other pointer is written `name+offset`: relative to the caller's
// buffers (real ones named through fake_hip_name_host_range; FAKE_HIP_BUFFERS: name=hex address, ... ; each 2^40 bytes) or to the live allocations, numbered in the order they were made (a0,
// a1, ...).  Events and streams are numbered the same way (e0 ...; s0 is the null stream).  hipMemsetAsync, hipMemcpyAsync, hipStreamWaitEvent
// and hipEventRecord are logged in order.  The stub never dereferences a pointer it did not allocate (host sources of uploads apart).
// For the hare_hist_* kernels the line holds their buffers and counts.  fake_hip_log_enable(2) also logs, for a test that counts them, every
// hipMalloc (`malloc a3 bytes=...`), hipFree (`free a3`) and hipStreamSynchronize (`sync s0`).
// Built with g++ alone: no HIP header, the runtime's enums are ints at the ABI.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <algorithm>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "hare_device.h"

using namespace hare;

namespace {

struct Alloc { char* base; size_t size; };
struct Region { std::string name; uintptr_t base; };
std::mutex g_mu;
std::vector<Alloc> g_allocs;              // live, in the order they were made
std::vector<void*> g_events, g_streams;   // live handles, in the order they were made
std::vector<Region> g_regions;
struct HostRange { std::string name; uintptr_t base; size_t bytes; };
std::vector<HostRange> g_host;            // the caller's real buffers (fake_hip_name_host_range)
std::set<std::string> g_names;            // interned kernel names: a hipFunction_t is the address of one
std::string g_log;
int g_log_on = 1;                         // 0: nothing; 1: launches, copies, memsets, events; 2: allocations, frees and synchronisations too
uintptr_t g_next_handle = 0x1000;
constexpr uintptr_t kRegionBytes = (uintptr_t)1 << 40;
constexpr size_t kBigAlloc = (size_t)1 << 20;

void read_regions()
{
    static bool done = false;
    if (done) return;
    done = true;
    const char* e = getenv("FAKE_HIP_BUFFERS");
    if (!e) return;
    std::string s(e);
    size_t p = 0;
    while (p < s.size()) {
        const size_t c = std::min(s.find(',', p), s.size()), q = s.find('=', p);
        if (q != std::string::npos && q < c) g_regions.push_back({s.substr(p, q - p), (uintptr_t)strtoull(s.substr(q + 1, c - q - 1).c_str(), nullptr, 16)});
        p = c + 1;
    }
}

const Alloc* find_alloc(const void* p, size_t* rank)
{
    for (size_t k = 0; k < g_allocs.size(); ++k)
        if ((const char*)p >= g_allocs[k].base && (const char*)p < g_allocs[k].base + std::max<size_t>(g_allocs[k].size, 1)) {
            if (rank) *rank = k;
            return &g_allocs[k];
        }
    return nullptr;
}

std::string ptr_name(const void* p)
{
    if (!p) return "null";
    read_regions();
    char buf[96];
    const uintptr_t x = (uintptr_t)p;
    for (const HostRange& r : g_host)
        if (x >= r.base && x < r.base + std::max<size_t>(r.bytes, 1)) {
            snprintf(buf, sizeof buf, "%s+%llu", r.name.c_str(), (unsigned long long)(x - r.base));
            return buf;
        }
    for (const Region& r : g_regions)
        if (x >= r.base && x < r.base + kRegionBytes) {
            snprintf(buf, sizeof buf, "%s+%llu", r.name.c_str(), (unsigned long long)(x - r.base));
            return buf;
        }
    size_t k = 0;
    if (const Alloc* a = find_alloc(p, &k)) {
        snprintf(buf, sizeof buf, "a%zu+%llu", k, (unsigned long long)((const char*)p - a->base));
        return buf;
    }
    return "?";
}

std::string handle_name(const std::vector<void*>& live, void* h, char letter)
{
    if (!h) return letter == 's' ? "s0" : "null";
    const auto it = std::find(live.begin(), live.end(), h);
    if (it == live.end()) return std::string(1, letter) + "?";
    return std::string(1, letter) + std::to_string((it - live.begin()) + (letter == 's' ? 1 : 0));
}

void add(std::string& o, const char* name, const void* p) { if (p) o += std::string(" ") + name + "=" + ptr_name(p); }
void add(std::string& o, const char* name, long long v) { if (v) o += std::string(" ") + name + "=" + std::to_string(v); }
void add(std::string& o, const char* name, int v) { add(o, name, (long long)v); }
void add(std::string& o, const char* name, long v) { add(o, name, (long long)v); }
void add(std::string& o, const char* name, unsigned v) { add(o, name, (long long)v); }
void add(std::string& o, const char* name, double v)
{
    if (v == 0) return;
    char buf[64];
    snprintf(buf, sizeof buf, " %s=%.17g", name, v);
    o += buf;
}
void add(std::string& o, const char* name, float v) { add(o, name, (double)v); }
template <class T, size_t N> void add(std::string& o, const char* name, const T (&v)[N])
{
    for (size_t k = 0; k < N; ++k) add(o, (std::string(name) + "[" + std::to_string(k) + "]").c_str(), v[k]);
}
void add(std::string& o, const char* name, const CullFrame& c)
{
    const std::string n(name);
    add(o, (n + ".org").c_str(), c.org);
    add(o, (n + ".step").c_str(), c.step);
    add(o, (n + ".err0").c_str(), c.err0);
    add(o, (n + ".stride").c_str(), c.stride);
}
#define F(x) add(o, #x, a.x)

std::string decode(const VoxelArgs& a)
{
    std::string o = "voxel{";
    F(polys); F(quads); F(cells); F(items); F(occ); F(ct); F(occ_words); F(occ_shift); F(occ_cd); F(omin); F(omax); F(vd); F(cull); F(cf);
    F(cellbox); F(cellbox_mid); F(cellbox_rad); F(bocc); F(bocc_nb); F(bocc_words);
    return o + " }";
}
std::string decode(const OctreeArgs& a)
{
    std::string o = "octree{";
    F(polys); F(quads); F(nodes); F(items); F(n_nodes); F(max_depth); F(cull); F(cf); F(tight); F(tight_mid); F(tight_rad);
    return o + " }";
}
std::string decode(const KdArgs& a)
{
    std::string o = "kd{";
    F(polys); F(quads); F(nodes); F(items); F(n_nodes); F(max_depth); F(cull); F(cf); F(tight); F(tight_mid); F(tight_rad); F(dnodes);
    return o + " }";
}
std::string decode(const ReduceArgs& a)
{
    std::string o = "reduce{";
    F(hist); F(weight); F(sums); F(cross); F(n_bins); F(bands); F(channels); F(n_win); F(n_lev);
    return o + " }";
}
std::string decode(const ProjectArgs& a)
{
    std::string o = "project{";
    F(hist); F(weight); F(coef); F(proj); F(n_bins); F(bands); F(channels); F(n_vec);
    return o + " }";
}
std::string decode(const RenderArgs& a)
{
    std::string o = "render{";
    F(hist); F(weight); F(taps); F(out); F(n_bins); F(bands); F(channels); F(frac_bits); F(M); F(T); F(tile_bins); F(tiles); F(sign_words);
    return o + " }";
}
std::string decode(const ShootIO& a)
{
    std::string o = "io{";
    F(rays); F(excl1); F(excl2); F(out); F(ctr); F(work); F(prof); F(n); F(flags); F(steps_per_round); F(refill_min_idle); F(ray_chunk);
    F(exact_min_parked); F(audit_polys); F(ticket_rays); F(static_rays); F(tmax); F(occluded); F(coop_tail); F(wide_drain); F(oct_tail);
    F(oct_tail_stride); F(oct_tail_levels); F(oct_tail_max); F(oct_tail_patience); F(bounce_casts); F(out_all); F(out_stride); F(ctr_casts);
    F(order); F(blocks); F(blk_words); F(walk_steps); F(hand_walk); F(oct_spill); F(oct_spill_cap);
    return o + " }";
}
#undef F

void log_line(const std::string& s, int level = 1)
{
    if (g_log_on >= level) { g_log += s; g_log += '\n'; }
}

bool starts(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

}  // namespace

extern "C" {

// ---- what the test reads (the same shared object, opened a second time with ctypes)
const char* fake_hip_log(void) { std::lock_guard<std::mutex> lk(g_mu); static std::string copy; copy = g_log; return copy.c_str(); }
void fake_hip_log_clear(void) { std::lock_guard<std::mutex> lk(g_mu); g_log.clear(); }
void fake_hip_log_enable(int on) { std::lock_guard<std::mutex> lk(g_mu); g_log_on = on; }
long long fake_hip_live_allocations(void) { std::lock_guard<std::mutex> lk(g_mu); return (long long)g_allocs.size(); }
// a real host buffer of the caller's: pointers into [base, base + bytes) print as name+offset (a null name forgets every range)
void fake_hip_name_host_range(const char* name, const void* base, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!name) g_host.clear();
    else g_host.push_back({name, (uintptr_t)base, bytes});
}

// ---- the entry points hiprt.cpp binds
int hipGetDeviceCount(int* n) { *n = 1; return 0; }
int hipSetDevice(int d) { return d == 0 ? 0 : 101; }
int hipGetDevice(int* d) { *d = 0; return 0; }
int hipDeviceGetAttribute(int* v, int, int)          // the library asks for one attribute: the compute units
{
    const char* e = getenv("FAKE_HIP_CUS");
    *v = e ? atoi(e) : 256;
    return 0;
}
int hipMalloc(void** p, size_t n)
{
    // from kBigAlloc on: address space without a reservation -- the rings of a scene are hundreds of MiB that nothing here touches, and
    // whether they can be had must not depend on the machine's memory
    char* m = n >= kBigAlloc ? (char*)mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0) : (char*)malloc(std::max<size_t>(n, 1));
    if (!m || m == (char*)MAP_FAILED) { *p = nullptr; return 2; }
    std::lock_guard<std::mutex> lk(g_mu);
    g_allocs.push_back({m, n});
    log_line("malloc a" + std::to_string(g_allocs.size() - 1) + " bytes=" + std::to_string(n), 2);
    *p = m;
    return 0;
}
int hipFree(void* p)
{
    if (!p) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    for (size_t k = 0; k < g_allocs.size(); ++k)
        if (g_allocs[k].base == p) {
            log_line("free a" + std::to_string(k), 2);
            if (g_allocs[k].size >= kBigAlloc) munmap(p, g_allocs[k].size);
            else free(p);
            g_allocs.erase(g_allocs.begin() + (long)k);
            return 0;
        }
    return 1;
}
int hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(std::max<size_t>(n, 1)); return *p ? 0 : 2; }
int hipHostFree(void* p) { free(p); return 0; }
static void copy_if_ours(void* dst, const void* src, size_t n, int kind)
{
    // 1 = host to device: the source is the library's host memory; everything else would read or write memory that may not exist
    const Alloc* a = find_alloc(dst, nullptr);
    if (kind == 1 && a && (char*)dst + n <= a->base + a->size) memcpy(dst, src, n);
}
int hipMemcpy(void* dst, const void* src, size_t n, int kind)
{
    std::lock_guard<std::mutex> lk(g_mu);
    copy_if_ours(dst, src, n, kind);
    return 0;
}
int hipMemcpyAsync(void* dst, const void* src, size_t n, int kind, void* st)
{
    std::lock_guard<std::mutex> lk(g_mu);
    log_line("memcpy " + ptr_name(dst) + " <- " + ptr_name(src) + " bytes=" + std::to_string(n) + " kind=" + std::to_string(kind) + " " + handle_name(g_streams, st, 's'));
    if (kind == 1) copy_if_ours(dst, src, n, kind);
    return 0;
}
static void set_if_ours(void* dst, int v, size_t n)
{
    const Alloc* a = find_alloc(dst, nullptr);
    if (a && (char*)dst + n <= a->base + a->size) memset(dst, v, n);
}
int hipMemset(void* dst, int v, size_t n)
{
    std::lock_guard<std::mutex> lk(g_mu);
    set_if_ours(dst, v, n);
    return 0;
}
int hipMemsetAsync(void* dst, int v, size_t n, void* st)
{
    std::lock_guard<std::mutex> lk(g_mu);
    log_line("memset " + ptr_name(dst) + " value=" + std::to_string(v) + " bytes=" + std::to_string(n) + " " + handle_name(g_streams, st, 's'));
    set_if_ours(dst, v, n);
    return 0;
}
int hipStreamCreate(void** s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    *s = (void*)(g_next_handle += 16);
    g_streams.push_back(*s);
    return 0;
}
int hipStreamDestroy(void* s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_streams.erase(std::remove(g_streams.begin(), g_streams.end(), s), g_streams.end());
    return 0;
}
int hipStreamSynchronize(void* st)
{
    std::lock_guard<std::mutex> lk(g_mu);
    log_line("sync " + handle_name(g_streams, st, 's'), 2);
    return 0;
}
int hipDeviceSynchronize(void) { return 0; }
int hipStreamIsCapturing(void*, int* status) { *status = 0; return 0; }
int hipModuleLoadData(void** m, const void*) { *m = (void*)(uintptr_t)0x10; return 0; }
int hipModuleUnload(void*) { return 0; }
int hipModuleGetFunction(void** f, void*, const char* name)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (const char* e = getenv("FAKE_HIP_MISSING")) {          // kernels this "code object" lacks: name,name,...
        const std::string all = std::string(",") + e + ",";
        if (all.find(std::string(",") + name + ",") != std::string::npos) { *f = nullptr; return 500; }
    }
    *f = (void*)&*g_names.insert(name).first;
    return 0;
}
int hipModuleLaunchKernel(void* f, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by, unsigned bz, unsigned lds, void* st, void** args, void**)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const std::string* name = nullptr;
    for (const std::string& n : g_names)
        if ((const void*)&n == f) name = &n;
    if (!name) return 98;                                       // hipErrorInvalidDeviceFunction: not a function of this module
    if (!g_log_on) return 0;
    std::string o = "launch " + *name + " grid=" + std::to_string(gx);
    if (gy != 1 || gz != 1) o += "x" + std::to_string(gy) + "x" + std::to_string(gz);
    o += " block=" + std::to_string(bx);
    if (by != 1 || bz != 1) o += "x" + std::to_string(by) + "x" + std::to_string(bz);
    o += " lds=" + std::to_string(lds) + " " + handle_name(g_streams, st, 's');
    const bool voxel = starts(*name, "hare_voxel_"), octree = starts(*name, "hare_octree_"), kd = starts(*name, "hare_kdtree_");
    if ((voxel || octree || kd) && args) {
        // (the argument array and the structs behind it are the library's own host memory)
        if (voxel) o += " " + decode(*(const VoxelArgs*)args[0]);
        if (octree) o += " " + decode(*(const OctreeArgs*)args[0]);
        if (kd) o += " " + decode(*(const KdArgs*)args[0]);
        o += " " + decode(*(const ShootIO*)args[1]);
        if (*name == "hare_octree_pool") o += " scratch=" + ptr_name(*(void**)args[2]) + " stride=" + std::to_string(*(unsigned*)args[3]);
    }
    if (*name == "hare_hist_reduce") o += " " + decode(*(const ReduceArgs*)args[0]);
    if (*name == "hare_hist_project") o += " " + decode(*(const ProjectArgs*)args[0]);
    if (*name == "hare_hist_render") o += " " + decode(*(const RenderArgs*)args[0]);
    log_line(o);
    return 0;
}
const char* hipGetErrorString(int e) { return e == 0 ? "no error" : (e == 2 ? "out of memory" : "fake HIP error"); }
int hipGetLastError(void) { return 0; }
int hipEventCreateWithFlags(void** e, unsigned)
{
    std::lock_guard<std::mutex> lk(g_mu);
    *e = (void*)(g_next_handle += 16);
    g_events.push_back(*e);
    return 0;
}
int hipEventCreate(void** e) { return hipEventCreateWithFlags(e, 0); }
int hipEventDestroy(void* e)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_events.erase(std::remove(g_events.begin(), g_events.end(), e), g_events.end());
    return 0;
}
int hipEventRecord(void* e, void* st)
{
    std::lock_guard<std::mutex> lk(g_mu);
    log_line("record " + handle_name(g_events, e, 'e') + " " + handle_name(g_streams, st, 's'));
    return 0;
}
int hipEventSynchronize(void*) { return 0; }
int hipStreamWaitEvent(void* st, void* e, unsigned)
{
    std::lock_guard<std::mutex> lk(g_mu);
    log_line("wait " + handle_name(g_events, e, 'e') + " " + handle_name(g_streams, st, 's'));
    return 0;
}
int hipEventElapsedTime(float* ms, void*, void*) { *ms = 0; return 0; }

}  // extern "C"
