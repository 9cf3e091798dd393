// launch.h -- declarations shared by api.cpp (the C-ABI), launch.cpp (kernel choice + launches) and device_scene.cpp (what a scene keeps
// on its device).  Product code; nothing from oracle/.
#pragma once
#include <algorithm>
#include <string>

#include "../../include/hare_hip.h"
#include "scene.h"
#include "fan_out.h"

namespace hare {

// a HIP call that must succeed: sets the thread-local message and returns HARE_E_NOMEM / HARE_E_HIP from the enclosing function
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            set_error(std::string(#expr) + " failed: " + (H->GetErrorString ? H->GetErrorString(_e) : "?")); \
            (void)H->GetLastError();                                                           \
            return (_e == hipErrorOutOfMemory) ? HARE_E_NOMEM : HARE_E_HIP;                    \
        }                                                                                      \
    } while (0)

constexpr unsigned kLdsMax = 160u * 1024u;
#ifndef HARE_K2P_WAVES_PER_EU
#define HARE_K2P_WAVES_PER_EU 4
#endif
#ifndef HARE_K2D_WAVES_PER_EU
#define HARE_K2D_WAVES_PER_EU 3      // K2d and the flags-only build of it (kernels.hip): 168 registers, nothing spilled
#endif
#ifndef HARE_OCCL_WAVES_PER_EU
#define HARE_OCCL_WAVES_PER_EU 4     // what the voxel occlusion build is compiled for (kernels.hip)
#endif

// ---- the sizes the launcher, the name query and the build-time reservations share: ONE definition each (kd_dense_lds: hare_device.h)
// a bitmap of `words` words as the kernels stage it in LDS: padded to 16 bytes (the occupancy bitmap: <= 64 KB, occ_layout)
constexpr unsigned bitmap_lds(long long words) { return (unsigned)((words + 3) / 4) * 16u; }
// K1q's dynamic LDS: the occupancy bitmap and the pools; the fused bounce build adds its per-wave block, "voxel_skip" its block bits
inline unsigned pool_lds(const Scene& s, bool bounce = false, int32_t bocc_words = 0)
{
    return bitmap_lds(s.occ_words) + (unsigned)kPoolWaves * (unsigned)(kPoolWaveBytes + (bounce ? kPoolBounceExtra : 0)) + (bocc_words > 0 ? bitmap_lds(bocc_words) : 0u);
}
// the pool kernel K1q can serve this grid: ct <= 512, bitmap + pools fit LDS
inline bool pool_can_serve(const Scene& s) { return pool_lds(s) <= kLdsMax && s.vox.ct <= 512; }
// K2p / K2d: 20 bytes x levels x 256 lanes per workgroup (interval + child word); the dense build: + its pending survivors and tables
constexpr unsigned oct_persist_lds(int levels, bool dense) { return (unsigned)levels * 256u * 20u + (dense ? kOctDenseExtra : 0u); }
// K2g: workgroups of four waves, the groups' stacks and pending lists (hare_device.h).  A ray's stack can hold 7 x levels + 8 entries (the
// reference's LIFO, "Octree - alt.cs":268-272); what LDS does not hold spills to a block of the scene's octree scratch ring
constexpr unsigned kGroupLds = 4u * (unsigned)kGroupWaveBytes;
constexpr int group_spill_entries(int levels) { return 7 * levels + 8 - kGroupStack > 0 ? 7 * levels + 8 - kGroupStack : 0; }
// bytes of one K2p -> tail hand-over record (OctTailRec + 20 bytes per level, padded to 16)
constexpr size_t oct_tail_stride(int levels) { return ((size_t)kOctTailHead + 20u * (size_t)levels + 15u) & ~(size_t)15u; }

// Octree launches get a block of the scene's octree scratch ring (one block per launch in flight, event-ordered):
//   tail_levels > 0     a K2p launch: hand-over records for the rays its waves give up (tail_max per wave), followed on the same
//                       stream, inside the slot's lock, by the tail kernel -- K2t (octree_coop.hip: a wave per ray, the last few
//                       rays of a wave) or K2g-tail (octree_group.hip: eight lanes per ray, ALL the rays a wave still holds when
//                       the tickets run dry)
//   spill_entries > 0   K2g's stack entries beyond what LDS holds (24 bytes x entries per group of eight lanes), for the K2g
//                       launch itself or for the K2g-tail behind K2p
struct OctScratch {
    int tail_levels = 0;
    int tail_max = 0, tail_patience = 0;
    bool group_tail = false;
    int spill_entries = 0;
};
// What a launch (grid x block) with that request takes of a scratch block, and the tail kernel's grid.  with_tail: a tail kernel follows
// (launch_on_slot: the option "coop_tail" and the kernel's presence; reserve_oct_scratch: the request asks for one)
struct OctBlock {
    unsigned tail_grid = 0;
    size_t stride = 0, rec_bytes = 0, spill_bytes = 0;
    size_t bytes() const { return rec_bytes + spill_bytes; }
};
inline OctBlock oct_scratch_block(unsigned grid, unsigned block, const OctScratch& oc, bool with_tail, unsigned cus)
{
    OctBlock b;
    // the tail kernel's grid: K2t a wave per ray of a typical hand-over; K2g-tail a chip full of groups (waves without a record end at once)
    b.tail_grid = !with_tail ? 0u : (oc.group_tail ? cus * (unsigned)HARE_K2G_WAVES_PER_EU : std::max(1u, std::min(grid, 4u * cus)));
    const unsigned spill_groups = oc.spill_entries <= 0 ? 0u : (with_tail && oc.group_tail ? b.tail_grid * 4u * 8u : grid * (block / 64u) * 8u);
    b.stride = !with_tail ? 0 : oct_tail_stride(oc.tail_levels);
    b.rec_bytes = !with_tail ? 0 : (((size_t)grid * (block / 64u) * (size_t)oc.tail_max * b.stride + 255u) & ~(size_t)255u);
    if (!oc.tail_levels || (with_tail && oc.group_tail)) b.spill_bytes = (size_t)spill_groups * (size_t)oc.spill_entries * 24u;
    return b;
}

// ---- device_scene.cpp
int get_module(const HipApi* H, int device, const DeviceModule** out);
int upload_cell_boxes(Scene& s, const HipApi* H);        // the voxels' tight boxes: only where they are used; never an error when they cannot be had
void upload_block_occ(Scene& s, const HipApi* H);        // option "voxel_skip": the block-level occupancy (device_scene.cpp)
void reserve_order_ring(Scene& s, const HipApi* H);      // the pool kernel's order ring (scene.h), sized by "voxel_order_max_rays"; called with every voxel build
void reserve_oct_scratch(Scene& s, const HipApi* H);     // the octree kernels' scratch ring, sized once for the largest launch the tree can get
int sync_partition_to_device(Scene& s, int kind);        // after a build: records, lists, tight boxes, kd device nodes

// ---- launch.cpp
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb);     // [a, a + na) and [b, b + nb) share a byte
void read_env_options(SceneOptions& o);
size_t voxel_scene_bytes(const Scene& s, size_t top);
enum class Kern { VoxelSimple, VoxelCount, VoxelAudit, VoxelProf, VoxelPool, VoxelBounce, VoxelPersist, VoxelOccl, OctSimple, OctCount, OctPool, OctPersist, OctDense,
                  OctGroup, OctOccl, KdSimple, KdCount, KdDense, None };
// The launch plan of one shoot: which kernel serves the batch (the fall-backs included: kernel missing from the code object, LDS that does not
// fit) and what its launch is made of.  Filled by plan_shoot (launch.cpp) from the scene, its options, the module, n and the flags alone, for the
// launchers, for hare_shoot_kernel_name (the name a profile is read by is the kernel that ran) and for reserve_oct_scratch (the ring holds what a
// launch will ask for).  f == nullptr with k != None: the kernel is missing; k == None: HARE_SHOOT_COUNT_OWN where no counting build exists.
struct ShootPlan {
    Kern k = Kern::None;
    const char* name = "";
    hipFunction_t f = nullptr;
    bool oct_dense = false;            // K2d, its counting build or its flags-only build: K2d's LDS and waves per SIMD
    unsigned grid = 0, block = 0, lds = 0;
    int32_t ticket_rays = 0, static_rays = 0, walk_steps = 0;      // ShootIO's fields of the same names (0: the kernel does not read it)
    int32_t refill_min_idle = 16;
    OctScratch oc;                     // the octree kernels' request to the scratch ring
};
// `M` may be null (no device yet): the rule alone, for a 256-CU part.  bounce_casts > 0: the plan of hare_bounce_device's ONE launch of
// `bounce_casts` casts (Kern::VoxelBounce) where the fused loop serves, else the plan of one cast.  Pure: no allocation, no lock, no device
ShootPlan plan_shoot(const Scene& s, const DeviceModule* M, int32_t kind, size_t top, int64_t n, uint32_t flags, bool flags_only = false, int32_t bounce_casts = 0);
int32_t voxel_block_bits_words(const Scene& s, size_t top);      // words of the "voxel_skip" block bits the pool kernel stages for this topology (0: none)

// The device prelude of a C-ABI call behind its checks (receive.cpp, hist.cpp): no exception out, the HIP runtime bound (HARE_E_NODEVICE),
// the scene's device current for the call and its module loaded; then body(H), whose code is the call's
template <class Body>
int device_call(Scene& s, Body body)
{
    GUARD_BEGIN
    const HipApi* H = api_or_err();
    if (!H) return HARE_E_NODEVICE;
    DeviceGuard dev_guard(H, s.device);
    if (!s.module) {
        int rc = ensure_device(s, H);
        if (rc) return rc;
    }
    return body(H);
    GUARD_END
}

}  // namespace hare
