/*
 * hare_hip.h -- C-ABI of libhare_hip.so: the MI355X (gfx950) implementation of Hare's ray-cast
 * hot path, Spatial_Partition.Shoot.
 *
 * The reference (PachydermAcoustic/Hare, C#) has NO native boundary; its seam is the abstract
 * class Hare.Geometry.Spatial_Partition (Spatial_Partition.cs:27-35).  A drop-in is a C# class
 * deriving from it that P/Invokes the functions below (bindings/csharp/).  Each
 * entry point names the reference member it stands in for (file:line into the reference).
 *
 * Conventions
 *   - extern "C", cdecl, plain pointers and sizes; no C++/torch types cross this boundary.
 *   - every function returns HARE_OK (0) or a negative HARE_E_* code; the message of the last
 *     failure on the calling thread is hare_last_error().  No exception crosses the ABI.
 *   - the caller owns every host buffer; the library never keeps a host pointer after a call
 *     returns.  Everything behind hare_scene* belongs to the library until hare_scene_destroy.
 *   - per-ray conditions (origin outside the grid, NaN direction, ...) are not errors: they give
 *     the miss record X_Event() (Hare_Geometry_Primitives.cs:454-462).
 *   - threading: build/destroy calls are single-caller; hare_shoot_batch may be called from
 *     several host threads on one scene: up to four calls run side by side, each on its own
 *     staging buffers and streams, further callers wait for a free set (what the reference's
 *     Ray.ThreadID / mailbox pool serve, Voxel_Grid.cs:334-342); hare_shoot_device is
 *     stream-ordered: it enqueues and returns -- no allocation, no free, no wait on the device, a stream
 *     or an event on the host (every scratch it uses was reserved when the partition went to the device;
 *     hare_scene_get_option "hip_malloc_calls" ... let a caller check).  What it does take, for the few
 *     enqueues of one call, is the mutex of the launch slot (and scratch block) the call uses: calls from
 *     several threads contend only when they draw the same slot of the ring.  hare_shoot_one takes no lock.
 *   - devices: every call acts on the scene's own device and leaves the calling thread's current
 *     HIP device as it found it.
 *   - batches have NO CPU fallback: hare_shoot_batch / hare_shoot_device run the HIP kernels and fail
 *     with HARE_E_NODEVICE when no gfx950 device / HIP runtime is available.  The single-ray call
 *     hare_shoot_one -- Spatial_Partition.Shoot exactly as the reference exposes it -- runs on the
 *     calling host thread (a GPU round trip per ray would be ~100x slower than the reference).
 */
#ifndef HARE_HIP_H
#define HARE_HIP_H

#include <stdint.h>

#if defined(__GNUC__)
#define HARE_API __attribute__((visibility("default")))
#else
#define HARE_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define HARE_OK 0
#define HARE_E_INVALID (-1)     /* bad argument                                   */
#define HARE_E_NOMEM (-2)       /* host or device allocation failed               */
#define HARE_E_HIP (-3)         /* a HIP runtime call failed                      */
#define HARE_E_NODEVICE (-4)    /* no HIP runtime / no usable GPU                 */
#define HARE_E_STATE (-5)       /* partition not built, scene not uploaded, ...   */
#define HARE_E_UNSUPPORTED (-6) /* e.g. polygon with more than 4 corners          */

/* Which Spatial_Partition subclass a shoot goes through */
#define HARE_KIND_VOXEL 0   /* Voxel_Grid  (Voxel_Grid.cs)       */
#define HARE_KIND_OCTREE 1  /* Octree      ("Octree - alt.cs")   */
#define HARE_KIND_KDTREE 2  /* KDTree      (KDTree.cs)           */

/* hare_shoot_* flags */
#define HARE_SHOOT_WRITEBACK_ORIGIN 1u /* also apply AABB.Intersect's origin move to rays[] (AABB_Main.cs:254-257) */
#define HARE_SHOOT_COUNT_WORK 2u       /* fill cells/entries/tests of hare_counters (slower diagnostic kernel)       */
#define HARE_SHOOT_SIMPLE_KERNEL 4u    /* voxel: one-ray-per-lane kernel instead of the persistent one (A/B testing) */
#define HARE_SHOOT_RETIRED_RAYS 8u     /* hare_shoot_device only (the bounce loop): poly_origin1 == -2 marks a ray that     */
                                       /* hare_reflect_device retired -> miss record, no traversal, not counted.  Without    */
                                       /* it -- and always in the host-buffer calls -- a negative poly_origin matches no      */
                                       /* polygon, as in the reference (Voxel_Grid.cs:477 compares indices only)              */

#define HARE_SHOOT_SLIM_EVENTS 16u     /* hare_shoot_batch / _sharded only: `out` receives slim records (below) instead of X_Events:   */
                                       /* 16 bytes per ray come back over the host link instead of 56.  Not together with                 */
                                       /* HARE_SHOOT_WRITEBACK_ORIGIN (HARE_E_INVALID): hare_expand_events redoes the origin move from    */
                                       /* the rays as they were passed in, which the write-back would have overwritten                   */

#define HARE_SHOOT_COUNT_OWN 64u       /* measurement: run the COUNTING BUILD of the production kernel the batch would get (the pool kernel of   */
                                       /* Voxel_Grid, hare_octree_dense, the kd-tree kernel) -- same events, slower -- and fill hare_counters     */
                                       /* with the work THAT kernel did: cells = voxels walked into / node records fetched, entries = list         */
                                       /* entries scanned, reserved[0] = candidates pre-culled, tests = exact polygon tests.  (COUNT_WORK counts   */
                                       /* the REFERENCE algorithm's work with a diagnostic kernel.)  HARE_E_UNSUPPORTED for a batch another        */
                                       /* kernel would serve.  No reference counterpart                                                            */
#define HARE_SHOOT_BOUNCE_LOOP 32u     /* hare_shoot_kernel_name only: name the kernel hare_bounce_device (<= 16 casts) launches for n rays           */
#define HARE_RECEIVE_DIFFUSE_RAIN 128u /* hare_receive_device / _batch / _batch_sharded only: diffuse rain ("receivers", "Diffuse rain", below)    */
#define HARE_RECEIVE_DIRECTIONAL 256u  /* the same three calls only: four channels per histogram word, W X Y Z ("receivers", "Directional", below) */
#define HARE_RECEIVE_TIME_LIMIT 512u   /* the same three calls only: a ray whose path has passed the histogram's end is retired ("receivers", "Termination")  */
#define HARE_RECEIVE_DIRECT 1024u      /* hare_receive_source / _sharded / _reduced and hare_receive_device only: the direct sound is deposited once per  */
                                       /* receiver, visibility-tested, and cast 0's receiver step is skipped ("receivers", "Direct sound")               */
#define HARE_RECEIVE_IMAGE 2048u       /* the same calls only: the first-order specular reflections are deposited once per (receiver, polygon) pair,      */
                                       /* visibility-tested, and cast 1's receiver step is skipped for the rays that left cast 0 specularly               */
                                       /* ("receivers", "Image sources (first order)").  The next bit, 0x1000, is the first developer bit                 */
#define HARE_RECEIVE_IMAGE2 65536u     /* the same calls, and only together with HARE_RECEIVE_IMAGE: the second-order specular reflections are deposited   */
                                       /* once per (receiver, polygon, polygon) path and cast 2's receiver step is skipped for the rays reflected          */
                                       /* specularly twice ("receivers", "Image sources (second order)").  0x10000: the first bit above the developer      */
                                       /* bits 0x1000 .. 0x8000 (0x8000 is the cull audit), below the internal bits 0x40000 and 0x80000                    */
#define HARE_RECEIVE_ORDER2 131072u    /* wherever HARE_RECEIVE_DIRECTIONAL is accepted, and only together with it: nine channels per histogram word,      */
                                       /* ambisonic orders 0..2 ("receivers", "Higher orders").  0x20000                                                   */
#define HARE_RECEIVE_ORDER3 1048576u   /* the same, sixteen channels, orders 0..3; not together with HARE_RECEIVE_ORDER2.  0x100000: the first bit above   */
                                       /* the internal bits 0x40000 and 0x80000                                                                            */

/* Hare.Geometry.Ray (Hare_Geometry_Primitives.cs:393-429): origin + direction.  Ray_ID/ThreadID
 * only serve the reference's mailbox pool and are not needed here. 48 bytes. */
typedef struct hare_ray {
    double x, y, z;
    double dx, dy, dz;
} hare_ray;

/* Hare.Geometry.X_Event (Hare_Geometry_Primitives.cs:435-481). 56 bytes.
 * Miss == X_Event(): t=u=v=0, X_Point null (0,0,0 here), Poly_id=-1, Hit=false. */
typedef struct hare_xevent {
    double t, u, v;
    double x, y, z;   /* X_Point */
    int32_t poly_id;  /* Poly_id */
    int32_t hit;      /* Hit     */
} hare_xevent;

/* Slim result records (HARE_SHOOT_SLIM_EVENTS): what an X_Event holds that the caller cannot recompute.
 *   X_Point is R.origin + R.direction * t by the reference's own expression (Hare_Geometry_Polygons.cs:652): evaluated by the
 *   caller in double precision without fusing it gives the same bits; Voxel_Grid.Shoot returns u = v = 0 (Voxel_Grid.cs:696-697).
 *   Voxel_Grid: hare_slim_event, 16 bytes.  hit = 1: t is X_Event.t and X_Point = o + d * t.  hit = 2: the ray started outside
 *   the grid and AABB.Intersect moved its origin (AABB_Main.cs:254-257): t is measured from the MOVED origin o'; X_Event.t =
 *   t + t_start and X_Point = o' + d * t -- hare_expand_events redoes the move and both sums bit for bit.
 *   Octree / KDTree: hare_slim_event_uv, 32 bytes (they return u, v; rays are never moved; hit is 0 or 1).
 * hare_expand_events turns n slim records back into full X_Events on the host (byte-identical to what the full call returns). */
typedef struct hare_slim_event {
    double t;
    int32_t poly_id;  /* -1 on a miss */
    int32_t hit;      /* 0 miss, 1 hit, 2 hit on a ray whose origin was moved (t from the moved origin) */
} hare_slim_event;
typedef struct hare_slim_event_uv {
    double t, u, v;
    int32_t poly_id;
    int32_t hit;
} hare_slim_event_uv;

/* Batch counters.  hits is what a multi-GPU run reduces across ranks. */
typedef struct hare_counters {
    uint64_t rays, hits;
    uint64_t cells;    /* grid cells / tree nodes visited (HARE_SHOOT_COUNT_WORK)           */
    uint64_t entries;  /* candidate-list entries scanned  (HARE_SHOOT_COUNT_WORK)           */
    uint64_t tests;    /* polygon tests performed; the GPU has no mailbox, so this counts   */
                       /* re-tests the reference's mailbox would skip                       */
    uint64_t reserved[3];
} hare_counters;

/* One Hare.Geometry.Topology as read back from the managed object:
 *   verts   = Model[m][poly, corner]          (Hare_Geometry_Topology.cs:418-424), P x 4 x 3 doubles,
 *             corner 3 ignored for triangles
 *   nverts  = Model[m].Polys[p].VertextCT     (Hare_Geometry_Polygons.cs:196), 3 or 4
 *   normals = Model[m].Normal(p)              (Hare_Geometry_Topology.cs:539), P x 3 doubles
 *   min/max = Model[m].Min / Model[m].Max     (Hare_Geometry_Topology.cs:50,58) after Finish_Topology() */
typedef struct hare_topology_desc {
    int32_t P;
    int32_t reserved;
    const double *verts;
    const int32_t *nverts;
    const double *normals;
    double min[3];
    double max[3];
} hare_topology_desc;

typedef struct hare_scene hare_scene;

/* ---- library / device ---- */
HARE_API const char *hare_version(void);
HARE_API const char *hare_last_error(void);
HARE_API int hare_device_count(int32_t *count);
/* Path of the HIP runtime the library bound to (diagnostics). */
HARE_API const char *hare_hip_runtime_path(void);

/* ---- helpers for hosts that do not go through the managed Topology ----
 * Polygon ctor normal (Hare_Geometry_Polygons.cs:159-171) and Finish_Topology bounds
 * (Hare_Geometry_Topology.cs:148-167), bit-identical to what the managed object would hold. */
HARE_API int hare_polygon_normals(const double *verts, const int32_t *nverts, int32_t P, double *normals_out);
HARE_API int hare_topology_bounds(const double *verts, const int32_t *nverts, int32_t P, double min_out[3], double max_out[3]);

/* Topology(Point[][]) ingest, for hosts that start from a raw polygon soup (Hare_Geometry_Topology.cs:120-142
 * ctor, :258-311 Build_Topology, :342-377 AddGetIndex; Point.Round / Point.Hash2
 * Hare_Geometry_Primitives.cs:230-250; MS_AABB Hare_Geometry_Topology.cs:677-697).  Every corner is rounded
 * with Math.Round(x, 15) and corners that fall into the same 1 mm Hash2 cell are merged onto the FIRST such
 * corner, in polygon order, exactly as the managed Topology does.
 *   soup           P x 4 x 3 corner coordinates (slot 3 ignored for triangles)
 *   verts_out      P x 4 x 3: the merged corner coordinates (unused slots zero) -- what hare_scene_create,
 *                  hare_polygon_normals and hare_topology_bounds expect
 *   corner_vertex  nullable, P x 4: index of each corner in Vertices_List order (-1 in unused slots)
 *   vertices_out   nullable, capacity sum(nverts) x 3: Vertices_List
 *   n_vertices_out nullable: length of Vertices_List
 * A polygon with nverts other than 3 or 4 is HARE_E_UNSUPPORTED (the reference throws NotImplementedException). */
HARE_API int hare_topology_ingest(const double *soup, const int32_t *nverts, int32_t P, double *verts_out,
                                  int32_t *corner_vertex, double *vertices_out, int32_t *n_vertices_out);

/* ---- scene = Spatial_Partition.Model (Spatial_Partition.cs:29) ----
 * Copies the topologies; `device` is the HIP device ordinal that will hold the scene. */
HARE_API int hare_scene_create(const hare_topology_desc *topos, int32_t n_topos, int32_t device, hare_scene **out);
HARE_API void hare_scene_destroy(hare_scene *s);

/* Diagnostics and A/B switches of ONE scene, for tests, profiling and tools; production callers never need them.  A scene takes
 * its defaults from the environment ONCE, inside hare_scene_create (HARE_BUILD=host; and, only in a process that opted in with
 * HARE_DEV=1, HARE_VOXEL_KERNEL = pool|persist, HARE_OCTREE_KERNEL = dense|group|persist|pool, HARE_TICKET, HARE_K1P_STATIC_RAYS, HARE_K2P_STATIC_RAYS,
 * HARE_BATCH_CHUNKS, HARE_OCTREE_TIGHT, HARE_VOXEL_TIGHT, HARE_TUNE): no call reads the environment afterwards.  Options:
 *   "build_host"      1: host builders even when a GPU is present (identical lists either way)
 *   "voxel_kernel"    0: the library's rule, 1: hare_voxel_persist_* (K1p), 2: hare_voxel_pool_* (K1q)
 *   "octree_kernel"   0: the library's rule (K2g below 81 920 rays on a 256-CU part -- 320 per CU --, K2d from there), 1: hare_octree_persist (K2p, one lane per ray),
 *                     2: hare_octree_pool (K2q), 3: hare_octree_group (K2g, eight lanes per ray), 4: hare_octree_dense (K2d: K2p with its leaf
 *                     entries spread densely over the wave and its exact tests deferred)
 *   "bounce_fused"    1: hare_bounce_device / hare_bounce_batch (last cast's events only) run a Voxel_Grid's bounce loop as ONE launch where they can; 0 (default): a launch per cast
 *   "bounce_pack"     1 (default): behind every reflection of a Voxel_Grid's launch-per-cast loop (last cast's events only) the blocks of 64 consecutive rays
 *                     in which a ray still lives are listed on the device, and the next cast walks that list: a cast costs nothing for rays retired in
 *                     whole blocks (open scenes: 72 -> 14 us per million retired rays).  One more one-workgroup launch per cast: 0 saves a closed room ~1 %
 *   "octree_tail"     what finishes the rays K2p's waves still walk at the end of a launch: 2 (default) hare_octree_group_tail (eight lanes per
 *                     ray, every ray a wave holds 32 rounds after its tickets ran dry), 1 hare_octree_tail (a wave per ray, a wave's last 16), 0 nothing
 *   "k2p_tail_max", "k2p_tail_patience"   the hand-over rule (0 / -1: the library's)
 *   "kdtree_kernel"   0 the library's rule (hare_kdtree_dense: persistent waves, one-line node records with both children's tight boxes,
 *                     leaves pre-culled densely, exact tests deferred), 1 hare_kdtree_shoot (one ray per lane: A/B baseline), 2 hare_kdtree_dense
 *   "ticket_rays", "k1p_static_rays" (both voxel kernels), "k2p_static_rays", "batch_chunks"   0: the library's rule, else the value
 *   "coop_tail"       1 (default): a wave that has drawn its last rays traces the last few with all 64 lanes (heavy rays); 0: off
 *   "wide_drain"      1 (default): the pool kernel spends the lanes its finished rays leave on the rays that remain (several lanes per
 *                     ray: its candidates four per lane, the occupied voxels ahead one per lane); 0: off.  Results never depend on it
 *   "voxel_walk"      1 (default): the pool kernel's DDA step loop (Voxel_Grid.cs:713-759) as written by hand for gfx950 -- the per-axis
 *                     updates under the axis' own EXEC mask; 0: the compiler's loop (A/B).  The same steps in the same order: results never depend on it
 *   "voxel_overlap"   1: a round of the pool kernel that holds enough rays for a cull task AND a walk task runs both: the cull's list
 *                     entries are requested first, the walk's step loops (LDS and VALU only) run while they are in flight, then the
 *                     cull consumes them; 0 (default): one phase per round -- the fused round was measured and is slower.  The option chooses the kernel (hare_voxel_pool_*_ov).  The same loads, the same operations per ray: results never depend on it
 *   "voxel_skip"      1: the pool kernel's walk crosses an EMPTY aligned block of 4 x 4 x 4 voxels in one operation -- the exact closed-form skip (the DDA as a
 *                     merge of three sequences of sequential adds): the same voxel, the same tMax bit patterns, the same results.  0 (default): it is
 *                     slower than the hand-written step on this hardware; kept as a tested option
 *   "octree_tight"    1 (default): the octree and kd-tree kernels drop a node whose subtree's polygons the ray cannot hit -- per node the box of
 *                     all polygons its subtree lists, built when the tree goes to the device; 0: every node the reference visits.  Results never
 *                     depend on it (an X_Event is the reference's bit for bit either way)
 *   "voxel_tight"     the same per voxel: a ray without a hit walks on past an occupied voxel whose polygons it cannot hit; 1 (default) / 0.
 *                     The boxes cost 32 B per voxel and topology and exist only while this is on and the pool kernel serves the grid (up to
 *                     512 voxels a side); switching it on later builds them then
 *   "voxel_order"     1 (default): the pool kernel takes the rays of a batch of primary rays (no exclusion arrays, from 1 572 864 rays), window by
 *                     window of 4 096, in the order of their estimated walk length -- a wave's rays then cost about the same; 0 never, 2 every
 *                     batch.  Rays and events stay where the caller has them; results never depend on it
 *   "voxel_order_max_rays"  the largest batch that pass serves (default 16 777 216): its scratch -- a ring of 4 blocks of that many 4-byte entries,
 *                     256 MiB by default -- is reserved when the grid goes to the device, so that no shoot ever allocates; a larger batch, a stream
 *                     under capture, or a failed reservation runs in the caller's order (same results).  0: no ring
 *   "voxel_tight_max_mb"  budget for those boxes in MiB (0, the default: none).  Over budget -- or out of device memory -- the grid is
 *                     built and traced without them: never an error, never a different result
 *   "receive_aggregate"  1 (default): hare_receive_reflect sums a wave's histogram adds per distinct (receiver, bin) before ONE atomic
 *                     instruction; 0: an atomic per detecting lane and band (A/B).  Results never depend on it
 *   "scatter_seed"    any int64 (default 0), read as uint64 bits: the seed S of the receive loop's scattering RNG ("receivers" below)
 *   "source_seed"     any int64 (default 0), read as uint64 bits: the seed S of the point source's directions ("receivers", "Source", below)
 *   "receive_floor_bits"  f = 0 (default: off) .. 1000: the receive loop's energy floor F = 2^-f ("receivers", "Termination", below)
 *   "receive_roulette"    0 (default) / 1: a ray under the floor plays Russian roulette instead of being retired outright (the same section)
 *   "dev"             1: developer flag bits of hare_shoot_* (timeline, phase profile, cull audit) pass
 * Single-caller like the build calls: not to be changed while shoots are in flight on the scene. */
HARE_API int hare_scene_set_option(hare_scene *s, const char *name, int64_t value);

/* Read an option back (any name hare_scene_set_option takes), or one of the read-only figures a host sizes its memory by:
 *   "voxel_tight_bytes"     device bytes the voxels' tight boxes take on this scene (32 B per voxel and topology; 0: none -- the option is
 *                           off, the grid is one the pool kernel does not serve, over "voxel_tight_max_mb", or their allocation failed:
 *                           the grid is then traced without them, same results)
 *   "voxel_order_bytes"     device bytes of the pool kernel's order ring (0: none -- "voxel_order" off, "voxel_order_max_rays" 0, a grid the
 *                           pool kernel does not serve, or the reservation failed)
 *   "hip_malloc_calls", "hip_free_calls", "hip_sync_calls"   process-wide counts of hipMalloc / hipFree / host-side waits (hipDeviceSynchronize,
 *                           hipStreamSynchronize, hipEventSynchronize) this library has made: a caller (or a test) can hold the stream-ordered
 *                           entry points to "none of these"
 *   "octree_scratch_bytes"  device bytes of the octree kernels' scratch ring (hand-over records and stack spill; 0 before the first
 *                           octree launch that needs one)
 *   "receivers", "bands"    K of hare_scene_set_receivers (0: none set) and B of topology 0's absorption / scattering tables (1: none);
 *   "bands:<top>"           B of topology <top> (e.g. "bands:1"; HARE_E_INVALID for a topology the scene does not have)
 *   "source", "source_bands", "source_res"   1 when hare_scene_set_source has set a source (0: none), its B and its table's R (0: no table)
 *   "edges", "edges:<top>"  E of hare_scene_set_edges for topology 0 and for topology <top> (0: no table)
 * No reference counterpart: Hare has no device memory to account for. */
HARE_API int hare_scene_get_option(const hare_scene *s, const char *name, int64_t *value);

/* ---- partition constructors ----
 * The voxel grid and the octree (of a single topology) are built on the GPU when one is present (environment
 * HARE_BUILD=host when the scene is created, or option "build_host", forces the host builders); both builders produce identical lists.  The KDTree is built on the host.
 * Voxel_Grid(Topology[] Model_in, int Domain)                      Voxel_Grid.cs:48-121  */
HARE_API int hare_voxel_build(hare_scene *s, int32_t domain);
/* Voxel_Grid(Topology[] Model_in, int MaxDomain, int Avg_polys)    Voxel_Grid.cs:128-254 */
HARE_API int hare_voxel_build_adaptive(hare_scene *s, int32_t max_domain, int32_t avg_polys);
/* Octree(Topology[] Model_In, int maxDepth, int maxPolygonsPerNode) "Octree - alt.cs":45-89
 * Several topologies: as the reference is written -- the root cube and the ids 0..P-1 of the LAST topology, binned by the
 * vertices of topology 0 (:63-88,123); the kd-tree's box grows over all topologies (KDTree.cs:67-87).  HARE_E_INVALID where
 * the reference would index out of range: a topology that gets split and has more polygons than topology 0 (at build), a
 * top_index whose topology has fewer polygons than the last one (at shoot). */
HARE_API int hare_octree_build(hare_scene *s, int32_t max_depth, int32_t max_polys);
/* KDTree(Topology[] Model_In, int maxDepth, int maxPolygonsPerNode) KDTree.cs:51-88 */
HARE_API int hare_kdtree_build(hare_scene *s, int32_t max_depth, int32_t max_polys);

/* ---- partition introspection (Voxel_Grid public members + what the parity tests compare) ---- */
typedef struct hare_voxel_info {
    int32_t ct;              /* VoxelCtX = VoxelCtY = VoxelCtZ                          */
    int32_t n_topos;
    double obox_min[3];      /* MinPt (Voxel_Grid.cs:785-791)                            */
    double obox_max[3];
    double box_dims[3];      /* Xdim / Ydim / Zdim (Voxel_Grid.cs:763-783)               */
    double voxel_dims[3];
    double char_step;        /* Spatial_Partition.Char_Step (Spatial_Partition.cs:31)    */
    uint64_t total_items;    /* sum of Voxel_Inv[x,y,z,m].Count over the grid, topology 0 */
    int32_t built_on_device; /* 1: lists came from the GPU builder, 0: from the host builder  */
    int32_t reserved;
} hare_voxel_info;
HARE_API int hare_voxel_get_info(const hare_scene *s, hare_voxel_info *out);
/* Voxel_Inv[x,y,z,top] (Voxel_Grid.cs:33) as CSR: cell = (x*ct + y)*ct + z; cell_start has
 * ct^3 + 1 entries, items has cell_start[ct^3] entries (ascending polygon index per cell).
 * items may be NULL to fetch cell_start only (its last entry sizes the items buffer). */
HARE_API int hare_voxel_get_lists(const hare_scene *s, int32_t top_index, uint32_t *cell_start, int32_t *items);

typedef struct hare_tree_info {
    int32_t n_nodes;
    int32_t max_depth;
    int32_t max_polys;
    int32_t built_on_device;    /* 1: the membership tests ran on the GPU (octree); same arrays either way */
    uint64_t total_items;
} hare_tree_info;
HARE_API int hare_octree_get_info(const hare_scene *s, hare_tree_info *out);
/* nodes in creation order (root, then each split's 8 children, depth-first):
 * boxes n x 6 (min xyz, max xyz), first_child (-1 = leaf), item_start/item_count into items */
HARE_API int hare_octree_get_nodes(const hare_scene *s, double *boxes, int32_t *first_child, int32_t *item_start,
                          int32_t *item_count, int32_t *items);
HARE_API int hare_kdtree_get_info(const hare_scene *s, hare_tree_info *out);
HARE_API int hare_kdtree_get_nodes(const hare_scene *s, double *boxes, double *split, int32_t *axis, int32_t *left,
                          int32_t *right, int32_t *item_start, int32_t *item_count, int32_t *items);

/* ---- Shoot ----
 * bool Shoot(Ray R, int top_index, out X_Event Ret_event)                                  Spatial_Partition.cs:32
 * bool Shoot(Ray R, int top_index, out X_Event Ret_event, int poly_origin1, int poly_origin2 = -1)   :33
 * for n rays at once.  excl1/excl2 (nullable) are poly_origin1/poly_origin2 per ray, -1 = none.
 * rays is read (and, with HARE_SHOOT_WRITEBACK_ORIGIN, updated like the reference mutates R).
 * Host buffers; the call copies to the scene's device, runs the kernel and copies back.  With HARE_SHOOT_SLIM_EVENTS `out` is
 * an array of n hare_slim_event (Voxel_Grid) or hare_slim_event_uv (Octree, KDTree) instead of n hare_xevent. */
HARE_API int hare_shoot_batch(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, hare_ray *rays,
                     const int32_t *excl1, const int32_t *excl2, uint32_t flags, hare_xevent *out,
                     hare_counters *ctr /* nullable */);

/* Slim records -> X_Events, on the calling host thread(s): `slim` is what a HARE_SHOOT_SLIM_EVENTS call on `s` wrote for `rays`
 * (the rays as they were passed in), kind as in that call.  Needs no GPU. */
HARE_API int hare_expand_events(const hare_scene *s, int32_t kind, int64_t n, const hare_ray *rays, const void *slim,
                                hare_xevent *out);

/* The same call over several devices of one node from ONE process (hosts without torch.distributed, e.g. the
 * .NET shim): scenes[k] is the scene on device k's ordinal of choice -- same topologies, same partition, built by
 * the caller with hare_scene_create(..., device_k, ...) + hare_*_build -- and rays [n*k/G, n*(k+1)/G) go to it
 * (the contiguous split of SURVEY.md 8(e); scene replicated, no exchange between devices).  One host thread per
 * scene drives its copies and kernel; outputs land in the same slices of `out`, so the result is byte-identical
 * to the one-device call; `ctr` is the sum over devices.  The first failing shard's code and message are returned. */
HARE_API int hare_shoot_batch_sharded(hare_scene *const *scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                                      hare_ray *rays, const int32_t *excl1, const int32_t *excl2, uint32_t flags,
                                      hare_xevent *out, hare_counters *ctr);

/* Same with DEVICE pointers on the scene's device and a caller stream (hipStream_t as void*,
 * NULL = default stream); stream-ordered, does not synchronise.  d_counters (nullable) points to
 * a device hare_counters that the kernel ACCUMULATES into.  Calls may be issued from several host
 * threads and on several streams; the scene keeps per-launch scratch (work tickets, counter shards) in a ring of
 * 64 slots: the 65th launch in flight is ordered behind the first (it waits for an event that launch recorded), so any
 * number of launches may be queued.  The same holds for the scratch rings some launches use beside it (the pool kernel's ray
 * order: 4 blocks; the octree kernels' hand-over records and stack spill: 8): a block's next user waits ON ITS STREAM for the event the previous
 * one recorded.  Under stream capture the order pass is skipped (results unchanged).  rays, the exclusion arrays, events and counters
 * must not overlap (HARE_E_INVALID). */
HARE_API int hare_shoot_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, void *d_rays,
                      const void *d_excl1, const void *d_excl2, uint32_t flags, void *d_out,
                      void *d_counters, void *stream);

/* Name of the gfx950 kernel a hare_shoot_device / hare_shoot_batch call with these arguments launches (for profiles:
 * rocprofv3 lists kernels by this name).  The voxel path has two production kernels and picks by batch size. */
HARE_API const char *hare_shoot_kernel_name(const hare_scene *s, int32_t kind, int32_t top_index, int64_t n, uint32_t flags);

/* ---- Shoot, one ray (unchanged reference call sites) ----
 * bool Shoot(Ray R, int top_index, out X_Event Ret_event, int poly_origin1 = -1, int poly_origin2 = -1)
 * (Spatial_Partition.cs:32-33; Voxel_Grid.cs:351,561; "Octree - alt.cs":154; KDTree.cs:193) for ONE ray, on the calling
 * host thread: the same trace the simple HIP kernels run (hare_amd/csrc/hare_trace.h), instantiated for the host over a
 * host mirror of the scene that is built on first use.  Results are bit-identical to the batch calls.  *ray is
 * updated like the reference mutates R when the origin lies outside the grid (AABB_Main.cs:254-257).  Needs no GPU;
 * lock-free, callable concurrently from any number of threads (no mailbox: SURVEY.md F7).  out->hit is the return
 * value of the reference's Shoot. */
HARE_API int hare_shoot_one(hare_scene *s, int32_t kind, int32_t top_index, hare_ray *ray, int32_t poly_origin1,
                            int32_t poly_origin2, hare_xevent *out);

/* ---- occlusion predicate (harness-defined, SURVEY.md F13 / 8(a) A9: the reference has no any-hit API; the seam it
 * would sit beside is Spatial_Partition.cs:32-33) ----
 * occluded[i] = Shoot(rays[i]) hit something AND that closest hit has t < tmax[i]  (tmax NULL: any hit counts).
 * Defined on the CLOSEST hit the reference's Shoot would return, so that it is pinned by the same oracle as Shoot, including
 * the reference's miss-on-grid-exit rule (Voxel_Grid.cs:716-757) and the octree's early return ("Octree - alt.cs":233).
 *   events != NULL   the closest-hit cast as hare_shoot_*, the X_Events returned, the flags derived from them
 *   events == NULL   flags only, from kernels that stop a ray as soon as its flag is decided: the voxel walk ends when it has
 *                    passed t_max without a hit below it pending (the pending-hit confirmation of Voxel_Grid.cs:705-709 is
 *                    kept: a hit counts when the reference would return it); the octree walk ends at the first hit below
 *                    t_max (no node is skipped for lying beyond t_max: with the reference's far-to-near order and early
 *                    return that would change which hit is "the" hit); the kd-tree walk ends at the first accepted hit below
 *                    t_max and never enters a subtree whose tight box the ray reaches at or beyond t_max (KDTree.Shoot returns
 *                    the smallest accepted t over ALL polygons, so "some polygon is accepted below t_max" is its flag).  The
 *                    flags are identical either way; the host call
 *                    then brings back 4 bytes per ray instead of 56.  counters: rays, and hits = number of occluded rays.
 * rays[] is never written. */
HARE_API int hare_occluded_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, void *d_rays,
                                  const void *d_excl1, const void *d_excl2, const void *d_tmax /* n doubles, nullable */,
                                  uint32_t flags, void *d_events /* n x 56 B, nullable */, void *d_occluded /* n int32 */,
                                  void *d_counters, void *stream);
HARE_API int hare_occluded_batch(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, hare_ray *rays,
                                 const int32_t *excl1, const int32_t *excl2, const double *tmax /* nullable */,
                                 uint32_t flags, int32_t *occluded, hare_xevent *events /* nullable */,
                                 hare_counters *ctr /* nullable */);
/* the same over several devices from one process (contiguous ray shards, as hare_shoot_batch_sharded) */
HARE_API int hare_occluded_batch_sharded(hare_scene *const *scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                                         hare_ray *rays, const int32_t *excl1, const int32_t *excl2, const double *tmax,
                                         uint32_t flags, int32_t *occluded, hare_xevent *events, hare_counters *ctr);

/* ---- specular bounce (harness-defined; the reference leaves reflection to its caller, which
 * re-shoots with poly_origin1 = the previous Poly_id -- Voxel_Grid.cs:351,477) ----
 * For every ray with events[i].hit: origin <- X_Point, direction <- d - (2*(d.n))*n with
 * n = Model[top].Normal(Poly_id), excl_out[i] <- Poly_id.  Rays that missed keep their record
 * and get excl_out[i] = -2 (dead: a later hare_shoot_device with HARE_SHOOT_RETIRED_RAYS reports a
 * miss for them immediately and does not count them).
 * Device pointers, stream-ordered. */
HARE_API int hare_reflect_device(hare_scene *s, int32_t top_index, int64_t n, void *d_rays, const void *d_events,
                        void *d_excl_out, void *stream);

/* ---- the bounce loop on DEVICE buffers, stream-ordered, no host synchronisation (harness-defined like hare_reflect_device) ----
 * `bounces` casts per ray: Shoot, reflect about Model[top].Normal(Poly_id) (Hare_Geometry_Polygons.cs:161-171), Shoot again with
 * poly_origin1 = the polygon just hit (Spatial_Partition.cs:33; Voxel_Grid.cs:351,477); a ray that misses is retired (its later
 * events are the miss record X_Event(), it is not counted).
 * By default `bounces` x (shoot + reflect) launches, retired rays skipped.  With the scene option "bounce_fused" = 1, a Voxel_Grid
 * wherever the pool kernel serves a batch, and bounces <= 16: ONE persistent launch (hare_voxel_bounce_*) in which every ray runs
 * through its casts on its own -- rays are independent across casts too, so no cast waits for the slowest ray of the one before.
 * Results are identical either way; measured on MI355X the single launch gains 2.5 % in the 100k-triangle hall and loses up to
 * 10 % in the 1M-triangle cathedral (profiles/r04_experiments/EXPERIMENTS.md), hence the default.
 *   d_rays               n rays: READ AND OVERWRITTEN (work array; every ray's last reflection remains)
 *   d_excl1 / d_excl2    nullable, read only: poly_origin1 / poly_origin2 of cast 0 (a negative index excludes nothing)
 *   d_work               scratch, 2 n int32
 *   d_events_all         nullable: bounces x n X_Events, cast-major
 *   d_events_last        the n X_Events of the last cast (nullable when d_events_all is given)
 *   d_counters           nullable: totals, ACCUMULATED (rays = casts with a live ray, hits)
 *   d_counters_per_cast  nullable: `bounces` hare_counters, ACCUMULATED (rays = rays alive in that cast, hits = rays that live on)
 *   flags                HARE_SHOOT_COUNT_WORK / HARE_SHOOT_SIMPLE_KERNEL only (either forces the launch per cast) */
HARE_API int hare_bounce_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, void *d_rays, const void *d_excl1,
                                const void *d_excl2, int32_t bounces, uint32_t flags, void *d_work, void *d_events_all,
                                void *d_events_last, void *d_counters, void *d_counters_per_cast, void *stream);

/* ---- the whole bounce loop behind one call, from host buffers (harness-defined like hare_reflect_device) ----
 * What a Pachyderm-style caller does per ray with the reference -- Shoot, reflect about Model[top].Normal(Poly_id)
 * (Hare_Geometry_Polygons.cs:161-171), Shoot again with poly_origin1 = the polygon just hit (Spatial_Partition.cs:33;
 * Voxel_Grid.cs:351,477) -- for n rays and `bounces` casts, device-resident: the rays go up once, every cast and every
 * reflection runs on the scene's GPU, and only the requested X_Events come down (the download of a cast overlaps the next cast).
 *   cast 0 shoots rays[] with excl1 / excl2 (nullable; poly_origin1 / poly_origin2 per ray as in hare_shoot_batch: a negative
 *   index excludes nothing); cast b > 0 shoots the reflections of the rays that hit in cast b - 1, excluding the polygon they
 *   left.  A ray that misses is retired: its X_Event in every later cast is the miss record X_Event(), and it is not counted.
 *   When a quarter or more of the rays in flight have died the survivors are packed (stably) and later casts run on them
 *   alone; their events are put back in the caller's order on the device.  Results do not depend on whether that happened.
 *   events_all     nullable: bounces x n records, cast-major (cast b at events_all + b * n)
 *   events_last    nullable: the n records of the last cast
 *   ctr            nullable: counters summed over the casts (rays = live casts)
 *   ctr_per_cast   nullable: `bounces` blocks, one per cast (rays = rays alive in that cast, hits = rays that live on)
 *   flags          HARE_SHOOT_COUNT_WORK / HARE_SHOOT_SIMPLE_KERNEL only; rays[] is never written
 * Threading as hare_shoot_batch (a staging context per call in flight, four per scene). */
HARE_API int hare_bounce_batch(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, const hare_ray *rays,
                               const int32_t *excl1, const int32_t *excl2, int32_t bounces, uint32_t flags,
                               hare_xevent *events_all, hare_xevent *events_last, hare_counters *ctr,
                               hare_counters *ctr_per_cast);
/* The same over several devices from one process: rays [n*k/G, n*(k+1)/G) go to scenes[k] (as hare_shoot_batch_sharded); every
 * shard keeps its rays resident on its own device for all casts; outputs are byte-identical to the one-device call. */
HARE_API int hare_bounce_batch_sharded(hare_scene *const *scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                                       const hare_ray *rays, const int32_t *excl1, const int32_t *excl2, int32_t bounces,
                                       uint32_t flags, hare_xevent *events_all, hare_xevent *events_last, hare_counters *ctr,
                                       hare_counters *ctr_per_cast);

/* ---- receivers: energy-time histograms from the bounce loop (harness-defined; the reference has no receivers -- Pachyderm, its
 * caller, intersects every reflected segment with its receivers on the host) ----
 * The scene holds receivers: K spheres (center c_k, radius r_k), with 1 <= K <= 256 (up to 65 536 as a map: "Receiver maps", below).  For each topology it may also hold an
 * absorption table: alpha[p][b], one value in [0, 1] per polygon p and band b, with 1 <= B <= 8 bands.  A topology with no table
 * acts as B = 1 with every alpha = 0.
 *
 * Every ray carries a state: a path parameter L and band energies E[0..B-1].  The loop is the bounce loop's: shoot, reflect about
 * Normal(Poly_id), exclude the polygon just left, and retire a ray that misses.  One step is added after each cast c (the last
 * cast included) and before that cast's reflection.  For every ray still live in cast c, it runs the ray through every receiver k
 * in ascending order.  Here o, d are the ray as cast c received it, e is its X_Event, and t_end = e.hit ? e.t : +inf (a miss is a
 * half-line).  All of it is FP64 with no contraction, in exactly this order:
 *
 *   wx = cx - ox; wy = cy - oy; wz = cz - oz
 *   s  = ((wx*dx + wy*dy) + wz*dz) / ((dx*dx + dy*dy) + dz*dz)
 *   qx = (ox + dx*s) - cx;  (same for y, z)
 *   detected  iff  s >= 0  &&  s < t_end  &&  ((qx*qx + qy*qy) + qz*qz) < r*r
 *   x   = (L + s) / bin_len            binned iff x >= 0 && x < n_bins (compared as doubles); bin = (int)floor(x)
 *   q_b = E[b] * 2^frac_bits; 0 unless q_b > 0; min(q_b, 2^63); rint -> uint64
 *   hist[(k*n_bins + bin)*B + b] += q_b            (uint64, wraps mod 2^64: the caller sizes frac_bits)
 *   detections[2k] += 1 if binned, detections[2k+1] += 1 otherwise
 *
 * After the receiver step, a ray that hit updates its state: E[b] = E[b] * (1.0 - alpha[Poly_id][b]) and L = L + e.t (in the last
 * cast too).  Then it is reflected as in the bounce loop (not behind the last cast).  A ray that missed is retired and its state is
 * left as it is.
 *
 * Scattering (diffuse, Lambertian).  A topology may also hold a scattering table: sigma[p][b], one value in [0, 1] per polygon and band.
 * It shares B with the topology's absorption table: whichever of the two is set first fixes B, and setting the other with a different B
 * is HARE_E_INVALID (absorption alone may still be replaced with a different B).  A topology with no scattering table reflects
 * specularly, as above.  With one, a ray that hit in cast c and will be reflected (never behind the last cast) chooses, after its
 * absorption update, between specular and diffuse.  FP64, no contraction; g is the ray's index in the call's `rays` (in the sharded call
 * the GLOBAL index, not the index in its shard), S the scene option "scatter_seed".  Integer arithmetic is uint64, wrapping mod 2^64:
 *
 *   G       = 0x9E3779B97F4A7C15
 *   mix(z)  = z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (SplitMix64's finaliser)
 *   base    = mix(mix(S + G) ^ g)
 *   u_j     = (double)(mix(base + (((uint64)c << 8) | j) * G) >> 11) * 2^-53          j = 0 .. 64, in [0, 1)
 *   p       = (((sigma[0] + sigma[1]) + ...) + sigma[B-1]) / (double)B                (left to right; sigma = sigma[Poly_id])
 *   diffuse = u_0 < p
 *   E[b]    = E[b] * (sigma[b] / p)                   if diffuse
 *   E[b]    = E[b] * ((1.0 - sigma[b]) / (1.0 - p))   otherwise
 *
 * (c < 4096 and j < 256: the word of each (c, j) is distinct.)  Each band's energy is unbiased in expectation; at p = 0 (an all-zero
 * row) no ray goes diffuse and every weight is exactly 1.  A specular ray is reflected as above.  A diffuse ray takes a cosine-distributed
 * direction (Malley's method in the branchless orthonormal basis of Duff et al. 2017):
 *
 *   n  = Normal(Poly_id); n' = dot3(d, n) > 0 ? -n : n                 (the side the ray came from: polygons are two-sided)
 *   for t = 0 .. 31: x = 2.0*u_{1+2t} - 1.0; y = 2.0*u_{2+2t} - 1.0; r2 = x*x + y*y; take the first with r2 < 1.0
 *                    (none taken: x = y = r2 = 0)
 *   z  = sqrt(1.0 - r2)
 *   sg = copysign(1.0, n'z); a = -1.0 / (sg + n'z); b = (n'x * n'y) * a
 *   t1 = (1.0 + ((sg * n'x) * n'x) * a,  sg * b,  -(sg * n'x));  t2 = (b,  sg + (n'y * n'y) * a,  -n'y)
 *   w_i = (x * t1_i + y * t2_i) + z * n'_i;  len = sqrt((dx*dx + dy*dy) + dz*dz);  d_out = (wx * len, wy * len, wz * len)
 *
 * from the X_Point, excluding Poly_id, as a specular ray does (|d_out| = |d|: L keeps its meaning).  The plain bounce loop is not affected.
 * Every call restarts c at 0: a device caller that splits one burst over several calls varies "scatter_seed" from call to call, or the
 * calls draw the same numbers.
 *
 * Diffuse rain (flag HARE_RECEIVE_DIFFUSE_RAIN; Heinz's diffuse rain, a form of next-event estimation).  Opt-in per call, and only on a
 * topology with a scattering table: without one the flag changes nothing.  At every hit that may go diffuse, the scattered share of the
 * energy goes straight to each receiver the hit point sees.  A ray takes part in cast c when it hit in cast c, c < bounces - 1 (it will be
 * reflected) and p > 0 (p as above).  Its rain comes after the receiver step and the absorption update, before the choice, with
 * x = X_Point, Ea[b] = E[b] after absorption, sg = sigma[Poly_id], n' the side normal above, len = sqrt((dx*dx + dy*dy) + dz*dz) of the
 * incoming direction, L' = L + e.t and rr the stored r*r; for each receiver k in ascending order, FP64, no contraction:
 *
 *   vx = cx - x.x; vy = cy - x.y; vz = cz - x.z
 *   d2 = (vx*vx + vy*vy) + vz*vz;  cs = (vx*n'x + vy*n'y) + vz*n'z
 *   eligible  iff  d2 > rr && cs > 0
 *   occluded  = the hare_occluded predicate on the shadow ray (origin x, direction v, poly_origin1 = Poly_id, t_max = 1.0):
 *               the closest hit has t < 1.0
 *   if eligible && !occluded:
 *     dist = sqrt(d2);  w = (cs / dist) * (rr / d2)
 *     xb   = (L' + dist / len) / bin_len                binned as in the receiver step
 *     q_b  = ((Ea[b] * sg[b]) * w) * 2^frac_bits        0 unless q_b > 0; min(q_b, 2^63); rint -> uint64
 *     hist[(k*n_bins + bin)*B + b] += q_b;  detections[2k] += 1 if binned, detections[2k+1] += 1 otherwise
 *
 * w is the sphere's projected solid angle over pi, the chance that a cosine-distributed direction from x passes through it.  It is exact
 * when the sphere lies wholly in front of the polygon's plane; for a sphere the plane cuts (near the horizon) it is an approximation.
 * Visibility is tested to the center only.  Suppression: a ray whose reflection in the previous cast was diffuse skips the receiver step
 * in this cast (no add, no detection) -- the rain has accounted for that segment.  Specular segments, and cast 0, detect as before.  The
 * flag is kept per ray in the rain's scratch and cleared at the start of every call; as the last cast of a call is never reflected, no
 * diffuse segment crosses from one call into the next.  Rain changes deposits only: the draws, choices, weights, directions, the final
 * state and rays are those of the call without it.  In a convex room whose receivers are clear of every wall plane by more than r, the
 * expected histogram total per band is the same with and without rain (the diffuse segment's hit probability there is exactly w); its
 * spread is smaller.  Cost: each reflecting cast runs K flags-only occlusion queries of n rays.
 *
 * Directional (flag HARE_RECEIVE_DIRECTIONAL; first-order, B-format).  Opt-in per call; it combines freely with HARE_RECEIVE_DIFFUSE_RAIN.
 * With the flag the histogram has four channels, channel innermost:
 *
 *   hist[((k*n_bins + bin)*B + b)*4 + ch]        ch 0 = W (omni), 1 = X, 2 = Y, 3 = Z        (K x n_bins x B x 4 uint64 words)
 *
 * Channel 0 is exactly the word the call writes without the flag.  Channels 1..3 are int64 in two's complement, added with the same
 * wrapping uint64 add.  For every add of the receiver step and of the rain above, with q_b as defined there and m_b the double that q_b
 * is the rint of (E[b] * 2^frac_bits, or in rain ((Ea[b] * sg[b]) * w) * 2^frac_bits; then 0 unless > 0; then min(., 2^63)), FP64, no
 * contraction:
 *
 *   receiver step:   len = sqrt((dx*dx + dy*dy) + dz*dz);   a = ( -(dx / len), -(dy / len), -(dz / len) )
 *   rain deposit:    a = ( -(vx / dist), -(vy / dist), -(vz / dist) )               (v, dist as in "Diffuse rain")
 *   v_i = m_b * a_i;   v_i = 0 unless v_i == v_i (NaN);   v_i = min(max(v_i, -2^62), 2^62);   s_i = (int64) rint(v_i)
 *   hist[... + 0] += q_b;   hist[... + 1 + i] += (uint64) s_i            i = 0, 1, 2
 *
 * a is the unit vector from the receiver towards where the sound came from, so a wave arriving from +x gives X > 0 (the ambisonic sign
 * convention); the channels are in world axes.  In the receiver step a is one vector per ray and cast, the same for every receiver.
 * sqrt and / are the correctly rounded FP64 ones.  What the caller has to know: frac_bits must leave a sign bit of headroom (the sums of
 * the signed channels must stay inside +-2^63, so size frac_bits for half the range the omni word alone would allow);
 * |hist[..., 1 + i]| as int64 never exceeds hist[..., 0] by more than the number of adds into that word (each rint moves a value by at most
 * 1/2); detections keep their shape and values; nothing about draws, choices, rays, state, suppression or detections changes.  d_hist of
 * the device call and hist of the host calls are four times as large, and the bound on the histogram becomes K x n_bins x B x 4 <= 2^27.
 *
 * Higher orders (flags HARE_RECEIVE_ORDER2 and HARE_RECEIVE_ORDER3; ambisonic orders 2 and 3).  Each is valid only together with
 * HARE_RECEIVE_DIRECTIONAL; either one without it, or both together, is HARE_E_INVALID, the first check of the call.  Each is accepted
 * wherever HARE_RECEIVE_DIRECTIONAL is -- hare_receive_device / _batch / _batch_sharded, hare_receive_source / _sharded, the two _reduced
 * calls, and the `flags` of hare_direct_device, hare_image_device and hare_image2_device -- and combines with diffuse rain, the
 * termination rules, receiver maps, HARE_RECEIVE_DIRECT, HARE_RECEIVE_IMAGE and HARE_RECEIVE_IMAGE2 as the first-order flag does.  The
 * histogram has C = 9 (order 2) or C = 16 (order 3) channels, channel innermost:
 *
 *   hist[((k*n_bins + bin)*B + b)*C + ch]        ch 0..3 = W, X, Y, Z;  ch 4..C-1 = ACN 4..C-1, SN3D        (K x n_bins x B x C uint64 words)
 *
 * Channels 0..3 are exactly those of "Directional": the same values as the call with HARE_RECEIVE_DIRECTIONAL alone.  Channels 4..15 are
 * the real spherical harmonics of orders 2 and 3 in ACN order and SN3D normalisation, evaluated on the same arrival vector
 * a = (x, y, z) -- the receiver step's, the rain deposit's, the direct deposit's or the image paths' last leg, each as it is defined in
 * its section.  They are polynomials of a: FP64, no contraction, in exactly this order, the six constants the correctly rounded doubles:
 *
 *   c3 = sqrt(3.0);  c3h = 0.5*c3;  c15 = sqrt(15.0);  c15h = 0.5*c15;  c58 = sqrt(0.625);  c38 = sqrt(0.375)
 *   xx = x*x;  yy = y*y;  zz = z*z;  d = xx - yy;  f = 5.0*zz - 1.0
 *   Y4  = c3*(x*y)      Y5  = c3*(y*z)     Y6  = 1.5*zz - 0.5     Y7 = c3*(x*z)     Y8 = c3h*d
 *   Y9  = c58*(y*(3.0*xx - yy))            Y10 = c15*((x*y)*z)    Y11 = c38*(y*f)   Y12 = z*(2.5*zz - 1.5)
 *   Y13 = c38*(x*f)     Y14 = c15h*(z*d)   Y15 = c58*(x*(xx - 3.0*yy))
 *   v = m_b * Y_ch;   v = 0 unless v == v (NaN);   v = min(max(v, -2^62), 2^62);   s_ch = (int64) rint(v);   hist[... + ch] += (uint64) s_ch
 *
 * with m_b as in "Directional".  What the caller has to know: |Y_ch| <= 1 up to rounding for a unit a, so the headroom rule of
 * "Directional" holds unchanged; order 2 of a call equals the first nine channels of order 3 of the same call; nothing about draws,
 * choices, rays, state, suppression or detections changes.  The bound on the histogram becomes K x n_bins x B x C <= 2^27.
 * hare_hist_reduce_device / hare_hist_reduce and the _reduced receive calls accept `channels` 9 and 16 and read word 0, as they do for 4.
 *
 * Termination (flag HARE_RECEIVE_TIME_LIMIT; scene options "receive_floor_bits" and "receive_roulette").  Two opt-in rules that retire a
 * ray before the call's `bounces` are spent.  Without the flag and with "receive_floor_bits" 0 nothing in this section applies.  Both are
 * decided in cast c for a ray that hit in cast c and would be reflected (c < bounces - 1), AFTER that cast's state update: after the
 * absorption update and, with a scattering table, after the scattering weights (and after the cast's rain, which deposits as before).
 * With L' = L + e.t and E[b] as that update leaves them, FP64, no contraction, in this order:
 *
 *   time limit (the flag):      retire  iff  (L' / bin_len) >= (double)n_bins          one division; a NaN L' is not retired
 *   energy floor (f > 0):       F = 2^-f (ldexp: exact)
 *     m = E[0];  for b = 1 .. B-1:  m = (E[b] > m) ? E[b] : m                          a NaN E[b] never replaces m; m = NaN: not below F
 *     if m < F:
 *       "receive_roulette" 0:   retire
 *       "receive_roulette" 1:   ps = m / F;  u = u_65 of the RNG above (cast c, word j = 65, base = mix(mix(S + G) ^ g) with g the GLOBAL
 *                               ray index and S = "scatter_seed" -- also on a topology without a scattering table)
 *                               u < ps:   the ray survives, E[b] = E[b] / ps for every b, and THAT is the state stored
 *                               else:     retire (the state stored is the undivided one)
 *
 * m <= 0 gives ps <= 0: such a ray never survives.  Word 65 is free (scattering draws j = 0 .. 64 and reserves j < 256).  The time limit
 * is tested first and a ray it retires draws nothing; as draws are per (g, c, j) this cannot be observed.
 * A ray a rule retires is treated as a ray that missed, but that its state update has happened and is stored: it is not reflected
 * (rays[i] stays as cast c received it), its mark becomes -2, its block counts as not live, its rain flag is not written, it takes part in
 * no later cast, and events_last holds the miss record for it, as for any ray retired before the last cast.
 * What the caller has to know.  Time limit: x = (L + s) / bin_len with s >= 0 only grows with L and rounding is monotone, so for hits
 * with t >= 0 every later x of a retired ray (the rain's xb too) is >= n_bins -- the histogram and detections[2k] are BYTE-IDENTICAL to
 * those of the same call without the flag, and as the RNG is per ray no other ray is affected.  Only detections[2k + 1], the final state,
 * the final rays, events_last and the counters differ.  Floor with roulette: every band's expected energy is kept (a ray survives with
 * probability ps and is then worth 1 / ps), at the price of variance in the late tail.  The plain floor is BIASED by design: it drops
 * what lies under F, at most F per ray and band.  Later casts run over the rays still live; the call makes no host round trip.
 *
 * Source (hare_scene_set_source; hare_emit_device, hare_receive_source / _sharded).  The scene may hold one point source: a position, a
 * power per band (B bands), and optionally a directivity table with the frame it is read in.  The source's rays and their starting state are
 * drawn on the device from a ray COUNT, bit-exact with a restatement on the host like everything else in the loop.  FP64, no contraction;
 * integers are uint64 and wrap; mix, G and u_j are those of "Scattering" above.  g = first_ray + i is the global index of ray i of a call, S
 * the scene option "source_seed" (any int64, default 0, read as uint64 bits like "scatter_seed"), and the counter is c = 4096 -- the casts
 * use c < 4096, so no word is shared with them even when both seeds are equal:
 *
 *   base = mix(mix(S + G) ^ g)
 *   for t = 0 .. 31: x = 2.0*u_{1+2t} - 1.0; y = 2.0*u_{2+2t} - 1.0; s = x*x + y*y; take the first with s < 1.0   (none taken: x = y = s = 0)
 *   h = sqrt(1.0 - s)
 *   d = ((2.0*x)*h, (2.0*y)*h, 1.0 - 2.0*s)            (Marsaglia 1972: uniform on the sphere; |d| = 1 up to rounding, not renormalised)
 *   ray = (pos, d);  L = 0;  E[b] = power[b] * gain_b(d)
 *
 * gain_b is 1.0 without a table.  With one it is a nearest-texel cube map of resolution R: table[6][R][R][B], band innermost, read in the
 * source's frame M (3 x 3, row-major; it need not be orthonormal):
 *
 *   l_i = (M[i][0]*dx + M[i][1]*dy) + M[i][2]*dz;  a_i = |l_i|                        i = 0, 1, 2
 *   f = 0; if (a_1 > a_f) f = 1; if (a_2 > a_f) f = 2                                 (ties and NaN keep the lower index)
 *   F = 2f + (l_f < 0 ? 1 : 0);  the texel axes are u = (f + 1) % 3 and v = (f + 2) % 3
 *   su = l_u / a_f;  tu = (su + 1.0) * (0.5 * R);  iu = tu >= 0 ? (tu < R ? (int)floor(tu) : R - 1) : 0      (NaN -> 0); iv likewise from l_v
 *   gain_b = table[((F*R + iv)*R + iu)*B + b]
 *
 * so face 0 / 1 is +x / -x of the frame, 2 / 3 is +y / -y, 4 / 5 is +z / -z (a zero frame gives 0 / 0: texel 0 of face 0).  Counter-based
 * means: rays [k, n) of a call with first_ray = a are the rays of a call with first_ray = a + k; and as hare_receive_source's scattering
 * and roulette draws use the same g = first_ray + i (with S = "scatter_seed"), a burst split into chunks gives, summed, the histogram and
 * detections of the one call -- no seed needs changing.
 *   hare_scene_set_source   a setter like those below.  pos: 3; power: B values, NULL for 1.0 in every band; frame: 9 values, NULL for the
 *                           identity; gain: 6 x R x R x B values, NULL iff R == 0.  HARE_E_INVALID for a non-finite pos or frame, B outside
 *                           1..8, R outside 0..64, R and gain disagreeing, any power or gain that is not finite and >= 0.
 *                           hare_scene_get_option reads "source" (0 / 1), "source_bands" and "source_res"
 *
 * Direct sound (flag HARE_RECEIVE_DIRECT; hare_direct_device).  The direct sound needs no sampling: the source, its power, its directivity
 * and the receivers all lie in the scene, so it is ONE visibility query and one deposit per receiver instead of however many of the burst's
 * rays happen to pass through the sphere in cast 0.  All arithmetic is FP64 with no contraction, in this order.  For each receiver k, in
 * any order (integer sums are order-free); pos, power[b] and gain_b are the scene's source, c and rr = r*r are receiver k as stored, and
 * W = (double)n_weight is the number of source rays that the deposit stands for:
 *
 *   vx = cx - pos.x; vy = cy - pos.y; vz = cz - pos.z
 *   d2 = (vx*vx + vy*vy) + vz*vz
 *   eligible  iff  d2 > rr                                  (a NaN is not eligible; a source inside the sphere gets no direct deposit)
 *   occluded  = the hare_occluded predicate on the shadow ray (origin pos, direction v, no exclusion, t_max = 1.0)
 *   if eligible && !occluded:
 *     dist = sqrt(d2);  x = rr / d2
 *     f    = (0.5 * x) / (1.0 + sqrt(1.0 - x))              the sphere's share of the directions, (1 - cos theta) / 2, without cancellation
 *     g_b  = gain_b(v)                                      "Source"'s cube-map lookup with d := v, not normalised (the lookup divides by a_f);
 *                                                           1.0 without a table
 *     m_b  = ((power[b] * g_b) * (f * W)) * 2^frac_bits     then 0 unless > 0; min(., 2^63); q_b = rint -> uint64, as in the receiver step
 *     xb   = dist / bin_len                                 binned as in the receiver step
 *     hist[(k*n_bins + bin)*B + b] += q_b;   detections[2k] += 1 if binned, detections[2k+1] += 1 otherwise
 *     directional: a = ( -(vx / dist), -(vy / dist), -(vz / dist) ), channels as in "Directional" with this m_b
 *
 * Visibility is tested to the center only, as the rain does: a sphere that a wall hides in part counts as wholly seen or wholly hidden.
 * The sound arrives at dist, the distance to the center (|d| = 1 for a source ray, so this is the path to the center, where the sampled
 * direct sound arrives at the closest-approach parameter s of each ray, up to r short of it).
 * Suppression.  In a call with the flag the receiver step of cast 0 is skipped for every ray: no add, no detection.  State update,
 * scattering, rain, termination, reflection, the final state, rays, events and counters are those of the call without the flag.  So, word
 * for word in wrapping uint64, and for detections alike:
 *
 *   hist(flag, bounces) = hist(no flag, bounces) - hist(no flag, bounces = 1) + direct
 *
 * (a one-cast call deposits exactly cast 0's receiver step and nothing else: rain and the rules need c < bounces - 1).
 * Where the flag is accepted.  hare_receive_source, hare_receive_source_sharded and hare_receive_source_reduced: suppression plus the
 * deposit with n_weight = n, the call's whole n, enqueued on the loop's stream before cast 0 (a call with n = 0 runs nothing).  In the
 * sharded call ONE scene makes the deposit, once: scenes[0] (the first scene whose shard holds a ray, which is scenes[0] whenever
 * n >= n_scenes).  hare_receive_device: suppression only; the device caller makes the deposit with hare_direct_device.
 * hare_receive_batch, hare_receive_batch_sharded and hare_receive_batch_reduced: HARE_E_INVALID, refused before anything runs (their
 * rays are the caller's: the library cannot know that they are the source's).  With a receiver map the flag works as with the linear
 * receivers; rain, channels and the termination rules combine freely with it.  No source set: HARE_E_STATE.  The source's B differing
 * from the topology's: HARE_E_INVALID, as without the flag.
 * Chunking.  A burst split into chunks, each with the flag, sums to the one call's histogram up to one unit per chunk, word and band:
 * each chunk rounds f * n_chunk on its own.  A caller who wants the bits of the one call makes ONE hare_direct_device deposit with the
 * whole count and runs the chunks through hare_receive_device with the flag.
 *
 * Image sources (first order) (flag HARE_RECEIVE_IMAGE; hare_image_device).  First-order specular reflections need no sampling either:
 * for each polygon the source is mirrored in its plane, and for each receiver the path exists if the segment from the image to the
 * receiver's center passes through that polygon; it counts if both of its legs are unoccluded.  This is the image-source method at order 1:
 * ONE deposit per (receiver, polygon) pair instead of the few rays per million that happen to take that path.  All arithmetic is FP64 with
 * no contraction, in this order.  pos, power[b] and gain_b are the scene's source; polygon p of top_index has corners v0..v2 (v3 for a
 * quadrilateral) and the stored n = Normal(p); alpha[p][b] and sigma[p][b] are the topology's rows (a missing table is all 0); c and rr are
 * receiver k as stored; W = (double)n_weight.
 * Per polygon p:
 *
 *   h  = dot3(pos.x - v0.x, pos.y - v0.y, pos.z - v0.z, n.x, n.y, n.z)
 *   nn = dot3(n, n)
 *   mirrored  iff  nn > 0 && (h > 0 || h < 0)              (a NaN, or a source on the polygon's plane, h == 0: no image)
 *   k2 = (2.0 * h) / nn
 *   S' = (pos.x - n.x * k2, pos.y - n.y * k2, pos.z - n.z * k2)
 *
 * Per pair (k, p) with p mirrored, in any order (integer sums are order-free):
 *
 *   v  = c - S';  d2 = (vx*vx + vy*vy) + vz*vz;  eligible iff d2 > rr
 *   on_poly = poly_fast(p, v3, o = S', d = v, t)  &&  t > 0.0 && t < 1.0
 *             (the reference's two-sided Triangle / Quadrilateral.Intersect, Ray_Side and the 1e-6 determinant threshold included)
 *   x  = (S'.x + vx*t, S'.y + vy*t, S'.z + vz*t)            the reflection point
 *   occluded = hare_occluded(origin x, direction c - x,   poly_origin1 = p, t_max = 1.0)
 *           || hare_occluded(origin x, direction pos - x, poly_origin1 = p, t_max = 1.0)
 *   if eligible && on_poly && !occluded:
 *     dist = sqrt(d2);  y = rr / d2;  f = (0.5 * y) / (1.0 + sqrt(1.0 - y))          as in "Direct sound"
 *     g_b  = gain_b(x - pos)                                 "Source"'s lookup, not normalised; 1.0 without a table
 *     r_b  = (1.0 - alpha[p][b]) * (1.0 - sigma[p][b])
 *     m_b  = (((power[b] * g_b) * r_b) * (f * W)) * 2^frac_bits      then quantised exactly as the direct deposit's m_b
 *     xb   = dist / bin_len                                  binned as in the receiver step
 *     hist[(k*n_bins + bin)*B + b] += q_b;   detections[2k] += 1 if binned, detections[2k+1] += 1 otherwise
 *     directional: a = ( -(vx / dist), -(vy / dist), -(vz / dist) ), channels as in "Directional" with this m_b
 *
 * What the caller has to know.  Visibility and the on-polygon test go to the receiver's CENTER only: a sphere whose cone a polygon's edge
 * clips counts wholly or not at all.  A center path through an edge shared by two coplanar polygons is accepted by both (the test is
 * inclusive, as in the tracer): a set of measure zero.  Each facet of a tessellated curved surface is its own mirror.  The arrival is at
 * dist, the path length to the center.  r_b is the expected specular share of the sampled loop: absorption, then probability 1 - p times
 * the weight (1 - sigma_b) / (1 - p).  The pair search runs a conservative FP32 pre-cull ahead of the exact test (scene option
 * "image_cull", default 1; 0: the exact test on every pair): it only rejects what the exact test rejects, the results are the same.
 * Suppression.  In a call with the flag, a ray skips cast 1's receiver step iff its reflection behind cast 0 was specular: no add, no
 * detection.  On a topology without a scattering table that is every ray; with one it is exactly the rays with !(u_0 < p) at c = 0 for
 * the polygon they hit in cast 0 -- the draw is counter-based, so cast 1 recomputes it from g, "scatter_seed" and the polygon the ray is
 * leaving.  Rays that went diffuse detect as before (with HARE_RECEIVE_DIFFUSE_RAIN they skip already).  State, draws, weights, rain,
 * termination, reflection, events and counters are those of the call without the flag.  Hence, on a topology without a scattering table
 * and for bounces >= 2, word for word in wrapping uint64 and for detections alike:
 *
 *   hist(flag, bounces) = hist(no flag, bounces) - hist(no flag, 2) + hist(no flag, 1) + image
 *
 * With bounces == 1 nothing is suppressed and the deposit is still made.
 * Where the flag is accepted: exactly where HARE_RECEIVE_DIRECT is.  hare_receive_source, hare_receive_source_sharded and
 * hare_receive_source_reduced: suppression plus the deposit with n_weight = n, before cast 0; in the sharded call ONE scene makes the
 * deposit, once, chosen as for the direct sound.  hare_receive_device: suppression only.  hare_receive_batch, hare_receive_batch_sharded
 * and hare_receive_batch_reduced: HARE_E_INVALID, refused before anything runs.  The flag combines freely with HARE_RECEIVE_DIRECT,
 * directional channels, rain, the termination rules and receiver maps.  No source set: HARE_E_STATE.  The source's B differing from the
 * topology's: HARE_E_INVALID.
 * The pair list.  Accepted pairs go to a list of max_pairs records; the host calls size it from the scene option "image_max_pairs"
 * (default 2^20, 1 .. 2^26).  If the scene yields more pairs, the deposit kernels add NOTHING at all (the count is order-free, so this
 * outcome is deterministic) and the host calls return HARE_E_NOMEM with the needed count in hare_last_error(); their outputs then hold the
 * sampled loop without the image sources.
 * Chunking.  As for the direct sound: a caller who wants the bits of the one call makes ONE hare_image_device deposit with the whole count
 * and runs the chunks through hare_receive_device with the flag.
 *
 * Image sources (second order) (flag HARE_RECEIVE_IMAGE2, with HARE_RECEIVE_IMAGE; hare_image2_device).  The specular paths off TWO polygons,
 * source -> p -> q -> receiver, are computed the same way: the image S' of the source in p's plane is mirrored again in q's plane, the
 * path exists if the segment from that second image S'' to the receiver's center passes through q at x2 and the segment from S' to x2
 * passes through p at x1, and it counts if its three legs are unoccluded.  ONE deposit per (receiver, p, q) path.  FP64, no contraction,
 * in this order; pos, power, gain_b, alpha, sigma, c, rr and W as in the first-order section; p is the polygon hit first, q the second.
 * Per polygon p: S'_p and mirrored_p exactly as first order.  Per ordered pair (p, q) with p != q, mirrored_p, and nn_q = dot3(n_q, n_q) > 0:
 *
 *   h2 = dot3(S'_p.x - v0_q.x, S'_p.y - v0_q.y, S'_p.z - v0_q.z, n_q.x, n_q.y, n_q.z)
 *   mirrored2  iff  h2 > 0 || h2 < 0
 *   k2 = (2.0 * h2) / nn_q
 *   S'' = (S'_p.x - n_q.x * k2, S'_p.y - n_q.y * k2, S'_p.z - n_q.z * k2)
 *
 * Per triple (k, p, q) with mirrored2, in any order:
 *
 *   v  = c - S'';  d2 = (vx*vx + vy*vy) + vz*vz;  eligible iff d2 > rr
 *   on_q = poly_fast(q, v3_q, o = S'', d = v, t2)  &&  t2 > 0.0 && t2 < 1.0
 *   x2 = (S''.x + vx*t2, S''.y + vy*t2, S''.z + vz*t2)
 *   w  = x2 - S'_p
 *   on_p = poly_fast(p, v3_p, o = S'_p, d = w, t1)  &&  t1 > 0.0 && t1 < 1.0
 *   x1 = (S'_p.x + wx*t1, S'_p.y + wy*t1, S'_p.z + wz*t1)
 *   occluded = hare_occluded(origin x2, direction c   - x2, poly_origin1 = q,                    t_max = 1.0)
 *           || hare_occluded(origin x1, direction x2  - x1, poly_origin1 = p, poly_origin2 = q, t_max = 1.0)
 *           || hare_occluded(origin x1, direction pos - x1, poly_origin1 = p,                    t_max = 1.0)
 *   if eligible && on_q && on_p && !occluded:
 *     dist = sqrt(d2);  y = rr / d2;  f = (0.5 * y) / (1.0 + sqrt(1.0 - y))
 *     g_b  = gain_b(x1 - pos)
 *     r_b  = ((1.0 - alpha[p][b]) * (1.0 - sigma[p][b])) * ((1.0 - alpha[q][b]) * (1.0 - sigma[q][b]))
 *     m_b  = (((power[b] * g_b) * r_b) * (f * W)) * 2^frac_bits
 *     directional: a = ( -(vx / dist), -(vy / dist), -(vz / dist) )
 *
 * m_b is quantised, binned at xb = dist / bin_len, deposited and counted in detections exactly as the first-order deposit's.
 * What the caller has to know.  The tests go to the receiver's CENTER only: a sphere whose cone an edge of p or q clips counts wholly or
 * not at all.  A center path through an edge that two polygons share is accepted by each of them, at p and at q alike (the tests are
 * inclusive): a set of measure zero.  Every facet of a tessellated surface is its own mirror, so a curved wall gives as many second images
 * as it has pairs of facets.
 * Suppression.  In a call with the flag, a ray skips cast 2's receiver step iff its reflections behind cast 0 AND behind cast 1 were both
 * specular.  On a topology without a scattering table that is every ray of cast 2.  With one, cast 2 cannot recompute cast 0's choice
 * (that polygon is no longer known), so cast 1, which recomputes it for HARE_RECEIVE_IMAGE and makes its own draw, stores the conjunction
 * as one byte per reflected ray and cast 2 reads it.  Everything else is the call's without the flag.  Hence, on a topology without a
 * scattering table and for bounces >= 3, word for word in wrapping uint64 and for detections alike:
 *
 *   hist(IMAGE | IMAGE2, bounces) = hist(0, bounces) - hist(0, 3) + hist(0, 1) + image + image2
 *
 * With bounces <= 2 nothing more is suppressed than HARE_RECEIVE_IMAGE suppresses, and the deposit is still made.
 * Where the flag is accepted: where HARE_RECEIVE_IMAGE is, and only together with it -- alone it is HARE_E_INVALID, the first check of the
 * call, before anything runs.  hare_receive_source, hare_receive_source_sharded and hare_receive_source_reduced: suppression plus ONE deposit
 * with n_weight = n, before cast 0; in the sharded call the scene that deposits the direct sound makes it.  hare_receive_device:
 * suppression only.  The hare_receive_batch calls refuse it as they refuse HARE_RECEIVE_IMAGE.  Rain, channels, termination rules and
 * receiver maps combine as at first order.
 * The byte array.  The host calls keep it in a buffer of their own.  hare_receive_device with the flag takes it from d_work, which then
 * holds HARE_RECEIVE_IMAGE2_WORK_BYTES(n) more bytes BEHIND what the other flags need: n bytes from offset 8 n, or from offset
 * HARE_RECEIVE_RAIN_WORK_BYTES(n) in a call with HARE_RECEIVE_DIFFUSE_RAIN.  It is written in cast 1 and read in cast 2 of calls with the
 * flag on a topology with a scattering table, and by nothing else; a call without the flag reads and writes the bytes it did before.
 * The two lists.  The candidate stage appends the ordered pairs (p, q) with mirrored2 to a list of max_cands records; the path stage appends
 * the triples with eligible && on_q && on_p to a list of max_paths records.  The host calls size them from the scene options
 * "image2_max_cands" (default 2^22: every ordered pair of up to 2 048 polygons) and "image2_max_paths" (default 2^20), both 1 .. 2^26.
 * A scene of 10^5 polygons yields 10^9 candidates even pruned: more than any list holds, so the call returns HARE_E_NOMEM there.  If EITHER list overflows, the second-order
 * deposit adds NOTHING at all, and the host calls return HARE_E_NOMEM with both counts in hare_last_error() (the path count is not known when
 * the candidates overflowed); their outputs then hold everything but the second order.
 * The prune (scene option "image2_prune", default 1).  With 0 every ordered pair with mirrored2 is a candidate.  With 1 a pair is dropped
 * when no receiver anywhere can pass both on_q and on_p: every x2 lies in the pyramid with apex S'_p over p, beyond p, so q is dropped if its
 * bounding sphere misses the bounding cone of that pyramid, or lies wholly behind p's plane as seen from the source -- both with outward
 * margins of 1e-9 of the coordinates' size.  Non-finite values, a pyramid wider than a right angle and coordinates whose squares overflow
 * take every pair.  The filter never decides a result: histogram, detections and the path count are the same with 0 and 1.
 *
 * Edge diffraction (first order) (hare_scene_set_edges; hare_diffract_device, hare_diffract_paths).  A receiver that the source cannot see
 * gets nothing from the direct sound, and a barrier, a balcony front or a column would cast a hard acoustic shadow.  The engineering remedy
 * is ONE diffracted path over each edge, source -> apex on the edge -> receiver, attenuated by Maekawa's thin-screen rule.  The edges are
 * the caller's: hare_scene_set_edges takes, per topology, E segments a -> b with the two polygons that meet in each (faces, numbered as
 * poly_origin1 numbers polygon p; -1 for none: a free edge of a screen) and inv_lambda[b] = f_b / c in 1/m for the table's B bands.  The
 * library detects no edges.  All arithmetic is FP64 with no contraction, in this order; sqrt and / are the correctly rounded ones; every
 * comparison with a NaN is false; dot(x, y) = (x0*y0 + x1*y1) + x2*y2.  S = pos, power[b] and gain_b are the scene's source; c and rr are
 * receiver k as stored; W = (double)n_weight; edge j is a, b with e = b - a (per component).
 * Per receiver k, exactly the shadow ray and the eligibility of "Direct sound":
 *
 *   v = c - S;  d2 = (vx*vx + vy*vy) + vz*vz;  eligible iff d2 > rr
 *   blocked_k = hare_occluded(origin S, direction v, no exclusion, t_max = 1.0)
 *
 * Per pair (j, k) with k eligible, in any order (integer sums are order-free):
 *
 *   ee = dot(e, e);  ts = dot(S - a, e) / ee;  tr = dot(c - a, e) / ee          the feet of S and c on the edge's line
 *   ps = S - (a + e*ts)  per component;  hs = sqrt(dot(ps, ps));  pr, hr likewise from c and tr
 *   hsum = hs + hr;  t = (ts*hr + tr*hs) / hsum                                  the apex of the shortest path over the line
 *   A = a + e*t;  u = A - S;  w = c - A;  ls2 = dot(u, u);  lr2 = dot(w, w)
 *   ls = sqrt(ls2);  lr = sqrt(lr2);  delta = (ls + lr) - sqrt(d2)               the detour
 *   accepted  iff  hsum > 0 && t > 0 && t < 1 && ls2 > 0 && lr2 > rr && delta > 0 && delta <= max_detour
 *   occluded = hare_occluded(origin A, direction w,     poly_origin1 = faces[2j], poly_origin2 = faces[2j+1], t_max = 1.0)
 *           || hare_occluded(origin A, direction S - A, poly_origin1 = faces[2j], poly_origin2 = faces[2j+1], t_max = 1.0)
 *   if accepted && blocked_k && !occluded:
 *     q  = ls / lr;  S* = (A.x - wx*q, A.y - wy*q, A.z - wz*q)                   the source unfolded about the apex onto the receiver's leg
 *     the deposit of "Image sources (first order)" with S* in S' 's place: v* = c - S*, d2* = dot(v*, v*), dist = sqrt(d2*),
 *     y = rr / d2*, f = (0.5 * y) / (1.0 + sqrt(1.0 - y)), xb = dist / bin_len, a = -(v* / dist), detections as there, and
 *     g_b = gain_b(u)                                        "Source"'s lookup, not normalised; 1.0 without a table
 *     r_b = 1.0 / (3.0 + 20.0 * ((2.0 * delta) * inv_lambda[b]))
 *     m_b = (((power[b] * g_b) * r_b) * (f * W)) * 2^frac_bits                   then quantised exactly as the direct deposit's m_b
 *
 * The deposit stores no detour: it forms u, ls, lr, d2 and delta again from the stored apex A and the stored w by the operations above, so
 * it sees the bits the search saw.
 * What this is and is not.  r_b is Maekawa's ENERGY attenuation for a thin screen, 1 / (3 + 20 N) with the Fresnel number
 * N = 2 delta / lambda_b: a 5 dB step (1/3) at the shadow boundary, falling with frequency and detour.  A receiver the source sees gets no
 * diffracted path at all: the direct sound covers it, so across the shadow boundary the energy steps from the direct sound's to a third of
 * it.  "Blocked" is a blocked CENTER ray, as in "Direct sound".  One edge per path: no path over two edges (a thick barrier's far edge), no
 * reflection before or behind the edge.  S* lies on the line from c through A, ls beyond A, so the arrival direction is
 * the apex's and the path length |c - S*| is ls + lr up to the rounding of the operations stated.  Both faces are excluded on both legs,
 * so a wedge's own faces do not block the legs that leave along them; walls and other obstacles do.
 * The pair list.  Accepted pairs go to a list of max_pairs records.  If the scene yields more, the deposit adds NOTHING at all (the count is
 * order-free, so this outcome is deterministic); hare_diffract_paths then returns HARE_E_NOMEM with the count in *found.
 * Where it goes.  No receive call takes a diffraction flag and hare_source_paths is unchanged: a caller adds the histogram of
 * hare_diffract_paths to that of hare_source_paths or of a receive call as wrapping uint64 words (or runs hare_diffract_device onto the same
 * device histogram), with the same n_weight, bin_len and frac_bits.  With bin_len = c / fs it is what hare_hist_impulses takes.
 *
 * The histogram is fixed point in uint64: integer sums do not depend on the order of the adds, so the result is bit-identical from
 * run to run, between the one-device and the sharded call, and against a restatement on the host.  (r*r is formed once, when the
 * receivers are set: the same FP64 product.)
 *
 * Receiver maps (hare_scene_set_receiver_map).  A map is a plane or cloud of up to 65 536 receivers, one histogram each.  The setter lays
 * a uniform grid over the centers, on the host, FP64, no contraction:
 *
 *   r_max = the largest radius;  lo_a / hi_a = the smallest / largest center coordinate on axis a (a = 0, 1, 2)
 *   h     = cell > 0 ? cell : 2.0 * r_max                       the cell edge; then, until n_0 * n_1 * n_2 <= 2^21:  h = h * 2.0
 *   n_a   = q >= 0 && q < 2^21 ? floor(q) + 1 : (q is NaN ? 1 : too many)          with q = (hi_a - lo_a) / h
 *   R     = r_max + h / 8.0;   P = R / h                          the pad, and the pad in cell edges
 *   cell of receiver k on axis a:  u = (c_a - lo_a) / h;  i_a = u >= 0 ? (u < n_a ? floor(u) : n_a - 1) : 0      (NaN: 0)
 *
 * Every receiver is listed in exactly ONE cell, the cell of its center; cell (i_0, i_1, i_2) has the index (i_2 * n_1 + i_1) * n_0 + i_0
 * and the lists are CSR: cell_start[cells + 1], cell_items[K], ascending k within a cell.  With a map set, the receiver step of a cast
 * is the one above -- the same test, the same binning, the same adds -- run not for k = 0 .. K-1 but for the ray's CANDIDATES: the
 * receivers listed in the cells the ray's segment VISITS.  The visit rule, in cell units, for the ray o, d and t_end of the receiver step
 * (t_end = +inf for a miss).  Every comparison with a NaN is false, and x ? a : b is exactly that:
 *
 *   u_a = (o_a - lo_a) / h;  v_a = d_a / h                                                    a = 0, 1, 2
 *   clip:   t0 = 0; t1 = t_end; ok = true; then for a = 0, 1, 2 with L = -P and H = (double)n_a + P:
 *             v_a == 0:   ok = ok && u_a >= L && u_a <= H
 *             otherwise:  ta = (L - u_a) / v_a;  tb = (H - u_a) / v_a;  ok = ok && ta == ta && tb == tb
 *                         tmin = ta < tb ? ta : tb;  tmax = ta < tb ? tb : ta;  t0 = tmin > t0 ? tmin : t0;  t1 = tmax < t1 ? tmax : t1
 *           no candidates unless  ok && t0 <= t1 && t1 < +inf
 *   major:  m = 0; if |v_1| > |v_m| then m = 1; if |v_2| > |v_m| then m = 2          (a tie goes to the lowest axis)
 *           no candidates if v_m == 0
 *   slabs:  a0 = u_m + v_m * t0;  a1 = u_m + v_m * t1;  amin = a0 < a1 ? a0 : a1;  amax = a0 < a1 ? a1 : a0
 *           jlo = idx(floor(amin - P), n_m);  jhi = idx(floor(amax + P), n_m)
 *           idx(x, n) = x >= 0 ? (x < n ? (int)x : n - 1) : 0          the clamp is made on the double; a NaN gives 0
 *   for every slab j = jlo .. jhi:
 *           tA = (((double)j - P) - u_m) / v_m;  tB = ((((double)j + 1.0) + P) - u_m) / v_m
 *           ts = max(t0, the smaller of tA, tB);  te = min(t1, the larger)      (selected as tmin / tmax above); skip j unless ts <= te
 *           on the axis m the cell range is [j, j]; on each other axis a:
 *             p0 = u_a + v_a * ts;  p1 = u_a + v_a * te;  pmin = p0 < p1 ? p0 : p1;  pmax = p0 < p1 ? p1 : p0
 *             range [idx(floor(pmin - P), n_a), idx(floor(pmax + P), n_a)]
 *           visit every cell of the three ranges
 *
 * The slabs are distinct, so no cell is visited twice and every receiver is tested at most once per ray and cast.  The histogram is a
 * function of the inputs for every input, NaN, infinite, denormal and enormous rays included.
 * The guarantee.  For a ray and a grid in this DOMAIN -- o, d, t_end (of a hit) and every center finite; |o_a - lo_a|, |c_a - lo_a| and, for
 * a hit, |(o_a + d_a * t_end) - lo_a| at most 2^20 * h on every axis, and |o_a|, |c_a| at most 2^20 * h too (the grid is not placed far
 * from the origin in units of its cell); h and the largest |d_a| between 2^-500 and 2^500 -- every receiver the linear definition above
 * detects is a candidate.  Inside the domain a map of K <= 256 receivers therefore gives the histogram, detections, state, rays and events
 * of hare_scene_set_receivers with the same receivers, byte for byte (integer sums do not depend on the order of the adds).  Outside the
 * domain the map's own definition, above, holds: a receiver that the linear loop would detect may then not be a candidate.  (DESIGN.md
 * 7b, "Receiver maps", argues the guarantee: the pad exceeds r_max by h / 8, a thousand times the rounding of every step above.)
 * Diffuse rain does not combine with a map (it costs K occlusion launches per cast): a receive call with HARE_RECEIVE_DIFFUSE_RAIN on a
 * scene that holds a map and, for that topology, a scattering table is HARE_E_INVALID, refused before anything runs.  Everything else --
 * HARE_RECEIVE_DIRECTIONAL, HARE_RECEIVE_TIME_LIMIT, the floor and roulette, scattering, every receive call -- works as without a map;
 * the histogram cap (K x n_bins x B, x 4 with channels, <= 2^27 words) stays.  The sharded calls refuse scenes whose maps differ.
 *
 * Reduction (hare_hist_reduce_device, hare_hist_reduce, hare_receive_batch_reduced, hare_receive_source_reduced).  What a map's user reads
 * from a histogram is a handful of numbers per receiver and band; the reduction forms them on the device, where the histogram lies, in
 * integer arithmetic only -- a function of the inputs, bit for bit, like the histogram itself.  Inputs: a histogram laid out as the
 * receive calls write it, K receivers x n_bins bins x B bands, with `channels` 1, 4, 9 or 16 words per entry (4: HARE_RECEIVE_DIRECTIONAL's, 9 and 16: the higher orders'; the
 * word of channel 0, W, is the one read):
 *
 *   h(k, i, b) = hist[((k * n_bins + i) * B + b) * channels]                                             (uint64)
 *   g(k, i, b) = weight ? floor(h * weight[i * B + b] / 2^32) : h        weight: n_bins x B uint32 in units of 2^-32, or NULL
 *
 * The product is 64 x 32 bits shifted right by 32 and fits uint64; with NULL g is h exactly (a weight cannot express 1.0).  The weights
 * are where air absorption goes: it depends on the distance only, that is on the bin and the band.
 * Windows: n_win (0 .. 16) bin ranges [lo_j, hi_j) = [win[2 j], win[2 j + 1]) with 0 <= lo_j <= hi_j <= n_bins; an empty window is legal.
 * Levels: n_lev (0 .. 32) fractions f_l, uint32 in units of 2^-32 (-5 dB is floor(10^-0.5 * 2^32)).  n_win + n_lev >= 1.
 * Outputs, for every receiver k and band b; every sum is an exact unsigned integer of 128 bits, returned as (lo, hi) uint64 pairs, and
 * nothing wraps (2^27 words below 2^64 stay below 2^91; with the bin factor below 2^122):
 *
 *   sums[((k * B + b) * n_win + j) * 4 + 0 .. 3] = S0_lo, S0_hi, S1_lo, S1_hi
 *       S0 = sum over i in [lo_j, hi_j) of g(k, i, b);   S1 = sum over the same i of i * g(k, i, b)
 *   cross[(k * B + b) * n_lev + l]  (int32):  with T = sum over all i of g, P(i) = sum over i' < i of g and R(i) = T - P(i), the
 *       smallest i in 0 .. n_bins with R(i) * 2^32 <= T * f_l, compared as 128-bit integers.  R(n_bins) = 0, so it always exists;
 *       T = 0 gives 0; f_l = 0 gives the first bin from which the histogram is empty
 *
 * What the caller does with them.  Level (G, SPL) and the clarity ratios (C50, C80, D50) are quotients of S0 of two windows; the centre
 * time is S1 / S0, a bin index, times bin_len; decay times (EDT, T20, T30) come from pairs of crossings of the backward-integrated decay
 * R, or from a regression over up to 32 of them -- ISO 3382's least-squares fit is the caller's, on the crossings; the resolution of a
 * crossing is one bin.  frac_bits cancels in every ratio.
 * One workgroup reduces one receiver (K up to 65 536 of them); K = 1 with a huge n_bins therefore runs on one workgroup: a host-sized
 * problem, and not what the call is for.  There are no sharded variants: a crossing is not additive over shards, and summing device
 * histograms across GPUs is not part of this call -- reduce the histogram the sharded receive call returns with hare_hist_reduce.
 *
 * Projection (hare_hist_project_device, hare_hist_project).  The reduction's sums are unsigned with a fixed weight (1 and i).  The general
 * operation is the projection of each receiver's band histogram onto a few vectors of the caller's over the bins -- cosine and sine tables
 * for the modulation transfer function behind the speech transmission index (IEC 60268-16), arbitrary time weightings, windows with soft
 * edges, regressions over the decay -- formed on the device in integer arithmetic only, exact like everything else read from a histogram.
 * Inputs: the histogram exactly as in "Reduction" (K x n_bins x B entries of `channels` 1, 4, 9 or 16 words; only the W word is read); the
 * optional weight of "Reduction" (n_bins x B uint32, g = floor(h * w / 2^32); NULL: g = h); and
 *
 *   coef: J x n_bins int32, vector-major: c_j[i] = coef[j * n_bins + i]; every int32 value is legal, INT32_MIN included.  1 <= J <= 32.
 *
 * Output, for every receiver k, band b and vector j: the exact signed sum as a 128-bit two's-complement integer in two uint64 words, lo
 * then hi:
 *
 *   proj[((k * B + b) * J + j) * 2 + 0 .. 1] = lo, hi of   sum over i in 0 .. n_bins-1 of  (int128) c_j[i] * g(k, i, b)
 *
 * Nothing wraps: |c| <= 2^31, g < 2^64 and at most 2^27 bins give |P| < 2^122.  What the caller does with it.  The units of c are the
 * caller's -- round(cos(.) * 2^30), say -- and are divided out by the caller; frac_bits cancels in every ratio of two projections.  A
 * vector of ones gives the total T = sum g, and c = i the reduction's S1 over the full window.  The modulation transfer function at the
 * frequency F is sqrt(C^2 + S^2) / (T * 2^30) with C and S the projections onto round(2^30 cos(2 pi F t_i)) and round(2^30 sin(2 pi F t_i)),
 * t_i the time of bin i's centre.  One workgroup projects one receiver, as in "Reduction".  There is no sharded variant and no _projected
 * receive call; unlike a crossing a projection IS additive over shards, so a caller may add, as 128-bit integers, the results of
 * hare_hist_project_device on each shard's device histogram (or project the histogram a sharded receive call returns).  With weight NULL
 * the sum of the shards' projections is exactly the projection of the summed histogram; with weights each shard's floor() is taken on its
 * own words, so g of the shards sums to at most one unit per bin, band and shard less than g of the summed histogram.
 *
 * Directional projection (hare_hist_project_channels_device, hare_hist_project_channels).  The projection reads W and drops the direction
 * a directional histogram recorded.  This call projects EVERY channel, so that the spatial parameters -- the intensity vector, the lateral
 * energy fraction LF, the late lateral level, a modulation transfer function per direction -- are formed where a map's histogram lies.
 * Inputs: exactly those of "Projection" -- the histogram (K x n_bins x B entries of `channels` 1, 4, 9 or 16 words, channel innermost), the
 * optional weight (n_bins x B uint32, units of 2^-32) and coef (J x n_bins int32, vector-major, 1 <= J <= 32, every int32 value legal).
 * Word 0 of an entry is the unsigned W word, as in "Reduction"; the words ch >= 1 are read as two's-complement int64, as the receive loop
 * wrote them ("Directional", "Higher orders"):
 *
 *   h(k, i, b, ch) = hist[((k * n_bins + i) * B + b) * channels + ch]                     ch = 0: uint64;  ch >= 1: (int64)
 *   g(k, i, b, ch) = weight ? floor(h * weight[i * B + b] / 2^32) : h
 *                    floor towards minus infinity for a negative h: (h * w) >> 32 on unbounded integers; h = -1, w = 1 gives -1, not 0
 *   proj[(((k * B + b) * J + j) * channels + ch) * 2 + 0 .. 1] = lo, hi of   sum over i of  (int128) c_j[i] * g(k, i, b, ch)
 *
 * the exact signed sum as a 128-bit two's-complement integer, lo then hi.  Nothing wraps: |c| <= 2^31, |g| < 2^64 and
 * n_bins x channels <= 2^27 give |P| < 2^122.  Consequences: the column ch = 0 is hare_hist_project's result bit for bit; with
 * channels = 1 the call IS hare_hist_project; with weight NULL the result is additive over shards, as 128-bit integers: the sum of the
 * shards' projections is exactly the projection of the summed histogram; with weights each shard's floor() is taken on its own words, so g
 * of the shards sums to at most one unit per bin, band, channel and shard less than g of the summed histogram.
 * What the caller does with it.  With 0 / 1 window vectors as c (and any other vector: an MTF table gives a modulation transfer function
 * per channel), per receiver, band and window, writing W, X, ... Y8 for the projections of the channels 0 .. 8:
 *   the intensity vector  I = (X, Y, Z) / W, the energy-weighted mean arrival direction, and 1 - |I| a diffuseness figure;
 *   the energy-weighted second moments of the arrival vector a, from the order-2 channels, with the SN3D polynomials of "Higher orders"
 *   and x^2 + y^2 + z^2 = 1:   zz = (2 Y6 + W) / 3;   xx - yy = 2 Y8 / sqrt(3), xx + yy = W - zz;   xy = Y4 / sqrt(3),
 *   yz = Y5 / sqrt(3),  xz = Y7 / sqrt(3)  -- hence the energy-weighted (a . u)^2 = u^T M u for any unit axis u;
 *   the early lateral energy fraction LF = M_uu(early window, 5 .. 80 ms) / W(0 .. 80 ms), u the axis through the listener's ears, and the
 *   late lateral level from M_uu(80 ms .. end) against a reference energy.
 * frac_bits cancels in every ratio; each rint of a deposit moved a signed word by at most 1/2, so none of these is exact, unlike the sums
 * they are formed from.  LFC, the |cos| form of the lateral fraction, is not a polynomial of the arrival vector: it cannot be formed
 * from these channels and is not offered.  One workgroup projects one receiver, as in "Reduction".  There is no sharded variant and no
 * _projected receive call: a device caller enqueues hare_hist_project_channels_device behind hare_receive_device on the same stream.
 *
 * Rendering (hare_hist_render_device, hare_hist_render).  The other thing wanted from a histogram is a pressure impulse response to listen
 * to: band-filtered noise shaped by the energy envelope, weighted per channel by the direction the histogram recorded -- the usual
 * rendering of the late part of a ray-traced response.  A pure function of the histogram, a seed and a filter table, formed on the device.
 * Inputs: a histogram as in "Reduction" (K x n_bins x B entries of `channels` 1, 4, 9 or 16 words, frac_bits as given to the receive
 * call); the optional weight of "Reduction" (n_bins x B uint32); M, the samples per bin (1 .. 1024); T, the taps per band filter
 * (1 .. 1024); taps, B x T doubles, one FIR filter per band; seed, a uint64.  Output: out[(k * channels + ch) * N + n], doubles, with
 * N = n_bins * M; every word is written once.  All floating-point work is FP64 without contraction, integers are uint64 and wrap, mix and
 * G are those of "Scattering", and the steps run in exactly this order:
 *
 *   base_k   = mix(mix(seed + G) ^ (uint64)k)
 *   s(k,i)   = (mix(base_k + (uint64)i * G) >> 63) ? -1.0 : 1.0            i = 0 .. N+T-2
 *   y(k,b,n) : y = taps[b*T+0] * s(k, n+T-1);  for t = 1 .. T-1:  y = y + taps[b*T+t] * s(k, n+T-1-t)
 *   p(k,b,i) : p = y0*y0;  for j = 1 .. M-1:  p = p + y_j*y_j           y_j = y(k,b,i*M+j); product rounded, then the add
 *   g(k,i,b)   as in "Reduction" (h, or floor(h*weight/2^32)); W word only
 *   e        = ldexp((double)g, -frac_bits)                               uint64 -> double, round to nearest even
 *   a        = (p > 0.0 && e > 0.0) ? sqrt(e / p) : 0.0                   NaN p gives 0; infinite p gives 0
 *   r_0 = 1.0;  for ch >= 1:  hW = hist[..+0] (unweighted), hc = (int64)hist[..+ch];  r_ch = hW != 0 ? (double)hc / (double)hW : 0.0
 *   out(k,ch,n): i = n / M;  z = (a(k,i,0)*r_ch(k,i,0)) * y(k,0,n);  for b = 1 .. B-1:  z = z + (a(k,i,b)*r_ch(k,i,b)) * y(k,b,n)
 *
 * What the caller has to know.  The product by +-1 is exact, so each y is a sequential sum of signed taps.  For one band alone the sum
 * of out^2 over a bin's samples equals e up to rounding; band cross terms vanish only as far as the caller's filters are orthogonal.  All
 * channels of a receiver share one noise sequence, so direction is carried by the gains; receivers are decorrelated through k.  r_ch is
 * the energy-weighted mean of the SN3D harmonic in that bin.  The gain is constant across a bin (no interpolation).  Deterministic early
 * paths are better rendered as impulses than as noise: a caller who wants that deposits the direct sound and the image sources into a
 * histogram of their own with the _device calls and renders only the rest here; rendering impulses is not part of this call
 * ("Impulses" below).  The
 * sequential order of y, p and z is part of the definition: parallelism is over (k, b, n) and (k, b, i), never inside a sum.
 *
 * Impulses (hare_hist_impulses_device, hare_hist_impulses, hare_source_paths).  The direct sound and the specular reflections of the first
 * and second order are the arrivals the ear locates; rendered as noise they become bursts a bin long with a random polarity.  The three
 * deposit calls accept any n_bins and bin_len: with a bin of ONE output sample (bin_len = c / fs) they deposit every path into the sample
 * it arrives in, as exact integers, whatever the order, the directional channels included.  This call turns such a per-sample histogram
 * into pressure rows: every non-empty (bin, band) becomes an impulse of amplitude sqrt(energy), positive, filtered by that band's FIR and
 * weighted per channel by the rendering's ratio; optionally added onto rows "Rendering" wrote (the noise tail), which makes the hybrid
 * response.  Inputs: a histogram as in "Reduction" (K x n_bins x B entries of `channels` 1, 4, 9 or 16 words), the optional weight of
 * "Reduction" (n_bins x B uint32), frac_bits, taps (B x T doubles, 1 <= T <= 1024), a window [n0, n0 + n_out) of the n_bins + T - 1
 * samples of the full result, out_stride >= n_out (doubles between the rows of out), and add, 0 or 1.  Output: out[(k * channels + ch) *
 * out_stride + (n - n0)], doubles.  All floating-point work is FP64 without contraction, in exactly this order:
 *
 *   per (k, i, b):  hW = hist[..+0];  g = hW, or the weighted word of "Reduction";  an ENTRY exists iff g != 0
 *   e = ldexp((double)g, -frac_bits);  a = sqrt(e)                            uint64 -> double, round to nearest even
 *   r_0 = 1.0;  for ch >= 1:  r_ch = (double)(int64)hist[..+ch] / (double)hW   (hW != 0 follows from g != 0);   gain_ch = a * r_ch
 *   out(k,ch,n): z = +0.0
 *     for b = 0 .. B-1 ascending:  for i = max(0, n - (T-1)) .. min(n_bins - 1, n) ascending:
 *       if (k, i, b) is an entry:  z = z + (gain_ch(k,i,b) * taps[b*T + (n - i)])       product rounded, then the add
 *   out[..] = z  (add == 0),  or  out[..] + z, one add  (add == 1)
 *
 * Bins without an entry and taps out of range contribute NO term: they are skipped, not multiplied by zero, for the reason "Convolution"
 * gives -- a tap that is not finite reaches exactly the outputs an entry carries it to, and the sparse sum is the dense one bit for bit.
 * The words from n_out to out_stride of a row are never touched.  A NaN output is "some NaN", as elsewhere.  Parallelism is over (k, n),
 * never inside a sum: a job cut over windows or over receivers is the one call byte for byte.  Two paths in one sample and band add as
 * energies (sqrt(e1 + e2)), not as pressures.  The energy an impulse puts into band b is e * sum_t taps[b][t]^2, so calibration against
 * the noise rendering is a matter of the taps (bindings: hare_amd.unit_energy_taps scales each band's row to unit energy; a convenience
 * outside this contract).  With taps whose bands telescope to a delay of D samples (hare_amd.band_taps: D = (T - 1) / 2), n0 = D aligns
 * output sample n with bin n.  hare_source_paths runs the three deposits alone, from the host: what hare_receive_source deposits ahead of
 * cast 0 under HARE_RECEIVE_DIRECT / _IMAGE / _IMAGE2 and nothing of the loop, word for word.
 *
 * Convolution (hare_convolve_device, hare_convolve).  What is listened to is not the response but a sound in the room: a dry signal
 * convolved with the response of every receiver channel.  This is that last step, in the time domain, on the device, so that the chain stays
 * a pure function of its inputs to the end.  Inputs: ir, R rows of N doubles -- exactly the rows "Rendering" writes (R = K * channels,
 * N = n_bins * M, row r = k * channels + ch), though the call does not care where they came from; x, ONE signal of L doubles shared by all
 * rows; and an output window [n0, n0 + n_out) of the N + L - 1 samples of the full convolution.  Output: y[r * n_out + (n - n0)], doubles,
 * every word written once.  All arithmetic is FP64 without contraction -- the product is rounded, then the add -- in exactly this order:
 *
 *   t_lo = max(0, n - (L - 1));   t_hi = min(N - 1, n)
 *   acc = +0.0;   for t = t_lo .. t_hi ascending:   acc = acc + ir[r*N + t] * x[n - t]
 *   y(r, n) = acc
 *
 * Terms outside [t_lo, t_hi] are SKIPPED, not formed against a zero: a value of ir or x that is not finite reaches exactly the outputs
 * whose range holds it.  Parallelism is over (r, n), never inside a sum, so a split of a job over output windows, or of its rows over
 * several calls or GPUs, is byte-identical to the one call; there is no sharded variant and no mixing between rows (a decode matrix is another call's
 * business: "Decoding" below).
 * Infinities, signed zeros and denormals follow IEEE 754 to the bit; the accumulator starts at +0.0 and is therefore never -0.0.  A NaN
 * output is "some NaN": its sign and payload are not defined (the one place where a comparison with a host is not byte for byte).  An FFT
 * would take fewer operations and has no statable order of its sums: not offered.
 * Limits (HARE_E_INVALID): 1 <= R <= 2^20, 1 <= N <= 2^24, 1 <= L <= 2^28; 0 <= n0, 1 <= n_out, n0 + n_out <= N + L - 1;
 * R * n_out <= 2^28 (the render call's output cap); and R * n_out * min(N, L) <= HARE_CONVOLVE_MAX_TERMS, an upper bound of the terms of
 * one call: the devices are shared and one launch is not to run for many seconds.  The cap, 2^44, is the largest power of two whose launch
 * stays under two seconds at the rate measured on an MI355X, 1.39e13 terms per second: 1.26 s ("Convolution"); a larger job
 * is cut into output windows by the caller.
 *
 * Decoding (hare_decode_device, hare_decode).  The rows of a directional receiver are ambisonic channels -- W X Y Z, then ACN 4..15 in SN3D
 * -- and nobody plays those back: they are decoded to ears or to loudspeakers, every output channel a sum over ALL input channels of that
 * channel filtered by a short FIR of its own (HRIR-derived for binaural, one gain each for a loudspeaker matrix, a few taps for a virtual
 * microphone).  This is the mixing between rows that "Convolution" leaves out.  Inputs: in, K x C rows of N doubles, row k * C + c --
 * exactly the rows "Rendering" writes (C = channels, N = n_bins * M), or equally the rows "Convolution" writes with a full window; h,
 * O x C filters of T doubles, h[(o*C + c)*T + t], shared by all receivers; and an output window [n0, n0 + n_out) of the N + T - 1 samples.
 * Output: y[(k*O + o)*n_out + (n - n0)], doubles, every word written once.  All arithmetic is FP64 without contraction -- the product is
 * rounded, then the add -- in exactly this order:
 *
 *   t_lo = max(0, n - (N - 1));   t_hi = min(T - 1, n)
 *   acc = +0.0
 *   for c = 0 .. C-1 ascending:   for t = t_lo .. t_hi ascending:   acc = acc + h[(o*C + c)*T + t] * in[(k*C + c)*N + (n - t)]
 *   y(k, o, n) = acc
 *
 * ONE accumulator runs through all channels: this is neither C convolutions added afterwards nor a sum with t outside and c inside.  The
 * rules of "Convolution" hold: terms outside [t_lo, t_hi] are SKIPPED, never formed against a zero, so a value of in or h that is not
 * finite reaches exactly the outputs whose range holds it; the accumulator starts at +0.0 and is never -0.0; a NaN output is "some NaN";
 * parallelism is over (k, o, n), never inside a sum, so a job cut over output windows, over outputs o (rows of h) or over receivers k (rows
 * of in) is the one call byte for byte, and there is no sharded variant.  With C = O = 1 the call IS hare_convolve with ir = h (R = 1,
 * its N this T) and x = in[k] (its L this N), bit for bit.  Helpers that build h (a sampling decoder, virtual
 * loudspeakers through a caller's HRIR set) are host code of the bindings (hare_amd/decoders.py); no HRIR data is shipped.
 * Limits (HARE_E_INVALID): 1 <= K <= 65 536, 1 <= C <= 64, 1 <= O <= 64; 1 <= N <= 2^24, 1 <= T <= 2^16; 0 <= n0, 1 <= n_out,
 * n0 + n_out <= N + T - 1; K * C * N <= 2^28 and K * O * n_out <= 2^28; and K * O * n_out * C * min(N, T) <= HARE_DECODE_MAX_TERMS, an
 * upper bound of the terms of one call, a constant of its own: the instruction mix is the convolution's, and so is the reason for the cap.
 * The cap, 2^42, is the largest power of two whose launch stays under two seconds at the rate measured on an MI355X for 16 third-order
 * receivers decoded to two ears through 512 taps, 4.31e12 terms per second: 1.02 s ("Decoding"); a larger job is cut into
 * output windows by the caller.
 *
 * Setters: single-caller, like the build calls.  They validate, keep a host copy, and upload it when a device is present (as a build
 * pushes its partition; on a GPU-less host the copy goes up with the first receive call).  No receive call allocates for them.
 *   hare_scene_set_receivers    replaces the receivers: centers K x 3, radii K.  HARE_E_INVALID for K outside 1..256, a non-finite
 *                               center, or a radius that is not finite and > 0
 *   hare_scene_set_absorption   alpha: P x B of Model[top_index] (row per polygon).  HARE_E_INVALID for a bad top_index, B outside 1..8,
 *                               any alpha outside [0, 1] or NaN, or a B other than that of the topology's scattering table
 *   hare_scene_set_scattering   sigma: P x B of Model[top_index], checked as alpha is (and against the absorption table's B); B = 0 with
 *                               sigma NULL removes the table
 *   hare_scene_set_receiver_map replaces the receivers by a map: 1 <= K <= 65 536, centers and radii as above; cell: the grid's cell edge,
 *                               0 for the default 2 r_max (either is doubled until the grid has at most 2^21 cells).  HARE_E_INVALID for
 *                               K outside the range, a non-finite center, a radius that is not finite and > 0, and a cell that is NaN,
 *                               negative or infinite; a refused call changes nothing.  hare_scene_set_receivers afterwards replaces the
 *                               map and returns the scene to the linear loop (its own limit stays K <= 256)
 *   hare_scene_get_receiver_map reads a map back (HARE_E_STATE when none is set); every output is nullable.  geom: 5 doubles, lo_0, lo_1,
 *                               lo_2, h and R; dims: n_0, n_1, n_2; cell_start: cells + 1 offsets; cell_items: K receiver indices
 * hare_scene_get_option also reads "receiver_map" (1 while a map is set, else 0), "receiver_map_cells" (the grid's cell count; 0 without
 * a map) and "receiver_map_cell" (the cell edge h as the 64 bits of the double, the getter's values being integers; 0 without a map).
 * hare_scene_get_option reads back "receivers" (K; 0 before the first set), "bands" (B of topology 0) and "bands:<top>" (B of topology
 * <top>): the sizes of a receive call's histogram (K x n_bins x B) and state ((1 + B) x n) for that topology.  The library cannot check the
 * size of a caller's host buffer: the bindings size theirs from these. */
HARE_API int hare_scene_set_receivers(hare_scene *s, int32_t K, const double *centers, const double *radii);
HARE_API int hare_scene_set_receiver_map(hare_scene *s, int32_t K, const double *centers /* K x 3 */, const double *radii /* K */,
                                         double cell /* 0: default */);
HARE_API int hare_scene_get_receiver_map(const hare_scene *s, double *geom /* 5 */, int32_t *dims /* 3 */, uint32_t *cell_start,
                                         uint32_t *cell_items);
HARE_API int hare_scene_set_absorption(hare_scene *s, int32_t top_index, int32_t B, const double *alpha);
HARE_API int hare_scene_set_scattering(hare_scene *s, int32_t top_index, int32_t B, const double *sigma);
HARE_API int hare_scene_set_source(hare_scene *s, const double pos[3], int32_t B, const double *power /* B, nullable */,
                                   const double *frame /* 9, nullable */, int32_t R, const double *gain /* 6 R R B, NULL iff R == 0 */);

/* The source's rays on DEVICE buffers: n hare_ray into d_rays and the (1 + B) x n doubles of their state into d_state (plane 0: L, planes
 * 1..B: E; B the source's), for the rays first_ray .. first_ray + n - 1 ("Source" above).  Stream-ordered like hare_shoot_device: no
 * allocation, no free, no wait.  HARE_E_INVALID unless 0 <= n <= 2^31 - 256, first_ray >= 0 and first_ray + n <= 2^62; for null or
 * overlapping buffers; then HARE_E_NODEVICE; then HARE_E_STATE when no source is set. */
HARE_API int hare_emit_device(hare_scene *s, int64_t n, int64_t first_ray, void *d_rays, void *d_state, void *stream);

/* The receive loop on DEVICE buffers: stream-ordered like hare_shoot_device -- no allocation, no free, no wait ("hip_malloc_calls" ...).
 * Always a launch per cast (the scene option "bounce_fused" does not apply; results are the same either way).
 *   d_rays, d_excl1, d_excl2, d_work (2 n int32), d_events_last   as in hare_bounce_device
 *   d_state        (1 + B) planes of n doubles: plane 0 is L, planes 1..B are E.  Read and overwritten
 *   d_hist         K x n_bins x B uint64 (x 4 with HARE_RECEIVE_DIRECTIONAL; x 9, x 16 with the order flags), ACCUMULATED;  d_detections: 2 K uint64, ACCUMULATED
 *   d_counters     nullable: totals, ACCUMULATED (as hare_bounce_device's; the rain's occlusion queries are not counted)
 *   flags          HARE_SHOOT_COUNT_WORK / HARE_SHOOT_SIMPLE_KERNEL (the casts), HARE_RECEIVE_DIFFUSE_RAIN, HARE_RECEIVE_DIRECTIONAL,
 *                  HARE_RECEIVE_TIME_LIMIT, HARE_RECEIVE_DIRECT, HARE_RECEIVE_IMAGE and HARE_RECEIVE_IMAGE2 (suppression only: "Direct sound",
 *                  "Image sources"; HARE_RECEIVE_IMAGE2 adds HARE_RECEIVE_IMAGE2_WORK_BYTES(n) bytes behind d_work's other contents);
 *                  other bits are ignored.  With
 *                  HARE_RECEIVE_DIFFUSE_RAIN d_work holds HARE_RECEIVE_RAIN_WORK_BYTES(n) bytes: the 2 n int32, then the rain's scratch
 * Arguments are checked before anything runs (HARE_E_INVALID): kind, top_index, 0 <= n <= 2^31 - 256, 1 <= bounces <= 4096,
 * n_bins >= 1, bin_len finite and > 0, 0 <= frac_bits <= 62, K x n_bins x B <= 2^27 (K x n_bins x B x 4 <= 2^27 with
 * HARE_RECEIVE_DIRECTIONAL), null or overlapping buffers (d_hist at the size the flags give it).  Then
 * HARE_E_NODEVICE, then HARE_E_STATE (no receivers set; partition not built). */
#define HARE_RECEIVE_RAIN_WORK_BYTES(n) (80 * (int64_t)(n) + 256)
HARE_API int hare_receive_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, void *d_rays, const void *d_excl1,
                                 const void *d_excl2, int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len,
                                 int32_t frac_bits, void *d_state, void *d_work, void *d_events_last, void *d_hist,
                                 void *d_detections, void *d_counters, void *stream);
/* The direct sound's deposit on DEVICE buffers ("receivers", "Direct sound"): one visibility query and one deposit per receiver of the
 * scene, from the scene's source, standing for n_weight source rays.  Stream-ordered like hare_emit_device: no allocation, no free, no
 * wait.  d_hist (K x n_bins x B uint64, x 4 with HARE_RECEIVE_DIRECTIONAL, x 9 or x 16 with HARE_RECEIVE_ORDER2 / _ORDER3 beside it: the only flags read) and d_detections (2 K uint64) are
 * ACCUMULATED; d_work is scratch of HARE_DIRECT_WORK_BYTES(K) bytes (K shadow rays, t_max, exclusion words and flags), B the source's.
 * Checked in this order: HARE_E_INVALID unless 1 <= n_weight <= 2^53, kind, top_index, n_bins >= 1, bin_len finite and > 0,
 * 0 <= frac_bits <= 62, the histogram within 2^27 words, no buffer null and none overlapping another, and a source whose B is not
 * the topology's; then HARE_E_NODEVICE; then HARE_E_STATE: no source, no receivers, or the partition not built. */
#define HARE_DIRECT_WORK_BYTES(K) (64 * (int64_t)(K) + 256)
HARE_API int hare_direct_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags /* HARE_RECEIVE_DIRECTIONAL, _ORDER2, _ORDER3 only */,
                                int32_t n_bins, double bin_len, int32_t frac_bits, void *d_work, void *d_hist, void *d_detections, void *stream);
/* The first-order image sources' deposit on DEVICE buffers ("receivers", "Image sources (first order)"): the pair search receivers x
 * polygons, one occlusion query of two shadow rays per accepted pair and one deposit per pair with both legs free, from the scene's source,
 * standing for n_weight source rays.  Stream-ordered like hare_direct_device: no allocation, no free, no wait.  d_hist and d_detections
 * are ACCUMULATED, shaped as hare_direct_device's.  d_work is scratch of HARE_IMAGE_WORK_BYTES(K, P, max_pairs) bytes on a 16-byte
 * boundary (P: the polygons of Model[top_index]): a 256-byte head whose first 8-byte word receives the number of pairs found, the P images,
 * and the list of max_pairs records (two shadow rays, their t_max and exclusion words, k and p, two flags), in unspecified order.  If more
 * than max_pairs pairs are found nothing is deposited; the caller reads the count from the first word behind the stream.
 * Checked as hare_direct_device checks, in its order, plus 1 <= max_pairs <= 2^26 and the work array's boundary (HARE_E_INVALID). */
#define HARE_IMAGE_WORK_BYTES(K, P, max_pairs) (256 + 32 * (int64_t)(P) + 136 * (int64_t)(max_pairs) + 0 * (int64_t)(K))
HARE_API int hare_image_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags /* HARE_RECEIVE_DIRECTIONAL, _ORDER2, _ORDER3 only */,
                               int32_t n_bins, double bin_len, int32_t frac_bits, int64_t max_pairs, void *d_work, void *d_hist,
                               void *d_detections, void *stream);
/* The second-order image sources' deposit on DEVICE buffers ("receivers", "Image sources (second order)"): the candidate stage polygons x
 * polygons, the path stage receivers x candidates, one occlusion query of three shadow rays per path and one deposit per path with all
 * legs free, from the scene's source, standing for n_weight source rays.  Stream-ordered: no allocation, no free, no wait.  d_hist and
 * d_detections are ACCUMULATED, shaped as hare_direct_device's.  d_work is scratch of HARE_IMAGE2_WORK_BYTES(P, max_cands, max_paths) bytes
 * on a 16-byte boundary (P: the polygons of Model[top_index]): a 256-byte head whose first 8-byte word receives the number of candidates
 * found and whose second the number of paths found; the P images (32 bytes each); the candidates (32 bytes: S'', p, q); the paths (212
 * bytes: three shadow rays, their t_max, two exclusion words and a flag each, k and the candidate's index), in unspecified order.  If
 * either count exceeds its list nothing is deposited (a candidate overflow leaves the path count 0); the caller reads both words behind
 * the stream.  Checked as hare_image_device checks, in its order, with 1 <= max_cands, max_paths <= 2^26 (HARE_E_INVALID). */
#define HARE_IMAGE2_WORK_BYTES(P, max_cands, max_paths) (256 + 32 * (int64_t)(P) + 32 * (int64_t)(max_cands) + 212 * (int64_t)(max_paths))
/* hare_receive_device with HARE_RECEIVE_IMAGE2: the bytes d_work holds behind its other contents ("Image sources (second order)", "The byte array") */
#define HARE_RECEIVE_IMAGE2_WORK_BYTES(n) ((int64_t)(n))
HARE_API int hare_image2_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags /* HARE_RECEIVE_DIRECTIONAL, _ORDER2, _ORDER3 only */,
                                int32_t n_bins, double bin_len, int32_t frac_bits, int64_t max_cands, int64_t max_paths, void *d_work,
                                void *d_hist, void *d_detections, void *stream);
/* The diffracting edges of Model[top_index] ("receivers", "Edge diffraction (first order)"): a setter like those above.  ends: E x 6 (a, b);
 * faces: E x 2, the polygons that meet in each edge, -1 for none; inv_lambda: B values f_b / c.  Checked in this order (HARE_E_INVALID; a
 * refused call changes nothing): top_index; E within 1 .. 2^20 and no array null (E = 0 with ends and faces NULL removes the table); every
 * end finite; a != b (the FP64 dot(e, e) > 0 and finite); every face within -1 .. P - 1; B within 1 .. 8; every inv_lambda finite and >= 0.
 * "edges" / "edges:<top>" read E back. */
HARE_API int hare_scene_set_edges(hare_scene *s, int32_t top_index, int32_t E, const double *ends /* E x 6: a, b */,
                                  const int32_t *faces /* E x 2 */, int32_t B, const double *inv_lambda /* B */);
/* First-order edge diffraction on DEVICE buffers ("receivers", "Edge diffraction (first order)"): one direct visibility query per receiver,
 * the pair search edges x receivers, two shadow rays per accepted pair -- ONE occlusion query for all of them -- and one deposit per pair
 * whose receiver the source does not see and whose legs are free, from the scene's source, standing for n_weight source rays.
 * Stream-ordered like hare_direct_device: no allocation, no free, no wait.  d_hist and d_detections are ACCUMULATED, shaped as
 * hare_direct_device's.  d_work is scratch of HARE_DIFFRACT_WORK_BYTES(K, max_pairs) bytes on a 16-byte boundary: a 256-byte head whose
 * first 8-byte word receives the number of pairs found; the K direct shadow rays with t_max, two exclusion words and a flag each; the list
 * of max_pairs records (two shadow rays, two t_max, 2 x 2 exclusion words, two flags, k and j; the detour is re-formed, not stored), in
 * unspecified order.  If more than max_pairs pairs are found nothing is deposited; the caller reads the count from the first word behind
 * the stream.  Checked as hare_image_device checks, in its order (1 <= max_pairs <= 2^26 in its place), then max_detour not NaN and >= 0
 * (+inf: no limit), then a source whose B is not the edge table's, then the buffers (HARE_E_INVALID); then HARE_E_NODEVICE; then
 * HARE_E_STATE: no source, no receivers, no edges for top_index, or the partition not built. */
#define HARE_DIFFRACT_WORK_BYTES(K, max_pairs) (256 + 68 * (int64_t)(K) + 144 * (int64_t)(max_pairs))
HARE_API int hare_diffract_device(hare_scene *s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags /* HARE_RECEIVE_DIRECTIONAL, _ORDER2, _ORDER3 only */,
                                  int32_t n_bins, double bin_len, int32_t frac_bits, double max_detour, int64_t max_pairs, void *d_work,
                                  void *d_hist, void *d_detections, void *stream);
/* The same from host buffers, built as hare_source_paths is: a batch context leased, histogram and detections zeroed, one enqueue, the
 * downloads, one synchronisation.  hist and detections are WRITTEN; found (nullable) receives the number of pairs found.  More pairs than
 * max_pairs: HARE_E_NOMEM, hist and detections all zero, the count in *found and in hare_last_error().  Checks and their order as
 * hare_diffract_device's, with hist and detections in the buffers' place. */
HARE_API int hare_diffract_paths(hare_scene *s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags /* HARE_RECEIVE_DIRECTIONAL, _ORDER2, _ORDER3 only */,
                                 int32_t n_bins, double bin_len, int32_t frac_bits, double max_detour, int64_t max_pairs, uint64_t *hist,
                                 uint64_t *detections, uint64_t *found /* nullable */);
/* The same from host buffers (threading and staging as hare_bounce_batch's last-cast-only path: one enqueue, one synchronisation; no
 * events are downloaded).  state_in nullable (every ray starts at L = 0, E = 1); state_out nullable ((1 + B) x n, as d_state).
 * hist (K x n_bins x B, x 4 with HARE_RECEIVE_DIRECTIONAL, x 9 / x 16 with the order flags) and detections (2 K) are WRITTEN, not accumulated; ctr nullable: counters summed over the casts.  flags as
 * hare_receive_device's (the call sizes the rain's scratch itself). */
HARE_API int hare_receive_batch(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, const hare_ray *rays,
                                const int32_t *excl1, const int32_t *excl2, int32_t bounces, uint32_t flags, int32_t n_bins,
                                double bin_len, int32_t frac_bits, const double *state_in, double *state_out, uint64_t *hist,
                                uint64_t *detections, hare_counters *ctr);
/* Over several devices: rays [n*k/G, n*(k+1)/G) go to scenes[k] (as hare_bounce_batch_sharded), the histograms and detections are
 * summed.  Byte-identical to the one-device call.  The scenes must hold the same receivers, bands, scattering table, "receive_floor_bits",
 * "receive_roulette" and (with a table, or with roulette) "scatter_seed" (HARE_E_INVALID otherwise). */
HARE_API int hare_receive_batch_sharded(hare_scene *const *scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                                        const hare_ray *rays, const int32_t *excl1, const int32_t *excl2, int32_t bounces,
                                        uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits,
                                        const double *state_in, double *state_out, uint64_t *hist, uint64_t *detections,
                                        hare_counters *ctr);

/* hare_receive_batch / _sharded with the upload of rays and state replaced by the source's emission on the loop's stream: the rays
 * first_ray .. first_ray + n - 1 of the scene's source ("Source" above), no exclusions.  In the sharded call the shard that starts at ray lo
 * emits from first_ray + lo.  Flags, checks and outputs as hare_receive_batch's, and HARE_E_INVALID when first_ray < 0 or
 * first_ray + n > 2^62, or when the source's B is not the band count of Model[top_index]; HARE_E_STATE when no source is set.  The sharded
 * call also refuses scenes whose source or "source_seed" differ.  These calls (and hare_receive_source_reduced) take HARE_RECEIVE_DIRECT
 * ("Direct sound"), HARE_RECEIVE_IMAGE ("Image sources (first order)") and, with it, HARE_RECEIVE_IMAGE2 ("Image sources (second order)");
 * the hare_receive_batch calls refuse all three. */
HARE_API int hare_receive_source(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, int64_t first_ray, int32_t bounces,
                                 uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits, double *state_out, uint64_t *hist,
                                 uint64_t *detections, hare_counters *ctr);
HARE_API int hare_receive_source_sharded(hare_scene *const *scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                                         int64_t first_ray, int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len,
                                         int32_t frac_bits, double *state_out, uint64_t *hist, uint64_t *detections, hare_counters *ctr);

/* The reduction of a histogram ("receivers", "Reduction" above) on DEVICE buffers: one launch, stream-ordered like hare_shoot_device -- no
 * allocation, no free, no wait.  win (2 n_win) and levels (n_lev) are HOST arrays, read at the call (they travel as kernel arguments);
 * d_weight nullable; d_sums (K x B x n_win x 4 uint64; unused when n_win = 0) and d_cross (K x B x n_lev int32; unused when n_lev = 0) are
 * WRITTEN, every word once.  Checked before anything runs (HARE_E_INVALID): 1 <= K <= 65 536, n_bins >= 1, 1 <= B <= 8, channels 1, 4, 9 or 16,
 * K x n_bins x B x channels <= 2^27, 0 <= n_win <= 16, 0 <= n_lev <= 32 and not both 0, every window 0 <= lo <= hi <= n_bins, null
 * buffers, and sums or crossings overlapping each other, the histogram or the weights.  Then HARE_E_NODEVICE, then HARE_E_STATE.  The
 * scene names the device; its geometry is not read. */
HARE_API int hare_hist_reduce_device(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void *d_hist,
                                     const void *d_weight /* nullable */, int32_t n_win, const int32_t *win /* host */, int32_t n_lev,
                                     const uint32_t *levels /* host */, void *d_sums, void *d_cross, void *stream);
/* The same from host buffers: upload, reduce, download, one synchronisation. */
HARE_API int hare_hist_reduce(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t *hist,
                              const uint32_t *weight /* nullable */, int32_t n_win, const int32_t *win, int32_t n_lev,
                              const uint32_t *levels, uint64_t *sums, int32_t *cross);
/* The projection of a histogram ("receivers", "Projection" above) on DEVICE buffers: one launch, stream-ordered like hare_shoot_device --
 * no allocation, no free, no wait, no upload.  d_coef (J x n_bins int32) is a device buffer of the caller's; d_weight nullable; d_proj
 * (K x B x J x 2 uint64) is WRITTEN, every word once.  Checked before anything runs (HARE_E_INVALID), in this order: 1 <= K <= 65 536,
 * n_bins >= 1, 1 <= B <= 8, channels 1, 4, 9 or 16, K x n_bins x B x channels <= 2^27; 1 <= J <= 32; null buffers; proj overlapping the
 * histogram, the weights or the coefficients.  Then HARE_E_NODEVICE, then HARE_E_STATE.  The scene names the device; its geometry is not
 * read.  Behind hare_receive_device on the same stream it projects the histogram that call accumulated. */
HARE_API int hare_hist_project_device(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void *d_hist,
                                      const void *d_weight /* nullable */, int32_t J, const void *d_coef, void *d_proj, void *stream);
/* The same from host buffers: one allocation, upload, project, download, one synchronisation. */
HARE_API int hare_hist_project(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t *hist,
                               const uint32_t *weight /* nullable */, int32_t J, const int32_t *coef, uint64_t *proj);
/* The projection of every channel of a histogram ("receivers", "Directional projection" above) on DEVICE buffers: one launch,
 * stream-ordered like hare_hist_project_device -- no allocation, no free, no wait, no upload.  d_coef (J x n_bins int32) is a device buffer
 * of the caller's; d_weight nullable; d_proj (K x B x J x channels x 2 uint64) is WRITTEN, every word once.  Checked before anything runs
 * (HARE_E_INVALID), in this order, as hare_hist_project_device checks: 1 <= K <= 65 536, n_bins >= 1, 1 <= B <= 8, channels 1, 4, 9 or
 * 16, K x n_bins x B x channels <= 2^27; 1 <= J <= 32; null buffers; proj overlapping the histogram, the weights or the coefficients.
 * Then HARE_E_NODEVICE, then HARE_E_STATE.  The scene names the device; its geometry is not read.  Behind hare_receive_device on the same
 * stream it projects the histogram that call accumulated. */
HARE_API int hare_hist_project_channels_device(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void *d_hist,
                                               const void *d_weight /* nullable */, int32_t J, const void *d_coef, void *d_proj,
                                               void *stream);
/* The same from host buffers: one allocation, upload, project, download, one synchronisation. */
HARE_API int hare_hist_project_channels(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t *hist,
                                        const uint32_t *weight /* nullable */, int32_t J, const int32_t *coef, uint64_t *proj);
/* The rendering of a histogram ("receivers", "Rendering" above) on DEVICE buffers: one launch, stream-ordered like hare_shoot_device -- no
 * allocation, no free, no wait.  d_taps (B x T doubles) is a device buffer of the caller's: the call has nothing to upload.  d_weight
 * nullable; d_out (K x channels x n_bins x M doubles) is WRITTEN, every word once.  Checked before anything runs (HARE_E_INVALID), in this
 * order: 1 <= K <= 65 536, n_bins >= 1, 1 <= B <= 8, channels 1, 4, 9 or 16, K x n_bins x B x channels <= 2^27; 1 <= M <= 1024 and
 * 1 <= T <= 1024; 0 <= frac_bits <= 62; K x channels x n_bins x M <= 2^28; null buffers; out overlapping the histogram, the weights or
 * the taps.  Then HARE_E_NODEVICE, then HARE_E_STATE.  The scene names the device; its geometry is not read. */
HARE_API int hare_hist_render_device(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void *d_hist,
                                     const void *d_weight /* nullable */, int32_t frac_bits, int32_t M, int32_t T, const void *d_taps,
                                     uint64_t seed, void *d_out, void *stream);
/* The same from host buffers: upload, render, download, one synchronisation.  Also HARE_E_INVALID: a tap that is not finite. */
HARE_API int hare_hist_render(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t *hist,
                              const uint32_t *weight /* nullable */, int32_t frac_bits, int32_t M, int32_t T, const double *taps,
                              uint64_t seed, double *out);
/* A per-sample histogram turned into pressure rows ("receivers", "Impulses" above) on DEVICE buffers: one launch, stream-ordered like
 * hare_hist_render_device -- no allocation, no free, no wait.  d_taps (B x T doubles) is a device buffer of the caller's; d_weight
 * nullable; of d_out (K x channels x out_stride doubles) the first n_out words of every row are WRITTEN (add == 0) or read and written
 * (add == 1), the rest never touched.  Behind hare_direct_device / hare_image_device / hare_image2_device on the same stream it renders
 * the paths those calls deposited; behind hare_hist_render_device, with add == 1 and out_stride that call's n_bins x M, it adds them onto
 * the noise rows; hare_decode_device may follow with N = out_stride.  Checked before anything runs (HARE_E_INVALID), in this order:
 * 1 <= K <= 65 536, n_bins >= 1, 1 <= B <= 8, channels 1, 4, 9 or 16, K x n_bins x B x channels <= 2^27; 1 <= T <= 1024;
 * 0 <= frac_bits <= 62; n0 >= 0, n_out >= 1, n0 + n_out <= n_bins + T - 1; out_stride >= n_out; K x channels x out_stride <= 2^28; add 0
 * or 1; null buffers; out overlapping the histogram, the weights or the taps.  Then HARE_E_NODEVICE, then HARE_E_STATE.  The scene names
 * the device; its geometry is not read. */
HARE_API int hare_hist_impulses_device(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void *d_hist,
                                       const void *d_weight /* nullable */, int32_t frac_bits, int32_t T, const void *d_taps, int64_t n0,
                                       int64_t n_out, int64_t out_stride, int32_t add, void *d_out, void *stream);
/* The same from host buffers: one allocation, upload, launch, download, one synchronisation.  out goes up first where the device must
 * see it: with add == 1, and with out_stride > n_out (the words between come down as they went up).  Also HARE_E_INVALID: a tap that is
 * not finite. */
HARE_API int hare_hist_impulses(hare_scene *s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t *hist,
                                const uint32_t *weight /* nullable */, int32_t frac_bits, int32_t T, const double *taps, int64_t n0,
                                int64_t n_out, int64_t out_stride, int32_t add, double *out);
/* The deterministic paths of the scene's source alone, from host buffers ("receivers", "Impulses" above): flags is a non-empty subset of
 * HARE_RECEIVE_DIRECT | HARE_RECEIVE_IMAGE | HARE_RECEIVE_IMAGE2 (_IMAGE2 only with _IMAGE) plus HARE_RECEIVE_DIRECTIONAL and the order
 * flags; anything else is HARE_E_INVALID, like 1 <= n_weight <= 2^53 and the receive calls' checks of kind, top_index, n_bins, bin_len,
 * frac_bits and the histogram's size.  A batch context is leased, the histogram zeroed, the three deposits enqueued as hare_receive_source
 * enqueues them (scratch sized from the scene options "image_max_pairs", "image2_max_cands", "image2_max_paths"), histogram, detections and
 * found-counts downloaded, one synchronisation.  An overflow of a list is HARE_E_NOMEM with hare_receive_source's message.  hist
 * (K x n_bins x B x channels uint64) and detections (K x 2 uint64) are WRITTEN.  With bin_len = c / fs the histogram is what
 * hare_hist_impulses takes.  HARE_E_STATE when no source or no receivers are set. */
HARE_API int hare_source_paths(hare_scene *s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins,
                               double bin_len, int32_t frac_bits, uint64_t *hist, uint64_t *detections);
/* The convolution of rows with a signal ("receivers", "Convolution" above) on DEVICE buffers: one launch, stream-ordered like
 * hare_hist_render_device -- no allocation, no free, no wait.  d_ir (R x N doubles), d_x (L doubles); d_y (R x n_out doubles) is WRITTEN,
 * every word once.  Behind hare_hist_render_device on the same stream, with d_ir its d_out, R = K x channels and N = n_bins x M, it convolves
 * the responses that call rendered.  Checked before anything runs (HARE_E_INVALID), in this order: 1 <= R <= 2^20, 1 <= N <= 2^24,
 * 1 <= L <= 2^28; n0 >= 0, n_out >= 1, n0 + n_out <= N + L - 1; R x n_out <= 2^28; R x n_out x min(N, L) <= HARE_CONVOLVE_MAX_TERMS; null
 * buffers; y overlapping ir or x.  Then HARE_E_NODEVICE, then HARE_E_STATE (the kernel is missing from the code object).  The scene names
 * the device; its geometry is not read. */
#define HARE_CONVOLVE_MAX_TERMS ((int64_t)1 << 44)
HARE_API int hare_convolve_device(hare_scene *s, int64_t R, int64_t N, const void *d_ir, int64_t L, const void *d_x, int64_t n0,
                                  int64_t n_out, void *d_y, void *stream);
/* The same from host buffers: one allocation, upload, convolve, download, one synchronisation. */
HARE_API int hare_convolve(hare_scene *s, int64_t R, int64_t N, const double *ir, int64_t L, const double *x, int64_t n0, int64_t n_out,
                           double *y);
/* The decoding of rows through a matrix of FIR filters ("receivers", "Decoding" above) on DEVICE buffers: one launch, stream-ordered like
 * hare_convolve_device -- no allocation, no free, no wait.  d_in (K x C x N doubles), d_h (O x C x T doubles); d_y (K x O x n_out doubles)
 * is WRITTEN, every word once.  Behind hare_hist_render_device on the same stream, with d_in its d_out, C = channels and N = n_bins x M, it
 * decodes the responses that call rendered; hare_convolve_device may follow on d_y with R = K x O.  Checked before anything runs
 * (HARE_E_INVALID), in this order: 1 <= K <= 65 536, 1 <= C <= 64, 1 <= O <= 64; 1 <= N <= 2^24, 1 <= T <= 2^16; n0 >= 0, n_out >= 1,
 * n0 + n_out <= N + T - 1; K x C x N <= 2^28 and K x O x n_out <= 2^28; K x O x n_out x C x min(N, T) <= HARE_DECODE_MAX_TERMS; null
 * buffers; y overlapping in or h.  Then HARE_E_NODEVICE, then HARE_E_STATE (the kernel is missing from the code object).  The scene names
 * the device; its geometry is not read. */
#define HARE_DECODE_MAX_TERMS ((int64_t)1 << 42)
HARE_API int hare_decode_device(hare_scene *s, int64_t K, int64_t C, int64_t N, const void *d_in, int64_t O, int64_t T, const void *d_h,
                                int64_t n0, int64_t n_out, void *d_y, void *stream);
/* The same from host buffers: one allocation, upload, decode, download, one synchronisation. */
HARE_API int hare_decode(hare_scene *s, int64_t K, int64_t C, int64_t N, const double *in, int64_t O, int64_t T, const double *h, int64_t n0,
                         int64_t n_out, double *y);
/* hare_receive_batch / hare_receive_source with `hist` replaced by the reduction's arguments: the loop runs as in the parent call, the
 * histogram stays on the device, the reduction is enqueued behind the last cast on the same stream, and sums, crossings, detections,
 * state and counters come down -- never the histogram.  K and B are the scene's; channels is 4 with HARE_RECEIVE_DIRECTIONAL (9, 16 with the order flags), else 1.
 * sums and cross are what hare_hist_reduce gives on the histogram the parent call returns.  Checks: the parent's, then the reduction's. */
HARE_API int hare_receive_batch_reduced(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, const hare_ray *rays,
                                        const int32_t *excl1, const int32_t *excl2, int32_t bounces, uint32_t flags, int32_t n_bins,
                                        double bin_len, int32_t frac_bits, const double *state_in, double *state_out,
                                        const uint32_t *weight /* nullable */, int32_t n_win, const int32_t *win, int32_t n_lev,
                                        const uint32_t *levels, uint64_t *sums, int32_t *cross, uint64_t *detections, hare_counters *ctr);
HARE_API int hare_receive_source_reduced(hare_scene *s, int32_t kind, int32_t top_index, int64_t n, int64_t first_ray, int32_t bounces,
                                         uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits, double *state_out,
                                         const uint32_t *weight /* nullable */, int32_t n_win, const int32_t *win, int32_t n_lev,
                                         const uint32_t *levels, uint64_t *sums, int32_t *cross, uint64_t *detections, hare_counters *ctr);

#ifdef __cplusplus
}
#endif
#endif /* HARE_HIP_H */
