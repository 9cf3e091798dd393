// bounce.cpp -- hare_bounce_batch: the device-resident specular bounce loop behind ONE C-ABI call from host buffers.
//
// Harness-defined: the reference leaves reflection to its caller, who re-shoots with
// poly_origin1 = the polygon just hit (Spatial_Partition.cs:33; Voxel_Grid.cs:351,477) after reflecting about
// Polygon.Normal (Hare_Geometry_Polygons.cs:161-171).  A managed caller holds no device pointers: done through
// hare_shoot_batch it would cross the host link (104 B per ray) every bounce and reflect in managed code.  Here the rays go
// up once, every cast and every reflection runs on the device, and what comes down is the X_Events the caller asks for.
//
// A call that wants the LAST cast's events only is enqueued once and synchronises once (below).  A call that wants every cast's
// events reads back, per cast, the 64-byte counter block (one stream synchronisation): the number of rays that hit is the
// number that live on.  When a quarter or more of the rays in flight have died since the last packing, the survivors are
// PACKED (hare_live_count / hare_scan_tiles / hare_reflect_compact: stable, so results and order are deterministic) and the
// next cast is launched on the survivors only -- SURVEY.md 7.1 step 9; in a closed room nearly nothing dies and the rays stay
// where they are (hare_reflect marks the few dead -2, the kernels skip them: HARE_SHOOT_RETIRED_RAYS).  Events of a packed
// cast are expanded to the caller's order on the device before they are downloaded.  The download of cast b runs beside
// cast b + 1 (it is issued after that cast's launches).
//
// Product code; nothing from oracle/.
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/hare_hip.h"
#include "scene.h"
#include "fan_out.h"

namespace hare {

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return hip_fail(H, _e, #expr);                                   \
    } while (0)

void free_bounce_buffers(const HipApi* H, Scene& s)
{
    for (Scene::BatchCtx& c : s.ctx) {
        Scene::BounceBuf& b = c.bounce;
        if (b.copy_st) { (void)H->StreamSynchronize(b.copy_st); (void)H->StreamDestroy(b.copy_st); b.copy_st = nullptr; }
        for (void** p : {&b.rays[0], &b.rays[1], &b.excl[0], &b.excl[1], &b.excl2, &b.idx[0], &b.idx[1], &b.ev[0], &b.ev[1], &b.full,
                         &b.tiles, &b.ctr, &b.state, &b.hist, &b.rain, &b.red, &b.direct, &b.image, &b.image2, &b.diffract, &b.spec2})
            dev_free(H, *p);
        b.cap = 0;
        b.ctr_cap = 0;
        b.state_cap = 0;
        b.hist_cap = 0;
        b.rain_cap = 0;
        b.red_cap = 0;
        b.direct_cap = 0;
        b.image_cap = 0;
        b.image2_cap = 0;
        b.diffract_cap = 0;
        b.spec2_cap = 0;
    }
}

namespace {

constexpr int64_t kCompactTile = 2048;          // kernels.hip: events per workgroup of the packing kernels
constexpr int64_t kPackMinRays = 16384;         // below this a cast is all launch latency: packing buys nothing

int ensure_bounce_buffers(const HipApi* H, Scene::BounceBuf& b, int64_t n, int32_t bounces)
{
    if (n > b.cap) {
        for (void** p : {&b.rays[0], &b.rays[1], &b.excl[0], &b.excl[1], &b.excl2, &b.idx[0], &b.idx[1], &b.ev[0], &b.ev[1], &b.full, &b.tiles})
            dev_free(H, *p);
        b.cap = 0;
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(H->Malloc(&b.rays[k], (size_t)n * sizeof(hare_ray)));
            HIP_TRY(H->Malloc(&b.excl[k], (size_t)n * sizeof(int32_t)));
            HIP_TRY(H->Malloc(&b.idx[k], (size_t)n * sizeof(int32_t)));
            HIP_TRY(H->Malloc(&b.ev[k], (size_t)n * sizeof(hare_xevent)));
        }
        HIP_TRY(H->Malloc(&b.excl2, (size_t)n * sizeof(int32_t)));
        HIP_TRY(H->Malloc(&b.full, (size_t)n * sizeof(hare_xevent)));
        HIP_TRY(H->Malloc(&b.tiles, (size_t)((n + kCompactTile - 1) / kCompactTile + 1) * sizeof(uint32_t)));
        b.cap = n;
    }
    if (bounces > b.ctr_cap) {
        dev_free(H, b.ctr);
        b.ctr_cap = 0;
        HIP_TRY(H->Malloc(&b.ctr, (size_t)bounces * sizeof(hare_counters)));
        b.ctr_cap = bounces;
    }
    if (!b.copy_st) HIP_TRY(H->StreamCreate(&b.copy_st));
    return HARE_OK;
}

// A device buffer of at least `bytes`: kept when it is large enough (0 bytes: always), else freed and allocated again
int grow(const HipApi* H, void*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap) return HARE_OK;
    dev_free(H, p);
    cap = 0;
    HIP_TRY(H->Malloc(&p, bytes));
    cap = bytes;
    return HARE_OK;
}

void fill_miss_host(hare_xevent* e, int64_t n)
{
    memset(e, 0, (size_t)n * sizeof(hare_xevent));          // X_Event(): Hare_Geometry_Primitives.cs:454-462
    for (int64_t i = 0; i < n; ++i) e[i].poly_id = -1;
}

// The loop for one scene (one device).  `stride` = distance between the casts of events_all (the whole batch's ray count when this
// is one shard of a sharded call).
int bounce_on_scene(Scene& s, const HipApi* H, Scene::BatchCtx& c, int32_t kind, int32_t top, int64_t n, const hare_ray* rays,
                    const int32_t* excl1, const int32_t* excl2, int32_t bounces, uint32_t flags, hare_xevent* events_all, int64_t stride,
                    hare_xevent* events_last, hare_counters* per_cast /* bounces entries, zeroed */)
{
    const DeviceModule& M = *s.module;
    if (!M.reflect || !M.live_count || !M.scan_tiles || !M.reflect_compact || !M.events_fill_miss || !M.events_expand) {
        set_error("hare_bounce_batch: bounce kernels missing from code object");
        return HARE_E_STATE;
    }
    Scene::BounceBuf& b = c.bounce;
    if (int rc = ensure_bounce_buffers(H, b, n, bounces)) return rc;
    if (!c.st[0]) HIP_TRY(H->StreamCreate(&c.st[0]));
    hipStream_t st = c.st[0];
    const void* polys = s.d_polys[(size_t)top];

    if (!events_all) {
        // ---- only the last cast's events are wanted: the whole loop is enqueued ONCE, with no host round trip between casts
        // (bounce_device_impl, launch.cpp: a launch per cast with the retired rays skipped -- or, under the scene option `bounce_fused`,
        // one launch for a Voxel_Grid where the pool kernel serves), and the call synchronises once, at its end.  No packing: a
        // retired ray costs its launch a record read and a miss record.  b.ev[1] serves as the loop's work array (2 n int32).
        HIP_TRY(H->MemcpyAsync(b.rays[0], rays, (size_t)n * sizeof(hare_ray), hipMemcpyHostToDevice, st));
        if (excl1) HIP_TRY(H->MemcpyAsync(b.excl[0], excl1, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (excl2) HIP_TRY(H->MemcpyAsync(b.excl2, excl2, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(H->MemsetAsync(b.ctr, 0, (size_t)bounces * sizeof(hare_counters), st));
        if (int rc = bounce_device_impl(s, H, kind, top, n, b.rays[0], excl1 ? b.excl[0] : nullptr, excl2 ? b.excl2 : nullptr, bounces, flags,
                                        b.ev[1], nullptr, b.ev[0], nullptr, b.ctr, st))
            return rc;
        if (events_last) HIP_TRY(H->MemcpyAsync(events_last, b.ev[0], (size_t)n * sizeof(hare_xevent), hipMemcpyDeviceToHost, st));
        HIP_TRY(H->MemcpyAsync(per_cast, b.ctr, (size_t)bounces * sizeof(hare_counters), hipMemcpyDeviceToHost, st));
        HIP_TRY(H->StreamSynchronize(st));
        return HARE_OK;
    }
    HIP_TRY(H->MemcpyAsync(b.rays[0], rays, (size_t)n * sizeof(hare_ray), hipMemcpyHostToDevice, st));
    if (excl1) HIP_TRY(H->MemcpyAsync(b.excl[0], excl1, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (excl2) HIP_TRY(H->MemcpyAsync(b.excl2, excl2, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(H->MemsetAsync(b.ctr, 0, (size_t)bounces * sizeof(hare_counters), st));

    int cur = 0;                 // which copy of rays / excl / idx the next cast reads
    int64_t m = n;               // rays in flight (packed: all of them live)
    bool packed = false;         // true: the arrays hold survivors only, idx maps them to the caller's positions
    bool marks = false;          // some of the m rays are dead and marked -2 (reflected in place since the last packing)

    auto shoot = [&](int cast) -> int {
        const void* e1 = (cast == 0) ? (excl1 ? b.excl[0] : nullptr) : b.excl[cur];
        const void* e2 = (cast == 0 && excl2) ? b.excl2 : nullptr;
        // the retire mark (-2) only means something to casts behind a reflection; a caller's own negative poly_origin excludes nothing
        const uint32_t f = (flags & ~HARE_SHOOT_RETIRED_RAYS) | ((cast > 0 && marks) ? HARE_SHOOT_RETIRED_RAYS : 0u);
        return shoot_device_impl(s, H, kind, top, m, b.rays[cur], e1, e2, f, b.ev[cast & 1], (hare_counters*)b.ctr + cast, st);
    };
    int rc = shoot(0);
    if (rc) return rc;

    for (int32_t cast = 0; cast < bounces; ++cast) {
        hare_xevent* dst = events_all ? events_all + (size_t)cast * (size_t)stride : ((cast == bounces - 1) ? events_last : nullptr);
        const void* src = b.ev[cast & 1];
        if (dst && packed) {     // back to the caller's order on the device
            unsigned blk = 256;
            long long nn = n, mm = m;
            void* full = b.full;
            const void* ev = b.ev[cast & 1];
            const void* idx = b.idx[cur];
            void* a1[] = {&full, &nn};
            if ((rc = launch(H, M.events_fill_miss, (unsigned)((n + blk - 1) / blk), blk, 0, st, a1))) return rc;
            void* a2[] = {&ev, &idx, &mm, &full};
            if ((rc = launch(H, M.events_expand, (unsigned)((m + blk - 1) / blk), blk, 0, st, a2))) return rc;
            src = b.full;
        }
        HIP_TRY(H->MemcpyAsync(&per_cast[cast], (hare_counters*)b.ctr + cast, sizeof(hare_counters), hipMemcpyDeviceToHost, st));
        HIP_TRY(H->StreamSynchronize(st));                  // cast `cast` (and its expansion) has finished; per_cast[cast] is here
        const int64_t hits = (int64_t)per_cast[cast].hits;
        const bool more = cast + 1 < bounces;
        if (more && hits > 0) {
            // ---- reflect, pack when it pays, and launch the NEXT cast before this cast's events go down the link
            unsigned blk = 256;
            const bool pack = hits * 4 <= m * 3 && m >= kPackMinRays;
            if (pack) {
                const long long mm = m, nt = (m + kCompactTile - 1) / kCompactTile;
                const void* ev = b.ev[cast & 1];
                void* tiles = b.tiles;
                void* total = (uint32_t*)b.tiles + nt;
                void* a1[] = {&ev, (void*)&mm, &tiles};
                if ((rc = launch(H, M.live_count, (unsigned)nt, 256, 0, st, a1))) return rc;
                void* a2[] = {&tiles, (void*)&nt, &total};
                if ((rc = launch(H, M.scan_tiles, 1, 1024, 0, st, a2))) return rc;
                const void* rin = b.rays[cur];
                const void* iin = packed ? b.idx[cur] : nullptr;
                void* rout = b.rays[cur ^ 1];
                void* eout = b.excl[cur ^ 1];
                void* iout = b.idx[cur ^ 1];
                void* a3[] = {&polys, &rin, &ev, &iin, &tiles, (void*)&mm, &rout, &eout, &iout};
                if ((rc = launch(H, M.reflect_compact, (unsigned)nt, 256, 0, st, a3))) return rc;
                cur ^= 1;
                m = hits;
                packed = true;
                marks = false;
            } else {
                long long mm = m;
                void* r = b.rays[cur];
                const void* ev = b.ev[cast & 1];
                void* ex = b.excl[cur];
                int32_t marks_valid = marks ? 1 : 0;       // excl[cur] carries the previous in-place reflection's marks: retired rays are not read again
                unsigned char* no_bytes = nullptr;
                void* a[] = {&polys, &r, &ev, &ex, &mm, &marks_valid, &no_bytes};
                if ((rc = launch(H, M.reflect, (unsigned)((m + blk - 1) / blk), blk, 0, st, a))) return rc;
                marks = true;
            }
            if ((rc = shoot(cast + 1))) return rc;
        }
        if (dst) {
            HIP_TRY(H->MemcpyAsync(dst, src, (size_t)n * sizeof(hare_xevent), hipMemcpyDeviceToHost, b.copy_st));
            HIP_TRY(H->StreamSynchronize(b.copy_st));
        }
        if (more && hits == 0) {       // nothing lives on: every later cast is all miss records, no ray counted
            for (int32_t k = cast + 1; k < bounces; ++k) {
                if (events_all) fill_miss_host(events_all + (size_t)k * (size_t)stride, n);
                else if (k == bounces - 1 && events_last) fill_miss_host(events_last, n);
            }
            break;
        }
    }
    HIP_TRY(H->StreamSynchronize(st));
    if (events_all && events_last) memcpy(events_last, events_all + (size_t)(bounces - 1) * (size_t)stride, (size_t)n * sizeof(hare_xevent));
    return HARE_OK;
}

// hare_receive_batch: what one scene's share of the rays computes, into host buffers.  The state planes of the caller's arrays are
// `stride` doubles apart (the whole batch's n); hist / det are this scene's own (written).
struct ReceiveJob {
    int32_t n_bins = 1;
    double bin_len = 1;
    int32_t frac_bits = 0;
    const double* state_in = nullptr;
    double* state_out = nullptr;
    int64_t stride = 0;
    uint64_t* hist = nullptr;
    uint64_t* det = nullptr;
    int64_t ray_base = 0;      // this shard's first ray in the whole batch (the scattering RNG's global ray index)
    uint32_t flags = 0;        // the call's HARE_RECEIVE_* bits
    bool from_source = false;  // hare_receive_source: rays and state come from hare_emit_source (rays from ray_base on), not from the caller
    int64_t direct_weight = 0; // HARE_RECEIVE_DIRECT: > 0 in the ONE scene that deposits the direct sound, for the call's whole n (else 0)
    int64_t image_weight = 0;  // HARE_RECEIVE_IMAGE: the same for the first-order image sources
    int64_t image2_weight = 0; // HARE_RECEIVE_IMAGE2: the same for the second-order image sources
    const char* who = "hare_receive_batch";
    // hare_receive_*_reduced: the histogram stays in BounceBuf::hist and hare_hist_reduce runs behind the last cast; sums and cross come
    // down in its place (hist is null)
    const ReduceSpec* reduce = nullptr;
    uint64_t* sums = nullptr;
    int32_t* cross = nullptr;
};

// The receive loop for one scene: rays, exclusions and state go up, the loop is enqueued ONCE (a launch per cast, hare_receive_reflect
// behind each), histogram, detections, final state and per-cast counters come down, one synchronisation -- hare_bounce_batch's
// last-cast-only path.  No events are downloaded.  job.from_source: nothing goes up -- the scene's source emits rays and state on the stream.
int receive_on_scene(Scene& s, const HipApi* H, Scene::BatchCtx& c, int32_t kind, int32_t top, int64_t n, const hare_ray* rays,
                     const int32_t* excl1, const int32_t* excl2, int32_t bounces, uint32_t flags, const ReceiveJob& job, hare_counters* per_cast)
{
    Scene::BounceBuf& b = c.bounce;
    if (int rc = ensure_bounce_buffers(H, b, n, bounces)) return rc;
    const int32_t B = scene_bands(s, top);
    const size_t K = s.rcv.size() / 4;
    const size_t state_bytes = (size_t)n * (size_t)(1 + B) * sizeof(double);
    const size_t hist_words = receive_hist_words(s, top, job.n_bins, job.flags), hist_bytes = (hist_words + 2 * K) * sizeof(uint64_t);
    if (int rc = grow(H, b.state, b.state_cap, state_bytes)) return rc;
    if (int rc = grow(H, b.hist, b.hist_cap, hist_bytes)) return rc;
    const bool rain = receive_rains(s, top, job.flags);
    if (int rc = grow(H, b.rain, b.rain_cap, rain ? (size_t)HARE_RECEIVE_RAIN_WORK_BYTES(n) : 0)) return rc;
    // the reduction's own block: sums, crossings, weights, each from a 16-byte boundary
    const ReduceSpec* const red = job.reduce;
    const size_t sums_bytes = red ? K * (size_t)B * (size_t)red->n_win * 4 * sizeof(uint64_t) : 0;
    const size_t cross_words = red ? K * (size_t)B * (size_t)red->n_lev : 0, cross_bytes = (cross_words * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t weight_bytes = red && red->weight ? (size_t)job.n_bins * (size_t)B * sizeof(uint32_t) : 0;
    if (int rc = grow(H, b.red, b.red_cap, red ? sums_bytes + cross_bytes + weight_bytes : 0)) return rc;
    if (int rc = grow(H, b.direct, b.direct_cap, job.direct_weight > 0 ? (size_t)HARE_DIRECT_WORK_BYTES(K) : 0)) return rc;
    const int64_t image_pairs = s.opt.image_max_pairs;
    if (int rc = grow(H, b.image, b.image_cap, job.image_weight > 0 ? (size_t)HARE_IMAGE_WORK_BYTES(K, s.topos[(size_t)top].P, image_pairs) : 0)) return rc;
    const int64_t image2_cands = s.opt.image2_max_cands, image2_paths = s.opt.image2_max_paths;
    if (int rc = grow(H, b.image2, b.image2_cap, job.image2_weight > 0 ? (size_t)HARE_IMAGE2_WORK_BYTES(s.topos[(size_t)top].P, image2_cands, image2_paths) : 0))
        return rc;
    // the loop's byte per ray (ReceiveArgs::spec2): only a topology with a scattering table reads or writes it
    const bool spec2 = (job.flags & HARE_RECEIVE_IMAGE2) && scene_has_scattering(s, top);
    if (int rc = grow(H, b.spec2, b.spec2_cap, spec2 ? (size_t)HARE_RECEIVE_IMAGE2_WORK_BYTES(n) : 0)) return rc;
    if (!c.st[0]) HIP_TRY(H->StreamCreate(&c.st[0]));
    hipStream_t st = c.st[0];
    uint64_t* const d_hist = (uint64_t*)b.hist;
    uint64_t* const d_det = d_hist + hist_words;
    double* const d_state = (double*)b.state;
    if (job.from_source) {
        if (int rc = emit_source(s, H, n, job.ray_base, b.rays[0], d_state, st)) return rc;
    } else {
        HIP_TRY(H->MemcpyAsync(b.rays[0], rays, (size_t)n * sizeof(hare_ray), hipMemcpyHostToDevice, st));
    }
    if (excl1) HIP_TRY(H->MemcpyAsync(b.excl[0], excl1, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (excl2) HIP_TRY(H->MemcpyAsync(b.excl2, excl2, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (job.state_in)
        for (int32_t p = 0; p <= B; ++p)
            HIP_TRY(H->MemcpyAsync(d_state + (size_t)p * (size_t)n, job.state_in + (size_t)p * (size_t)job.stride, (size_t)n * sizeof(double),
                                   hipMemcpyHostToDevice, st));
    HIP_TRY(H->MemsetAsync(b.hist, 0, hist_bytes, st));
    HIP_TRY(H->MemsetAsync(b.ctr, 0, (size_t)bounces * sizeof(hare_counters), st));
    void* const work = rain ? b.rain : b.ev[1];         // b.ev[1] holds the loop's 2 n int32; with rain, a buffer of its own holds them and the rain's scratch
    if (job.direct_weight > 0)      // the direct sound, once per call, ahead of cast 0 (whose receiver step the flag switches off)
        if (int rc = direct_enqueue(s, H, kind, top, job.direct_weight, job.flags, job.n_bins, job.bin_len, job.frac_bits, b.direct, d_hist, d_det, st))
            return rc;
    if (job.image_weight > 0)       // the first-order image sources, once per call (cast 1's receiver step is switched off for the specular rays)
        if (int rc = image_enqueue(s, H, kind, top, job.image_weight, job.flags, job.n_bins, job.bin_len, job.frac_bits, image_pairs, b.image, d_hist,
                                   d_det, st))
            return rc;
    if (job.image2_weight > 0)      // the second-order image sources, once per call (cast 2's receiver step is switched off for the twice-specular rays)
        if (int rc = image2_enqueue(s, H, kind, top, job.image2_weight, job.flags, job.n_bins, job.bin_len, job.frac_bits, image2_cands, image2_paths,
                                    b.image2, d_hist, d_det, st))
            return rc;
    ReceivePlan plan;
    if (int rc = receive_plan(s, top, job.flags, n, job.n_bins, job.bin_len, job.frac_bits, d_state, d_hist, d_det, work,
                              job.state_in == nullptr && !job.from_source, job.ray_base, plan))
        return rc;
    if (plan.args.spec2) plan.args.spec2 = (unsigned char*)b.spec2;      // the host calls keep the byte per ray in a buffer of its own, not behind `work`
    if (int rc = bounce_device_impl(s, H, kind, top, n, b.rays[0], excl1 ? b.excl[0] : nullptr, excl2 ? b.excl2 : nullptr, bounces, flags, work,
                                    nullptr, b.ev[0], nullptr, b.ctr, st, &plan))
        return rc;
    if (red) {
        char* const d_sums = (char*)b.red;
        char* const d_cross = d_sums + sums_bytes;
        char* const d_weight = d_cross + cross_bytes;
        if (weight_bytes) HIP_TRY(H->MemcpyAsync(d_weight, red->weight, weight_bytes, hipMemcpyHostToDevice, st));
        if (int rc = reduce_enqueue(s, H, (int32_t)K, job.n_bins, B, receive_channels(job.flags), d_hist,
                                    weight_bytes ? d_weight : nullptr, *red, d_sums, d_cross, st))
            return rc;
        if (sums_bytes) HIP_TRY(H->MemcpyAsync(job.sums, d_sums, sums_bytes, hipMemcpyDeviceToHost, st));
        if (cross_words) HIP_TRY(H->MemcpyAsync(job.cross, d_cross, cross_words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        HIP_TRY(H->MemcpyAsync(job.hist, d_hist, hist_words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(H->MemcpyAsync(job.det, d_det, 2 * K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (job.state_out)
        for (int32_t p = 0; p <= B; ++p)
            HIP_TRY(H->MemcpyAsync(job.state_out + (size_t)p * (size_t)job.stride, d_state + (size_t)p * (size_t)n, (size_t)n * sizeof(double),
                                   hipMemcpyDeviceToHost, st));
    HIP_TRY(H->MemcpyAsync(per_cast, b.ctr, (size_t)bounces * sizeof(hare_counters), hipMemcpyDeviceToHost, st));
    uint64_t image_found = 0;       // the pairs the search found: the last download, so that no return lies between it and the wait
    if (job.image_weight > 0) HIP_TRY(H->MemcpyAsync(&image_found, b.image, sizeof image_found, hipMemcpyDeviceToHost, st));
    uint64_t image2_found[2] = {0, 0};      // candidates and paths
    if (job.image2_weight > 0) HIP_TRY(H->MemcpyAsync(image2_found, b.image2, sizeof image2_found, hipMemcpyDeviceToHost, st));
    HIP_TRY(H->StreamSynchronize(st));
    if (image2_found[0] > (uint64_t)image2_cands || image2_found[1] > (uint64_t)image2_paths) {      // nothing of the second order was deposited
        set_error(std::string(job.who) + ": the scene yields " + std::to_string(image2_found[0]) + " second-order candidates and " +
                  (image2_found[0] > (uint64_t)image2_cands ? std::string("an unknown number of") : std::to_string(image2_found[1])) +
                  " paths, \"image2_max_cands\" is " + std::to_string(image2_cands) + " and \"image2_max_paths\" " + std::to_string(image2_paths) +
                  " (needed: " + std::to_string(image2_found[0]) + ", " + std::to_string(image2_found[1]) + ")");
        return HARE_E_NOMEM;
    }
    if (image_found > (uint64_t)image_pairs) {      // the deposit kernels added nothing: the caller's results hold no image sources
        set_error(std::string(job.who) + ": the scene yields " + std::to_string(image_found) + " image-source pairs, \"image_max_pairs\" is " +
                  std::to_string(image_pairs) + " (needed: " + std::to_string(image_found) + ")");
        return HARE_E_NOMEM;
    }
    return HARE_OK;
}

int check_args(const char* who, int64_t n, const hare_ray* rays, int32_t bounces, hare_xevent* events_all, hare_xevent* events_last)
{
    if (n < 0 || bounces < 1 || bounces > 4096 || (n > 0 && !rays)) {
        set_error(std::string(who) + ": bad arguments (n >= 0, 1 <= bounces <= 4096, rays)");
        return HARE_E_INVALID;
    }
    (void)events_all;
    (void)events_last;
    return HARE_OK;
}

int bounce_one(hare_scene* s, int32_t kind, int32_t top, int64_t n, const hare_ray* rays, const int32_t* excl1, const int32_t* excl2,
               int32_t bounces, uint32_t flags, hare_xevent* events_all, int64_t stride, hare_xevent* events_last, hare_counters* per_cast,
               const ReceiveJob* job = nullptr)
{
    if (top < 0 || top >= (int32_t)s->topos.size()) {
        set_error("hare_bounce_batch: bad top_index");
        return HARE_E_INVALID;
    }
    // host-buffer callers: the reference's meaning of poly_origin (a negative index excludes nothing); no developer bits, no
    // origin write-back (the rays are the caller's constant input here)
    flags = sanitize_flags(*s, flags) & (HARE_SHOOT_COUNT_WORK | HARE_SHOOT_SIMPLE_KERNEL);
    DeviceGuard dev_guard(hip_api(nullptr), s->device);
    const HipApi* H = nullptr;
    std::unique_lock<std::mutex> lk(s->mu);
    int rc = ensure_device(*s, H);
    if (rc) return rc;
    rc = upload_polys(*s, H);
    if (rc) return rc;
    if (job && (rc = receive_ready(*s, H, job->who))) return rc;
    if (job && job->from_source && (rc = source_ready(*s, H, job->who))) return rc;
    if (n == 0) return HARE_OK;
    const CtxLease lease(*s, lk, [n](const Scene::BatchCtx& x) { return x.bounce.cap >= n; });       // (releases lk)
    Scene::BatchCtx* const c = lease.get();
    rc = job ? receive_on_scene(*s, H, *c, kind, top, n, rays, excl1, excl2, bounces, flags, *job, per_cast)
                       : bounce_on_scene(*s, H, *c, kind, top, n, rays, excl1, excl2, bounces, flags, events_all, stride, events_last, per_cast);
    if (rc != HARE_OK) {          // copies into the caller's buffers may still be in flight: drain before the error returns
        if (c->st[0]) (void)H->StreamSynchronize(c->st[0]);
        if (c->bounce.copy_st) (void)H->StreamSynchronize(c->bounce.copy_st);
    }
    return rc;
}

// one shard's counters per cast into the call's total and (nullable both) its per-cast array
void add_cast_counters(hare_counters* ctr, hare_counters* ctr_per_cast, const std::vector<hare_counters>& pc)
{
    for (size_t b = 0; b < pc.size(); ++b) {
        if (ctr) add_counters(*ctr, pc[b]);
        if (ctr_per_cast) add_counters(ctr_per_cast[b], pc[b]);
    }
}

}  // namespace
}  // namespace hare

using namespace hare;

extern "C" {

int hare_bounce_batch(hare_scene* s, int32_t kind, int32_t top_index, int64_t n, const hare_ray* rays, const int32_t* excl1,
                      const int32_t* excl2, int32_t bounces, uint32_t flags, hare_xevent* events_all, hare_xevent* events_last,
                      hare_counters* ctr, hare_counters* ctr_per_cast)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (int rc = check_args("hare_bounce_batch", n, rays, bounces, events_all, events_last)) return rc;
    GUARD_BEGIN
    std::vector<hare_counters> pc((size_t)bounces);
    memset(pc.data(), 0, pc.size() * sizeof(hare_counters));
    if (ctr) memset(ctr, 0, sizeof *ctr);
    if (ctr_per_cast) memset(ctr_per_cast, 0, (size_t)bounces * sizeof(hare_counters));
    const int rc = bounce_one(s, kind, top_index, n, rays, excl1, excl2, bounces, flags, events_all, n, events_last, pc.data());
    if (rc) return rc;
    add_cast_counters(ctr, ctr_per_cast, pc);
    return HARE_OK;
    GUARD_END
}

int hare_bounce_batch_sharded(hare_scene* const* scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                              const hare_ray* rays, const int32_t* excl1, const int32_t* excl2, int32_t bounces, uint32_t flags,
                              hare_xevent* events_all, hare_xevent* events_last, hare_counters* ctr, hare_counters* ctr_per_cast)
{
    if (int rc = check_scenes("hare_bounce_batch_sharded", scenes, n_scenes)) return rc;
    if (int rc = check_args("hare_bounce_batch_sharded", n, rays, bounces, events_all, events_last)) return rc;
    GUARD_BEGIN
    const int G = n_scenes;
    std::vector<std::vector<hare_counters>> pcs((size_t)G, std::vector<hare_counters>((size_t)bounces));      // (zeroed)
    const FanResult f = fan_out(G, "hare_bounce_batch_sharded: exception in a shard", [&](int k) {
        const PartRange r = part_range(n, k, G);
        return bounce_one(scenes[k], kind, top_index, r.size(), rays ? rays + r.lo : nullptr, excl1 ? excl1 + r.lo : nullptr,
                          excl2 ? excl2 + r.lo : nullptr, bounces, flags, events_all ? events_all + r.lo : nullptr, n,
                          events_last ? events_last + r.lo : nullptr, pcs[(size_t)k].data());
    });
    if (f.rc != HARE_OK) {
        set_error(f.shard_text());
        return f.rc;
    }
    if (ctr) memset(ctr, 0, sizeof *ctr);
    if (ctr_per_cast) memset(ctr_per_cast, 0, (size_t)bounces * sizeof(hare_counters));
    for (const std::vector<hare_counters>& pc : pcs) add_cast_counters(ctr, ctr_per_cast, pc);
    return HARE_OK;
    GUARD_END
}

}  // extern "C"

// hare_receive_batch / _sharded and, with first_ray non-null, hare_receive_source / _sharded: the same call with the upload of rays and
// state replaced by the source's emission (shard k emits the rays from *first_ray + lo on)
static int receive_sharded(const char* who, hare_scene* const* scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n,
                           const hare_ray* rays, const int32_t* excl1, const int32_t* excl2, int32_t bounces, uint32_t flags, int32_t n_bins,
                           double bin_len, int32_t frac_bits, const double* state_in, double* state_out, uint64_t* hist, uint64_t* detections,
                           hare_counters* ctr, const int64_t* first_ray, const ReduceSpec* red = nullptr, uint64_t* sums = nullptr,
                           int32_t* cross = nullptr)
{
    if (int rc = check_scenes(who, scenes, n_scenes, true)) return rc;
    hare_scene* const s0 = scenes[0];
    if (int rc = receive_check_args(who, *s0, flags, kind, top_index, n, bounces, n_bins, bin_len, frac_bits)) return rc;
    if ((flags & HARE_RECEIVE_DIRECT) && !first_ray) {      // the caller's rays: the library cannot know them to be the source's
        set_error(std::string(who) + ": HARE_RECEIVE_DIRECT needs the scene's source (hare_receive_source, hare_receive_device + hare_direct_device)");
        return HARE_E_INVALID;
    }
    if ((flags & HARE_RECEIVE_IMAGE) && !first_ray) {
        set_error(std::string(who) + ": HARE_RECEIVE_IMAGE needs the scene's source (hare_receive_source, hare_receive_device + hare_image_device)");
        return HARE_E_INVALID;
    }
    if ((flags & HARE_RECEIVE_IMAGE2) && !first_ray) {
        set_error(std::string(who) + ": HARE_RECEIVE_IMAGE2 needs the scene's source (hare_receive_source, hare_receive_device + hare_image2_device)");
        return HARE_E_INVALID;
    }
    if ((n > 0 && !rays && !first_ray) || (!hist && !red) || !detections) {
        set_error(std::string(who) + ": null rays, histogram or detections");
        return HARE_E_INVALID;
    }
    if (red && n_scenes != 1) {      // a crossing is not additive over shards
        set_error(std::string(who) + ": the reduction runs on one scene");
        return HARE_E_INVALID;
    }
    if (red) {      // the _reduced calls: the reduction's own checks, at the histogram's shape
        const size_t K1 = std::max<size_t>(1, s0->rcv.size() / 4), KB = K1 * (size_t)scene_bands(*s0, top_index);
        if (int rc = reduce_check_spec(who, (int64_t)K1, n_bins, scene_bands(*s0, top_index), receive_channels(flags), *red)) return rc;
        if ((red->n_win > 0 && !sums) || (red->n_lev > 0 && !cross)) {
            set_error(std::string(who) + ": null sums / crossings");
            return HARE_E_INVALID;
        }
        // the two new outputs against each other and the rest; the parent's buffers are checked as the parent checks them
        if (spans_overlap({{sums, KB * (size_t)red->n_win * 4 * sizeof(uint64_t)},
                           {cross, KB * (size_t)red->n_lev * sizeof(int32_t)},
                           {detections, K1 * 2 * sizeof(uint64_t)},
                           {state_out, (size_t)n * (size_t)(1 + scene_bands(*s0, top_index)) * sizeof(double)},
                           {red->weight, (size_t)n_bins * (size_t)scene_bands(*s0, top_index) * sizeof(uint32_t)}}, 2)) {
            set_error(std::string(who) + ": sums, crossings, detections, state and weights must not overlap");
            return HARE_E_INVALID;
        }
    }
    if (first_ray) {
        if (int rc = source_check_range(who, n, *first_ray)) return rc;
        if (s0->src.set && s0->src.B != scene_bands(*s0, top_index)) {
            set_error(std::string(who) + ": the source has " + std::to_string(s0->src.B) + " bands, the topology " +
                      std::to_string(scene_bands(*s0, top_index)));
            return HARE_E_INVALID;
        }
        for (int32_t k = 1; k < n_scenes; ++k)
            if (!scenes[k]->src.same_as(s0->src) || scenes[k]->opt.source_seed != s0->opt.source_seed) {
                set_error(std::string(who) + ": the scenes differ in source or source_seed");
                return HARE_E_INVALID;
            }
    }
    auto sigma_of = [&](const Scene& s) -> const std::vector<double>* {
        return scene_has_scattering(s, top_index) ? &s.sigma[(size_t)top_index].host : nullptr;
    };
    for (int32_t k = 1; k < n_scenes; ++k) {     // the shards must compute the same thing
        const std::vector<double>* sk = sigma_of(*scenes[k]);
        const std::vector<double>* s0s = sigma_of(*s0);
        const Scene::ReceiverMap &mk = scenes[k]->rmap, &m0 = s0->rmap;      // the same receivers through the same loop: a map's grid too
        if (scenes[k]->rcv != s0->rcv || mk.set != m0.set || (m0.set && (mk.h != m0.h || mk.start != m0.start || mk.items != m0.items)) ||
            scene_bands(*scenes[k], top_index) != scene_bands(*s0, top_index) ||
            (top_index < (int32_t)scenes[k]->topos.size() ? scenes[k]->topos[(size_t)top_index].P : -1) != s0->topos[(size_t)top_index].P) {
            set_error(std::string(who) + ": the scenes differ in receivers, bands or polygons");
            return HARE_E_INVALID;
        }
        if ((sk == nullptr) != (s0s == nullptr) || (sk && *sk != *s0s) || (s0s && scenes[k]->opt.scatter_seed != s0->opt.scatter_seed)) {
            set_error(std::string(who) + ": the scenes differ in scattering tables or scatter_seed");
            return HARE_E_INVALID;
        }
        const bool roulette = s0->opt.receive_floor_bits > 0 && s0->opt.receive_roulette != 0;      // draws from "scatter_seed" without a table too
        if (scenes[k]->opt.receive_floor_bits != s0->opt.receive_floor_bits || scenes[k]->opt.receive_roulette != s0->opt.receive_roulette ||
            (roulette && scenes[k]->opt.scatter_seed != s0->opt.scatter_seed)) {
            set_error(std::string(who) + ": the scenes differ in receive_floor_bits, receive_roulette or (with roulette) scatter_seed");
            return HARE_E_INVALID;
        }
    }
    GUARD_BEGIN
    const int G = n_scenes;
    const size_t K = s0->rcv.size() / 4, hist_words = receive_hist_words(*s0, top_index, n_bins, flags);
    if (hist) memset(hist, 0, hist_words * sizeof(uint64_t));
    if (red) {      // n == 0 runs nothing: the reduction of an empty histogram
        if (red->n_win > 0) memset(sums, 0, K * (size_t)scene_bands(*s0, top_index) * (size_t)red->n_win * 4 * sizeof(uint64_t));
        if (red->n_lev > 0) memset(cross, 0, K * (size_t)scene_bands(*s0, top_index) * (size_t)red->n_lev * sizeof(int32_t));
    }
    memset(detections, 0, 2 * K * sizeof(uint64_t));
    if (ctr) memset(ctr, 0, sizeof *ctr);
    std::vector<std::vector<hare_counters>> pcs((size_t)G, std::vector<hare_counters>((size_t)bounces));      // (zeroed)
    std::vector<std::vector<uint64_t>> hists((size_t)G), dets((size_t)G);    // shard 0 writes the caller's arrays
    for (int k = 1; k < G; ++k) {
        hists[(size_t)k].assign(hist_words, 0);
        dets[(size_t)k].assign(2 * K, 0);
    }
    auto shard = [&](int k) -> int {
        const int64_t lo = part_range(n, k, G).lo, hi = part_range(n, k, G).hi;
        ReceiveJob job;
        job.n_bins = n_bins;
        job.bin_len = bin_len;
        job.frac_bits = frac_bits;
        job.state_in = state_in ? state_in + lo : nullptr;
        job.state_out = state_out ? state_out + lo : nullptr;
        job.stride = n;
        job.hist = k == 0 ? hist : hists[(size_t)k].data();
        job.det = k == 0 ? detections : dets[(size_t)k].data();
        job.ray_base = (first_ray ? *first_ray : 0) + lo;
        job.flags = flags;
        job.from_source = first_ray != nullptr;
        // the direct sound is deposited once, for the whole n: by the first scene whose shard holds a ray (scenes[0] whenever n >= G)
        job.direct_weight = ((flags & HARE_RECEIVE_DIRECT) && hi > lo && lo == 0) ? n : 0;
        job.image_weight = ((flags & HARE_RECEIVE_IMAGE) && hi > lo && lo == 0) ? n : 0;
        job.image2_weight = ((flags & HARE_RECEIVE_IMAGE2) && hi > lo && lo == 0) ? n : 0;
        job.who = who;
        job.reduce = red;
        job.sums = sums;
        job.cross = cross;
        return bounce_one(scenes[k], kind, top_index, hi - lo, rays ? rays + lo : nullptr, excl1 ? excl1 + lo : nullptr,
                          excl2 ? excl2 + lo : nullptr, bounces, flags, nullptr, n, nullptr, pcs[(size_t)k].data(), &job);
    };
    const std::string thrown = std::string(who) + ": exception in a shard";
    const FanResult f = fan_out(G, thrown.c_str(), shard);
    if (f.rc != HARE_OK) {
        set_error(G == 1 ? f.text : f.shard_text());
        return f.rc;
    }
    for (int k = 1; k < G; ++k) {                 // integer sums (mod 2^64, so right for the signed channels too): the order of the shards does not matter
        for (size_t w = 0; w < hist_words; ++w) hist[w] += hists[(size_t)k][w];
        for (size_t w = 0; w < 2 * K; ++w) detections[w] += dets[(size_t)k][w];
    }
    for (const std::vector<hare_counters>& pc : pcs) add_cast_counters(ctr, nullptr, pc);
    return HARE_OK;
    GUARD_END
}

extern "C" {

int hare_receive_batch(hare_scene* s, int32_t kind, int32_t top_index, int64_t n, const hare_ray* rays, const int32_t* excl1,
                       const int32_t* excl2, int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits,
                       const double* state_in, double* state_out, uint64_t* hist, uint64_t* detections, hare_counters* ctr)
{
    hare_scene* const one[1] = {s};
    return receive_sharded("hare_receive_batch", one, 1, kind, top_index, n, rays, excl1, excl2, bounces, flags, n_bins, bin_len, frac_bits,
                           state_in, state_out, hist, detections, ctr, nullptr);
}

int hare_receive_batch_sharded(hare_scene* const* scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n, const hare_ray* rays,
                               const int32_t* excl1, const int32_t* excl2, int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len,
                               int32_t frac_bits, const double* state_in, double* state_out, uint64_t* hist, uint64_t* detections,
                               hare_counters* ctr)
{
    return receive_sharded(n_scenes == 1 ? "hare_receive_batch" : "hare_receive_batch_sharded", scenes, n_scenes, kind, top_index, n, rays, excl1,
                           excl2, bounces, flags, n_bins, bin_len, frac_bits, state_in, state_out, hist, detections, ctr, nullptr);
}

int hare_receive_source(hare_scene* s, int32_t kind, int32_t top_index, int64_t n, int64_t first_ray, int32_t bounces, uint32_t flags,
                        int32_t n_bins, double bin_len, int32_t frac_bits, double* state_out, uint64_t* hist, uint64_t* detections,
                        hare_counters* ctr)
{
    hare_scene* const one[1] = {s};
    return receive_sharded("hare_receive_source", one, 1, kind, top_index, n, nullptr, nullptr, nullptr, bounces, flags, n_bins, bin_len,
                           frac_bits, nullptr, state_out, hist, detections, ctr, &first_ray);
}

int hare_receive_source_sharded(hare_scene* const* scenes, int32_t n_scenes, int32_t kind, int32_t top_index, int64_t n, int64_t first_ray,
                                int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits, double* state_out,
                                uint64_t* hist, uint64_t* detections, hare_counters* ctr)
{
    return receive_sharded(n_scenes == 1 ? "hare_receive_source" : "hare_receive_source_sharded", scenes, n_scenes, kind, top_index, n, nullptr,
                           nullptr, nullptr, bounces, flags, n_bins, bin_len, frac_bits, nullptr, state_out, hist, detections, ctr, &first_ray);
}

}  // extern "C"

// hare_source_paths: the deterministic paths from the scene's source alone -- the direct sound and the image sources of the first and the
// second order -- deposited into a zeroed histogram from host buffers (include/hare_hip.h, "receivers", "Impulses").  What receive_on_scene
// enqueues ahead of cast 0, in its order and through the same three plans, and nothing of the loop: the histogram and the detections are
// zeroed, direct_enqueue / image_enqueue / image2_enqueue run on the context's stream with scratch sized from the scene's options, the
// histogram, the detections and the found-counts come down, one synchronisation
static int source_paths_on_scene(Scene& s, const HipApi* H, Scene::BatchCtx& c, int32_t kind, int32_t top, int64_t n_weight, uint32_t flags,
                                 int32_t n_bins, double bin_len, int32_t frac_bits, uint64_t* hist, uint64_t* det)
{
    Scene::BounceBuf& b = c.bounce;
    const size_t K = s.rcv.size() / 4, P = (size_t)s.topos[(size_t)top].P;
    const size_t hist_words = receive_hist_words(s, top, n_bins, flags), hist_bytes = (hist_words + 2 * K) * sizeof(uint64_t);
    const bool direct = (flags & HARE_RECEIVE_DIRECT) != 0, image = (flags & HARE_RECEIVE_IMAGE) != 0, image2 = (flags & HARE_RECEIVE_IMAGE2) != 0;
    const int64_t image_pairs = s.opt.image_max_pairs, image2_cands = s.opt.image2_max_cands, image2_paths = s.opt.image2_max_paths;
    if (int rc = grow(H, b.hist, b.hist_cap, hist_bytes)) return rc;
    if (int rc = grow(H, b.direct, b.direct_cap, direct ? (size_t)HARE_DIRECT_WORK_BYTES(K) : 0)) return rc;
    if (int rc = grow(H, b.image, b.image_cap, image ? (size_t)HARE_IMAGE_WORK_BYTES(K, P, image_pairs) : 0)) return rc;
    if (int rc = grow(H, b.image2, b.image2_cap, image2 ? (size_t)HARE_IMAGE2_WORK_BYTES(P, image2_cands, image2_paths) : 0)) return rc;
    if (!c.st[0]) HIP_TRY(H->StreamCreate(&c.st[0]));
    hipStream_t st = c.st[0];
    uint64_t* const d_hist = (uint64_t*)b.hist;
    uint64_t* const d_det = d_hist + hist_words;
    HIP_TRY(H->MemsetAsync(b.hist, 0, hist_bytes, st));
    if (direct)
        if (int rc = direct_enqueue(s, H, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, b.direct, d_hist, d_det, st)) return rc;
    if (image)
        if (int rc = image_enqueue(s, H, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, image_pairs, b.image, d_hist, d_det, st)) return rc;
    if (image2)
        if (int rc = image2_enqueue(s, H, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, image2_cands, image2_paths, b.image2, d_hist, d_det, st))
            return rc;
    HIP_TRY(H->MemcpyAsync(hist, d_hist, hist_words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(H->MemcpyAsync(det, d_det, 2 * K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    uint64_t image_found = 0;       // the last downloads, so that no return lies between them and the wait
    if (image) HIP_TRY(H->MemcpyAsync(&image_found, b.image, sizeof image_found, hipMemcpyDeviceToHost, st));
    uint64_t image2_found[2] = {0, 0};
    if (image2) HIP_TRY(H->MemcpyAsync(image2_found, b.image2, sizeof image2_found, hipMemcpyDeviceToHost, st));
    HIP_TRY(H->StreamSynchronize(st));
    const std::string who = "hare_source_paths";
    if (image2_found[0] > (uint64_t)image2_cands || image2_found[1] > (uint64_t)image2_paths) {      // receive_on_scene's messages
        set_error(who + ": the scene yields " + std::to_string(image2_found[0]) + " second-order candidates and " +
                  (image2_found[0] > (uint64_t)image2_cands ? std::string("an unknown number of") : std::to_string(image2_found[1])) +
                  " paths, \"image2_max_cands\" is " + std::to_string(image2_cands) + " and \"image2_max_paths\" " + std::to_string(image2_paths) +
                  " (needed: " + std::to_string(image2_found[0]) + ", " + std::to_string(image2_found[1]) + ")");
        return HARE_E_NOMEM;
    }
    if (image_found > (uint64_t)image_pairs) {
        set_error(who + ": the scene yields " + std::to_string(image_found) + " image-source pairs, \"image_max_pairs\" is " +
                  std::to_string(image_pairs) + " (needed: " + std::to_string(image_found) + ")");
        return HARE_E_NOMEM;
    }
    return HARE_OK;
}

extern "C" int hare_source_paths(hare_scene* s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                                 int32_t frac_bits, uint64_t* hist, uint64_t* detections)
{
    const char* const who = "hare_source_paths";
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    const uint32_t paths = HARE_RECEIVE_DIRECT | HARE_RECEIVE_IMAGE | HARE_RECEIVE_IMAGE2;
    if (flags & ~(paths | kReceiveChannelFlags))
        return bad("flags other than HARE_RECEIVE_DIRECT / _IMAGE / _IMAGE2 and the directional and order flags");
    if (!(flags & paths)) return bad("nothing to deposit: none of HARE_RECEIVE_DIRECT / _IMAGE / _IMAGE2");
    if (int rc = receive_check_args(who, *s, flags, kind, top_index, 0, 1, n_bins, bin_len, frac_bits)) return rc;      // the order flags, _IMAGE2 without _IMAGE
    if (n_weight < 1 || n_weight > ((int64_t)1 << 53)) return bad("n_weight out of range (1 .. 2^53)");
    if (s->src.set && s->src.B != scene_bands(*s, top_index))
        return bad("the source has " + std::to_string(s->src.B) + " bands, the topology " + std::to_string(scene_bands(*s, top_index)));
    if (!hist || !detections) return bad("null histogram / detections");
    const size_t K1 = std::max<size_t>(1, s->rcv.size() / 4);
    if (spans_overlap({{hist, receive_hist_words(*s, top_index, n_bins, flags, 1) * sizeof(uint64_t)}, {detections, K1 * 2 * sizeof(uint64_t)}}, 2))
        return bad("histogram and detections must not overlap");
    GUARD_BEGIN
    DeviceGuard dev_guard(hip_api(nullptr), s->device);
    const HipApi* H = nullptr;
    std::unique_lock<std::mutex> lk(s->mu);
    if (int rc = ensure_device(*s, H)) return rc;
    if (int rc = source_ready(*s, H, who)) return rc;
    if (int rc = upload_polys(*s, H)) return rc;
    if (int rc = receive_ready(*s, H, who)) return rc;
    const CtxLease lease(*s, lk, [](const Scene::BatchCtx&) { return true; });       // (releases lk)
    Scene::BatchCtx* const c = lease.get();
    const int rc = source_paths_on_scene(*s, H, *c, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, hist, detections);
    if (rc != HARE_OK && c->st[0]) (void)H->StreamSynchronize(c->st[0]);          // copies into the caller's buffers may still be in flight
    return rc;
    GUARD_END
}

// hare_diffract_paths: first-order edge diffraction from host buffers (include/hare_hip.h, "receivers", "Edge diffraction (first order)"),
// built as hare_source_paths is: the histogram and the detections zeroed on a leased context's stream, diffract_enqueue, the three downloads,
// one synchronisation
static int diffract_paths_on_scene(Scene& s, const HipApi* H, Scene::BatchCtx& c, int32_t kind, int32_t top, int64_t n_weight, uint32_t flags,
                                   int32_t n_bins, double bin_len, int32_t frac_bits, double max_detour, int64_t max_pairs, uint64_t* hist,
                                   uint64_t* det, uint64_t* found)
{
    Scene::BounceBuf& b = c.bounce;
    const size_t K = s.rcv.size() / 4;
    const size_t hist_words = receive_hist_words(s, top, n_bins, flags), hist_bytes = (hist_words + 2 * K) * sizeof(uint64_t);
    if (int rc = grow(H, b.hist, b.hist_cap, hist_bytes)) return rc;
    if (int rc = grow(H, b.diffract, b.diffract_cap, (size_t)HARE_DIFFRACT_WORK_BYTES(K, max_pairs))) return rc;
    if (!c.st[0]) HIP_TRY(H->StreamCreate(&c.st[0]));
    hipStream_t st = c.st[0];
    uint64_t* const d_hist = (uint64_t*)b.hist;
    uint64_t* const d_det = d_hist + hist_words;
    HIP_TRY(H->MemsetAsync(b.hist, 0, hist_bytes, st));
    if (int rc = diffract_enqueue(s, H, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, max_detour, max_pairs, b.diffract, d_hist, d_det, st))
        return rc;
    HIP_TRY(H->MemcpyAsync(hist, d_hist, hist_words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(H->MemcpyAsync(det, d_det, 2 * K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    uint64_t pairs = 0;             // the last download, so that no return lies between it and the wait
    HIP_TRY(H->MemcpyAsync(&pairs, b.diffract, sizeof pairs, hipMemcpyDeviceToHost, st));
    HIP_TRY(H->StreamSynchronize(st));
    if (found) *found = pairs;
    if (pairs > (uint64_t)max_pairs) {
        set_error("hare_diffract_paths: the scene yields " + std::to_string(pairs) + " edge-receiver pairs, max_pairs is " + std::to_string(max_pairs) +
                  " (needed: " + std::to_string(pairs) + ")");
        return HARE_E_NOMEM;
    }
    return HARE_OK;
}

extern "C" int hare_diffract_paths(hare_scene* s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                                   int32_t frac_bits, double max_detour, int64_t max_pairs, uint64_t* hist, uint64_t* detections, uint64_t* found)
{
    const char* const who = "hare_diffract_paths";
    if (int rc = diffract_call_check(who, s, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_detour, max_pairs)) return rc;
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (!hist || !detections) return bad("null histogram / detections");
    const size_t K1 = std::max<size_t>(1, s->rcv.size() / 4);
    if (spans_overlap({{hist, receive_hist_words(*s, top_index, n_bins, flags, 1) * sizeof(uint64_t)}, {detections, K1 * 2 * sizeof(uint64_t)}, {found, sizeof(uint64_t)}}, 3))
        return bad("histogram, detections and found must not overlap");
    GUARD_BEGIN
    DeviceGuard dev_guard(hip_api(nullptr), s->device);
    const HipApi* H = nullptr;
    std::unique_lock<std::mutex> lk(s->mu);
    if (int rc = ensure_device(*s, H)) return rc;
    if (int rc = source_ready(*s, H, who)) return rc;
    if (int rc = upload_polys(*s, H)) return rc;
    if (int rc = receive_ready(*s, H, who)) return rc;
    if (int rc = diffract_ready(*s, H, top_index, who)) return rc;
    const CtxLease lease(*s, lk, [](const Scene::BatchCtx&) { return true; });       // (releases lk)
    Scene::BatchCtx* const c = lease.get();
    const int rc = diffract_paths_on_scene(*s, H, *c, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_detour, max_pairs, hist,
                                           detections, found);
    if (rc != HARE_OK && c->st[0]) (void)H->StreamSynchronize(c->st[0]);          // copies into the caller's buffers may still be in flight
    return rc;
    GUARD_END
}

// hare_receive_batch / hare_receive_source with the histogram reduced on the device (include/hare_hip.h, "receivers", "Reduction")
static ReduceSpec reduce_spec(const uint32_t* weight, int32_t n_win, const int32_t* win, int32_t n_lev, const uint32_t* levels)
{
    ReduceSpec r;
    r.weight = weight;
    r.n_win = n_win;
    r.win = win;
    r.n_lev = n_lev;
    r.levels = levels;
    return r;
}

extern "C" {

int hare_receive_batch_reduced(hare_scene* s, int32_t kind, int32_t top_index, int64_t n, const hare_ray* rays, const int32_t* excl1,
                               const int32_t* excl2, int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits,
                               const double* state_in, double* state_out, const uint32_t* weight, int32_t n_win, const int32_t* win,
                               int32_t n_lev, const uint32_t* levels, uint64_t* sums, int32_t* cross, uint64_t* detections, hare_counters* ctr)
{
    hare_scene* const one[1] = {s};
    const ReduceSpec r = reduce_spec(weight, n_win, win, n_lev, levels);
    return receive_sharded("hare_receive_batch_reduced", one, 1, kind, top_index, n, rays, excl1, excl2, bounces, flags, n_bins, bin_len, frac_bits,
                           state_in, state_out, nullptr, detections, ctr, nullptr, &r, sums, cross);
}

int hare_receive_source_reduced(hare_scene* s, int32_t kind, int32_t top_index, int64_t n, int64_t first_ray, int32_t bounces, uint32_t flags,
                                int32_t n_bins, double bin_len, int32_t frac_bits, double* state_out, const uint32_t* weight, int32_t n_win,
                                const int32_t* win, int32_t n_lev, const uint32_t* levels, uint64_t* sums, int32_t* cross, uint64_t* detections,
                                hare_counters* ctr)
{
    hare_scene* const one[1] = {s};
    const ReduceSpec r = reduce_spec(weight, n_win, win, n_lev, levels);
    return receive_sharded("hare_receive_source_reduced", one, 1, kind, top_index, n, nullptr, nullptr, nullptr, bounces, flags, n_bins, bin_len,
                           frac_bits, nullptr, state_out, nullptr, detections, ctr, &first_ray, &r, sums, cross);
}

}  // extern "C"
