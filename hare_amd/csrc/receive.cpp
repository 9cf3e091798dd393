// receive.cpp -- receivers, absorption and scattering of a scene (hare_scene_set_receivers / _absorption / _scattering), the receive loop's plan
// and its per-cast step (receive_plan, receive_step: what bounce_device_impl, launch.cpp, runs between its casts) and hare_receive_device
// (include/hare_hip.h, "receivers"; the kernels: receive.hip); the point source (hare_scene_set_source, hare_emit_device; the kernel:
// source.hip); the direct sound (direct_enqueue, hare_direct_device; the kernels: direct.hip); first-order image sources (image_enqueue,
// hare_image_device; the kernels: image.hip) and second-order ones (image2_enqueue, hare_image2_device; the kernels: image2.hip); first-order edge
// diffraction (hare_scene_set_edges, diffract_enqueue, hare_diffract_device; the kernels: diffract.hip).  The
// plans fill what their kernels share through deposit_fill and image_scene_fill, and the calls check and prepare through
// deposit_call_check, deposit_buffers_check and deposit_call_run.  The host-buffer calls hare_receive_batch / _sharded and
// hare_receive_source / _sharded are in bounce.cpp, beside the loop they share with hare_bounce_batch; what post-processes a histogram
// (hare_hist_reduce, _project, _render) is in hist.cpp.
//
// Harness-defined: the reference has no receivers (Pachyderm, its caller, detects them on the host per ray).
// Product code; nothing from oracle/.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/hare_hip.h"
#include "launch.h"
#include "scene.h"
#include "fan_out.h"

namespace hare {

namespace {

bool device_present(const HipApi*& H)
{
    std::string e;
    H = hip_api(&e);
    int n = 0;
    return H && H->GetDeviceCount(&n) == hipSuccess && n > 0;
}

}  // namespace

// The host copies to the device: the linear loop's fixed-size receiver block (allocated once, never reallocated), a map's three blocks (its
// receivers, cell_start, cell_items: sized by the map, so upload() frees and allocates them again for every hare_scene_set_receiver_map),
// an absorption and a scattering table per topology.  Called by the setters when a device is present -- as a build pushes its partition --
// and by a receive call only for what a setter could not upload: no receive call reallocates anything a setter has uploaded.
// hare_scene_set_receivers behind a map leaves the map's device blocks where they are, unused, until the next map replaces them or
// free_receivers frees them with the scene.
int upload_receivers(Scene& s, const HipApi* H)
{
    if (s.rmap.set && !s.rcv.empty() && !s.rcv_on_device) {      // a map: a block of its own size, and the grid next to it
        Scene::ReceiverMap& m = s.rmap;
        if (int rc = upload(H, &m.d_rcv, s.rcv.data(), s.rcv.size() * sizeof(double))) return rc;
        if (int rc = upload(H, &m.d_start, m.start.data(), m.start.size() * sizeof(uint32_t))) return rc;
        if (int rc = upload(H, &m.d_items, m.items.data(), m.items.size() * sizeof(uint32_t))) return rc;
        s.rcv_on_device = true;
    }
    if (!s.rcv.empty() && !s.rcv_on_device) {
        if (!s.d_rcv) HIP_TRY(H->Malloc(&s.d_rcv, (size_t)kMaxReceivers * 4 * sizeof(double)));
        HIP_TRY(H->Memcpy(s.d_rcv, s.rcv.data(), s.rcv.size() * sizeof(double), hipMemcpyHostToDevice));
        s.rcv_on_device = true;
    }
    for (std::vector<Scene::BandTable>* tables : {&s.alpha, &s.sigma})
        for (Scene::BandTable& t : *tables) {
            if (t.host.empty() || t.on_device) continue;
            if (int rc = upload(H, &t.dev, t.host.data(), t.host.size() * sizeof(double))) return rc;
            t.on_device = true;
        }
    return HARE_OK;
}

void free_receivers(const HipApi* H, Scene& s)
{
    dev_free(H, s.d_rcv);
    dev_free(H, s.rmap.d_rcv);
    dev_free(H, s.rmap.d_start);
    dev_free(H, s.rmap.d_items);
    dev_free(H, s.src.d_gain);
    for (Scene::EdgeTable& t : s.edges) {
        dev_free(H, t.d_ends);
        dev_free(H, t.d_faces);
    }
    for (std::vector<Scene::BandTable>* tables : {&s.alpha, &s.sigma})
        for (Scene::BandTable& t : *tables) dev_free(H, t.dev);
}

static bool has_table(const std::vector<Scene::BandTable>& tables, int32_t top)
{
    return top >= 0 && (size_t)top < tables.size() && !tables[(size_t)top].host.empty();
}

bool scene_has_scattering(const Scene& s, int32_t top)
{
    return has_table(s.sigma, top);
}

bool receive_rains(const Scene& s, int32_t top, uint32_t flags)
{
    return (flags & HARE_RECEIVE_DIFFUSE_RAIN) && scene_has_scattering(s, top);
}

int32_t scene_bands(const Scene& s, int32_t top)
{
    return (top >= 0 && (size_t)top < s.bands.size() && s.bands[(size_t)top] > 0) ? s.bands[(size_t)top] : 1;
}

size_t receive_hist_words(const Scene& s, int32_t top, int32_t n_bins, uint32_t flags, size_t min_K)
{
    const size_t K = std::max<size_t>(min_K, s.rcv.size() / 4);
    return K * (size_t)n_bins * (size_t)scene_bands(s, top) * (size_t)receive_channels(flags);
}

int receive_check_order(const char* who, uint32_t flags)
{
    const uint32_t order = flags & (HARE_RECEIVE_ORDER2 | HARE_RECEIVE_ORDER3);
    if (order && (!(flags & HARE_RECEIVE_DIRECTIONAL) || order == (HARE_RECEIVE_ORDER2 | HARE_RECEIVE_ORDER3))) {
        set_error(std::string(who) + ": HARE_RECEIVE_ORDER2 / HARE_RECEIVE_ORDER3 are accepted only together with HARE_RECEIVE_DIRECTIONAL, and one of them at most");
        return HARE_E_INVALID;
    }
    return HARE_OK;
}

// Everything a receive call checks before anything runs (HARE_E_INVALID); "no receivers" is HARE_E_STATE, after the device checks
int receive_check_args(const char* who, const Scene& s, uint32_t flags, int32_t kind, int32_t top, int64_t n, int32_t bounces, int32_t n_bins, double bin_len,
                       int32_t frac_bits)
{
    auto bad = [&](const char* what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (int rc = receive_check_order(who, flags)) return rc;
    if ((flags & HARE_RECEIVE_IMAGE2) && !(flags & HARE_RECEIVE_IMAGE))
        return bad("HARE_RECEIVE_IMAGE2 is accepted only together with HARE_RECEIVE_IMAGE (the second order stands on the first)");
    if (kind < HARE_KIND_VOXEL || kind > HARE_KIND_KDTREE) return bad("bad kind");
    if (top < 0 || top >= (int32_t)s.topos.size()) return bad("bad top_index");
    if (n < 0 || n > 0x7FFFFF00ll) return bad("n out of range (0 .. 2^31 - 256)");
    if (bounces < 1 || bounces > 4096) return bad("bounces out of range (1 .. 4096)");
    if (n_bins < 1) return bad("n_bins must be >= 1");
    if (!(std::isfinite(bin_len) && bin_len > 0)) return bad("bin_len must be finite and > 0");
    if (frac_bits < 0 || frac_bits > 62) return bad("frac_bits out of range (0 .. 62)");
    if (receive_hist_words(s, top, n_bins, 0, 1) > ((size_t)1 << 27)) return bad("receivers x n_bins x bands exceeds 2^27");
    if (receive_hist_words(s, top, n_bins, flags, 1) > ((size_t)1 << 27))
        return bad(flags & HARE_RECEIVE_ORDER3   ? "receivers x n_bins x bands x 16 channels (HARE_RECEIVE_ORDER3) exceeds 2^27"
                   : flags & HARE_RECEIVE_ORDER2 ? "receivers x n_bins x bands x 9 channels (HARE_RECEIVE_ORDER2) exceeds 2^27"
                                                 : "receivers x n_bins x bands x 4 channels (HARE_RECEIVE_DIRECTIONAL) exceeds 2^27");
    if (s.rmap.set && receive_rains(s, top, flags))
        return bad("HARE_RECEIVE_DIFFUSE_RAIN does not combine with a receiver map (hare_scene_set_receiver_map)");
    return HARE_OK;
}

// The rain's scratch in a receive call's work array: behind the loop's 2 n int32, from a 16-byte boundary: n shadow rays (48 B), n t_max,
// n exclusions, n occlusion flags, n suppression flags: 76 n bytes in all and at most 15 of padding, within HARE_RECEIVE_RAIN_WORK_BYTES(n)
static RainWork rain_work(void* d_work, int64_t n)
{
    RainWork w;
    w.rays = (RayRec*)(((uintptr_t)d_work + (uintptr_t)n * 8u + 15u) & ~(uintptr_t)15u);
    w.tmax = (double*)(w.rays + n);
    w.excl = (int32_t*)(w.tmax + n);
    w.occ = w.excl + n;
    w.flag = w.occ + n;
    return w;
}

int receive_plan(const Scene& s, int32_t top, uint32_t flags, int64_t n, int32_t n_bins, double bin_len, int32_t frac_bits, void* d_state,
                 void* d_hist, void* d_det, void* d_work, bool init_state, int64_t ray_base, ReceivePlan& p)
{
    ReceiveMapArgs& ra = p.args;
    memset((void*)&ra, 0, sizeof ra);
    ra.state = (double*)d_state;
    ra.alpha = has_table(s.alpha, top) ? (const double*)s.alpha[(size_t)top].dev : nullptr;
    ra.rcv = (const double*)(s.rmap.set ? s.rmap.d_rcv : s.d_rcv);
    ra.hist = (unsigned long long*)d_hist;
    ra.det = (unsigned long long*)d_det;
    ra.bin_len = bin_len;
    ra.scale = ldexp(1.0, frac_bits);
    ra.bands = scene_bands(s, top);
    ra.n_rcv = (int32_t)(s.rcv.size() / 4);
    ra.n_bins = n_bins;
    ra.aggregate = s.opt.receive_aggregate;
    ra.init_state = init_state ? 1 : 0;
    ra.sigma = has_table(s.sigma, top) ? (const double*)s.sigma[(size_t)top].dev : nullptr;
    ra.seed = (unsigned long long)s.opt.scatter_seed;
    ra.ray_base = (long long)ray_base;
    if (ra.sigma == nullptr && has_table(s.sigma, top)) {
        set_error("receive: scattering table not on the device");
        return HARE_E_STATE;
    }
    if (ra.alpha == nullptr && has_table(s.alpha, top)) {
        set_error("receive: absorption table not on the device");
        return HARE_E_STATE;
    }
    // termination (the header's "Termination"): the flag and the two scene options, as the kernels' one field
    ra.cut = ((flags & HARE_RECEIVE_TIME_LIMIT) ? kCutTime : 0) |
             (s.opt.receive_floor_bits > 0 ? (kCutFloor | (s.opt.receive_roulette ? kCutRoulette : 0)) : 0);
    ra.floor = ldexp(1.0, -s.opt.receive_floor_bits);
    p.map = s.rmap.set;
    if (p.map) {
        const Scene::ReceiverMap& m = s.rmap;
        if (!m.d_rcv || !m.d_start || !m.d_items) {
            set_error("receive: receiver map not on the device");
            return HARE_E_STATE;
        }
        ra.map_start = (const uint32_t*)m.d_start;
        ra.map_items = (const uint32_t*)m.d_items;
        for (int k = 0; k < 3; ++k) {
            ra.map_n[k] = m.n[k];
            ra.map_org[k] = m.org[k];
        }
        ra.map_h = m.h;
        ra.map_pad = m.pad;
    }
    p.directional = receive_channel_form(flags);
    p.rain = receive_rains(s, top, flags);
    p.work = p.rain ? rain_work(d_work, n) : RainWork();
    ra.rain_flag = p.work.flag;
    p.skip_cast0 = (flags & HARE_RECEIVE_DIRECT) != 0;
    p.skip_cast1_specular = (flags & HARE_RECEIVE_IMAGE) != 0;
    p.skip_cast2_specular = (flags & HARE_RECEIVE_IMAGE2) != 0;
    // the byte per ray of casts 1 and 2 (a scattering table only): behind everything else the work array holds -- the loop's 2 n int32, or
    // HARE_RECEIVE_RAIN_WORK_BYTES(n) in a call with HARE_RECEIVE_DIFFUSE_RAIN.  Null in every call without the flag
    if (p.skip_cast2_specular && ra.sigma)
        ra.spec2 = (unsigned char*)d_work + ((flags & HARE_RECEIVE_DIFFUSE_RAIN) ? (size_t)HARE_RECEIVE_RAIN_WORK_BYTES(n) : (size_t)n * 2 * sizeof(int32_t));
    return HARE_OK;
}

// hare_rain_step reads what the receive kernel of the same cast reads, before that kernel overwrites rays and state
static RainArgs rain_args(const ReceiveArgs& ra, const RainWork& w)
{
    RainArgs g;
    memset(&g, 0, sizeof g);
    g.polys = ra.polys;
    g.rays = ra.rays;
    g.ev = ra.ev;
    g.marks = ra.excl;
    g.state = ra.state;
    g.alpha = ra.alpha;
    g.sigma = ra.sigma;
    g.rcv = ra.rcv;
    g.hist = ra.hist;
    g.det = ra.det;
    g.srays = w.rays;
    g.stmax = w.tmax;
    g.sexcl = w.excl;
    g.socc = w.occ;
    g.n = ra.n;
    g.bin_len = ra.bin_len;
    g.scale = ra.scale;
    g.bands = ra.bands;
    g.n_bins = ra.n_bins;
    g.marks_valid = ra.marks_valid;
    g.init_state = ra.init_state;
    return g;
}

// The receiver step, the state update and (but behind the last cast) the reflection: hare_receive_reflect in hare_reflect's place,
// hare_receive_scatter where Model[top] has a scattering table, hare_receive_scatter_rain behind the rain
int receive_step(Scene& s, const HipApi* H, int32_t kind, int32_t top, int64_t n, const ReceivePlan& p, void* d_rays, void* d_ev,
                 int32_t* marks, unsigned char* block_live, int32_t cast, bool last_cast, hipStream_t st)
{
    const DeviceModule& M = *s.module;
    const unsigned grid = (unsigned)((n + 255) / 256);
    ReceiveMapArgs ra = p.args;                             // the kernels without a map read its ReceiveArgs, which lies in front
    ra.polys = (const PolyRec*)s.d_polys[(size_t)top];
    ra.rays = (RayRec*)d_rays;
    ra.ev = (XEventRec*)d_ev;
    ra.excl = marks;
    ra.block_live = block_live;
    ra.n = n;
    ra.marks_valid = cast > 0 ? 1 : 0;
    ra.last = last_cast ? 1 : 0;
    ra.init_state = cast == 0 ? p.args.init_state : 0;      // the starting state is the first cast's business only
    ra.cast = cast;
    if (p.skip_cast0 && cast == 0) ra.cut |= kCutSkipDetect;      // the direct sound is hare_direct_deposit's: calls without the flag pass today's bytes
    // the first-order specular paths are hare_image_deposit's: without a scattering table every ray of cast 1 has left cast 0 specularly; with
    // one, the scatter kernels recompute each ray's choice
    if (p.skip_cast1_specular && cast == 1) ra.cut |= ra.sigma ? kCutSkipSpecular : kCutSkipDetect;
    // the second-order specular paths are hare_image2_deposit's: without a table every ray of cast 2 was reflected specularly twice; with one,
    // cast 1 stores each reflected ray's conjunction (its recomputed outcome of cast 0 and its own draw) and cast 2 reads it
    if (p.skip_cast2_specular && cast == 1 && ra.sigma && !last_cast) ra.cut |= kCutStoreSpecular2;
    if (p.skip_cast2_specular && cast == 2) ra.cut |= ra.sigma ? kCutSkipSpecular2 : kCutSkipDetect;
    if (p.rain && !last_cast) {
        // diffuse rain (receive.hip: hare_rain_step): receiver k's query is emitted, answered by the flags-only occlusion kernel of this
        // partition, and deposited by the launch that emits k + 1's
        RainArgs g = rain_args(ra, p.work);
        for (int32_t k = 0; k <= ra.n_rcv; ++k) {
            g.k_dep = k - 1;
            g.k_emit = k < ra.n_rcv ? k : -1;
            void* ga[] = {&g};
            if (int rc = launch(H, M.rain_step[p.directional], grid, 256, 0, st, ga)) return rc;
            if (k == ra.n_rcv) break;
            if (int rc = shoot_device_impl(s, H, kind, top, n, p.work.rays, p.work.excl, nullptr, HARE_SHOOT_RETIRED_RAYS, nullptr, nullptr, st,
                                           p.work.tmax, p.work.occ))
                return rc;
        }
    }
    void* a[] = {&ra};
    return launch(H, M.receive[receive_form(p)][p.directional], grid, 256, 0, st, a);
}

// After the device checks: receivers set, and on the device (uploads only what a setter run without a device left behind)
int receive_ready(Scene& s, const HipApi* H, const char* who)
{
    if (s.rcv.empty()) {
        set_error(std::string(who) + ": no receivers set (hare_scene_set_receivers)");
        return HARE_E_STATE;
    }
    return upload_receivers(s, H);
}

// ---- the point source (include/hare_hip.h, "receivers", "Source")
bool Scene::Source::same_as(const Source& o) const
{
    return set == o.set && B == o.B && R == o.R && memcmp(pos, o.pos, sizeof pos) == 0 && memcmp(power, o.power, sizeof power) == 0 &&
           memcmp(frame, o.frame, sizeof frame) == 0 && gain == o.gain;
}

int source_check_range(const char* who, int64_t n, int64_t first_ray)
{
    if (first_ray < 0 || n < 0 || first_ray > ((int64_t)1 << 62) - n) {
        set_error(std::string(who) + ": first_ray out of range (first_ray >= 0, first_ray + n <= 2^62)");
        return HARE_E_INVALID;
    }
    return HARE_OK;
}

static int upload_source(Scene& s, const HipApi* H)
{
    Scene::Source& src = s.src;
    if (!src.set || src.gain.empty() || src.on_device) return HARE_OK;
    if (int rc = upload(H, &src.d_gain, src.gain.data(), src.gain.size() * sizeof(double))) return rc;
    src.on_device = true;
    return HARE_OK;
}

// After the device checks: a source set, and its table on the device (uploads only what a setter run without a device left behind)
int source_ready(Scene& s, const HipApi* H, const char* who)
{
    if (!s.src.set) {
        set_error(std::string(who) + ": no source set (hare_scene_set_source)");
        return HARE_E_STATE;
    }
    return upload_source(s, H);
}

int emit_source(const Scene& s, const HipApi* H, int64_t n, int64_t first_ray, void* d_rays, void* d_state, hipStream_t st)
{
    const Scene::Source& src = s.src;
    if (!s.module || !s.module->emit_source) {
        set_error("hare_emit_source missing from code object");
        return HARE_E_STATE;
    }
    if (n == 0) return HARE_OK;
    SourceArgs a;
    memset(&a, 0, sizeof a);
    a.rays = (RayRec*)d_rays;
    a.state = (double*)d_state;
    a.gain = src.R > 0 ? (const double*)src.d_gain : nullptr;
    a.n = n;
    a.first_ray = first_ray;
    a.seed = (unsigned long long)s.opt.source_seed;
    memcpy(a.pos, src.pos, sizeof a.pos);
    memcpy(a.power, src.power, sizeof a.power);
    memcpy(a.frame, src.frame, sizeof a.frame);
    a.bands = src.B;
    a.res = src.R;
    if (src.R > 0 && !a.gain) {
        set_error("source: directivity table not on the device");
        return HARE_E_STATE;
    }
    void* args[] = {&a};
    return launch(H, s.module->emit_source, (unsigned)((n + 255) / 256), 256, 0, st, args);
}

// ---- the deterministic source paths: what their three plans share
// The fields every deposit reads (DepositArgs), but for the four shadow-ray arrays, which each plan carves from its own scratch.  False:
// receivers or directivity table not on the device
static bool deposit_fill(DepositArgs& d, const Scene& s, int64_t n_weight, int32_t n_bins, double bin_len, int32_t frac_bits, void* d_hist, void* d_det)
{
    const Scene::Source& src = s.src;
    d.rcv = (const double*)(s.rmap.set ? s.rmap.d_rcv : s.d_rcv);
    d.gain = src.R > 0 ? (const double*)src.d_gain : nullptr;
    d.hist = (unsigned long long*)d_hist;
    d.det = (unsigned long long*)d_det;
    memcpy(d.pos, src.pos, sizeof d.pos);
    memcpy(d.power, src.power, sizeof d.power);
    memcpy(d.frame, src.frame, sizeof d.frame);
    d.bin_len = bin_len;
    d.scale = ldexp(1.0, frac_bits);
    d.weight = (double)n_weight;
    d.n_rcv = (int32_t)(s.rcv.size() / 4);
    d.bands = src.B;
    d.res = src.R;
    d.n_bins = n_bins;
    return d.rcv && (src.R == 0 || d.gain);
}

// The topology as the image-source kernels read it (ImageScene), and the image sources' one "not on the device" for it and for what
// deposit_fill found
static int image_scene_fill(ImageScene& sc, const Scene& s, int32_t top, bool deposit_on_device)
{
    sc.polys = (const PolyRec*)s.d_polys[(size_t)top];
    sc.quads = (const QuadRec*)s.d_quads[(size_t)top];
    sc.cull = (const unsigned char*)s.d_cull[(size_t)top];
    sc.alpha = has_table(s.alpha, top) ? (const double*)s.alpha[(size_t)top].dev : nullptr;
    sc.sigma = has_table(s.sigma, top) ? (const double*)s.sigma[(size_t)top].dev : nullptr;
    sc.cf = s.cull_frames[(size_t)top];
    sc.n_poly = (int32_t)s.topos[(size_t)top].P;
    if (!deposit_on_device || !sc.polys || !sc.cull || (has_table(s.alpha, top) && !sc.alpha) || (has_table(s.sigma, top) && !sc.sigma)) {
        set_error("image sources: polygons, receivers or tables not on the device");
        return HARE_E_STATE;
    }
    return HARE_OK;
}

// ---- the direct sound (include/hare_hip.h, "receivers", "Direct sound"; the kernels: direct.hip)
// The scratch of a deposit: K shadow rays (48 B) from a 16-byte boundary, K t_max, K exclusion words, K occlusion flags: 64 K bytes and at
// most 15 of padding, within HARE_DIRECT_WORK_BYTES(K)
int direct_enqueue(Scene& s, const HipApi* H, int32_t kind, int32_t top, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                   int32_t frac_bits, void* d_work, void* d_hist, void* d_det, hipStream_t st)
{
    const int dir = receive_channel_form(flags);
    if (!s.module || !s.module->direct_emit || !s.module->direct_deposit[dir]) {
        set_error("hare_direct_emit / hare_direct_deposit missing from code object");
        return HARE_E_STATE;
    }
    const int64_t K = (int64_t)(s.rcv.size() / 4);
    DirectArgs a;
    memset(&a, 0, sizeof a);
    DepositArgs& d = a.d;
    d.srays = (RayRec*)(((uintptr_t)d_work + 15u) & ~(uintptr_t)15u);
    d.stmax = (double*)(d.srays + K);
    d.sexcl = (int32_t*)(d.stmax + K);
    int32_t* const occ = d.sexcl + K;
    d.socc = occ;
    if (!deposit_fill(d, s, n_weight, n_bins, bin_len, frac_bits, d_hist, d_det)) {
        set_error("direct sound: receivers or directivity table not on the device");
        return HARE_E_STATE;
    }
    const unsigned grid = (unsigned)((K + 255) / 256);
    void* args[] = {&a};
    if (int rc = launch(H, s.module->direct_emit, grid, 256, 0, st, args)) return rc;
    if (int rc = shoot_device_impl(s, H, kind, top, K, d.srays, d.sexcl, nullptr, HARE_SHOOT_RETIRED_RAYS, nullptr, nullptr, st, d.stmax, occ)) return rc;
    return launch(H, s.module->direct_deposit[dir], grid, 256, 0, st, args);
}

// ---- first-order image sources (include/hare_hip.h, "receivers", "Image sources (first order)"; the kernels: image.hip)
// The scratch of a deposit, from d_work (a 16-byte boundary): 256 bytes whose first word is the pair count; P images (32 B); then per list
// slot two shadow rays (96 B), two t_max (16 B), the pair's k and p (8 B), two exclusion words (8 B), two occlusion flags (8 B):
// 256 + 32 P + 136 max_pairs = HARE_IMAGE_WORK_BYTES
int image_enqueue(Scene& s, const HipApi* H, int32_t kind, int32_t top, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                  int32_t frac_bits, int64_t max_pairs, void* d_work, void* d_hist, void* d_det, hipStream_t st)
{
    const int dir = receive_channel_form(flags);
    if (!s.module || !s.module->image_mirror || !s.module->image_pairs || !s.module->image_deposit[dir]) {
        set_error("hare_image_mirror / hare_image_pairs / hare_image_deposit missing from code object");
        return HARE_E_STATE;
    }
    const int64_t K = (int64_t)(s.rcv.size() / 4), P = s.topos[(size_t)top].P, M = max_pairs;
    ImageArgs a;
    memset((void*)&a, 0, sizeof a);
    DepositArgs& d = a.d;
    char* const w = (char*)d_work;
    a.count = (unsigned long long*)w;
    a.img = (double*)(w + 256);
    d.srays = (RayRec*)(a.img + 4 * P);
    d.stmax = (double*)(d.srays + 2 * M);
    a.pair_kp = (int32_t*)(d.stmax + 2 * M);
    d.sexcl = a.pair_kp + 2 * M;
    int32_t* const occ = d.sexcl + 2 * M;
    d.socc = occ;
    a.max_pairs = M;
    a.use_cull = s.opt.image_cull;
    if (int rc = image_scene_fill(a.sc, s, top, deposit_fill(d, s, n_weight, n_bins, bin_len, frac_bits, d_hist, d_det))) return rc;
    if (P == 0) return HARE_OK;     // no polygon, no image (a topology is never empty today: hare_scene_create refuses P < 1)
    void* args[] = {&a};
    const int64_t fill = std::max<int64_t>(P, 2 * M);
    if (int rc = launch(H, s.module->image_mirror, (unsigned)std::min<int64_t>((fill + 255) / 256, 4096), 256, 0, st, args)) return rc;
    {
        // hare_image_pairs: (polygon blocks) x (receiver tiles of 256), through the module API like the rest
        const unsigned gx = (unsigned)((P + 255) / 256), gy = (unsigned)((K + 255) / 256);
        HIP_TRY(H->ModuleLaunchKernel(s.module->image_pairs, gx, gy, 1, 256, 1, 1, 0, st, args, nullptr));
    }
    if (int rc = shoot_device_impl(s, H, kind, top, 2 * M, d.srays, d.sexcl, nullptr, HARE_SHOOT_RETIRED_RAYS, nullptr, nullptr, st, d.stmax, occ)) return rc;
    return launch(H, s.module->image_deposit[dir], (unsigned)((M + 255) / 256), 256, 0, st, args);
}

// ---- second-order image sources (include/hare_hip.h, "receivers", "Image sources (second order)"; the kernels: image2.hip)
// The scratch of a deposit, from d_work (a 16-byte boundary): 256 bytes whose first two words are the candidate count and the path count;
// P images (32 B); per candidate S'' (24 B) and p, q (8 B); per path three shadow rays (144 B), three t_max (24 B), k and the candidate's
// index (8 B), three poly_origin1, three poly_origin2 and three occlusion flags (36 B):
// 256 + 32 P + 32 max_cands + 212 max_paths = HARE_IMAGE2_WORK_BYTES
int image2_enqueue(Scene& s, const HipApi* H, int32_t kind, int32_t top, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                   int32_t frac_bits, int64_t max_cands, int64_t max_paths, void* d_work, void* d_hist, void* d_det, hipStream_t st)
{
    const int dir = receive_channel_form(flags);
    const DeviceModule* const m = s.module;
    if (!m || !m->image2_mirror || !m->image2_cands || !m->image2_paths || !m->image2_deposit[dir]) {
        set_error("hare_image2_mirror / hare_image2_cands / hare_image2_paths / hare_image2_deposit missing from code object");
        return HARE_E_STATE;
    }
    const int64_t K = (int64_t)(s.rcv.size() / 4), P = s.topos[(size_t)top].P, C = max_cands, M = max_paths;
    Image2Args a;
    memset((void*)&a, 0, sizeof a);
    DepositArgs& d = a.d;
    char* const w = (char*)d_work;
    a.count = (unsigned long long*)w;
    a.img = (double*)(w + 256);
    a.cand_s = a.img + 4 * P;
    a.cand_pq = (int32_t*)(a.cand_s + 3 * C);
    d.srays = (RayRec*)(a.cand_pq + 2 * C);
    d.stmax = (double*)(d.srays + 3 * M);
    a.path_kc = (int32_t*)(d.stmax + 3 * M);
    d.sexcl = a.path_kc + 2 * M;
    a.sexcl2 = d.sexcl + 3 * M;
    int32_t* const occ = a.sexcl2 + 3 * M;
    d.socc = occ;
    a.max_cands = C;
    a.max_paths = M;
    a.prune = s.opt.image2_prune;
    if (int rc = image_scene_fill(a.sc, s, top, deposit_fill(d, s, n_weight, n_bins, bin_len, frac_bits, d_hist, d_det))) return rc;
    if (P == 0) return HARE_OK;
    void* args[] = {&a};
    const int64_t fill = std::max<int64_t>(P, 3 * M);
    if (int rc = launch(H, m->image2_mirror, (unsigned)std::min<int64_t>((fill + 255) / 256, 4096), 256, 0, st, args)) return rc;
    {
        // hare_image2_cands: (p blocks) x (q tiles of 256); hare_image2_paths: (candidate blocks) x (receiver tiles of 256).  A grid's
        // second dimension holds at most 65 535 blocks: K <= 65 536 receivers are 256 tiles; P is refused beyond 65 535 * 256 polygons
        if (P > 65535ll * 256) {
            set_error("image sources (second order): more than 16 776 960 polygons");
            return HARE_E_INVALID;
        }
        const unsigned gp = (unsigned)((P + 255) / 256);
        HIP_TRY(H->ModuleLaunchKernel(m->image2_cands, gp, gp, 1, 256, 1, 1, 0, st, args, nullptr));
        HIP_TRY(H->ModuleLaunchKernel(m->image2_paths, (unsigned)((C + 255) / 256), (unsigned)((K + 255) / 256), 1, 256, 1, 1, 0, st, args, nullptr));
    }
    if (int rc = shoot_device_impl(s, H, kind, top, 3 * M, d.srays, d.sexcl, a.sexcl2, HARE_SHOOT_RETIRED_RAYS, nullptr, nullptr, st, d.stmax, occ)) return rc;
    return launch(H, m->image2_deposit[dir], (unsigned)((M + 255) / 256), 256, 0, st, args);
}

// ---- first-order edge diffraction (include/hare_hip.h, "receivers", "Edge diffraction (first order)"; the kernels: diffract.hip)
int64_t scene_edges(const Scene& s, int32_t top)
{
    return (top >= 0 && (size_t)top < s.edges.size()) ? (int64_t)(s.edges[(size_t)top].ends.size() / 6) : 0;
}

static int upload_edges(Scene::EdgeTable& t, const HipApi* H)
{
    if (t.ends.empty() || t.on_device) return HARE_OK;
    if (int rc = upload(H, &t.d_ends, t.ends.data(), t.ends.size() * sizeof(double))) return rc;
    if (int rc = upload(H, &t.d_faces, t.faces.data(), t.faces.size() * sizeof(int32_t))) return rc;
    t.on_device = true;
    return HARE_OK;
}

// After the device checks: an edge table set for the topology, and on the device (uploads only what a setter run without a device left behind)
int diffract_ready(Scene& s, const HipApi* H, int32_t top, const char* who)
{
    if (scene_edges(s, top) == 0) {
        set_error(std::string(who) + ": no edges set (hare_scene_set_edges)");
        return HARE_E_STATE;
    }
    return upload_edges(s.edges[(size_t)top], H);
}

// The scratch of a deposit, from d_work (a 16-byte boundary): 256 bytes whose first word is the pair count; then ONE run of K + 2 max_pairs
// shadow slots, array by array -- the rays (48 B), t_max (8 B), poly_origin1, poly_origin2 and the occlusion flags (4 B each): 68 bytes a
// slot -- and the pairs' k and j (8 B): 256 + 68 K + 144 max_pairs = HARE_DIFFRACT_WORK_BYTES
int diffract_enqueue(Scene& s, const HipApi* H, int32_t kind, int32_t top, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                     int32_t frac_bits, double max_detour, int64_t max_pairs, void* d_work, void* d_hist, void* d_det, hipStream_t st)
{
    const int dir = receive_channel_form(flags);
    const DeviceModule* const m = s.module;
    if (!m || !m->diffract_emit || !m->diffract_pairs || !m->diffract_deposit[dir]) {
        set_error("hare_diffract_emit / hare_diffract_pairs / hare_diffract_deposit missing from code object");
        return HARE_E_STATE;
    }
    const Scene::EdgeTable& t = s.edges[(size_t)top];
    const int64_t K = (int64_t)(s.rcv.size() / 4), E = scene_edges(s, top), M = max_pairs, S = K + 2 * M;
    DiffractArgs a;
    memset((void*)&a, 0, sizeof a);
    DepositArgs& d = a.d;
    char* const w = (char*)d_work;
    a.count = (unsigned long long*)w;
    d.srays = (RayRec*)(w + 256);
    d.stmax = (double*)(d.srays + S);
    d.sexcl = (int32_t*)(d.stmax + S);
    a.sexcl2 = d.sexcl + S;
    int32_t* const occ = a.sexcl2 + S;
    d.socc = occ;
    a.pair_kj = occ + S;
    a.ends = (const double*)t.d_ends;
    a.faces = (const int32_t*)t.d_faces;
    a.max_pairs = M;
    a.max_detour = max_detour;
    memcpy(a.inv_lambda, t.inv_lambda, sizeof a.inv_lambda);
    a.n_edges = (int32_t)E;
    if (!deposit_fill(d, s, n_weight, n_bins, bin_len, frac_bits, d_hist, d_det) || !a.ends || !a.faces) {
        set_error("edge diffraction: receivers, edges or directivity table not on the device");
        return HARE_E_STATE;
    }
    void* args[] = {&a};
    if (int rc = launch(H, m->diffract_emit, (unsigned)std::min<int64_t>((S + 255) / 256, 4096), 256, 0, st, args)) return rc;
    {
        // hare_diffract_pairs: (edge blocks) x (receiver tiles of 256): E <= 2^20 edges are 4 096 blocks, K <= 65 536 receivers 256 tiles
        const unsigned gx = (unsigned)((E + 255) / 256), gy = (unsigned)((K + 255) / 256);
        HIP_TRY(H->ModuleLaunchKernel(m->diffract_pairs, gx, gy, 1, 256, 1, 1, 0, st, args, nullptr));
    }
    if (int rc = shoot_device_impl(s, H, kind, top, S, d.srays, d.sexcl, a.sexcl2, HARE_SHOOT_RETIRED_RAYS, nullptr, nullptr, st, d.stmax, occ)) return rc;
    return launch(H, m->diffract_deposit[dir], (unsigned)((M + 255) / 256), 256, 0, st, args);
}

// hare_scene_set_absorption / _scattering behind their own checks of top_index and B: P x B coefficients in [0, 1] become Model[top]'s
// table `mine` (`name` in the messages), with the B of the topology's other table where it has one
static int set_band_table(Scene& s, const char* who, const char* name, std::vector<Scene::BandTable>& mine, const std::vector<Scene::BandTable>& other,
                   const char* other_name, int32_t top, int32_t B, const double* v)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    const size_t cnt = (size_t)s.topos[(size_t)top].P * (size_t)B;
    if (cnt > 0 && !v) return bad(std::string("null ") + name);
    for (size_t k = 0; k < cnt; ++k)
        if (!(v[k] >= 0.0 && v[k] <= 1.0)) return bad(std::string(name) + "[" + std::to_string(k) + "] outside [0, 1]");
    if (has_table(other, top) && B != scene_bands(s, top))
        return bad(std::string("B differs from the topology's ") + other_name + " table (" + std::to_string(scene_bands(s, top)) + " bands)");
    mine.resize(s.topos.size());
    s.bands.resize(s.topos.size(), 1);
    std::vector<double> t(v, v + cnt);
    if (t.empty()) t.assign((size_t)B, 0.0);       // a topology without polygons: a table of one row no ray reads
    mine[(size_t)top].host.swap(t);
    mine[(size_t)top].on_device = false;
    s.bands[(size_t)top] = B;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;
    DeviceGuard dev_guard(H, s.device);
    if (int rc = ensure_device(s, H)) return rc;
    return upload_receivers(s, H);
}

// what both receiver setters check, and the K x 4 block (cx, cy, cz, r * r) they keep
static int check_receivers(const char* who, int32_t K, int32_t K_max, const double* centers, const double* radii)
{
    if (K < 1 || K > K_max || !centers || !radii) {
        set_error(std::string(who) + ": need 1 .. " + std::to_string(K_max) + " receivers, centers and radii");
        return HARE_E_INVALID;
    }
    for (int32_t k = 0; k < K; ++k) {
        if (!std::isfinite(centers[3 * k]) || !std::isfinite(centers[3 * k + 1]) || !std::isfinite(centers[3 * k + 2])) {
            set_error(std::string(who) + ": receiver " + std::to_string(k) + " has a non-finite center");
            return HARE_E_INVALID;
        }
        if (!(std::isfinite(radii[k]) && radii[k] > 0)) {
            set_error(std::string(who) + ": receiver " + std::to_string(k) + " needs a finite radius > 0");
            return HARE_E_INVALID;
        }
    }
    return HARE_OK;
}

static std::vector<double> receiver_block(int32_t K, const double* centers, const double* radii)
{
    std::vector<double> r((size_t)K * 4);
    for (int32_t k = 0; k < K; ++k) {
        r[4 * (size_t)k + 0] = centers[3 * k];
        r[4 * (size_t)k + 1] = centers[3 * k + 1];
        r[4 * (size_t)k + 2] = centers[3 * k + 2];
        r[4 * (size_t)k + 3] = radii[k] * radii[k];
    }
    return r;
}

// the receivers are replaced (host copies): up they go when a device is present
static int push_receivers(hare_scene* s)
{
    s->rcv_on_device = false;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;          // GPU-less: the host copy goes up with the first receive call
    DeviceGuard dev_guard(H, s->device);
    if (int rc = ensure_device(*s, H)) return rc;
    if (!s->rmap.set) {                              // back to the linear loop: the map's device copies go
        dev_free(H, s->rmap.d_rcv);
        dev_free(H, s->rmap.d_start);
        dev_free(H, s->rmap.d_items);
    }
    return upload_receivers(*s, H);
}

// The grid of a receiver map (include/hare_hip.h, "Receiver maps"): FP64, no contraction, in the header's order
static void build_receiver_map(Scene::ReceiverMap& m, int32_t K, const double* centers, const double* radii, double cell)
{
    double r_max = radii[0], lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = centers[a];
    for (int32_t k = 1; k < K; ++k) {
        r_max = radii[k] > r_max ? radii[k] : r_max;
        for (int a = 0; a < 3; ++a) {
            const double c = centers[3 * k + a];
            lo[a] = c < lo[a] ? c : lo[a];
            hi[a] = c > hi[a] ? c : hi[a];
        }
    }
    double h = cell > 0 ? cell : 2.0 * r_max;
    int64_t n[3];
    for (;;) {
        for (int a = 0; a < 3; ++a) {
            const double q = (hi[a] - lo[a]) / h;
            n[a] = (q >= 0 && q < (double)kMaxMapCells) ? (int64_t)floor(q) + 1 : (q != q ? 1 : (int64_t)kMaxMapCells + 1);
        }
        if (n[0] <= kMaxMapCells && n[1] <= kMaxMapCells && n[0] * n[1] <= kMaxMapCells && n[0] * n[1] * n[2] <= kMaxMapCells) break;
        h = h * 2.0;
    }
    m.h = h;
    m.R = r_max + h / 8.0;
    m.pad = m.R / h;
    for (int a = 0; a < 3; ++a) {
        m.org[a] = lo[a];
        m.n[a] = (int32_t)n[a];
    }
    const size_t cells = (size_t)(n[0] * n[1] * n[2]);
    std::vector<uint32_t> cell_of((size_t)K);
    m.start.assign(cells + 1, 0);
    for (int32_t k = 0; k < K; ++k) {
        int64_t i[3];
        for (int a = 0; a < 3; ++a) {
            const double u = (centers[3 * k + a] - lo[a]) / h;
            i[a] = u >= 0 ? (u < (double)n[a] ? (int64_t)floor(u) : n[a] - 1) : 0;      // clamped as a double; NaN -> 0
        }
        cell_of[(size_t)k] = (uint32_t)((i[2] * n[1] + i[1]) * n[0] + i[0]);
        ++m.start[cell_of[(size_t)k] + 1];
    }
    for (size_t c = 0; c < cells; ++c) m.start[c + 1] += m.start[c];
    std::vector<uint32_t> at(m.start.begin(), m.start.end() - 1);
    m.items.assign((size_t)K, 0);
    for (int32_t k = 0; k < K; ++k) m.items[at[cell_of[(size_t)k]]++] = (uint32_t)k;          // ascending k within a cell
    m.set = true;
}

}  // namespace hare

using namespace hare;

// ---- what hare_direct_device, hare_image_device and hare_image2_device share (the calls themselves are below).  Their checks fire in
// this order: deposit_call_check, the call's own list lengths, deposit_buffers_check -- all HARE_E_INVALID, ahead of the device.
// The scene, the weight and the numbers; flags comes back masked to what these calls read
static int deposit_call_check(const char* who, const Scene* s, int32_t kind, int32_t top, int64_t n_weight, uint32_t& flags, int32_t n_bins,
                              double bin_len, int32_t frac_bits)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (int rc = receive_check_order(who, flags)) return rc;
    if (n_weight < 1 || n_weight > ((int64_t)1 << 53)) {
        set_error(std::string(who) + ": n_weight out of range (1 .. 2^53)");
        return HARE_E_INVALID;
    }
    flags &= kReceiveChannelFlags;
    if (int rc = receive_check_args(who, *s, flags, kind, top, 0, 1, n_bins, bin_len, frac_bits)) return rc;
    if (s->src.set && s->src.B != scene_bands(*s, top)) {
        set_error(std::string(who) + ": the source has " + std::to_string(s->src.B) + " bands, the topology " + std::to_string(scene_bands(*s, top)));
        return HARE_E_INVALID;
    }
    return HARE_OK;
}

// hare_image_device's checks in its order, then the detour and the edge table's band count
int hare::diffract_call_check(const char* who, const Scene* s, int32_t kind, int32_t top, int64_t n_weight, uint32_t& flags, int32_t n_bins,
                              double bin_len, int32_t frac_bits, double max_detour, int64_t max_pairs)
{
    if (int rc = deposit_call_check(who, s, kind, top, n_weight, flags, n_bins, bin_len, frac_bits)) return rc;
    if (max_pairs < 1 || max_pairs > ((int64_t)1 << 26)) {
        set_error(std::string(who) + ": max_pairs out of range (1 .. 2^26)");
        return HARE_E_INVALID;
    }
    if (!(max_detour >= 0)) {
        set_error(std::string(who) + ": max_detour must be >= 0 (+inf: no limit)");
        return HARE_E_INVALID;
    }
    if (s->src.set && scene_edges(*s, top) > 0 && s->src.B != s->edges[(size_t)top].B) {
        set_error(std::string(who) + ": the source has " + std::to_string(s->src.B) + " bands, the edge table " +
                  std::to_string(s->edges[(size_t)top].B));
        return HARE_E_INVALID;
    }
    return HARE_OK;
}

// The three buffers: none null, the work array on a 16-byte boundary where the call does not align it itself, no two overlapping
static int deposit_buffers_check(const char* who, const Scene& s, int32_t top, uint32_t flags, int32_t n_bins, const void* d_work, size_t work_bytes,
                                 bool need_aligned, const void* d_hist, const void* d_det)
{
    if (!d_work || !d_hist || !d_det || (need_aligned && ((uintptr_t)d_work & 15u))) {
        set_error(std::string(who) + ": null work array / histogram / detections" + (need_aligned ? ", or a work array off a 16-byte boundary" : ""));
        return HARE_E_INVALID;
    }
    const size_t K = std::max<size_t>(1, s.rcv.size() / 4);
    if (spans_overlap({{d_work, work_bytes}, {d_hist, receive_hist_words(s, top, n_bins, flags, 1) * sizeof(uint64_t)}, {d_det, K * 2 * sizeof(uint64_t)}}, 3)) {
        set_error(std::string(who) + ": work array, histogram and detections must not overlap");
        return HARE_E_INVALID;
    }
    return HARE_OK;
}

// The device, the module, the source, the polygons and the receivers, then the call's own enqueue under the scene's device
template <class Enqueue>
static int deposit_call_run(Scene& s, const char* who, Enqueue enqueue)
{
    return device_call(s, [&](const HipApi* H) -> int {
        if (int rc = source_ready(s, H, who)) return rc;
        if (int rc = upload_polys(s, H)) return rc;
        if (int rc = receive_ready(s, H, who)) return rc;
        return enqueue(H);
    });
}

extern "C" {

int hare_scene_set_receivers(hare_scene* s, int32_t K, const double* centers, const double* radii)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (int rc = check_receivers("hare_scene_set_receivers", K, kMaxReceivers, centers, radii)) return rc;
    GUARD_BEGIN
    std::vector<double> r = receiver_block(K, centers, radii);
    s->rcv.swap(r);
    s->rmap.set = false;
    s->rmap.start.clear();
    s->rmap.items.clear();
    return push_receivers(s);
    GUARD_END
}

int hare_scene_set_receiver_map(hare_scene* s, int32_t K, const double* centers, const double* radii, double cell)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (int rc = check_receivers("hare_scene_set_receiver_map", K, kMaxMapReceivers, centers, radii)) return rc;
    if (!(cell >= 0 && std::isfinite(cell))) {
        set_error("hare_scene_set_receiver_map: cell must be finite and >= 0 (0: 2 r_max)");
        return HARE_E_INVALID;
    }
    GUARD_BEGIN
    std::vector<double> r = receiver_block(K, centers, radii);
    Scene::ReceiverMap m;
    build_receiver_map(m, K, centers, radii, cell);
    m.d_rcv = s->rmap.d_rcv;                         // the device copies are replaced by the upload
    m.d_start = s->rmap.d_start;
    m.d_items = s->rmap.d_items;
    s->rcv.swap(r);
    s->rmap = std::move(m);
    return push_receivers(s);
    GUARD_END
}

int hare_scene_get_receiver_map(const hare_scene* s, double* geom, int32_t* dims, uint32_t* cell_start, uint32_t* cell_items)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (!s->rmap.set) {
        set_error("hare_scene_get_receiver_map: no receiver map set (hare_scene_set_receiver_map)");
        return HARE_E_STATE;
    }
    const Scene::ReceiverMap& m = s->rmap;
    if (geom) {
        for (int a = 0; a < 3; ++a) geom[a] = m.org[a];
        geom[3] = m.h;
        geom[4] = m.R;
    }
    if (dims)
        for (int a = 0; a < 3; ++a) dims[a] = m.n[a];
    if (cell_start) memcpy(cell_start, m.start.data(), m.start.size() * sizeof(uint32_t));
    if (cell_items) memcpy(cell_items, m.items.data(), m.items.size() * sizeof(uint32_t));
    return HARE_OK;
}

int hare_scene_set_absorption(hare_scene* s, int32_t top_index, int32_t B, const double* alpha)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (top_index < 0 || top_index >= (int32_t)s->topos.size() || B < 1 || B > kMaxBands) {
        set_error("hare_scene_set_absorption: bad top_index or bands (1 .. 8)");
        return HARE_E_INVALID;
    }
    GUARD_BEGIN
    return set_band_table(*s, "hare_scene_set_absorption", "alpha", s->alpha, s->sigma, "scattering", top_index, B, alpha);
    GUARD_END
}

int hare_scene_set_scattering(hare_scene* s, int32_t top_index, int32_t B, const double* sigma)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (top_index < 0 || top_index >= (int32_t)s->topos.size()) {
        set_error("hare_scene_set_scattering: bad top_index");
        return HARE_E_INVALID;
    }
    if (B == 0 && !sigma) {                          // removal
        if (!has_table(s->sigma, top_index)) return HARE_OK;
        Scene::BandTable& t = s->sigma[(size_t)top_index];
        t.host.clear();
        t.on_device = false;
        if (!has_table(s->alpha, top_index)) s->bands[(size_t)top_index] = 1;
        const HipApi* H = t.dev ? hip_api(nullptr) : nullptr;
        if (H) {
            DeviceGuard dev_guard(H, s->device);
            dev_free(H, t.dev);
        }
        return HARE_OK;
    }
    if (B < 1 || B > kMaxBands) {
        set_error("hare_scene_set_scattering: bands out of range (1 .. 8; 0 with a null table removes it)");
        return HARE_E_INVALID;
    }
    GUARD_BEGIN
    return set_band_table(*s, "hare_scene_set_scattering", "sigma", s->sigma, s->alpha, "absorption", top_index, B, sigma);
    GUARD_END
}

int hare_scene_set_source(hare_scene* s, const double pos[3], int32_t B, const double* power, const double* frame, int32_t R, const double* gain)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    auto bad = [&](const std::string& what) {
        set_error("hare_scene_set_source: " + what);
        return HARE_E_INVALID;
    };
    if (!pos || !(std::isfinite(pos[0]) && std::isfinite(pos[1]) && std::isfinite(pos[2]))) return bad("need a finite position");
    if (B < 1 || B > kMaxBands) return bad("bands out of range (1 .. 8)");
    if (R < 0 || R > kMaxSourceRes) return bad("table resolution out of range (0 .. 64)");
    if ((R == 0) != (gain == nullptr)) return bad("a directivity table needs R >= 1, and R >= 1 a table");
    if (frame)
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(frame[k])) return bad("non-finite frame");
    if (power)
        for (int32_t b = 0; b < B; ++b)
            if (!(std::isfinite(power[b]) && power[b] >= 0)) return bad("power[" + std::to_string(b) + "] must be finite and >= 0");
    const size_t cnt = (size_t)6 * (size_t)R * (size_t)R * (size_t)B;
    for (size_t k = 0; k < cnt; ++k)
        if (!(std::isfinite(gain[k]) && gain[k] >= 0)) return bad("gain[" + std::to_string(k) + "] must be finite and >= 0");
    GUARD_BEGIN
    std::vector<double> g(gain, gain + cnt);
    Scene::Source& src = s->src;
    memcpy(src.pos, pos, sizeof src.pos);
    src.B = B;
    for (int32_t b = 0; b < kMaxBands; ++b) src.power[b] = b < B ? (power ? power[b] : 1.0) : 0.0;
    for (int k = 0; k < 9; ++k) src.frame[k] = frame ? frame[k] : (k % 4 == 0 ? 1.0 : 0.0);
    src.R = R;
    src.gain.swap(g);
    src.on_device = false;
    src.set = true;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;          // GPU-less: the table goes up with the first call that emits
    DeviceGuard dev_guard(H, s->device);
    if (int rc = ensure_device(*s, H)) return rc;
    if (src.gain.empty()) {                          // a table replaced by none
        dev_free(H, src.d_gain);
        return HARE_OK;
    }
    return upload_source(*s, H);
    GUARD_END
}

int hare_scene_set_edges(hare_scene* s, int32_t top_index, int32_t E, const double* ends, const int32_t* faces, int32_t B, const double* inv_lambda)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    auto bad = [&](const std::string& what) {
        set_error("hare_scene_set_edges: " + what);
        return HARE_E_INVALID;
    };
    if (top_index < 0 || top_index >= (int32_t)s->topos.size()) return bad("bad top_index");
    if (E == 0 && !ends && !faces) {                 // removal
        if (scene_edges(*s, top_index) == 0) return HARE_OK;
        Scene::EdgeTable& t = s->edges[(size_t)top_index];
        t.ends.clear();
        t.faces.clear();
        t.B = 0;
        t.on_device = false;
        const HipApi* H = (t.d_ends || t.d_faces) ? hip_api(nullptr) : nullptr;
        if (H) {
            DeviceGuard dev_guard(H, s->device);
            dev_free(H, t.d_ends);
            dev_free(H, t.d_faces);
        }
        return HARE_OK;
    }
    if (E < 1 || E > (1 << 20)) return bad("E out of range (1 .. 2^20; 0 with null arrays removes the table)");
    if (!ends || !faces) return bad("null ends / faces");
    const int64_t P = s->topos[(size_t)top_index].P;
    for (int32_t j = 0; j < E; ++j) {
        const double* const a = ends + 6 * (size_t)j;
        for (int c = 0; c < 6; ++c)
            if (!std::isfinite(a[c])) return bad("edge " + std::to_string(j) + " has a non-finite end");
        const double ex = a[3] - a[0], ey = a[4] - a[1], ez = a[5] - a[2];
        const double ee = (ex * ex + ey * ey) + ez * ez;
        if (!(ee > 0 && std::isfinite(ee))) return bad("edge " + std::to_string(j) + " has no length (a == b), or one whose square overflows");
    }
    for (size_t k = 0; k < 2 * (size_t)E; ++k)
        if (faces[k] < -1 || faces[k] >= P) return bad("faces[" + std::to_string(k) + "] outside -1 .. P - 1");
    if (B < 1 || B > kMaxBands) return bad("bands out of range (1 .. 8)");
    if (!inv_lambda) return bad("null inv_lambda");
    for (int32_t b = 0; b < B; ++b)
        if (!(inv_lambda[b] >= 0 && std::isfinite(inv_lambda[b]))) return bad("inv_lambda[" + std::to_string(b) + "] must be finite and >= 0");
    GUARD_BEGIN
    std::vector<double> e(ends, ends + 6 * (size_t)E);
    std::vector<int32_t> f(faces, faces + 2 * (size_t)E);
    if (s->edges.size() < s->topos.size()) s->edges.resize(s->topos.size());
    Scene::EdgeTable& t = s->edges[(size_t)top_index];
    t.ends.swap(e);
    t.faces.swap(f);
    t.B = B;
    for (int32_t b = 0; b < kMaxBands; ++b) t.inv_lambda[b] = b < B ? inv_lambda[b] : 0.0;
    t.on_device = false;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;          // GPU-less: the table goes up with the first diffraction call
    DeviceGuard dev_guard(H, s->device);
    if (int rc = ensure_device(*s, H)) return rc;
    return upload_edges(t, H);
    GUARD_END
}

int hare_emit_device(hare_scene* s, int64_t n, int64_t first_ray, void* d_rays, void* d_state, void* stream)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (n < 0 || n > 0x7FFFFF00ll) {
        set_error("hare_emit_device: n out of range (0 .. 2^31 - 256)");
        return HARE_E_INVALID;
    }
    if (int rc = source_check_range("hare_emit_device", n, first_ray)) return rc;
    if (n > 0) {
        const int32_t B = s->src.set ? s->src.B : 1;
        if (!d_rays || !d_state) {
            set_error("hare_emit_device: null rays / state");
            return HARE_E_INVALID;
        }
        if (ranges_overlap(d_rays, (size_t)n * sizeof(hare_ray), d_state, (size_t)n * (size_t)(1 + B) * sizeof(double))) {
            set_error("hare_emit_device: rays and state must not overlap");
            return HARE_E_INVALID;
        }
    }
    return device_call(*s, [&](const HipApi* H) -> int {
        if (int rc = source_ready(*s, H, "hare_emit_device")) return rc;
        return emit_source(*s, H, n, first_ray, d_rays, d_state, (hipStream_t)stream);
    });
}

int hare_direct_device(hare_scene* s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                       int32_t frac_bits, void* d_work, void* d_hist, void* d_detections, void* stream)
{
    const char* const who = "hare_direct_device";
    if (int rc = deposit_call_check(who, s, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits)) return rc;
    const size_t K = std::max<size_t>(1, s->rcv.size() / 4);
    if (int rc = deposit_buffers_check(who, *s, top_index, flags, n_bins, d_work, (size_t)HARE_DIRECT_WORK_BYTES(K), false, d_hist, d_detections)) return rc;
    return deposit_call_run(*s, who, [&](const HipApi* H) {
        return direct_enqueue(*s, H, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, d_work, d_hist, d_detections, (hipStream_t)stream);
    });
}

int hare_image_device(hare_scene* s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                      int32_t frac_bits, int64_t max_pairs, void* d_work, void* d_hist, void* d_detections, void* stream)
{
    const char* const who = "hare_image_device";
    if (int rc = deposit_call_check(who, s, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits)) return rc;
    if (max_pairs < 1 || max_pairs > ((int64_t)1 << 26)) {
        set_error(std::string(who) + ": max_pairs out of range (1 .. 2^26)");
        return HARE_E_INVALID;
    }
    const size_t K = std::max<size_t>(1, s->rcv.size() / 4);
    const size_t work_bytes = (size_t)HARE_IMAGE_WORK_BYTES(K, s->topos[(size_t)top_index].P, max_pairs);
    if (int rc = deposit_buffers_check(who, *s, top_index, flags, n_bins, d_work, work_bytes, true, d_hist, d_detections)) return rc;
    return deposit_call_run(*s, who, [&](const HipApi* H) {
        return image_enqueue(*s, H, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_pairs, d_work, d_hist, d_detections,
                             (hipStream_t)stream);
    });
}

int hare_image2_device(hare_scene* s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                       int32_t frac_bits, int64_t max_cands, int64_t max_paths, void* d_work, void* d_hist, void* d_detections, void* stream)
{
    const char* const who = "hare_image2_device";
    if (int rc = deposit_call_check(who, s, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits)) return rc;
    if (max_cands < 1 || max_cands > ((int64_t)1 << 26) || max_paths < 1 || max_paths > ((int64_t)1 << 26)) {
        set_error(std::string(who) + ": max_cands or max_paths out of range (1 .. 2^26)");
        return HARE_E_INVALID;
    }
    const size_t work_bytes = (size_t)HARE_IMAGE2_WORK_BYTES(s->topos[(size_t)top_index].P, max_cands, max_paths);
    if (int rc = deposit_buffers_check(who, *s, top_index, flags, n_bins, d_work, work_bytes, true, d_hist, d_detections)) return rc;
    return deposit_call_run(*s, who, [&](const HipApi* H) {
        return image2_enqueue(*s, H, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_cands, max_paths, d_work, d_hist, d_detections,
                              (hipStream_t)stream);
    });
}

int hare_diffract_device(hare_scene* s, int32_t kind, int32_t top_index, int64_t n_weight, uint32_t flags, int32_t n_bins, double bin_len,
                         int32_t frac_bits, double max_detour, int64_t max_pairs, void* d_work, void* d_hist, void* d_detections, void* stream)
{
    const char* const who = "hare_diffract_device";
    if (int rc = diffract_call_check(who, s, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_detour, max_pairs)) return rc;
    const size_t K = std::max<size_t>(1, s->rcv.size() / 4);
    if (int rc = deposit_buffers_check(who, *s, top_index, flags, n_bins, d_work, (size_t)HARE_DIFFRACT_WORK_BYTES(K, max_pairs), true, d_hist, d_detections))
        return rc;
    return deposit_call_run(*s, who, [&](const HipApi* H) -> int {
        if (int rc = diffract_ready(*s, H, top_index, who)) return rc;
        return diffract_enqueue(*s, H, kind, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_detour, max_pairs, d_work, d_hist,
                                d_detections, (hipStream_t)stream);
    });
}

int hare_receive_device(hare_scene* s, int32_t kind, int32_t top_index, int64_t n, void* d_rays, const void* d_excl1, const void* d_excl2,
                        int32_t bounces, uint32_t flags, int32_t n_bins, double bin_len, int32_t frac_bits, void* d_state, void* d_work,
                        void* d_events_last, void* d_hist, void* d_detections, void* d_counters, void* stream)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (int rc = receive_check_args("hare_receive_device", *s, flags, kind, top_index, n, bounces, n_bins, bin_len, frac_bits)) return rc;
    if ((flags & (HARE_RECEIVE_DIRECT | HARE_RECEIVE_IMAGE)) && s->src.set && s->src.B != scene_bands(*s, top_index)) {
        set_error("hare_receive_device: the source has " + std::to_string(s->src.B) + " bands, the topology " + std::to_string(scene_bands(*s, top_index)));
        return HARE_E_INVALID;
    }
    const size_t K = std::max<size_t>(1, s->rcv.size() / 4);
    const int32_t B = scene_bands(*s, top_index);
    const bool rain = (flags & HARE_RECEIVE_DIFFUSE_RAIN) != 0;
    if (n > 0) {
        if (!d_rays || !d_state || !d_work || !d_events_last || !d_hist || !d_detections) {
            set_error("hare_receive_device: null rays / state / work array / events / histogram / detections");
            return HARE_E_INVALID;
        }
        struct Buf { const void* p; size_t bytes; bool written; };
        const Buf bufs[] = {{d_rays, (size_t)n * sizeof(hare_ray), true},
                            {d_state, (size_t)n * (size_t)(1 + B) * sizeof(double), true},
                            {d_work, (rain ? (size_t)HARE_RECEIVE_RAIN_WORK_BYTES(n) : (size_t)n * 2 * sizeof(int32_t)) +
                                         ((flags & HARE_RECEIVE_IMAGE2) ? (size_t)HARE_RECEIVE_IMAGE2_WORK_BYTES(n) : 0), true},
                            {d_events_last, (size_t)n * sizeof(hare_xevent), true},
                            {d_hist, receive_hist_words(*s, top_index, n_bins, flags, 1) * sizeof(uint64_t), true},
                            {d_detections, K * 2 * sizeof(uint64_t), true},
                            {d_counters, sizeof(hare_counters), true},
                            {d_excl1, (size_t)n * sizeof(int32_t), false},
                            {d_excl2, (size_t)n * sizeof(int32_t), false}};
        const size_t nb = sizeof bufs / sizeof bufs[0];
        for (size_t a = 0; a < nb; ++a)
            for (size_t b = a + 1; b < nb; ++b)
                if ((bufs[a].written || bufs[b].written) && ranges_overlap(bufs[a].p, bufs[a].bytes, bufs[b].p, bufs[b].bytes)) {
                    set_error("hare_receive_device: rays, exclusions, state, work array, events, histogram, detections and counters must not overlap");
                    return HARE_E_INVALID;
                }
    }
    return device_call(*s, [&](const HipApi* H) -> int {
        if (int rc = upload_polys(*s, H)) return rc;
        if (int rc = receive_ready(*s, H, "hare_receive_device")) return rc;
        if (flags & (HARE_RECEIVE_DIRECT | HARE_RECEIVE_IMAGE))      // suppression only, but of the SOURCE's paths: hare_direct_device / hare_image_device deposit them
            if (int rc = source_ready(*s, H, "hare_receive_device")) return rc;
        if (n == 0) return HARE_OK;
        ReceivePlan plan;
        if (int rc = receive_plan(*s, top_index, flags, n, n_bins, bin_len, frac_bits, d_state, d_hist, d_detections, d_work, false, 0, plan)) return rc;
        flags &= HARE_SHOOT_COUNT_WORK | HARE_SHOOT_SIMPLE_KERNEL;
        return bounce_device_impl(*s, H, kind, top_index, n, d_rays, d_excl1, d_excl2, bounces, flags, d_work, nullptr, d_events_last, d_counters,
                                  nullptr, (hipStream_t)stream, &plan);
    });
}

}  // extern "C"
