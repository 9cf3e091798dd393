// receive.cpp -- receivers, absorption and scattering of a scene (hare_scene_set_receivers / _absorption / _scattering) and hare_receive_device,
// the bounce loop with the receiver step (and, on request, diffuse rain) between its casts (include/hare_hip.h, "receivers"; the kernel: receive.hip).  The host-buffer
// calls hare_receive_batch / _sharded are in bounce.cpp, beside the loop they share with hare_bounce_batch.
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

// The host copies to the device: fixed-size receiver block (never reallocated), an absorption and a scattering table per topology.  Called by the setters
// when a device is present -- as a build pushes its partition -- and by a receive call only for what a setter could not upload.
int upload_receivers(Scene& s, const HipApi* H)
{
    if (!s.rcv.empty() && !s.rcv_on_device) {
        if (!s.d_rcv) HIP_TRY(H->Malloc(&s.d_rcv, (size_t)kMaxReceivers * 4 * sizeof(double)));
        HIP_TRY(H->Memcpy(s.d_rcv, s.rcv.data(), s.rcv.size() * sizeof(double), hipMemcpyHostToDevice));
        s.rcv_on_device = true;
    }
    s.d_alpha.resize(s.topos.size(), nullptr);
    s.alpha_on_device.resize(s.topos.size(), 0);
    for (size_t m = 0; m < s.alpha.size(); ++m) {
        if (s.alpha[m].empty() || s.alpha_on_device[m]) continue;
        if (int rc = upload(H, &s.d_alpha[m], s.alpha[m].data(), s.alpha[m].size() * sizeof(double))) return rc;
        s.alpha_on_device[m] = 1;
    }
    s.d_sigma.resize(s.topos.size(), nullptr);
    s.sigma_on_device.resize(s.topos.size(), 0);
    for (size_t m = 0; m < s.sigma.size(); ++m) {
        if (s.sigma[m].empty() || s.sigma_on_device[m]) continue;
        if (int rc = upload(H, &s.d_sigma[m], s.sigma[m].data(), s.sigma[m].size() * sizeof(double))) return rc;
        s.sigma_on_device[m] = 1;
    }
    return HARE_OK;
}

void free_receivers(const HipApi* H, Scene& s)
{
    dev_free(H, s.d_rcv);
    for (void*& p : s.d_alpha) dev_free(H, p);
    for (void*& p : s.d_sigma) dev_free(H, p);
}

bool scene_has_scattering(const Scene& s, int32_t top)
{
    return top >= 0 && (size_t)top < s.sigma.size() && !s.sigma[(size_t)top].empty();
}

int32_t scene_bands(const Scene& s, int32_t top)
{
    return (top >= 0 && (size_t)top < s.bands.size() && s.bands[(size_t)top] > 0) ? s.bands[(size_t)top] : 1;
}

// Everything a receive call checks before anything runs (HARE_E_INVALID); K is the scene's receiver count (0: unset, counted as 1 here --
// "no receivers" is HARE_E_STATE, after the device checks)
int receive_check_args(const char* who, const Scene& s, uint32_t flags, int32_t kind, int32_t top, int64_t n, int32_t bounces, int32_t n_bins, double bin_len,
                       int32_t frac_bits)
{
    auto bad = [&](const char* what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (kind < HARE_KIND_VOXEL || kind > HARE_KIND_KDTREE) return bad("bad kind");
    if (top < 0 || top >= (int32_t)s.topos.size()) return bad("bad top_index");
    if (n < 0 || n > 0x7FFFFF00ll) return bad("n out of range (0 .. 2^31 - 256)");
    if (bounces < 1 || bounces > 4096) return bad("bounces out of range (1 .. 4096)");
    if (n_bins < 1) return bad("n_bins must be >= 1");
    if (!(std::isfinite(bin_len) && bin_len > 0)) return bad("bin_len must be finite and > 0");
    if (frac_bits < 0 || frac_bits > 62) return bad("frac_bits out of range (0 .. 62)");
    const int64_t K = std::max<int64_t>(1, (int64_t)(s.rcv.size() / 4));
    if (K * (int64_t)n_bins * (int64_t)scene_bands(s, top) > ((int64_t)1 << 27)) return bad("receivers x n_bins x bands exceeds 2^27");
    if ((flags & HARE_RECEIVE_DIRECTIONAL) && K * (int64_t)n_bins * (int64_t)scene_bands(s, top) * 4 > ((int64_t)1 << 27))
        return bad("receivers x n_bins x bands x 4 channels (HARE_RECEIVE_DIRECTIONAL) exceeds 2^27");
    return HARE_OK;
}

// The ReceiveArgs of one call (the loop fills in rays, events, marks per cast); receivers and tables must be on the device
int receive_args(const Scene& s, int32_t top, int32_t n_bins, double bin_len, int32_t frac_bits, void* d_state, void* d_hist, void* d_det,
                 bool init_state, int64_t ray_base, ReceiveArgs& ra)
{
    memset(&ra, 0, sizeof ra);
    const int32_t B = scene_bands(s, top);
    ra.state = (double*)d_state;
    ra.alpha = ((size_t)top < s.d_alpha.size() && (size_t)top < s.alpha.size() && !s.alpha[(size_t)top].empty()) ? (const double*)s.d_alpha[(size_t)top] : nullptr;
    ra.rcv = (const double*)s.d_rcv;
    ra.hist = (unsigned long long*)d_hist;
    ra.det = (unsigned long long*)d_det;
    ra.bin_len = bin_len;
    ra.scale = ldexp(1.0, frac_bits);
    ra.bands = B;
    ra.n_rcv = (int32_t)(s.rcv.size() / 4);
    ra.n_bins = n_bins;
    ra.aggregate = s.opt.receive_aggregate;
    ra.init_state = init_state ? 1 : 0;
    ra.sigma = ((size_t)top < s.d_sigma.size() && scene_has_scattering(s, top)) ? (const double*)s.d_sigma[(size_t)top] : nullptr;
    ra.seed = (unsigned long long)s.opt.scatter_seed;
    ra.ray_base = (long long)ray_base;
    if (ra.sigma == nullptr && scene_has_scattering(s, top)) {
        set_error("receive: scattering table not on the device");
        return HARE_E_STATE;
    }
    if (ra.alpha == nullptr && !s.alpha.empty() && (size_t)top < s.alpha.size() && !s.alpha[(size_t)top].empty()) {
        set_error("receive: absorption table not on the device");
        return HARE_E_STATE;
    }
    return HARE_OK;
}

// The rain's scratch in a receive call's work array: behind the loop's 2 n int32, from a 16-byte boundary: n shadow rays (48 B), n t_max,
// n exclusions, n occlusion flags, n suppression flags: 76 n bytes in all and at most 15 of padding, within HARE_RECEIVE_RAIN_WORK_BYTES(n)
RainWork rain_work(void* d_work, int64_t n)
{
    RainWork w;
    w.rays = (RayRec*)(((uintptr_t)d_work + (uintptr_t)n * 8u + 15u) & ~(uintptr_t)15u);
    w.tmax = (double*)(w.rays + n);
    w.excl = (int32_t*)(w.tmax + n);
    w.occ = w.excl + n;
    w.flag = w.occ + n;
    return w;
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

}  // namespace hare

using namespace hare;

#define GUARD_BEGIN try {
#define GUARD_END                                               \
    }                                                           \
    catch (const std::bad_alloc&)                               \
    {                                                           \
        set_error("out of host memory");                        \
        return HARE_E_NOMEM;                                    \
    }                                                           \
    catch (...)                                                 \
    {                                                           \
        set_error("unexpected C++ exception");                  \
        return HARE_E_INVALID;                                  \
    }

extern "C" {

int hare_scene_set_receivers(hare_scene* s, int32_t K, const double* centers, const double* radii)
{
    if (!s) {
        set_error("null scene");
        return HARE_E_INVALID;
    }
    if (K < 1 || K > kMaxReceivers || !centers || !radii) {
        set_error("hare_scene_set_receivers: need 1 .. 256 receivers, centers and radii");
        return HARE_E_INVALID;
    }
    for (int32_t k = 0; k < K; ++k) {
        if (!std::isfinite(centers[3 * k]) || !std::isfinite(centers[3 * k + 1]) || !std::isfinite(centers[3 * k + 2])) {
            set_error("hare_scene_set_receivers: receiver " + std::to_string(k) + " has a non-finite center");
            return HARE_E_INVALID;
        }
        if (!(std::isfinite(radii[k]) && radii[k] > 0)) {
            set_error("hare_scene_set_receivers: receiver " + std::to_string(k) + " needs a finite radius > 0");
            return HARE_E_INVALID;
        }
    }
    GUARD_BEGIN
    std::vector<double> r((size_t)K * 4);
    for (int32_t k = 0; k < K; ++k) {
        r[4 * (size_t)k + 0] = centers[3 * k];
        r[4 * (size_t)k + 1] = centers[3 * k + 1];
        r[4 * (size_t)k + 2] = centers[3 * k + 2];
        r[4 * (size_t)k + 3] = radii[k] * radii[k];
    }
    s->rcv.swap(r);
    s->rcv_on_device = false;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;          // GPU-less: the host copy goes up with the first receive call
    DeviceGuard dev_guard(H, s->device);
    if (int rc = ensure_device(*s, H)) return rc;
    return upload_receivers(*s, H);
    GUARD_END
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
    const size_t cnt = (size_t)s->topos[(size_t)top_index].P * (size_t)B;
    if (cnt > 0 && !alpha) {
        set_error("hare_scene_set_absorption: null alpha");
        return HARE_E_INVALID;
    }
    for (size_t k = 0; k < cnt; ++k)
        if (!(alpha[k] >= 0.0 && alpha[k] <= 1.0)) {
            set_error("hare_scene_set_absorption: alpha[" + std::to_string(k) + "] outside [0, 1]");
            return HARE_E_INVALID;
        }
    if (scene_has_scattering(*s, top_index) && B != scene_bands(*s, top_index)) {
        set_error("hare_scene_set_absorption: B differs from the topology's scattering table (" + std::to_string(scene_bands(*s, top_index)) + " bands)");
        return HARE_E_INVALID;
    }
    GUARD_BEGIN
    s->alpha.resize(s->topos.size());
    s->bands.resize(s->topos.size(), 1);
    s->alpha_on_device.resize(s->topos.size(), 0);
    std::vector<double> a(alpha, alpha + cnt);
    if (a.empty()) a.assign((size_t)B, 0.0);       // a topology without polygons: a table of one row no ray reads
    s->alpha[(size_t)top_index].swap(a);
    s->bands[(size_t)top_index] = B;
    s->alpha_on_device[(size_t)top_index] = 0;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;
    DeviceGuard dev_guard(H, s->device);
    if (int rc = ensure_device(*s, H)) return rc;
    return upload_receivers(*s, H);
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
    const bool remove = B == 0 && !sigma;
    if (!remove && (B < 1 || B > kMaxBands)) {
        set_error("hare_scene_set_scattering: bands out of range (1 .. 8; 0 with a null table removes it)");
        return HARE_E_INVALID;
    }
    const size_t cnt = remove ? 0 : (size_t)s->topos[(size_t)top_index].P * (size_t)B;
    if (!remove && cnt > 0 && !sigma) {
        set_error("hare_scene_set_scattering: null sigma");
        return HARE_E_INVALID;
    }
    for (size_t k = 0; k < cnt; ++k)
        if (!(sigma[k] >= 0.0 && sigma[k] <= 1.0)) {
            set_error("hare_scene_set_scattering: sigma[" + std::to_string(k) + "] outside [0, 1]");
            return HARE_E_INVALID;
        }
    const bool has_alpha = (size_t)top_index < s->alpha.size() && !s->alpha[(size_t)top_index].empty();
    if (!remove && has_alpha && B != scene_bands(*s, top_index)) {
        set_error("hare_scene_set_scattering: B differs from the topology's absorption table (" + std::to_string(scene_bands(*s, top_index)) + " bands)");
        return HARE_E_INVALID;
    }
    GUARD_BEGIN
    s->sigma.resize(s->topos.size());
    s->bands.resize(s->topos.size(), 1);
    s->sigma_on_device.resize(s->topos.size(), 0);
    s->d_sigma.resize(s->topos.size(), nullptr);
    if (remove) {
        s->sigma[(size_t)top_index].clear();
        if (!has_alpha) s->bands[(size_t)top_index] = 1;
        s->sigma_on_device[(size_t)top_index] = 0;
        if (s->d_sigma[(size_t)top_index]) {
            const HipApi* H = hip_api(nullptr);
            if (H) {
                DeviceGuard dev_guard(H, s->device);
                dev_free(H, s->d_sigma[(size_t)top_index]);
            }
        }
        return HARE_OK;
    }
    std::vector<double> t(sigma, sigma + cnt);
    if (t.empty()) t.assign((size_t)B, 0.0);       // a topology without polygons: a table of one row no ray reads
    s->sigma[(size_t)top_index].swap(t);
    s->bands[(size_t)top_index] = B;
    s->sigma_on_device[(size_t)top_index] = 0;
    const HipApi* H = nullptr;
    if (!device_present(H)) return HARE_OK;
    DeviceGuard dev_guard(H, s->device);
    if (int rc = ensure_device(*s, H)) return rc;
    return upload_receivers(*s, H);
    GUARD_END
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
    const int64_t K = std::max<int64_t>(1, (int64_t)(s->rcv.size() / 4));
    const int32_t B = scene_bands(*s, top_index);
    const bool rain = (flags & HARE_RECEIVE_DIFFUSE_RAIN) != 0;
    const bool directional = (flags & HARE_RECEIVE_DIRECTIONAL) != 0;      // four channels per histogram word
    if (n > 0) {
        if (!d_rays || !d_state || !d_work || !d_events_last || !d_hist || !d_detections) {
            set_error("hare_receive_device: null rays / state / work array / events / histogram / detections");
            return HARE_E_INVALID;
        }
        struct Buf { const void* p; size_t bytes; bool written; };
        const Buf bufs[] = {{d_rays, (size_t)n * sizeof(hare_ray), true},
                            {d_state, (size_t)n * (size_t)(1 + B) * sizeof(double), true},
                            {d_work, rain ? (size_t)HARE_RECEIVE_RAIN_WORK_BYTES(n) : (size_t)n * 2 * sizeof(int32_t), true},
                            {d_events_last, (size_t)n * sizeof(hare_xevent), true},
                            {d_hist, (size_t)K * (size_t)n_bins * (size_t)B * (directional ? 4u : 1u) * sizeof(uint64_t), true},
                            {d_detections, (size_t)K * 2 * sizeof(uint64_t), true},
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
    GUARD_BEGIN
    const HipApi* H = api_or_err();
    if (!H) return HARE_E_NODEVICE;
    DeviceGuard dev_guard(H, s->device);
    if (!s->module) {
        int rc = ensure_device(*s, H);
        if (rc) return rc;
    }
    if (int rc = upload_polys(*s, H)) return rc;
    if (int rc = receive_ready(*s, H, "hare_receive_device")) return rc;
    if (n == 0) return HARE_OK;
    ReceiveArgs ra;
    if (int rc = receive_args(*s, top_index, n_bins, bin_len, frac_bits, d_state, d_hist, d_detections, false, 0, ra)) return rc;
    flags &= HARE_SHOOT_COUNT_WORK | HARE_SHOOT_SIMPLE_KERNEL;
    RainWork rw;
    if (rain && ra.sigma) {                 // rain needs a scattering table: without one the flag changes nothing
        rw = rain_work(d_work, n);
        ra.rain_flag = rw.flag;
    }
    return bounce_device_impl(*s, H, kind, top_index, n, d_rays, d_excl1, d_excl2, bounces, flags, d_work, nullptr, d_events_last, d_counters,
                              nullptr, (hipStream_t)stream, &ra, ra.rain_flag ? &rw : nullptr, directional);
    GUARD_END
}

}  // extern "C"
