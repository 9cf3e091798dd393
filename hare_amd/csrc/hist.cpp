// hist.cpp -- what runs on a receive histogram once it is on the device (include/hare_hip.h, "receivers"): the reduction (hare_hist_reduce
// / _device; the kernel: reduce.hip), the projection (hare_hist_project / _device; project.hip) and its directional form (hare_hist_project_channels / _device; project_channels.hip), the rendering (hare_hist_render /
// _device; render.hip), the impulses of a per-sample histogram (hare_hist_impulses / _device; impulses.hip) and, on the rendered rows, the convolution with a dry signal (hare_convolve / _device; convolve.hip) and the
// decoding through a matrix of FIR filters (hare_decode / _device; decode.hip).  A call is its own check and its own enqueue; what the calls share is the device prelude (device_call, launch.h),
// the overlap test (spans_overlap, scene.h), one byte count per buffer, used by the check and by the staging, and the staging of the
// host-buffer calls (staged_run).  reduce_check_spec and reduce_enqueue also serve hare_receive_*_reduced (bounce.cpp).
// Product code; nothing from oracle/.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "../../include/hare_hip.h"
#include "launch.h"
#include "scene.h"

namespace hare {

namespace {

int null_scene()
{
    set_error("null scene");
    return HARE_E_INVALID;
}

// the two buffers every call reads
size_t hist_bytes(int64_t K, int32_t n_bins, int32_t B, int32_t channels)
{
    return (size_t)K * (size_t)n_bins * (size_t)B * (size_t)channels * sizeof(uint64_t);
}
size_t weight_bytes(int32_t n_bins, int32_t B)
{
    return (size_t)n_bins * (size_t)B * sizeof(uint32_t);
}

// One buffer of a host-buffer call: copied up from src, down to dst, or neither
struct StagePart {
    size_t bytes;
    const void* src;
    void* dst;
};

// The host-buffer calls: ONE device block carved into the parts, each from a 16-byte boundary; the up-copies in list order, the call's
// enqueue on the device addresses (null for a part of no bytes: an optional input left out, an output not asked for), the down-copies, one
// synchronisation.  Everything on the null stream
template <size_t N, class Enqueue>
int staged_run(const HipApi* H, const StagePart (&parts)[N], Enqueue enqueue)
{
    size_t at[N], total = 0;
    for (size_t x = 0; x < N; ++x) {
        at[x] = total;
        total += (parts[x].bytes + 15) & ~(size_t)15;
    }
    void* block = nullptr;
    HIP_TRY(H->Malloc(&block, total));
    void* d[N];
    for (size_t x = 0; x < N; ++x) d[x] = parts[x].bytes ? (char*)block + at[x] : nullptr;
    auto run = [&]() -> int {
        for (size_t x = 0; x < N; ++x)
            if (d[x] && parts[x].src) HIP_TRY(H->MemcpyAsync(d[x], parts[x].src, parts[x].bytes, hipMemcpyHostToDevice, nullptr));
        if (int rc = enqueue(d)) return rc;
        for (size_t x = 0; x < N; ++x)
            if (d[x] && parts[x].dst) HIP_TRY(H->MemcpyAsync(parts[x].dst, d[x], parts[x].bytes, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(H->StreamSynchronize(nullptr));
        return HARE_OK;
    };
    const int rc = run();
    if (rc != HARE_OK) (void)H->StreamSynchronize(nullptr);      // copies may still be in flight
    dev_free(H, block);
    return rc;
}

// what the three calls check of a histogram's shape
int hist_check_shape(const char* who, int64_t K, int32_t n_bins, int32_t B, int32_t channels)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (K < 1 || K > kMaxMapReceivers) return bad("K out of range (1 .. 65 536)");
    if (n_bins < 1) return bad("n_bins must be >= 1");
    if (B < 1 || B > kMaxBands) return bad("bands out of range (1 .. 8)");
    if (channels != 1 && channels != 4 && channels != 9 && channels != 16) return bad("channels must be 1, 4, 9 or 16");
    if ((unsigned __int128)K * (unsigned)n_bins * (unsigned)B * (unsigned)channels > ((size_t)1 << 27)) return bad("K x n_bins x bands x channels exceeds 2^27");
    return HARE_OK;
}

}  // namespace

// ---- the reduction (include/hare_hip.h, "receivers", "Reduction"; the kernel: reduce.hip)
int reduce_check_spec(const char* who, int64_t K, int32_t n_bins, int32_t B, int32_t channels, const ReduceSpec& r)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (int rc = hist_check_shape(who, K, n_bins, B, channels)) return rc;
    if (r.n_win < 0 || r.n_win > kMaxReduceWindows) return bad("n_win out of range (0 .. 16)");
    if (r.n_lev < 0 || r.n_lev > kMaxReduceLevels) return bad("n_lev out of range (0 .. 32)");
    if (r.n_win + r.n_lev < 1) return bad("nothing to compute: n_win and n_lev are both 0");
    if ((r.n_win > 0 && !r.win) || (r.n_lev > 0 && !r.levels)) return bad("null win / levels");
    for (int32_t j = 0; j < r.n_win; ++j)
        if (r.win[2 * j] < 0 || r.win[2 * j] > r.win[2 * j + 1] || r.win[2 * j + 1] > n_bins)
            return bad("window " + std::to_string(j) + " is not 0 <= lo <= hi <= n_bins");
    return HARE_OK;
}

int reduce_enqueue(const Scene& s, const HipApi* H, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist,
                   const void* d_weight, const ReduceSpec& r, void* d_sums, void* d_cross, hipStream_t st)
{
    if (!s.module || !s.module->hist_reduce) {
        set_error("hare_hist_reduce missing from code object");
        return HARE_E_STATE;
    }
    ReduceArgs a;
    memset(&a, 0, sizeof a);
    a.hist = (const unsigned long long*)d_hist;
    a.weight = (const uint32_t*)d_weight;
    a.sums = (unsigned long long*)d_sums;
    a.cross = (int32_t*)d_cross;
    a.n_bins = n_bins;
    a.bands = B;
    a.channels = channels;
    a.n_win = r.n_win;
    a.n_lev = r.n_lev;
    for (int32_t j = 0; j < 2 * r.n_win; ++j) a.win[j] = r.win[j];
    for (int32_t l = 0; l < r.n_lev; ++l) a.levels[l] = r.levels[l];
    void* args[] = {&a};
    return launch(H, s.module->hist_reduce, (unsigned)K, 256, 0, st, args);          // a workgroup per receiver
}

namespace {

struct ReduceBytes {
    size_t hist, weight, sums, cross;
};

// what both reduce calls check of their buffers, device or host, behind reduce_check_spec: none null that is used, no output on another buffer
int reduce_check_buffers(const char* who, int64_t K, int32_t n_bins, int32_t B, int32_t channels, const void* hist, const void* weight,
                         const ReduceSpec& r, const void* sums, const void* cross, ReduceBytes& z)
{
    if (!hist || (r.n_win > 0 && !sums) || (r.n_lev > 0 && !cross)) {
        set_error(std::string(who) + ": null histogram / sums / crossings");
        return HARE_E_INVALID;
    }
    const size_t KB = (size_t)K * (size_t)B;
    z = {hist_bytes(K, n_bins, B, channels), weight_bytes(n_bins, B), KB * (size_t)r.n_win * 4 * sizeof(uint64_t), KB * (size_t)r.n_lev * sizeof(int32_t)};
    if (spans_overlap({{sums, z.sums}, {cross, z.cross}, {hist, z.hist}, {weight, z.weight}}, 2)) {
        set_error(std::string(who) + ": sums and crossings must not overlap each other, the histogram or the weights");
        return HARE_E_INVALID;
    }
    return HARE_OK;
}

// ---- the projection (include/hare_hip.h, "receivers", "Projection"; the kernel: project.hip)
struct ProjectBytes {
    size_t hist, weight, coef, proj;
};

// everything the project calls check before anything runs, in the header's order; buffers device or host.  out_channels: 1 for the
// projection of W, `channels` for the directional projection, whose output holds every channel
int project_check(const char* who, int64_t K, int32_t n_bins, int32_t B, int32_t channels, const void* hist, const void* weight, int32_t J,
                  const void* coef, const void* proj, int32_t out_channels, ProjectBytes& z)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (int rc = hist_check_shape(who, K, n_bins, B, channels)) return rc;
    if (J < 1 || J > kMaxProjectVectors) return bad("J out of range (1 .. 32)");
    if (!hist || !coef || !proj) return bad("null histogram / coefficients / output");
    z = {hist_bytes(K, n_bins, B, channels), weight_bytes(n_bins, B), (size_t)J * (size_t)n_bins * sizeof(int32_t),
         (size_t)K * (size_t)B * (size_t)J * (size_t)out_channels * 2 * sizeof(uint64_t)};
    if (spans_overlap({{proj, z.proj}, {hist, z.hist}, {weight, z.weight}, {coef, z.coef}}, 1))
        return bad("the output must not overlap the histogram, the weights or the coefficients");
    return HARE_OK;
}

int project_enqueue(const Scene& s, const HipApi* H, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                    int32_t J, const void* d_coef, void* d_proj, hipStream_t st)
{
    if (!s.module || !s.module->hist_project) {
        set_error("hare_hist_project missing from code object");
        return HARE_E_STATE;
    }
    ProjectArgs a;
    memset(&a, 0, sizeof a);
    a.hist = (const unsigned long long*)d_hist;
    a.weight = (const uint32_t*)d_weight;
    a.coef = (const int32_t*)d_coef;
    a.proj = (unsigned long long*)d_proj;
    a.n_bins = n_bins;
    a.bands = B;
    a.channels = channels;
    a.n_vec = J;
    void* args[] = {&a};
    return launch(H, s.module->hist_project, (unsigned)K, 256, 0, st, args);         // a workgroup per receiver
}

// ---- the directional projection (include/hare_hip.h, "receivers", "Directional projection"; the kernel: project_channels.hip): the
// projection's checks (project_check with out_channels = channels) and one launch with the projection's arguments
int project_channels_enqueue(const Scene& s, const HipApi* H, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist,
                             const void* d_weight, int32_t J, const void* d_coef, void* d_proj, hipStream_t st)
{
    if (!s.module || !s.module->hist_project_channels) {
        set_error("hare_hist_project_channels missing from code object");
        return HARE_E_STATE;
    }
    ProjectArgs a;
    memset(&a, 0, sizeof a);
    a.hist = (const unsigned long long*)d_hist;
    a.weight = (const uint32_t*)d_weight;
    a.coef = (const int32_t*)d_coef;
    a.proj = (unsigned long long*)d_proj;
    a.n_bins = n_bins;
    a.bands = B;
    a.channels = channels;
    a.n_vec = J;
    void* args[] = {&a};
    return launch(H, s.module->hist_project_channels, (unsigned)K, 256, 0, st, args);         // a workgroup per receiver
}

// ---- the rendering (include/hare_hip.h, "receivers", "Rendering"; the kernel: render.hip)
struct RenderBytes {
    size_t hist, weight, taps, out;
};

// everything both render calls check before anything runs, in the header's order; buffers device or host
int render_check(const char* who, int64_t K, int32_t n_bins, int32_t B, int32_t channels, const void* hist, const void* weight, int32_t frac_bits,
                 int32_t M, int32_t T, const void* taps, const void* out, RenderBytes& z)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (int rc = hist_check_shape(who, K, n_bins, B, channels)) return rc;
    if (M < 1 || M > kMaxRenderBin) return bad("M out of range (1 .. 1024)");
    if (T < 1 || T > kMaxRenderTaps) return bad("T out of range (1 .. 1024)");
    if (frac_bits < 0 || frac_bits > 62) return bad("frac_bits out of range (0 .. 62)");
    if ((unsigned __int128)K * (unsigned)channels * (unsigned)n_bins * (unsigned)M > ((size_t)1 << 28)) return bad("K x channels x n_bins x M exceeds 2^28");
    if (!hist || !taps || !out) return bad("null histogram / taps / output");
    z = {hist_bytes(K, n_bins, B, channels), weight_bytes(n_bins, B), (size_t)B * (size_t)T * sizeof(double),
         (size_t)K * (size_t)channels * (size_t)n_bins * (size_t)M * sizeof(double)};
    if (spans_overlap({{out, z.out}, {hist, z.hist}, {weight, z.weight}, {taps, z.taps}}, 1))
        return bad("the output must not overlap the histogram, the weights or the taps");
    return HARE_OK;
}

// The tile of hare_hist_render (render.hip): whole bins, as many as keep the B x S filtered samples near 32 KiB and the gains within
// 16 KiB -- one bin where a bin alone is more.  LDS: taps, samples, gains, a, sign mask: at most 8 * (8192 + 8192 + 2048 + 256 + 35) bytes
unsigned render_plan(RenderArgs& a)
{
    const int32_t B = a.bands, C = a.channels;
    a.tile_bins = std::max<int32_t>(1, std::min<int32_t>({(4096 / B) / a.M, 2048 / (B * C), a.n_bins}));
    a.tiles = (a.n_bins + a.tile_bins - 1) / a.tile_bins;
    const int32_t S = a.tile_bins * a.M;
    a.sign_words = ((S + a.T + kRenderRun + 62) >> 6) + 2;
    return (unsigned)(sizeof(double) * (size_t)(B * a.T + B * S + a.tile_bins * B * C + a.tile_bins * B + a.sign_words));
}

int render_enqueue(const Scene& s, const HipApi* H, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                   int32_t frac_bits, int32_t M, int32_t T, const void* d_taps, uint64_t seed, void* d_out, hipStream_t st)
{
    if (!s.module || !s.module->hist_render) {
        set_error("hare_hist_render missing from code object");
        return HARE_E_STATE;
    }
    RenderArgs a;
    memset(&a, 0, sizeof a);
    a.hist = (const unsigned long long*)d_hist;
    a.weight = (const uint32_t*)d_weight;
    a.taps = (const double*)d_taps;
    a.out = (double*)d_out;
    a.seed = seed;
    a.n_bins = n_bins;
    a.bands = B;
    a.channels = channels;
    a.frac_bits = frac_bits;
    a.M = M;
    a.T = T;
    const unsigned lds = render_plan(a);
    void* args[] = {&a};
    return launch(H, s.module->hist_render, (unsigned)K * (unsigned)a.tiles, kRenderThreads, lds, st, args);      // K x n_bins <= 2^27 workgroups
}

// ---- the impulses (include/hare_hip.h, "receivers", "Impulses"; the kernel: impulses.hip)
struct ImpulseBytes {
    size_t hist, weight, taps, out;
};

// everything both impulse calls check before anything runs, in the header's order; buffers device or host
int impulses_check(const char* who, int64_t K, int32_t n_bins, int32_t B, int32_t channels, const void* hist, const void* weight, int32_t frac_bits,
                   int32_t T, const void* taps, int64_t n0, int64_t n_out, int64_t out_stride, int32_t add, const void* out, ImpulseBytes& z)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (int rc = hist_check_shape(who, K, n_bins, B, channels)) return rc;
    if (T < 1 || T > kMaxRenderTaps) return bad("T out of range (1 .. 1024)");
    if (frac_bits < 0 || frac_bits > 62) return bad("frac_bits out of range (0 .. 62)");
    const int64_t total = (int64_t)n_bins + T - 1;
    if (n0 < 0 || n_out < 1 || n0 > total || n_out > total - n0) return bad("the window is not 0 <= n0, 1 <= n_out, n0 + n_out <= n_bins + T - 1");
    if (out_stride < n_out) return bad("out_stride must be >= n_out");
    if ((unsigned __int128)K * (unsigned)channels * (unsigned __int128)out_stride > ((size_t)1 << 28)) return bad("K x channels x out_stride exceeds 2^28");
    if (add != 0 && add != 1) return bad("add must be 0 or 1");
    if (!hist || !taps || !out) return bad("null histogram / taps / output");
    z = {hist_bytes(K, n_bins, B, channels), weight_bytes(n_bins, B), (size_t)B * (size_t)T * sizeof(double),
         (size_t)K * (size_t)channels * (size_t)out_stride * sizeof(double)};
    if (spans_overlap({{out, z.out}, {hist, z.hist}, {weight, z.weight}, {taps, z.taps}}, 1))
        return bad("the output must not overlap the histogram, the weights or the taps");
    return HARE_OK;
}

// The launch of hare_hist_impulses (impulses.hip): a workgroup per receiver and tile of kImpulseTile outputs, all channels; LDS: the taps,
// then the list of one chunk's entries: at most 8 * 8192 + 256 * (8 * 18 + 4) + 16 = 103 440 bytes
unsigned impulses_plan(ImpulseArgs& a)
{
    a.tiles = (a.n_out + kImpulseTile - 1) / kImpulseTile;
    return (unsigned)(sizeof(double) * (size_t)(a.bands * a.T) + (size_t)impulse_list_bytes(a.channels));
}

int impulses_enqueue(const Scene& s, const HipApi* H, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                     int32_t frac_bits, int32_t T, const void* d_taps, int64_t n0, int64_t n_out, int64_t out_stride, int32_t add, void* d_out,
                     hipStream_t st)
{
    if (!s.module || !s.module->hist_impulses) {
        set_error("hare_hist_impulses missing from code object");
        return HARE_E_STATE;
    }
    ImpulseArgs a;
    memset(&a, 0, sizeof a);
    a.hist = (const unsigned long long*)d_hist;
    a.weight = (const uint32_t*)d_weight;
    a.taps = (const double*)d_taps;
    a.out = (double*)d_out;
    a.out_stride = out_stride;
    a.n_bins = n_bins;
    a.bands = B;
    a.channels = channels;
    a.frac_bits = frac_bits;
    a.T = T;
    a.n0 = (int32_t)n0;
    a.n_out = (int32_t)n_out;
    a.add = add;
    const unsigned lds = impulses_plan(a);
    void* args[] = {&a};
    return launch(H, s.module->hist_impulses, (unsigned)K * (unsigned)a.tiles, kImpulseThreads, lds, st, args);      // K x tiles <= 2^20 + 2^16 workgroups
}

// ---- the convolution (include/hare_hip.h, "receivers", "Convolution"; the kernel: convolve.hip)
struct ConvolveBytes {
    size_t ir, x, y;
};

// everything both convolve calls check before anything runs, in the header's order; buffers device or host
int convolve_check(const char* who, int64_t R, int64_t N, const void* ir, int64_t L, const void* x, int64_t n0, int64_t n_out, const void* y,
                   ConvolveBytes& z)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (R < 1 || R > ((int64_t)1 << 20)) return bad("R out of range (1 .. 2^20)");
    if (N < 1 || N > ((int64_t)1 << 24)) return bad("N out of range (1 .. 2^24)");
    if (L < 1 || L > ((int64_t)1 << 28)) return bad("L out of range (1 .. 2^28)");
    if (n0 < 0 || n_out < 1 || n0 > N + L - 1 || n_out > N + L - 1 - n0) return bad("the window is not 0 <= n0, 1 <= n_out, n0 + n_out <= N + L - 1");
    if (R * n_out > ((int64_t)1 << 28)) return bad("R x n_out exceeds 2^28");
    if ((unsigned __int128)(R * n_out) * (unsigned __int128)std::min(N, L) > (unsigned __int128)HARE_CONVOLVE_MAX_TERMS)
        return bad("R x n_out x min(N, L) exceeds the work cap HARE_CONVOLVE_MAX_TERMS: split the output window");
    if (!ir || !x || !y) return bad("null ir / x / y");
    z = {(size_t)R * (size_t)N * sizeof(double), (size_t)L * sizeof(double), (size_t)R * (size_t)n_out * sizeof(double)};
    if (spans_overlap({{y, z.y}, {ir, z.ir}, {x, z.x}}, 1)) return bad("y must not overlap ir or x");
    return HARE_OK;
}

// The launch of hare_convolve (convolve.hip): a workgroup per row and tile of kConvolveTile outputs; LDS: a chunk of taps and the padded
// segment of x it meets, the same for every shape
unsigned convolve_plan(ConvolveArgs& a)
{
    a.tiles = (a.n_out + kConvolveTile - 1) / kConvolveTile;
    return (unsigned)(sizeof(double) * (size_t)kConvolveLdsDoubles);
}

int convolve_enqueue(const Scene& s, const HipApi* H, int64_t R, int64_t N, const void* d_ir, int64_t L, const void* d_x, int64_t n0, int64_t n_out,
                     void* d_y, hipStream_t st)
{
    if (!s.module || !s.module->convolve) {
        set_error("hare_convolve missing from code object");
        return HARE_E_STATE;
    }
    ConvolveArgs a;
    memset(&a, 0, sizeof a);
    a.ir = (const double*)d_ir;
    a.x = (const double*)d_x;
    a.y = (double*)d_y;
    a.N = (int32_t)N;
    a.L = (int32_t)L;
    a.n0 = (int32_t)n0;
    a.n_out = (int32_t)n_out;
    const unsigned lds = convolve_plan(a);
    void* args[] = {&a};
    return launch(H, s.module->convolve, (unsigned)R * (unsigned)a.tiles, kConvolveThreads, lds, st, args);      // R x tiles <= 2^20 + 2^17 workgroups
}

// ---- the decoding (include/hare_hip.h, "receivers", "Decoding"; the kernel: decode.hip)
struct DecodeBytes {
    size_t in, h, y;
};

// everything both decode calls check before anything runs, in the header's order; buffers device or host
int decode_check(const char* who, int64_t K, int64_t C, int64_t N, const void* in, int64_t O, int64_t T, const void* h, int64_t n0, int64_t n_out,
                 const void* y, DecodeBytes& z)
{
    auto bad = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return HARE_E_INVALID;
    };
    if (K < 1 || K > 65536) return bad("K out of range (1 .. 65536)");
    if (C < 1 || C > 64) return bad("C out of range (1 .. 64)");
    if (O < 1 || O > 64) return bad("O out of range (1 .. 64)");
    if (N < 1 || N > ((int64_t)1 << 24)) return bad("N out of range (1 .. 2^24)");
    if (T < 1 || T > ((int64_t)1 << 16)) return bad("T out of range (1 .. 2^16)");
    if (n0 < 0 || n_out < 1 || n0 > N + T - 1 || n_out > N + T - 1 - n0) return bad("the window is not 0 <= n0, 1 <= n_out, n0 + n_out <= N + T - 1");
    if (K * C * N > ((int64_t)1 << 28)) return bad("K x C x N exceeds 2^28");
    if (K * O * n_out > ((int64_t)1 << 28)) return bad("K x O x n_out exceeds 2^28");
    if ((unsigned __int128)(K * O * n_out) * (unsigned __int128)(C * std::min(N, T)) > (unsigned __int128)HARE_DECODE_MAX_TERMS)
        return bad("K x O x n_out x C x min(N, T) exceeds the work cap HARE_DECODE_MAX_TERMS: split the output window");
    if (!in || !h || !y) return bad("null in / h / y");
    z = {(size_t)(K * C * N) * sizeof(double), (size_t)(O * C * T) * sizeof(double), (size_t)(K * O * n_out) * sizeof(double)};
    if (spans_overlap({{y, z.y}, {in, z.in}, {h, z.h}}, 1)) return bad("y must not overlap in or h");
    return HARE_OK;
}

// The launch of hare_decode (decode.hip): a workgroup per (k, o) and tile of kDecodeTile outputs; LDS: a chunk of a filter's taps and the
// padded segment of in[k, c] it meets, the same for every shape
unsigned decode_plan(DecodeArgs& a)
{
    a.tiles = (a.n_out + kDecodeTile - 1) / kDecodeTile;
    return (unsigned)(sizeof(double) * (size_t)kDecodeLdsDoubles);
}

int decode_enqueue(const Scene& s, const HipApi* H, int64_t K, int64_t C, int64_t N, const void* d_in, int64_t O, int64_t T, const void* d_h, int64_t n0,
                   int64_t n_out, void* d_y, hipStream_t st)
{
    if (!s.module || !s.module->decode) {
        set_error("hare_decode missing from code object");
        return HARE_E_STATE;
    }
    DecodeArgs a;
    memset(&a, 0, sizeof a);
    a.in = (const double*)d_in;
    a.h = (const double*)d_h;
    a.y = (double*)d_y;
    a.C = (int32_t)C;
    a.O = (int32_t)O;
    a.N = (int32_t)N;
    a.T = (int32_t)T;
    a.n0 = (int32_t)n0;
    a.n_out = (int32_t)n_out;
    const unsigned lds = decode_plan(a);
    void* args[] = {&a};
    return launch(H, s.module->decode, (unsigned)(K * O) * (unsigned)a.tiles, kDecodeThreads, lds, st, args);      // K x O x tiles <= 2^22 + 2^17 workgroups
}

}  // namespace

}  // namespace hare

using namespace hare;

extern "C" {

int hare_hist_reduce_device(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                            int32_t n_win, const int32_t* win, int32_t n_lev, const uint32_t* levels, void* d_sums, void* d_cross, void* stream)
{
    if (!s) return null_scene();
    const ReduceSpec r = {nullptr, n_win, win, n_lev, levels};
    ReduceBytes z;
    if (int rc = reduce_check_spec("hare_hist_reduce_device", K, n_bins, B, channels, r)) return rc;
    if (int rc = reduce_check_buffers("hare_hist_reduce_device", K, n_bins, B, channels, d_hist, d_weight, r, d_sums, d_cross, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        return reduce_enqueue(*s, H, K, n_bins, B, channels, d_hist, d_weight, r, d_sums, d_cross, (hipStream_t)stream);
    });
}

int hare_hist_reduce(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t* hist, const uint32_t* weight,
                     int32_t n_win, const int32_t* win, int32_t n_lev, const uint32_t* levels, uint64_t* sums, int32_t* cross)
{
    if (!s) return null_scene();
    const ReduceSpec r = {weight, n_win, win, n_lev, levels};
    ReduceBytes z;
    if (int rc = reduce_check_spec("hare_hist_reduce", K, n_bins, B, channels, r)) return rc;
    if (int rc = reduce_check_buffers("hare_hist_reduce", K, n_bins, B, channels, hist, weight, r, sums, cross, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.hist, hist, nullptr}, {z.sums, nullptr, sums}, {z.cross, nullptr, cross}, {weight ? z.weight : 0, weight, nullptr}};
        return staged_run(H, parts, [&](void* const* d) { return reduce_enqueue(*s, H, K, n_bins, B, channels, d[0], d[3], r, d[1], d[2], nullptr); });
    });
}

int hare_hist_project_device(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                             int32_t J, const void* d_coef, void* d_proj, void* stream)
{
    if (!s) return null_scene();
    ProjectBytes z;
    if (int rc = project_check("hare_hist_project_device", K, n_bins, B, channels, d_hist, d_weight, J, d_coef, d_proj, 1, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        return project_enqueue(*s, H, K, n_bins, B, channels, d_hist, d_weight, J, d_coef, d_proj, (hipStream_t)stream);
    });
}

int hare_hist_project(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t* hist, const uint32_t* weight,
                      int32_t J, const int32_t* coef, uint64_t* proj)
{
    if (!s) return null_scene();
    ProjectBytes z;
    if (int rc = project_check("hare_hist_project", K, n_bins, B, channels, hist, weight, J, coef, proj, 1, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.hist, hist, nullptr}, {z.proj, nullptr, proj}, {z.coef, coef, nullptr}, {weight ? z.weight : 0, weight, nullptr}};
        return staged_run(H, parts, [&](void* const* d) { return project_enqueue(*s, H, K, n_bins, B, channels, d[0], d[3], J, d[2], d[1], nullptr); });
    });
}

int hare_hist_project_channels_device(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist,
                                      const void* d_weight, int32_t J, const void* d_coef, void* d_proj, void* stream)
{
    if (!s) return null_scene();
    ProjectBytes z;
    if (int rc = project_check("hare_hist_project_channels_device", K, n_bins, B, channels, d_hist, d_weight, J, d_coef, d_proj, channels, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        return project_channels_enqueue(*s, H, K, n_bins, B, channels, d_hist, d_weight, J, d_coef, d_proj, (hipStream_t)stream);
    });
}

int hare_hist_project_channels(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t* hist,
                               const uint32_t* weight, int32_t J, const int32_t* coef, uint64_t* proj)
{
    if (!s) return null_scene();
    ProjectBytes z;
    if (int rc = project_check("hare_hist_project_channels", K, n_bins, B, channels, hist, weight, J, coef, proj, channels, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.hist, hist, nullptr}, {z.proj, nullptr, proj}, {z.coef, coef, nullptr}, {weight ? z.weight : 0, weight, nullptr}};
        return staged_run(H, parts, [&](void* const* d) {
            return project_channels_enqueue(*s, H, K, n_bins, B, channels, d[0], d[3], J, d[2], d[1], nullptr);
        });
    });
}

int hare_hist_render_device(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                            int32_t frac_bits, int32_t M, int32_t T, const void* d_taps, uint64_t seed, void* d_out, void* stream)
{
    if (!s) return null_scene();
    RenderBytes z;
    if (int rc = render_check("hare_hist_render_device", K, n_bins, B, channels, d_hist, d_weight, frac_bits, M, T, d_taps, d_out, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        return render_enqueue(*s, H, K, n_bins, B, channels, d_hist, d_weight, frac_bits, M, T, d_taps, seed, d_out, (hipStream_t)stream);
    });
}

int hare_hist_render(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t* hist, const uint32_t* weight,
                     int32_t frac_bits, int32_t M, int32_t T, const double* taps, uint64_t seed, double* out)
{
    if (!s) return null_scene();
    RenderBytes z;
    if (int rc = render_check("hare_hist_render", K, n_bins, B, channels, hist, weight, frac_bits, M, T, taps, out, z)) return rc;
    for (size_t x = 0; x < (size_t)B * (size_t)T; ++x)
        if (!std::isfinite(taps[x])) {
            set_error("hare_hist_render: taps[" + std::to_string(x) + "] is not finite");
            return HARE_E_INVALID;
        }
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.out, nullptr, out}, {z.hist, hist, nullptr}, {z.taps, taps, nullptr}, {weight ? z.weight : 0, weight, nullptr}};
        return staged_run(H, parts, [&](void* const* d) {
            return render_enqueue(*s, H, K, n_bins, B, channels, d[1], d[3], frac_bits, M, T, d[2], seed, d[0], nullptr);
        });
    });
}

int hare_hist_impulses_device(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const void* d_hist, const void* d_weight,
                              int32_t frac_bits, int32_t T, const void* d_taps, int64_t n0, int64_t n_out, int64_t out_stride, int32_t add, void* d_out,
                              void* stream)
{
    if (!s) return null_scene();
    ImpulseBytes z;
    if (int rc = impulses_check("hare_hist_impulses_device", K, n_bins, B, channels, d_hist, d_weight, frac_bits, T, d_taps, n0, n_out, out_stride, add,
                                d_out, z))
        return rc;
    return device_call(*s, [&](const HipApi* H) {
        return impulses_enqueue(*s, H, K, n_bins, B, channels, d_hist, d_weight, frac_bits, T, d_taps, n0, n_out, out_stride, add, d_out,
                                (hipStream_t)stream);
    });
}

int hare_hist_impulses(hare_scene* s, int32_t K, int32_t n_bins, int32_t B, int32_t channels, const uint64_t* hist, const uint32_t* weight,
                       int32_t frac_bits, int32_t T, const double* taps, int64_t n0, int64_t n_out, int64_t out_stride, int32_t add, double* out)
{
    if (!s) return null_scene();
    ImpulseBytes z;
    if (int rc = impulses_check("hare_hist_impulses", K, n_bins, B, channels, hist, weight, frac_bits, T, taps, n0, n_out, out_stride, add, out, z))
        return rc;
    for (size_t x = 0; x < (size_t)B * (size_t)T; ++x)
        if (!std::isfinite(taps[x])) {
            set_error("hare_hist_impulses: taps[" + std::to_string(x) + "] is not finite");
            return HARE_E_INVALID;
        }
    // out goes up first where the device must see it: the rows it adds onto, and the words between n_out and out_stride, which come down as they went up
    const bool up = add == 1 || out_stride > n_out;
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.out, up ? out : nullptr, out}, {z.hist, hist, nullptr}, {z.taps, taps, nullptr}, {weight ? z.weight : 0, weight, nullptr}};
        return staged_run(H, parts, [&](void* const* d) {
            return impulses_enqueue(*s, H, K, n_bins, B, channels, d[1], d[3], frac_bits, T, d[2], n0, n_out, out_stride, add, d[0], nullptr);
        });
    });
}

int hare_convolve_device(hare_scene* s, int64_t R, int64_t N, const void* d_ir, int64_t L, const void* d_x, int64_t n0, int64_t n_out, void* d_y,
                         void* stream)
{
    if (!s) return null_scene();
    ConvolveBytes z;
    if (int rc = convolve_check("hare_convolve_device", R, N, d_ir, L, d_x, n0, n_out, d_y, z)) return rc;
    return device_call(*s, [&](const HipApi* H) { return convolve_enqueue(*s, H, R, N, d_ir, L, d_x, n0, n_out, d_y, (hipStream_t)stream); });
}

int hare_convolve(hare_scene* s, int64_t R, int64_t N, const double* ir, int64_t L, const double* x, int64_t n0, int64_t n_out, double* y)
{
    if (!s) return null_scene();
    ConvolveBytes z;
    if (int rc = convolve_check("hare_convolve", R, N, ir, L, x, n0, n_out, y, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.y, nullptr, y}, {z.ir, ir, nullptr}, {z.x, x, nullptr}};
        return staged_run(H, parts, [&](void* const* d) { return convolve_enqueue(*s, H, R, N, d[1], L, d[2], n0, n_out, d[0], nullptr); });
    });
}

int hare_decode_device(hare_scene* s, int64_t K, int64_t C, int64_t N, const void* d_in, int64_t O, int64_t T, const void* d_h, int64_t n0,
                       int64_t n_out, void* d_y, void* stream)
{
    if (!s) return null_scene();
    DecodeBytes z;
    if (int rc = decode_check("hare_decode_device", K, C, N, d_in, O, T, d_h, n0, n_out, d_y, z)) return rc;
    return device_call(*s, [&](const HipApi* H) { return decode_enqueue(*s, H, K, C, N, d_in, O, T, d_h, n0, n_out, d_y, (hipStream_t)stream); });
}

int hare_decode(hare_scene* s, int64_t K, int64_t C, int64_t N, const double* in, int64_t O, int64_t T, const double* h, int64_t n0, int64_t n_out,
                double* y)
{
    if (!s) return null_scene();
    DecodeBytes z;
    if (int rc = decode_check("hare_decode", K, C, N, in, O, T, h, n0, n_out, y, z)) return rc;
    return device_call(*s, [&](const HipApi* H) {
        const StagePart parts[] = {{z.y, nullptr, y}, {z.in, in, nullptr}, {z.h, h, nullptr}};
        return staged_run(H, parts, [&](void* const* d) { return decode_enqueue(*s, H, K, C, N, d[1], O, T, d[2], n0, n_out, d[0], nullptr); });
    });
}

}  // extern "C"
