// direct.hip -- hare_direct_emit, hare_direct_deposit, hare_direct_deposit_dir: the direct sound (include/hare_hip.h, "receivers", "Direct
// sound"), #included from kernels.hip behind receive.hip and source.hip, whose quantising helpers (quant_m, dir_q) and cube-map lookup
// (source_gains) it shares.
//
// One lane per RECEIVER (K <= 65 536: at most 256 workgroups), three short launches per call (receive.cpp: direct_enqueue): the emission
// writes each receiver's shadow ray from the source to its center; the flags-only occlusion kernels of the call's partition answer it -- no
// traversal code here; the deposit adds the words of the receivers the source sees.  Position, power and frame are by-value arguments, as in
// hare_emit_source.  Each histogram word and each detection counter is touched by one lane of the deposit.  FP64, no contraction; sqrt and /
// are the correctly rounded ones: bit-exact with tests/direct_ref.py.

// v = c_k - pos and d2 = |v|^2 of lane k's receiver, the same operations in both kernels (so the deposit sees the emission's bits)
static __device__ __forceinline__ double direct_vector(const DirectArgs& a, int k, double& vx, double& vy, double& vz, double& rr)
{
    const double cx = a.rcv[4 * (size_t)k + 0], cy = a.rcv[4 * (size_t)k + 1], cz = a.rcv[4 * (size_t)k + 2];
    rr = a.rcv[4 * (size_t)k + 3];
    vx = cx - a.pos[0];
    vy = cy - a.pos[1];
    vz = cz - a.pos[2];
    return (vx * vx + vy * vy) + vz * vz;
}

// A slot without a query (the source inside the sphere, or a NaN) is marked -2, which the occlusion kernels skip under
// HARE_SHOOT_RETIRED_RAYS (no traversal, flag 0), as hare_rain_step marks its own
extern "C" __global__ __launch_bounds__(256) void hare_direct_emit(DirectArgs a)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= a.n_rcv) return;
    double vx, vy, vz, rr;
    const double d2 = direct_vector(a, k, vx, vy, vz, rr);
    RayRec s;
    s.x = a.pos[0]; s.y = a.pos[1]; s.z = a.pos[2];
    s.dx = vx; s.dy = vy; s.dz = vz;
    a.srays[k] = s;
    a.stmax[k] = 1.0;
    a.sexcl[k] = d2 > rr ? -1 : -2;
}

template <bool DIR>
static __device__ __forceinline__ void direct_deposit_body(const DirectArgs& a)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= a.n_rcv) return;
    if (a.sexcl[k] == -2 || a.socc[k] != 0) return;             // not eligible, or the source does not see the center
    const int B = a.bands;
    double vx, vy, vz, rr;
    const double d2 = direct_vector(a, k, vx, vy, vz, rr);
    const double dist = sqrt(d2);
    const double x = rr / d2;
    const double f = (0.5 * x) / (1.0 + sqrt(1.0 - x));         // (1 - cos theta) / 2 with sin^2 theta = x
    const double fw = f * a.weight;
    const double xb = dist / a.bin_len;
    const bool binned = xb >= 0 && xb < (double)a.n_bins;
    atomicAdd(&a.det[2 * (size_t)k + (binned ? 0 : 1)], 1ull);
    if (!binned) return;
    const int bin = (int)floor(xb);
    const double* const g = a.res > 0 ? source_gains(a.gain, a.frame, a.res, B, vx, vy, vz) : nullptr;
    unsigned long long* const w = a.hist + ((size_t)k * (size_t)a.n_bins + (size_t)bin) * (size_t)B * (DIR ? 4 : 1);
    [[maybe_unused]] double ax = 0, ay = 0, az = 0;
    if constexpr (DIR) {
        ax = -(vx / dist);
        ay = -(vy / dist);
        az = -(vz / dist);
    }
#pragma unroll
    for (int b = 0; b < kMaxBands; ++b) {
        if (b < B) {
            const double m = quant_m(((a.power[b] * (g ? g[b] : 1.0)) * fw) * a.scale);
            if constexpr (DIR) {
                atomicAdd(&w[4 * b + 0], (unsigned long long)rint(m));
                atomicAdd(&w[4 * b + 1], dir_q(m, ax));
                atomicAdd(&w[4 * b + 2], dir_q(m, ay));
                atomicAdd(&w[4 * b + 3], dir_q(m, az));
            } else {
                atomicAdd(&w[b], (unsigned long long)rint(m));
            }
        }
    }
}

extern "C" __global__ __launch_bounds__(256) void hare_direct_deposit(DirectArgs a)
{
    direct_deposit_body<false>(a);
}

extern "C" __global__ __launch_bounds__(256) void hare_direct_deposit_dir(DirectArgs a)
{
    direct_deposit_body<true>(a);
}
