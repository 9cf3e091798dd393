// source.hip -- hare_emit_source: the scene's point source (include/hare_hip.h, "receivers", "Source"), #included from kernels.hip behind
// receive.hip, whose RNG it shares (scatter_mix, scatter_u).
//
// One lane per ray: the ray's direction is drawn from the counter-based RNG at counter c = 4096 (the casts use c < 4096, so no word is
// shared with them even under equal seeds) by Marsaglia's 1972 method -- a point of the unit disc by rejection, then + - * and one sqrt:
// uniform on the sphere without trigonometry, bit-exact with tests/source_ref.py.  Only a lane that rejected loops on, drawing its words
// as it goes (about 1.27 tries per ray).  Position, power and frame are by-value arguments (scalar registers); the directivity is a
// nearest-texel cube map (6 x R x R x B doubles, band innermost: a lane's B gains are contiguous; 1.5 MiB at most, L2-resident) looked up
// in the source's frame with a compare, a select and one division per texel axis.  A lane writes 48 B of ray and 1 + B plane stores
// (consecutive lanes, consecutive doubles).  FP64, no contraction; sqrt and / are the correctly rounded ones.
// The cube-map lookup of the header's "Source": the B contiguous gains of the texel that direction d reads in the frame M (d need not be
// normalised: the texel coordinates divide by a_f).  Shared with the direct sound (direct.hip), which reads it along source -> receiver.
static __device__ __forceinline__ const double* source_gains(const double* gain, const double (&M)[9], int R, int B, double dx, double dy, double dz)
{
    const double l0 = (M[0] * dx + M[1] * dy) + M[2] * dz;
    const double l1 = (M[3] * dx + M[4] * dy) + M[5] * dz;
    const double l2 = (M[6] * dx + M[7] * dy) + M[8] * dz;
    const double a0 = fabs(l0), a1 = fabs(l1), a2 = fabs(l2);
    int f = 0;
    double af = a0;                                  // ties and NaN keep the lower index
    if (a1 > af) { f = 1; af = a1; }
    if (a2 > af) { f = 2; af = a2; }
    const double lf = f == 0 ? l0 : (f == 1 ? l1 : l2);
    const double lu = f == 0 ? l1 : (f == 1 ? l2 : l0);              // axis (f + 1) % 3
    const double lv = f == 0 ? l2 : (f == 1 ? l0 : l1);              // axis (f + 2) % 3
    const double Rd = (double)R, half = 0.5 * Rd;
    const double tu = (lu / af + 1.0) * half, tv = (lv / af + 1.0) * half;
    const int iu = tu >= 0 ? (tu < Rd ? (int)floor(tu) : R - 1) : 0;             // NaN -> 0
    const int iv = tv >= 0 ? (tv < Rd ? (int)floor(tv) : R - 1) : 0;
    const int F = 2 * f + (lf < 0 ? 1 : 0);
    return gain + ((size_t)(F * R + iv) * (size_t)R + (size_t)iu) * (size_t)B;
}

extern "C" __global__ __launch_bounds__(256) void hare_emit_source(SourceArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int B = a.bands;
    const unsigned long long base = scatter_mix(scatter_mix(a.seed + kScatterGamma) ^ (unsigned long long)(a.first_ray + i));
    const unsigned long long c8 = (unsigned long long)kSourceCounter << 8;
    double x = 0, y = 0, s = 0;
    for (unsigned t = 0; t < 32; ++t) {
        const double xt = 2.0 * scatter_u(base, c8, 1 + 2 * t) - 1.0;
        const double yt = 2.0 * scatter_u(base, c8, 2 + 2 * t) - 1.0;
        const double st = xt * xt + yt * yt;
        if (st < 1.0) {
            x = xt;
            y = yt;
            s = st;
            break;
        }
    }
    const double h = sqrt(1.0 - s);
    RayRec r;
    r.x = a.pos[0]; r.y = a.pos[1]; r.z = a.pos[2];
    r.dx = (2.0 * x) * h;
    r.dy = (2.0 * y) * h;
    r.dz = 1.0 - 2.0 * s;
    const double* const g = a.res > 0 ? source_gains(a.gain, a.frame, a.res, B, r.dx, r.dy, r.dz) : nullptr;      // null: no table, every gain 1.0
    a.rays[i] = r;
    a.state[i] = 0.0;                                // L
#pragma unroll
    for (int b = 0; b < kMaxBands; ++b)
        if (b < B) a.state[(size_t)(b + 1) * (size_t)a.n + (size_t)i] = g ? a.power[b] * g[b] : a.power[b] * 1.0;
}
