// deposit.hip -- what the deterministic source paths share (direct.hip, image.hip, image2.hip), #included from kernels.hip behind
// source.hip and ahead of the three: the vector from a (mirrored) source to a receiver's center and the deposit of one path into the
// receiver's histogram (DepositArgs, hare_device.h).  No kernel here.  FP64, no contraction; sqrt and / are the correctly rounded ones:
// bit-exact with tests/direct_ref.py, image_ref.py and image2_ref.py, which share this arithmetic too.

// v = c - S and d2 = |v|^2: the same operations wherever a path's vector is formed (the direct emission, the searches, the deposits), so a
// deposit sees the bits its search saw.  S is the source, its image S' or its second image S''
static __device__ __forceinline__ double path_vector(double cx, double cy, double cz, double sx, double sy, double sz, double& vx, double& vy,
                                                     double& vz)
{
    vx = cx - sx;
    vy = cy - sy;
    vz = cz - sz;
    return (vx * vx + vy * vy) + vz * vz;
}

// One visible path from S = (sx, sy, sz) to receiver k: the detection counter and, when the arrival falls in a bin, B histogram words (4 B in
// the _dir form: the energy and its three arrival-axis moments; 9 B and 16 B in the _dir2 and _dir3 forms, the higher orders' channels of the
// same arrival vector behind them: C is the channel count).  Every add is an atomic: several paths of a call can land in one word.
//   gain_vec(gx, gy, gz): the direction in which the path leaves the source, for the directivity lookup.  It is handed v = c_k - S, which
//     the direct sound leaves as it is, and is asked only when the path is binned and the source has a table (the image deposits read a
//     shadow ray for it);
//   refl(b): the path's reflectance in band b.  The band's energy is (((power * g) * refl(b)) * fw) * scale in this association; the direct
//     sound passes the literal 1.0, a multiplication that is exact for every operand (no fast-math here) and that the compiler drops.
template <int C, class GainVec, class Refl>
static __device__ __forceinline__ void deposit_tail(const DepositArgs& a, int k, double sx, double sy, double sz, GainVec gain_vec, Refl refl)
{
    const int B = a.bands;
    const double* const rc = a.rcv + 4 * (size_t)k;
    const double rr = rc[3];
    double vx, vy, vz;
    const double d2 = path_vector(rc[0], rc[1], rc[2], sx, sy, sz, vx, vy, vz);
    const double dist = sqrt(d2);
    const double x = rr / d2;
    const double f = (0.5 * x) / (1.0 + sqrt(1.0 - x));         // (1 - cos theta) / 2 with sin^2 theta = x: the sphere's share of the solid angle
    const double fw = f * a.weight;
    const double xb = dist / a.bin_len;
    const bool binned = xb >= 0 && xb < (double)a.n_bins;
    atomicAdd(&a.det[2 * (size_t)k + (binned ? 0 : 1)], 1ull);
    if (!binned) return;
    const int bin = (int)floor(xb);
    const double* g = nullptr;                                  // null: no table, every gain 1.0
    if (a.res > 0) {
        double gx = vx, gy = vy, gz = vz;
        gain_vec(gx, gy, gz);
        g = source_gains(a.gain, a.frame, a.res, B, gx, gy, gz);
    }
    unsigned long long* const w = a.hist + ((size_t)k * (size_t)a.n_bins + (size_t)bin) * (size_t)B * C;
    [[maybe_unused]] double ax = 0, ay = 0, az = 0;
    [[maybe_unused]] double Y[kAmbiMax];
    if constexpr (C >= 4) {
        ax = -(vx / dist);
        ay = -(vy / dist);
        az = -(vz / dist);
        if constexpr (C > 4) ambi_harmonics<C>(ax, ay, az, Y);
    }
#pragma unroll
    for (int b = 0; b < kMaxBands; ++b)
        if (b < B) hist_add<C>(&w[C * b], quant_m((((a.power[b] * (g ? g[b] : 1.0)) * refl(b)) * fw) * a.scale), ax, ay, az, Y);
}
