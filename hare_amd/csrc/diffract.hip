// diffract.hip -- hare_diffract_emit, hare_diffract_pairs, hare_diffract_deposit[_dir, _dir2, _dir3]: first-order edge diffraction
// (include/hare_hip.h, "receivers", "Edge diffraction (first order)"), #included from kernels.hip behind image2.hip.  It shares deposit.hip's
// vector and deposit (path_vector, deposit_tail) and image.hip's receiver tile and append (stage_receivers, wave_append).  Four launches per
// call (receive.cpp: diffract_enqueue): the emission writes each receiver's direct shadow ray as hare_direct_emit does, marks the pairs'
// slots -2 and zeroes the count; the pair search finds the (edge, receiver) pairs whose shortest path over the edge has its apex inside the
// edge and a detour within max_detour, and appends, per pair, the apex's two shadow rays; the flags-only occlusion kernels of the call's
// partition answer the direct rays and the legs in ONE query -- no traversal code here; the deposit adds the words of the pairs whose
// receiver the source does not see and both of whose legs are free.  FP64, no contraction; sqrt and / are the correctly rounded ones:
// bit-exact with tests/diffract_ref.py.
//
// The pair search, edges x receivers, is the hot path.  Its tiling is hare_image_pairs': a lane per EDGE, the receivers streamed past it.
//   - What is fixed per edge: a and e = b - a (six doubles), ee = dot(e, e), the source's foot parameter ts and its distance hs from the
//     edge's line, and the two faces: eleven doubles and two words in registers for the lane's whole life.  ts and hs do not depend on the
//     receiver, so they are formed once, by the operations the header states (no reciprocal of ee is kept: ts and tr are quotients).
//   - What streams is 32 bytes per receiver (center, r * r), from the 256-entry LDS tile with wave-uniform addresses: broadcast reads, no
//     bank conflicts, no vector-memory traffic in the loop.
//   - The grid is (edge blocks) x (receiver tiles).  Accepted pairs are appended with ONE atomic per wave.
// A pair costs two divisions and four square roots in FP64 when it runs to the end; the tests are ordered so that a pair leaves at the first
// that fails (a wave goes on while any of its lanes is still in).  The detour is not stored: the deposit forms it again from the stored
// apex by the search's own operations.

static __device__ __forceinline__ double len3(double x, double y, double z)
{
    return sqrt(dot3(x, y, z, x, y, z));
}

// The K direct rays (hare_direct_emit's, with poly_origin2 -1), the marks of the 2 max_pairs leg slots and the zeroed count
extern "C" __global__ __launch_bounds__(256) void hare_diffract_emit(DiffractArgs a)
{
    const DepositArgs& d = a.d;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (tid == 0) *a.count = 0ull;
    for (long long k = tid; k < (long long)d.n_rcv; k += stride) {
        const double* const rc = d.rcv + 4 * (size_t)k;
        double vx, vy, vz;
        const double d2 = path_vector(rc[0], rc[1], rc[2], d.pos[0], d.pos[1], d.pos[2], vx, vy, vz);
        RayRec s;
        s.x = d.pos[0]; s.y = d.pos[1]; s.z = d.pos[2];
        s.dx = vx; s.dy = vy; s.dz = vz;
        d.srays[k] = s;
        d.stmax[k] = 1.0;
        d.sexcl[k] = d2 > rc[3] ? -1 : -2;
        a.sexcl2[k] = -1;
    }
    const long long slots = (long long)d.n_rcv + 2 * a.max_pairs;
    for (long long i = (long long)d.n_rcv + tid; i < slots; i += stride) {
        d.sexcl[i] = -2;
        a.sexcl2[i] = -1;
    }
}

extern "C" __global__ __launch_bounds__(256) void hare_diffract_pairs(DiffractArgs a)
{
    __shared__ double rcv[kImageTile * 4];
    const int lane = threadIdx.x & 63;
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int k0 = (int)blockIdx.y * kImageTile;
    const int nk = a.d.n_rcv - k0 < kImageTile ? a.d.n_rcv - k0 : kImageTile;
    stage_receivers(rcv, a.d.rcv, k0, nk);
    const bool on = j < a.n_edges;
    if (__ballot(on) == 0ull) return;                                  // a wave beyond the table
    const double* const en = a.ends + 6 * (size_t)(on ? j : 0);
    const double ax = en[0], ay = en[1], az = en[2];
    const double ex = en[3] - ax, ey = en[4] - ay, ez = en[5] - az;
    const double sx = a.d.pos[0], sy = a.d.pos[1], sz = a.d.pos[2];
    const double ee = dot3(ex, ey, ez, ex, ey, ez);
    const double ts = dot3(sx - ax, sy - ay, sz - az, ex, ey, ez) / ee;
    const double hs = len3(sx - (ax + ex * ts), sy - (ay + ey * ts), sz - (az + ez * ts));
    const int f0 = a.faces[2 * (size_t)(on ? j : 0)], f1 = a.faces[2 * (size_t)(on ? j : 0) + 1];
    const size_t K = (size_t)a.d.n_rcv;
    for (int i = 0; i < nk; ++i) {
        const double cx = rcv[4 * i + 0], cy = rcv[4 * i + 1], cz = rcv[4 * i + 2], rr = rcv[4 * i + 3];
        bool acc = false;
        double px = 0, py = 0, pz = 0, wx = 0, wy = 0, wz = 0;
        if (on) {
            double vx, vy, vz;
            const double d2 = path_vector(cx, cy, cz, sx, sy, sz, vx, vy, vz);
            if (d2 > rr) {
                const double tr = dot3(cx - ax, cy - ay, cz - az, ex, ey, ez) / ee;
                const double hr = len3(cx - (ax + ex * tr), cy - (ay + ey * tr), cz - (az + ez * tr));
                const double hsum = hs + hr;
                const double t = (ts * hr + tr * hs) / hsum;
                if (hsum > 0 && t > 0 && t < 1) {
                    px = ax + ex * t;
                    py = ay + ey * t;
                    pz = az + ez * t;
                    const double ux = px - sx, uy = py - sy, uz = pz - sz;
                    wx = cx - px;
                    wy = cy - py;
                    wz = cz - pz;
                    const double ls2 = dot3(ux, uy, uz, ux, uy, uz), lr2 = dot3(wx, wy, wz, wx, wy, wz);
                    if (ls2 > 0 && lr2 > rr) {
                        const double delta = (sqrt(ls2) + sqrt(lr2)) - sqrt(d2);
                        acc = delta > 0 && delta <= a.max_detour;
                    }
                }
            }
        }
        wave_append(acc, a.count, lane, [&](unsigned long long slot) {
            if (slot >= (unsigned long long)a.max_pairs) return;        // beyond the list: counted, not written (the deposit then adds nothing)
            const size_t r = K + 2 * (size_t)slot;
            RayRec s;
            s.x = px;
            s.y = py;
            s.z = pz;
            s.dx = wx;                                                  // apex -> center
            s.dy = wy;
            s.dz = wz;
            a.d.srays[r] = s;
            s.dx = sx - px;                                             // apex -> source
            s.dy = sy - py;
            s.dz = sz - pz;
            a.d.srays[r + 1] = s;
            a.d.stmax[r] = 1.0;
            a.d.stmax[r + 1] = 1.0;
            a.d.sexcl[r] = f0;
            a.d.sexcl[r + 1] = f0;
            a.sexcl2[r] = f1;
            a.sexcl2[r + 1] = f1;
            a.pair_kj[2 * slot] = k0 + i;
            a.pair_kj[2 * slot + 1] = j;
        });
    }
}

// A lane per pair of the list.  Several pairs can land in one histogram word (a receiver behind two edges at the same path length): every add
// is an atomic.
template <int C>
static __device__ __forceinline__ void diffract_deposit_body(const DiffractArgs& a)
{
    const unsigned long long found = *a.count;
    if (found > (unsigned long long)a.max_pairs) return;               // the list overflowed: nothing at all is added
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= found) return;
    const size_t r = (size_t)a.d.n_rcv + 2 * (size_t)i;
    const int k = a.pair_kj[2 * i];
    if (a.d.socc[k] == 0) return;                                       // the source sees the center: the direct sound covers this receiver
    if (a.d.socc[r] != 0 || a.d.socc[r + 1] != 0) return;               // a leg is occluded
    // the apex and w = c - A as the search stored them; u, the lengths and the detour by the search's own operations
    const RayRec s = a.d.srays[r];
    const double sx = a.d.pos[0], sy = a.d.pos[1], sz = a.d.pos[2];
    const double ux = s.x - sx, uy = s.y - sy, uz = s.z - sz;
    const double ls = len3(ux, uy, uz), lr = len3(s.dx, s.dy, s.dz);
    const double* const rc = a.d.rcv + 4 * (size_t)k;
    double vx, vy, vz;
    const double d2 = path_vector(rc[0], rc[1], rc[2], sx, sy, sz, vx, vy, vz);
    const double delta = (ls + lr) - sqrt(d2);
    const double q = ls / lr;
    deposit_tail<C>(
        a.d, k, s.x - s.dx * q, s.y - s.dy * q, s.z - s.dz * q,        // S*: the source unfolded about the apex onto the receiver's leg
        [&](double& gx, double& gy, double& gz) {                       // source -> apex: the origin of the pair's shadow rays
            gx = ux;
            gy = uy;
            gz = uz;
        },
        [&](int b) { return 1.0 / (3.0 + 20.0 * ((2.0 * delta) * a.inv_lambda[b])); });
}

#define HARE_DIFFRACT_DEPOSIT_KERNEL(SUFFIX, C)                                                     \
    extern "C" __global__ __launch_bounds__(256) void hare_diffract_deposit##SUFFIX(DiffractArgs a) \
    {                                                                                               \
        diffract_deposit_body<C>(a);                                                                \
    }
HARE_CHANNEL_FORMS(HARE_DIFFRACT_DEPOSIT_KERNEL)
#undef HARE_DIFFRACT_DEPOSIT_KERNEL
