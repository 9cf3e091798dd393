// image2.hip -- hare_image2_mirror, hare_image2_cands, hare_image2_paths, hare_image2_deposit, hare_image2_deposit_dir: second-order image
// sources (include/hare_hip.h, "receivers", "Image sources (second order)"), #included from kernels.hip behind image.hip, whose helpers
// (image_mirror_point, image_mirror_fill, stage_receivers, load_image, quad_v3, wave_append, poly_reflectance) and deposit.hip's
// (path_vector, deposit_tail) it shares.  Five launches per call (receive.cpp:
// image2_enqueue): the mirror writes each polygon's image S' of the source; the candidate stage finds the ordered pairs (p, q) whose second
// image S'' exists and that the prune cannot rule out, and appends (p, q, S''); the path stage finds the (receiver, candidate) triples whose
// segment S'' -> center passes through q and whose segment S' -> x2 passes through p, and appends, per triple, three shadow rays; the
// flags-only occlusion kernels of the call's partition answer them -- no traversal code here; the deposit adds the words of the paths all of
// whose legs are free.  FP64, no contraction; sqrt and / are the correctly rounded ones: bit-exact with tests/image2_ref.py.
//
// The candidate stage, polygons x polygons, is the new hot loop (10^10 ordered pairs in the 100 908-triangle hall).  Its tiling is
// image.hip's: a lane per FIRST polygon p, the second polygons q streamed past it.
//   - What is fixed per p: S' (three doubles), the bounding cone of the pyramid (apex S', base p) -- unit axis, the smallest cosine and the
//     largest sine over the corners -- and p's plane with the source's side (normal, v0, sign, |n|): 17 doubles, in registers for the lane's
//     whole life.
//   - What streams is 80 bytes per q: normal and v0 (the mirror's operands), center and radius of the bounding sphere (the prune's).  A
//     workgroup stages a tile of 256 of them in LDS (20 KiB; the bounding spheres are formed while staging) and every lane reads entry j
//     with a wave-uniform address: broadcast reads, no bank conflicts, no vector-memory traffic in the loop.
//   - The grid is (p blocks) x (q tiles).  Accepted pairs are appended with ONE atomic per wave (ballot, popcount, the leader adds).
// The prune (scene option "image2_prune") is a conservative filter in FP64 with explicit outward margins ("Image sources
// (second order)"): it never decides a result.  Every comparison is written so that a NaN or an infinity keeps the pair.
//
// The path stage, receivers x candidates: a lane per CANDIDATE, the receivers streamed through LDS, as in hare_image_pairs and for its
// reasons -- a candidate carries the larger operand (S'', S' of p, the pre-cull record of q and the origin part of the pre-cull's ray, both
// polygons' records for the exact tests), a receiver 32 bytes; and a linear call has K = 8 receivers against 10^5 .. 10^7 candidates, so a
// lane per receiver would leave most of the machine idle.  The grid is (max_cands / 256) x (receiver tiles); blocks beyond the count leave
// at once.  The FP32 pre-cull on q (tv = S'' - v0_q) runs first, the two exact tests on its survivors.

// image_mirror_fill with all 3 * max_paths shadow-ray slots and their poly_origin2; the same launch zeroes both counts
extern "C" __global__ __launch_bounds__(256) void hare_image2_mirror(Image2Args a)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (tid == 0) {
        a.count[0] = 0ull;
        a.count[1] = 0ull;
    }
    image_mirror_fill(a.d, a.sc, a.img, 3 * a.max_paths, a.sexcl2, tid, stride);
}

constexpr int kImage2Tile = 256;         // second polygons (80 B each) / receivers (32 B each) a workgroup stages in LDS
constexpr int kImage2Rec = 10;           // doubles per staged q: n, v0, sphere center, sphere radius
constexpr double kImage2Tol = 1e-9;      // the prune's relative margin: five orders above the rounding of its FP64 arithmetic

static __device__ __forceinline__ double norm3(double x, double y, double z)
{
    return sqrt((x * x + y * y) + z * z);
}

extern "C" __global__ __launch_bounds__(256) void hare_image2_cands(Image2Args a)
{
    __shared__ double qt[kImage2Tile * kImage2Rec];
    const int lane = threadIdx.x & 63;
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int q0 = (int)blockIdx.y * kImage2Tile;
    const int nq = a.sc.n_poly - q0 < kImage2Tile ? a.sc.n_poly - q0 : kImage2Tile;
    if ((int)threadIdx.x < nq) {         // stage q = q0 + threadIdx.x: the mirror's operands and the bounding sphere (centroid, farthest corner)
        const int q = q0 + (int)threadIdx.x;
        const PolyRec& pr = a.sc.polys[q];
        const double* const v3 = quad_v3(a.sc.quads, q);
        double mx = (pr.v0[0] + pr.v1[0]) + pr.v2[0], my = (pr.v0[1] + pr.v1[1]) + pr.v2[1], mz = (pr.v0[2] + pr.v1[2]) + pr.v2[2];
        if (v3) {
            mx = (mx + v3[0]) / 4.0;
            my = (my + v3[1]) / 4.0;
            mz = (mz + v3[2]) / 4.0;
        } else {
            mx = mx / 3.0;
            my = my / 3.0;
            mz = mz / 3.0;
        }
        double rho = norm3(pr.v0[0] - mx, pr.v0[1] - my, pr.v0[2] - mz);
        const double r1 = norm3(pr.v1[0] - mx, pr.v1[1] - my, pr.v1[2] - mz), r2 = norm3(pr.v2[0] - mx, pr.v2[1] - my, pr.v2[2] - mz);
        rho = r1 > rho ? r1 : rho;
        rho = r2 > rho ? r2 : rho;
        if (v3) {
            const double r3 = norm3(v3[0] - mx, v3[1] - my, v3[2] - mz);
            rho = r3 > rho ? r3 : rho;
        }
        if (!(rho == rho) || !(r1 == r1) || !(r2 == r2)) rho = __builtin_inf();      // a NaN corner: a sphere that nothing rules out
        double* const o = qt + kImage2Rec * threadIdx.x;
        o[0] = pr.n[0]; o[1] = pr.n[1]; o[2] = pr.n[2];
        o[3] = pr.v0[0]; o[4] = pr.v0[1]; o[5] = pr.v0[2];
        o[6] = mx; o[7] = my; o[8] = mz;
        o[9] = rho;
    }
    __syncthreads();
    bool on = p < a.sc.n_poly;
    double sx, sy, sz;
    load_image(a.img, p, on, sx, sy, sz);
    if (__ballot(on) == 0ull) return;                                  // a wave without a mirrored polygon
    // ---- what the prune holds of p: the bounding cone of the pyramid (apex S', base p) and p's plane with the source's side
    bool prune = a.prune != 0 && on;
    double ax = 0, ay = 0, az = 0, cosm = 1.0, sinm = 0.0, pnx = 0, pny = 0, pnz = 0, pvx = 0, pvy = 0, pvz = 0, sgn = 0, nlen = 0, s1 = 0;
    if (prune) {
        const PolyRec& pr = a.sc.polys[p];
        const double* const v3 = quad_v3(a.sc.quads, p);
        const double nv = v3 ? 4.0 : 3.0;
        const double gx = ((pr.v0[0] + pr.v1[0]) + pr.v2[0]) + (v3 ? v3[0] : 0.0), gy = ((pr.v0[1] + pr.v1[1]) + pr.v2[1]) + (v3 ? v3[1] : 0.0),
                     gz = ((pr.v0[2] + pr.v1[2]) + pr.v2[2]) + (v3 ? v3[2] : 0.0);
        ax = gx / nv - sx;
        ay = gy / nv - sy;
        az = gz / nv - sz;
        const double la = norm3(ax, ay, az);
        prune = la > 0 && la < __builtin_inf();
        ax /= la;
        ay /= la;
        az /= la;
        auto corner = [&](const double* v) {                           // the corner's angle from the axis: its cosine and its sine
            const double ux = v[0] - sx, uy = v[1] - sy, uz = v[2] - sz;
            const double lu = norm3(ux, uy, uz);
            const double ci = dot3(ax, ay, az, ux, uy, uz) / lu;
            const double si = norm3(ay * uz - az * uy, az * ux - ax * uz, ax * uy - ay * ux) / lu;
            cosm = ci < cosm ? ci : cosm;
            sinm = si > sinm ? si : sinm;
            prune = prune && lu > 0 && lu < __builtin_inf() && ci == ci && si == si;
        };
        corner(pr.v0);
        corner(pr.v1);
        corner(pr.v2);
        if (v3) corner(v3);
        prune = prune && cosm > 1e-6;                                  // a cone of less than a right angle, or no prune for this p
        pnx = pr.n[0]; pny = pr.n[1]; pnz = pr.n[2];
        pvx = pr.v0[0]; pvy = pr.v0[1]; pvz = pr.v0[2];
        sgn = dot3(a.d.pos[0] - pvx, a.d.pos[1] - pvy, a.d.pos[2] - pvz, pnx, pny, pnz) > 0 ? 1.0 : -1.0;
        nlen = norm3(pnx, pny, pnz);
        s1 = (fabs(sx) + fabs(sy)) + fabs(sz);
    }
    for (int j = 0; j < nq; ++j) {
        const double* const e = qt + kImage2Rec * j;                   // wave-uniform: broadcast reads
        const double nx = e[0], ny = e[1], nz = e[2], vx = e[3], vy = e[4], vz = e[5];
        const int q = q0 + j;
        bool acc = false;
        double h2 = 0, nn = 0;
        if (on && q != p) {
            h2 = dot3(sx - vx, sy - vy, sz - vz, nx, ny, nz);
            nn = dot3(nx, ny, nz, nx, ny, nz);
            acc = nn > 0 && (h2 > 0 || h2 < 0);
            if (acc && prune) {
                const double mx = e[6], my = e[7], mz = e[8], rho = e[9];
                const double wx = mx - sx, wy = my - sy, wz = mz - sz;
                const double tol = kImage2Tol * ((s1 + ((fabs(mx) + fabs(my)) + fabs(mz))) + rho);
                // (1) the sphere against the cone: its center's distance from the cone is at least s cos - c sin (s, c: across and along the axis)
                const double c = dot3(wx, wy, wz, ax, ay, az);
                const double s = norm3(wy * az - wz * ay, wz * ax - wx * az, wx * ay - wy * ax);
                const bool out_cone = c >= 0 && (s * cosm - c * sinm) > rho + tol;
                // (2) the sphere against p's plane: wholly on the side away from the source (where S' lies), no x2 lies in it
                const double dpl = sgn * dot3(mx - pvx, my - pvy, mz - pvz, pnx, pny, pnz);
                const bool out_side = dpl + rho * nlen < -(tol * nlen);
                acc = !(out_cone || out_side);
            }
        }
        wave_append(acc, &a.count[0], lane, [&](unsigned long long slot) {
            if (slot >= (unsigned long long)a.max_cands) return;        // beyond the list: counted, not written (then nothing is deposited)
            const double k2 = (2.0 * h2) / nn;
            double* const o = a.cand_s + 3 * slot;
            o[0] = sx - nx * k2;
            o[1] = sy - ny * k2;
            o[2] = sz - nz * k2;
            a.cand_pq[2 * slot] = p;
            a.cand_pq[2 * slot + 1] = q;
        });
    }
}

extern "C" __global__ __launch_bounds__(256) void hare_image2_paths(Image2Args a)
{
    __shared__ double rcv[kImage2Tile * 4];
    const unsigned long long found = a.count[0];
    if (found > (unsigned long long)a.max_cands) return;               // the candidate list overflowed: nothing at all is added (uniform)
    if ((unsigned long long)blockIdx.x * blockDim.x >= found) return;  // a block beyond the list (uniform)
    const int lane = threadIdx.x & 63;
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int k0 = (int)blockIdx.y * kImage2Tile;
    const int nk = a.d.n_rcv - k0 < kImage2Tile ? a.d.n_rcv - k0 : kImage2Tile;
    stage_receivers(rcv, a.d.rcv, k0, nk);
    const bool on = i < found;
    if (__ballot(on) == 0ull) return;
    const unsigned long long ci = on ? i : 0ull;
    const int p = a.cand_pq[2 * ci], q = a.cand_pq[2 * ci + 1];
    const double sx = a.cand_s[3 * ci], sy = a.cand_s[3 * ci + 1], sz = a.cand_s[3 * ci + 2];     // S''
    const double* const im = a.img + 4 * (size_t)p;
    const V3 o1 = {im[0], im[1], im[2]};                                                            // S' of p
    CullRaw cr = cull_load(a.sc, q);
    CullRay ray = cull_ray(a.sc, sx, sy, sz, 0.0, 0.0, 0.0);            // the origin part: S'' for every receiver
    const double* const v3q = quad_v3(a.sc.quads, q);
    const double* const v3p = quad_v3(a.sc.quads, p);
    const V3 o2 = {sx, sy, sz};
    for (int j = 0; j < nk; ++j) {
        const double cx = rcv[4 * j + 0], cy = rcv[4 * j + 1], cz = rcv[4 * j + 2], rr = rcv[4 * j + 3];
        bool acc = false;
        double t1 = 0, t2 = 0, vx = 0, vy = 0, vz = 0;
        V3 x2 = {0, 0, 0}, w = {0, 0, 0};
        if (on) {
            const double d2 = path_vector(cx, cy, cz, sx, sy, sz, vx, vy, vz);
            if (d2 > rr) {
                ray.dfx = (float)vx;
                ray.dfy = (float)vy;
                ray.dfz = (float)vz;
                ray.dm = fabsf(ray.dfx) + fabsf(ray.dfy) + fabsf(ray.dfz);
                if (!cull_test(a.sc, ray, cr)) {
                    const V3 d = {vx, vy, vz};
                    if (poly_fast(a.sc.polys[q], v3q, o2, d, t2) && t2 > 0.0 && t2 < 1.0) {
                        x2.x = sx + vx * t2;
                        x2.y = sy + vy * t2;
                        x2.z = sz + vz * t2;
                        w.x = x2.x - o1.x;
                        w.y = x2.y - o1.y;
                        w.z = x2.z - o1.z;
                        acc = poly_fast(a.sc.polys[p], v3p, o1, w, t1) && t1 > 0.0 && t1 < 1.0;
                    }
                }
            }
        }
        wave_append(acc, &a.count[1], lane, [&](unsigned long long slot) {
            if (slot >= (unsigned long long)a.max_paths) return;        // beyond the list: counted, not written
            RayRec s;
            s.x = x2.x;                                             // x2 -> center, leaving q
            s.y = x2.y;
            s.z = x2.z;
            s.dx = cx - x2.x;
            s.dy = cy - x2.y;
            s.dz = cz - x2.z;
            a.d.srays[3 * slot] = s;
            s.x = o1.x + w.x * t1;                                  // x1 -> x2, leaving p, arriving on q
            s.y = o1.y + w.y * t1;
            s.z = o1.z + w.z * t1;
            s.dx = x2.x - s.x;
            s.dy = x2.y - s.y;
            s.dz = x2.z - s.z;
            a.d.srays[3 * slot + 1] = s;
            s.dx = a.d.pos[0] - s.x;                                  // x1 -> source, leaving p
            s.dy = a.d.pos[1] - s.y;
            s.dz = a.d.pos[2] - s.z;
            a.d.srays[3 * slot + 2] = s;
            a.d.stmax[3 * slot] = 1.0;
            a.d.stmax[3 * slot + 1] = 1.0;
            a.d.stmax[3 * slot + 2] = 1.0;
            a.d.sexcl[3 * slot] = q;
            a.d.sexcl[3 * slot + 1] = p;
            a.d.sexcl[3 * slot + 2] = p;
            a.sexcl2[3 * slot + 1] = q;
            a.path_kc[2 * slot] = k0 + j;
            a.path_kc[2 * slot + 1] = (int)i;
        });
    }
}

// A lane per path of the list; several paths can land in one histogram word: every add is an atomic.
template <int C>
static __device__ __forceinline__ void image2_deposit_body(const Image2Args& a)
{
    const unsigned long long found = a.count[1];
    if (a.count[0] > (unsigned long long)a.max_cands || found > (unsigned long long)a.max_paths) return;      // a list overflowed: nothing at all is added
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= found) return;
    if (a.d.socc[3 * i] != 0 || a.d.socc[3 * i + 1] != 0 || a.d.socc[3 * i + 2] != 0) return;      // a leg is occluded
    const int k = a.path_kc[2 * i];
    const size_t ci = (size_t)a.path_kc[2 * i + 1];
    const int p = a.cand_pq[2 * ci], q = a.cand_pq[2 * ci + 1];
    deposit_tail<C>(
        a.d, k, a.cand_s[3 * ci], a.cand_s[3 * ci + 1], a.cand_s[3 * ci + 2],
        [&](double& gx, double& gy, double& gz) {                       // source -> x1, the first reflection point: the origin of the middle leg
            const RayRec& s = a.d.srays[3 * i + 1];
            gx = s.x - a.d.pos[0];
            gy = s.y - a.d.pos[1];
            gz = s.z - a.d.pos[2];
        },
        [&](int b) { return poly_reflectance(a.sc, a.d.bands, p, b) * poly_reflectance(a.sc, a.d.bands, q, b); });
}

#define HARE_IMAGE2_DEPOSIT_KERNEL(SUFFIX, C)                                                   \
    extern "C" __global__ __launch_bounds__(256) void hare_image2_deposit##SUFFIX(Image2Args a) \
    {                                                                                           \
        image2_deposit_body<C>(a);                                                              \
    }
HARE_CHANNEL_FORMS(HARE_IMAGE2_DEPOSIT_KERNEL)
#undef HARE_IMAGE2_DEPOSIT_KERNEL
