// image.hip -- hare_image_mirror, hare_image_pairs, hare_image_deposit, hare_image_deposit_dir: first-order image sources (include/hare_hip.h,
// "receivers", "Image sources (first order)"), #included from kernels.hip behind direct.hip, whose helpers (source_gains, quant_m, dir_q) it
// shares.  Four launches per call (receive.cpp: image_enqueue): the mirror writes each polygon's image S' of the source; the pair search
// finds the (receiver, polygon) pairs whose segment S' -> center passes through the polygon and appends, per pair, the reflection point's
// two shadow rays; the flags-only occlusion kernels of the call's partition answer them -- no traversal code here; the deposit adds the
// words of the pairs both of whose legs are free.  FP64, no contraction; sqrt and / are the correctly rounded ones: bit-exact with
// tests/image_ref.py.
//
// The pair search, receivers x polygons, is the hot path.  Its tiling: a lane per POLYGON, the receivers streamed past it.
//   - What is fixed per polygon is the larger half of a pair's operands: S' (three doubles), the pre-cull's record (32 or 48 bytes) and the
//     origin part of the pre-cull's ray, tv = S' - v0 (the ray S' -> c starts at the same point for every receiver).  A lane holds them in
//     registers for its whole life (about 30 VGPRs), and the compiler hoists what cull_test forms from them out of the loop.
//   - What streams is 32 bytes per receiver (center, r * r).  A workgroup stages a tile of 256 receivers in LDS (8 KiB) once and every
//     lane reads receiver j of the tile with a wave-uniform address: one broadcast ds_read_b128 pair per pair-of-the-search per wave, no
//     bank conflicts, no vector-memory traffic in the loop at all.  The transpose (a lane per receiver, polygons streamed) would stream 32 to
//     48 bytes of record plus 32 of S' per pair and leave most of a wave idle for a call with few receivers (K = 8 is a common linear call;
//     a room has thousands of polygons).
//   - The grid is (polygon blocks) x (receiver tiles): the hall's map, 4 000 x 100 000, is 6 400 workgroups of 256 x 256 pairs.
// Each pair goes through the conservative FP32 pre-cull first (cull_load / cull_ray / cull_test, hare_device.h: it may only reject what the
// exact test rejects); the exact two-sided FP64 test (poly_fast, hare_math.h) runs on the survivors, which are about as many as the pairs
// found.  Accepted pairs are appended with ONE atomic per wave (ballot, popcount, the leader adds, the lanes take their ranks).

// v = c_k - S' and d2 = |v|^2, the same operations in the pair search and in the deposit (so the deposit sees the search's bits)
static __device__ __forceinline__ double image_vector(double cx, double cy, double cz, double sx, double sy, double sz, double& vx, double& vy,
                                                      double& vz)
{
    vx = cx - sx;
    vy = cy - sy;
    vz = cz - sz;
    return (vx * vx + vy * vy) + vz * vz;
}

// The point (sx, sy, sz) mirrored in the plane of polygon pr: o[0 .. 2] = the image, o[3] = 1.0 when mirrored, else 0.0 (a NaN, a point on the
// plane or a normal of length 0: no image).  hare_image_mirror's arithmetic, shared with image2.hip (which mirrors S' again)
static __device__ __forceinline__ bool image_mirror_point(const PolyRec& pr, double sx, double sy, double sz, double* o)
{
    const double nx = pr.n[0], ny = pr.n[1], nz = pr.n[2];
    const double h = dot3(sx - pr.v0[0], sy - pr.v0[1], sz - pr.v0[2], nx, ny, nz);
    const double nn = dot3(nx, ny, nz, nx, ny, nz);
    const bool mirrored = nn > 0 && (h > 0 || h < 0);
    const double k2 = (2.0 * h) / nn;
    o[0] = sx - nx * k2;
    o[1] = sy - ny * k2;
    o[2] = sz - nz * k2;
    o[3] = mirrored ? 1.0 : 0.0;
    return mirrored;
}

// A lane per polygon (grid-stride): S' and the mirrored mark, img[4 p .. 4 p + 3] = S'.x, S'.y, S'.z, 1.0 / 0.0.  The same launch zeroes the
// pair count and marks all 2 * max_pairs shadow-ray slots -2 (no query: the occlusion kernels skip them under HARE_SHOOT_RETIRED_RAYS), so
// the occlusion launch needs no count on the host.
extern "C" __global__ __launch_bounds__(256) void hare_image_mirror(ImageArgs a)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (tid == 0) *a.count = 0ull;
    for (long long i = tid; i < 2 * a.max_pairs; i += stride) a.sexcl[i] = -2;
    for (long long p = tid; p < (long long)a.n_poly; p += stride) {
        image_mirror_point(a.polys[p], a.pos[0], a.pos[1], a.pos[2], a.img + 4 * (size_t)p);
    }
}

constexpr int kImageTile = 256;          // receivers a workgroup stages in LDS (32 B each)

extern "C" __global__ __launch_bounds__(256) void hare_image_pairs(ImageArgs a)
{
    __shared__ double rcv[kImageTile * 4];
    const int lane = threadIdx.x & 63;
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int k0 = (int)blockIdx.y * kImageTile;
    const int nk = a.n_rcv - k0 < kImageTile ? a.n_rcv - k0 : kImageTile;
    for (int j = threadIdx.x; j < nk * 4; j += blockDim.x) rcv[j] = a.rcv[4 * (size_t)k0 + (size_t)j];
    __syncthreads();
    bool on = p < a.n_poly;
    double sx = 0, sy = 0, sz = 0;
    if (on) {
        const double* const im = a.img + 4 * (size_t)p;
        sx = im[0];
        sy = im[1];
        sz = im[2];
        on = im[3] != 0.0;
    }
    if (__ballot(on) == 0ull) return;                                  // a wave without a mirrored polygon
    const int pi = on ? p : 0;
    const bool cull = a.use_cull != 0;                                  // scene option "image_cull" (uniform)
    CullRaw cr = cull_load(a, pi);
    CullRay ray = cull_ray(a, sx, sy, sz, 0.0, 0.0, 0.0);               // the origin part: S' for every receiver
    const double* const v3 = (a.quads && a.quads[pi].nverts == 4) ? a.quads[pi].v3 : nullptr;
    const V3 o = {sx, sy, sz};
    for (int j = 0; j < nk; ++j) {
        const double cx = rcv[4 * j + 0], cy = rcv[4 * j + 1], cz = rcv[4 * j + 2], rr = rcv[4 * j + 3];
        bool acc = false;
        double t = 0, vx = 0, vy = 0, vz = 0;
        if (on) {
            const double d2 = image_vector(cx, cy, cz, sx, sy, sz, vx, vy, vz);
            if (d2 > rr) {
                bool test = true;
                if (cull) {
                    ray.dfx = (float)vx;
                    ray.dfy = (float)vy;
                    ray.dfz = (float)vz;
                    ray.dm = fabsf(ray.dfx) + fabsf(ray.dfy) + fabsf(ray.dfz);
                    test = !cull_test(a, ray, cr);
                }
                if (test) {
                    const V3 d = {vx, vy, vz};
                    acc = poly_fast(a.polys[pi], v3, o, d, t) && t > 0.0 && t < 1.0;
                }
            }
        }
        const unsigned long long m = __ballot(acc);
        if (m == 0ull) continue;                                        // the common case: no lane's polygon reflects to receiver j
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(a.count, (unsigned long long)__popcll(m));
        base = __shfl(base, leader, 64);
        if (acc) {
            const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (slot < (unsigned long long)a.max_pairs) {              // beyond the list: counted, not written (the deposit then adds nothing)
                RayRec s;
                s.x = sx + vx * t;
                s.y = sy + vy * t;
                s.z = sz + vz * t;
                s.dx = cx - s.x;
                s.dy = cy - s.y;
                s.dz = cz - s.z;
                a.srays[2 * slot] = s;
                s.dx = a.pos[0] - s.x;
                s.dy = a.pos[1] - s.y;
                s.dz = a.pos[2] - s.z;
                a.srays[2 * slot + 1] = s;
                a.stmax[2 * slot] = 1.0;
                a.stmax[2 * slot + 1] = 1.0;
                a.sexcl[2 * slot] = p;
                a.sexcl[2 * slot + 1] = p;
                a.pair_kp[2 * slot] = k0 + j;
                a.pair_kp[2 * slot + 1] = p;
            }
        }
    }
}

// A lane per pair of the list.  Several pairs can land in one histogram word (a receiver's reflections off two walls at the same
// distance; a path through an edge that two coplanar polygons share): every add is an atomic.
template <bool DIR>
static __device__ __forceinline__ void image_deposit_body(const ImageArgs& a)
{
    const unsigned long long found = *a.count;
    if (found > (unsigned long long)a.max_pairs) return;               // the list overflowed: nothing at all is added
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= found) return;
    if (a.socc[2 * i] != 0 || a.socc[2 * i + 1] != 0) return;           // a leg is occluded
    const int k = a.pair_kp[2 * i], p = a.pair_kp[2 * i + 1];
    const int B = a.bands;
    const double* const im = a.img + 4 * (size_t)p;
    const double* const rc = a.rcv + 4 * (size_t)k;
    const double rr = rc[3];
    double vx, vy, vz;
    const double d2 = image_vector(rc[0], rc[1], rc[2], im[0], im[1], im[2], vx, vy, vz);
    const double dist = sqrt(d2);
    const double y = rr / d2;
    const double f = (0.5 * y) / (1.0 + sqrt(1.0 - y));
    const double fw = f * a.weight;
    const double xb = dist / a.bin_len;
    const bool binned = xb >= 0 && xb < (double)a.n_bins;
    atomicAdd(&a.det[2 * (size_t)k + (binned ? 0 : 1)], 1ull);
    if (!binned) return;
    const int bin = (int)floor(xb);
    const RayRec& s = a.srays[2 * i];                                   // its origin: the reflection point x
    const double* const g = a.res > 0 ? source_gains(a.gain, a.frame, a.res, B, s.x - a.pos[0], s.y - a.pos[1], s.z - a.pos[2]) : nullptr;
    const double* const al = a.alpha ? a.alpha + (size_t)p * (size_t)B : nullptr;
    const double* const sg = a.sigma ? a.sigma + (size_t)p * (size_t)B : nullptr;
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
            const double r = (1.0 - (al ? al[b] : 0.0)) * (1.0 - (sg ? sg[b] : 0.0));
            const double m = quant_m((((a.power[b] * (g ? g[b] : 1.0)) * r) * fw) * a.scale);
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

extern "C" __global__ __launch_bounds__(256) void hare_image_deposit(ImageArgs a)
{
    image_deposit_body<false>(a);
}

extern "C" __global__ __launch_bounds__(256) void hare_image_deposit_dir(ImageArgs a)
{
    image_deposit_body<true>(a);
}
