// image.hip -- hare_image_mirror, hare_image_pairs, hare_image_deposit, hare_image_deposit_dir: first-order image sources (include/hare_hip.h,
// "receivers", "Image sources (first order)"), #included from kernels.hip behind deposit.hip, whose vector (path_vector) and deposit
// (deposit_tail) it shares.  What it shares with image2.hip is here: the mirror's arithmetic and fill, the receiver tile, the image load, the
// append of the searches (wave_append) and a polygon's reflectance.  Four launches per call (receive.cpp: image_enqueue): the mirror writes each polygon's image S' of the source; the pair search
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

// The mirror kernels' body, a lane per polygon (grid-stride: lane tid of stride, which the kernel forms): S' and the mirrored mark, img[4 p .. 4 p + 3] = S'.x, S'.y, S'.z, 1.0 / 0.0.  The
// same launch marks all `slots` shadow-ray slots -2 (no query: the occlusion kernels skip them under HARE_SHOOT_RETIRED_RAYS), with
// poly_origin2 -1 where the call has a second exclusion array, so the occlusion launch needs no count on the host
static __device__ __forceinline__ void image_mirror_fill(const DepositArgs& d, const ImageScene& sc, double* img, long long slots, int32_t* sexcl2,
                                                         long long tid, long long stride)
{
    for (long long i = tid; i < slots; i += stride) {
        d.sexcl[i] = -2;
        if (sexcl2) sexcl2[i] = -1;
    }
    for (long long p = tid; p < (long long)sc.n_poly; p += stride) image_mirror_point(sc.polys[p], d.pos[0], d.pos[1], d.pos[2], img + 4 * (size_t)p);
}

// The same launch also zeroes the pair count
extern "C" __global__ __launch_bounds__(256) void hare_image_mirror(ImageArgs a)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (tid == 0) *a.count = 0ull;
    image_mirror_fill(a.d, a.sc, a.img, 2 * a.max_pairs, nullptr, tid, stride);
}

constexpr int kImageTile = 256;          // receivers a workgroup stages in LDS (32 B each)

// Receivers k0 .. k0 + nk - 1 (center, r * r) into the workgroup's tile, and the barrier behind it
static __device__ __forceinline__ void stage_receivers(double* lds, const double* rcv, int k0, int nk)
{
    for (int j = threadIdx.x; j < nk * 4; j += blockDim.x) lds[j] = rcv[4 * (size_t)k0 + (size_t)j];
    __syncthreads();
}

// S' of polygon p for a lane that is on; `on` goes off where p has no image
static __device__ __forceinline__ void load_image(const double* img, int p, bool& on, double& sx, double& sy, double& sz)
{
    sx = sy = sz = 0;
    if (on) {
        const double* const im = img + 4 * (size_t)p;
        sx = im[0];
        sy = im[1];
        sz = im[2];
        on = im[3] != 0.0;
    }
}

// The fourth corner of polygon p, null for a triangle
static __device__ __forceinline__ const double* quad_v3(const QuadRec* quads, int p)
{
    return (quads && quads[p].nverts == 4) ? quads[p].v3 : nullptr;
}

// The reflectance of polygon p in band b: (1 - alpha) (1 - sigma), a missing table counting as zeros.  The deposits ask per band, behind the
// bin test: row pointers formed ahead of deposit_tail would stay live across it (six more VGPRs in the second-order deposit)
static __device__ __forceinline__ double poly_reflectance(const ImageScene& sc, int B, int p, int b)
{
    const size_t j = (size_t)p * (size_t)B + (size_t)b;
    return (1.0 - (sc.alpha ? sc.alpha[j] : 0.0)) * (1.0 - (sc.sigma ? sc.sigma[j] : 0.0));
}

// The append of the three searches, ONE atomic per wave: the lanes that accepted are counted (ballot, popcount), the first of them adds the
// count to *counter, and each takes its rank behind the old value and hands its slot to write(slot).  The slot may lie beyond the caller's
// list (counted, not written): write tests slot < its limit.  A wave in which no lane accepted -- the common case -- leaves behind the
// ballot.  (A form that returns the slot to the caller costs the empty wave four more instructions and pairs / cands two VGPRs: the
// compiler keeps the merged "no slot" value alive instead of branching on.)
template <class Write>
static __device__ __forceinline__ void wave_append(bool acc, unsigned long long* counter, int lane, Write write)
{
    const unsigned long long m = __ballot(acc);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader, 64);
    if (acc) write(base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull)));
}

extern "C" __global__ __launch_bounds__(256) void hare_image_pairs(ImageArgs a)
{
    __shared__ double rcv[kImageTile * 4];
    const int lane = threadIdx.x & 63;
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int k0 = (int)blockIdx.y * kImageTile;
    const int nk = a.d.n_rcv - k0 < kImageTile ? a.d.n_rcv - k0 : kImageTile;
    stage_receivers(rcv, a.d.rcv, k0, nk);
    bool on = p < a.sc.n_poly;
    double sx, sy, sz;
    load_image(a.img, p, on, sx, sy, sz);
    if (__ballot(on) == 0ull) return;                                  // a wave without a mirrored polygon
    const int pi = on ? p : 0;
    const bool cull = a.use_cull != 0;                                  // scene option "image_cull" (uniform)
    CullRaw cr = cull_load(a.sc, pi);
    CullRay ray = cull_ray(a.sc, sx, sy, sz, 0.0, 0.0, 0.0);            // the origin part: S' for every receiver
    const double* const v3 = quad_v3(a.sc.quads, pi);
    const V3 o = {sx, sy, sz};
    for (int j = 0; j < nk; ++j) {
        const double cx = rcv[4 * j + 0], cy = rcv[4 * j + 1], cz = rcv[4 * j + 2], rr = rcv[4 * j + 3];
        bool acc = false;
        double t = 0, vx = 0, vy = 0, vz = 0;
        if (on) {
            const double d2 = path_vector(cx, cy, cz, sx, sy, sz, vx, vy, vz);
            if (d2 > rr) {
                bool test = true;
                if (cull) {
                    ray.dfx = (float)vx;
                    ray.dfy = (float)vy;
                    ray.dfz = (float)vz;
                    ray.dm = fabsf(ray.dfx) + fabsf(ray.dfy) + fabsf(ray.dfz);
                    test = !cull_test(a.sc, ray, cr);
                }
                if (test) {
                    const V3 d = {vx, vy, vz};
                    acc = poly_fast(a.sc.polys[pi], v3, o, d, t) && t > 0.0 && t < 1.0;
                }
            }
        }
        wave_append(acc, a.count, lane, [&](unsigned long long slot) {
            if (slot >= (unsigned long long)a.max_pairs) return;        // beyond the list: counted, not written (the deposit then adds nothing)
            RayRec s;
            s.x = sx + vx * t;
            s.y = sy + vy * t;
            s.z = sz + vz * t;
            s.dx = cx - s.x;
            s.dy = cy - s.y;
            s.dz = cz - s.z;
            a.d.srays[2 * slot] = s;
            s.dx = a.d.pos[0] - s.x;
            s.dy = a.d.pos[1] - s.y;
            s.dz = a.d.pos[2] - s.z;
            a.d.srays[2 * slot + 1] = s;
            a.d.stmax[2 * slot] = 1.0;
            a.d.stmax[2 * slot + 1] = 1.0;
            a.d.sexcl[2 * slot] = p;
            a.d.sexcl[2 * slot + 1] = p;
            a.pair_kp[2 * slot] = k0 + j;
            a.pair_kp[2 * slot + 1] = p;
        });
    }
}

// A lane per pair of the list.  Several pairs can land in one histogram word (a receiver's reflections off two walls at the same
// distance; a path through an edge that two coplanar polygons share): every add is an atomic.
template <int C>
static __device__ __forceinline__ void image_deposit_body(const ImageArgs& a)
{
    const unsigned long long found = *a.count;
    if (found > (unsigned long long)a.max_pairs) return;               // the list overflowed: nothing at all is added
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= found) return;
    if (a.d.socc[2 * i] != 0 || a.d.socc[2 * i + 1] != 0) return;       // a leg is occluded
    const int k = a.pair_kp[2 * i], p = a.pair_kp[2 * i + 1];
    const double* const im = a.img + 4 * (size_t)p;
    deposit_tail<C>(
        a.d, k, im[0], im[1], im[2],
        [&](double& gx, double& gy, double& gz) {                       // source -> x, the reflection point: the origin of the pair's shadow rays
            const RayRec& s = a.d.srays[2 * i];
            gx = s.x - a.d.pos[0];
            gy = s.y - a.d.pos[1];
            gz = s.z - a.d.pos[2];
        },
        [&](int b) { return poly_reflectance(a.sc, a.d.bands, p, b); });
}

#define HARE_IMAGE_DEPOSIT_KERNEL(SUFFIX, C)                                                  \
    extern "C" __global__ __launch_bounds__(256) void hare_image_deposit##SUFFIX(ImageArgs a) \
    {                                                                                         \
        image_deposit_body<C>(a);                                                             \
    }
HARE_CHANNEL_FORMS(HARE_IMAGE_DEPOSIT_KERNEL)
#undef HARE_IMAGE_DEPOSIT_KERNEL
