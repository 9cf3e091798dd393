// receive.hip -- the receiver step of the receive loop (include/hare_hip.h, "receivers"), #included from kernels.hip.  One body
// (receive_body) makes hare_receive_reflect, hare_receive_scatter, hare_receive_scatter_rain and the two _map kernels, each in the four
// channel forms of HARE_CHANNEL_FORMS (20 entry points): scattering, rain, the channel count and the receiver map are compile-time
// switches.  And hare_rain_step, diffuse rain's emit and deposit (rain_body, four forms).  The pieces every kernel that adds histogram
// words shares are here too: quant_m, dir_q, ambi_harmonics, hist_add, scatter_base and the form list.
//
// One lane per ray, in place of hare_reflect behind every cast of hare_receive_device's loop (receive.cpp: receive_step, which
// bounce_device_impl runs behind every cast).  A live ray reads its ray, its event and its state once; runs through every receiver sphere in ascending order with the
// FP64 test of the header (no contraction: -ffp-contract=off); updates its state; and, except in the last cast, is reflected exactly as
// hare_reflect does it (the same function, reflect_hit; the same marks and live-block byte).  A retired ray (-2) costs one 4-byte load; a
// workgroup whose rays are all retired also passes one barrier and stages no receivers.  The termination rules of the header (time limit,
// energy floor, roulette: ReceiveArgs::cut) retire a ray behind its state update with the mark and the live-block byte of a miss.
//
// The receivers (at most 256 x 32 B) are staged in LDS once per workgroup and read with wave-uniform addresses (the loop index is uniform):
// one broadcast ds_read per receiver.  (Read straight from the device array they compiled to vector loads: the atomics in the loop keep
// the compiler from proving the array unchanged, so it does not use scalar loads.)
// No pre-cull: the test is a handful of FP64 operations per receiver and the exact test decides anyway.
// Histogram adds are uint64 fixed point, so their order does not matter.  A detection is rare except in the direct sound of a burst,
// where a wave's rays that pass a receiver near the source land in one or two bins: with `aggregate` the wave sums its lanes' adds
// per distinct bin first and issues ONE atomic instruction per (receiver, bin), lanes 0 .. B-1 adding the B bands (8 B contiguous bytes).

// m_b of the header, the double that the histogram word q_b is the rint of: v = energy * 2^frac_bits; 0 unless > 0; min(., 2^63)
static __device__ __forceinline__ double quant_m(double v)
{
    if (!(v > 0)) v = 0;
    return v < 9223372036854775808.0 ? v : 9223372036854775808.0;
}

static __device__ __forceinline__ unsigned long long wave_allsum_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;  // every lane
}

// hare_receive_scatter (SCATTER): the same, and a ray that hit in a cast that is not the last chooses diffuse or specular (the counter-based
// RNG of the header, "receivers": SplitMix64's finaliser on (seed, global ray index, cast, word)), weights its band energies and, when diffuse,
// leaves along a cosine-distributed direction (Malley's method in Duff et al.'s branchless basis) instead of reflect_hit's.  Only a lane that
// went diffuse runs the rejection loop, drawing its words as it goes (about 1.27 tries).  Integer ops, + - * /, sqrt and copysign only, FP64,
// no contraction: bit-exact with tests/scatter_ref.py.  sqrt is LLVM's correctly rounded FP64 expansion (v_rsq_f64 + refinement), as numpy's.
static __device__ __forceinline__ unsigned long long scatter_mix(unsigned long long z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
constexpr unsigned long long kScatterGamma = 0x9E3779B97F4A7C15ull;
// u_j of the header: (double)(mix(base + ((c << 8) | j) * G) >> 11) * 2^-53, in [0, 1)
static __device__ __forceinline__ double scatter_u(unsigned long long base, unsigned long long c8, unsigned j)
{
    return (double)(scatter_mix(base + (c8 | (unsigned long long)j) * kScatterGamma) >> 11) * 0x1p-53;
}
// the stream of ray i of a call, the `base` of its draws: mix(mix(seed + G) ^ global ray index).  Counter-based: whoever asks for word j
// of cast c of this ray draws the same bits
template <class Args>
static __device__ __forceinline__ unsigned long long scatter_base(const Args& a, int64_t i)
{
    return scatter_mix(scatter_mix(a.seed + kScatterGamma) ^ (unsigned long long)(a.ray_base + i));
}
// the diffuse direction of a ray r that hit a polygon of normal n at e (|d_out| = |d|): the header's operations in the header's order
static __device__ __forceinline__ RayRec scatter_hit(double nx, double ny, double nz, const RayRec& r, const XEventRec& e,
                                                     unsigned long long base, unsigned long long c8)
{
    if (dot3(r.dx, r.dy, r.dz, nx, ny, nz) > 0) {          // back into the half-space the ray came from
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    double x = 0, y = 0, r2 = 0;
    for (unsigned t = 0; t < 32; ++t) {
        const double xt = 2.0 * scatter_u(base, c8, 1 + 2 * t) - 1.0;
        const double yt = 2.0 * scatter_u(base, c8, 2 + 2 * t) - 1.0;
        const double rt = xt * xt + yt * yt;
        if (rt < 1.0) {
            x = xt;
            y = yt;
            r2 = rt;
            break;
        }
    }
    const double z = sqrt(1.0 - r2);
    const double sg = copysign(1.0, nz);
    const double ia = -1.0 / (sg + nz);
    const double ib = (nx * ny) * ia;
    const double t1x = 1.0 + ((sg * nx) * nx) * ia, t1y = sg * ib, t1z = -(sg * nx);
    const double t2x = ib, t2y = sg + (ny * ny) * ia, t2z = -ny;
    const double len = sqrt((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
    RayRec o;
    o.x = e.x; o.y = e.y; o.z = e.z;
    o.dx = ((x * t1x + y * t2x) + z * nx) * len;
    o.dy = ((x * t1y + y * t2y) + z * ny) * len;
    o.dz = ((x * t1z + y * t2z) + z * nz) * len;
    return o;
}

// ---- directional receivers (HARE_RECEIVE_DIRECTIONAL; the header's "receivers", "Directional"): four words per (receiver, bin, band),
// channel innermost: W (the omni word, unchanged) and X, Y, Z, the add weighted by the unit vector towards where the sound came from, as
// int64 in two's complement.  They are added with the same wrapping uint64 adds, so every sum stays an exact integer sum.
// s_i of the header as a two's-complement word: m * a_i, 0 for NaN, clamped to +-2^62, rint
static __device__ __forceinline__ unsigned long long dir_q(double m, double ai)
{
    double v = m * ai;
    if (!(v == v)) v = 0;
    v = v > -4611686018427387904.0 ? v : -4611686018427387904.0;
    v = v < 4611686018427387904.0 ? v : 4611686018427387904.0;
    return (unsigned long long)(long long)rint(v);
}
// The wave's sums of four words per lane (W, X, Y, Z of one band) in 7 exchanges instead of 4 x 6: the first two steps halve what a lane
// holds (lanes 32.. keep Y, Z and pass W, X on; then bit 4 of the lane picks one of the two), the last four are the plain butterfly.
// Returns, in every lane, the wave's sum of channel lane >> 4.  Wrapping uint64 adds only: exact whatever the order.
static __device__ __forceinline__ unsigned long long wave_sum4_u64(unsigned long long w, unsigned long long x, unsigned long long y,
                                                                   unsigned long long z, int lane)
{
    const bool hi = (lane & 32) != 0, b4 = (lane & 16) != 0;
    unsigned long long k0 = hi ? y : w, k1 = hi ? z : x;
    k0 += __shfl_xor(hi ? w : y, 32, 64);
    k1 += __shfl_xor(hi ? x : z, 32, 64);
    unsigned long long v = (b4 ? k1 : k0) + __shfl_xor(b4 ? k0 : k1, 16, 64);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- higher orders (HARE_RECEIVE_ORDER2 / _ORDER3; the header's "receivers", "Higher orders"): C = 9 or 16 channels per (receiver, bin,
// band).  Channels 0..3 are the four above; channels 4 .. C - 1 are ACN 4 .. C - 1 in SN3D, polynomials of the arrival vector, quantised
// with dir_q like X, Y, Z.  The kernels' DIR switch is the channel count C: 1 and 4 are the kernels above, unchanged; 9 and 16 are the
// _dir2 and _dir3 forms.  The six constants are the correctly rounded doubles, written as their bits (tests/test_ambi_reference.py
// compares them with numpy.sqrt).
constexpr double kAmbiC3 = 0x1.bb67ae8584caap+0;        // sqrt(3)
constexpr double kAmbiC3h = 0x1.bb67ae8584caap-1;       // 0.5 * sqrt(3)
constexpr double kAmbiC15 = 0x1.efbdeb14f4edap+1;       // sqrt(15)
constexpr double kAmbiC15h = 0x1.efbdeb14f4edap+0;      // 0.5 * sqrt(15)
constexpr double kAmbiC58 = 0x1.94c583ada5b53p-1;       // sqrt(0.625)
constexpr double kAmbiC38 = 0x1.3988e1409212ep-1;       // sqrt(0.375)
constexpr int kAmbiMax = 12;                            // channels 4 .. 15
// Y[j] = Y_{4 + j}(x, y, z), j < C - 4: the header's operations in the header's order
template <int C>
static __device__ __forceinline__ void ambi_harmonics(double x, double y, double z, double (&Y)[kAmbiMax])
{
    const double xx = x * x, yy = y * y, zz = z * z;
    const double d = xx - yy;
    Y[0] = kAmbiC3 * (x * y);
    Y[1] = kAmbiC3 * (y * z);
    Y[2] = 1.5 * zz - 0.5;
    Y[3] = kAmbiC3 * (x * z);
    Y[4] = kAmbiC3h * d;
    if constexpr (C > 9) {
        const double f = 5.0 * zz - 1.0;
        Y[5] = kAmbiC58 * (y * (3.0 * xx - yy));
        Y[6] = kAmbiC15 * ((x * y) * z);
        Y[7] = kAmbiC38 * (y * f);
        Y[8] = z * (2.5 * zz - 1.5);
        Y[9] = kAmbiC38 * (x * f);
        Y[10] = kAmbiC15h * (z * d);
        Y[11] = kAmbiC58 * (x * (xx - 3.0 * yy));
    }
}
// The channel forms of a kernel, (name suffix, channel count C): the host names them through the same list (scene.h: kChannelSuffix).
// Every kernel that adds histogram words -- the five receive kernels, hare_rain_step and the three deposits of the source paths
// (direct.hip, image.hip, image2.hip) -- is instantiated from it
#define HARE_CHANNEL_FORMS(X) X(, 1) X(_dir, 4) X(_dir2, 9) X(_dir3, 16)
// THE band writer: a lane's own adds of the C words of one band at w (the map kernels, the naive form, the rain and the source paths add
// per lane).  Word 0 is rint(m); words 1 .. 3 are m times the arrival vector a and words 4 .. C - 1 m times its polynomials Y, through
// dir_q.  C = 1 reads neither a nor Y
template <int C>
static __device__ __forceinline__ void hist_add(unsigned long long* w, double m, double ax, double ay, double az, const double (&Y)[kAmbiMax])
{
    atomicAdd(&w[0], (unsigned long long)rint(m));
    if constexpr (C >= 4) {
        atomicAdd(&w[1], dir_q(m, ax));
        atomicAdd(&w[2], dir_q(m, ay));
        atomicAdd(&w[3], dir_q(m, az));
#pragma unroll
        for (int j = 0; j < C - 4; ++j) atomicAdd(&w[4 + j], dir_q(m, Y[j]));
    }
}
// The wave's sums of sixteen words per lane in 17 exchanges instead of 16 x 6: four steps halve what a lane holds (bit 5, 4, 3, 2 of the
// lane picks the half it keeps and passes the other on), the last two are the plain butterfly.  Returns, in every lane, the wave's sum of
// word (lane >> 2).  Wrapping uint64 adds only: exact whatever the order.  Nine channels run padded with zero words.  word(j) forms
// the lane's word j; the first step takes the words in pairs (j, 8 + j) and the scheduler is held to that order, so that eight sums
// and one pair are live, not sixteen words and what forming them takes.
template <class Word>
static __device__ __forceinline__ unsigned long long wave_sum16_u64(Word word, int lane)
{
    const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0, h3 = (lane & 8) != 0, h2 = (lane & 4) != 0;
    unsigned long long a[8], b[4], c[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned long long v0 = word(j), v1 = word(8 + j);
        a[j] = (h5 ? v1 : v0) + __shfl_xor(h5 ? v0 : v1, 32, 64);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = (h4 ? a[4 + j] : a[j]) + __shfl_xor(h4 ? a[j] : a[4 + j], 16, 64);
#pragma unroll
    for (int j = 0; j < 2; ++j) c[j] = (h3 ? b[2 + j] : b[j]) + __shfl_xor(h3 ? b[j] : b[2 + j], 8, 64);
    unsigned long long s = (h2 ? c[1] : c[0]) + __shfl_xor(h2 ? c[0] : c[1], 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    return s;
}

// ---- receiver maps (hare_scene_set_receiver_map; the header's "receivers", "Receiver maps"): the _map kernels run a ray through its
// CANDIDATES only, the receivers listed in the grid cells its segment visits, with the test, the binning and the adds of the loop above.
// The receivers (up to 65 536 x 32 B) are not staged: every lane walks its own cells and reads its own candidates with vector loads;
// the grid's offsets and items and the receivers are L2-resident (2.5 MiB at most, 8 MiB of offsets for the largest grid).  The receiver
// index is per lane, so nothing is summed over a wave: a detecting lane adds its own B (4 B) words and its own detection count.  A map's
// detections are spread over many receivers, so those adds rarely meet.
// The visit rule, operation by operation as the header states it (FP64, no contraction); every double is clamped AS A DOUBLE before it
// becomes an index (map_cell), so no conversion of a NaN or of a value out of range is left to the compiler.
static __device__ __forceinline__ int map_cell(double v, int n)      // v = floor(.): the cell index clamped to 0 .. n - 1; NaN -> 0
{
    return v >= 0 ? (v < (double)n ? (int)v : n - 1) : 0;
}
// the slab test of one axis on [t0, t1], in cell units: the grid's extent 0 .. n grown by P
static __device__ __forceinline__ void map_clip(double u, double v, int n, double P, double& t0, double& t1, bool& ok)
{
    const double lo = -P, hi = (double)n + P;
    if (v == 0) {
        ok = ok && u >= lo && u <= hi;
        return;
    }
    const double ta = (lo - u) / v, tb = (hi - u) / v;
    ok = ok && ta == ta && tb == tb;
    const double tmin = ta < tb ? ta : tb, tmax = ta < tb ? tb : ta;
    t0 = tmin > t0 ? tmin : t0;
    t1 = tmax < t1 ? tmax : t1;
}
// the cells of one axis that the points of [ts, te] come within P of
static __device__ __forceinline__ void map_range(double u, double v, double ts, double te, double P, int n, int& lo, int& hi)
{
    const double p0 = u + v * ts, p1 = u + v * te;
    const double pmin = p0 < p1 ? p0 : p1, pmax = p0 < p1 ? p1 : p0;
    lo = map_cell(floor(pmin - P), n);
    hi = map_cell(floor(pmax + P), n);
}

template <int C>
static __device__ __forceinline__ void map_receivers(const ReceiveMapArgs& a, int64_t i, const RayRec& r, double t_end, double L)
{
    const int B = a.bands;
    const double h = a.map_h, P = a.map_pad;
    const int n0 = a.map_n[0], n1 = a.map_n[1], n2 = a.map_n[2];
    const double u0 = (r.x - a.map_org[0]) / h, u1 = (r.y - a.map_org[1]) / h, u2 = (r.z - a.map_org[2]) / h;
    const double v0 = r.dx / h, v1 = r.dy / h, v2 = r.dz / h;
    double t0 = 0, t1 = t_end;
    bool ok = true;
    map_clip(u0, v0, n0, P, t0, t1, ok);
    map_clip(u1, v1, n1, P, t0, t1, ok);
    map_clip(u2, v2, n2, P, t0, t1, ok);
    if (!(ok && t0 <= t1 && t1 < __builtin_inf())) return;
    int m = 0;                                                          // the major axis: a tie goes to the lowest
    double vm = v0;
    if (fabs(v1) > fabs(vm)) { m = 1; vm = v1; }
    if (fabs(v2) > fabs(vm)) { m = 2; vm = v2; }
    if (vm == 0) return;
    const double um = m == 0 ? u0 : (m == 1 ? u1 : u2);
    const int nm = m == 0 ? n0 : (m == 1 ? n1 : n2);
    const double a0 = um + vm * t0, a1 = um + vm * t1;
    const double amin = a0 < a1 ? a0 : a1, amax = a0 < a1 ? a1 : a0;
    const int jlo = map_cell(floor(amin - P), nm), jhi = map_cell(floor(amax + P), nm);
    const double nb = (double)a.n_bins;
    for (int j = jlo; j <= jhi; ++j) {                                  // the slabs of cells along the major axis: distinct, so no cell twice
        const double fj = (double)j;
        const double tA = ((fj - P) - um) / vm, tB = (((fj + 1.0) + P) - um) / vm;
        const double tlo = tA < tB ? tA : tB, thi = tA < tB ? tB : tA;
        const double ts = tlo > t0 ? tlo : t0, te = thi < t1 ? thi : t1;
        if (!(ts <= te)) continue;
        int lo0, hi0, lo1, hi1, lo2, hi2;
        map_range(u0, v0, ts, te, P, n0, lo0, hi0);
        map_range(u1, v1, ts, te, P, n1, lo1, hi1);
        map_range(u2, v2, ts, te, P, n2, lo2, hi2);
        if (m == 0) lo0 = hi0 = j;
        if (m == 1) lo1 = hi1 = j;
        if (m == 2) lo2 = hi2 = j;
        for (int iz = lo2; iz <= hi2; ++iz)
            for (int iy = lo1; iy <= hi1; ++iy) {
                // cells lo0 .. hi0 of a row are consecutive, and so are their items: one range of the CSR
                const size_t row = ((size_t)iz * (size_t)n1 + (size_t)iy) * (size_t)n0;
                unsigned q = a.map_start[row + (size_t)lo0];
                const unsigned qe = a.map_start[row + (size_t)hi0 + 1];
                for (; q < qe; ++q) {
                    const int k = (int)a.map_items[q];
                    const double cx = a.rcv[4 * (size_t)k + 0], cy = a.rcv[4 * (size_t)k + 1], cz = a.rcv[4 * (size_t)k + 2],
                                 r2 = a.rcv[4 * (size_t)k + 3];
                    const double wx = cx - r.x, wy = cy - r.y, wz = cz - r.z;
                    const double s = ((wx * r.dx + wy * r.dy) + wz * r.dz) / ((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
                    const double qx = (r.x + r.dx * s) - cx, qy = (r.y + r.dy * s) - cy, qz = (r.z + r.dz * s) - cz;
                    if (!(s >= 0 && s < t_end && ((qx * qx + qy * qy) + qz * qz) < r2)) continue;
                    const double x = (L + s) / a.bin_len;
                    const bool binned = x >= 0 && x < nb;
                    atomicAdd(&a.det[2 * (size_t)k + (binned ? 0 : 1)], 1ull);
                    if (!binned) continue;
                    const int bin = (int)floor(x);
                    // a detection is rare beside the cells walked: the ray's energies are read here, not held through the walk, and the
                    // arrival vector is formed per detection
                    if constexpr (C >= 4) {
                        const double len = sqrt((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
                        const double ax = -(r.dx / len), ay = -(r.dy / len), az = -(r.dz / len);
                        [[maybe_unused]] double Y[kAmbiMax];                    // C > 4: per detection too, like a (nothing held through the walk)
                        if constexpr (C > 4) ambi_harmonics<C>(ax, ay, az, Y);
                        unsigned long long* const w = a.hist + ((size_t)k * (size_t)a.n_bins + (size_t)bin) * (size_t)B * C;
                        for (int b = 0; b < B; ++b) {
                            const double Eb = a.init_state ? 1.0 : a.state[(size_t)(b + 1) * (size_t)a.n + (size_t)i];
                            const double mb = quant_m(Eb * a.scale);
                            hist_add<C>(&w[C * b], mb, ax, ay, az, Y);
                        }
                    } else {
                        unsigned long long* const w = a.hist + ((size_t)k * (size_t)a.n_bins + (size_t)bin) * (size_t)B;
                        for (int b = 0; b < B; ++b) {
                            const double Eb = a.init_state ? 1.0 : a.state[(size_t)(b + 1) * (size_t)a.n + (size_t)i];
                            atomicAdd(&w[b], (unsigned long long)rint(quant_m(Eb * a.scale)));
                        }
                    }
                }
            }
    }
}

// The body of one cast, a lane per ray, in four parts.
//   1. Who takes the receiver step.  A retired ray takes none of the body.  With RAIN a ray whose last reflection was diffuse
//      (ReceiveArgs::rain_flag) skips the step: hare_rain_step has deposited that segment.  In a call with the image flags a ray whose
//      reflections so far were specular skips it too (`imaged`): those paths are the image deposits'.
//   2. The receiver step.  MAP: map_receivers, above, per lane and before the event and the energies are read.  Otherwise the linear
//      loop over the staged receivers: the header's test, a ballot, the detection counters from lane 0, and the adds of the lanes that
//      are binned.  The arrival vector (C >= 4) costs a sqrt and three divisions and, for C > 4, its polynomials, held through the loop
//      (10 or 24 VGPRs): it is formed once per ray and cast, behind the first ballot that found a binned detection.  Naive
//      (`aggregate` 0), a lane adds its own words with hist_add (C = 1: its B quantised words).  Aggregated, the wave runs one round per
//      distinct bin and sums its lanes' words first; the quantised words are formed inside the band loop, never held.  Which lane ends
//      up with which word is what differs between the channel counts:
//        C = 1   wave_allsum_u64 per band; lane b adds band b: B contiguous words, one atomic instruction;
//        C = 4   wave_sum4_u64 per band; lane 16 ch + b adds channel ch of band b: 4 B contiguous words, one instruction;
//        C > 4   wave_sum16_u64 per band; lane 4 ch + s holds channel ch and keeps bands s and s + 4: the B C contiguous words go out
//                in one pass over bands 0 .. 3 and, for B > 4, a second over bands 4 .. 7, one atomic per word per wave.
//   3. State update and termination: absorption, with SCATTER the choice (scatter_base, word 0 of this cast's counter against the row
//      mean p) and its weights, the rules of ReceiveArgs::cut, then the stores.
//   4. Reflection, marks and the live-block byte, as hare_reflect; with RAIN every reflected ray writes its flag after its choice.
template <bool SCATTER, bool RAIN = false, int C = 1, bool MAP = false, typename Args = ReceiveArgs>
static __device__ __forceinline__ void receive_body(const Args& a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int B = a.bands;
    __shared__ double rcv[kMaxReceivers * 4];                        // the receivers: uniform LDS reads (broadcast) in the loop below
                                                                     // (MAP: never referenced, so the _map kernels hold none of it)
    bool live = i < a.n;
    if (live && a.marks_valid && a.excl[i] == -2) live = false;
    // a workgroup whose 256 rays are all retired stages nothing: its rays cost their 4-byte mark and this one barrier (it still writes
    // its live-block bytes, below)
    if (!__syncthreads_or(live ? 1 : 0)) {
        if (a.block_live && lane == 0) {
            const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
            if (blk * 64 < a.n) a.block_live[blk] = 0;
        }
        return;
    }
    if constexpr (!MAP) {
        for (int k = threadIdx.x; k < a.n_rcv * 4; k += blockDim.x) rcv[k] = a.rcv[k];
        __syncthreads();
    }
    XEventRec e;
    RayRec r;
    double L = 0;
    double E[kMaxBands];
#pragma unroll
    for (int b = 0; b < kMaxBands; ++b) E[b] = 0;
    bool rained = false;
    // HARE_RECEIVE_IMAGE, cast 1 of the scatter kernels (kCutSkipSpecular, uniform): the first-order specular paths are hare_image_deposit's, so
    // a ray whose reflection behind cast 0 was specular -- !(u_0 < p) at c = 0 for the polygon it is leaving, its mark -- runs no receiver step
    bool imaged = false;
    if constexpr (SCATTER) {
        if ((a.cut & kCutSkipSpecular) && live && a.excl[i] >= 0) {
            const double* sg = a.sigma + (size_t)a.excl[i] * (size_t)B;
            double p = sg[0];
            for (int b = 1; b < B; ++b) p = p + sg[b];
            p = p / (double)B;
            imaged = !(scatter_u(scatter_base(a, i), 0ull, 0) < p);
        }
    }
    // HARE_RECEIVE_IMAGE2 (uniform bits; the scatter kernels).  Cast 1 stores the byte HERE, from cast 0's outcome and this cast's own draw,
    // which it makes a second time for the purpose -- the draw is counter-based, so these are the bits the reflection below draws (same p,
    // same word 0 of counter c = 1).  Nothing is held across the body and nothing is stored behind the reflection: a store there cost
    // hare_receive_scatter_map_dir four VGPRs, and the second draw runs in one cast of a flagged call only.  A ray that misses is retired and
    // its byte never read.  In cast 2 the byte IS the skip -- both reflections were specular: hare_image2_deposit's paths
    if constexpr (SCATTER) {
        if ((a.cut & kCutStoreSpecular2) && live) {
            bool spec = false;
            if (imaged && a.ev[i].hit) {
                const double* sg = a.sigma + (size_t)a.ev[i].poly_id * (size_t)B;
                double p = sg[0];
                for (int b = 1; b < B; ++b) p = p + sg[b];
                p = p / (double)B;
                spec = !(scatter_u(scatter_base(a, i), (unsigned long long)a.cast << 8, 0) < p);
            }
            a.spec2[i] = spec ? 1 : 0;
        }
        if ((a.cut & kCutSkipSpecular2) && live) imaged = a.spec2[i] != 0;
    }
    if constexpr (MAP) {
        // the walk holds the ray, t_end and L only: the event and the energies are read behind it (nothing the walk adds to overlaps them)
        if (live) {
            r = a.rays[i];
            if (!a.init_state) L = a.state[i];
            const XEventRec& ei = a.ev[i];
            if (!(a.cut & kCutSkipDetect) && !imaged) map_receivers<C>(a, i, r, ei.hit ? ei.t : __builtin_inf(), L);
        }
    }
    if (live) {
        e = a.ev[i];
        if constexpr (!MAP) r = a.rays[i];
        if constexpr (RAIN) rained = a.rain_flag[i] != 0;
        if (a.init_state) {
#pragma unroll
            for (int b = 0; b < kMaxBands; ++b) E[b] = 1.0;
        } else {
            if constexpr (!MAP) L = a.state[i];
#pragma unroll
            for (int b = 0; b < kMaxBands; ++b)
                if (b < B) E[b] = a.state[(size_t)(b + 1) * (size_t)a.n + (size_t)i];
        }
    }
    // ---- receivers
    if constexpr (!MAP) {                                                // the linear step; a map has taken its own, above
        const bool seen = live && !rained && !imaged;
        if (!(a.cut & kCutSkipDetect) && __ballot(seen) != 0ull) {      // kCutSkipDetect: cast 0 of a call with HARE_RECEIVE_DIRECT (uniform)
            const double t_end = (live && e.hit) ? e.t : __builtin_inf();
            const double nb = (double)a.n_bins;
            [[maybe_unused]] double ax = 0, ay = 0, az = 0;
            [[maybe_unused]] double Y[kAmbiMax];                                // C > 4: channels 4 .. C - 1 of a
            if constexpr (C > 4) {
#pragma unroll
                for (int j = 0; j < kAmbiMax; ++j) Y[j] = 0;
            }
            [[maybe_unused]] bool have_a = false;                               // wave-uniform
            for (int k = 0; k < a.n_rcv; ++k) {
                const double cx = rcv[4 * k + 0], cy = rcv[4 * k + 1], cz = rcv[4 * k + 2], r2 = rcv[4 * k + 3];
                bool det = false, binned = false;
                int bin = 0;
                if (seen) {
                    const double wx = cx - r.x, wy = cy - r.y, wz = cz - r.z;
                    const double s = ((wx * r.dx + wy * r.dy) + wz * r.dz) / ((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
                    const double qx = (r.x + r.dx * s) - cx, qy = (r.y + r.dy * s) - cy, qz = (r.z + r.dz * s) - cz;
                    det = s >= 0 && s < t_end && ((qx * qx + qy * qy) + qz * qz) < r2;
                    if (det) {
                        const double x = (L + s) / a.bin_len;
                        binned = x >= 0 && x < nb;
                        if (binned) bin = (int)floor(x);
                    }
                }
                const unsigned long long dm = __ballot(det);
                if (dm == 0ull) continue;                                       // the common case: nobody passed receiver k
                const unsigned long long bm = __ballot(binned);
                if (lane == 0) {
                    if (bm) atomicAdd(&a.det[2 * k], (unsigned long long)__popcll(bm));
                    if (dm & ~bm) atomicAdd(&a.det[2 * k + 1], (unsigned long long)__popcll(dm & ~bm));
                }
                if (bm == 0ull) continue;
                if constexpr (C >= 4) {
                    if (!have_a) {
                        have_a = true;
                        if (seen) {
                            const double len = sqrt((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
                            ax = -(r.dx / len);
                            ay = -(r.dy / len);
                            az = -(r.dz / len);
                            if constexpr (C > 4) ambi_harmonics<C>(ax, ay, az, Y);
                        }
                    }
                    unsigned long long* const row = a.hist + (size_t)k * (size_t)a.n_bins * (size_t)B * C;
                    if (!a.aggregate) {                                          // naive form (A/B): every detecting lane adds its own words
                        if (binned)
                            for (int b = 0; b < B; ++b) hist_add<C>(&row[((size_t)bin * B + b) * C], quant_m(E[b] * a.scale), ax, ay, az, Y);
                        continue;
                    }
                    unsigned long long todo = bm;
                    if constexpr (C > 4) {
                        while (todo) {                                           // one round per distinct bin among the wave's detections
                            const int leader = __ffsll((long long)todo) - 1;
                            const int lb = __shfl(bin, leader, 64);
                            const bool mine = binned && bin == lb;
                            todo &= ~__ballot(mine);
                            unsigned long long lo = 0, hi = 0;                   // channel lane >> 2 of bands (lane & 3) and (lane & 3) + 4
#pragma unroll
                            for (int b = 0; b < kMaxBands; ++b) {
                                if (b < B) {
                                    const double m = mine ? quant_m(E[b] * a.scale) : 0.0;     // m = 0 quantises to C zero words
                                    const unsigned long long sb = wave_sum16_u64(
                                        [&](int j) -> unsigned long long {
                                            if (j == 0) return (unsigned long long)rint(m);
                                            if (j >= C) return 0ull;
                                            return dir_q(m, j == 1 ? ax : (j == 2 ? ay : (j == 3 ? az : Y[j < 4 ? 0 : j - 4])));
                                        },
                                        lane);
                                    if ((lane & 3) == (b & 3)) (b < 4 ? lo : hi) = sb;
                                }
                            }
                            const int ch = lane >> 2, s = lane & 3;
                            unsigned long long* const w = &row[(size_t)lb * B * C];
                            if (ch < C && s < B) atomicAdd(&w[s * C + ch], lo);
                            if (ch < C && s + 4 < B) atomicAdd(&w[(s + 4) * C + ch], hi);
                        }
                        continue;
                    }
                    while (todo) {                                               // one round per distinct bin among the wave's detections
                        const int leader = __ffsll((long long)todo) - 1;
                        const int lb = __shfl(bin, leader, 64);
                        const bool mine = binned && bin == lb;
                        todo &= ~__ballot(mine);
                        unsigned long long mysum = 0;
#pragma unroll
                        for (int b = 0; b < kMaxBands; ++b) {
                            if (b < B) {
                                const double m = mine ? quant_m(E[b] * a.scale) : 0.0;     // m = 0 quantises to four zero words
                                const unsigned long long sb =
                                    wave_sum4_u64((unsigned long long)rint(m), dir_q(m, ax), dir_q(m, ay), dir_q(m, az), lane);
                                if ((lane & 15) == b) mysum = sb;
                            }
                        }
                        // lane 16 ch + b holds channel ch of band b: 4 B contiguous 8-byte adds, one instruction
                        if ((lane & 15) < B) atomicAdd(&row[((size_t)lb * B + (lane & 15)) * 4 + (lane >> 4)], mysum);
                    }
                    continue;
                }
                unsigned long long q[kMaxBands];
#pragma unroll
                for (int b = 0; b < kMaxBands; ++b) {
                    q[b] = 0;
                    if (b < B && binned) q[b] = (unsigned long long)rint(quant_m(E[b] * a.scale));
                }
                unsigned long long* const row = a.hist + (size_t)k * (size_t)a.n_bins * (size_t)B;
                if (!a.aggregate) {                                              // naive form (A/B): every detecting lane adds its own bands
                    if (binned)
                        for (int b = 0; b < B; ++b) atomicAdd(&row[(size_t)bin * B + b], q[b]);
                    continue;
                }
                unsigned long long todo = bm;
                while (todo) {                                                   // one round per distinct bin among the wave's detections
                    const int leader = __ffsll((long long)todo) - 1;
                    const int lb = __shfl(bin, leader, 64);
                    const bool mine = binned && bin == lb;
                    todo &= ~__ballot(mine);
                    unsigned long long mysum = 0;
#pragma unroll
                    for (int b = 0; b < kMaxBands; ++b) {
                        if (b < B) {
                            const unsigned long long sb = wave_allsum_u64(mine ? q[b] : 0ull);
                            if (lane == b) mysum = sb;
                        }
                    }
                    if (lane < B) atomicAdd(&row[(size_t)lb * B + lane], mysum);     // B contiguous 8-byte adds: one instruction
                }
            }
        }
    }
    // ---- state update, termination, reflection (hare_reflect's arithmetic and marks)
    bool lives_on = false;
    if (live) {
        bool diffuse = false;
        bool cut = false;                              // a termination rule retires the ray (the header's "Termination")
        unsigned long long base = 0, c8 = 0;
        double nx = 0, ny = 0, nz = 0;
        if (e.hit || a.init_state) {               // a miss leaves its state as it is (init_state: as it starts)
            const double* al = (e.hit && a.alpha) ? a.alpha + (size_t)e.poly_id * (size_t)B : nullptr;
            const bool scat = e.hit && !a.last;                // the choice, its weights and the rules: only a ray that will be reflected
            if constexpr (SCATTER) {
                // every load (absorption, scattering and normal of the polygon) ahead of the first store to the state, which the compiler
                // must assume may alias them: issued together, their latencies overlap
                const double* sg = a.sigma + (size_t)(scat ? e.poly_id : 0) * (size_t)B;
                double sig[kMaxBands];
#pragma unroll
                for (int b = 0; b < kMaxBands; ++b) sig[b] = (scat && b < B) ? sg[b] : 0.0;
                if (scat) {
                    const PolyRec& pr = a.polys[e.poly_id];
                    nx = pr.n[0]; ny = pr.n[1]; nz = pr.n[2];
                }
#pragma unroll
                for (int b = 0; b < kMaxBands; ++b)
                    if (b < B && al) E[b] = E[b] * (1.0 - al[b]);
                if (scat) {
                    double p = sig[0];
#pragma unroll
                    for (int b = 1; b < kMaxBands; ++b)
                        if (b < B) p = p + sig[b];
                    p = p / (double)B;
                    base = scatter_base(a, i);
                    c8 = (unsigned long long)a.cast << 8;
                    diffuse = scatter_u(base, c8, 0) < p;
                    const double den = diffuse ? p : 1.0 - p;                  // one division per band: sigma / p or (1 - sigma) / (1 - p)
#pragma unroll
                    for (int b = 0; b < kMaxBands; ++b)
                        if (b < B) E[b] = E[b] * ((diffuse ? sig[b] : 1.0 - sig[b]) / den);
                }
            } else {
#pragma unroll
                for (int b = 0; b < kMaxBands; ++b)
                    if (b < B && al) E[b] = E[b] * (1.0 - al[b]);              // no table: alpha = 0
            }
            const double Lp = e.hit ? L + e.t : L;
            if ((a.cut & (kCutTime | kCutFloor)) != 0 && scat) {      // a.cut is uniform: a call without a rule pays this one scalar test
                if ((a.cut & kCutTime) && Lp / a.bin_len >= (double)a.n_bins) {
                    cut = true;
                } else if (a.cut & kCutFloor) {
                    double m = E[0];
#pragma unroll
                    for (int b = 1; b < kMaxBands; ++b)
                        if (b < B) m = (E[b] > m) ? E[b] : m;
                    if (m < a.floor) {
                        cut = true;
                        if (a.cut & kCutRoulette) {
                            if constexpr (!SCATTER) {
                                base = scatter_base(a, i);
                                c8 = (unsigned long long)a.cast << 8;
                            }
                            const double ps = m / a.floor;
                            if (scatter_u(base, c8, 65) < ps) {                // the survivor carries what the casualties held
                                cut = false;
#pragma unroll
                                for (int b = 0; b < kMaxBands; ++b)
                                    if (b < B) E[b] = E[b] / ps;
                            }
                        }
                    }
                }
            }
            a.state[i] = Lp;
#pragma unroll
            for (int b = 0; b < kMaxBands; ++b)
                if (b < B) a.state[(size_t)(b + 1) * (size_t)a.n + (size_t)i] = E[b];
        }
        if (e.hit) {
            if (cut) {                                 // as a miss: no reflection, the mark, and the miss record later casts leave in place
                a.excl[i] = -2;
                XEventRec me;
                set_miss(me);
                a.ev[i] = me;
            } else if (!a.last) {
                if constexpr (SCATTER) a.rays[i] = diffuse ? scatter_hit(nx, ny, nz, r, e, base, c8) : reflect_about(nx, ny, nz, r, e);
                else a.rays[i] = reflect_hit(a.polys, r, e);         // kernels.hip: hare_reflect's arithmetic, shared
                a.excl[i] = e.poly_id;
                if constexpr (RAIN) a.rain_flag[i] = diffuse ? 1 : 0;
                lives_on = true;
            }
        } else if (!a.last) {
            a.excl[i] = -2;
        }
    }
    if (a.block_live) {
        const unsigned long long lm = __ballot(lives_on);
        const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (lane == 0 && blk * 64 < a.n) a.block_live[blk] = lm != 0ull ? 1 : 0;
    }
}

#define HARE_RECEIVE_KERNELS(SUFFIX, C)                                                                            \
    extern "C" __global__ __launch_bounds__(256) void hare_receive_reflect##SUFFIX(ReceiveArgs a)                  \
    {                                                                                                              \
        receive_body<false, false, C>(a);                                                                          \
    }                                                                                                              \
    extern "C" __global__ __launch_bounds__(256) void hare_receive_scatter##SUFFIX(ReceiveArgs a)                  \
    {                                                                                                              \
        receive_body<true, false, C>(a);                                                                           \
    }                                                                                                              \
    extern "C" __global__ __launch_bounds__(256) void hare_receive_scatter_rain##SUFFIX(ReceiveArgs a)             \
    {                                                                                                              \
        receive_body<true, true, C>(a);                                                                            \
    }                                                                                                              \
    extern "C" __global__ __launch_bounds__(256) void hare_receive_reflect_map##SUFFIX(ReceiveMapArgs a)           \
    {                                                                                                              \
        receive_body<false, false, C, true, ReceiveMapArgs>(a);                                                    \
    }                                                                                                              \
    extern "C" __global__ __launch_bounds__(256) void hare_receive_scatter_map##SUFFIX(ReceiveMapArgs a)           \
    {                                                                                                              \
        receive_body<true, false, C, true, ReceiveMapArgs>(a);                                                     \
    }
HARE_CHANNEL_FORMS(HARE_RECEIVE_KERNELS)
#undef HARE_RECEIVE_KERNELS

// ---- diffuse rain (HARE_RECEIVE_DIFFUSE_RAIN; the header's "receivers", "Diffuse rain")
// hare_rain_step runs between a cast's shoot and hare_receive_scatter_rain, which overwrites the rays and the state: a lane per ray reads what
// that kernel reads and recomputes E after absorption and L' = L + e.t with the same FP64 operations.  One launch deposits receiver k_dep
// (the flags the occlusion kernel left for the query the previous launch emitted) and emits receiver k_emit's query, so K receivers cost
// K + 1 launches of this kernel and K occlusion launches per cast (receive.cpp: receive_step).  A slot without a query is marked -2, which the occlusion
// kernels skip under HARE_SHOOT_RETIRED_RAYS (no traversal, flag 0).  The deposit adds per lane, not per distinct bin of a wave as the
// receiver step does: nearly every visible ray deposits and their bins are spread, so the wave's rounds over distinct bins cost more than
// they save (hall, 1M rays, K = 8, B = 8: the rain loop 94.5 ms aggregated, 79.5 ms per lane; the same histogram).
// C is the channel count: for C >= 4 the deposit adds a band's C words with hist_add, weighted by the arrival vector -(v / dist) and its
// polynomials, quantised where they are added; C = 1 adds the B words it quantised in the band loop.
template <int C>
static __device__ __forceinline__ void rain_body(const RainArgs& a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int B = a.bands;
    const bool in = i < a.n;
    const bool vis = in && a.k_dep >= 0 && a.sexcl[i] != -2 && a.socc[i] == 0;     // eligible for receiver k_dep and not occluded
    // a ray takes part when it is live, hit and its polygon's row mean p > 0 (the loop launches this kernel only in casts that reflect);
    // vis implies it: the previous launch found the same
    bool part = false;
    XEventRec e;
    double sig[kMaxBands];
#pragma unroll
    for (int b = 0; b < kMaxBands; ++b) sig[b] = 0;
    if (in && (a.k_emit >= 0 || vis) && !(a.marks_valid && a.marks[i] == -2)) {
        e = a.ev[i];
        if (e.hit) {
            const double* sg = a.sigma + (size_t)e.poly_id * (size_t)B;
#pragma unroll
            for (int b = 0; b < kMaxBands; ++b)
                if (b < B) sig[b] = sg[b];
            double p = sig[0];
#pragma unroll
            for (int b = 1; b < kMaxBands; ++b)
                if (b < B) p = p + sig[b];
            part = p / (double)B > 0;
        }
    }
    double nx = 0, ny = 0, nz = 0, len = 1;
    if (part) {
        const RayRec r = a.rays[i];
        const PolyRec& pr = a.polys[e.poly_id];
        nx = pr.n[0]; ny = pr.n[1]; nz = pr.n[2];
        if (dot3(r.dx, r.dy, r.dz, nx, ny, nz) > 0) {      // n': the side the ray came from
            nx = -nx;
            ny = -ny;
            nz = -nz;
        }
        len = sqrt((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
    }
    // ---- deposit: receiver k_dep, the eligible rays its query found unoccluded
    if (a.k_dep >= 0 && __ballot(vis) != 0ull) {
        const int k = a.k_dep;
        bool binned = false;
        int bin = 0;
        unsigned long long q[kMaxBands];
#pragma unroll
        for (int b = 0; b < kMaxBands; ++b) q[b] = 0;
        [[maybe_unused]] double mq[kMaxBands];                          // DIR: m_b, quantised where it is added
        [[maybe_unused]] double ax = 0, ay = 0, az = 0;
        [[maybe_unused]] double Y[kAmbiMax];                            // C > 4: channels 4 .. C - 1 of a
        if constexpr (C >= 4) {
#pragma unroll
            for (int b = 0; b < kMaxBands; ++b) mq[b] = 0;
        }
        if (vis) {
            const double cx = a.rcv[4 * k + 0], cy = a.rcv[4 * k + 1], cz = a.rcv[4 * k + 2], rr = a.rcv[4 * k + 3];
            const double vx = cx - e.x, vy = cy - e.y, vz = cz - e.z;
            const double d2 = (vx * vx + vy * vy) + vz * vz;
            const double cs = (vx * nx + vy * ny) + vz * nz;
            const double dist = sqrt(d2);
            const double w = (cs / dist) * (rr / d2);
            const double L = a.init_state ? 0.0 : a.state[i];
            const double x = ((L + e.t) + dist / len) / a.bin_len;
            binned = x >= 0 && x < (double)a.n_bins;
            if (binned) {
                bin = (int)floor(x);
                const double* al = a.alpha ? a.alpha + (size_t)e.poly_id * (size_t)B : nullptr;
                if constexpr (C >= 4) {
                    ax = -(vx / dist);
                    ay = -(vy / dist);
                    az = -(vz / dist);
                    if constexpr (C > 4) ambi_harmonics<C>(ax, ay, az, Y);
                }
#pragma unroll
                for (int b = 0; b < kMaxBands; ++b) {
                    if (b < B) {
                        const double E = a.init_state ? 1.0 : a.state[(size_t)(b + 1) * (size_t)a.n + (size_t)i];
                        const double Ea = al ? E * (1.0 - al[b]) : E;
                        const double v = quant_m(((Ea * sig[b]) * w) * a.scale);
                        if constexpr (C >= 4) mq[b] = v;
                        else q[b] = (unsigned long long)rint(v);
                    }
                }
            }
        }
        const unsigned long long dm = __ballot(vis), bm = __ballot(binned);
        if (lane == 0) {
            if (bm) atomicAdd(&a.det[2 * k], (unsigned long long)__popcll(bm));
            if (dm & ~bm) atomicAdd(&a.det[2 * k + 1], (unsigned long long)__popcll(dm & ~bm));
        }
        if constexpr (C >= 4) {
            if (binned) {                                               // per lane, the C words of a band one by one
                unsigned long long* const row = a.hist + ((size_t)k * (size_t)a.n_bins + (size_t)bin) * (size_t)B * C;
#pragma unroll
                for (int b = 0; b < kMaxBands; ++b) {
                    if (b < B) hist_add<C>(&row[C * b], mq[b], ax, ay, az, Y);
                }
            }
        } else if (binned) {                                            // per lane: rain's bins are spread, see above
            unsigned long long* const row = a.hist + ((size_t)k * (size_t)a.n_bins + (size_t)bin) * (size_t)B;
            for (int b = 0; b < B; ++b) atomicAdd(&row[b], q[b]);
        }
    }
    // ---- emit: receiver k_emit's query
    if (a.k_emit >= 0 && in) {
        const int k = a.k_emit;
        bool elig = false;
        if (part) {
            const double cx = a.rcv[4 * k + 0], cy = a.rcv[4 * k + 1], cz = a.rcv[4 * k + 2], rr = a.rcv[4 * k + 3];
            const double vx = cx - e.x, vy = cy - e.y, vz = cz - e.z;
            const double d2 = (vx * vx + vy * vy) + vz * vz;
            const double cs = (vx * nx + vy * ny) + vz * nz;
            elig = d2 > rr && cs > 0;
            if (elig) {
                RayRec s;
                s.x = e.x; s.y = e.y; s.z = e.z;
                s.dx = vx; s.dy = vy; s.dz = vz;
                a.srays[i] = s;
                a.stmax[i] = 1.0;
            }
        }
        a.sexcl[i] = elig ? e.poly_id : -2;
    }
}

#define HARE_RAIN_KERNEL(SUFFIX, C)                                                                \
    extern "C" __global__ __launch_bounds__(256) void hare_rain_step##SUFFIX(RainArgs a)           \
    {                                                                                              \
        rain_body<C>(a);                                                                           \
    }
HARE_CHANNEL_FORMS(HARE_RAIN_KERNEL)
#undef HARE_RAIN_KERNEL
