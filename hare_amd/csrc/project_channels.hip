// project_channels.hip -- hare_hist_project_channels: the projection of project.hip for EVERY channel of a directional histogram
// (include/hare_hip.h, "receivers", "Directional projection"): per receiver k, band b, vector j and channel ch the exact signed sum
// P(k, b, j, ch) = sum over i of c_j[i] * g(k, i, b, ch) as a 128-bit two's-complement integer; word 0 of an entry (W) is unsigned, the
// words ch >= 1 are two's-complement int64 and weighted with a floor towards minus infinity.  #included from kernels.hip behind hist_block.h
// and project.hip, whose 128-bit pieces (U128, add128, sub128, wave_scan, weighted) and product (hare_project::Acc, mul_add) it shares by
// name.  Integer arithmetic only: the result is a function of the inputs, bit for bit (tests/project_channels_ref.py restates it).
//
//   layout   a workgroup of 256 threads per receiver, whose n_bins x P words (P = B x channels <= 128 pairs of band and channel) are
//            contiguous.  A tile is step = 256 / P bins = step * P consecutive words; thread t < step * P takes word t of every tile and so
//            keeps ONE pair p = t % P = b * channels + ch and the bin t / P of every tile; at most P - 1 threads idle.  Every word of a
//            line the kernel fetches is used, where hare_hist_project at `channels` 16 uses one in sixteen.
//   signs    no sign test and no select on a word's sign in the loop.  A signed word is offset to unsigned, h' = h ^ 2^63 = h + 2^63, by a
//            per-thread mask that is 0 for W.  floor((h' - 2^63) w / 2^32) = weighted(h', w) - 2^31 w exactly (2^31 w is an integer), so
//            G = weighted(h', w) - 2^31 w + 2^63 = g + 2^63 is an unsigned 64-bit number formed with one masked 64-bit add; without weights
//            G = h'.  For W, G = g.  The coefficient is offset as in project.hip, c' = c ^ 0x80000000, and the loop accumulates the
//            unsigned 96-bit products c' * G.  With T = sum G and, for a signed pair, S_j = sum c_j (int64),
//                P = sum c' G  -  2^31 T  -  [ch >= 1] 2^63 S_j      (mod 2^128),
//            applied once per pair and vector at the end.  S_j does not depend on the pair: the workgroup sums the sweep's vectors once,
//            thread t over the bins t, t + 256, ... (1 / P of the loop's coefficient loads; skipped at channels = 1).
//   sweeps   up to kGroup = 8 vectors per sweep, compiled once per count as in project.hip; four tiles' words and coefficients in flight.
//   coef     through the vector cache: the P lanes of a bin share c_j[i].  No barrier in the tile loop.
//   sums     the lanes of a pair are summed by wave_scan at lane stride P where P < 64 (the last P lanes of a wave hold its P totals:
//            four partial sums per pair, one per wave); where P >= 64 a wave holds a pair at most once and every active thread's own sum
//            is a partial, t / P <= 3 of them per pair.  Either way at most four partials per pair, written to s_part[.][slot][p] and
//            summed by the thread that writes the output word.  The quantities go through LDS four at a time (T alone, then the
//            vectors 0 .. 3 and 4 .. 7 of the sweep): 4 x 4 x 128 x 16 bytes.  Every output word is written once; no atomics.
//
// No scratch, no VGPR spilled (tests/test_project_channels_kernel_resources.py); LDS static.  Nothing depends on the grid beyond
// blockIdx.x = k.  band_total (hist_block.h) is typed for kMaxBands columns and is not used: a pair's partials are added in place.
namespace hare_project_channels {

using namespace hare_hist;
using hare_project::Acc;
using hare_project::mul_add;
constexpr int kGroup = kProjectGroup;           // vectors per sweep, at most
constexpr int kMaxPairs = 128;                  // B x channels
constexpr int kRound = 4;                       // quantities that pass through LDS together

struct Pairs {                                  // what a thread knows of its receiver's block
    const unsigned long long* h;                // the block's word p of bin 0
    const uint32_t* weight;                     // weight[b] of bin 0, or null
    unsigned long long flip;                    // 2^63 for a signed channel, 0 for W: h ^ flip = h', and the bias of G
    unsigned long long smask;                   // all ones for a signed channel, 0 for W
    int nb, B, P, p, li, step, tiles;
    bool on;
    // G of this thread's pair for the bins i0 + q * step, q = 0 .. 3; 0 past the end and for an idle thread, which reads bin 0's word and
    // drops it (hist_block.h, Block::g4, does the same): the loads go out together, then the weights' products
    __device__ __forceinline__ void g4(int i0, unsigned long long (&g)[4]) const
    {
        int e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * step;
            e[q] = on && i < nb ? i : -1;
            g[q] = h[(size_t)max(e[q], 0) * (size_t)P] ^ flip;
        }
        if (weight) {
            unsigned long long w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = weight[(size_t)max(e[q], 0) * (size_t)B];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = weighted(g[q], w[q]) + (flip - ((w[q] << 31) & smask));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = e[q] >= 0 ? g[q] : 0ull;
    }
};

__device__ __forceinline__ Pairs pairs_of(const unsigned long long* hist, const uint32_t* weight, int n_bins, int bands, int channels)
{
    const int t = threadIdx.x;
    Pairs k;
    k.nb = n_bins;
    k.B = bands;
    k.P = bands * channels;
    k.step = 256 / k.P;
    k.p = t % k.P;
    k.li = t / k.P;
    k.on = t < k.step * k.P;
    k.tiles = (k.nb + k.step - 1) / k.step;
    const bool sgn = k.p % channels != 0;
    k.flip = sgn ? 1ull << 63 : 0ull;
    k.smask = sgn ? ~0ull : 0ull;
    k.h = hist + (size_t)blockIdx.x * (size_t)k.nb * (size_t)k.P + (size_t)k.p;
    k.weight = weight ? weight + k.p / channels : nullptr;
    return k;
}

// The partial sums of one quantity: this thread's, or with P < 64 the wave's per pair in its last P lanes
__device__ __forceinline__ void put(const Pairs& k, U128 v, U128 (*part)[kMaxPairs], int lane, int wv)
{
    if (k.P < 64) {
        v = wave_scan(v, k.P, lane);
        if (lane >= 64 - k.P) part[wv][k.p] = v;
    } else if (k.on) {
        part[k.li][k.p] = v;
    }
}
// pair p's total of one quantity from its partials: four waves', or those of the threads p, p + P, ... < step * P
__device__ __forceinline__ U128 total(const U128 (*part)[kMaxPairs], int P, int step, int p)
{
    const int n = P < 64 ? 4 : step;
    U128 s = part[0][p];
    for (int x = 1; x < n; ++x) s = add128(s, part[x][p]);
    return s;
}

// One sweep over the block for the N vectors j0 .. at c0 (vector-major, n_bins apart): the sums U_u of c'_u[i] * G per thread, with WANT_T
// the sum of G; then, through LDS, a round per four quantities, the output words of these vectors
template <int N>
__device__ __forceinline__ void sweep(const Pairs& k, const ProjectArgs& a, int j0, bool want_T, U128 (*s_part)[4][kMaxPairs], U128* s_T,
                                      long long (*s_C)[kGroup], int t, int lane, int wv)
{
    const int32_t* const c0 = a.coef + (size_t)j0 * (size_t)k.nb;
    const int C = a.channels;
    if (C > 1) {                                                              // S_u = sum over i of c_u[i], per wave; uniform
        long long S[N];
#pragma unroll
        for (int u = 0; u < N; ++u) S[u] = 0;
        for (int i = t; i < k.nb; i += 256) {
#pragma unroll
            for (int u = 0; u < N; ++u) S[u] += (long long)c0[(size_t)u * (size_t)k.nb + (size_t)i];
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
            for (int d = 32; d >= 1; d >>= 1) S[u] += __shfl_xor(S[u], d);
            if (lane == 0) s_C[wv][u] = S[u];
        }
    }
    Acc U[N];
#pragma unroll
    for (int u = 0; u < N; ++u) U[u].a0 = U[u].a1 = 0, U[u].a23 = 0;
    U128 T = make128(0);
    for (int tile = 0; tile < k.tiles; tile += 4) {
        unsigned long long g[4];
        uint32_t c[4][N];
        k.g4(tile * k.step + k.li, g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int32_t* const cq = c0 + min((tile + q) * k.step + k.li, k.nb - 1);      // past the end G is 0: any coefficient serves
#pragma unroll
            for (int u = 0; u < N; ++u) c[q][u] = (uint32_t)cq[(size_t)u * (size_t)k.nb] ^ 0x80000000u;
        }
        if (want_T) {
#pragma unroll
            for (int q = 0; q < 4; ++q) T = add128(T, make128(g[q]));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int u = 0; u < N; ++u) mul_add(U[u], g[q], c[q][u]);
        }
    }
    if (want_T) {                                                             // uniform
        put(k, T, s_part[0], lane, wv);
        __syncthreads();
        if (t < k.P) {
            const U128 s = total(s_part[0], k.P, k.step, t);
            s_T[t] = make128(s.lo << 31, (s.hi << 31) | (s.lo >> 33));       // T < 2^91: nothing is shifted out
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < N; r += kRound) {
#pragma unroll
        for (int u = r; u < r + kRound && u < N; ++u)
            put(k, make128((unsigned long long)U[u].a0 | ((unsigned long long)U[u].a1 << 32), U[u].a23), s_part[u - r], lane, wv);
        __syncthreads();
        const int n_q = min(kRound, N - r);
        for (int o = t; o < n_q * k.P; o += 256) {                           // (u, p): vector j0 + r + u of pair p
            const int u = o / k.P, p = o - u * k.P;
            const int b = p / C, ch = p - b * C;
            U128 v = sub128(total(s_part[u], k.P, k.step, p), s_T[p]);       // mod 2^128: the two's complement of a negative sum
            if (ch) {                                                         // a signed pair: minus 2^63 S
                const long long S = s_C[0][r + u] + s_C[1][r + u] + s_C[2][r + u] + s_C[3][r + u];
                v = sub128(v, make128((unsigned long long)S << 63, (unsigned long long)(S >> 1)));
            }
            const size_t j = (size_t)(j0 + r + u);
            unsigned long long* out = a.proj + ((((size_t)blockIdx.x * (size_t)k.B + (size_t)b) * (size_t)a.n_vec + j) * (size_t)C + (size_t)ch) * 2;
            out[0] = v.lo;
            out[1] = v.hi;
        }
        __syncthreads();
    }
}

}  // namespace hare_project_channels

extern "C" __global__ __launch_bounds__(256) void hare_hist_project_channels(ProjectArgs a)
{
    using namespace hare_project_channels;
    __shared__ U128 s_part[kRound][4][kMaxPairs];      // per quantity of a round, partial and pair
    __shared__ U128 s_T[kMaxPairs];                    // 2^31 * T per pair, from the first sweep on
    __shared__ long long s_C[4][kGroup];               // per wave and vector of the sweep: its share of sum c

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int J = a.n_vec;
    const Pairs k = pairs_of(a.hist, a.weight, a.n_bins, a.bands, a.channels);

    for (int j0 = 0; j0 < J; j0 += kGroup) {
        const int n_act = min(kGroup, J - j0);                                // vectors of this sweep
        const bool want_T = j0 == 0;
        switch (n_act) {                                                       // uniform
        case 8: sweep<8>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        case 7: sweep<7>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        case 6: sweep<6>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        case 5: sweep<5>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        case 4: sweep<4>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        case 3: sweep<3>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        case 2: sweep<2>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        default: sweep<1>(k, a, j0, want_T, s_part, s_T, s_C, t, lane, wv); break;
        }
    }
}
