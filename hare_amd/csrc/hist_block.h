// hist_block.h -- what the kernels on a receive histogram share (reduce.hip, project.hip, render.hip).  #included from kernels.hip ahead of
// reduce.hip.  Integer arithmetic only, 128 bits from 64-bit pieces.
//   U128 ...      the 128-bit pieces: make128, add128, sub128, lt128, mul_64x32, and wave_scan, the sum of a band's lanes within a wave
//   weighted      g = floor(h * w / 2^32), the header's weighting of a histogram word: the ONE statement of it on the device
//   band_total    a band's total over the workgroup from its four waves' totals in LDS
//   Block         the integer kernels' layout (hare_hist_reduce, hare_hist_project): a workgroup of 256 threads owns a receiver, whose
//                 n_bins x B (x channels) words are contiguous, and reads them in TILES of step = 256 / B bins = step * B words, thread
//                 t < step * B taking word t of each tile: consecutive lanes read consecutive words (8 B each; with four channels every fourth
//                 word, the W channel -- the line is fetched either way), and a thread keeps ONE band, b = t % B, and the bin t / B of every
//                 tile.  (At most 4 threads idle for B = 3, 5, 6, 7.)  The two kernels load through loaders of their own: g_at (reduce.hip), a
//                 word at a time and branchy, and g4 here, four words together and branch-free; each was scheduled and measured for its kernel.
// Product code; nothing from oracle/.
#pragma once

namespace hare_hist {

struct U128 {
    unsigned long long lo, hi;
};
__device__ __forceinline__ U128 make128(unsigned long long lo, unsigned long long hi = 0)
{
    U128 r;
    r.lo = lo;
    r.hi = hi;
    return r;
}
__device__ __forceinline__ U128 add128(U128 a, U128 b)          // add with carry
{
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
    return r;
}
__device__ __forceinline__ U128 sub128(U128 a, U128 b)          // a >= b
{
    U128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull);
    return r;
}
__device__ __forceinline__ bool lt128(U128 a, U128 b)
{
    return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo);
}
// x * m, 96 bits, from two 32 x 32 -> 64 multiply-adds
__device__ __forceinline__ U128 mul_64x32(unsigned long long x, uint32_t m)
{
    const unsigned long long p0 = (x & 0xFFFFFFFFull) * m;
    const unsigned long long p1 = (x >> 32) * m + (p0 >> 32);
    return make128((p0 & 0xFFFFFFFFull) | (p1 << 32), p1 >> 32);
}
// Inclusive scan over the lanes of a wave that share a band: lane L receives the sum of lanes L, L - B, L - 2 B, ...
__device__ __forceinline__ U128 wave_scan(U128 v, int B, int lane)
{
    for (int d = B; d < 64; d <<= 1) {
        U128 o;
        o.lo = __shfl_up(v.lo, (unsigned)d);
        o.hi = __shfl_up(v.hi, (unsigned)d);
        if (lane >= d) v = add128(v, o);
    }
    return v;
}
// floor(h * w / 2^32) from h's 32-bit halves; w < 2^32
__device__ __forceinline__ unsigned long long weighted(unsigned long long h, unsigned long long w)
{
    return (h >> 32) * w + (((h & 0xFFFFFFFFull) * w) >> 32);
}
// band b's total from the four waves' (wave_scan: the last B lanes of a wave hold its B totals)
__device__ __forceinline__ U128 band_total(const U128 (&tot)[4][kMaxBands], int b)
{
    return add128(add128(tot[0][b], tot[1][b]), add128(tot[2][b], tot[3][b]));
}

struct Block {                                  // what a thread knows of its receiver's block
    const unsigned long long* h;
    const uint32_t* weight;
    size_t ch;
    int nb, B, b, li, step, tiles;
    bool on;
    // g(k, i, b) of this thread's band for the bins i0 + q * step, q = 0 .. 3; 0 past the end and for an idle thread.  Without a branch per
    // word: such a thread reads word 0 of the block, which exists, and drops it; the loads go out together, then the weights' products
    __device__ __forceinline__ void g4(int i0, unsigned long long (&g)[4]) const
    {
        int e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * step;
            e[q] = on && i < nb ? i * B + b : -1;
            g[q] = h[(size_t)max(e[q], 0) * ch];
        }
        if (weight) {
            unsigned long long w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = weight[max(e[q], 0)];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = weighted(g[q], w[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = e[q] >= 0 ? g[q] : 0ull;
    }
};
// the block of receiver blockIdx.x as thread threadIdx.x of its workgroup sees it
__device__ __forceinline__ Block block_of(const unsigned long long* hist, const uint32_t* weight, int n_bins, int bands, int channels)
{
    const int t = threadIdx.x;
    Block k;
    k.nb = n_bins;
    k.B = bands;
    k.step = 256 / k.B;
    k.b = t % k.B;
    k.li = t / k.B;
    k.on = t < k.step * k.B;
    k.tiles = (k.nb + k.step - 1) / k.step;
    k.ch = (size_t)channels;
    k.h = hist + (size_t)blockIdx.x * (size_t)k.nb * (size_t)k.B * k.ch;
    k.weight = weight;
    return k;
}

}  // namespace hare_hist
