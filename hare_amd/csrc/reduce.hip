// reduce.hip -- hare_hist_reduce: a receive histogram reduced, on the device, to what a receiver map's user reads from it (include/hare_hip.h,
// "receivers", "Reduction"): per receiver and band the sums S0 = sum g and S1 = sum i * g over up to 16 bin windows, and the bins at which the
// backward-integrated decay R(i) crosses up to 32 levels.  #included from kernels.hip behind hist_block.h, which holds what this kernel
// shares with hare_hist_project and hare_hist_render: the 128-bit pieces (U128, add128, ..., wave_scan), the weighting (weighted), a band's
// total over the four waves (band_total) and the layout -- Block: a workgroup of 256 threads owns a receiver and reads its block in tiles of
// step = 256 / B bins, a thread keeping ONE band, b = t % B, and the bin li = t / B of every tile.  Integer arithmetic only: the result is a
// function of the inputs, bit for bit (tests/reduce_ref.py restates it in Python integers).
//
//   pass 1   T and the window sums.  A thread adds its words into T, S0[u], S1[u] (128 bits each) for four windows at a time -- a sweep
//            over the block per four windows: one for the usual n_win <= 4, later sweeps read the 64 KiB or so from L2 -- four loads in
//            flight.  A sweep does the arithmetic of its own windows only, and T is formed only when there are levels.  The threads of a
//            band are then summed by a wave scan at lane stride B (the last B lanes of a wave hold its B totals) and four LDS words per
//            band; the thread (u, b) writes window j0 + u of band b: every output word once, no atomics.
//   pass 2   the crossings.  With thr = floor(T * f / 2^32), R(i) * 2^32 <= T * f is R(i) <= thr, that is P(i) >= need = T - thr, and P does
//            not decrease: the crossing is the NUMBER of bins with P(i) < need.  The thread (l, b) = (t / B, t % B) owns level l of band b
//            (B * n_lev <= 256) and holds need and its count in registers.  Per tile a forward scan gives every bin its P(i): the same wave
//            scan, the waves' totals through LDS, a 128-bit carry per band from tile to tile; the prefixes go to LDS.  The owner of an open
//            level compares the tile's END (the carry) with need: below, all the tile's bins count; else the tile holds the crossing, found
//            by bisection in the tile's prefixes (8 steps at most), and the level is closed.  This tests every bin of a tile against every
//            open level at the price of one compare.  The loop ends when no level is open.  The next tile's word is loaded before this
//            tile's barriers; the block was just read by this CU, so pass 2 is served from L2.
//
// No scratch, no VGPR spilled (tests/test_hist_reduce_kernel_resources.py); LDS 8 832 bytes.  Nothing depends on the grid beyond blockIdx.x = k.
// K = 1 with a huge n_bins runs on this one workgroup: a host-sized problem, and not what the kernel is for.
namespace hare_reduce {

constexpr int kSweep = 4;                       // windows per sweep of pass 1
constexpr int kQ = 1 + 2 * kSweep;              // T, then S0 and S1 per window

}  // namespace hare_reduce

extern "C" __global__ __launch_bounds__(256) void hare_hist_reduce(ReduceArgs a)
{
    using namespace hare_hist;
    using namespace hare_reduce;
    __shared__ U128 s_tot[kQ][4][kMaxBands];    // per quantity, wave and band: the wave's total
    __shared__ U128 s_T[kMaxBands];
    __shared__ U128 s_pre[256];                 // pass 2: the tile's exclusive prefixes P(i), word order

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n_win = a.n_win, n_lev = a.n_lev;
    const Block k = block_of(a.hist, a.weight, a.n_bins, a.bands, a.channels);
    const int B = k.B, nb = k.nb, step = k.step, b = k.b, li = k.li, tiles = k.tiles;
    const bool on = k.on;

    // g(k, i, b) of this thread's band; 0 past the end and for an idle thread
    auto g_at = [&](int i) -> unsigned long long {
        if (!on || i >= nb) return 0ull;
        const int e = i * B + b;
        const unsigned long long hv = k.h[(size_t)e * k.ch];
        return k.weight ? weighted(hv, k.weight[e]) : hv;
    };

    // ---- pass 1
    for (int j0 = 0; j0 == 0 || j0 < n_win; j0 += kSweep) {
        const int n_act = min(kSweep, n_win - j0);                             // windows of this sweep (0: levels only)
        const bool want_T = j0 == 0 && n_lev > 0;                              // T serves pass 2 alone
        int lo[kSweep], hi[kSweep];
#pragma unroll
        for (int u = 0; u < kSweep; ++u) {
            lo[u] = u < n_act ? a.win[2 * (j0 + u)] : 0;
            hi[u] = u < n_act ? a.win[2 * (j0 + u) + 1] : 0;
        }
        U128 T = make128(0), S0[kSweep], S1[kSweep];
#pragma unroll
        for (int u = 0; u < kSweep; ++u) S0[u] = S1[u] = make128(0);
        for (int tile = 0; tile < tiles; tile += 4) {
            unsigned long long g[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = g_at((tile + q) * step + li);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = (tile + q) * step + li;
                const U128 p = mul_64x32(g[q], (uint32_t)i);
                if (want_T) T = add128(T, make128(g[q]));
#pragma unroll
                for (int u = 0; u < kSweep; ++u) {
                    if (u >= n_act) break;                                     // uniform: an unused slot costs nothing
                    const bool in = i >= lo[u] && i < hi[u];
                    S0[u] = add128(S0[u], make128(in ? g[q] : 0ull));
                    S1[u] = add128(S1[u], in ? p : make128(0));
                }
            }
        }
        if (want_T) {
            const U128 s = wave_scan(T, B, lane);
            if (lane >= 64 - B) s_tot[0][wv][b] = s;
        }
#pragma unroll
        for (int u = 0; u < kSweep; ++u) {
            if (u >= n_act) break;
            const U128 s0 = wave_scan(S0[u], B, lane), s1 = wave_scan(S1[u], B, lane);
            if (lane >= 64 - B) {
                s_tot[1 + 2 * u][wv][b] = s0;
                s_tot[2 + 2 * u][wv][b] = s1;
            }
        }
        __syncthreads();
        if (want_T && t < B) s_T[t] = band_total(s_tot[0], t);
        if (t < kSweep * B && j0 + li < n_win) {                               // thread (u, b) = (li, b): window j0 + u of band b
            const U128 s0 = band_total(s_tot[1 + 2 * li], b), s1 = band_total(s_tot[2 + 2 * li], b);
            unsigned long long* out = a.sums + (((size_t)blockIdx.x * (size_t)B + (size_t)b) * (size_t)n_win + (size_t)(j0 + li)) * 4;
            out[0] = s0.lo;
            out[1] = s0.hi;
            out[2] = s1.lo;
            out[3] = s1.hi;
        }
        __syncthreads();
    }
    if (n_lev == 0) return;

    // ---- pass 2
    const bool owner = on && li < n_lev;                                       // of level li of band b
    U128 need = make128(0);
    if (owner) {
        const U128 T = s_T[b];
        const uint32_t f = a.levels[li];
        U128 x = mul_64x32(T.lo, f);                                           // T * f: T < 2^91, so the high part fits
        x.hi += T.hi * f;
        need = sub128(T, make128((x.lo >> 32) | (x.hi << 32), x.hi >> 32));    // T - floor(T * f / 2^32)
    }
    int cnt = 0;
    bool open = owner;
    U128 carry = make128(0);                                                   // P at the tile's first bin, this thread's band
    unsigned long long g_next = g_at(li);
    for (int tile = 0; tile < tiles; ++tile) {
        const unsigned long long g = g_next;
        g_next = g_at((tile + 1) * step + li);
        const U128 s = wave_scan(make128(g), B, lane);
        if (lane >= 64 - B) s_tot[0][wv][b] = s;
        __syncthreads();
        U128 before = carry;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const U128 tw = s_tot[0][w][b];
            carry = add128(carry, tw);
            if (w < wv) before = add128(before, tw);
        }
        s_pre[t] = sub128(add128(before, s), make128(g));
        __syncthreads();
        if (open) {
            const int here = min(step, nb - tile * step);                      // bins of this tile
            if (lt128(carry, need)) {
                cnt += here;
            } else {
                int l0 = 0, l1 = here;                                         // the number of bins of the tile with P(i) < need
                while (l0 < l1) {
                    const int mid = (l0 + l1) >> 1;
                    if (lt128(s_pre[mid * B + b], need)) l0 = mid + 1;
                    else l1 = mid;
                }
                cnt += l0;
                open = false;
            }
        }
        if (__syncthreads_count(open ? 1 : 0) == 0) break;
    }
    if (owner) a.cross[((size_t)blockIdx.x * (size_t)B + (size_t)b) * (size_t)n_lev + (size_t)li] = cnt;
}
