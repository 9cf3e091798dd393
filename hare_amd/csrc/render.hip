// render.hip -- hare_hist_render: a receive histogram rendered, on the device, to pressure impulse responses (include/hare_hip.h, "receivers",
// "Rendering"): per receiver a +-1 noise sequence, filtered per band by the caller's FIR taps, scaled per bin and band so that the band's
// energy in the bin is the histogram's, weighted per channel by the direction the histogram recorded, and summed over the bands.  #included
// from kernels.hip.  FP64, no contraction; every sum runs in the header's order (tests/render_ref.py restates it in numpy).
//
// Tiling: WHOLE BINS.  p(k, b, i) needs all M samples of a bin before one of them can be scaled, so a workgroup of 512 threads owns
// `tile_bins` consecutive bins of one receiver (S = tile_bins * M samples; the host picks tile_bins so that the B x S filtered samples are
// about 32 KiB, or one bin where a bin alone is more) and keeps y(k, b, n) of the tile in LDS from the filter to the output: y is computed
// once, and nothing proportional to N exists outside `out`.  LDS, dynamic: the taps (B x T doubles, <= 64 KiB), y (B x S, <= 64 KiB), the
// gains a * r_ch (tile_bins x B x channels, <= 16 KiB), a (tile_bins x B) and the sign mask: <= 148 KiB of the 160; the usual shapes take
// less than 80 and two workgroups share a CU.
//
//   signs    s(k, i) for the tile's S samples and the T - 1 behind them (the halo): one mix per sample, a wave's 64 signs become one 64-bit word of
//            the mask by a ballot (bit set: -1.0).  A word of padding in front keeps every window below inside the mask.
//   filter   a wave takes one band and 64 runs of R = 8 consecutive samples, a run per lane.  The taps go by in blocks of 32: for a block the
//            lane needs the 32 + R - 1 signs s(m0 + T - 1 - t0 - 31 ..), one funnel shift of two mask words; a sign becomes the double
//            +-1.0 by a shift and an and-or, once, and slides through the R accumulators as t advances.  y = y + tap * s is ONE fma: the
//            product by +-1.0 is exact, so rounding the sum once is rounding the sum of the rounded product -- bit for bit the header's
//            multiply and add (zeros and NaNs included), at one instruction per tap and sample.  The accumulator starts at -0.0, the
//            identity of the add, so tap 0 needs no form of its own.  The tap is one LDS read at a wave-uniform address per R fmas.
//   p, a     a thread per (bin, band): the sequential sum of squares over the bin's samples from LDS, then g, e and a = sqrt(e / p).
//   gains    a thread per (bin, band, channel): r_ch from the histogram's signed word, a * r_ch into LDS -- one division per entry,
//            not per sample.
//   output   a thread per (channel, sample), consecutive lanes on consecutive samples: the sum over the bands in order, one store.
//
// No scratch, no VGPR spilled (tests/test_render_kernel_resources.py).  Nothing is read or written outside the tile's own words: the last
// tile of a receiver holds n_bins - i0 bins and every loop runs to that count.
namespace hare_render {

constexpr int R = kRenderRun;
constexpr int kWaves = kRenderThreads / 64;

// +1.0, or -1.0 when bit p (0 .. 63, known at compile time after unrolling) of the window (wlo, whi) is set
__device__ __forceinline__ double sign_at(uint32_t wlo, uint32_t whi, int p)
{
    const uint32_t w = p < 32 ? (wlo << (31 - p)) : (whi << (63 - p));
    return __hiloint2double((int)((w & 0x80000000u) | 0x3FF00000u), 0);
}

// taps t0 .. t0 + 31 (FULL) or t0 .. t0 + rem - 1 of one band into the R accumulators of a run.  Bit p of the window is the sign
// s(m0 + T - 1 - t0 - 31 + p): tap t0 + u meets sample m0 + r at p = 31 - u + r
template <bool FULL> __device__ __forceinline__ void taps32(double (&y)[R], const double* tp, int rem, uint32_t wlo, uint32_t whi)
{
    double sd[R];
#pragma unroll
    for (int q = 0; q + 1 < R; ++q) sd[q] = sign_at(wlo, whi, 32 + q);
    sd[R - 1] = 0.0;
#pragma unroll
    for (int u = 0; u < 32; ++u) {
        if (!FULL && u >= rem) break;
#pragma unroll
        for (int r = R - 1; r > 0; --r) sd[r] = sd[r - 1];
        sd[0] = sign_at(wlo, whi, 31 - u);
        const double c = tp[u];
#pragma unroll
        for (int r = 0; r < R; ++r) y[r] = fma(c, sd[r], y[r]);          // c * (+-1.0) is exact: the rounded product, then the add
    }
}

}  // namespace hare_render

extern "C" __global__ __launch_bounds__(kRenderThreads, 4) void hare_hist_render(RenderArgs a)
{
    using namespace hare_render;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int B = a.bands, C = a.channels, M = a.M, T = a.T, nb = a.n_bins;
    const int S = a.tile_bins * M;                                          // the tile's samples: the stride of a band in s_y
    double* const s_taps = (double*)lds;                                   // B x T
    double* const s_y = s_taps + B * T;                                    // B x S
    double* const s_gain = s_y + B * S;                                    // tile_bins x B x C: a * r_ch
    double* const s_a = s_gain + a.tile_bins * B * C;                      // tile_bins x B
    unsigned long long* const s_sign = (unsigned long long*)(s_a + a.tile_bins * B);          // sign_words of 64 bits

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int k = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const int i0 = tile * a.tile_bins, bins = min(a.tile_bins, nb - i0), Sh = bins * M;      // this tile's bins and samples
    const size_t N = (size_t)nb * (size_t)M, n0 = (size_t)i0 * (size_t)M;

    // ---- taps and signs.  Mask bit 64 + j (j = 0 .. Sh + T - 2) is the sign of s(k, n0 + j); sample m of the tile meets tap t at j = m + T - 1 - t
    for (int x = t; x < B * T; x += kRenderThreads) s_taps[x] = a.taps[x];
    const unsigned long long base = scatter_mix(scatter_mix(a.seed + kScatterGamma) ^ (unsigned long long)k);
    const int n_sign = Sh + T - 1;
    for (int w = wv; w < a.sign_words; w += kWaves) {
        const int j = (w - 1) * 64 + lane;
        bool neg = false;
        if (w > 0 && j < n_sign) neg = (scatter_mix(base + ((unsigned long long)n0 + (unsigned long long)j) * kScatterGamma) >> 63) != 0;
        const unsigned long long word = __ballot(neg ? 1 : 0);
        if (lane == 0) s_sign[w] = word;
    }
    __syncthreads();

    // ---- filter: y(k, b, n0 + m) into s_y[b * S + m]
    {
        const int G = (Sh + R - 1) / R, G64 = (G + 63) / 64;              // runs of the tile; wave-loads of runs per band
        for (int wt = wv; wt < B * G64; wt += kWaves) {
            const int b = wt / G64;                                         // wave-uniform
            const int g = (wt % G64) * 64 + lane;
            const int m0 = min(g, G - 1) * R;                               // a lane past the last run repeats it and stores nothing
            const double* const tp = s_taps + b * T;
            double y[R];
#pragma unroll
            for (int r = 0; r < R; ++r) y[r] = -0.0;
            for (int t0 = 0; t0 < T; t0 += 32) {
                const int pos = 64 + m0 + T - 1 - t0 - 31;                  // >= 33: the pad word
                const unsigned long long w0 = s_sign[pos >> 6], w1 = s_sign[(pos >> 6) + 1];
                const int sh = pos & 63;
                const unsigned long long W = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
                const int rem = T - t0;
                if (rem >= 32) taps32<true>(y, tp + t0, 32, (uint32_t)W, (uint32_t)(W >> 32));
                else taps32<false>(y, tp + t0, rem, (uint32_t)W, (uint32_t)(W >> 32));
            }
            if (g < G) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (m0 + r < Sh) s_y[b * S + m0 + r] = y[r];
            }
        }
    }
    __syncthreads();

    // ---- p and a per (bin, band)
    for (int x = t; x < bins * B; x += kRenderThreads) {
        const int il = x / B, b = x % B;
        const double* const yy = s_y + b * S + il * M;
        double p = yy[0] * yy[0];
        for (int j = 1; j < M; ++j) p = p + yy[j] * yy[j];
        const size_t e = (size_t)(i0 + il) * (size_t)B + (size_t)b;
        unsigned long long g = a.hist[((size_t)k * (size_t)nb * (size_t)B + e) * (size_t)C];
        if (a.weight) g = hare_hist::weighted(g, a.weight[e]);
        const double en = ldexp((double)g, -a.frac_bits);
        s_a[x] = (p > 0.0 && en > 0.0) ? sqrt(en / p) : 0.0;
    }
    __syncthreads();

    // ---- gains a * r_ch per (bin, band, channel)
    for (int x = t; x < bins * B * C; x += kRenderThreads) {
        const int ch = x % C, ib = x / C;                                   // ib = il * B + b
        double r = 1.0;
        if (ch) {
            const unsigned long long* const e = a.hist + (((size_t)k * (size_t)nb + (size_t)i0) * (size_t)B + (size_t)ib) * (size_t)C;
            const unsigned long long hW = e[0];
            const long long hc = (long long)e[ch];
            r = hW != 0 ? (double)hc / (double)hW : 0.0;
        }
        s_gain[x] = s_a[ib] * r;
    }
    __syncthreads();

    // ---- output: the bands in order
    for (int ch = 0; ch < C; ++ch) {
        double* const o = a.out + ((size_t)k * (size_t)C + (size_t)ch) * N + n0;
        for (int m = t; m < Sh; m += kRenderThreads) {
            const double* const gn = s_gain + (m / M) * B * C + ch;
            double z = gn[0] * s_y[m];
            for (int b = 1; b < B; ++b) z = z + gn[b * C] * s_y[b * S + m];
            o[m] = z;
        }
    }
}
