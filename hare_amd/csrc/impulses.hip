// impulses.hip -- hare_hist_impulses: a receive histogram whose bin is one output sample turned, on the device, into pressure rows
// (include/hare_hip.h, "receivers", "Impulses"): every (bin, band) whose weighted W word g is not zero is an ENTRY, an impulse of amplitude
// a = sqrt(g * 2^-frac_bits) at sample `bin`, filtered by the band's FIR taps and weighted per channel by the rendering's ratio
// r_ch = h_ch / h_W.  #included from kernels.hip behind render.hip.  FP64, no contraction: the product is rounded, then the add, and every
// output is ONE sequential sum from +0.0 over the bands ascending and, within a band, over the entries in ascending bin
// (tests/impulse_ref.py restates it in numpy).  Bins without an entry and taps out of range add NO term.  Parallelism is over
// (k, output sample) only; a lane carries its sample's sums of all channels.
//
// The input is sparse -- some paths among n_bins x B words -- and the kernel is built for that: what scales with the histogram is a scan
// of one word per (bin, band); what scales with the taps is paid per entry.
//
// Tiling.  A workgroup of 256 threads owns one receiver and kImpulseTile = 256 consecutive outputs of ALL channels, an output to a lane,
// `channels` accumulators in registers (the kernel body is compiled once per channel count).  The taps (B x T doubles) are staged once.
// Bands outer, ascending; the bins that reach the tile, max(0, nb - (T - 1)) .. min(n_bins - 1, last output), inner, ascending, in chunks of
// 256, a bin to a thread:
//   scan     the thread reads its bin's W word (and weight) and decides g != 0; a ballot and a count of the set bits below the lane place
//            the wave's entries, the waves' totals (LDS) place the waves: the chunk's entries land in an LDS list IN ASCENDING BIN ORDER
//            with their bin, a and W word.  Order-preserving compaction is what keeps the order of the sum.
//   gains    a thread per (entry, channel): r_ch from the histogram's signed word, a * r_ch into LDS -- one division per entry and
//            channel, whatever the number of outputs the entry reaches.
//   walk     every lane walks the list.  The entry's bin is wave-uniform (an entry no output of the wave can meet is skipped by the whole
//            wave), its gains are LDS broadcasts, the tap taps[b][n - bin] a read at consecutive addresses across the lanes: one range
//            test per entry and lane, then `channels` multiply-add pairs.
// The list is per chunk, so nothing scales with the number of entries: a histogram with every bin an entry costs what the dense sum costs.
//
// No scratch, no VGPR spilled, no fused multiply-add (tests/test_impulse_kernel_resources.py).  Nothing outside hist[k], the weights, the
// taps and the tile's own outputs is touched: a thread past the scan's last bin reads nothing and holds no entry, a lane past the window's
// last sample accumulates and stores nothing, and the words from n_out to out_stride of a row are never addressed.
namespace hare_imp {

constexpr int kWaves = kImpulseThreads / 64;

// The square root and the division are correctly rounded sequences that the compiler builds from fused multiply-adds.  They are kept out
// of the kernel's body, functions of their own, so that the body holds FP64 multiplies and adds alone and a contraction of the sum's
// multiply and add would show there (tests/test_impulse_kernel_resources.py)
__device__ __attribute__((noinline)) double amplitude(unsigned long long g, int frac_bits)
{
    return sqrt(ldexp((double)g, -frac_bits));
}
__device__ __attribute__((noinline)) double ratio(long long hc, unsigned long long hW)
{
    return (double)hc / (double)hW;
}

template <int C> __device__ __forceinline__ void run(const ImpulseArgs& a, unsigned char* lds)
{
#pragma clang fp contract(off)          // the definition's: a multiply, then an add, whatever the build's flags say
    const int B = a.bands, T = a.T, nbins = a.n_bins;
    double* const s_taps = (double*)lds;                                   // B x T
    double* const s_gain = s_taps + B * T;                                 // list slot x C: a * r_ch
    double* const s_a = s_gain + kImpulseChunk * C;                        // list slot: a
    unsigned long long* const s_hw = (unsigned long long*)(s_a + kImpulseChunk);          // list slot: the W word
    int* const s_bin = (int*)(s_hw + kImpulseChunk);                       // list slot: the bin
    int* const s_cnt = s_bin + kImpulseChunk;                              // entries per wave of the chunk

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const int nb = a.n0 + tile * kImpulseTile;                              // the tile's first output sample
    const int n_end = min(nb + kImpulseTile, a.n0 + a.n_out);               // one past its last
    const int scan_lo = max(0, nb - (T - 1)), scan_hi = min(nbins - 1, n_end - 1);          // the bins any output of the tile meets
    const int n = nb + tid;                                                 // the lane's output sample
    const bool active = n < n_end;
    const int nw_lo = nb + wv * 64, nw_hi = min(nw_lo + 63, n_end - 1);     // the wave's outputs (none: nw_hi < nw_lo)
    const unsigned long long* const hk = a.hist + (size_t)k * (size_t)nbins * (size_t)B * (size_t)C;

    for (int x = tid; x < B * T; x += kImpulseThreads) s_taps[x] = a.taps[x];

    double acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0;

    for (int b = 0; b < B; ++b) {
        const double* const tp = s_taps + b * T;
        for (int c0 = scan_lo; c0 <= scan_hi; c0 += kImpulseChunk) {
            // ---- scan: a bin to a thread
            const int i = c0 + tid;
            unsigned long long hW = 0, g = 0;
            if (i <= scan_hi) {
                const size_t e = (size_t)i * (size_t)B + (size_t)b;
                hW = hk[e * (size_t)C];
                g = a.weight ? hare_hist::weighted(hW, a.weight[e]) : hW;
            }
            const unsigned long long vote = __ballot(g != 0 ? 1 : 0);
            const int below = __popcll(vote & ((1ull << lane) - 1ull));
            if (lane == 0) s_cnt[wv] = __popcll(vote);
            __syncthreads();                                                // the counts are there; the chunk before has been walked
            int at = below, n_ent = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const int c = s_cnt[w];
                if (w < wv) at += c;
                n_ent += c;
            }
            if (g != 0) {
                s_bin[at] = i;
                s_hw[at] = hW;
                s_a[at] = amplitude(g, a.frac_bits);
            }
            __syncthreads();
            // ---- gains: a thread per (entry, channel)
            for (int x = tid; x < n_ent * C; x += kImpulseThreads) {
                const int e = x / C, ch = x - e * C;
                double r = 1.0;
                if (ch) {
                    const long long hc = (long long)hk[((size_t)s_bin[e] * (size_t)B + (size_t)b) * (size_t)C + (size_t)ch];
                    r = ratio(hc, s_hw[e]);
                }
                s_gain[x] = s_a[e] * r;
            }
            __syncthreads();
            // ---- walk: the list in order
            for (int e = 0; e < n_ent; ++e) {
                const int ei = __builtin_amdgcn_readfirstlane(s_bin[e]);
                if (ei > nw_hi || ei + (T - 1) < nw_lo) continue;           // no output of this wave meets the entry
                const int d = n - ei;
                if (active && d >= 0 && d < T) {
                    const double tap = tp[d];
                    const double* const gn = s_gain + e * C;
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) acc[ch] = acc[ch] + gn[ch] * tap;
                }
            }
        }
    }

    if (active) {
        double* const o = a.out + (size_t)k * (size_t)C * (size_t)a.out_stride + (size_t)(n - a.n0);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            double* const p = o + (size_t)ch * (size_t)a.out_stride;
            *p = a.add ? *p + acc[ch] : acc[ch];
        }
    }
}

}  // namespace hare_imp

extern "C" __global__ __launch_bounds__(kImpulseThreads) void hare_hist_impulses(ImpulseArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    switch (a.channels) {
    case 1: hare_imp::run<1>(a, lds); break;
    case 4: hare_imp::run<4>(a, lds); break;
    case 9: hare_imp::run<9>(a, lds); break;
    default: hare_imp::run<16>(a, lds); break;
    }
}
