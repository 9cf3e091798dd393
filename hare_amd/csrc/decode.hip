// decode.hip -- hare_decode: K x C rows of N doubles (the rows hare_hist_render writes: ambisonic channels per receiver) decoded to K x O
// rows through a matrix of O x C FIR filters of T doubles; a window [n0, n0 + n_out) of the N + T - 1 samples is written
// (include/hare_hip.h, "receivers", "Decoding").  #included from kernels.hip behind convolve.hip, whose tile, pad() and block forms it
// takes over.  FP64, no contraction: the product is rounded, then the add, and every output is ONE sequential sum from +0.0 over the
// input channels c ascending and, within a channel, over the taps t ascending (tests/decode_ref.py restates it in numpy).  Parallelism
// is over (k, o, output) only.
//
// Tiling.  A workgroup of 256 threads owns one (k, o) and kDecodeTile = 2048 consecutive outputs, a run of P = 8 to a lane, the 16
// accumulator registers of the run live from the first term of channel 0 to the store.  The roles of convolve.hip: the broadcast taps are
// the filter h[o, c, .], the lane's sliding window runs over in[k, c, .] -- the long operand fills the waves' windows, so that a filter of
// 32 taps or more reaches the interior path.  The channel loop goes AROUND the chunk loop: per channel the taps the tile meets --
// max(0, nb - (N - 1)) .. min(T - 1, last output), the same for every channel -- go by in chunks of 256, the chunk's taps and the
// 2048 + 255 samples of in[k, c] they meet staged in LDS (the samples padded by a word after every 8), and nothing else is read from memory.
// A wave takes a chunk in blocks of 32 taps, each nothing, interior (32 x 8 multiply-add pairs and nothing else) or edge (each output's
// own test 0 <= n - t < N; a term out of range is SKIPPED, never formed against a zero), in ascending t whatever their kind.
//
// No scratch, no VGPR spilled, no fused multiply-add (tests/test_decode_kernel_resources.py).  Nothing outside in[k, .], h[o, .] and the
// tile's own outputs is touched: the staging tests every index, and the slots it cannot fill hold 0.0 that no sum reads.
namespace hare_dec {

using hare_conv::pad;
constexpr int P = kDecodeRun, CH = kDecodeChunk, U = kDecodeBlock, TILE = kDecodeTile, WAVE_OUT = 64 * P;
constexpr int STAGE = (TILE + CH - 1 + kDecodeThreads - 1) / kDecodeThreads;          // samples a lane stages per chunk: 9
static_assert(TILE == kDecodeThreads * P && CH == kDecodeThreads && CH % U == 0 && U % 8 == 0 && P <= 8, "decode.hip: tile");
static_assert(kDecodeLdsDoubles >= CH + 9 * ((TILE + CH + 7) / 8), "decode.hip: LDS");

}  // namespace hare_dec

extern "C" __global__ __launch_bounds__(kDecodeThreads, 4) void hare_decode(DecodeArgs a)
{
#pragma clang fp contract(off)          // the definition's: a multiply, then an add, whatever the build's flags say
    using namespace hare_dec;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double* const s_h = (double*)lds;                                      // CH taps: h[o, c, tc ..]
    double* const s_x = s_h + CH;                                          // TILE + CH - 1 samples, padded: sample j is in[k, c, nb - tc - (CH - 1) + j]

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ko = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const int k = ko / a.O, o = ko % a.O;
    const int C = a.C, N = a.N, T = a.T;
    const int nb = a.n0 + tile * TILE;                                      // the tile's first output sample
    const int n_end = min(nb + TILE, a.n0 + a.n_out);                       // one past its last
    const int t_first = max(0, nb - (N - 1)), t_last = min(T - 1, n_end - 1);          // the taps any output of the tile meets, whatever the channel
    const int m0 = tid * P;                                                 // the lane's first output, within the tile
    const int nw = nb + wv * WAVE_OUT;                                      // the wave's first output sample
    const double* x = a.in + (size_t)k * (size_t)C * (size_t)N;           // in[k, c, .], c = 0
    const double* h = a.h + (size_t)o * (size_t)C * (size_t)T;            // h[o, c, .], c = 0

    double acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.0;

    for (int c = 0; c < C; ++c, x += N, h += T) {
        for (int tc = t_first; tc <= t_last; tc += CH) {
            // the lane's STAGE samples and its tap are requested together, before the barrier, and stored behind it: one memory latency per
            // chunk, not one per sample (unlike the convolution's one signal, in[k, c] is new to the cache for every tile and channel)
            const int xs0 = nb - tc - (CH - 1);
            double v[STAGE];
#pragma unroll
            for (int i = 0; i < STAGE; ++i) {
                const int j = tid + i * kDecodeThreads, xi = xs0 + j;
                v[i] = (j < TILE + CH - 1 && xi >= 0 && xi < N) ? x[xi] : 0.0;
            }
            const double g0 = tc + tid <= t_last ? h[tc + tid] : 0.0;
            __syncthreads();                                                // the chunk before has been read
            s_h[tid] = g0;
#pragma unroll
            for (int i = 0; i < STAGE; ++i) {
                const int j = tid + i * kDecodeThreads;
                if (j < TILE + CH - 1) s_x[pad(j)] = v[i];
            }
            __syncthreads();

            for (int ub = 0; ub < CH; ub += U) {
                const int tb = tc + ub;                                     // the block's first tap
                if (tb > t_last) break;
                if (tb > nw + WAVE_OUT - 1 || nw - (tb + U - 1) > N - 1) continue;          // nothing: n - t < 0, or > N - 1, for the whole wave
                if (tb + U - 1 <= t_last && nw - (tb + U - 1) >= 0 && nw + WAVE_OUT - 1 - tb <= N - 1) {
                    // interior.  Output m0 + p meets tap ub + u at sample j = 8 tid + (CH - U - ub) + d, d = U - 1 - u + p in 0 .. U + P - 2
                    const double* const xb = s_x + 9 * (tid + (CH - U - ub) / 8);
                    const double* const cp = s_h + ub;
                    double w[P];
#pragma unroll
                    for (int p = 0; p < P; ++p) w[p] = xb[pad(U - 1 + p)];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double g = cp[u];
#pragma unroll
                        for (int p = 0; p < P; ++p) acc[p] = acc[p] + g * w[p];
                        if (u + 1 < U) {
#pragma unroll
                            for (int p = P - 1; p > 0; --p) w[p] = w[p - 1];
                            w[0] = xb[pad(U - 2 - u)];
                        }
                    }
                } else {
                    // edge: each output's own range
                    for (int u = 0; u < U && tb + u <= t_last; ++u) {
                        const double g = s_h[ub + u];
                        const int xi0 = nb + m0 - (tb + u), j0 = m0 + CH - 1 - ub - u;
#pragma unroll
                        for (int p = 0; p < P; ++p)
                            if (xi0 + p >= 0 && xi0 + p < N) acc[p] = acc[p] + g * s_x[pad(j0 + p)];
                    }
                }
            }
        }
    }

    double* const y = a.y + (size_t)ko * (size_t)a.n_out + (size_t)(nb - a.n0);
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (nb + m0 + p < n_end) y[m0 + p] = acc[p];
}
