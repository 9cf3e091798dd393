// convolve.hip -- hare_convolve: R rows of N doubles (the rows hare_hist_render writes, or any others), each convolved in the time domain
// with one dry signal of L doubles; a window [n0, n0 + n_out) of the N + L - 1 samples of the full convolution is written
// (include/hare_hip.h, "receivers", "Convolution").  #included from kernels.hip.  FP64, no contraction: the product is rounded, then the
// add, and every output is ONE sequential sum over its taps in ascending order from +0.0 (tests/convolve_ref.py restates it in numpy).
// Parallelism is over (row, output) only.
//
// Tiling.  A workgroup of 256 threads owns one row and kConvolveTile = 2048 consecutive outputs, a run of P = 8 to a lane, the 16 accumulator
// registers of the run live from the first tap to the store.  The taps the tile meets -- max(0, nb - (L - 1)) .. min(N - 1, last output) --
// go by in chunks of kConvolveChunk = 256: the chunk's taps and the 2048 + 255 samples of x they meet are staged in LDS (x padded by a word
// after every 8, so that lanes 8 samples apart read distinct banks: stride 18 dwords over 64 banks), and nothing else is read from memory.
//
//   block     a wave takes the chunk in blocks of 32 taps and decides PER BLOCK, with scalar compares, which of three things it is:
//     nothing   no tap of the block is in range for any of the wave's 512 outputs: skipped
//     interior  every tap is in range for every output: 32 x 8 multiply-add pairs and nothing else.  The lane's window of x -- 8 samples --
//               slides through the accumulators as t advances: one new LDS read per tap and lane, one broadcast read of the tap per wave
//     edge      the first and last blocks of a tile's range: tap by tap, each output's own test 0 <= n - t < L.  A term out of range is
//               SKIPPED, never formed against a zero: a NaN or an infinity reaches exactly the outputs whose range holds it
//   Blocks go by in ascending t whatever their kind, so the order of each sum is the header's.
//
// No scratch, no VGPR spilled, no fused multiply-add (tests/test_convolve_kernel_resources.py).  Nothing outside ir[row], x and the
// tile's own outputs is touched: the staging tests every index, and the slots it cannot fill hold 0.0 that no sum reads.
namespace hare_conv {

constexpr int P = kConvolveRun, CH = kConvolveChunk, U = kConvolveBlock, TILE = kConvolveTile, WAVE_OUT = 64 * P;
static_assert(TILE == kConvolveThreads * P && CH == kConvolveThreads && CH % U == 0 && U % 8 == 0 && P <= 8, "convolve.hip: tile");

// where sample j of the staged segment of x lies: a pad word after every 8
__device__ __forceinline__ constexpr int pad(int j) { return j + (j >> 3); }

}  // namespace hare_conv

extern "C" __global__ __launch_bounds__(kConvolveThreads, 4) void hare_convolve(ConvolveArgs a)
{
#pragma clang fp contract(off)          // the definition's: a multiply, then an add, whatever the build's flags say
    using namespace hare_conv;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double* const s_ir = (double*)lds;                                     // CH taps: ir[tc ..]
    double* const s_x = s_ir + CH;                                         // TILE + CH - 1 samples, padded: sample j is x[nb - tc - (CH - 1) + j]

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const int N = a.N, L = a.L;
    const int nb = a.n0 + tile * TILE;                                      // the tile's first output sample
    const int n_end = min(nb + TILE, a.n0 + a.n_out);                       // one past its last
    const int t_first = max(0, nb - (L - 1)), t_last = min(N - 1, n_end - 1);          // the taps any output of the tile meets
    const int m0 = tid * P;                                                 // the lane's first output, within the tile
    const int nw = nb + wv * WAVE_OUT;                                      // the wave's first output sample
    const double* const ir = a.ir + (size_t)r * (size_t)N;

    double acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.0;

    for (int tc = t_first; tc <= t_last; tc += CH) {
        __syncthreads();                                                    // the chunk before has been read
        s_ir[tid] = tc + tid <= t_last ? ir[tc + tid] : 0.0;
        const int xs0 = nb - tc - (CH - 1);
        for (int j = tid; j < TILE + CH - 1; j += kConvolveThreads) {
            const int xi = xs0 + j;
            s_x[pad(j)] = (xi >= 0 && xi < L) ? a.x[xi] : 0.0;
        }
        __syncthreads();

        for (int ub = 0; ub < CH; ub += U) {
            const int tb = tc + ub;                                         // the block's first tap
            if (tb > t_last) break;
            if (tb > nw + WAVE_OUT - 1 || nw - (tb + U - 1) > L - 1) continue;          // nothing: n - t < 0, or > L - 1, for the whole wave
            if (tb + U - 1 <= t_last && nw - (tb + U - 1) >= 0 && nw + WAVE_OUT - 1 - tb <= L - 1) {
                // interior.  Output m0 + p meets tap ub + u at sample j = 8 tid + (CH - U - ub) + d, d = U - 1 - u + p in 0 .. U + P - 2
                const double* const xb = s_x + 9 * (tid + (CH - U - ub) / 8);
                const double* const cp = s_ir + ub;
                double w[P];
#pragma unroll
                for (int p = 0; p < P; ++p) w[p] = xb[pad(U - 1 + p)];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double c = cp[u];
#pragma unroll
                    for (int p = 0; p < P; ++p) acc[p] = acc[p] + c * w[p];
                    if (u + 1 < U) {
#pragma unroll
                        for (int p = P - 1; p > 0; --p) w[p] = w[p - 1];
                        w[0] = xb[pad(U - 2 - u)];
                    }
                }
            } else {
                // edge: each output's own range
                for (int u = 0; u < U && tb + u <= t_last; ++u) {
                    const double c = s_ir[ub + u];
                    const int xi0 = nb + m0 - (tb + u), j0 = m0 + CH - 1 - ub - u;
#pragma unroll
                    for (int p = 0; p < P; ++p)
                        if (xi0 + p >= 0 && xi0 + p < L) acc[p] = acc[p] + c * s_x[pad(j0 + p)];
                }
            }
        }
    }

    double* const y = a.y + (size_t)r * (size_t)a.n_out + (size_t)(nb - a.n0);
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (nb + m0 + p < n_end) y[m0 + p] = acc[p];
}
