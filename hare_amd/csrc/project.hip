// project.hip -- hare_hist_project: a receive histogram projected, on the device, onto up to 32 caller-supplied integer vectors over the
// bins (include/hare_hip.h, "receivers", "Projection"): per receiver k, band b and vector j the exact signed sum
// P(k, b, j) = sum over i of c_j[i] * g(k, i, b) as a 128-bit two's-complement integer.  #included from kernels.hip behind hist_block.h,
// whose 128-bit pieces, band totals and layout it shares with hare_hist_reduce: Block, a workgroup of 256 threads per receiver, a thread on
// ONE band and one bin of every tile, and Block::g4, this kernel's loader: four tiles' words in flight, no branch.  Integer arithmetic
// only: the result is a function of the inputs, bit for bit (tests/project_ref.py restates it in Python integers).
//
//   signs    c * g is signed 32 x unsigned 64.  The kernel multiplies by the OFFSET coefficient c' = c + 2^31 (one xor of the top bit), which
//            is an unsigned 32-bit number: U_j = sum c'_j[i] * g is a sum of unsigned 96-bit products (U_j < 2^32 * 2^91), and with
//            T = sum g, formed once, P_j = U_j - 2^31 * T  (mod 2^128): the two's-complement result.  No sign test, no select and no
//            signed carry in the loop.
//   product  the accumulator is kept as two 32-bit limbs and a 64-bit top (Acc).  g_lo * c' + a0 and g_hi * c' + a1 + carry both fit
//            64 bits ((2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1), so each is ONE v_mad_u64_u32 with its addend, and the top takes one 64-bit
//            add: per word and vector two multiply-adds and two 64-bit adds, no compare for a carry.
//   sweeps   up to kGroup = 8 vectors per sweep over the block: 8 x 4 accumulator dwords in registers; J = 29 takes four sweeps (8, 8, 8,
//            5), the later ones served from L2 (the block is 64 KiB at n_bins = 1 024, B = 8).  The sweep is compiled once per vector count
//            1 .. 8: no branch in the loop, a sweep does the arithmetic of its own vectors only, and the coefficient loads of four tiles
//            are issued together, in front of the arithmetic.
//   coef     read through the vector cache, not staged in LDS: the B lanes of a bin share c_j[i] (one address), a wave reads 64 / B
//            consecutive dwords per vector and tile, and all K workgroups read the same J x n_bins table, which stays in L2.  No barrier
//            in the loop.
//   sums     the threads of a band are summed by the wave scan at lane stride B (the last B lanes of a wave hold its B totals) and four LDS
//            words per band and quantity; thread (u, b) writes vector j0 + u of band b: every output word once, no atomics.
//
// No scratch, no VGPR spilled (tests/test_project_kernel_resources.py); LDS 4 736 bytes, static.  Nothing depends on the grid beyond
// blockIdx.x = k.  K = 1 with a huge n_bins runs on this one workgroup: a host-sized problem, and not what the kernel is for.
namespace hare_project {

using namespace hare_hist;
constexpr int kGroup = kProjectGroup;           // vectors per sweep, at most

struct Acc {                                    // a 128-bit unsigned sum: bits 0 .. 31, 32 .. 63, 64 .. 127
    uint32_t a0, a1;
    unsigned long long a23;
};
// acc += x * m, the product 96 bits
__device__ __forceinline__ void mul_add(Acc& acc, unsigned long long x, uint32_t m)
{
    const unsigned long long p0 = (x & 0xFFFFFFFFull) * m + acc.a0;
    const unsigned long long p1 = (x >> 32) * m + ((p0 >> 32) + (unsigned long long)acc.a1);
    acc.a0 = (uint32_t)p0;
    acc.a1 = (uint32_t)p1;
    acc.a23 += p1 >> 32;
}

// One sweep over the block for the N vectors at c0 (vector-major, n_bins apart): the thread's sums U_u of c'_u[i] * g into s_tot[1 + u],
// and with WANT_T its sum of g into s_tot[0]; per wave and band
template <int N> __device__ __forceinline__ void sweep(const Block& k, const int32_t* c0, bool want_T, U128 (*s_tot)[4][kMaxBands], int lane, int wv)
{
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
            const int32_t* const cq = c0 + min((tile + q) * k.step + k.li, k.nb - 1);      // past the end g is 0: any coefficient serves
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
    if (want_T) {
        const U128 s = wave_scan(T, k.B, lane);
        if (lane >= 64 - k.B) s_tot[0][wv][k.b] = s;
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const U128 s = wave_scan(make128((unsigned long long)U[u].a0 | ((unsigned long long)U[u].a1 << 32), U[u].a23), k.B, lane);
        if (lane >= 64 - k.B) s_tot[1 + u][wv][k.b] = s;
    }
}

}  // namespace hare_project

extern "C" __global__ __launch_bounds__(256) void hare_hist_project(ProjectArgs a)
{
    using namespace hare_project;
    __shared__ U128 s_tot[1 + kGroup][4][kMaxBands];   // T, then U per vector of the sweep; per wave and band: the wave's total
    __shared__ U128 s_T[kMaxBands];                     // 2^31 * T per band, from the first sweep on

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int J = a.n_vec;
    const Block k = block_of(a.hist, a.weight, a.n_bins, a.bands, a.channels);
    const int b = k.b, li = k.li;

    for (int j0 = 0; j0 < J; j0 += kGroup) {
        const int n_act = min(kGroup, J - j0);                                // vectors of this sweep
        const bool want_T = j0 == 0;
        const int32_t* const c0 = a.coef + (size_t)j0 * (size_t)k.nb;
        switch (n_act) {                                                       // uniform
        case 8: sweep<8>(k, c0, want_T, s_tot, lane, wv); break;
        case 7: sweep<7>(k, c0, want_T, s_tot, lane, wv); break;
        case 6: sweep<6>(k, c0, want_T, s_tot, lane, wv); break;
        case 5: sweep<5>(k, c0, want_T, s_tot, lane, wv); break;
        case 4: sweep<4>(k, c0, want_T, s_tot, lane, wv); break;
        case 3: sweep<3>(k, c0, want_T, s_tot, lane, wv); break;
        case 2: sweep<2>(k, c0, want_T, s_tot, lane, wv); break;
        default: sweep<1>(k, c0, want_T, s_tot, lane, wv); break;
        }
        __syncthreads();
        if (want_T && t < k.B) {
            const U128 s = band_total(s_tot[0], t);
            s_T[t] = make128(s.lo << 31, (s.hi << 31) | (s.lo >> 33));        // T < 2^91: nothing is shifted out
        }
        __syncthreads();
        if (t < kGroup * k.B && li < n_act) {                                  // thread (u, b) = (li, b): vector j0 + u of band b
            // band_total, written out: through the helper the compiler orders this tail's LDS reads and adds differently, and the
            // kernel's instruction stream is kept as it was measured
            const U128 s = add128(add128(s_tot[1 + li][0][b], s_tot[1 + li][1][b]), add128(s_tot[1 + li][2][b], s_tot[1 + li][3][b]));
            const U128 p = sub128(s, s_T[b]);                                  // mod 2^128: the two's complement of a negative sum
            unsigned long long* out = a.proj + (((size_t)blockIdx.x * (size_t)k.B + (size_t)b) * (size_t)J + (size_t)(j0 + li)) * 2;
            out[0] = p.lo;
            out[1] = p.hi;
        }
        __syncthreads();
    }
}
