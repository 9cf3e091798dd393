// direct.hip -- hare_direct_emit, hare_direct_deposit, hare_direct_deposit_dir: the direct sound (include/hare_hip.h, "receivers", "Direct
// sound"), #included from kernels.hip behind deposit.hip, whose vector (path_vector) and deposit (deposit_tail) it shares with the image
// sources.
//
// One lane per RECEIVER (K <= 65 536: at most 256 workgroups), three short launches per call (receive.cpp: direct_enqueue): the emission
// writes each receiver's shadow ray from the source to its center; the flags-only occlusion kernels of the call's partition answer it -- no
// traversal code here; the deposit adds the words of the receivers the source sees.  Position, power and frame are by-value arguments, as in
// hare_emit_source.  Each histogram word and each detection counter is touched by one lane of the deposit.  Bit-exact with tests/direct_ref.py.

// A slot without a query (the source inside the sphere, or a NaN) is marked -2, which the occlusion kernels skip under
// HARE_SHOOT_RETIRED_RAYS (no traversal, flag 0), as hare_rain_step marks its own
extern "C" __global__ __launch_bounds__(256) void hare_direct_emit(DirectArgs da)
{
    const DepositArgs& a = da.d;
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= a.n_rcv) return;
    const double* const rc = a.rcv + 4 * (size_t)k;
    double vx, vy, vz;
    const double d2 = path_vector(rc[0], rc[1], rc[2], a.pos[0], a.pos[1], a.pos[2], vx, vy, vz);
    RayRec s;
    s.x = a.pos[0]; s.y = a.pos[1]; s.z = a.pos[2];
    s.dx = vx; s.dy = vy; s.dz = vz;
    a.srays[k] = s;
    a.stmax[k] = 1.0;
    a.sexcl[k] = d2 > rc[3] ? -1 : -2;
}

template <int C>
static __device__ __forceinline__ void direct_deposit_body(const DepositArgs& a)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= a.n_rcv) return;
    if (a.sexcl[k] == -2 || a.socc[k] != 0) return;             // not eligible, or the source does not see the center
    // the source's ray to the center is the path's own vector (the emission's: the same operations); no wall, reflectance 1.0
    deposit_tail<C>(a, k, a.pos[0], a.pos[1], a.pos[2], [](double&, double&, double&) {}, [](int) { return 1.0; });
}

#define HARE_DIRECT_DEPOSIT_KERNEL(SUFFIX, C)                                                   \
    extern "C" __global__ __launch_bounds__(256) void hare_direct_deposit##SUFFIX(DirectArgs a) \
    {                                                                                           \
        direct_deposit_body<C>(a.d);                                                            \
    }
HARE_CHANNEL_FORMS(HARE_DIRECT_DEPOSIT_KERNEL)
#undef HARE_DIRECT_DEPOSIT_KERNEL
