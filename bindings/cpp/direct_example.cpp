// direct_example.cpp -- the C++ mirror's direct sound (include/hare_hip.h, "receivers", "Direct sound") on source_example.cpp's room: a
// source that radiates into +x only, a receiver in front of it and one behind it.  With HARE_RECEIVE_DIRECT a one-cast call is the deposit
// alone: one add per receiver the source sees (of zero energy behind it), the same whatever the seed, and f * n of the burst's power
// instead of a count that fluctuates.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/direct_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_direct
// Without a GPU the flag, the scratch size and the argument checks work; ReceiveSource throws "no HIP device visible".
#include <cstdio>

#include "hare.hpp"

using namespace Hare::Geometry;

int main()
{
    // the cube [0,2]^3 as 12 triangles
    const double c[8][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}};
    const int f[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 5, 1}, {0, 4, 5}, {3, 2, 6}, {3, 6, 7}, {0, 3, 7}, {0, 7, 4}, {1, 5, 6}, {1, 6, 2}};
    std::vector<double> verts(12 * 12, 0.0);
    std::vector<int32_t> nverts(12, 3);
    for (int p = 0; p < 12; ++p)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts[p * 12 + 3 * k + a] = c[f[p][k]][a];
    Topology t0(verts.data(), nverts.data(), 12);
    try {
        Voxel_Grid grid({&t0}, 4);
        grid.SetReceivers({1.5, 1.0, 1.0, 0.5, 1.0, 1.0}, {0.25, 0.25});        // receiver 0 on the source's +x side, receiver 1 behind it
        grid.SetAbsorption(0, 2, std::vector<double>(12 * 2, 0.2));
        std::vector<double> gain(6 * 2, 0.0);
        gain[0] = gain[1] = 1.0;                                               // face 0 (+x), both bands
        grid.SetSource({1.0, 1.0, 1.0}, {1.0, 0.5}, {}, 1, gain);
        std::printf("flag %u, work bytes %lld\n", HARE_RECEIVE_DIRECT, (long long)Spatial_Partition::DirectWorkBytes(2));
        int refused = 0;
        char buf[64];
        try { grid.DirectDevice(0, 0, 16, 0.25, 30, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }        // n_weight 0
        try { grid.DirectDevice(0, 4096, 16, 0.25, 30, nullptr, buf, buf + 32); } catch (const std::invalid_argument&) { ++refused; }      // no scratch
        try {                                                                                                                              // the caller's rays
            std::vector<hare_ray> rays(1, hare_ray{1.0, 1.0, 1.0, 1.0, 0.0, 0.0});
            std::vector<uint64_t> hist(2 * 16 * 2), det(4);
            hare_counters ctr{};
            if (hare_receive_batch(grid.native(), HARE_KIND_VOXEL, 0, 1, rays.data(), nullptr, nullptr, 1, HARE_RECEIVE_DIRECT, 16, 0.25, 30, nullptr,
                                   nullptr, hist.data(), det.data(), &ctr) == HARE_E_INVALID)
                ++refused;
        } catch (const std::exception&) {
        }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        const int64_t n = 4096;
        std::vector<uint64_t> h, det, h2, det2, hs, dets;
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, h, det, nullptr, false, false, true);          // one cast with the flag: the deposit alone
        grid.SetOption("source_seed", 42);
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, h2, det2, nullptr, false, false, true);        // no ray of the burst enters it
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, hs, dets);                                     // the sampled direct sound
        // receiver 0: dist 0.5 (bin 2), x = rr / d2 = 0.25, f = (1 - sqrt(0.75)) / 2; band 0 holds f * n * 2^30, band 1 half of it
        std::printf("direct: detections front %llu, behind %llu, seeds %s\n", (unsigned long long)det[0], (unsigned long long)det[2],
                    h == h2 && det == det2 ? "agree" : "differ");
        std::printf("words: %llu %llu\n", (unsigned long long)h[(0 * 16 + 2) * 2 + 0], (unsigned long long)h[(0 * 16 + 2) * 2 + 1]);
        std::printf("sampled: detections front %llu, behind %llu\n", (unsigned long long)dets[0], (unsigned long long)dets[2]);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
