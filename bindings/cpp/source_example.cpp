// source_example.cpp -- the C++ mirror's point source: a room of one topology with two receivers and a source that radiates into +x only
// (a cube map of resolution 1: six faces), a burst emitted on the device in one call and in two chunks (the same histogram).
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/source_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_src
// Without a GPU the setter, its checks and the read-backs work; ReceiveSource throws "no HIP device visible".
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
        grid.SetOption("source_seed", 42);
        std::printf("source %lld, bands %lld, res %lld, seed %lld\n", (long long)grid.GetOption("source"), (long long)grid.GetOption("source_bands"),
                    (long long)grid.GetOption("source_res"), (long long)grid.GetOption("source_seed"));
        int refused = 0;
        try { grid.SetSource({1.0, 1.0, 1.0}, {1.0, 0.5}, {}, 1, std::vector<double>(6, 1.0)); } catch (const std::invalid_argument&) { ++refused; }   // short table
        try { grid.SetSource({1.0, 1.0, 1.0}, {1.0, -0.5}); } catch (const std::invalid_argument&) { ++refused; }                                    // negative power
        try { grid.SetSource({1.0, 1.0, 1.0}, std::vector<double>(9, 1.0)); } catch (const std::invalid_argument&) { ++refused; }                   // nine bands
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        std::vector<uint64_t> h, ha, hb, det, da, db;
        grid.ReceiveSource(4096, 0, 0, 1, 16, 0.25, 30, h, det);               // the direct sound only
        grid.ReceiveSource(1000, 0, 0, 1, 16, 0.25, 30, ha, da);
        grid.ReceiveSource(3096, 1000, 0, 1, 16, 0.25, 30, hb, db);
        bool same = true;
        for (size_t w = 0; w < h.size(); ++w) same = same && h[w] == ha[w] + hb[w];
        std::printf("receive: detections front %llu, behind %llu, chunks %s\n", (unsigned long long)det[0], (unsigned long long)det[2],
                    same ? "sum to the one call" : "differ");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
