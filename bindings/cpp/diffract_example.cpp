// diffract_example.cpp -- the C++ mirror's first-order edge diffraction (include/hare_hip.h, "receivers", "Edge diffraction (first order)")
// in direct_example.cpp's room, the cube [0,2]^3, with a screen standing on the floor at x = 1 (one quadrilateral, polygon 12) between an
// omnidirectional source and one receiver.  The receiver lies in the screen's shadow: the direct sound gives it nothing, and DiffractPaths
// gives it one path over each of the screen's three free edges, attenuated by Maekawa's 1 / (3 + 20 N).
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/diffract_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_diffract
// Without a GPU the scratch size, the edge table and the argument checks work; DiffractPaths throws "no HIP device visible".
#include <cstdio>
#include <limits>

#include "hare.hpp"

using namespace Hare::Geometry;

int main()
{
    const double c[8][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}};
    const int f[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 5, 1}, {0, 4, 5}, {3, 2, 6}, {3, 6, 7}, {0, 3, 7}, {0, 7, 4}, {1, 5, 6}, {1, 6, 2}};
    const double screen[4][3] = {{1, 0.5, 0}, {1, 1.5, 0}, {1, 1.5, 1.25}, {1, 0.5, 1.25}};
    std::vector<double> verts(13 * 12, 0.0);
    std::vector<int32_t> nverts(13, 3);
    for (int p = 0; p < 12; ++p)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts[p * 12 + 3 * k + a] = c[f[p][k]][a];
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a) verts[12 * 12 + 3 * k + a] = screen[k][a];
    nverts[12] = 4;
    Topology t0(verts.data(), nverts.data(), 13);
    try {
        Voxel_Grid grid({&t0}, 4);
        grid.SetReceivers({1.625, 1.0, 0.375}, {0.125});
        grid.SetAbsorption(0, 2, std::vector<double>(13 * 2, 0.2));
        grid.SetSource({0.5, 1.0, 0.5}, {1.0, 0.5}, {}, 0, {});
        const std::vector<double> ends = {1, 0.5, 1.25, 1, 1.5, 1.25, 1, 0.5, 0, 1, 0.5, 1.25, 1, 1.5, 0, 1, 1.5, 1.25};      // the top and the two upright edges
        const std::vector<int32_t> faces = {12, -1, 12, -1, 12, -1};
        grid.SetEdges(0, ends, faces, {250.0 / 343.0, 1000.0 / 343.0});
        std::printf("work bytes %lld, edges %lld\n", (long long)Spatial_Partition::DiffractWorkBytes(1, 64), (long long)grid.GetOption("edges"));
        int refused = 0;
        alignas(16) char buf[64];
        const double inf = std::numeric_limits<double>::infinity();
        try { grid.DiffractDevice(0, 0, 16, 0.25, 30, inf, 64, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }        // n_weight 0
        try { grid.DiffractDevice(0, 4096, 16, 0.25, 30, inf, 0, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }     // max_pairs 0
        try { grid.DiffractDevice(0, 4096, 16, 0.25, 30, -1.0, 64, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }   // a negative detour
        try { grid.DiffractDevice(0, 4096, 16, 0.25, 30, inf, 64, nullptr, buf, buf + 32); } catch (const std::invalid_argument&) { ++refused; }     // no scratch
        try { grid.SetEdges(0, ends, {12, -1, 13, -1, 12, -1}, {1.0, 2.0}); } catch (const std::invalid_argument&) { ++refused; }                    // polygon 13 does not exist
        std::printf("refused %d, edges %lld\n", refused, (long long)grid.GetOption("edges"));
        std::fflush(stdout);
        std::vector<uint64_t> h, det, hd, detd;
        const uint64_t found = grid.DiffractPaths(0, 4096, 16, 0.25, 30, inf, 64, h, det, 1, 2);
        grid.SourcePaths(0, 4096, 16, 0.25, 30, hd, detd, 1, 2, false, 1, true, false, false);                                                    // the direct sound alone
        std::printf("diffract: found %llu, detections %llu, direct detections %llu\n", (unsigned long long)found, (unsigned long long)det[0],
                    (unsigned long long)detd[0]);
        std::printf("words:");
        for (size_t w = 0; w < h.size(); ++w) std::printf(" %llu", (unsigned long long)h[w]);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
