// reduce_example.cpp -- the C++ mirror's reduction calls (include/hare_hip.h, "receivers", "Reduction") on receivers_example.cpp's scene:
// Receive, HistReduce on its histogram, and ReceiveReduced, which must agree; with air-absorption weights from AirWeights.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/reduce_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_red
// Without a GPU the helpers and the size checks work; the calls throw "no HIP device visible".
#include <cstdio>

#include "hare.hpp"

using namespace Hare::Geometry;

int main()
{
    const double c[8][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}};
    const int f[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 5, 1}, {0, 4, 5}, {3, 2, 6}, {3, 6, 7}, {0, 3, 7}, {0, 7, 4}, {1, 5, 6}, {1, 6, 2}};
    std::vector<double> verts(12 * 12, 0.0);
    std::vector<int32_t> nverts(12, 3);
    for (int p = 0; p < 12; ++p)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts[p * 12 + 3 * k + a] = c[f[p][k]][a];
    Topology t0(verts.data(), nverts.data(), 12), t1(verts.data(), nverts.data(), 12);
    try {
        Voxel_Grid grid({&t0, &t1}, 4);
        grid.SetReceivers({1.0, 0.75, 0.5, 0.5, 0.5, 0.5}, {0.25, 0.125});
        grid.SetAbsorption(1, 8, std::vector<double>(12 * 8, 0.25));
        const int n_bins = 16, B = 8;
        Spatial_Partition::Reduction r;
        r.windows = {0, n_bins, 0, 2, 2, n_bins};
        r.levels = {Spatial_Partition::DecayLevel(-5.0), Spatial_Partition::DecayLevel(-10.0), 0u};
        r.weight = Spatial_Partition::AirWeights(std::vector<double>(B, 0.1), 0.5, n_bins);
        std::printf("levels %u %u, weight %zu: %u %u\n", r.levels[0], r.levels[1], r.weight.size(), r.weight[0], r.weight[(size_t)(n_bins * B - 1)]);
        int refused = 0;
        std::vector<uint64_t> hist(7), sums, det;
        std::vector<int32_t> cross;
        try { grid.HistReduce(hist, 2, n_bins, B, 1, r, sums, cross); } catch (const std::invalid_argument&) { ++refused; }
        Spatial_Partition::Reduction odd = r;
        odd.windows.push_back(3);
        try { grid.HistReduce(std::vector<uint64_t>(2 * n_bins * B), 2, n_bins, B, 1, odd, sums, cross); } catch (const std::invalid_argument&) { ++refused; }
        odd = r;
        odd.weight.pop_back();
        try { grid.HistReduce(std::vector<uint64_t>(2 * n_bins * B), 2, n_bins, B, 1, odd, sums, cross); } catch (const std::invalid_argument&) { ++refused; }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        std::vector<hare_ray> rays;
        for (int k = 0; k < 6; ++k) {
            hare_ray ray{1.0, 0.75, 0.5, 0.0, 0.0, 0.0};
            (&ray.dx)[k / 2] = (k & 1) ? -1.0 : 1.0;
            rays.push_back(ray);
        }
        grid.Receive(rays, 1, 3, n_bins, 0.5, 20, hist, det);
        grid.HistReduce(hist, 2, n_bins, B, 1, r, sums, cross);
        std::vector<uint64_t> sums2, det2;
        std::vector<int32_t> cross2;
        grid.ReceiveReduced(rays, 1, 3, n_bins, 0.5, 20, r, sums2, cross2, det2);
        std::printf("reduce: sums %zu, cross %zu, agree %d\n", sums.size(), cross.size(), (int)(sums == sums2 && cross == cross2 && det == det2));
        std::printf("sums:");
        for (uint64_t v : sums) std::printf(" %llu", (unsigned long long)v);
        std::printf("\ncross:");
        for (int32_t v : cross) std::printf(" %d", v);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
