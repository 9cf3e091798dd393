// project_channels_example.cpp -- the C++ mirror's directional projection (include/hare_hip.h, "receivers", "Directional projection") on
// project_example.cpp's scene: Receive with four channels per word (HARE_RECEIVE_DIRECTIONAL), then HistProjectChannels on its histogram
// with three vectors -- ones, the bin index and a negative ramp -- with air-absorption weights; its column of channel 0 must equal
// HistProject's result on the same histogram.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/project_channels_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_projc
// Without a GPU the size checks work; the calls throw "no HIP device visible".
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
        const int n_bins = 16, B = 8, J = 3, C = 4;
        std::vector<int32_t> coef((size_t)(J * n_bins));
        for (int i = 0; i < n_bins; ++i) {
            coef[(size_t)i] = 1;
            coef[(size_t)(n_bins + i)] = i;
            coef[(size_t)(2 * n_bins + i)] = -1000 * (i + 1);
        }
        const std::vector<uint32_t> weight = Spatial_Partition::AirWeights(std::vector<double>(B, 0.1), 0.5, n_bins);
        std::printf("coef %zu: %d %d\n", coef.size(), coef[0], coef[(size_t)(J * n_bins - 1)]);
        int refused = 0;
        std::vector<uint64_t> hist(7), proj, w_only, det;
        try { grid.HistProjectChannels(hist, 2, n_bins, B, C, coef, proj, weight); } catch (const std::invalid_argument&) { ++refused; }
        hist.assign((size_t)(2 * n_bins * B * C), 0);
        try { grid.HistProjectChannels(hist, 2, n_bins, B, C, std::vector<int32_t>(n_bins + 1), proj, weight); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.HistProjectChannels(hist, 2, n_bins, B, C, coef, proj, std::vector<uint32_t>(5)); } catch (const std::invalid_argument&) { ++refused; }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        std::vector<hare_ray> rays;
        for (int k = 0; k < 6; ++k) {
            hare_ray ray{1.0, 0.75, 0.5, 0.0, 0.0, 0.0};
            (&ray.dx)[k / 2] = (k & 1) ? -1.0 : 1.0;
            rays.push_back(ray);
        }
        grid.Receive(rays, 1, 3, n_bins, 0.5, 20, hist, det, nullptr, nullptr, false, true);          // directional: four channels
        grid.HistProjectChannels(hist, 2, n_bins, B, C, coef, proj, weight);
        grid.HistProject(hist, 2, n_bins, B, C, coef, w_only, weight);
        bool agree = hist.size() == (size_t)(2 * n_bins * B * C) && proj.size() == (size_t)(2 * B * J * C * 2) && w_only.size() == (size_t)(2 * B * J * 2);
        for (size_t kbj = 0; agree && kbj < (size_t)(2 * B * J); ++kbj)
            for (size_t w = 0; w < 2; ++w) agree = agree && proj[kbj * C * 2 + w] == w_only[kbj * 2 + w];          // channel 0: lo, hi
        std::printf("project_channels: proj %zu, agree %d\n", proj.size(), (int)agree);
        std::printf("proj:");
        for (uint64_t v : proj) std::printf(" %llu", (unsigned long long)v);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
