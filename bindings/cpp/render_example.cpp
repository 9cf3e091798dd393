// render_example.cpp -- the C++ mirror's rendering call (include/hare_hip.h, "receivers", "Rendering") on receivers_example.cpp's scene:
// a directional Receive, then HistRender on its histogram with two-tap band filters: four channels of M samples per bin for each receiver.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/render_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_render
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
        const int n_bins = 16, B = 8, M = 4, T = 2, channels = 4, frac_bits = 20;
        std::vector<double> taps((size_t)(B * T));
        for (int b = 0; b < B; ++b) {                  // band b: 1 / (b + 1) now, -0.5 / (b + 1) a sample later
            taps[(size_t)(b * T)] = 1.0 / (b + 1);
            taps[(size_t)(b * T + 1)] = -0.5 / (b + 1);
        }
        std::printf("taps %zu: %.17g %.17g\n", taps.size(), taps[0], taps[(size_t)(B * T - 1)]);
        int refused = 0;
        std::vector<uint64_t> hist(7), det;
        std::vector<double> out;
        try { grid.HistRender(hist, 2, n_bins, B, channels, frac_bits, M, taps, 1, out); } catch (const std::invalid_argument&) { ++refused; }
        hist.assign((size_t)(2 * n_bins * B * channels), 0);
        try { grid.HistRender(hist, 2, n_bins, B, channels, frac_bits, M, std::vector<double>(15), 1, out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.HistRender(hist, 2, n_bins, B, channels, frac_bits, M, taps, 1, out, std::vector<uint32_t>(5)); } catch (const std::invalid_argument&) { ++refused; }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        std::vector<hare_ray> rays;
        for (int k = 0; k < 6; ++k) {
            hare_ray ray{1.0, 0.75, 0.5, 0.0, 0.0, 0.0};
            (&ray.dx)[k / 2] = (k & 1) ? -1.0 : 1.0;
            rays.push_back(ray);
        }
        grid.Receive(rays, 1, 3, n_bins, 0.5, frac_bits, hist, det, nullptr, nullptr, false, true);
        grid.HistRender(hist, 2, n_bins, B, channels, frac_bits, M, taps, 2024, out);
        std::vector<double> again;
        grid.HistRender(hist, 2, n_bins, B, channels, frac_bits, M, taps, 2024, again);
        std::printf("render: out %zu, same twice %d\n", out.size(), (int)(out == again));
        std::printf("out:");
        for (double v : out) std::printf(" %.17g", v);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
