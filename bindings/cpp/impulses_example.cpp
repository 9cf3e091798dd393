// impulses_example.cpp -- the C++ mirror's early reflections as impulses (include/hare_hip.h, "receivers", "Impulses"): a shoebox with a
// source and two receivers, SourcePaths at a bin of one sample (bin_len = 343 / 48000), HistImpulses through two three-tap band filters,
// and the peak sample of receiver 0.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/impulses_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_impulses
// Without a GPU the size checks work; the calls throw "no HIP device visible".
#include <cmath>
#include <cstdio>

#include "hare.hpp"

using namespace Hare::Geometry;

int main()
{
    const double L[3] = {5, 4, 3};
    const double c[8][3] = {{0, 0, 0}, {L[0], 0, 0}, {L[0], L[1], 0}, {0, L[1], 0}, {0, 0, L[2]}, {L[0], 0, L[2]}, {L[0], L[1], L[2]}, {0, L[1], L[2]}};
    const int f[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 5, 1}, {0, 4, 5}, {3, 2, 6}, {3, 6, 7}, {0, 3, 7}, {0, 7, 4}, {1, 5, 6}, {1, 6, 2}};
    std::vector<double> verts(12 * 12, 0.0);
    std::vector<int32_t> nverts(12, 3);
    for (int p = 0; p < 12; ++p)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts[p * 12 + 3 * k + a] = c[f[p][k]][a];
    Topology t0(verts.data(), nverts.data(), 12);
    try {
        Voxel_Grid grid({&t0}, 4);
        const int K = 2, B = 2, n_bins = 2048, frac_bits = 40;
        const double bin_len = 343.0 / 48000.0;
        grid.SetReceivers({3.5, 2.5, 1.5, 1.0, 3.0, 2.0}, {0.25, 0.25});
        const double pos[3] = {1.5, 1.0, 1.25}, power[2] = {1.0, 0.5};
        if (hare_scene_set_source(grid.native(), pos, B, power, nullptr, 0, nullptr) != HARE_OK) throw std::runtime_error(hare_last_error());
        std::vector<double> alpha(12 * B, 0.25);
        if (hare_scene_set_absorption(grid.native(), 0, B, alpha.data()) != HARE_OK) throw std::runtime_error(hare_last_error());
        const std::vector<double> taps = {0.25, 0.5, 0.25, -0.25, 0.5, -0.25};          // a lowpass and its complement: together a delay of one sample
        std::vector<uint64_t> hist((size_t)(K * n_bins * B), 0), det;
        std::vector<double> out;
        int refused = 0;
        try { grid.HistImpulses(std::vector<uint64_t>(7), K, n_bins, B, 1, frac_bits, taps, out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.HistImpulses(hist, K, n_bins, B, 1, frac_bits, std::vector<double>(5), out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.HistImpulses(hist, K, n_bins, B, 1, frac_bits, taps, out, 2049, 2); } catch (const std::invalid_argument&) { ++refused; }          // n_bins + T - 1 = 2050
        try { grid.HistImpulses(hist, K, n_bins, B, 1, frac_bits, taps, out, 0, -1, true); } catch (const std::invalid_argument&) { ++refused; }      // nothing to add onto
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        grid.SourcePaths(0, 1 << 20, n_bins, bin_len, frac_bits, hist, det, K, B);
        size_t entries = 0;
        for (uint64_t w : hist) entries += w != 0;
        grid.HistImpulses(hist, K, n_bins, B, 1, frac_bits, taps, out, 1, n_bins);          // n0 = 1, the filters' delay: sample n is bin n
        int peak = 0;
        for (int n = 1; n < n_bins; ++n)
            if (std::fabs(out[(size_t)n]) > std::fabs(out[(size_t)peak])) peak = n;
        std::printf("impulses: entries %zu, out %zu, receiver 0 peak at sample %d (%.4f m) value %.17g\n", entries, out.size(), peak, peak * bin_len, out[(size_t)peak]);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
