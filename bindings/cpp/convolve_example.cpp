// convolve_example.cpp -- the C++ mirror's convolution call (include/hare_hip.h, "receivers", "Convolution"): three rows of 50 samples, each
// convolved with one signal of 20 samples by Convolve; once whole, once cut into two output windows, which must give the same doubles.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/convolve_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_convolve
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
    Topology t0(verts.data(), nverts.data(), 12);
    try {
        Voxel_Grid grid({&t0}, 4);                      // the scene names the device; its geometry is not read
        const int R = 3, N = 50, L = 20;
        std::vector<double> ir((size_t)(R * N)), x((size_t)L);
        for (int r = 0; r < R; ++r)
            for (int t = 0; t < N; ++t) ir[(size_t)(r * N + t)] = ((t & 1) ? -1.0 : 1.0) / (1 + r + t);          // a decaying, alternating row
        for (int i = 0; i < L; ++i) x[(size_t)i] = 0.25 * i - 1.0;
        std::printf("ir %zu: %.17g %.17g, x %zu: %.17g %.17g\n", ir.size(), ir[0], ir[(size_t)(R * N - 1)], x.size(), x[0], x[(size_t)(L - 1)]);
        int refused = 0;
        std::vector<double> out;
        try { grid.Convolve(std::vector<double>(7), R, x, out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.Convolve(ir, R, std::vector<double>(), out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.Convolve(ir, R, x, out, 60, 10); } catch (const std::invalid_argument&) { ++refused; }          // N + L - 1 = 69
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        grid.Convolve(ir, R, x, out);
        std::vector<double> head, tail;
        grid.Convolve(ir, R, x, head, 0, 31);
        grid.Convolve(ir, R, x, tail, 31);
        bool same = head.size() == (size_t)(R * 31) && tail.size() == (size_t)(R * 38);
        for (int r = 0; same && r < R; ++r)
            for (int n = 0; n < N + L - 1; ++n)
                same = same && out[(size_t)(r * (N + L - 1) + n)] == (n < 31 ? head[(size_t)(r * 31 + n)] : tail[(size_t)(r * 38 + n - 31)]);
        std::printf("convolve: out %zu, windows same %d\n", out.size(), (int)same);
        std::printf("out:");
        for (double v : out) std::printf(" %.17g", v);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
