// decode_example.cpp -- the C++ mirror's decoding call (include/hare_hip.h, "receivers", "Decoding"): two receivers of four channels of 50
// samples decoded to two outputs through 2 x 4 filters of 12 taps by Decode; once whole, once cut into two output windows, which must give
// the same doubles.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/decode_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_decode
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
        const int K = 2, C = 4, N = 50, O = 2, T = 12;
        std::vector<double> in((size_t)(K * C * N)), h((size_t)(O * C * T));
        for (int r = 0; r < K * C; ++r)
            for (int t = 0; t < N; ++t) in[(size_t)(r * N + t)] = ((t & 1) ? -1.0 : 1.0) / (1 + r + t);          // decaying, alternating rows
        for (int i = 0; i < O * C * T; ++i) h[(size_t)i] = 0.125 * (i % 7) - 0.3;
        std::printf("in %zu: %.17g %.17g, h %zu: %.17g %.17g\n", in.size(), in[0], in[(size_t)(K * C * N - 1)], h.size(), h[0], h[(size_t)(O * C * T - 1)]);
        int refused = 0;
        std::vector<double> out;
        try { grid.Decode(std::vector<double>(7), K, C, h, O, out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.Decode(in, K, C, std::vector<double>(), O, out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.Decode(in, K, C, std::vector<double>(9), O, out); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.Decode(in, K, C, h, O, out, 52, 10); } catch (const std::invalid_argument&) { ++refused; }          // N + T - 1 = 61
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        grid.Decode(in, K, C, h, O, out);
        const int total = N + T - 1, cut = 23;
        std::vector<double> head, tail;
        grid.Decode(in, K, C, h, O, head, 0, cut);
        grid.Decode(in, K, C, h, O, tail, cut);
        bool same = head.size() == (size_t)(K * O * cut) && tail.size() == (size_t)(K * O * (total - cut));
        for (int r = 0; same && r < K * O; ++r)
            for (int n = 0; n < total; ++n)
                same = same && out[(size_t)(r * total + n)] == (n < cut ? head[(size_t)(r * cut + n)] : tail[(size_t)(r * (total - cut) + n - cut)]);
        std::printf("decode: out %zu, windows same %d\n", out.size(), (int)same);
        std::printf("out:");
        for (double v : out) std::printf(" %.17g", v);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
