// scattering_example.cpp -- the C++ mirror's scattering calls: a room of one topology with absorption and scattering tables of 8 bands,
// a seeded burst through the receive loop, the same burst again (the same histogram) and with another seed (a different one).
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/scattering_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_sc
// Without a GPU the setters, their checks and the read-backs work; Receive throws "no HIP device visible".
#include <cmath>
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
        grid.SetReceivers({1.0, 0.75, 0.5, 0.5, 1.5, 1.5}, {0.25, 0.25});
        std::vector<double> alpha(12 * 8, 0.1), sigma(12 * 8);
        for (int p = 0; p < 12; ++p)
            for (int b = 0; b < 8; ++b) sigma[p * 8 + b] = 0.1 * b;        // more scattering in the higher bands
        grid.SetAbsorption(0, 8, alpha);
        grid.SetScattering(0, 8, sigma);
        grid.SetOption("scatter_seed", -7);
        std::printf("bands %lld, scatter_seed %lld\n", (long long)grid.Bands(0), (long long)grid.GetOption("scatter_seed"));
        int refused = 0;
        try { grid.SetScattering(0, 8, std::vector<double>(12 * 7, 0.5)); } catch (const std::invalid_argument&) { ++refused; }   // short table
        try { grid.SetScattering(1, 8, sigma); } catch (const std::invalid_argument&) { ++refused; }                              // no topology 1
        try { grid.SetScattering(0, 4, std::vector<double>(12 * 4, 0.5)); } catch (const std::invalid_argument&) { ++refused; }   // B != absorption's
        try { grid.SetScattering(0, 8, std::vector<double>(12 * 8, 1.5)); } catch (const std::invalid_argument&) { ++refused; }   // outside [0, 1]
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        // a burst of 4096 rays from receiver 0's center
        std::vector<hare_ray> rays;
        for (int k = 0; k < 4096; ++k) {
            const double z = 1.0 - (2.0 * k + 1.0) / 4096.0, r = std::sqrt(1.0 - z * z), phi = 2.399963229728653 * k;
            rays.push_back(hare_ray{1.0, 0.75, 0.5, r * std::cos(phi), r * std::sin(phi), z});
        }
        std::vector<uint64_t> h1, h2, h3, det;
        grid.Receive(rays, 0, 8, 64, 0.25, 30, h1, det);
        grid.Receive(rays, 0, 8, 64, 0.25, 30, h2, det);
        grid.SetOption("scatter_seed", 8);
        grid.Receive(rays, 0, 8, 64, 0.25, 30, h3, det);
        uint64_t late = 0;
        for (size_t w = 64 * 8; w < h1.size(); ++w) late += h1[w];
        std::printf("receive: hist %zu, same seed %s, other seed %s, receiver 1 nonzero %s\n", h1.size(), h1 == h2 ? "equal" : "differs",
                    h1 == h3 ? "equal" : "differs", late ? "yes" : "no");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
