// receivers_example.cpp -- the C++ mirror's receiver calls on a scene of two topologies, the second with an absorption table of 8 bands.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/receivers_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_rcv
// Without a GPU the setters, the size checks and the bands read-back work; Receive throws "no HIP device visible".
#include <cstdio>

#include "hare.hpp"

using namespace Hare::Geometry;

int main()
{
    // the cube [0,2]^3 as 12 triangles, twice: topology 0 and topology 1
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
        std::vector<double> alpha(12 * 8, 0.25);
        grid.SetAbsorption(1, 8, alpha);
        std::printf("receivers %lld, bands %lld / %lld\n", (long long)grid.GetOption("receivers"), (long long)grid.Bands(0), (long long)grid.Bands(1));
        int refused = 0;
        try { grid.SetReceivers({1.0, 1.0}, {0.25}); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.SetAbsorption(1, 8, std::vector<double>(12 * 7, 0.25)); } catch (const std::invalid_argument&) { ++refused; }
        try { grid.SetAbsorption(2, 1, std::vector<double>(12, 0.25)); } catch (const std::invalid_argument&) { ++refused; }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        // six rays from receiver 0's center along the axes (off every face's diagonal): each passes receiver 0 in every cast, receiver 1 never
        std::vector<hare_ray> rays;
        for (int k = 0; k < 6; ++k) {
            hare_ray r{1.0, 0.75, 0.5, 0.0, 0.0, 0.0};
            (&r.dx)[k / 2] = (k & 1) ? -1.0 : 1.0;
            rays.push_back(r);
        }
        std::vector<uint64_t> hist, det;
        std::vector<double> state;
        grid.Receive(rays, 1, 3, 16, 0.5, 20, hist, det, nullptr, &state);
        uint64_t bins = 0;
        for (uint64_t v : hist) bins += v != 0;
        std::printf("receive: hist %zu, state %zu, detections %llu %llu, band 7 of receiver 0 bin 0: %llu, nonzero %llu\n", hist.size(), state.size(),
                    (unsigned long long)det[0], (unsigned long long)det[2], (unsigned long long)hist[7], (unsigned long long)bins);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
