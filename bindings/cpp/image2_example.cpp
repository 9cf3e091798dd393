// image2_example.cpp -- the C++ mirror's second-order image sources (include/hare_hip.h, "receivers", "Image sources (second order)") on
// image_example.cpp's room, the cube [0,2]^3, with an omnidirectional source at its center and one receiver.  With HARE_RECEIVE_DIRECT,
// HARE_RECEIVE_IMAGE and HARE_RECEIVE_IMAGE2 a one-cast call is the three deposits alone -- the direct sound, one reflection per wall and
// the paths off two walls -- the same whatever the seed.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/image2_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_image2
// Without a GPU the flag, the scratch size and the argument checks work; ReceiveSource throws "no HIP device visible".
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
        Voxel_Grid grid({&t0}, 4);
        grid.SetReceivers({1.5, 0.75, 1.25}, {0.25});
        grid.SetAbsorption(0, 2, std::vector<double>(12 * 2, 0.2));
        grid.SetSource({1.0, 1.0, 1.0}, {1.0, 0.5}, {}, 0, {});
        std::printf("flag %u, work bytes %lld, max cands %lld, max paths %lld, prune %lld\n", HARE_RECEIVE_IMAGE2,
                    (long long)Spatial_Partition::Image2WorkBytes(12, 132, 64), (long long)grid.GetOption("image2_max_cands"),
                    (long long)grid.GetOption("image2_max_paths"), (long long)grid.GetOption("image2_prune"));
        int refused = 0;
        alignas(16) char buf[64];
        try { grid.Image2Device(0, 0, 16, 0.25, 30, 132, 64, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }        // n_weight 0
        try { grid.Image2Device(0, 4096, 16, 0.25, 30, 0, 64, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }     // max_cands 0
        try { grid.Image2Device(0, 4096, 16, 0.25, 30, 132, 0, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }    // max_paths 0
        try { grid.Image2Device(0, 4096, 16, 0.25, 30, 132, 64, nullptr, buf, buf + 32); } catch (const std::invalid_argument&) { ++refused; }    // no scratch
        try {                                                                                                                                     // the flag alone
            std::vector<uint64_t> h, d;
            grid.ReceiveSource(16, 0, 0, 3, 16, 0.25, 30, h, d, nullptr, false, false, false, false, true);
        } catch (const std::invalid_argument&) {
            ++refused;
        } catch (const std::exception&) {
        }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        const int64_t n = 4096;
        std::vector<uint64_t> h, det, h2, det2;
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, h, det, nullptr, false, false, true, true, true);        // one cast, all three flags: the deposits alone
        grid.SetOption("source_seed", 42);
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, h2, det2, nullptr, false, false, true, true, true);
        std::printf("image2: detections %llu, seeds %s\n", (unsigned long long)(det[0] + det[1]), h == h2 && det == det2 ? "agree" : "differ");
        std::printf("words:");
        for (size_t w = 0; w < h.size(); ++w) std::printf(" %llu", (unsigned long long)h[w]);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
