// image_example.cpp -- the C++ mirror's first-order image sources (include/hare_hip.h, "receivers", "Image sources (first order)") on
// direct_example.cpp's room, the cube [0,2]^3, with an omnidirectional source at its center and one receiver.  With HARE_RECEIVE_IMAGE a
// one-cast call is cast 0's sampled direct sound plus the deposit: one add per wall the source sees the receiver in (six in a cube), the
// same whatever the seed.  With HARE_RECEIVE_DIRECT as well nothing of the result is sampled.
// Build:  g++ -std=c++17 -I include -I bindings/cpp bindings/cpp/image_example.cpp -L hare_amd -lhare_hip -Wl,-rpath,$PWD/hare_amd -o /tmp/hare_image
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
        std::printf("flag %u, work bytes %lld, max pairs %lld\n", HARE_RECEIVE_IMAGE, (long long)Spatial_Partition::ImageWorkBytes(1, 12, 64),
                    (long long)grid.GetOption("image_max_pairs"));
        int refused = 0;
        alignas(16) char buf[64];
        try { grid.ImageDevice(0, 0, 16, 0.25, 30, 64, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }        // n_weight 0
        try { grid.ImageDevice(0, 4096, 16, 0.25, 30, 0, buf, buf + 16, buf + 32); } catch (const std::invalid_argument&) { ++refused; }     // max_pairs 0
        try { grid.ImageDevice(0, 4096, 16, 0.25, 30, 64, nullptr, buf, buf + 32); } catch (const std::invalid_argument&) { ++refused; }     // no scratch
        try {                                                                                                                                // the caller's rays
            std::vector<hare_ray> rays(1, hare_ray{1.0, 1.0, 1.0, 1.0, 0.0, 0.0});
            std::vector<uint64_t> hist(16 * 2), det(2);
            hare_counters ctr{};
            if (hare_receive_batch(grid.native(), HARE_KIND_VOXEL, 0, 1, rays.data(), nullptr, nullptr, 1, HARE_RECEIVE_IMAGE, 16, 0.25, 30, nullptr,
                                   nullptr, hist.data(), det.data(), &ctr) == HARE_E_INVALID)
                ++refused;
        } catch (const std::exception&) {
        }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        const int64_t n = 4096;
        std::vector<uint64_t> h, det, h2, det2;
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, h, det, nullptr, false, false, true, true);        // one cast, both flags: the two deposits alone
        grid.SetOption("source_seed", 42);
        grid.ReceiveSource(n, 0, 0, 1, 16, 0.25, 30, h2, det2, nullptr, false, false, true, true);
        std::printf("image: detections %llu, seeds %s\n", (unsigned long long)det[0], h == h2 && det == det2 ? "agree" : "differ");
        std::printf("words:");
        for (size_t w = 0; w < h.size(); ++w) std::printf(" %llu", (unsigned long long)h[w]);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
