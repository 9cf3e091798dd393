// fan_out_tsan.cpp -- the host threading of the batch calls under ThreadSanitizer (hare_amd/csrc/Makefile: tsan-test).  Linked with the
// library's host sources; the library binds tests/stubs/fake_hip.cpp through HARE_HIP_RUNTIME, so nothing here needs a GPU.
//   fan_out alone    1, 2 and 64 parts: a part that fails with a message, a part that throws std::bad_alloc, one that throws an int, and two
//                    failing parts, of which the lower index is reported
//   part_range       the parts tile [0, n) for n in {0, 1, 63, 2^40 + 1} and 1, 3, 64 parts; INT64_MAX / 2 in 64 parts does not overflow
//   the lease        twelve threads x 50 hare_shoot_batch calls of 37 rays on one scene (four staging contexts), beside one thread running
//                    hare_bounce_batch_sharded over three further scenes; every call returns HARE_OK
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "hare_hip.h"
#include "fan_out.h"

static int g_failures = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) { ++g_failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

static void test_fan_out()
{
    using hare::fan_out;
    using hare::FanResult;
    const char* thrown = "test: exception in a part";
    for (int parts : {1, 2, 64}) {
        const int last = parts - 1;
        std::atomic<int> ran{0};
        FanResult f = fan_out(parts, thrown, [&](int) { ++ran; return (int)HARE_OK; });
        EXPECT(f.rc == HARE_OK && ran == parts && f.text.empty());
        f = fan_out(parts, thrown, [&](int k) {
            if (k != last) return (int)HARE_OK;
            hare::set_error("part " + std::to_string(k) + " failed");
            return (int)HARE_E_HIP;
        });
        EXPECT(f.rc == HARE_E_HIP && f.part == last && f.text == "part " + std::to_string(last) + " failed");
        f = fan_out(parts, thrown, [&](int k) -> int {
            if (k == last) throw std::bad_alloc();
            return HARE_OK;
        });
        EXPECT(f.rc == HARE_E_NOMEM && f.part == last && f.text == thrown);
        f = fan_out(parts, thrown, [&](int k) -> int {
            if (k == last) throw 7;
            return HARE_OK;
        });
        EXPECT(f.rc == HARE_E_NOMEM && f.part == last && f.text == thrown);
        EXPECT(f.shard_text() == "shard " + std::to_string(last) + ": " + thrown);
        if (parts > 1) {      // two failing parts: the lower index wins
            const int lower = parts / 2;
            f = fan_out(parts, thrown, [&](int k) -> int {
                if (k == lower) { hare::set_error("the lower one"); return HARE_E_STATE; }
                if (k == last) { hare::set_error("the upper one"); return HARE_E_HIP; }
                return HARE_OK;
            });
            EXPECT(f.rc == HARE_E_STATE && f.part == lower && f.text == "the lower one");
        }
    }
    EXPECT(fan_out(0, thrown, [](int) { return (int)HARE_OK; }).rc == HARE_E_INVALID);
    EXPECT(fan_out(65, thrown, [](int) { return (int)HARE_OK; }).rc == HARE_E_INVALID);
}

static void test_part_range()
{
    using hare::part_range;
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, ((int64_t)1 << 40) + 1})
        for (int parts : {1, 3, 64}) {
            int64_t at = 0;
            for (int k = 0; k < parts; ++k) {
                const hare::PartRange r = part_range(n, k, parts);
                EXPECT(r.lo == at && r.hi >= r.lo && r.size() <= n / parts + 1);
                at = r.hi;
            }
            EXPECT(at == n);
        }
    const int64_t big = INT64_MAX / 2;
    int64_t at = 0;
    for (int k = 0; k < 64; ++k) {
        const hare::PartRange r = part_range(big, k, 64);
        EXPECT(r.lo == at && r.size() >= big / 64 && r.size() <= big / 64 + 1);
        at = r.hi;
    }
    EXPECT(at == big);
}

// a 2 x 2 x 2 box of twelve triangles
struct Box {
    std::vector<double> verts, normals;
    std::vector<int32_t> nverts;
    double mn[3], mx[3];
    Box() : verts(12 * 12, 0.0), normals(12 * 3), nverts(12, 3)
    {
        const double c[8][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}};
        const int q[6][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 5, 4}, {3, 2, 6, 7}, {0, 3, 7, 4}, {1, 2, 6, 5}};
        for (int f = 0; f < 6; ++f)
            for (int t = 0; t < 2; ++t) {
                const int tri[3] = {q[f][0], q[f][1 + t], q[f][2 + t]};
                for (int v = 0; v < 3; ++v) memcpy(&verts[((size_t)(2 * f + t) * 4 + v) * 3], c[tri[v]], 3 * sizeof(double));
            }
        EXPECT(hare_polygon_normals(verts.data(), nverts.data(), 12, normals.data()) == HARE_OK);
        EXPECT(hare_topology_bounds(verts.data(), nverts.data(), 12, mn, mx) == HARE_OK);
    }
    hare_scene* voxel_scene() const
    {
        hare_topology_desc d{};
        d.P = 12;
        d.verts = verts.data();
        d.nverts = nverts.data();
        d.normals = normals.data();
        for (int a = 0; a < 3; ++a) { d.min[a] = mn[a]; d.max[a] = mx[a]; }
        hare_scene* s = nullptr;
        EXPECT(hare_scene_create(&d, 1, 0, &s) == HARE_OK && s);
        EXPECT(hare_voxel_build(s, 4) == HARE_OK);
        return s;
    }
};

static std::vector<hare_ray> some_rays(int n)
{
    std::vector<hare_ray> r((size_t)n);
    memset(r.data(), 0, r.size() * sizeof(hare_ray));
    for (int i = 0; i < n; ++i) {
        r[(size_t)i].x = r[(size_t)i].y = r[(size_t)i].z = 1.0;
        (i % 3 == 0 ? r[(size_t)i].dx : (i % 3 == 1 ? r[(size_t)i].dy : r[(size_t)i].dz)) = (i & 1) ? 1.0 : -1.0;
    }
    return r;
}

static void test_lease()
{
    const Box box;
    hare_scene* one = box.voxel_scene();
    hare_scene* three[3] = {box.voxel_scene(), box.voxel_scene(), box.voxel_scene()};
    constexpr int kThreads = 12, kCalls = 50, kRays = 37;
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
        th.emplace_back([&] {
            std::vector<hare_ray> rays = some_rays(kRays);
            std::vector<hare_xevent> out((size_t)kRays);
            hare_counters ctr;
            for (int c = 0; c < kCalls; ++c)
                if (hare_shoot_batch(one, HARE_KIND_VOXEL, 0, kRays, rays.data(), nullptr, nullptr, 0, out.data(), &ctr) != HARE_OK) ++bad;
        });
    th.emplace_back([&] {
        std::vector<hare_ray> rays = some_rays(kRays);
        std::vector<hare_xevent> last((size_t)kRays);
        hare_counters ctr;
        for (int c = 0; c < kCalls; ++c)
            if (hare_bounce_batch_sharded(three, 3, HARE_KIND_VOXEL, 0, kRays, rays.data(), nullptr, nullptr, 2, 0, nullptr, last.data(), &ctr, nullptr) != HARE_OK)
                ++bad;
    });
    for (std::thread& t : th) t.join();
    EXPECT(bad == 0);
    if (bad != 0) printf("last error: %s\n", hare_last_error());
    hare_scene_destroy(one);
    for (hare_scene* s : three) hare_scene_destroy(s);
}

int main()
{
    int32_t devices = 0;
    EXPECT(hare_device_count(&devices) == HARE_OK && devices == 1);
    test_fan_out();
    test_part_range();
    test_lease();
    printf("fan_out_tsan: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
