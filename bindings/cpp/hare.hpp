// hare.hpp -- C++ host-side mirror of the reference interface for the ray-cast path, over the C-ABI
// (include/hare_hip.h).  The reference is a compiled C# library whose toolchain is absent from the
// build image, so the compiled-language host side is written in C++ with the reference's names,
// argument meaning and error behaviour:
//   Hare::Geometry::Ray / X_Event          Hare_Geometry_Primitives.cs:393-481
//   Hare::Geometry::Topology               the members a partition reads (Hare_Geometry_Topology.cs:418-424,482,539,50/58)
//   Hare::Geometry::Spatial_Partition      Spatial_Partition.cs:27-35
//   Voxel_Grid / Octree / KDTree           Voxel_Grid.cs:48,128  "Octree - alt.cs":45  KDTree.cs:51
// Header-only; link with -lhare_hip.  Errors become exceptions, like in .NET.
#pragma once
#include <array>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "hare_hip.h"

namespace Hare {
namespace Geometry {

struct Ray {                       // Hare_Geometry_Primitives.cs:393-429
    double x, y, z, dx, dy, dz;
    int ThreadID = 0, Ray_ID = 0;
    Ray(double x_, double y_, double z_, double dx_, double dy_, double dz_, int ThreadID_IN = 0, int ID = 0)
        : x(x_), y(y_), z(z_), dx(dx_), dy(dy_), dz(dz_), ThreadID(ThreadID_IN), Ray_ID(ID) {}
    void Reverse() { dx *= -1; dy *= -1; dz *= -1; }
};

struct X_Event {                   // Hare_Geometry_Primitives.cs:435-481
    double u = 0, v = 0, t = 0;
    bool Hit = false;
    bool has_point = false;        // X_Point == null on a miss
    std::array<double, 3> X_Point{{0, 0, 0}};
    int Poly_id = -1;
    X_Event() = default;           // :454-462
    explicit X_Event(const hare_xevent& e)
    {
        if (e.hit) { u = e.u; v = e.v; t = e.t; Hit = true; has_point = true; X_Point = {{e.x, e.y, e.z}}; Poly_id = e.poly_id; }
    }
};

inline void check(int rc)
{
    if (rc == HARE_OK) return;
    const std::string msg = std::string("hare_hip error ") + std::to_string(rc) + ": " + hare_last_error();
    if (rc == HARE_E_INVALID) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}

// ambisonic order of a directional histogram (include/hare_hip.h, "Higher orders"): the channels per word and the calls' flag bits
inline int Channels(int order)
{
    if (order < 1 || order > 3) throw std::invalid_argument("order must be 1, 2 or 3");
    return order == 1 ? 4 : (order == 2 ? 9 : 16);
}
inline uint32_t ChannelFlags(bool directional, int order = 1)
{
    (void)Channels(order);
    return (directional ? HARE_RECEIVE_DIRECTIONAL : 0u) | (order == 2 ? HARE_RECEIVE_ORDER2 : (order == 3 ? HARE_RECEIVE_ORDER3 : 0u));
}

class Topology {
public:
    std::vector<double> verts;     // P x 4 x 3
    std::vector<int32_t> nverts;   // P
    std::vector<double> normals;   // P x 3
    double Min[3], Max[3];

    // polygons: P x 4 x 3 doubles (corner 3 ignored for triangles) + corner counts; normals and the
    // Min/Max box are computed by the library's restatements of the Polygon ctor / Finish_Topology
    Topology(const double* v, const int32_t* nv, int32_t P) : verts(v, v + (size_t)P * 12), nverts(nv, nv + P), normals((size_t)P * 3)
    {
        check(hare_polygon_normals(verts.data(), nverts.data(), P, normals.data()));
        check(hare_topology_bounds(verts.data(), nverts.data(), P, Min, Max));
    }
    // Topology(Point[][]) + Finish_Topology(): raw polygon soup through the reference's ingest (Round(15) and the
    // 1 mm Hash2 corner merge) first.  Vertices_List and the per-corner vertex index are returned on request.
    static Topology from_polygons(const double* soup, const int32_t* nv, int32_t P, std::vector<double>* vertices = nullptr,
                                  std::vector<int32_t>* corner_vertex = nullptr)
    {
        std::vector<double> merged((size_t)P * 12), vlist;
        std::vector<int32_t> cv((size_t)P * 4);
        size_t corners = 0;
        for (int32_t p = 0; p < P; ++p) corners += (size_t)(nv[p] > 0 ? nv[p] : 0);
        vlist.resize(corners * 3 + 3);
        int32_t n_vertices = 0;
        check(hare_topology_ingest(soup, nv, P, merged.data(), cv.data(), vlist.data(), &n_vertices));
        vlist.resize((size_t)n_vertices * 3);
        if (vertices) *vertices = std::move(vlist);
        if (corner_vertex) *corner_vertex = std::move(cv);
        return Topology(merged.data(), nv, P);
    }
    int Polygon_Count() const { return (int)nverts.size(); }
    std::array<double, 3> Normal(int Poly_ID) const { return {{normals[3 * Poly_ID], normals[3 * Poly_ID + 1], normals[3 * Poly_ID + 2]}}; }
    std::array<double, 3> operator()(int Poly_ID, int Corner_ID) const
    {
        const double* p = &verts[(size_t)Poly_ID * 12 + 3 * Corner_ID];
        return {{p[0], p[1], p[2]}};
    }
    hare_topology_desc desc() const
    {
        hare_topology_desc d{};
        d.P = Polygon_Count();
        d.verts = verts.data();
        d.nverts = nverts.data();
        d.normals = normals.data();
        for (int a = 0; a < 3; ++a) { d.min[a] = Min[a]; d.max[a] = Max[a]; }
        return d;
    }
};

class Spatial_Partition {          // Spatial_Partition.cs:27-35
public:
    std::vector<const Topology*> Model;
    double Char_Step = 0;

    virtual ~Spatial_Partition() { hare_scene_destroy(scene_); }
    Spatial_Partition(const Spatial_Partition&) = delete;
    Spatial_Partition& operator=(const Spatial_Partition&) = delete;

    // bool Shoot(Ray R, int top_index, out X_Event Ret_event[, int poly_origin1, int poly_origin2 = -1])
    bool Shoot(Ray& R, int top_index, X_Event& Ret_event, int poly_origin1 = -1, int poly_origin2 = -1)
    {
        // one ray = the reference call site: traced on the calling host thread (hare_shoot_one; lock-free, no GPU round trip)
        hare_ray r{R.x, R.y, R.z, R.dx, R.dy, R.dz};
        hare_xevent e;
        check(hare_shoot_one(scene_, kind_, top_index, &r, poly_origin1, poly_origin2, &e));
        R.x = r.x; R.y = r.y; R.z = r.z;     // the reference moves R when it starts outside the grid
        Ret_event = X_Event(e);
        return Ret_event.Hit;
    }

    // the batch entry: n rays at once through the HIP kernels; returns the number of hits
    uint64_t Shoot(std::vector<hare_ray>& rays, int top_index, std::vector<hare_xevent>& results,
                   const int32_t* poly_origin1 = nullptr, const int32_t* poly_origin2 = nullptr, bool move_origins = false)
    {
        results.resize(rays.size());
        hare_counters c{};
        check(hare_shoot_batch(scene_, kind_, top_index, (int64_t)rays.size(), rays.data(), poly_origin1, poly_origin2,
                               move_origins ? HARE_SHOOT_WRITEBACK_ORIGIN : 0u, results.data(), &c));
        return c.hits;
    }
    // occlusion predicate (harness-defined): occluded[i] = closest hit of rays[i] exists and t < t_max[i] (null: any hit)
    std::vector<int32_t> Occluded(std::vector<hare_ray>& rays, int top_index, const double* t_max = nullptr,
                                  const int32_t* poly_origin1 = nullptr, const int32_t* poly_origin2 = nullptr)
    {
        std::vector<int32_t> occ(rays.size());
        check(hare_occluded_batch(scene_, kind_, top_index, (int64_t)rays.size(), rays.data(), poly_origin1, poly_origin2, t_max, 0u,
                                  occ.data(), nullptr, nullptr));
        return occ;
    }
    // the bounce loop in one call (harness-defined; the reference leaves reflection to its caller, who re-shoots with
    // poly_origin1 = the polygon just hit, Spatial_Partition.cs:33): `bounces` casts, rays resident on the GPU throughout.
    // events_all: bounces x rays.size() records, cast-major.  Returns the hits over all casts.
    uint64_t Bounce(const std::vector<hare_ray>& rays, int top_index, int bounces, std::vector<hare_xevent>& events_all,
                    const int32_t* poly_origin1 = nullptr, const int32_t* poly_origin2 = nullptr, std::vector<hare_counters>* per_cast = nullptr)
    {
        events_all.resize(rays.size() * (size_t)(bounces > 0 ? bounces : 0));
        if (per_cast) per_cast->resize((size_t)(bounces > 0 ? bounces : 0));
        hare_counters c{};
        check(hare_bounce_batch(scene_, kind_, top_index, (int64_t)rays.size(), rays.data(), poly_origin1, poly_origin2, bounces, 0u,
                                events_all.data(), nullptr, &c, per_cast ? per_cast->data() : nullptr));
        return c.hits;
    }
    // receivers (include/hare_hip.h, "receivers"): K spheres, an absorption table per topology, and the bounce loop with the receiver
    // step between its casts.  hist: K x n_bins x B fixed-point sums (scale 2^-frac_bits), B = Bands(top_index); detections: 2 K;
    // state: (1 + B) x rays.size() (L, then E per band); rain: diffuse rain (HARE_RECEIVE_DIFFUSE_RAIN).  Returns the hits over all casts.  Sizes are checked here: the library reads and
    // writes as many values as the scene says, whatever the vectors hold.  directional (HARE_RECEIVE_DIRECTIONAL): hist is K x n_bins x B x 4,
    // channel innermost: W (the omni word), then X, Y, Z as int64 in two's complement (positive for sound arriving from +x, +y, +z).
    // order 2 or 3 beside it (HARE_RECEIVE_ORDER2 / HARE_RECEIVE_ORDER3; the header's "Higher orders"): hist is K x n_bins x B x 9 or x 16,
    // the four channels first, then ACN 4 .. 8 or 4 .. 15 in SN3D, int64 like X, Y, Z.  A third-order room response of a burst:
    //     std::vector<uint64_t> hist, det;
    //     grid.ReceiveOrder(rays, 0, 8, 512, 0.25, 40, hist, det, nullptr, nullptr, false, /*directional=*/true, /*order=*/3);
    //     int64_t y6 = (int64_t)hist[((k * 512 + bin) * B + b) * Hare::Geometry::Channels(3) + 6];      // ACN 6 of receiver k, bin, band b
    // ChannelFlags(directional, order) gives the bits for the calls on native() that take `flags` (hare_receive_source, hare_direct_device ...).
    // Termination (the header's section of that name).  HARE_RECEIVE_TIME_LIMIT (512u, a flag of hare_receive_batch on native(); Receive
    // below does not set it): a ray whose path L has reached n_bins * bin_len after a hit is retired; hist and detections[2k] are
    // those of the call without it, detections[2k + 1] and the final state differ.  The energy
    // floor is the scene's: SetOption("receive_floor_bits", f) retires a ray whose largest band lies under 2^-f (0: off; biased by
    // design), SetOption("receive_roulette", 1) lets it survive with probability ps = m / F, divided by ps (expectation kept).
    void SetReceivers(const std::vector<double>& centers, const std::vector<double>& radii)
    {
        if (centers.size() != 3 * radii.size()) throw std::invalid_argument("SetReceivers: centers must hold 3 x radii.size() values");
        check(hare_scene_set_receivers(scene_, (int32_t)radii.size(), centers.data(), radii.data()));
    }
    // A receiver map (hare_scene_set_receiver_map): up to 65 536 receivers found through a uniform grid over their centers; cell 0: twice
    // the largest radius.  Diffuse rain does not combine with a map; SetReceivers afterwards returns the scene to the linear loop.
    void SetReceiverMap(const std::vector<double>& centers, const std::vector<double>& radii, double cell = 0.0)
    {
        if (centers.size() != 3 * radii.size()) throw std::invalid_argument("SetReceiverMap: centers must hold 3 x radii.size() values");
        check(hare_scene_set_receiver_map(scene_, (int32_t)radii.size(), centers.data(), radii.data(), cell));
    }
    void SetAbsorption(int top_index, int bands, const std::vector<double>& alpha)
    {
        if (top_index < 0 || (size_t)top_index >= Model.size()) throw std::invalid_argument("SetAbsorption: bad top_index");
        if (bands < 1 || alpha.size() != (size_t)Model[(size_t)top_index]->Polygon_Count() * (size_t)bands)
            throw std::invalid_argument("SetAbsorption: alpha must hold Polygon_Count x bands values");
        check(hare_scene_set_absorption(scene_, top_index, bands, alpha.data()));
    }
    // scattering table of Model[top_index] (hare_scene_set_scattering): Polygon_Count x bands values in [0, 1], the same bands as its absorption
    // table if it has one; the receive loop then scatters diffusely (seed: SetOption("scatter_seed", ...)).  ClearScattering removes it.
    void SetScattering(int top_index, int bands, const std::vector<double>& sigma)
    {
        if (top_index < 0 || (size_t)top_index >= Model.size()) throw std::invalid_argument("SetScattering: bad top_index");
        if (bands < 1 || sigma.size() != (size_t)Model[(size_t)top_index]->Polygon_Count() * (size_t)bands)
            throw std::invalid_argument("SetScattering: sigma must hold Polygon_Count x bands values");
        check(hare_scene_set_scattering(scene_, top_index, bands, sigma.data()));
    }
    void ClearScattering(int top_index) { check(hare_scene_set_scattering(scene_, top_index, 0, nullptr)); }
    int64_t Bands(int top_index) const { return GetOption(("bands:" + std::to_string(top_index)).c_str()); }
    uint64_t Receive(const std::vector<hare_ray>& rays, int top_index, int bounces, int n_bins, double bin_len, int frac_bits,
                     std::vector<uint64_t>& hist, std::vector<uint64_t>& detections, const std::vector<double>* state_in = nullptr,
                     std::vector<double>* state_out = nullptr, bool rain = false, bool directional = false)
    {
        return ReceiveOrder(rays, top_index, bounces, n_bins, bin_len, frac_bits, hist, detections, state_in, state_out, rain, directional, 1);
    }
    // Receive at ambisonic order 1, 2 or 3 (2, 3: only with directional)
    uint64_t ReceiveOrder(const std::vector<hare_ray>& rays, int top_index, int bounces, int n_bins, double bin_len, int frac_bits,
                          std::vector<uint64_t>& hist, std::vector<uint64_t>& detections, const std::vector<double>* state_in,
                          std::vector<double>* state_out, bool rain, bool directional, int order)
    {
        const int64_t K = GetOption("receivers"), B = Bands(top_index);
        const size_t n_state = (size_t)(1 + B) * rays.size();
        if (state_in && state_in->size() != n_state) throw std::invalid_argument("Receive: state_in must hold (1 + B) x rays.size() values");
        hist.assign((size_t)(K * (n_bins > 0 ? n_bins : 0) * B * (directional ? Channels(order) : 1)), 0);
        detections.assign((size_t)(2 * K), 0);
        if (state_out) state_out->assign(n_state, 0.0);
        hare_counters c{};
        check(hare_receive_batch(scene_, kind_, top_index, (int64_t)rays.size(), rays.data(), nullptr, nullptr, bounces,
                                 (rain ? HARE_RECEIVE_DIFFUSE_RAIN : 0u) | ChannelFlags(directional, order), n_bins, bin_len,
                                 frac_bits, state_in ? state_in->data() : nullptr, state_out ? state_out->data() : nullptr, hist.data(),
                                 detections.data(), &c));
        return c.hits;
    }
    // the point source (include/hare_hip.h, "receivers", "Source"; hare_scene_set_source): a position, a power per band (power.size() = B),
    // and optionally a directivity table gain[6][R][R][B] (band innermost) read in the frame (9 values, row-major; empty: identity).  Seed:
    // SetOption("source_seed", ...).  ReceiveSource is Receive with the rays first_ray .. first_ray + n - 1 and their state emitted on the
    // device: nothing but the count goes up, and calls over [0, k) and [k, n) sum to the histogram of the one call.
    void SetSource(const std::array<double, 3>& pos, const std::vector<double>& power, const std::vector<double>& frame = {}, int R = 0,
                   const std::vector<double>& gain = {})
    {
        if (!frame.empty() && frame.size() != 9) throw std::invalid_argument("SetSource: frame must hold 9 values (or none)");
        if (R < 0 || gain.size() != (size_t)6 * (size_t)R * (size_t)R * power.size())
            throw std::invalid_argument("SetSource: gain must hold 6 x R x R x power.size() values");
        check(hare_scene_set_source(scene_, pos.data(), (int32_t)power.size(), power.data(), frame.empty() ? nullptr : frame.data(), R,
                                    R > 0 ? gain.data() : nullptr));
    }
    // direct (HARE_RECEIVE_DIRECT; the header's "Direct sound"): the direct sound is one visibility-tested deposit per receiver, standing
    // for the call's n rays, and cast 0 detects nothing.  image (HARE_RECEIVE_IMAGE; "Image sources (first order)"): the first-order specular
    // reflections are one visibility-tested deposit per (receiver, polygon) pair, and in cast 1 the rays that left cast 0 specularly detect
    // nothing; the pair list holds GetOption("image_max_pairs") pairs (std::runtime_error, HARE_E_NOMEM with the needed count, when the scene yields more).
    // image2 (HARE_RECEIVE_IMAGE2, only with image; "Image sources (second order)"): the specular paths off two polygons are one deposit each
    // and in cast 2 the rays reflected specularly twice detect nothing; the lists hold GetOption("image2_max_cands") candidates and
    // GetOption("image2_max_paths") paths (std::runtime_error, HARE_E_NOMEM with both counts, when the scene yields more).
    uint64_t ReceiveSource(int64_t n, int64_t first_ray, int top_index, int bounces, int n_bins, double bin_len, int frac_bits,
                           std::vector<uint64_t>& hist, std::vector<uint64_t>& detections, std::vector<double>* state_out = nullptr,
                           bool rain = false, bool directional = false, bool direct = false, bool image = false, bool image2 = false)
    {
        if (n < 0) throw std::invalid_argument("ReceiveSource: n must be >= 0");
        const int64_t K = GetOption("receivers"), B = Bands(top_index);
        hist.assign((size_t)(K * (n_bins > 0 ? n_bins : 0) * B * (directional ? 4 : 1)), 0);
        detections.assign((size_t)(2 * K), 0);
        if (state_out) state_out->assign((size_t)(1 + B) * (size_t)n, 0.0);
        hare_counters c{};
        check(hare_receive_source(scene_, kind_, top_index, n, first_ray, bounces,
                                  (rain ? HARE_RECEIVE_DIFFUSE_RAIN : 0u) | (directional ? HARE_RECEIVE_DIRECTIONAL : 0u) |
                                      (direct ? HARE_RECEIVE_DIRECT : 0u) | (image ? HARE_RECEIVE_IMAGE : 0u) | (image2 ? HARE_RECEIVE_IMAGE2 : 0u),
                                  n_bins, bin_len, frac_bits, state_out ? state_out->data() : nullptr, hist.data(), detections.data(), &c));
        return c.hits;
    }
    // hare_direct_device on device pointers and a hipStream_t: the direct sound's deposit alone, for n_weight source rays, ACCUMULATED into
    // d_hist (K x n_bins x B, x 4 with directional) and d_detections (2 K); d_work holds DirectWorkBytes(K) bytes.  Stream-ordered.  For a
    // caller who runs the burst in chunks through hare_receive_device (on native()) with HARE_RECEIVE_DIRECT: one deposit for the whole count.
    static int64_t DirectWorkBytes(int64_t K) { return HARE_DIRECT_WORK_BYTES(K); }
    void DirectDevice(int top_index, int64_t n_weight, int n_bins, double bin_len, int frac_bits, void* d_work, void* d_hist, void* d_detections,
                      bool directional = false, void* stream = nullptr)
    {
        check(hare_direct_device(scene_, kind_, top_index, n_weight, directional ? HARE_RECEIVE_DIRECTIONAL : 0u, n_bins, bin_len, frac_bits,
                                 d_work, d_hist, d_detections, stream));
    }
    // hare_image_device on device pointers and a hipStream_t: the first-order image sources' deposit alone, for n_weight source rays,
    // ACCUMULATED into d_hist and d_detections (shaped as DirectDevice's); d_work holds ImageWorkBytes(K, P, max_pairs) bytes on a 16-byte
    // boundary, and its first uint64 receives the number of pairs found (more than max_pairs: nothing was deposited).  Stream-ordered.
    static int64_t ImageWorkBytes(int64_t K, int64_t P, int64_t max_pairs) { return HARE_IMAGE_WORK_BYTES(K, P, max_pairs); }
    void ImageDevice(int top_index, int64_t n_weight, int n_bins, double bin_len, int frac_bits, int64_t max_pairs, void* d_work, void* d_hist,
                     void* d_detections, bool directional = false, void* stream = nullptr)
    {
        check(hare_image_device(scene_, kind_, top_index, n_weight, directional ? HARE_RECEIVE_DIRECTIONAL : 0u, n_bins, bin_len, frac_bits,
                                max_pairs, d_work, d_hist, d_detections, stream));
    }
    // hare_image2_device on device pointers and a hipStream_t: the second-order image sources' deposit alone, ACCUMULATED into d_hist and
    // d_detections; d_work holds Image2WorkBytes(P, max_cands, max_paths) bytes on a 16-byte boundary, and its first two uint64 receive the
    // candidates and the paths found (either beyond its list: nothing was deposited).  Stream-ordered.
    static int64_t Image2WorkBytes(int64_t P, int64_t max_cands, int64_t max_paths) { return HARE_IMAGE2_WORK_BYTES(P, max_cands, max_paths); }
    void Image2Device(int top_index, int64_t n_weight, int n_bins, double bin_len, int frac_bits, int64_t max_cands, int64_t max_paths, void* d_work,
                      void* d_hist, void* d_detections, bool directional = false, void* stream = nullptr)
    {
        check(hare_image2_device(scene_, kind_, top_index, n_weight, directional ? HARE_RECEIVE_DIRECTIONAL : 0u, n_bins, bin_len, frac_bits,
                                 max_cands, max_paths, d_work, d_hist, d_detections, stream));
    }
    // the reduction of a histogram on the device (include/hare_hip.h, "receivers", "Reduction"): per receiver and band, the sums S0 = sum g
    // and S1 = sum i g over bin windows and the bins at which the backward-integrated decay crosses the levels.  What to compute:
    struct Reduction {
        std::vector<int32_t> windows;       // lo_0, hi_0, lo_1, hi_1, ...: up to 16 bin ranges [lo, hi)
        std::vector<uint32_t> levels;       // up to 32 fractions in units of 2^-32 (DecayLevel)
        std::vector<uint32_t> weight;       // n_bins x B in units of 2^-32 (AirWeights), or empty: none
    };
    static uint32_t DecayLevel(double dB)   // min(2^32 - 1, floor(10^(dB / 10) * 2^32)), dB <= 0
    {
        const double f = std::floor(std::pow(10.0, dB / 10.0) * 4294967296.0);
        return f >= 4294967295.0 ? 4294967295u : (f > 0 ? (uint32_t)f : 0u);
    }
    // weights for air absorption: m holds the energy attenuation per unit of path length of each band;
    // min(2^32 - 1, floor(exp(-m_b * (i + 0.5) * bin_len) * 2^32)), bin-major
    static std::vector<uint32_t> AirWeights(const std::vector<double>& m, double bin_len, int n_bins)
    {
        std::vector<uint32_t> w((size_t)(n_bins > 0 ? n_bins : 0) * m.size());
        for (int i = 0; i < n_bins; ++i)
            for (size_t b = 0; b < m.size(); ++b) {
                const double f = std::floor(std::exp(-m[b] * ((double)i + 0.5) * bin_len) * 4294967296.0);
                w[(size_t)i * m.size() + b] = f >= 4294967295.0 ? 4294967295u : (f > 0 ? (uint32_t)f : 0u);
            }
        return w;
    }
    // hare_hist_reduce: hist is K x n_bins x B (x 4 with channels = 4; channel 0 is read) as Receive returns it.  sums: K x B x n_win x 4
    // (S0 lo, S0 hi, S1 lo, S1 hi); cross: K x B x n_lev
    void HistReduce(const std::vector<uint64_t>& hist, int K, int n_bins, int B, int channels, const Reduction& r, std::vector<uint64_t>& sums,
                    std::vector<int32_t>& cross)
    {
        if (K < 0 || n_bins < 0 || B < 0 || channels < 0 || hist.size() != (size_t)K * (size_t)n_bins * (size_t)B * (size_t)channels)
            throw std::invalid_argument("HistReduce: hist must hold K x n_bins x B x channels values");
        const int n_win = check_reduction(r, n_bins, B, "HistReduce"), n_lev = (int)r.levels.size();
        sums.assign((size_t)K * (size_t)B * (size_t)n_win * 4, 0);
        cross.assign((size_t)K * (size_t)B * (size_t)n_lev, 0);
        check(hare_hist_reduce(scene_, K, n_bins, B, channels, hist.data(), r.weight.empty() ? nullptr : r.weight.data(), n_win, r.windows.data(),
                               n_lev, r.levels.data(), sums.data(), cross.data()));
    }
    // hare_hist_project (include/hare_hip.h, "receivers", "Projection"): hist as Receive returns it (K x n_bins x B x channels; channel 0 is
    // read) projected onto the vectors coef (J x n_bins, vector-major, 1 <= J <= 32).  proj: K x B x J x 2, the lo and hi words of the exact
    // 128-bit two's-complement sums over the bins of coef[j][i] * g(k, i, b).  weight: n_bins x B in units of 2^-32 (AirWeights), or empty: none
    void HistProject(const std::vector<uint64_t>& hist, int K, int n_bins, int B, int channels, const std::vector<int32_t>& coef,
                     std::vector<uint64_t>& proj, const std::vector<uint32_t>& weight = {})
    {
        if (K < 0 || n_bins < 1 || B < 0 || channels < 0 || hist.size() != (size_t)K * (size_t)n_bins * (size_t)B * (size_t)channels)
            throw std::invalid_argument("HistProject: hist must hold K x n_bins x B x channels values");
        if (coef.empty() || coef.size() % (size_t)n_bins != 0) throw std::invalid_argument("HistProject: coef must hold J x n_bins values");
        if (!weight.empty() && weight.size() != (size_t)n_bins * (size_t)B) throw std::invalid_argument("HistProject: weight must hold n_bins x B values (or none)");
        const size_t J = coef.size() / (size_t)n_bins;
        proj.assign((size_t)K * (size_t)B * J * 2, 0);
        check(hare_hist_project(scene_, K, n_bins, B, channels, hist.data(), weight.empty() ? nullptr : weight.data(), (int32_t)J, coef.data(),
                                proj.data()));
    }
    // hare_hist_project_device on device pointers and a hipStream_t: d_proj (K x B x J x 2 uint64) written.  Stream-ordered.
    void HistProjectDevice(int K, int n_bins, int B, int channels, const void* d_hist, int J, const void* d_coef, void* d_proj,
                           const void* d_weight = nullptr, void* stream = nullptr)
    {
        check(hare_hist_project_device(scene_, K, n_bins, B, channels, d_hist, d_weight, J, d_coef, d_proj, stream));
    }
    // hare_hist_project_channels (include/hare_hip.h, "receivers", "Directional projection"): HistProject for every channel of hist, the
    // channels after W read as two's-complement int64.  proj: K x B x J x channels x 2, the lo and hi words of the exact 128-bit sums
    void HistProjectChannels(const std::vector<uint64_t>& hist, int K, int n_bins, int B, int channels, const std::vector<int32_t>& coef,
                             std::vector<uint64_t>& proj, const std::vector<uint32_t>& weight = {})
    {
        if (K < 0 || n_bins < 1 || B < 0 || channels < 0 || hist.size() != (size_t)K * (size_t)n_bins * (size_t)B * (size_t)channels)
            throw std::invalid_argument("HistProjectChannels: hist must hold K x n_bins x B x channels values");
        if (coef.empty() || coef.size() % (size_t)n_bins != 0) throw std::invalid_argument("HistProjectChannels: coef must hold J x n_bins values");
        if (!weight.empty() && weight.size() != (size_t)n_bins * (size_t)B)
            throw std::invalid_argument("HistProjectChannels: weight must hold n_bins x B values (or none)");
        const size_t J = coef.size() / (size_t)n_bins;
        proj.assign((size_t)K * (size_t)B * J * (size_t)channels * 2, 0);
        check(hare_hist_project_channels(scene_, K, n_bins, B, channels, hist.data(), weight.empty() ? nullptr : weight.data(), (int32_t)J,
                                         coef.data(), proj.data()));
    }
    // hare_hist_project_channels_device on device pointers and a hipStream_t: d_proj (K x B x J x channels x 2 uint64) written.  Stream-ordered.
    void HistProjectChannelsDevice(int K, int n_bins, int B, int channels, const void* d_hist, int J, const void* d_coef, void* d_proj,
                                   const void* d_weight = nullptr, void* stream = nullptr)
    {
        check(hare_hist_project_channels_device(scene_, K, n_bins, B, channels, d_hist, d_weight, J, d_coef, d_proj, stream));
    }
    // hare_hist_render (include/hare_hip.h, "receivers", "Rendering"): hist as Receive returns it (K x n_bins x B x channels), rendered to
    // impulse responses of M samples per bin -- noise from `seed`, filtered per band by taps (B x T), shaped by the histogram.  out:
    // K x channels x (n_bins * M).  weight: n_bins x B in units of 2^-32 (AirWeights), or empty: none
    void HistRender(const std::vector<uint64_t>& hist, int K, int n_bins, int B, int channels, int frac_bits, int M, const std::vector<double>& taps,
                    uint64_t seed, std::vector<double>& out, const std::vector<uint32_t>& weight = {})
    {
        if (K < 0 || n_bins < 0 || B < 1 || channels < 0 || M < 0 || hist.size() != (size_t)K * (size_t)n_bins * (size_t)B * (size_t)channels)
            throw std::invalid_argument("HistRender: hist must hold K x n_bins x B x channels values");
        if (taps.empty() || taps.size() % (size_t)B != 0) throw std::invalid_argument("HistRender: taps must hold B x T values");
        if (!weight.empty() && weight.size() != (size_t)n_bins * (size_t)B) throw std::invalid_argument("HistRender: weight must hold n_bins x B values (or none)");
        out.assign((size_t)K * (size_t)channels * (size_t)n_bins * (size_t)M, 0.0);
        check(hare_hist_render(scene_, K, n_bins, B, channels, hist.data(), weight.empty() ? nullptr : weight.data(), frac_bits, M,
                               (int32_t)(taps.size() / (size_t)B), taps.data(), seed, out.data()));
    }
    // hare_hist_render_device on device pointers and a hipStream_t: d_out (K x channels x n_bins x M doubles) written.  Stream-ordered.
    void HistRenderDevice(int K, int n_bins, int B, int channels, const void* d_hist, int frac_bits, int M, int T, const void* d_taps, uint64_t seed,
                          void* d_out, const void* d_weight = nullptr, void* stream = nullptr)
    {
        check(hare_hist_render_device(scene_, K, n_bins, B, channels, d_hist, d_weight, frac_bits, M, T, d_taps, seed, d_out, stream));
    }
    // hare_hist_impulses (include/hare_hip.h, "receivers", "Impulses"): a PER-SAMPLE histogram (SourcePaths with bin_len = c / fs;
    // K x n_bins x B x channels) turned into pressure rows, every non-empty (bin, band) an impulse of amplitude sqrt(energy) through that
    // band's row of taps (B x T).  The samples n0 .. n0 + n_out - 1 of the n_bins + T - 1; n_out < 0: everything from n0 on.  add false:
    // out becomes K x channels x n_out.  add true: out holds K x channels rows of equal length >= n_out (e.g. what HistRender wrote) and the
    // impulses are added onto the first n_out samples of each
    void HistImpulses(const std::vector<uint64_t>& hist, int K, int n_bins, int B, int channels, int frac_bits, const std::vector<double>& taps,
                      std::vector<double>& out, int64_t n0 = 0, int64_t n_out = -1, bool add = false, const std::vector<uint32_t>& weight = {})
    {
        if (K < 1 || n_bins < 1 || B < 1 || channels < 1 || hist.size() != (size_t)K * (size_t)n_bins * (size_t)B * (size_t)channels)
            throw std::invalid_argument("HistImpulses: hist must hold K x n_bins x B x channels values");
        if (taps.empty() || taps.size() % (size_t)B != 0) throw std::invalid_argument("HistImpulses: taps must hold B x T values");
        if (!weight.empty() && weight.size() != (size_t)n_bins * (size_t)B) throw std::invalid_argument("HistImpulses: weight must hold n_bins x B values (or none)");
        const int32_t T = (int32_t)(taps.size() / (size_t)B);
        if (n_out < 0) n_out = (int64_t)n_bins + T - 1 - n0;
        if (n0 < 0 || n_out < 1 || n0 + n_out > (int64_t)n_bins + T - 1) throw std::invalid_argument("HistImpulses: the window must lie within the n_bins + T - 1 samples");
        const size_t rows = (size_t)K * (size_t)channels;
        if (!add) out.assign(rows * (size_t)n_out, 0.0);
        if (out.empty() || out.size() % rows != 0 || out.size() / rows < (size_t)n_out)
            throw std::invalid_argument("HistImpulses: out must hold K x channels rows of at least n_out values");
        check(hare_hist_impulses(scene_, K, n_bins, B, channels, hist.data(), weight.empty() ? nullptr : weight.data(), frac_bits, T, taps.data(), n0, n_out,
                                 (int64_t)(out.size() / rows), add ? 1 : 0, out.data()));
    }
    // hare_hist_impulses_device on device pointers and a hipStream_t: the first n_out doubles of every row of d_out (K x channels x out_stride)
    // written, or added onto.  Stream-ordered.
    void HistImpulsesDevice(int K, int n_bins, int B, int channels, const void* d_hist, int frac_bits, int T, const void* d_taps, int64_t n0, int64_t n_out,
                            int64_t out_stride, bool add, void* d_out, const void* d_weight = nullptr, void* stream = nullptr)
    {
        check(hare_hist_impulses_device(scene_, K, n_bins, B, channels, d_hist, d_weight, frac_bits, T, d_taps, n0, n_out, out_stride, add ? 1 : 0, d_out, stream));
    }
    // hare_source_paths: the direct sound (direct) and the image sources of the first (image) and second order (image2, only with image) of the
    // scene's source alone, each standing for n_weight rays, into a zeroed histogram: K x n_bins x B (x 4, 9, 16 with directional and order)
    void SourcePaths(int top_index, int64_t n_weight, int n_bins, double bin_len, int frac_bits, std::vector<uint64_t>& hist, std::vector<uint64_t>& detections,
                     int K, int B, bool directional = false, int order = 1, bool direct = true, bool image = true, bool image2 = true)
    {
        const uint32_t flags = (directional ? HARE_RECEIVE_DIRECTIONAL | (order == 2 ? HARE_RECEIVE_ORDER2 : order == 3 ? HARE_RECEIVE_ORDER3 : 0u) : 0u) |
                               (direct ? HARE_RECEIVE_DIRECT : 0u) | (image ? HARE_RECEIVE_IMAGE : 0u) | (image2 ? HARE_RECEIVE_IMAGE2 : 0u);
        const size_t channels = directional ? (order == 3 ? 16 : order == 2 ? 9 : 4) : 1;
        if (K < 1 || B < 1 || n_bins < 1) throw std::invalid_argument("SourcePaths: K, B and n_bins must be >= 1");
        hist.assign((size_t)K * (size_t)n_bins * (size_t)B * channels, 0);
        detections.assign((size_t)K * 2, 0);
        check(hare_source_paths(scene_, kind_, top_index, n_weight, flags, n_bins, bin_len, frac_bits, hist.data(), detections.data()));
    }
    // first-order edge diffraction (include/hare_hip.h, "receivers", "Edge diffraction (first order)").  SetEdges: the diffracting edges of
    // Model[top_index] -- ends E x 6 (a, b), faces E x 2 (the polygons that meet in the edge, -1 for none), inv_lambda f_b / c per band; all
    // empty removes the table.  DiffractPaths: one diffracted path per (edge, receiver) pair whose receiver the source does not see, Maekawa's
    // 1 / (3 + 20 N), into a zeroed histogram K x n_bins x B (x 4, 9, 16 with directional and order); returns the pairs found
    // (std::runtime_error, HARE_E_NOMEM, when the scene yields more than max_pairs).  Add it to SourcePaths' histogram word by word.
    // DiffractDevice: the same ACCUMULATED on device pointers and a hipStream_t; d_work holds DiffractWorkBytes(K, max_pairs) bytes
    void SetEdges(int top_index, const std::vector<double>& ends, const std::vector<int32_t>& faces, const std::vector<double>& inv_lambda)
    {
        if (ends.size() % 6 != 0 || faces.size() * 3 != ends.size()) throw std::invalid_argument("SetEdges: ends must hold E x 6 values and faces E x 2");
        const bool none = ends.empty();
        check(hare_scene_set_edges(scene_, top_index, (int32_t)(ends.size() / 6), none ? nullptr : ends.data(), none ? nullptr : faces.data(),
                                   (int32_t)inv_lambda.size(), inv_lambda.empty() ? nullptr : inv_lambda.data()));
    }
    uint64_t DiffractPaths(int top_index, int64_t n_weight, int n_bins, double bin_len, int frac_bits, double max_detour, int64_t max_pairs,
                           std::vector<uint64_t>& hist, std::vector<uint64_t>& detections, int K, int B, bool directional = false, int order = 1)
    {
        const uint32_t flags = directional ? HARE_RECEIVE_DIRECTIONAL | (order == 2 ? HARE_RECEIVE_ORDER2 : order == 3 ? HARE_RECEIVE_ORDER3 : 0u) : 0u;
        const size_t channels = directional ? (order == 3 ? 16 : order == 2 ? 9 : 4) : 1;
        if (K < 1 || B < 1 || n_bins < 1) throw std::invalid_argument("DiffractPaths: K, B and n_bins must be >= 1");
        hist.assign((size_t)K * (size_t)n_bins * (size_t)B * channels, 0);
        detections.assign((size_t)K * 2, 0);
        uint64_t found = 0;
        check(hare_diffract_paths(scene_, kind_, top_index, n_weight, flags, n_bins, bin_len, frac_bits, max_detour, max_pairs, hist.data(),
                                  detections.data(), &found));
        return found;
    }
    static int64_t DiffractWorkBytes(int64_t K, int64_t max_pairs) { return HARE_DIFFRACT_WORK_BYTES(K, max_pairs); }
    void DiffractDevice(int top_index, int64_t n_weight, int n_bins, double bin_len, int frac_bits, double max_detour, int64_t max_pairs, void* d_work,
                        void* d_hist, void* d_detections, bool directional = false, void* stream = nullptr)
    {
        check(hare_diffract_device(scene_, kind_, top_index, n_weight, directional ? HARE_RECEIVE_DIRECTIONAL : 0u, n_bins, bin_len, frac_bits,
                                   max_detour, max_pairs, d_work, d_hist, d_detections, stream));
    }
    // hare_convolve (include/hare_hip.h, "receivers", "Convolution"): the R rows of N doubles in ir -- the rows HistRender writes, R = K x
    // channels -- each convolved in the time domain with the one signal x; the samples n0 .. n0 + n_out - 1 of the N + L - 1 of the full
    // convolution into out, R x n_out.  n_out < 0: everything from n0 on
    void Convolve(const std::vector<double>& ir, int64_t R, const std::vector<double>& x, std::vector<double>& out, int64_t n0 = 0, int64_t n_out = -1)
    {
        if (R < 1 || ir.empty() || ir.size() % (size_t)R != 0) throw std::invalid_argument("Convolve: ir must hold R x N values");
        if (x.empty()) throw std::invalid_argument("Convolve: x must hold the signal");
        const int64_t N = (int64_t)(ir.size() / (size_t)R), L = (int64_t)x.size();
        if (n_out < 0) n_out = N + L - 1 - n0;
        if (n0 < 0 || n_out < 1 || n0 + n_out > N + L - 1) throw std::invalid_argument("Convolve: the window must lie within the N + L - 1 samples");
        out.assign((size_t)R * (size_t)n_out, 0.0);
        check(hare_convolve(scene_, R, N, ir.data(), L, x.data(), n0, n_out, out.data()));
    }
    // hare_convolve_device on device pointers and a hipStream_t: d_y (R x n_out doubles) written.  Stream-ordered.
    void ConvolveDevice(int64_t R, int64_t N, const void* d_ir, int64_t L, const void* d_x, int64_t n0, int64_t n_out, void* d_y, void* stream = nullptr)
    {
        check(hare_convolve_device(scene_, R, N, d_ir, L, d_x, n0, n_out, d_y, stream));
    }
    // hare_decode (include/hare_hip.h, "receivers", "Decoding"): the K x C rows of N doubles in in -- the rows HistRender writes, C =
    // channels -- decoded through the O x C filters of T doubles in h (h[(o*C + c)*T + t]): output (k, o) sums over all c the row (k, c)
    // filtered by h[o, c].  The samples n0 .. n0 + n_out - 1 of the N + T - 1 into out, K x O x n_out.  n_out < 0: everything from n0 on
    void Decode(const std::vector<double>& in, int64_t K, int64_t C, const std::vector<double>& h, int64_t O, std::vector<double>& out, int64_t n0 = 0,
                int64_t n_out = -1)
    {
        if (K < 1 || C < 1 || in.empty() || in.size() % (size_t)(K * C) != 0) throw std::invalid_argument("Decode: in must hold K x C x N values");
        if (O < 1 || h.empty() || h.size() % (size_t)(O * C) != 0) throw std::invalid_argument("Decode: h must hold O x C x T values");
        const int64_t N = (int64_t)(in.size() / (size_t)(K * C)), T = (int64_t)(h.size() / (size_t)(O * C));
        if (n_out < 0) n_out = N + T - 1 - n0;
        if (n0 < 0 || n_out < 1 || n0 + n_out > N + T - 1) throw std::invalid_argument("Decode: the window must lie within the N + T - 1 samples");
        out.assign((size_t)(K * O) * (size_t)n_out, 0.0);
        check(hare_decode(scene_, K, C, N, in.data(), O, T, h.data(), n0, n_out, out.data()));
    }
    // hare_decode_device on device pointers and a hipStream_t: d_y (K x O x n_out doubles) written.  Stream-ordered.
    void DecodeDevice(int64_t K, int64_t C, int64_t N, const void* d_in, int64_t O, int64_t T, const void* d_h, int64_t n0, int64_t n_out, void* d_y,
                      void* stream = nullptr)
    {
        check(hare_decode_device(scene_, K, C, N, d_in, O, T, d_h, n0, n_out, d_y, stream));
    }
    // Receive / ReceiveSource with the histogram reduced on the device (hare_receive_batch_reduced / hare_receive_source_reduced): sums and
    // cross as HistReduce gives them on the histogram Receive returns; the histogram itself never comes down
    uint64_t ReceiveReduced(const std::vector<hare_ray>& rays, int top_index, int bounces, int n_bins, double bin_len, int frac_bits,
                            const Reduction& r, std::vector<uint64_t>& sums, std::vector<int32_t>& cross, std::vector<uint64_t>& detections,
                            const std::vector<double>* state_in = nullptr, std::vector<double>* state_out = nullptr, bool directional = false)
    {
        const int64_t K = GetOption("receivers"), B = Bands(top_index);
        const size_t n_state = (size_t)(1 + B) * rays.size();
        if (state_in && state_in->size() != n_state) throw std::invalid_argument("ReceiveReduced: state_in must hold (1 + B) x rays.size() values");
        const int n_win = check_reduction(r, n_bins, (int)B, "ReceiveReduced"), n_lev = (int)r.levels.size();
        sums.assign((size_t)(K * B) * (size_t)n_win * 4, 0);
        cross.assign((size_t)(K * B) * (size_t)n_lev, 0);
        detections.assign((size_t)(2 * K), 0);
        if (state_out) state_out->assign(n_state, 0.0);
        hare_counters c{};
        check(hare_receive_batch_reduced(scene_, kind_, top_index, (int64_t)rays.size(), rays.data(), nullptr, nullptr, bounces,
                                         directional ? HARE_RECEIVE_DIRECTIONAL : 0u, n_bins, bin_len, frac_bits,
                                         state_in ? state_in->data() : nullptr, state_out ? state_out->data() : nullptr,
                                         r.weight.empty() ? nullptr : r.weight.data(), n_win, r.windows.data(), n_lev, r.levels.data(), sums.data(),
                                         cross.data(), detections.data(), &c));
        return c.hits;
    }
    uint64_t ReceiveSourceReduced(int64_t n, int64_t first_ray, int top_index, int bounces, int n_bins, double bin_len, int frac_bits,
                                  const Reduction& r, std::vector<uint64_t>& sums, std::vector<int32_t>& cross, std::vector<uint64_t>& detections,
                                  std::vector<double>* state_out = nullptr, bool directional = false, bool direct = false, bool image = false,
                                  bool image2 = false)
    {
        if (n < 0) throw std::invalid_argument("ReceiveSourceReduced: n must be >= 0");
        const int64_t K = GetOption("receivers"), B = Bands(top_index);
        const int n_win = check_reduction(r, n_bins, (int)B, "ReceiveSourceReduced"), n_lev = (int)r.levels.size();
        sums.assign((size_t)(K * B) * (size_t)n_win * 4, 0);
        cross.assign((size_t)(K * B) * (size_t)n_lev, 0);
        detections.assign((size_t)(2 * K), 0);
        if (state_out) state_out->assign((size_t)(1 + B) * (size_t)n, 0.0);
        hare_counters c{};
        check(hare_receive_source_reduced(scene_, kind_, top_index, n, first_ray, bounces,
                                          (directional ? HARE_RECEIVE_DIRECTIONAL : 0u) | (direct ? HARE_RECEIVE_DIRECT : 0u) |
                                              (image ? HARE_RECEIVE_IMAGE : 0u) | (image2 ? HARE_RECEIVE_IMAGE2 : 0u),
                                          n_bins,
                                          bin_len, frac_bits, state_out ? state_out->data() : nullptr,
                                          r.weight.empty() ? nullptr : r.weight.data(), n_win, r.windows.data(), n_lev, r.levels.data(), sums.data(),
                                          cross.data(), detections.data(), &c));
        return c.hits;
    }
    void SetOption(const char* name, int64_t value) { check(hare_scene_set_option(scene_, name, value)); }
    int64_t GetOption(const char* name) const { int64_t v = 0; check(hare_scene_get_option(scene_, name, &v)); return v; }
    hare_scene* native() const { return scene_; }

protected:
    // what the library cannot check of a Reduction -- the sizes of its vectors; returns n_win
    static int check_reduction(const Reduction& r, int n_bins, int B, const char* who)
    {
        if (r.windows.size() % 2 != 0) throw std::invalid_argument(std::string(who) + ": windows must hold lo, hi pairs");
        if (!r.weight.empty() && (n_bins < 0 || B < 0 || r.weight.size() != (size_t)n_bins * (size_t)B))
            throw std::invalid_argument(std::string(who) + ": weight must hold n_bins x B values (or none)");
        return (int)(r.windows.size() / 2);
    }
    Spatial_Partition(const std::vector<const Topology*>& Model_in, int kind, int device) : Model(Model_in), kind_(kind)
    {
        std::vector<hare_topology_desc> d;
        for (const Topology* t : Model) d.push_back(t->desc());
        check(hare_scene_create(d.data(), (int32_t)d.size(), device, &scene_));
    }
    hare_scene* scene_ = nullptr;
    int kind_;
};

class Voxel_Grid : public Spatial_Partition {
public:
    Voxel_Grid(const std::vector<const Topology*>& Model_in, int Domain, int device = 0) : Spatial_Partition(Model_in, HARE_KIND_VOXEL, device)
    {
        check(hare_voxel_build(scene_, Domain));
        refresh();
    }
    Voxel_Grid(const std::vector<const Topology*>& Model_in, int MaxDomain, int Avg_polys, int device) : Spatial_Partition(Model_in, HARE_KIND_VOXEL, device)
    {
        check(hare_voxel_build_adaptive(scene_, MaxDomain, Avg_polys));
        refresh();
    }
    double Xdim() const { return info_.box_dims[0]; }
    double Ydim() const { return info_.box_dims[1]; }
    double Zdim() const { return info_.box_dims[2]; }
    std::array<double, 3> MinPt() const { return {{info_.obox_min[0], info_.obox_min[1], info_.obox_min[2]}}; }
    int VoxelCode(int X, int Y, int Z) const { return info_.ct * info_.ct * Z + info_.ct * X + Y; }          // Voxel_Grid.cs:264-267
    void VoxelDecode(int Code, int& X, int& Y, int& Z) const                                                    // :256-262
    {
        const int XYTot = info_.ct * info_.ct;
        Z = Code / XYTot;
        Code -= Z * XYTot;
        Y = Code / info_.ct;
        X = Code - Y * info_.ct;
    }
    void PointInVoxel(const double Pt[3], int& X, int& Y, int& Z) const                                         // :322-327
    {
        X = (int)std::floor((Pt[0] - info_.obox_min[0]) / info_.voxel_dims[0]);
        Y = (int)std::floor((Pt[1] - info_.obox_min[1]) / info_.voxel_dims[1]);
        Z = (int)std::floor((Pt[2] - info_.obox_min[2]) / info_.voxel_dims[2]);
    }
    int PointInVoxel(const double Pt[3]) const                                                                   // :329-332
    {
        int X, Y, Z;
        PointInVoxel(Pt, X, Y, Z);
        return VoxelCode(X, Y, Z);
    }
    const hare_voxel_info& info() const { return info_; }

private:
    void refresh()
    {
        check(hare_voxel_get_info(scene_, &info_));
        Char_Step = info_.char_step;
    }
    hare_voxel_info info_{};
};

class Octree : public Spatial_Partition {
public:
    Octree(const std::vector<const Topology*>& Model_In, int maxDepth, int maxPolygonsPerNode, int device = 0)
        : Spatial_Partition(Model_In, HARE_KIND_OCTREE, device)
    {
        check(hare_octree_build(scene_, maxDepth, maxPolygonsPerNode));
    }
};

class KDTree : public Spatial_Partition {
public:
    KDTree(const std::vector<const Topology*>& Model_In, int maxDepth, int maxPolygonsPerNode, int device = 0)
        : Spatial_Partition(Model_In, HARE_KIND_KDTREE, device)
    {
        check(hare_kdtree_build(scene_, maxDepth, maxPolygonsPerNode));
    }
};

}  // namespace Geometry
}  // namespace Hare
