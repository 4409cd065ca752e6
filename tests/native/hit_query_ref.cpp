// hit_query_ref.cpp — CPU reference of the all-hits ray queries (rt_count_ray_hits_device / rt_fill_ray_hits_device /
// rt_list_ray_hits_device), a stand-alone program built by tests/hit_exact.py with g++ -std=c++17 -ffp-contract=off
// (and once more with -fsanitize=address,undefined).  It answers every ray with the arithmetic of csrc/ray_parity.h:
//   (a) brute force: ALL triangles that ray_tri_t accepts with 0 < t < tmax, sorted ascending by (t, original index) - the
//       definition of the answer, no tree;
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) with the kernels' slab test (node_step of
//       csrc/pt_traverse.h restated with scalar per-child code as tests/native/side_query_ref.cpp does; the ray in traversal form as
//       make_tray forms it: safe_inv's reciprocals, the octant by sign bit; tmax = +inf throughout, the caller's limit on the
//       triangle's t alone) that collects the same hits under the boxes the ray passes through, in walk order, and sorts them - plus the nodes it fetched and the
//       triangles it tested.
// (a) == (b), entry for entry and bit for bit, is the test of tree independence; the GPU kernel is compared with (a).
//   hit_query_ref <mesh> <rays> <out>
// mesh: raw float32, 9 per triangle (v0, v1, v2 as rt_set_mesh takes them); rays: raw float32, 7 per ray (origin, direction, tmax).
// out: uint64 n, hits, walk nodes, walk triangles, invalid rays; then i32 count[n] (-2: invalid ray, nothing else is computed for
// it), i32 walk_count[n], i32 same[n] (1: the walk's sorted list is the brute force's), i64 offsets[n + 1], f32 t[hits], i32 tri[hits].
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../raytracing_engine_amd/csrc/ray_parity.h"
#define REF_IO_TREE
#include "ref_io.h"

namespace {

using ref::fail;
using ref::read_all;

struct Mesh {
    std::vector<float> v0, e1, e2;  // original order, edges formed in fp32 as rt_abi_mesh.hip forms them
    size_t n = 0;
    rt::P3 at(const std::vector<float>& a, size_t t) const { return rt::P3{a[3 * t], a[3 * t + 1], a[3 * t + 2]}; }
};

typedef std::pair<float, int32_t> HitEntry;  // (t, original index): std::pair's order is the list's

// the triangle step of pt_query_hits
bool accepts(const Mesh& m, size_t i, rt::P3 o, rt::P3 d, float limit, float* t) {
    return rt::ray_tri_t(o, d, m.at(m.v0, i), m.at(m.e1, i), m.at(m.e2, i), *t) && *t > 0.0f && *t < limit;
}

float safe_inv(float d) {  // rt_device_math.h / pt_traverse.h
    const float x = std::fabs(d) > 1e-20f ? d : std::copysign(1e-20f, d);
    return 1.0f / x;
}

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint64_t nodes = 0, tris = 0;
    rt::P3 o{}, d{}, inv{}, noi{};
    bool pos[3] = {};
    float limit = 0.0f;
    std::vector<HitEntry> found;
    void start(rt::P3 o_, rt::P3 d_, float limit_) {
        o = o_;
        d = d_;
        inv = rt::P3{safe_inv(d.x), safe_inv(d.y), safe_inv(d.z)};
        noi = rt::P3{-(o.x * inv.x), -(o.y * inv.y), -(o.z * inv.z)};
        pos[0] = !std::signbit(d.x);
        pos[1] = !std::signbit(d.y);
        pos[2] = !std::signbit(d.z);
        limit = limit_;
        found.clear();
    }
    void visit(uint32_t node) {
        nodes++;
        const uint32_t* w = rt::node_at(b.nodes.data(), node);
        const uint8_t* q = reinterpret_cast<const uint8_t*>(&w[8]);  // qlo.x[8] qlo.y[8] qlo.z[8] qhi.x[8] qhi.y[8] qhi.z[8]
        const float iv[3] = {inv.x, inv.y, inv.z}, nv[3] = {noi.x, noi.y, noi.z};
        float a_[3], b_[3];
        for (int a = 0; a < 3; a++) {  // plane t = q * (s * inv) + (p * inv - o * inv)
            a_[a] = rt::node_scale(w, a) * iv[a];
            b_[a] = fmaf(rt::node_origin(w, a), iv[a], nv[a]);
        }
        const uint32_t imask = rt::node_imask(w), leafmask = rt::node_leafmask(w);
        for (uint32_t slot = 0; slot < 8; slot++) {
            const bool inner = (imask >> slot) & 1u, leaf = (leafmask >> slot) & 1u;
            if (!inner && !leaf) continue;
            float tn = 0.0f, tf = std::numeric_limits<float>::infinity();  // tmax = +inf: no box is culled against the limit
            for (int a = 0; a < 3; a++) {
                const float lo = (float)q[8 * a + slot], hi = (float)q[24 + 8 * a + slot];
                tn = std::fmax(tn, fmaf(pos[a] ? lo : hi, a_[a], b_[a]));
                tf = std::fmin(tf, fmaf(pos[a] ? hi : lo, a_[a], b_[a]));
            }
            if (std::signbit(tf - tn)) continue;  // the kernels collect sign bits of tf - tn
            if (leaf) {
                tris++;
                const uint32_t tri = b.order[rt::node_leaf_tri(w, slot)];
                float t;
                if (accepts(m, tri, o, d, limit, &t)) found.push_back(HitEntry(t, (int32_t)tri));
            } else {
                visit(rt::node_inner_child(w, slot));
            }
        }
    }
};

bool same_bits(const std::vector<HitEntry>& a, const std::vector<HitEntry>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (std::memcmp(&a[i].first, &b[i].first, 4) != 0 || a[i].second != b[i].second) return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fputs("usage: hit_query_ref <mesh> <rays> <out>\n", stderr);
        return 2;
    }
    std::vector<float> rays;
    if (!read_all(argv[2], rays) || rays.size() % 7) return fail("cannot read the rays");
    const size_t n = rays.size() / 7;
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    std::vector<int32_t> count(n), wcount(n), same(n), tri_out;
    std::vector<int64_t> offsets(n + 1);
    std::vector<float> t_out;
    std::vector<HitEntry> list;
    Walk walk{m, b};
    uint64_t invalid = 0;
    for (size_t i = 0; i < n; i++) {
        const float* r = &rays[7 * i];
        const rt::P3 o{r[0], r[1], r[2]}, d{r[3], r[4], r[5]};
        const float limit = r[6];
        offsets[i] = (int64_t)t_out.size();
        if (!(rt::point_in_reach(o, reach) && std::isfinite(d.x) && std::isfinite(d.y) && std::isfinite(d.z) && limit == limit)) {
            count[i] = -2;
            same[i] = 1;  // (two empty lists)
            invalid++;
            continue;
        }
        if (!(limit > 0.0f)) {  // an empty interval: count 0 without a walk
            same[i] = 1;
            continue;
        }
        list.clear();
        for (size_t k = 0; k < m.n; k++) {
            float t;
            if (accepts(m, k, o, d, limit, &t)) list.push_back(HitEntry(t, (int32_t)k));
        }
        std::sort(list.begin(), list.end());
        walk.start(o, d, limit);
        walk.visit(0);
        std::sort(walk.found.begin(), walk.found.end());
        count[i] = (int32_t)list.size();
        wcount[i] = (int32_t)walk.found.size();
        same[i] = same_bits(list, walk.found) ? 1 : 0;
        for (const HitEntry& h : list) {
            t_out.push_back(h.first);
            tri_out.push_back(h.second);
        }
    }
    offsets[n] = (int64_t)t_out.size();
    const size_t hits = t_out.size();
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[5] = {(uint64_t)n, (uint64_t)hits, walk.nodes, walk.tris, invalid};
    const auto put = [f](const void* p, size_t size, size_t items) { return items == 0 || std::fwrite(p, size, items, f) == items; };  // (an empty vector's data() may be null)
    const bool ok = put(head, 8, 5) && put(count.data(), 4, n) && put(wcount.data(), 4, n) && put(same.data(), 4, n) && put(offsets.data(), 8, n + 1) &&
                    put(t_out.data(), 4, hits) && put(tri_out.data(), 4, hits);
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK rays=%zu tris=%zu depth=%u hits=%zu invalid=%llu nodes/ray=%.2f tris/ray=%.2f\n", n, m.n, b.depth, hits, (unsigned long long)invalid,
                n ? (double)walk.nodes / (double)n : 0.0, n ? (double)walk.tris / (double)n : 0.0);
    return 0;
}
