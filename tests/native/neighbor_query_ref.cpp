// neighbor_query_ref.cpp — CPU reference of the neighbour queries (rt_count / fill / list_neighbors_device), a
// stand-alone program built by tests/neighbor_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with
// -fsanitize=address,undefined).  It answers every point twice with the arithmetic of csrc/point_tri.h:
//   (a) brute force: every triangle with d2 < limit2 (strictly), sorted ascending by (d2, original triangle index) - the definition
//       of the answer, no tree;
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) that skips a child box or a leaf slot exactly when
//       child_lb2 >= limit2 (a NaN bound is entered), children in slot order, its finds sorted the same way - plus the nodes it
//       fetched and the triangles it tested, per point.  The bound is fixed, so the order of the walk changes neither.
// (a) == (b) entry for entry and bit for bit is the test of the culling argument; the GPU kernel is compared with (a), its counters with (b).
//   neighbor_query_ref <mesh> <points> <rmax> <out>
// mesh: raw float32, 9 per triangle (v0, v1, v2 as rt_set_mesh takes them); points: raw float32, 3 per point; rmax: raw float32, one
// per point.  out: uint64 n, neighbours (a), neighbours (b), walk nodes, walk triangles, invalid points; then count i32[n] (a; -2: an
// invalid point), walk_count i32[n], nodes u32[n], tris u32[n], offsets i64[n + 1] (a), d2 f32, dist f32, tri i32 of (a), then
// d2 f32, tri i32 of (b).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../raytracing_engine_amd/csrc/point_tri.h"
#define REF_IO_TREE
#include "ref_io.h"

namespace {

using ref::fail;
using ref::read_all;
using ref::write_all;

struct Mesh {
    std::vector<float> v0, e1, e2;  // original order, edges formed in fp32 as rt_abi_mesh.hip forms them
    size_t n = 0;
    rt::P3 at(const std::vector<float>& a, size_t t) const { return rt::P3{a[3 * t], a[3 * t + 1], a[3 * t + 2]}; }
    float d2(uint32_t t, rt::P3 p) const { return rt::closest_on_tri(p, at(v0, t), at(e1, t), at(e2, t)).d2; }
};

typedef std::pair<float, uint32_t> Entry;  // (d2, original triangle index): std::pair's < is the list's order (no NaN gets in)

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint32_t nodes = 0, tris = 0;
    void visit(uint32_t node, rt::P3 p, float limit2, std::vector<Entry>& found) {
        nodes++;
        const uint32_t* w = rt::node_at(b.nodes.data(), node);
        for (uint32_t s = 0; s < 8; s++) {
            const bool leaf = (rt::node_leafmask(w) >> s) & 1u, inner = (rt::node_imask(w) >> s) & 1u;
            if (!leaf && !inner) continue;
            if (rt::child_lb2(w, s, p) >= limit2) continue;  // (false for a NaN bound: entered)
            if (leaf) {
                tris++;
                const uint32_t t = b.order[rt::node_leaf_tri(w, s)];
                const float d2 = m.d2(t, p);
                if (d2 < limit2) found.push_back(Entry(d2, t));
            } else {
                visit(rt::node_inner_child(w, s), p, limit2, found);
            }
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fputs("usage: neighbor_query_ref <mesh> <points> <rmax> <out>\n", stderr);
        return 2;
    }
    std::vector<float> pts, rmax;
    if (!read_all(argv[2], pts) || pts.size() % 3) return fail("cannot read the points");
    const size_t n = pts.size() / 3;
    if (!read_all(argv[3], rmax) || rmax.size() != n) return fail("cannot read rmax");
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    std::vector<int32_t> count(n), walk_count(n), tri_a, tri_b;
    std::vector<uint32_t> nodes(n), tris(n);
    std::vector<int64_t> offsets(n + 1);
    std::vector<float> d2_a, dist_a, d2_b;
    uint64_t total_nodes = 0, total_tris = 0, invalid_points = 0;
    std::vector<Entry> brute, walked;
    for (size_t i = 0; i < n; i++) {
        const rt::P3 p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        const float r = rmax[i];
        const float limit2 = rt::point_limit2(r);
        const bool invalid = !(rt::point_in_reach(p, reach) && r == r);
        brute.clear();
        walked.clear();
        Walk walk{m, b};
        if (!invalid && r > 0.0f && limit2 > 0.0f) {
            for (uint32_t t = 0; t < (uint32_t)m.n; t++) {
                const float d2 = m.d2(t, p);
                if (d2 < limit2) brute.push_back(Entry(d2, t));
            }
            walk.visit(0, p, limit2, walked);
            std::sort(brute.begin(), brute.end());
            std::sort(walked.begin(), walked.end());
        }
        invalid_points += invalid ? 1u : 0u;
        count[i] = invalid ? -2 : (int32_t)brute.size();
        walk_count[i] = invalid ? -2 : (int32_t)walked.size();
        nodes[i] = walk.nodes;
        tris[i] = walk.tris;
        total_nodes += walk.nodes;
        total_tris += walk.tris;
        offsets[i] = (int64_t)tri_a.size();
        for (const Entry& e : brute) {
            d2_a.push_back(e.first);
            dist_a.push_back(std::sqrt(e.first));
            tri_a.push_back((int32_t)e.second);
        }
        for (const Entry& e : walked) {
            d2_b.push_back(e.first);
            tri_b.push_back((int32_t)e.second);
        }
    }
    offsets[n] = (int64_t)tri_a.size();
    FILE* f = std::fopen(argv[4], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[6] = {(uint64_t)n, (uint64_t)tri_a.size(), (uint64_t)tri_b.size(), total_nodes, total_tris, invalid_points};
    const bool ok = std::fwrite(head, 8, 6, f) == 6 && write_all(f, count) && write_all(f, walk_count) && write_all(f, nodes) && write_all(f, tris) &&
                    write_all(f, offsets) && write_all(f, d2_a) && write_all(f, dist_a) && write_all(f, tri_a) && write_all(f, d2_b) && write_all(f, tri_b);
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK points=%zu tris=%zu depth=%u neighbours/point=%.2f nodes/point=%.2f tris/point=%.2f\n", n, m.n, b.depth, n ? (double)tri_a.size() / n : 0.0,
                n ? (double)total_nodes / n : 0.0, n ? (double)total_tris / n : 0.0);
    return 0;
}
