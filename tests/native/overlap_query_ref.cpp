// overlap_query_ref.cpp — CPU reference of the overlap queries (rt_count / fill / list_overlaps_device), a
// stand-alone program built by tests/overlap_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with
// -fsanitize=address,undefined).  It answers every query triangle twice with the arithmetic of csrc/tri_overlap.h:
//   (a) brute force: every mesh triangle with cand and mask != 0, ascending by original triangle index - the definition of the
//       answer, no tree;
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) that skips a child box or a leaf slot exactly when its
//       decoded box does not overlap the query's box (child_overlaps), children in slot order, its finds sorted the same way - plus
//       the nodes it fetched and the triangle records it fetched, per query.  The box is fixed, so the order of the walk changes neither.
// (a) == (b) entry for entry is the test of the culling argument; the GPU kernel is compared with (a), its counters with (b).
//   overlap_query_ref <mesh> <queries> <out>
// mesh, queries: raw float32, 9 per triangle (the three vertices as rt_set_mesh takes them).  out: uint64 n, overlaps (a), overlaps
// (b), walk nodes, walk records, invalid queries, cand pairs; then count i32[n] (a; -2: an invalid query), walk_count i32[n], nodes
// u32[n], tris u32[n], offsets i64[n + 1] (a), tri i32 and mask i32 of (a), tri i32 and mask i32 of (b), and every pair with cand,
// query-major and ascending by triangle: query i32, tri i32, mask i32 (0 included).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../raytracing_engine_amd/csrc/tri_overlap.h"
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
};

typedef std::pair<uint32_t, uint32_t> Entry;  // (original triangle index, mask)

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint32_t nodes = 0, tris = 0;
    void visit(uint32_t node, const rt::QueryTri& A, const rt::Box& Q, std::vector<Entry>& found) {
        nodes++;
        const uint32_t* w = rt::node_at(b.nodes.data(), node);
        for (uint32_t s = 0; s < 8; s++) {
            const bool leaf = (rt::node_leafmask(w) >> s) & 1u, inner = (rt::node_imask(w) >> s) & 1u;
            if (!leaf && !inner) continue;
            if (!rt::child_overlaps(w, s, Q)) continue;
            if (leaf) {
                tris++;
                const uint32_t t = b.order[rt::node_leaf_tri(w, s)];
                if (!rt::overlap_cand(Q, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t))) continue;
                const uint32_t mask = rt::overlap_mask(A, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t));
                if (mask) found.push_back(Entry(t, mask));
            } else {
                visit(rt::node_inner_child(w, s), A, Q, found);
            }
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fputs("usage: overlap_query_ref <mesh> <queries> <out>\n", stderr);
        return 2;
    }
    std::vector<float> qs;
    if (!read_all(argv[2], qs) || qs.size() % 9) return fail("cannot read the queries");
    const size_t n = qs.size() / 9;
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    std::vector<int32_t> count(n), walk_count(n), tri_a, mask_a, tri_b, mask_b, pair_q, pair_t, pair_m;
    std::vector<uint32_t> nodes(n), tris(n);
    std::vector<int64_t> offsets(n + 1);
    uint64_t total_nodes = 0, total_tris = 0, invalid_queries = 0;
    std::vector<Entry> walked;
    for (size_t i = 0; i < n; i++) {
        const float* p = &qs[9 * i];
        const rt::QueryTri A{rt::P3{p[0], p[1], p[2]}, rt::P3{p[3], p[4], p[5]}, rt::P3{p[6], p[7], p[8]}};
        const bool invalid = !rt::tri_in_reach(A, reach);
        walked.clear();
        Walk walk{m, b};
        offsets[i] = (int64_t)tri_a.size();
        if (!invalid) {
            const rt::Box Q = rt::query_box(A);
            for (uint32_t t = 0; t < (uint32_t)m.n; t++) {
                if (!rt::overlap_cand(Q, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t))) continue;
                const uint32_t mask = rt::overlap_mask(A, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t));
                pair_q.push_back((int32_t)i);
                pair_t.push_back((int32_t)t);
                pair_m.push_back((int32_t)mask);
                if (mask) {
                    tri_a.push_back((int32_t)t);
                    mask_a.push_back((int32_t)mask);
                }
            }
            walk.visit(0, A, Q, walked);
            std::sort(walked.begin(), walked.end());
        }
        invalid_queries += invalid ? 1u : 0u;
        count[i] = invalid ? -2 : (int32_t)(tri_a.size() - (size_t)offsets[i]);
        walk_count[i] = invalid ? -2 : (int32_t)walked.size();
        nodes[i] = walk.nodes;
        tris[i] = walk.tris;
        total_nodes += walk.nodes;
        total_tris += walk.tris;
        for (const Entry& e : walked) {
            tri_b.push_back((int32_t)e.first);
            mask_b.push_back((int32_t)e.second);
        }
    }
    offsets[n] = (int64_t)tri_a.size();
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[7] = {(uint64_t)n, (uint64_t)tri_a.size(), (uint64_t)tri_b.size(), total_nodes, total_tris, invalid_queries, (uint64_t)pair_q.size()};
    const bool ok = std::fwrite(head, 8, 7, f) == 7 && write_all(f, count) && write_all(f, walk_count) && write_all(f, nodes) && write_all(f, tris) &&
                    write_all(f, offsets) && write_all(f, tri_a) && write_all(f, mask_a) && write_all(f, tri_b) && write_all(f, mask_b) && write_all(f, pair_q) &&
                    write_all(f, pair_t) && write_all(f, pair_m);
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK queries=%zu tris=%zu depth=%u overlaps/query=%.2f nodes/query=%.2f records/query=%.2f\n", n, m.n, b.depth, n ? (double)tri_a.size() / n : 0.0,
                n ? (double)total_nodes / n : 0.0, n ? (double)total_tris / n : 0.0);
    return 0;
}
