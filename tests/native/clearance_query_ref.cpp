// clearance_query_ref.cpp — CPU reference of the clearance query (rt_query_clearance_device), a stand-alone
// program built by tests/clearance_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with -fsanitize=address,undefined).
// It answers every query triangle twice with the arithmetic of csrc/tri_dist.h:
//   (a) brute force: the lexicographic minimum of (d2, original triangle index) over ALL mesh triangles with d2 < limit2 - the
//       definition of the answer, no tree;
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) that skips a child box or a leaf only when
//       box_lb2 > the best d2 so far, leaves first, inner children nearest first - plus the nodes and the records it fetched, per query.
// (a) == (b) bit for bit is the test of the culling argument; the GPU kernel is compared with (a), its counters with (b).
//   clearance_query_ref <mesh> <queries> <out> [rmax | -] [pairs] [nopad]
// mesh, queries: raw float32, 9 per triangle (the three vertices as rt_set_mesh takes them); rmax: raw float32, one per query, or
// absent ("-").  pairs: raw int32 (query, triangle) pairs, or "-"; the d2 of each pair (tri_dist's) is appended to out as f32.
// nopad: the walk bounds against Q itself, without the padding (an experiment of the tests: the padding is what the proof needs).
// out: uint64 n, walk nodes, walk records; nodes u32[n], records u32[n]; then for (a) and for (b): tri i32[n], d2, uq, vq, um, vm,
// dist f32[n] each, cand i32[n] (which candidate of tri_dist won, -1: none), point_query f32[3n], point_mesh f32[3n].  Miss: tri -1,
// d2 = dist = inf, the rest NaN.  Invalid query: tri -2, everything NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raytracing_engine_amd/csrc/tri_dist.h"
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

struct Answer {
    float d2 = std::numeric_limits<float>::infinity();
    uint32_t id = 0xffffffffu;
    bool found = false;
};

void offer(const Mesh& m, uint32_t t, const rt::QueryTri& A, const rt::Box& Q, Answer& best) {
    const rt::TriDist td = rt::tri_dist(A, Q, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t));
    if (rt::nearer(td.d2, t, best.d2, best.id)) best = Answer{td.d2, t, true};
}

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint32_t nodes = 0, tris = 0;
    void visit(uint32_t node, const rt::QueryTri& A, const rt::Box& Q, const rt::Box& Qp, Answer& best) {
        nodes++;
        const uint32_t* w = rt::node_at(b.nodes.data(), node);
        float lb[8];
        for (uint32_t s = 0; s < 8; s++) lb[s] = rt::box_lb2(w, s, Qp);
        for (uint32_t s = 0; s < 8; s++)  // leaves first: they shrink the radius the inner children are judged by
            if (((rt::node_leafmask(w) >> s) & 1u) && !(lb[s] > best.d2)) {
                tris++;
                offer(m, b.order[rt::node_leaf_tri(w, s)], A, Q, best);
            }
        bool done[8] = {};
        for (;;) {  // inner children, nearest first; each judged when its turn comes
            int pick = -1;
            for (int s = 0; s < 8; s++)
                if (((rt::node_imask(w) >> s) & 1u) && !done[s] && (pick < 0 || lb[s] < lb[pick])) pick = s;
            if (pick < 0) break;
            done[pick] = true;
            if (!(lb[pick] > best.d2)) visit(rt::node_inner_child(w, (uint32_t)pick), A, Q, Qp, best);
        }
    }
};

struct Column {
    std::vector<int32_t> tri, cand;
    std::vector<float> d2, uq, vq, um, vm, dist, pq, pm;
    explicit Column(size_t n) : tri(n), cand(n), d2(n), uq(n), vq(n), um(n), vm(n), dist(n), pq(3 * n), pm(3 * n) {}
    void set(size_t i, const Mesh& m, const rt::QueryTri& A, const Answer& a, float limit2, int invalid) {
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        const bool hit = !invalid && a.found && a.d2 < limit2;
        tri[i] = invalid ? -2 : hit ? (int32_t)a.id : -1;
        d2[i] = invalid ? nan : hit ? a.d2 : inf;
        dist[i] = invalid ? nan : hit ? std::sqrt(a.d2) : inf;
        rt::P3 q{nan, nan, nan}, c{nan, nan, nan};
        rt::TriDist td{nan, nan, nan, nan, nan, -1};
        if (hit) {  // the winner once more, as the kernel does at retire
            const rt::Box Q = rt::query_box(A);
            td = rt::tri_dist(A, Q, m.at(m.v0, a.id), m.at(m.e1, a.id), m.at(m.e2, a.id));
            rt::tri_dist_points(A, m.at(m.v0, a.id), m.at(m.e1, a.id), m.at(m.e2, a.id), td, q, c);
        }
        uq[i] = td.uq, vq[i] = td.vq, um[i] = td.um, vm[i] = td.vm;
        cand[i] = hit ? td.cand : -1;
        pq[3 * i] = q.x, pq[3 * i + 1] = q.y, pq[3 * i + 2] = q.z;
        pm[3 * i] = c.x, pm[3 * i + 1] = c.y, pm[3 * i + 2] = c.z;
    }
    bool write(FILE* f) const {
        return write_all(f, tri) && write_all(f, d2) && write_all(f, uq) && write_all(f, vq) && write_all(f, um) && write_all(f, vm) && write_all(f, dist) &&
               write_all(f, cand) && write_all(f, pq) && write_all(f, pm);
    }
};

rt::QueryTri query_at(const std::vector<float>& qs, size_t i) {
    const float* p = &qs[9 * i];
    return rt::QueryTri{rt::P3{p[0], p[1], p[2]}, rt::P3{p[3], p[4], p[5]}, rt::P3{p[6], p[7], p[8]}};
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fputs("usage: clearance_query_ref <mesh> <queries> <out> [rmax | -] [pairs | -] [nopad]\n", stderr);
        return 2;
    }
    std::vector<float> qs, rmax;
    if (!read_all(argv[2], qs) || qs.size() % 9) return fail("cannot read the queries");
    const size_t n = qs.size() / 9;
    if (argc > 4 && std::strcmp(argv[4], "-") != 0 && (!read_all(argv[4], rmax) || rmax.size() != n)) return fail("cannot read rmax");
    const bool nopad = argc > 6 && std::strcmp(argv[6], "nopad") == 0;
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    Column brute(n), walked(n);
    std::vector<uint32_t> nodes(n), tris(n);
    uint64_t total_nodes = 0, total_tris = 0;
    for (size_t i = 0; i < n; i++) {
        const rt::QueryTri A = query_at(qs, i);
        const float r = rmax.empty() ? std::numeric_limits<float>::infinity() : rmax[i];
        const float limit2 = rt::point_limit2(r);
        const int invalid = !(rt::tri_in_reach(A, reach) && r == r);
        Answer a, w;
        Walk walk{m, b};
        if (!invalid && r > 0.0f && limit2 > 0.0f) {
            const rt::Box Q = rt::query_box(A);
            for (uint32_t t = 0; t < (uint32_t)m.n; t++) offer(m, t, A, Q, a);
            w.d2 = limit2;  // boxes beyond the limit are culled from the start, as the kernel does
            walk.visit(0, A, Q, nopad ? Q : rt::padded_query_box(A), w);
        }
        nodes[i] = walk.nodes, tris[i] = walk.tris;
        total_nodes += walk.nodes, total_tris += walk.tris;
        brute.set(i, m, A, a, limit2, invalid);
        walked.set(i, m, A, w, limit2, invalid);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[3] = {(uint64_t)n, total_nodes, total_tris};
    bool ok = std::fwrite(head, 8, 3, f) == 3 && write_all(f, nodes) && write_all(f, tris) && brute.write(f) && walked.write(f);
    if (argc > 5 && std::strcmp(argv[5], "-") != 0) {
        std::vector<int32_t> pairs;
        ok = ok && read_all(argv[5], pairs) && pairs.size() % 2 == 0;
        for (size_t k = 0; ok && k + 1 < pairs.size(); k += 2) {
            const size_t i = (size_t)pairs[k], t = (size_t)pairs[k + 1];
            if (pairs[k] < 0 || pairs[k + 1] < 0 || i >= n || t >= m.n) { ok = false; break; }
            const rt::QueryTri A = query_at(qs, i);
            const float d2 = rt::tri_dist(A, rt::query_box(A), m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t)).d2;
            ok = std::fwrite(&d2, 4, 1, f) == 1;
        }
    }
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK queries=%zu tris=%zu depth=%u nodes/query=%.2f records/query=%.2f\n", n, m.n, b.depth, n ? (double)total_nodes / n : 0.0,
                n ? (double)total_tris / n : 0.0);
    return 0;
}
