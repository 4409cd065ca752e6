// point_query_ref.cpp — CPU reference of the closest-point query (rt_query_points_device), a stand-alone
// program built by tests/point_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with -fsanitize=address,undefined).
// It answers every point twice with the arithmetic of csrc/point_tri.h:
//   (a) brute force: the lexicographic minimum of (d2, original triangle index) over ALL triangles with d2 < limit2 - the
//       definition of the answer, no tree;
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) that skips a child box or a leaf only when
//       child_lb2 > the best d2 so far, children nearest first - plus the nodes it fetched and the triangles it tested.
// (a) == (b) bit for bit is the test of the culling argument; the GPU kernel is compared with (a).
//   point_query_ref <mesh> <points> <out> [rmax | -] [pairs]
// mesh: raw float32, 9 per triangle (v0, v1, v2 as rt_set_mesh takes them); points: raw float32, 3 per point; rmax: raw float32,
// one per point, or absent ("-").  pairs: raw int32 (point, triangle) pairs whose d2 is appended to out as f32 (the tie tests look at
// the candidates' own d2, not only at the winner's).  out: uint64 n, walk nodes, walk triangles; then for (a) and for (b): tri i32[n], d2 f32[n], u f32[n],
// v f32[n], dist f32[n], point f32[3n].  Miss: tri -1, d2 = dist = inf, the rest NaN.  Invalid point: tri -2, everything NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raytracing_engine_amd/csrc/point_tri.h"
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

struct Answer {
    float d2 = std::numeric_limits<float>::infinity();
    uint32_t id = 0xffffffffu;
    float u = 0.0f, v = 0.0f;
    bool found = false;
};

void offer(const Mesh& m, uint32_t t, rt::P3 p, Answer& best) {
    const rt::ClosestTri c = rt::closest_on_tri(p, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t));
    if (rt::nearer(c.d2, t, best.d2, best.id)) best = Answer{c.d2, t, c.u, c.v, true};
}

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint64_t nodes = 0, tris = 0;
    void visit(uint32_t node, rt::P3 p, Answer& best) {
        nodes++;
        const uint32_t* w = rt::node_at(b.nodes.data(), node);
        float lb[8];
        for (uint32_t s = 0; s < 8; s++) lb[s] = rt::child_lb2(w, s, p);
        for (uint32_t s = 0; s < 8; s++)  // leaves first: they shrink the radius the inner children are judged by
            if (((rt::node_leafmask(w) >> s) & 1u) && !(lb[s] > best.d2)) {
                tris++;
                offer(m, b.order[rt::node_leaf_tri(w, s)], p, best);
            }
        bool done[8] = {};
        for (;;) {  // inner children, nearest first; each judged when its turn comes
            int pick = -1;
            for (int s = 0; s < 8; s++)
                if (((rt::node_imask(w) >> s) & 1u) && !done[s] && (pick < 0 || lb[s] < lb[pick])) pick = s;
            if (pick < 0) break;
            done[pick] = true;
            if (!(lb[pick] > best.d2)) visit(rt::node_inner_child(w, (uint32_t)pick), p, best);
        }
    }
};

struct Column {
    std::vector<int32_t> tri;
    std::vector<float> d2, u, v, dist, c;
    explicit Column(size_t n) : tri(n), d2(n), u(n), v(n), dist(n), c(3 * n) {}
    void set(size_t i, const Mesh& m, rt::P3 p, const Answer& a, float limit2, int invalid) {
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        const bool hit = !invalid && a.found && a.d2 < limit2;
        tri[i] = invalid ? -2 : hit ? (int32_t)a.id : -1;
        d2[i] = invalid ? nan : hit ? a.d2 : inf;
        dist[i] = invalid ? nan : hit ? std::sqrt(a.d2) : inf;
        u[i] = hit ? a.u : nan;
        v[i] = hit ? a.v : nan;
        rt::P3 cp{nan, nan, nan};
        if (hit) cp = rt::tri_point(m.at(m.v0, a.id), m.at(m.e1, a.id), m.at(m.e2, a.id), a.u, a.v);
        (void)p;
        c[3 * i] = cp.x;
        c[3 * i + 1] = cp.y;
        c[3 * i + 2] = cp.z;
    }
    bool write(FILE* f) const {
        const size_t n = tri.size();
        return std::fwrite(tri.data(), 4, n, f) == n && std::fwrite(d2.data(), 4, n, f) == n && std::fwrite(u.data(), 4, n, f) == n &&
               std::fwrite(v.data(), 4, n, f) == n && std::fwrite(dist.data(), 4, n, f) == n && std::fwrite(c.data(), 4, 3 * n, f) == 3 * n;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fputs("usage: point_query_ref <mesh> <points> <out> [rmax | -] [pairs]\n", stderr);
        return 2;
    }
    std::vector<float> pts, rmax;
    if (!read_all(argv[2], pts) || pts.size() % 3) return fail("cannot read the points");
    const size_t n = pts.size() / 3;
    if (argc > 4 && std::strcmp(argv[4], "-") != 0 && (!read_all(argv[4], rmax) || rmax.size() != n)) return fail("cannot read rmax");
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    Column brute(n), walked(n);
    Walk walk{m, b};
    for (size_t i = 0; i < n; i++) {
        const rt::P3 p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        const float r = rmax.empty() ? std::numeric_limits<float>::infinity() : rmax[i];
        const float limit2 = rt::point_limit2(r);
        const int invalid = !(rt::point_in_reach(p, reach) && r == r);
        Answer a, w;
        if (!invalid && r > 0.0f && limit2 > 0.0f) {
            for (uint32_t t = 0; t < (uint32_t)m.n; t++) offer(m, t, p, a);
            w.d2 = limit2;  // boxes beyond the limit are culled from the start, as the kernel does
            walk.visit(0, p, w);
        }
        brute.set(i, m, p, a, limit2, invalid);
        walked.set(i, m, p, w, limit2, invalid);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[3] = {(uint64_t)n, walk.nodes, walk.tris};
    bool ok = std::fwrite(head, 8, 3, f) == 3 && brute.write(f) && walked.write(f);
    if (argc > 5) {
        std::vector<int32_t> pairs;
        ok = ok && read_all(argv[5], pairs) && pairs.size() % 2 == 0;
        for (size_t k = 0; ok && k + 1 < pairs.size(); k += 2) {
            const size_t i = (size_t)pairs[k], t = (size_t)pairs[k + 1];
            if (i >= n || t >= m.n) { ok = false; break; }
            const float d2 = rt::closest_on_tri(rt::P3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t)).d2;
            ok = std::fwrite(&d2, 4, 1, f) == 1;
        }
    }
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK points=%zu tris=%zu depth=%u nodes/point=%.2f tris/point=%.2f\n", n, m.n, b.depth, n ? (double)walk.nodes / n : 0.0, n ? (double)walk.tris / n : 0.0);
    return 0;
}
