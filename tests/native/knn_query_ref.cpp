// knn_query_ref.cpp — CPU reference of the k-nearest queries (rt_query_knn_device), a stand-alone program built by
// tests/knn_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with -fsanitize=address,undefined).  It answers every
// point twice with the arithmetic of csrc/point_tri.h:
//   (a) brute force: every triangle with d2 < limit2 (strictly), sorted ascending by (d2, original triangle index), cut at k - the
//       definition of the answer, no tree;
//   (b) a walk of the host-built BVH8 (csrc/bvh_build.cpp) under exactly the kernel's rule: a sorted list of at most k entries, a
//       bound that is limit2 while fewer than k are held and then the d2 of the last entry; a triangle is accepted iff d2 < limit2
//       and, with k held, (d2, index) lies below the last entry; a child box, a leaf slot or a popped entry is skipped only when
//       lb2 > bound (a NaN bound is entered, a tie is entered).  The order is the kernel's too - of a node's passing inner children
//       the nearest is kept aside and the others are pushed in slot order, then its passing leaf slots are tested, then the nearest
//       child is judged again - so the nodes it fetches and the triangles it tests, per point, are figures of the same walk.
// (a) == (b) entry for entry and bit for bit is the test of the culling argument; the GPU kernel is compared with (a).
//   knn_query_ref <mesh> <points> <rmax> <k> <out>
// mesh: raw float32, 9 per triangle (v0, v1, v2 as rt_set_mesh takes them); points: raw float32, 3 per point; rmax: raw float32, one
// per point (+inf: no limit); k: raw uint32, one per point, 1 .. 1024 - so that one run answers a batch under several k (a point that
// repeats the one before it bit for bit, radius included, reuses that point's sorted list; the walk is made anew).
// out: uint64 n, entries (= the sum of k), neighbours (a), neighbours (b), walk nodes, walk triangles, invalid points; then
// count i32[n] (a; -2: an invalid point), walk_count i32[n], nodes u32[n], tris u32[n], and the rows, k[i] entries each, one after the
// other: d2 f32, dist f32, tri i32 of (a), then d2 f32, tri i32 of (b).  Behind count the entries are +inf and -1; the row of an
// invalid point is NaN and -2.
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
    std::vector<Entry> held;                          // sorted, at most k
    std::vector<std::pair<uint32_t, float>> stack;    // (node, lb2): one pending sibling each

    void offer(float d2, uint32_t t, float limit2, uint32_t k, float& bound) {
        if (!(d2 < limit2)) return;  // (a NaN, +inf)
        const Entry e(d2, t);
        if (held.size() == k) {
            if (!(e < held.back())) return;
            held.pop_back();
        }
        held.insert(std::upper_bound(held.begin(), held.end(), e), e);
        if (held.size() == k) bound = held.back().first;
    }

    void run(rt::P3 p, float limit2, uint32_t k) {
        float bound = limit2;
        uint32_t cur = 0;
        const uint32_t none = 0xffffffffu;
        for (;;) {
            if (cur == none) {
                while (!stack.empty()) {
                    const std::pair<uint32_t, float> e = stack.back();
                    stack.pop_back();
                    if (!(e.second > bound)) {
                        cur = e.first;
                        break;
                    }
                }
                if (cur == none) return;
            }
            nodes++;
            const uint32_t* w = rt::node_at(b.nodes.data(), cur);
            float lb[8];
            uint32_t pass = 0;
            for (uint32_t s = 0; s < 8; s++) {
                const bool used = ((rt::node_leafmask(w) | rt::node_imask(w)) >> s) & 1u;
                lb[s] = used ? rt::child_lb2(w, s, p) : 0.0f;
                if (used && !(lb[s] > bound)) pass |= 1u << s;
            }
            uint32_t smin = 8;
            for (uint32_t s = 0; s < 8; s++)
                if (((pass & rt::node_imask(w)) >> s) & 1u)
                    if (smin == 8 || lb[s] < lb[smin]) smin = s;
            for (uint32_t s = 0; s < 8; s++)
                if ((((pass & rt::node_imask(w)) >> s) & 1u) && s != smin) stack.push_back(std::make_pair(rt::node_inner_child(w, s), lb[s]));
            for (uint32_t s = 0; s < 8; s++)
                if (((pass & rt::node_leafmask(w)) >> s) & 1u) {
                    tris++;
                    const uint32_t t = b.order[rt::node_leaf_tri(w, s)];
                    offer(m.d2(t, p), t, limit2, k, bound);
                }
            cur = (smin != 8 && !(lb[smin] > bound)) ? rt::node_inner_child(w, smin) : none;
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fputs("usage: knn_query_ref <mesh> <points> <rmax> <k> <out>\n", stderr);
        return 2;
    }
    std::vector<float> pts, rmax;
    std::vector<uint32_t> ks;
    if (!read_all(argv[2], pts) || pts.size() % 3) return fail("cannot read the points");
    const size_t n = pts.size() / 3;
    if (!read_all(argv[3], rmax) || rmax.size() != n) return fail("cannot read rmax");
    if (!read_all(argv[4], ks) || ks.size() != n) return fail("cannot read k");
    for (uint32_t k : ks)
        if (k == 0 || k > 1024) return fail("k must be 1 .. 1024");
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    std::vector<int32_t> count(n), walk_count(n), tri_a, tri_b;
    std::vector<uint32_t> nodes(n), tris(n);
    std::vector<float> d2_a, dist_a, d2_b;
    uint64_t total_nodes = 0, total_tris = 0, invalid_points = 0, found_a = 0, found_b = 0;
    std::vector<Entry> brute, sorted;  // sorted: the whole list of the point before this one, kept for a batch that asks one point under several k in a row
    bool have_sorted = false;
    for (size_t i = 0; i < n; i++) {
        const rt::P3 p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        const float r = rmax[i];
        const uint32_t k = ks[i];
        const float limit2 = rt::point_limit2(r);
        const bool invalid = !(rt::point_in_reach(p, reach) && r == r);
        brute.clear();
        Walk walk{m, b};
        const bool walked = !invalid && r > 0.0f && limit2 > 0.0f;
        const bool same = have_sorted && i > 0 && std::memcmp(&pts[3 * i], &pts[3 * (i - 1)], 12) == 0 && std::memcmp(&rmax[i], &rmax[i - 1], 4) == 0;
        if (walked) {
            if (!same) {
                sorted.clear();
                for (uint32_t t = 0; t < (uint32_t)m.n; t++) {
                    const float d2 = m.d2(t, p);
                    if (d2 < limit2) sorted.push_back(Entry(d2, t));
                }
                std::sort(sorted.begin(), sorted.end());
            }
            brute.assign(sorted.begin(), sorted.begin() + std::min<size_t>(sorted.size(), k));
            walk.run(p, limit2, k);
        }
        have_sorted = walked;
        invalid_points += invalid ? 1u : 0u;
        count[i] = invalid ? -2 : (int32_t)brute.size();
        walk_count[i] = invalid ? -2 : (int32_t)walk.held.size();
        found_a += brute.size();
        found_b += walk.held.size();
        nodes[i] = walk.nodes;
        tris[i] = walk.tris;
        total_nodes += walk.nodes;
        total_tris += walk.tris;
        for (uint32_t j = 0; j < k; j++) {
            const bool in_a = j < brute.size(), in_b = j < walk.held.size();
            d2_a.push_back(invalid ? nan : in_a ? brute[j].first : inf);
            dist_a.push_back(invalid ? nan : in_a ? std::sqrt(brute[j].first) : inf);
            tri_a.push_back(invalid ? -2 : in_a ? (int32_t)brute[j].second : -1);
            d2_b.push_back(invalid ? nan : in_b ? walk.held[j].first : inf);
            tri_b.push_back(invalid ? -2 : in_b ? (int32_t)walk.held[j].second : -1);
        }
    }
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[7] = {(uint64_t)n, (uint64_t)tri_a.size(), found_a, found_b, total_nodes, total_tris, invalid_points};
    const bool ok = std::fwrite(head, 8, 7, f) == 7 && write_all(f, count) && write_all(f, walk_count) && write_all(f, nodes) && write_all(f, tris) &&
                    write_all(f, d2_a) && write_all(f, dist_a) && write_all(f, tri_a) && write_all(f, d2_b) && write_all(f, tri_b);
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK points=%zu tris=%zu depth=%u neighbours/point=%.2f nodes/point=%.2f tris/point=%.2f\n", n, m.n, b.depth, n ? (double)found_a / n : 0.0,
                n ? (double)total_nodes / n : 0.0, n ? (double)total_tris / n : 0.0);
    return 0;
}
