// sweep_query_ref.cpp — CPU reference of the sphere-cast query (rt_query_sweeps_device), a stand-alone program
// built by tests/sweep_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with -fsanitize=address,undefined).
// It answers every item twice with the arithmetic of csrc/sweep_tri.h:
//   (a) brute force: the lexicographic minimum of (toi, original triangle index) over ALL mesh triangles with toi < tmax - the
//       definition of the answer, no tree, every candidate of every triangle evaluated (tcut = FLT_MAX);
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) that skips a child box or a leaf only when
//       sweep_child_bound > the best t so far, leaves first, inner children nearest first, and hands the best t to sweep_toi as
//       tcut - plus the nodes and the records it fetched, per item.
// (a) == (b) bit for bit is the test of the culling argument; the GPU kernel is compared with (a).
//   sweep_query_ref <mesh> <origins> <dirs> <radius> <out> [tmax | -] [mode] [pairs]
// mesh: raw float32, 9 per triangle; origins, dirs: raw float32, 3 per item; radius, tmax: raw float32, one per item.
// mode: all (default) | noedges | novertices | faceunchecked: the features sweep_toi is given (the mutated references of the
// contract's tests) | withhold: the brute force once more without the triangle that won.  pairs: raw int32 (item, triangle) pairs;
// the toi of each pair is appended to out as f32 (+inf: not touched).
// out: uint64 n, walk nodes, walk records, nodes in the tree; nodes u32[n], records u32[n]; then for (a) and for (b): t f32[n],
// tri i32[n], point f32[3n].  Miss: tri -1, t = inf, point NaN.  Invalid item: tri -2, everything NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raytracing_engine_amd/csrc/sweep_tri.h"
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
    float t;
    uint32_t id = 0xffffffffu;
    bool found = false;
};

void offer(const Mesh& m, uint32_t t, const rt::Sweep& s, uint32_t features, bool cut, Answer& best) {
    const rt::SweepToi toi = rt::sweep_toi(s, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t), cut ? best.t : rt::kSweepTmaxCap, features);
    if (toi.hit && rt::nearer(toi.t, t, best.t, best.id)) best = Answer{toi.t, t, true};
}

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint32_t features;
    uint32_t nodes = 0, tris = 0;
    void visit(uint32_t node, const rt::Sweep& s, const rt::SweepSlabs& sl, Answer& best) {
        nodes++;
        const uint32_t* w = rt::node_at(b.nodes.data(), node);
        float lb[8];
        for (uint32_t k = 0; k < 8; k++) lb[k] = rt::sweep_child_bound(w, k, s, sl);
        for (uint32_t k = 0; k < 8; k++)  // leaves first: they shrink the time the inner children are judged by
            if (((rt::node_leafmask(w) >> k) & 1u) && !(lb[k] > best.t)) {
                tris++;
                offer(m, b.order[rt::node_leaf_tri(w, k)], s, features, true, best);
            }
        bool done[8] = {};
        for (;;) {  // inner children, nearest first; each judged when its turn comes
            int pick = -1;
            for (int k = 0; k < 8; k++)
                if (((rt::node_imask(w) >> k) & 1u) && !done[k] && (pick < 0 || lb[k] < lb[pick])) pick = k;
            if (pick < 0) break;
            done[pick] = true;
            if (!(lb[pick] > best.t)) visit(rt::node_inner_child(w, (uint32_t)pick), s, sl, best);
        }
    }
};

struct Column {
    std::vector<float> t, point;
    std::vector<int32_t> tri;
    explicit Column(size_t n) : t(n), point(3 * n), tri(n) {}
    void set(size_t i, const Mesh& m, const rt::Sweep& s, const Answer& a, float tmax, bool invalid) {
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        const bool hit = !invalid && a.found && a.t < tmax;
        tri[i] = invalid ? -2 : hit ? (int32_t)a.id : -1;
        t[i] = invalid ? nan : hit ? a.t : inf;
        rt::P3 c{nan, nan, nan};
        if (hit) {  // the contact point from the record, as the kernel forms it at retire
            const rt::P3 v0 = m.at(m.v0, a.id), e1 = m.at(m.e1, a.id), e2 = m.at(m.e2, a.id);
            const rt::ClosestTri ct = rt::closest_on_tri(rt::sweep_centre(s.o, s.d, a.t), v0, e1, e2);
            c = rt::tri_point(v0, e1, e2, ct.u, ct.v);
        }
        point[3 * i] = c.x, point[3 * i + 1] = c.y, point[3 * i + 2] = c.z;
    }
    bool write(FILE* f) const { return write_all(f, t) && write_all(f, tri) && write_all(f, point); }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fputs("usage: sweep_query_ref <mesh> <origins> <dirs> <radius> <out> [tmax | -] [mode] [pairs]\n", stderr);
        return 2;
    }
    std::vector<float> os, ds, rs, tmaxs;
    if (!read_all(argv[2], os) || os.size() % 3) return fail("cannot read the origins");
    const size_t n = os.size() / 3;
    if (!read_all(argv[3], ds) || ds.size() != 3 * n) return fail("cannot read the directions");
    if (!read_all(argv[4], rs) || rs.size() != n) return fail("cannot read the radii");
    if (argc > 6 && std::strcmp(argv[6], "-") != 0 && (!read_all(argv[6], tmaxs) || tmaxs.size() != n)) return fail("cannot read tmax");
    const char* mode = argc > 7 ? argv[7] : "all";
    uint32_t features = rt::kSweepAll;
    bool withhold = false;
    if (!std::strcmp(mode, "noedges")) features &= ~rt::kSweepEdges;
    else if (!std::strcmp(mode, "novertices")) features &= ~rt::kSweepVertices;
    else if (!std::strcmp(mode, "faceunchecked")) features |= rt::kSweepFaceUnchecked;
    else if (!std::strcmp(mode, "withhold")) withhold = true;
    else if (std::strcmp(mode, "all") != 0) return fail("unknown mode");
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    const float inf = std::numeric_limits<float>::infinity();
    Column brute(n), walked(n);
    std::vector<uint32_t> nodes(n), tris(n);
    uint64_t total_nodes = 0, total_tris = 0;
    auto item = [&](size_t i) { return rt::Sweep{rt::P3{os[3 * i], os[3 * i + 1], os[3 * i + 2]}, rt::P3{ds[3 * i], ds[3 * i + 1], ds[3 * i + 2]}, rs[i]}; };
    for (size_t i = 0; i < n; i++) {
        const rt::Sweep s = item(i);
        const float tmax = tmaxs.empty() ? inf : tmaxs[i];
        const bool invalid = !rt::sweep_valid(s, tmax, reach);
        Answer a{rt::sweep_start_bound(tmax)}, w{rt::sweep_start_bound(tmax)};
        Walk walk{m, b, features};
        if (!invalid && tmax > 0.0f) {
            for (uint32_t t = 0; t < (uint32_t)m.n; t++) offer(m, t, s, features, false, a);
            if (withhold && a.found) {
                const uint32_t winner = a.id;
                a = Answer{rt::sweep_start_bound(tmax)};
                for (uint32_t t = 0; t < (uint32_t)m.n; t++)
                    if (t != winner) offer(m, t, s, features, false, a);
            }
            walk.visit(0, s, rt::sweep_slabs(s, reach), w);
        }
        nodes[i] = walk.nodes, tris[i] = walk.tris;
        total_nodes += walk.nodes, total_tris += walk.tris;
        brute.set(i, m, s, a, tmax, invalid);
        walked.set(i, m, s, w, tmax, invalid);
    }
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[4] = {(uint64_t)n, total_nodes, total_tris, (uint64_t)b.n_nodes};
    bool ok = std::fwrite(head, 8, 4, f) == 4 && write_all(f, nodes) && write_all(f, tris) && brute.write(f) && walked.write(f);
    if (argc > 8) {
        std::vector<int32_t> pairs;
        ok = ok && read_all(argv[8], pairs) && pairs.size() % 2 == 0;
        for (size_t k = 0; ok && k + 1 < pairs.size(); k += 2) {
            const size_t i = (size_t)pairs[k], t = (size_t)pairs[k + 1];
            if (pairs[k] < 0 || pairs[k + 1] < 0 || i >= n || t >= m.n) { ok = false; break; }
            const rt::SweepToi toi = rt::sweep_toi(item(i), m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t), rt::kSweepTmaxCap, features);
            const float v = toi.hit ? toi.t : inf;
            ok = std::fwrite(&v, 4, 1, f) == 1;
        }
    }
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK items=%zu tris=%zu depth=%u nodes/item=%.2f records/item=%.2f\n", n, m.n, b.depth, n ? (double)total_nodes / n : 0.0,
                n ? (double)total_tris / n : 0.0);
    return 0;
}
