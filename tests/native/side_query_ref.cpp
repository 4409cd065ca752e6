// side_query_ref.cpp — CPU reference of the inside/outside query (rt_query_sides_device), a stand-alone program
// built by tests/sign_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with -fsanitize=address,undefined).
// It answers every point with the arithmetic of csrc/ray_parity.h:
//   (a) brute force: for each of the three directions the number of ALL triangles that ray_crosses accepts - the definition of
//       the answer, no tree - and from the three parities `inside` by the lazy rule, plus whether the third parity was needed;
//   (b) a plain recursive walk of the host-built BVH8 (csrc/bvh_build.cpp) with the kernels' slab test (node_step of
//       csrc/pt_traverse.h restated with scalar per-child code as tests/native/bvh8_walk.cpp does, tmax = +inf throughout, the
//       reciprocals and octants of parity_dir) that counts the same crossings under the boxes the ray passes through - plus the
//       nodes it fetched and the triangles it tested;
//   (c) the closest accepted triangle, the lexicographic minimum of (t, original index) over all triangles with t > 0, along the
//       three directions and, when a ray file is given, along caller-supplied rays: what the oracle's brute-force closest_hit
//       returns, which shows that the restated triangle test is §6.3's.
// (a) == (b) is the test of tree independence; the GPU kernel is compared with (a).
//   side_query_ref <mesh> <points> <out> [rays]
// mesh: raw float32, 9 per triangle (v0, v1, v2 as rt_set_mesh takes them); points: raw float32, 3 per point; rays: raw float32,
// 6 per ray (origin, direction).  out: uint64 n, walk nodes, walk triangles, third walks, rays; then i32 inside[n] (-2: invalid
// point, nothing else is computed for it), i32 third[n], i32 brute[3n], i32 walk[3n], f32 t[3n], i32 tri[3n] (miss: inf, -1); then
// per ray f32 t[rays], i32 tri[rays].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

struct Closest {
    float t = std::numeric_limits<float>::infinity();
    int32_t tri = -1;
};

// (a) and (c) for one ray: crossings over all triangles, the nearest accepted one
uint32_t brute(const Mesh& m, rt::P3 o, rt::P3 d, Closest* best) {
    uint32_t crossings = 0;
    for (size_t i = 0; i < m.n; i++) {
        float t;
        if (rt::ray_tri_t(o, d, m.at(m.v0, i), m.at(m.e1, i), m.at(m.e2, i), t) && t > 0.0f) {
            crossings++;
            if (t < best->t) {  // ascending index: the first of equals stays
                best->t = t;
                best->tri = (int32_t)i;
            }
        }
    }
    return crossings;
}

struct Walk {
    const Mesh& m;
    const rt::BvhResult& b;
    uint64_t nodes = 0, tris = 0;
    rt::P3 o{}, d{}, inv{}, noi{};
    bool pos[3] = {};
    uint32_t crossings = 0;
    void start(rt::P3 p, uint32_t k) {
        const rt::ParityDir pd = rt::parity_dir(k);
        o = p;
        d = pd.d;
        inv = pd.inv;
        noi = rt::P3{-(p.x * inv.x), -(p.y * inv.y), -(p.z * inv.z)};
        pos[0] = (pd.oct_inv & 4u) != 0u;
        pos[1] = (pd.oct_inv & 2u) != 0u;
        pos[2] = (pd.oct_inv & 1u) != 0u;
        crossings = 0;
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
            float tn = 0.0f, tf = std::numeric_limits<float>::infinity();  // tmax = +inf: nothing ever shrinks it
            for (int a = 0; a < 3; a++) {
                const float lo = (float)q[8 * a + slot], hi = (float)q[24 + 8 * a + slot];
                tn = std::fmax(tn, fmaf(pos[a] ? lo : hi, a_[a], b_[a]));
                tf = std::fmin(tf, fmaf(pos[a] ? hi : lo, a_[a], b_[a]));
            }
            if (std::signbit(tf - tn)) continue;  // the kernels collect sign bits of tf - tn
            if (leaf) {
                tris++;
                const uint32_t t = b.order[rt::node_leaf_tri(w, slot)];
                if (rt::ray_crosses(o, d, m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t))) crossings++;
            } else {
                visit(rt::node_inner_child(w, slot));
            }
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fputs("usage: side_query_ref <mesh> <points> <out> [rays]\n", stderr);
        return 2;
    }
    std::vector<float> pts, rays;
    if (!read_all(argv[2], pts) || pts.size() % 3) return fail("cannot read the points");
    if (argc > 4 && (!read_all(argv[4], rays) || rays.size() % 6)) return fail("cannot read the rays");
    const size_t n = pts.size() / 3, n_rays = rays.size() / 6;
    Mesh m;
    rt::BvhResult b;
    float reach;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    if (!ref::build_tree(m.v0, m.e1, m.e2, m.n, b, reach)) return fail("build failed");

    std::vector<int32_t> inside(n), third(n), cb(3 * n), cw(3 * n), ctri(3 * n, -1), rtri(n_rays, -1);
    std::vector<float> ct(3 * n, std::numeric_limits<float>::infinity()), rtt(n_rays, std::numeric_limits<float>::infinity());
    Walk walk{m, b};
    uint64_t thirds = 0;
    for (size_t i = 0; i < n; i++) {
        const rt::P3 p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (!rt::point_in_reach(p, reach)) {
            inside[i] = -2;
            continue;
        }
        for (uint32_t k = 0; k < (uint32_t)rt::kParityDirs; k++) {
            Closest best;
            cb[3 * i + k] = (int32_t)brute(m, p, rt::parity_dir(k).d, &best);
            ct[3 * i + k] = best.t;
            ctri[3 * i + k] = best.tri;
            walk.start(p, k);
            walk.visit(0);
            cw[3 * i + k] = (int32_t)walk.crossings;
        }
        third[i] = rt::needs_third_parity((uint32_t)cb[3 * i], (uint32_t)cb[3 * i + 1]) ? 1 : 0;
        thirds += (uint64_t)third[i];
        inside[i] = (int32_t)rt::side_of_parities((uint32_t)cb[3 * i], (uint32_t)cb[3 * i + 1], (uint32_t)cb[3 * i + 2]);
    }
    for (size_t r = 0; r < n_rays; r++) {
        Closest best;
        brute(m, rt::P3{rays[6 * r], rays[6 * r + 1], rays[6 * r + 2]}, rt::P3{rays[6 * r + 3], rays[6 * r + 4], rays[6 * r + 5]}, &best);
        rtt[r] = best.t;
        rtri[r] = best.tri;
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[5] = {(uint64_t)n, walk.nodes, walk.tris, thirds, (uint64_t)n_rays};
    const bool ok = std::fwrite(head, 8, 5, f) == 5 && std::fwrite(inside.data(), 4, n, f) == n && std::fwrite(third.data(), 4, n, f) == n &&
                    std::fwrite(cb.data(), 4, 3 * n, f) == 3 * n && std::fwrite(cw.data(), 4, 3 * n, f) == 3 * n && std::fwrite(ct.data(), 4, 3 * n, f) == 3 * n &&
                    std::fwrite(ctri.data(), 4, 3 * n, f) == 3 * n && std::fwrite(rtt.data(), 4, n_rays, f) == n_rays && std::fwrite(rtri.data(), 4, n_rays, f) == n_rays;
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK points=%zu tris=%zu depth=%u third=%llu nodes/walk=%.2f tris/walk=%.2f\n", n, m.n, b.depth, (unsigned long long)thirds,
                n ? (double)walk.nodes / (3.0 * n) : 0.0, n ? (double)walk.tris / (3.0 * n) : 0.0);
    return 0;
}
