// hit_attr_ref.cpp — CPU reference of the hit attributes (rt_query_rays_attr_device / rt_query_points_attr_device), a
// stand-alone program built by tests/attr_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with
// -fsanitize=address,undefined).  No tree: for every ray the winner is the lexicographic minimum of (t, original triangle index) over
// ALL triangles that §6.3's test accepts with 0 < t - the definition of the closest hit - found with csrc/hit_attr.h's u, v, det and
// ray_parity.h's t (the two restatements of tri_test must agree on every pair, or the program fails), on edges formed in fp32 as
// rt_abi_mesh.hip forms them; a winner at t >= tmax is a miss, as in the kernel.  Validity is the kernel's.
//   hit_attr_ref <mesh> <rays> <out> [tmax | -] [tris]
// mesh: raw float32, 9 per triangle (v0, v1, v2 as rt_set_mesh takes them); rays: raw float32, 6 per ray (origin, direction); tmax: raw
// float32, one per ray, or absent ("-").  tris: raw int32 triangle indices whose unit normals are appended to out, three f32 each - the
// normals for the (point, triangle) answers of point_query_ref: a normal depends on the triangle alone.
// out: uint64 n; t f32[n], tri i32[n], ub f32[n], vb f32[n], (u, v, det) f32[3n] as the test forms them, normal f32[3n].  Miss: tri -1,
// t = inf, the rest NaN.  Invalid ray: tri -2, everything NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raytracing_engine_amd/csrc/hit_attr.h"
#include "../../raytracing_engine_amd/csrc/ray_parity.h"
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

bool finite3(rt::P3 a) { return std::fabs(a.x) < INFINITY && std::fabs(a.y) < INFINITY && std::fabs(a.z) < INFINITY; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fputs("usage: hit_attr_ref <mesh> <rays> <out> [tmax | -] [tris]\n", stderr);
        return 2;
    }
    std::vector<float> raw, rays, tmax;
    if (!read_all(argv[2], rays) || rays.size() % 6) return fail("cannot read the rays");
    const size_t n = rays.size() / 6;
    if (argc > 4 && std::strcmp(argv[4], "-") != 0 && (!read_all(argv[4], tmax) || tmax.size() != n)) return fail("cannot read tmax");
    Mesh m;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n, &raw)) return fail("cannot read the mesh");
    float maxabs = 1.0f;  // over the vertices as given
    for (float x : raw) maxabs = std::fmax(maxabs, std::fabs(x));
    const float reach = ref::reach_of(maxabs);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    std::vector<float> t_out(n), ub(n), vb(n), uvd(3 * n), nrm(3 * n);
    std::vector<int32_t> tri_out(n);
    size_t hits = 0;
    for (size_t i = 0; i < n; i++) {
        const rt::P3 o{rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]}, d{rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
        const float limit = tmax.empty() ? inf : tmax[i];
        const bool valid = rt::point_in_reach(o, reach) && finite3(d) && limit == limit;
        float best_t = inf;
        uint32_t best_id = 0xffffffffu;
        bool found = false;
        if (valid && limit > 0.0f) {
            for (uint32_t k = 0; k < (uint32_t)m.n; k++) {
                const rt::P3 v0 = m.at(m.v0, k), e1 = m.at(m.e1, k), e2 = m.at(m.e2, k);
                float t = 0.0f;
                const bool line = rt::ray_tri_t(o, d, v0, e1, e2, t);
                if (line != rt::ray_uvdet_accepted(rt::ray_tri_uvdet(o, d, v0, e1, e2))) return fail("hit_attr.h and ray_parity.h disagree on a pair");
                if (line && t > 0.0f && (t < best_t || (t == best_t && k < best_id))) {
                    best_t = t;
                    best_id = k;
                    found = true;
                }
            }
        }
        const bool hit = found && best_t < limit;
        tri_out[i] = !valid ? -2 : hit ? (int32_t)best_id : -1;
        t_out[i] = !valid ? nan : hit ? best_t : inf;
        rt::RayUvDet a{nan, nan, nan};
        rt::Bary b{nan, nan};
        rt::P3 nn{nan, nan, nan};
        if (hit) {
            const rt::P3 v0 = m.at(m.v0, best_id), e1 = m.at(m.e1, best_id), e2 = m.at(m.e2, best_id);
            a = rt::ray_tri_uvdet(o, d, v0, e1, e2);
            b = rt::ray_bary(o, d, v0, e1, e2);
            nn = rt::unit_normal(e1, e2);
            hits++;
        }
        ub[i] = b.u;
        vb[i] = b.v;
        uvd[3 * i] = a.u;
        uvd[3 * i + 1] = a.v;
        uvd[3 * i + 2] = a.det;
        rt::write_attr(nullptr, nrm.data(), i, 0.0f, 0.0f, nn);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head = (uint64_t)n;
    bool ok = std::fwrite(&head, 8, 1, f) == 1 && write_all(f, t_out) && write_all(f, tri_out) && write_all(f, ub) && write_all(f, vb) && write_all(f, uvd) && write_all(f, nrm);
    size_t n_tris = 0;
    if (argc > 5) {
        std::vector<int32_t> tris;
        ok = ok && read_all(argv[5], tris);
        n_tris = tris.size();
        for (size_t k = 0; ok && k < tris.size(); k++) {
            float row[3] = {nan, nan, nan};
            if (tris[k] >= 0) {
                if ((size_t)tris[k] >= m.n) { ok = false; break; }
                rt::write_attr(nullptr, row, 0, 0.0f, 0.0f, rt::unit_normal(m.at(m.e1, (size_t)tris[k]), m.at(m.e2, (size_t)tris[k])));
            }
            ok = std::fwrite(row, 4, 3, f) == 3;
        }
    }
    std::fclose(f);
    if (!ok) return fail("short write or a bad triangle index");
    std::printf("OK rays=%zu tris=%zu hits=%zu normals=%zu\n", n, m.n, hits, n_tris);
    return 0;
}
