// overlap_segment_ref.cpp — CPU reference of the overlap segments (rt_overlap_segments_device), a stand-alone
// program built by tests/section_exact.py with g++ -std=c++17 -ffp-contract=off (and once more with -fsanitize=address,undefined).
// Brute force over all pairs with the arithmetic of csrc/tri_overlap.h (which pairs are listed: cand and mask != 0, ascending by
// original triangle index - the list of overlap_query_ref.cpp's part (a)) and of csrc/tri_section.h (the segment of each listed pair).
// No tree.
//   overlap_segment_ref <mesh> <queries> <out> [<pairs>]
// mesh, queries: raw float32, 9 per triangle (the three vertices as rt_set_mesh takes them).  pairs (optional): raw int32, (query,
// triangle) twice per pair - pairs the caller wants answered whether they are listed or not.
// out: uint64 n, entries, invalid queries, pairs; then count i32[n] (-2: an invalid query), offsets i64[n + 1], and per entry of the
// brute-force CSR: tri i32, mask i32, seg f32 x 6, ends i32, d2 f32 x 15 (every pair b < c of set bits in lexicographic order, NaN for
// the others); then per pair of <pairs>: mask i32, seg f32 x 6, ends i32 (an invalid query or a triangle out of range: 0, NaN, -1).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raytracing_engine_amd/csrc/tri_section.h"
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

void push_segment(std::vector<float>& seg, const rt::Section& s) {
    for (float x : {s.p0.x, s.p0.y, s.p0.z, s.p1.x, s.p1.y, s.p1.z}) seg.push_back(x);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4 && argc != 5) {
        std::fputs("usage: overlap_segment_ref <mesh> <queries> <out> [<pairs>]\n", stderr);
        return 2;
    }
    std::vector<float> qs;
    std::vector<int32_t> pairs;
    if (!read_all(argv[2], qs) || qs.size() % 9) return fail("cannot read the queries");
    if (argc == 5 && (!read_all(argv[4], pairs) || pairs.size() % 2)) return fail("cannot read the pairs");
    const size_t n = qs.size() / 9;
    Mesh m;
    if (!ref::load_mesh(argv[1], m.v0, m.e1, m.e2, m.n)) return fail("cannot read the mesh");
    float maxabs = 1.0f;  // max(1, largest |coordinate| of v0, fl(v0 + e1), fl(v0 + e2)): build_bvh's maxabs (csrc/bvh_build.cpp)
    for (size_t i = 0; i < 3 * m.n; i++)
        maxabs = std::fmax(maxabs, std::fmax(std::fabs(m.v0[i]), std::fmax(std::fabs(m.v0[i] + m.e1[i]), std::fabs(m.v0[i] + m.e2[i]))));
    const float reach = ref::reach_of(maxabs);

    const auto query = [&](size_t i) {
        const float* p = &qs[9 * i];
        return rt::QueryTri{rt::P3{p[0], p[1], p[2]}, rt::P3{p[3], p[4], p[5]}, rt::P3{p[6], p[7], p[8]}};
    };
    std::vector<int32_t> count(n), tri, mask, ends, pair_mask, pair_ends;
    std::vector<int64_t> offsets(n + 1);
    std::vector<float> seg, d2, pair_seg;
    uint64_t invalid_queries = 0;
    float pair_d2[rt::kSectionPairs];
    for (size_t i = 0; i < n; i++) {
        const rt::QueryTri A = query(i);
        const bool invalid = !rt::tri_in_reach(A, reach);
        offsets[i] = (int64_t)tri.size();
        if (!invalid) {
            const rt::Box Q = rt::query_box(A);
            for (uint32_t t = 0; t < (uint32_t)m.n; t++) {
                const rt::P3 v0 = m.at(m.v0, t), e1 = m.at(m.e1, t), e2 = m.at(m.e2, t);
                if (!rt::overlap_cand(Q, v0, e1, e2) || !rt::overlap_mask(A, v0, e1, e2)) continue;  // the list is tri_overlap.h's
                const rt::Section s = rt::overlap_section(A, Q, v0, e1, e2, pair_d2);
                tri.push_back((int32_t)t);
                mask.push_back((int32_t)s.mask);
                ends.push_back(s.ends);
                push_segment(seg, s);
                d2.insert(d2.end(), pair_d2, pair_d2 + rt::kSectionPairs);
            }
        }
        invalid_queries += invalid ? 1u : 0u;
        count[i] = invalid ? -2 : (int32_t)(tri.size() - (size_t)offsets[i]);
    }
    offsets[n] = (int64_t)tri.size();
    for (size_t k = 0; k + 1 < pairs.size(); k += 2) {
        rt::Section s = rt::section_none();
        if (pairs[k] >= 0 && (size_t)pairs[k] < n && pairs[k + 1] >= 0 && (size_t)pairs[k + 1] < m.n) {
            const rt::QueryTri A = query((size_t)pairs[k]);
            const size_t t = (size_t)pairs[k + 1];
            if (rt::tri_in_reach(A, reach)) s = rt::overlap_section(A, rt::query_box(A), m.at(m.v0, t), m.at(m.e1, t), m.at(m.e2, t));
        }
        pair_mask.push_back((int32_t)s.mask);
        pair_ends.push_back(s.ends);
        push_segment(pair_seg, s);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot write the answers");
    const uint64_t head[4] = {(uint64_t)n, (uint64_t)tri.size(), invalid_queries, (uint64_t)pair_mask.size()};
    const bool ok = std::fwrite(head, 8, 4, f) == 4 && write_all(f, count) && write_all(f, offsets) && write_all(f, tri) && write_all(f, mask) && write_all(f, seg) &&
                    write_all(f, ends) && write_all(f, d2) && write_all(f, pair_mask) && write_all(f, pair_seg) && write_all(f, pair_ends);
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK queries=%zu tris=%zu entries=%zu pairs=%zu\n", n, m.n, tri.size(), pair_mask.size());
    return 0;
}
