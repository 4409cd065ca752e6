// bvh_node_check.cpp — host test of csrc/bvh_node.h (tests/test_bvh_node_host.py): quantise() and assign_slots() called
// directly, on ordinary and on degenerate nodes (zero extent, a single child, every child at the same centre, non-finite
// boxes).  The de-quantised boxes must contain their inputs, empty slots must hold the inverted box, every child must get a
// slot of its own, and the words that quantise() does not own must stay as they were.  Prints OK.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../raytracing_engine_amd/csrc/bvh_node.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                 \
        }                                                             \
    } while (0)

using rt::Box;

static Box make(float x0, float y0, float z0, float x1, float y1, float z1) { return Box{{x0, y0, z0}, {x1, y1, z1}}; }

// plane q (0 .. 5: lo.xyz, hi.xyz) of slot s
static uint32_t plane(const uint32_t* w, int q, int s) { return (w[8 + 2 * q + s / 4] >> (8 * (s % 4))) & 0xffu; }

// slots, quantisation and topology words of one node with children `ch`
static int check_node(const std::vector<Box>& ch) {
    const int k = (int)ch.size();
    Box nb = Box::empty();
    for (const Box& b : ch) nb.grow(b);
    int child_in[8];
    rt::assign_slots(ch.data(), k, nb, child_in);
    int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0}, placed = 0;
    for (int s = 0; s < 8; s++) {
        CHECK(child_in[s] >= -1 && child_in[s] < k);
        if (child_in[s] < 0) continue;
        CHECK(seen[child_in[s]]++ == 0);  // a slot of its own
        placed++;
    }
    CHECK(placed == k);

    Box cb[8];
    uint32_t occ = 0;
    for (int s = 0; s < 8; s++)
        if (child_in[s] >= 0) {
            cb[s] = ch[child_in[s]];
            occ |= 1u << s;
        }
    uint32_t w[rt::kNodeWords];
    for (uint32_t& x : w) x = 0xdeadbeefu;
    rt::quantise(nb, cb, occ, w);
    CHECK(rt::node_imask(w) == 0);                                              // left for node_set_topology
    for (int i = 4; i < 8; i++) CHECK(w[i] == 0xdeadbeefu);                     // not quantise()'s words
    const uint32_t imask = occ & 0x55u, leafmask = occ & ~imask;
    const uint32_t w3 = w[3];
    rt::node_set_topology(w, imask, 17u, 40u, leafmask);
    CHECK((w[3] & 0x00ffffffu) == (w3 & 0x00ffffffu) && w[7] == 0);
    CHECK(rt::node_imask(w) == imask && rt::node_leafmask(w) == leafmask && rt::node_child_base(w) == 17u && rt::node_tri_base(w) == 40u);
    CHECK(rt::node_inner_count(w) == (uint32_t)__builtin_popcount(imask));
    uint32_t inner = 0, leaves = 0;
    for (uint32_t s = 0; s < 8; s++) {
        if ((imask >> s) & 1u) CHECK(rt::node_inner_child(w, s) == 17u + inner++);
        if ((leafmask >> s) & 1u) CHECK(rt::node_leaf_tri(w, s) == 40u + leaves++);
    }
    for (int a = 0; a < 3; a++) {
        const float p = rt::node_origin(w, a), sc = rt::node_scale(w, a);
        CHECK(p == nb.lo[a] && sc > 0.0f && std::isfinite(sc));
        CHECK(p + 255.0f * sc >= nb.hi[a]);  // the frame spans the node
        for (int s = 0; s < 8; s++) {
            const uint32_t ql = plane(w, a, s), qh = plane(w, 3 + a, s);
            if (!((occ >> s) & 1u)) {
                CHECK(ql == 255u && qh == 0u);  // inverted: no ray hits it
                continue;
            }
            CHECK(ql <= qh);
            const float lo = p + (float)ql * sc, hi = p + (float)qh * sc;  // fp32, as the kernels de-quantise
            CHECK(lo <= cb[s].lo[a] && hi >= cb[s].hi[a]);
        }
    }
    // the flatten's writers
    uint32_t moved[rt::kNodeWords], top[rt::kNodeWords];
    for (uint32_t i = 0; i < rt::kNodeWords; i++) moved[i] = top[i] = w[i];
    rt::node_relocate(moved, 1000u, 2000u);
    rt::node_leaves_to_inner(top, 77u);
    for (uint32_t i = 0; i < rt::kNodeWords; i++) {
        if (i != 4 && i != 5) CHECK(moved[i] == w[i]);
        if (i < 3 || i >= 8) CHECK(top[i] == w[i]);
    }
    CHECK(rt::node_child_base(moved) == 1000u && rt::node_tri_base(moved) == 2000u);
    CHECK(rt::node_imask(top) == occ && rt::node_leafmask(top) == 0 && rt::node_child_base(top) == 77u && rt::node_tri_base(top) == 0 && top[7] == 0);
    CHECK((top[3] & 0x00ffffffu) == (w[3] & 0x00ffffffu));
    return 0;
}

int main() {
    // ordinary nodes of 1 .. 8 children, small and large coordinates
    std::mt19937 rng(5);
    for (float size : {1e-3f, 1.0f, 3e4f}) {
        std::uniform_real_distribution<float> u(-size, size);
        for (int k = 1; k <= 8; k++)
            for (int rep = 0; rep < 50; rep++) {
                std::vector<Box> ch;
                for (int i = 0; i < k; i++) {
                    const float x = u(rng), y = u(rng), z = u(rng);
                    ch.push_back(make(x, y, z, x + std::fabs(u(rng)), y + std::fabs(u(rng)), z + std::fabs(u(rng))));
                }
                if (check_node(ch)) return 1;
            }
    }
    // zero extent: a point, a node flat in one axis, a node flat in all three with eight children
    if (check_node({make(1, 2, 3, 1, 2, 3)})) return 1;
    if (check_node({make(-1, 2, -1, 0, 2, 0), make(0, 2, 0, 1, 2, 1), make(-1, 2, 0, 0, 2, 1)})) return 1;
    if (check_node(std::vector<Box>(8, make(-4, 5, 6, -4, 5, 6)))) return 1;
    if (check_node({make(0, 0, 0, 0, 0, 0)})) return 1;
    // a single child: a root over one triangle
    if (check_node({make(-1, 5, -1, 1, 6, 1)})) return 1;
    if (check_node({make(-1e4f, -1e-3f, 0, 1e4f, 1e-3f, 1e-30f)})) return 1;
    // every child at the same centre: identical boxes, and nested ones
    if (check_node(std::vector<Box>(8, make(-1, 5, -1, 1, 6, 1)))) return 1;
    if (check_node(std::vector<Box>(5, make(0, 0, 0, 2, 2, 2)))) return 1;
    {
        std::vector<Box> nested;
        for (int i = 1; i <= 8; i++) nested.push_back(make(-1.0f * i, -2.0f * i, -0.5f * i, 1.0f * i, 2.0f * i, 0.5f * i));
        if (check_node(nested)) return 1;
    }
    // non-finite boxes (not for validated input): the scores are NaN, every child still gets a slot of its own and no index leaves its array
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        for (int k = 1; k <= 8; k++) {
            std::vector<Box> ch(k, make(-inf, -inf, -inf, inf, inf, inf));
            Box nb = make(-inf, -inf, -inf, inf, inf, inf);
            int child_in[8];
            rt::assign_slots(ch.data(), k, nb, child_in);
            int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0}, placed = 0;
            for (int s = 0; s < 8; s++)
                if (child_in[s] >= 0) {
                    CHECK(child_in[s] < k && seen[child_in[s]]++ == 0);
                    placed++;
                }
            CHECK(placed == k);
            ch.assign(k, make(nan, nan, nan, nan, nan, nan));
            rt::assign_slots(ch.data(), k, ch[0], child_in);
            placed = 0;
            for (int s = 0; s < 8; s++) placed += child_in[s] >= 0;
            CHECK(placed == k);
        }
    }
    // triangle helpers
    {
        const float p0[3] = {1, 2, 3}, e1[3] = {-1, 0, 2}, e2[3] = {0.5f, -3, 0};
        const Box b = rt::tri_box(p0, e1, e2, 0.25f);
        CHECK(b.lo[0] == -0.25f && b.lo[1] == -1.25f && b.lo[2] == 2.75f && b.hi[0] == 1.75f && b.hi[1] == 2.25f && b.hi[2] == 5.25f);
        CHECK(b.half_area() == 2.0f * 3.5f + 3.5f * 2.5f + 2.5f * 2.0f);
        float r[rt::kTriWords];
        rt::pack_tri_record(p0, e1, e2, 0x01020304u, true, r);
        uint32_t id, light;
        __builtin_memcpy(&id, &r[rt::kTriIdWord], 4);
        __builtin_memcpy(&light, &r[rt::kTriLightWord], 4);
        CHECK(r[0] == 1 && r[2] == 3 && r[3] == -1 && r[5] == 2 && r[6] == 0.5f && r[8] == 0 && id == 0x01020304u && light == 1u && r[11] == 0.0f);
        const float dark[3] = {0, 0, 0}, neg[3] = {-1, 0, -2}, lit[3] = {0, 0, 1e-30f};
        CHECK(!rt::is_emissive(dark) && !rt::is_emissive(neg) && rt::is_emissive(lit));
    }
    std::printf("OK\n");
    return 0;
}
