// lbvh_ref.cpp — the device BVH build and the refit of DESIGN.md §6.9 / §6.10 restated on the CPU, stage by stage and by the
// simplest means that define the same function (tests/lbvh_exact.py; tests/test_lbvh_ref_host.py, tests/test_gpu_device_bvh_exact.py).
// The build is a deterministic function of the mesh, so the kernels' rt_read_bvh output must equal this program's byte for byte.
// Nothing here follows csrc/bvh_build_gpu.hip: the order is std::sort, the binary tree a top-down recursion on the highest
// differing key bit, the boxes recursive unions, the layout a queue.  Shared with the library are only the definitions that
// csrc/bvh_node.h holds for every builder (Box, tri_box, assign_slots, quantise, node_set_topology), which
// tests/native/bvh_node_check.cpp pins on their own.
//
//   lbvh_ref build MESH OUT              MESH: n x 9 fp32 (v0 v1 v2 per triangle)
//   lbvh_ref refit TOPO LEAF MESH OUT    TOPO: n_nodes x 20 u32 of which only the imask byte of word 3 and words 4-7 are read;
//                                        LEAF: n u32, the leaf order; MESH: the new vertices
// OUT, little-endian: six u64 (n, n_nodes, depth, number of level starts, number of keys, number of binary nodes), two f32 (M, pad),
// then the sorted keys (u64), the node words (n_nodes x 20 u32), the leaf order (n u32), the level starts (u32) and the binary
// radix tree in preorder (first, last, split: three u32 per internal node).  refit writes no keys, levels or binary nodes.
// Prints "OK ..." on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_engine_amd/csrc/bvh_node.h"
#include "ref_io.h"

using rt::Box;
using rt::kNodeWords;

namespace {

using ref::fail;
using ref::read_all;
using ref::write_all;

// §6.9 (1): M = the largest |coordinate| of the vertices p0, p0 + (p1 - p0), p0 + (p2 - p0) formed in fp32, at least 1
float measure(const std::vector<float>& v, size_t n) {
    float m = 1.0f;
    for (size_t t = 0; t < n; t++)
        for (int a = 0; a < 3; a++) {
            const float p0 = v[9 * t + a], p1 = p0 + (v[9 * t + 3 + a] - p0), p2 = p0 + (v[9 * t + 6 + a] - p0);
            m = std::max(m, std::max(std::fabs(p0), std::max(std::fabs(p1), std::fabs(p2))));
        }
    return m;
}

// §6.9 (2): the padded box of triangle t over p0, p0 + e1, p0 + e2 with the edges e = p - p0 formed in fp32
Box triangle_box(const std::vector<float>& v, size_t t, float pad) {
    const float* p = &v[9 * t];
    float e1[3], e2[3];
    for (int a = 0; a < 3; a++) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
    }
    return rt::tri_box(p, e1, e2, pad);
}

Box join(const Box& a, const Box& b) {
    Box r = a;
    r.grow(b);
    return r;
}

struct Written {
    uint64_t n = 0, depth = 0;
    float maxabs = 0, pad = 0;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> nodes, leaf, level_start, binary;
};

int write_out(const char* path, const Written& w) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return fail("cannot write the output file");
    const uint64_t head[6] = {w.n, w.nodes.size() / kNodeWords, w.depth, w.level_start.size(), w.keys.size(), w.binary.size() / 3};
    std::fwrite(head, 8, 6, f);
    std::fwrite(&w.maxabs, 4, 1, f);
    std::fwrite(&w.pad, 4, 1, f);
    write_all(f, w.keys);
    write_all(f, w.nodes);
    write_all(f, w.leaf);
    write_all(f, w.level_start);
    write_all(f, w.binary);
    const bool ok = std::fflush(f) == 0 && !std::ferror(f);
    std::fclose(f);
    if (!ok) return fail("short write");
    std::printf("OK n %llu nodes %llu depth %llu\n", (unsigned long long)head[0], (unsigned long long)head[1], (unsigned long long)head[2]);
    return 0;
}

// ---- build ----------------------------------------------------------------------------------------------------------------------
struct Binary {  // the radix tree over the sorted keys: a reference is an index into `inner`, or ~(sorted position) of a leaf
    struct Inner {
        int32_t left, right;
        uint32_t first, last, split;
        Box box;
    };
    std::vector<Inner> inner;
    std::vector<Box> leaf_box;  // by sorted position
    const Box& box(int32_t ref) const { return ref >= 0 ? inner[(size_t)ref].box : leaf_box[(size_t)~ref]; }
};

// §6.9 (5) and (6): the node over sorted positions [a, b], a < b, splits after the last key whose highest differing bit of
// key[a] ^ key[b] is clear (the keys are sorted and unique: those keys are a prefix of the range); its box is its children's union
int32_t subtree(const std::vector<uint64_t>& keys, uint32_t a, uint32_t b, Binary& bt) {
    if (a == b) return ~(int32_t)a;
    const uint64_t diff = keys[a] ^ keys[b];
    int top = 63;
    while (!((diff >> top) & 1u)) top--;
    uint32_t split = a;
    while (!((keys[split + 1] >> top) & 1u)) split++;
    const int32_t self = (int32_t)bt.inner.size();
    bt.inner.push_back({0, 0, a, b, split, Box::empty()});
    const int32_t left = subtree(keys, a, split, bt), right = subtree(keys, split + 1, b, bt);
    Binary::Inner& me = bt.inner[(size_t)self];
    me.left = left;
    me.right = right;
    me.box = join(bt.box(left), bt.box(right));
    return self;
}

int build(const char* mesh_path, const char* out_path) {
    std::vector<float> v;
    if (!read_all(mesh_path, v) || v.empty() || v.size() % 9) return fail("the mesh file does not hold n x 9 floats, n >= 1");
    const size_t n = v.size() / 9;
    if (n >= (1u << 28)) return fail("too many triangles");
    Written out;
    out.n = n;
    out.maxabs = measure(v, n);
    out.pad = 2e-5f * out.maxabs;
    const float pad = out.pad;

    // (3) keys: Morton code of the box centroid over the centroid bounds, then the triangle index
    std::vector<Box> tb(n);
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) lo[a] = std::numeric_limits<float>::infinity(), hi[a] = -lo[a];
    for (size_t t = 0; t < n; t++) {
        tb[t] = triangle_box(v, t, pad);
        for (int a = 0; a < 3; a++) {
            const float c = 0.5f * (tb[t].lo[a] + tb[t].hi[a]);
            lo[a] = std::min(lo[a], c);
            hi[a] = std::max(hi[a], c);
        }
    }
    out.keys.resize(n);
    for (size_t t = 0; t < n; t++) {
        uint32_t morton = 0;
        for (int a = 0; a < 3; a++) {
            const float c = 0.5f * (tb[t].lo[a] + tb[t].hi[a]), ext = hi[a] - lo[a];
            uint32_t cell = 0;
            if (ext > 0.0f) cell = (uint32_t)std::min(std::max((c - lo[a]) / ext * 1024.0f, 0.0f), 1023.0f);
            for (int bit = 0; bit < 10; bit++) morton |= ((cell >> bit) & 1u) << (3 * bit + (2 - a));  // x is the highest bit of each triple
        }
        out.keys[t] = ((uint64_t)morton << 32) | (uint64_t)t;
    }
    // (4) order
    std::sort(out.keys.begin(), out.keys.end());

    // (5), (6) binary tree and boxes
    Binary bt;
    bt.leaf_box.resize(n);
    for (size_t i = 0; i < n; i++) bt.leaf_box[i] = tb[(uint32_t)out.keys[i]];
    bt.inner.reserve(n);
    const int32_t root = subtree(out.keys, 0, (uint32_t)(n - 1), bt);
    for (const Binary::Inner& b : bt.inner) {
        out.binary.push_back(b.first);
        out.binary.push_back(b.last);
        out.binary.push_back(b.split);
    }

    // (7) collapse, breadth first: `level` holds the references (binary inner nodes, or the single leaf of a one-triangle mesh)
    // whose 8-wide nodes make up the current level, in node order
    std::vector<int32_t> level{root}, next;
    uint32_t n_nodes = 0, n_placed = 0;
    out.level_start.push_back(0);
    while (!level.empty()) {
        uint32_t next_child = n_nodes + (uint32_t)level.size();  // the first node of the next level
        next.clear();
        for (int32_t ref : level) {
            int32_t ch[8];
            int k;
            if (ref < 0) {  // n == 1: a root with one leaf
                ch[0] = ref;
                k = 1;
            } else {
                ch[0] = bt.inner[(size_t)ref].left;
                ch[1] = bt.inner[(size_t)ref].right;
                k = 2;
                while (k < 8) {
                    int best = -1;
                    float best_area = 0.0f;
                    for (int i = 0; i < k; i++) {
                        if (ch[i] < 0) continue;
                        const float area = bt.box(ch[i]).half_area();
                        if (best < 0 || area > best_area) best = i, best_area = area;  // strict: the first of equals stays
                    }
                    if (best < 0) break;
                    const Binary::Inner& open = bt.inner[(size_t)ch[best]];
                    ch[best] = open.left;
                    ch[k++] = open.right;
                }
            }
            Box by_entry[8], node_box = Box::empty();
            for (int i = 0; i < k; i++) {
                by_entry[i] = bt.box(ch[i]);
                node_box.grow(by_entry[i]);
            }
            int child_in[8];
            rt::assign_slots(by_entry, k, node_box, child_in);
            Box by_slot[8];
            uint32_t imask = 0, leafmask = 0;
            const uint32_t child_base = next_child, tri_base = n_placed;
            for (int s = 0; s < 8; s++) {
                if (child_in[s] < 0) continue;
                const int32_t c = ch[child_in[s]];
                by_slot[s] = by_entry[child_in[s]];
                if (c >= 0) {
                    imask |= 1u << s;
                    next.push_back(c);
                    next_child++;
                } else {
                    leafmask |= 1u << s;
                    out.leaf.push_back((uint32_t)out.keys[(size_t)~c]);
                    n_placed++;
                }
            }
            uint32_t w[kNodeWords] = {};
            rt::quantise(node_box, by_slot, imask | leafmask, w);
            rt::node_set_topology(w, imask, child_base, tri_base, leafmask);
            out.nodes.insert(out.nodes.end(), w, w + kNodeWords);
        }
        n_nodes += (uint32_t)level.size();
        out.level_start.push_back(n_nodes);
        out.depth++;
        level.swap(next);
    }
    if (n_placed != n) return fail("the collapse lost a triangle");
    return write_out(out_path, out);
}

// ---- refit (§6.10) ------------------------------------------------------------------------------------------------------------------
int refit(const char* topo_path, const char* leaf_path, const char* mesh_path, const char* out_path) {
    std::vector<uint32_t> topo, leaf;
    std::vector<float> v;
    if (!read_all(topo_path, topo) || topo.empty() || topo.size() % kNodeWords) return fail("the topology file does not hold n_nodes x 20 words");
    if (!read_all(leaf_path, leaf) || leaf.empty()) return fail("no leaf order");
    if (!read_all(mesh_path, v) || v.size() != 9 * leaf.size()) return fail("the mesh file does not hold 9 floats per leaf");
    const size_t n = leaf.size(), nn = topo.size() / kNodeWords;
    Written out;
    out.n = n;
    out.maxabs = measure(v, n);
    out.pad = 2e-5f * out.maxabs;
    out.leaf = leaf;
    out.nodes.assign(nn * kNodeWords, 0u);
    std::vector<Box> exact(nn);
    for (size_t k = nn; k-- > 0;) {  // breadth-first numbering: a node's children have larger indices than the node
        const uint32_t* in = &topo[k * kNodeWords];
        const uint32_t imask = in[3] >> 24, leafmask = in[6] & 0xffu & ~imask, child_base = in[4], tri_base = in[5];
        Box by_slot[8], node_box = Box::empty();
        uint32_t inner_seen = 0, leaves_seen = 0;
        for (int s = 0; s < 8; s++) {
            if ((imask >> s) & 1u) {
                const size_t c = (size_t)child_base + inner_seen++;
                if (c <= k || c >= nn) return fail("a child index does not lie behind its parent");
                by_slot[s] = exact[c];
            } else if ((leafmask >> s) & 1u) {
                const size_t li = (size_t)tri_base + leaves_seen++;
                if (li >= n || leaf[li] >= n) return fail("a leaf position or triangle index is out of range");
                by_slot[s] = triangle_box(v, leaf[li], out.pad);
            } else {
                continue;
            }
            node_box.grow(by_slot[s]);
        }
        uint32_t* w = &out.nodes[k * kNodeWords];
        rt::quantise(node_box, by_slot, imask | leafmask, w);
        w[3] |= imask << 24;
        for (int i = 4; i < 8; i++) w[i] = in[i];  // words 4-7 stay as they were
        exact[k] = node_box;
    }
    return write_out(out_path, out);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "build")) return build(argv[2], argv[3]);
    if (argc == 6 && !std::strcmp(argv[1], "refit")) return refit(argv[2], argv[3], argv[4], argv[5]);
    std::printf("usage: lbvh_ref build MESH OUT | lbvh_ref refit TOPO LEAF MESH OUT\n");
    return 2;
}
