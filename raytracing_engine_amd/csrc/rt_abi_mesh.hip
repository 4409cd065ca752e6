// rt_abi_mesh.hip — lifetime of path B's device mesh behind the C ABI: set (host and device build), chunk rebuild, refit,
// surfaces, read-back, the sharing of one resident mesh among the contexts that were given it, and the borrowing
// of a parent's mesh by its frame-slot lanes.  No reference counterpart
// (include/rt_abi.h, "Path B").  The frames that render the mesh are in rt_abi_pt.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <system_error>
#include <vector>

#include "bvh_build.h"
#include "bvh_node.h"
#include "mesh_registry.h"
#include "rt_internal.h"

using rt::Ctx;
using rt::DeviceMesh;
using rt::PtData;

namespace rt {
void pt_free_mesh(PtData& pt) {
    pt.borrowed = nullptr;  // the parent context holds those arrays
    pt.own.reset();         // the arrays go with their last holder
    pt.d_spill.reset();
    pt.spill_words = 0;
    pt.d_refit.reset();
    for (rt::Event& e : pt.ev_refit) e.reset();
    pt.stats = rt_pt_stats{};
}

// a device allocation of `c`'s device that holds at least `bytes` bytes from p on
int check_device_array(Ctx* c, const void* p, size_t bytes, const char* what) {
    if (!p) return c->fail(RT_ERR_INVALID, "%s is NULL", what);
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return c->fail(RT_ERR_INVALID, "%s is not a device pointer", what);
    }
    if (a.type != hipMemoryTypeDevice || a.device != c->device)
        return c->fail(RT_ERR_INVALID, "%s is not device memory of device %d (memory type %d, device %d)", what, c->device, (int)a.type, a.device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return c->fail(RT_ERR_INVALID, "%s: allocation range unknown", what);
    }
    if (static_cast<const char*>(p) + bytes > static_cast<const char*>(base) + size)
        return c->fail(RT_ERR_INVALID, "%s: the allocation holds fewer than the %zu bytes of %s", what, bytes, what);
    return RT_OK;
}
}  // namespace rt

namespace {

using rt::check_device_array;
using rt::pt_free_mesh;

// The mesh part of rt_pt_stats, from the record (and the host side of a two-level mesh) the context renders
void publish_mesh_stats(PtData& pt) {
    const DeviceMesh& m = pt.mesh();
    const rt::TwoLevelBvh* tl = pt.host() ? &pt.host()->tl : nullptr;
    rt_pt_stats& s = pt.stats;
    s.n_tris = m.n_tris;
    s.n_nodes = m.n_nodes;
    s.bvh_depth = m.depth;
    s.stack_need = m.stack_need;
    s.n_lights = m.n_lights;
    s.bvh_build_ms = m.build_ms;
    s.bvh_levels = tl ? 2u : 1u;
    s.blas_chunks = tl ? (uint32_t)tl->blas.size() : 0u;
    s.tlas_nodes = tl ? tl->tlas_nodes : 0u;
    s.ms_build_blas = tl ? (float)tl->ms_blas : 0.0f;
    s.ms_build_tlas = tl ? (float)tl->ms_tlas : 0.0f;
    s.ms_build_flatten = tl ? (float)tl->ms_flatten : 0.0f;
}

// leaf-order records [li0, li1) of the device triangle / material arrays from the host copies; surf (may be NULL = all Lambert):
// albedo.w per original triangle
void pack_leaf_range(const rt::BvhResult& bvh, const float* v0, const float* e1, const float* e2, const float* albedo, const float* emission,
                     const float* surf, size_t li0, size_t li1, float* tris, float* alb, float* emi) {
    for (size_t li = li0; li < li1; li++) {
        const uint32_t t = bvh.order[li];
        rt::pack_tri_record(&v0[3 * (size_t)t], &e1[3 * (size_t)t], &e2[3 * (size_t)t], t, rt::is_emissive(&emission[3 * (size_t)t]),
                            &tris[rt::kTriWords * (li - li0)]);
        for (int a = 0; a < 3; a++) {
            alb[4 * (li - li0) + a] = albedo[3 * (size_t)t + a];
            emi[4 * (li - li0) + a] = emission[3 * (size_t)t + a];
        }
        alb[4 * (li - li0) + 3] = surf ? surf[t] : 0.0f;
        emi[4 * (li - li0) + 3] = 0.0f;
    }
}

// level ranges of a breadth-first tree (both builders emit one): level 0 = the root, level d + 1 = the inner children of level d,
// consecutive.  Empty if the words do not describe such a tree of n_nodes nodes
std::vector<uint32_t> level_starts(const std::vector<uint32_t>& nodes, uint32_t n_nodes) {
    std::vector<uint32_t> start{0};
    uint32_t first = 0, count = n_nodes ? 1u : 0u;
    while (count) {
        if ((uint64_t)first + count > n_nodes) return {};
        uint64_t next = 0;
        for (uint32_t k = first; k < first + count; k++) next += rt::node_inner_count(rt::node_at(nodes.data(), k));
        first += count;
        start.push_back(first);
        if (next > n_nodes) return {};
        count = (uint32_t)next;
    }
    if (first != n_nodes) return {};
    return start;
}

void set_tree_shape(DeviceMesh& m, const rt::BvhResult& bvh) {  // what the record says about the tree in m.nodes
    m.n_nodes = bvh.n_nodes;
    m.depth = bvh.depth;
    m.stack_need = bvh.stack_need;
    m.pad = bvh.pad;
    m.maxabs = bvh.maxabs;
}

float ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// Everything that renders the context's mesh goes idle, the mesh is freed, the frame-slot lanes re-sync on their next submit
int retire_mesh(Ctx* c) {
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream.get()));
    rt::frames_drop_mesh(c);  // frame-slot lanes render with this mesh
    pt_free_mesh(c->pt);
    c->state_version++;
    return RT_OK;
}

// A finished mesh of either builder, or one that other contexts render already, becomes the context's mesh, after retire_mesh
void adopt_mesh(Ctx* c, std::shared_ptr<DeviceMesh> m) {
    c->pt.own = std::move(m);
    publish_mesh_stats(c->pt);
}

// ---- one resident mesh for the contexts that were given the same one --------------------------------------
// Host-built meshes only.  A listed mesh is complete (its uploads were waited for before it was listed) and nobody writes into it:
// a context that is about to passes detach_mesh first.
rt::WeakRegistry<DeviceMesh>& resident_meshes() {
    static auto* r = new rt::WeakRegistry<DeviceMesh>;  // never destroyed: contexts may be closed while the process exits
    return *r;
}

bool sharing_enabled() {  // RT_AMD_MESH_SHARING=0: every rt_set_mesh builds and uploads for itself
    const char* e = std::getenv("RT_AMD_MESH_SHARING");
    return !(e && e[0] == '0' && e[1] == 0);
}

uint32_t builder_constants() {
    uint32_t cost;
    const float cost_prim = rt::BvhResult{}.cost_prim;
    std::memcpy(&cost, &cost_prim, 4);
    return cost ^ rt::kBvhMaxDepth;
}

// A copy of `src` in device memory of its own, complete on return
int clone_mesh(Ctx* c, const DeviceMesh& src, DeviceMesh* m) {
    const size_t n = src.n_tris, n_lights = std::max<size_t>(src.n_lights, 1);
    if (!dalloc(m->nodes, src.cap_nodes * 5) || !dalloc(m->tris, n * 3) || !dalloc(m->albedo, n) || !dalloc(m->emission, n) || !dalloc(m->lights, n_lights))
        return c->fail(RT_ERR_OOM, "copy of a shared mesh of %u triangles (the mesh is unchanged)", src.n_tris);
    RT_HIP(c, hipMemcpy(m->nodes.get(), src.nodes.get(), (size_t)src.n_nodes * 80, hipMemcpyDeviceToDevice));
    RT_HIP(c, hipMemcpy(m->tris.get(), src.tris.get(), n * 48, hipMemcpyDeviceToDevice));
    RT_HIP(c, hipMemcpy(m->albedo.get(), src.albedo.get(), n * 16, hipMemcpyDeviceToDevice));
    RT_HIP(c, hipMemcpy(m->emission.get(), src.emission.get(), n * 16, hipMemcpyDeviceToDevice));
    RT_HIP(c, hipMemcpy(m->lights.get(), src.lights.get(), n_lights * 4, hipMemcpyDeviceToDevice));
    RT_HIP(c, hipDeviceSynchronize());  // null-stream copies before anything on the context's non-blocking streams
    m->n_tris = src.n_tris;
    m->n_nodes = src.n_nodes;
    m->n_lights = src.n_lights;
    m->depth = src.depth;
    m->stack_need = src.stack_need;
    m->pad = src.pad;
    m->maxabs = src.maxabs;
    m->build_ms = src.build_ms;
    m->cap_nodes = src.cap_nodes;
    m->has_surfaces = src.has_surfaces;
    m->level_start = src.level_start;
    if (src.host) m->host.reset(new rt::MeshHost(*src.host));
    return RT_OK;
}

// Copy on write: every entry point that writes into the context's mesh calls this first, after its last refusal.  On return the
// context is the mesh's only holder and the mesh is not listed, so no other context sees what is written: a mesh others render
// too is left to them (and stays listed) and the context goes on with a copy.  A failure leaves everything as it was.
int detach_mesh(Ctx* c) {
    PtData& pt = c->pt;
    if (!resident_meshes().shared_or_unlist(pt.own)) return RT_OK;
    auto copy = std::make_shared<DeviceMesh>();
    if (int rc = clone_mesh(c, *pt.own, copy.get())) return rc;
    // the context's own frames may still read the arrays it lets go of, which the other holders may free at any time
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream.get()));
    rt::frames_drop_mesh(c);
    pt.own = std::move(copy);
    return RT_OK;
}

// The host build: BVH (one or two levels), leaf-order records, upload, light list.  m->host: what a chunk rebuild needs (two levels only)
int build_mesh_host(Ctx* c, const float* verts, const float* albedo, const float* emission, uint32_t n_tris, uint32_t levels, uint32_t chunks, DeviceMesh* m) {
    std::unique_ptr<rt::MeshHost>* host = &m->host;
    const size_t n = n_tris;
    // spec section 6.1: edges are formed once, in fp32
    std::vector<float> v0(3 * n), e1(3 * n), e2(3 * n);
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            v0[3 * i + a] = verts[9 * i + a];
            e1[3 * i + a] = verts[9 * i + 3 + a] - verts[9 * i + a];
            e2[3 * i + a] = verts[9 * i + 6 + a] - verts[9 * i + a];
        }
    const auto t0 = std::chrono::steady_clock::now();
    rt::BvhResult bvh;
    if (levels == 2u) {
        host->reset(new rt::MeshHost());
        if (!rt::build_bvh_two_level(v0.data(), e1.data(), e2.data(), n_tris, chunks, rt::kBvhMaxDepth, &(*host)->tl, &bvh))
            return c->fail(RT_ERR_INVALID, "two-level BVH build failed");
    } else if (!rt::build_bvh(v0.data(), e1.data(), e2.data(), n_tris, rt::kBvhMaxDepth, &bvh)) {
        return c->fail(RT_ERR_INVALID, "BVH build failed");
    }
    m->build_ms = ms_since(t0);

    // leaf-order triangle records + materials; lights in ascending original index
    std::vector<float> tris(rt::kTriWords * n), alb(4 * n), emi(4 * n);
    pack_leaf_range(bvh, v0.data(), e1.data(), e2.data(), albedo, emission, nullptr, 0, n, tris.data(), alb.data(), emi.data());
    std::vector<uint32_t> leaf_pos(n);
    for (size_t li = 0; li < n; li++) leaf_pos[bvh.order[li]] = (uint32_t)li;
    std::vector<uint32_t> lights, light_ids;
    for (size_t t = 0; t < n; t++)
        if (rt::is_emissive(&emission[3 * t])) {
            lights.push_back(leaf_pos[t]);
            light_ids.push_back((uint32_t)t);
        }

    // a two-level mesh keeps room for the node count to move when a chunk is rebuilt
    m->cap_nodes = levels == 2u ? (size_t)bvh.n_nodes + bvh.n_nodes / 8 + 1024 : bvh.n_nodes;
    if (!dalloc(m->nodes, m->cap_nodes * 5) || !dalloc(m->tris, n * 3) || !dalloc(m->albedo, n) || !dalloc(m->emission, n) ||
        !dalloc(m->lights, std::max<size_t>(lights.size(), 1)))
        return c->fail(RT_ERR_OOM, "mesh of %u triangles", n_tris);
    RT_HIP(c, hipMemcpy(m->nodes.get(), bvh.nodes.data(), (size_t)bvh.n_nodes * 80, hipMemcpyHostToDevice));
    RT_HIP(c, hipMemcpy(m->tris.get(), tris.data(), n * 48, hipMemcpyHostToDevice));
    RT_HIP(c, hipMemcpy(m->albedo.get(), alb.data(), n * 16, hipMemcpyHostToDevice));
    RT_HIP(c, hipMemcpy(m->emission.get(), emi.data(), n * 16, hipMemcpyHostToDevice));
    if (!lights.empty()) RT_HIP(c, hipMemcpy(m->lights.get(), lights.data(), lights.size() * 4, hipMemcpyHostToDevice));
    RT_HIP(c, hipDeviceSynchronize());  // the uploads ran on the null stream; the context's streams are non-blocking and do not wait for it
    m->n_tris = n_tris;
    m->n_lights = (uint32_t)lights.size();
    set_tree_shape(*m, bvh);
    if (*host) {  // what a chunk rebuild needs: the mesh in original order and where the lights are
        rt::MeshHost& h = **host;
        h.v0.swap(v0);
        h.e1.swap(e1);
        h.e2.swap(e2);
        h.albedo.assign(albedo, albedo + 3 * n);
        h.emission.assign(emission, emission + 3 * n);
        h.light_ids.swap(light_ids);
    }
    if (levels == 1u) m->level_start = level_starts(bvh.nodes, bvh.n_nodes);  // what a refit walks
    return RT_OK;
}

int set_mesh_impl(Ctx* c, const float* verts, const float* albedo, const float* emission, uint32_t n_tris, const rt_mesh_options* opt) {
    if (!verts || !albedo || !emission) return c->fail(RT_ERR_INVALID, "mesh arrays must not be NULL");
    if (n_tris == 0 || n_tris >= (1u << 28)) return c->fail(RT_ERR_INVALID, "n_tris %u out of [1, 2^28)", n_tris);
    const uint32_t levels = opt ? opt->bvh_levels : 1u, chunks = opt && opt->blas_chunks ? opt->blas_chunks : 64u;
    if (levels != 1u && levels != 2u) return c->fail(RT_ERR_INVALID, "bvh_levels %u (1 or 2)", levels);
    if (chunks > 65536u) return c->fail(RT_ERR_INVALID, "blas_chunks %u > 65536", chunks);
    for (size_t i = 0; i < (size_t)n_tris * 9; i++)
        if (!std::isfinite(verts[i])) return c->fail(RT_ERR_INVALID, "vertex data is not finite at float %zu", i);
    if (int rc = rt::bind(c)) return rc;
    // the old mesh goes before the new one is built (peak device memory stays one mesh): a failure from here on leaves the context without a mesh
    if (int rc = retire_mesh(c)) return rc;
    const bool share = sharing_enabled();
    rt::MeshKey key;
    if (share) {
        key = rt::mesh_key(c->device, verts, albedo, emission, n_tris, levels, chunks, builder_constants());
        if (std::shared_ptr<DeviceMesh> resident = resident_meshes().find(key)) {  // another context renders this very mesh: no build, no upload
            adopt_mesh(c, std::move(resident));
            return RT_OK;
        }
    }
    auto m = std::make_shared<DeviceMesh>();
    if (int rc = build_mesh_host(c, verts, albedo, emission, n_tris, levels, chunks, m.get())) return rc;
    if (share) resident_meshes().insert(key, m);  // complete: build_mesh_host waited for its uploads
    adopt_mesh(c, std::move(m));
    return RT_OK;
}

int update_chunk_impl(Ctx* c, uint32_t chunk, const float* verts, uint32_t n_tris) {
    PtData& pt = c->pt;
    if (!pt.host()) return c->fail(RT_ERR_STATE, "rt_update_mesh_chunk needs a two-level mesh (rt_set_mesh_ex with bvh_levels = 2) owned by this context");
    const rt::TwoLevelBvh& tl = pt.host()->tl;
    if (chunk >= tl.blas.size()) return c->fail(RT_ERR_INVALID, "chunk %u of %zu", chunk, tl.blas.size());
    if (!verts) return c->fail(RT_ERR_INVALID, "verts is NULL");
    const uint32_t first = tl.first[chunk], count = tl.first[chunk + 1] - first;
    if (n_tris != count) return c->fail(RT_ERR_INVALID, "chunk %u holds %u triangles, verts holds %u (rt_mesh_chunk_info)", chunk, count, n_tris);
    for (size_t i = 0; i < (size_t)count * 9; i++)
        if (!std::isfinite(verts[i])) return c->fail(RT_ERR_INVALID, "vertex data is not finite at float %zu", i);
    if (int rc = rt::bind(c)) return rc;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream.get()));
    rt::frames_drop_mesh(c);  // lanes re-borrow the mesh on their next submit
    c->state_version++;
    if (int rc = detach_mesh(c)) return rc;  // from here on `tl` may be another context's
    rt::MeshHost& h = *pt.host();
    DeviceMesh& m = *pt.own;
    const auto t0 = std::chrono::steady_clock::now();
    // Transactional: the host copy and the chunk's bottom-level structure change first and are put back if anything up to
    // the device allocation fails; the device arrays are written only after everything host-side (and the node array's
    // regrow) has succeeded.  An upload that fails half-way leaves the device arrays undefined: the mesh is dropped then.
    std::vector<float> old((size_t)count * 9);
    auto swap_in = [&](const float* src, bool edges_formed) {
        for (uint32_t i = 0; i < count; i++) {
            const size_t t = h.tl.sorted[first + i];
            for (int a = 0; a < 3; a++) {
                h.v0[3 * t + a] = src[9 * (size_t)i + a];
                h.e1[3 * t + a] = edges_formed ? src[9 * (size_t)i + 3 + a] : src[9 * (size_t)i + 3 + a] - src[9 * (size_t)i + a];
                h.e2[3 * t + a] = edges_formed ? src[9 * (size_t)i + 6 + a] : src[9 * (size_t)i + 6 + a] - src[9 * (size_t)i + a];
            }
        }
    };
    for (uint32_t i = 0; i < count; i++) {
        const size_t t = h.tl.sorted[first + i];
        for (int a = 0; a < 3; a++) {
            old[9 * (size_t)i + a] = h.v0[3 * t + a];
            old[9 * (size_t)i + 3 + a] = h.e1[3 * t + a];
            old[9 * (size_t)i + 6 + a] = h.e2[3 * t + a];
        }
    }
    swap_in(verts, false);
    rt::BvhResult bvh, displaced;
    const uint32_t n = m.n_tris;
    bool built = false;
    try {
        built = rt::rebuild_chunk(h.v0.data(), h.e1.data(), h.e2.data(), n, chunk, rt::kBvhMaxDepth, &h.tl, &bvh, &displaced);
    } catch (...) {
        swap_in(old.data(), true);
        throw;  // guarded() turns it into a status; the mesh is as it was
    }
    if (!built) {
        swap_in(old.data(), true);
        return c->fail(RT_ERR_INVALID, "chunk rebuild refused: the moved vertices leave the coordinate range the mesh's box padding was chosen for (call rt_set_mesh_ex again)");
    }
    auto roll_back = [&]() {
        std::swap(h.tl.blas[chunk], displaced);
        swap_in(old.data(), true);
    };
    const float build_ms = ms_since(t0);
    rt::DevPtr<float4> new_nodes;  // only if the node array has to grow
    const size_t new_cap = (size_t)bvh.n_nodes + bvh.n_nodes / 8 + 1024;
    if (bvh.n_nodes > m.cap_nodes && !dalloc(new_nodes, new_cap * 5)) {
        roll_back();
        return c->fail(RT_ERR_OOM, "node array of %u nodes (the mesh is unchanged)", bvh.n_nodes);
    }
    // the chunk's triangles keep their range of the leaf order (chunks are laid out in chunk order); inside it the order is new
    size_t li0 = 0;
    for (uint32_t b = 0; b < chunk; b++) li0 += h.tl.blas[b].order.size();
    const size_t li1 = li0 + count;
    std::vector<float> tris, alb, emi;
    std::vector<uint32_t> leaf_of;
    try {
        tris.resize(rt::kTriWords * (size_t)count);
        alb.resize(4 * (size_t)count);
        emi.resize(4 * (size_t)count);
        pack_leaf_range(bvh, h.v0.data(), h.e1.data(), h.e2.data(), h.albedo.data(), h.emission.data(), h.surf.empty() ? nullptr : h.surf.data(), li0, li1,
                        tris.data(), alb.data(), emi.data());  // the surfaces stay with their triangles
        if (!h.light_ids.empty()) {  // lights are listed by leaf position, in ascending original index
            bool moved = false;
            for (size_t li = li0; li < li1 && !moved; li++) moved = std::binary_search(h.light_ids.begin(), h.light_ids.end(), bvh.order[li]);
            if (moved) {
                std::vector<uint32_t> leaf_pos(n);
                for (size_t li = 0; li < n; li++) leaf_pos[bvh.order[li]] = (uint32_t)li;
                leaf_of.resize(h.light_ids.size());
                for (size_t k = 0; k < h.light_ids.size(); k++) leaf_of[k] = leaf_pos[h.light_ids[k]];
            }
        }
    } catch (...) {
        roll_back();
        throw;
    }
    // commit to the device
    if (new_nodes) {
        m.nodes = std::move(new_nodes);
        m.cap_nodes = new_cap;
    }
    hipError_t e = hipMemcpy(m.nodes.get(), bvh.nodes.data(), (size_t)bvh.n_nodes * 80, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.tris.get() + li0 * 3, tris.data(), (size_t)count * 48, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.albedo.get() + li0, alb.data(), (size_t)count * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.emission.get() + li0, emi.data(), (size_t)count * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !leaf_of.empty()) e = hipMemcpy(m.lights.get(), leaf_of.data(), leaf_of.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();  // null-stream uploads before anything on the context's non-blocking streams
    if (e != hipSuccess) {
        pt_free_mesh(pt);  // host tree and device arrays may disagree: no frame may be traced against them
        return c->fail(RT_ERR_STATE, "chunk upload failed (%s): the mesh has been dropped, call rt_set_mesh_ex again", hipGetErrorString(e));
    }
    set_tree_shape(m, bvh);
    m.build_ms = build_ms;
    publish_mesh_stats(pt);
    return RT_OK;
}

int set_mesh_device_impl(Ctx* c, const void* verts, const void* albedo, const void* emission, uint32_t n_tris) {
    if (n_tris == 0 || n_tris >= (1u << 28)) return c->fail(RT_ERR_INVALID, "n_tris %u out of [1, 2^28)", n_tris);
    if (int rc = rt::bind(c)) return rc;
    if (int rc = check_device_array(c, verts, (size_t)n_tris * 36, "verts")) return rc;
    if (int rc = check_device_array(c, albedo, (size_t)n_tris * 12, "albedo")) return rc;
    if (int rc = check_device_array(c, emission, (size_t)n_tris * 12, "emission")) return rc;
    // the new mesh is complete before the old one is dropped: any failure up to here leaves the context as it was
    auto m = std::make_shared<DeviceMesh>();  // never listed: device-resident inputs are not compared
    if (int rc = rt::build_bvh_device(c, static_cast<const float*>(verts), static_cast<const float*>(albedo), static_cast<const float*>(emission), n_tris, m.get()))
        return rc;
    if (int rc = retire_mesh(c)) return rc;
    adopt_mesh(c, std::move(m));  // a device-built mesh is single-level
    return RT_OK;
}

int refit_mesh_device_impl(Ctx* c, const void* verts, uint32_t n_tris) {
    PtData& pt = c->pt;
    if (!pt.mesh().n_tris) return c->fail(RT_ERR_STATE, "no mesh has been set");
    if (pt.host()) return c->fail(RT_ERR_STATE, "rt_refit_mesh_device needs a single-level mesh (a two-level mesh updates with rt_update_mesh_chunk)");
    if (!pt.own || pt.own->level_start.size() < 2) return c->fail(RT_ERR_STATE, "rt_refit_mesh_device: the mesh is not refittable by this context");
    if (n_tris != pt.own->n_tris) return c->fail(RT_ERR_INVALID, "the mesh holds %u triangles, n_tris is %u", pt.own->n_tris, n_tris);
    if (int rc = rt::bind(c)) return rc;
    if (int rc = check_device_array(c, verts, (size_t)n_tris * 36, "verts")) return rc;
    if (!pt.d_refit) {  // first refit of this mesh: scratch and timing events, all of them or none, stay until the mesh is freed
        rt::DevPtr<char> scratch;
        rt::Event ev[2];
        if (!dalloc(scratch, rt::refit_scratch_size(pt.own->n_nodes))) return c->fail(RT_ERR_OOM, "refit scratch for %u nodes", pt.own->n_nodes);
        for (rt::Event& e : ev) RT_HIP_AS(c, rt::kTextEventCreate, rt::make_event(e));
        pt.d_refit = std::move(scratch);
        pt.ev_refit[0] = std::move(ev[0]);
        pt.ev_refit[1] = std::move(ev[1]);
    }
    // 1. validate and measure: the last point at which the call may refuse; nothing of the mesh has been written
    const float* v = static_cast<const float*>(verts);
    float maxabs = 0.0f;
    if (int rc = rt::refit_measure(c, v, n_tris, pt.d_refit.get(), pt.ev_refit[0].get(), &maxabs)) return rc;
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream.get()));
    if (int rc = detach_mesh(c)) return rc;  // a mesh other contexts render too is left to them
    DeviceMesh& m = *pt.own;
    // 2. commit: frame-slot lanes are idled (they re-borrow the mesh on their next submit), then the arrays are rewritten in place
    rt::frames_drop_mesh(c);
    c->state_version++;
    const float maxabs1 = std::max(maxabs, 1.0f), pad = 2e-5f * maxabs1;  // build_bvh's padding, for the NEW coordinate range
    float ms = 0.0f;
    if (int rc = rt::refit_write(c, v, n_tris, pad, m.n_nodes, m.nodes.get(), m.tris.get(), m.level_start, pt.d_refit.get(), pt.ev_refit[0].get(), pt.ev_refit[1].get(), &ms)) {
        (void)rc;
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        const std::string why = c->err;
        pt_free_mesh(pt);  // boxes and records may disagree: no frame may be traced against them
        return c->fail(RT_ERR_STATE, "refit failed after the mesh was written (%s): the mesh has been dropped, set it again", why.c_str());
    }
    m.maxabs = maxabs1;
    m.pad = pad;
    m.build_ms = ms;
    publish_mesh_stats(pt);
    return RT_OK;
}

// DESIGN.md §6.11.  Everything is checked on the host before anything is written: a refusal leaves the surfaces as they were
int set_surfaces_impl(Ctx* c, const uint32_t* kind, const float* ior, uint32_t n_tris) {
    PtData& pt = c->pt;
    if (!pt.own) return c->fail(RT_ERR_STATE, "no mesh has been set");  // none, or a borrowed one
    if (n_tris != pt.own->n_tris) return c->fail(RT_ERR_INVALID, "the mesh holds %u triangles, n_tris is %u", pt.own->n_tris, n_tris);
    // surface word per triangle, the leaf-order albedo.w: 0 Lambert, -1 mirror, eta glass.  Empty: all Lambert
    std::vector<float> w;
    if (kind) {
        w.assign(n_tris, 0.0f);
        bool any = false;
        for (uint32_t i = 0; i < n_tris; i++) {
            if (kind[i] == RT_SURFACE_LAMBERT) continue;
            if (kind[i] == RT_SURFACE_MIRROR) {
                w[i] = -1.0f;
            } else if (kind[i] == RT_SURFACE_GLASS) {
                if (!ior) return c->fail(RT_ERR_INVALID, "triangle %u is glass and ior is NULL", i);
                if (!(std::isfinite(ior[i]) && ior[i] >= 1.0f && ior[i] <= 4.0f))
                    return c->fail(RT_ERR_INVALID, "triangle %u: index of refraction %g outside [1, 4]", i, (double)ior[i]);
                w[i] = ior[i];
            } else {
                return c->fail(RT_ERR_INVALID, "triangle %u: surface kind %u (0 .. 2)", i, kind[i]);
            }
            any = true;
        }
        if (!any) w.clear();
    }
    if (int rc = rt::bind(c)) return rc;
    rt::DevPtr<float> d_w;
    if (!w.empty() && !dalloc(d_w, w.size())) return c->fail(RT_ERR_OOM, "surface words of %u triangles", n_tris);
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream.get()));
    if (int rc = detach_mesh(c)) return rc;  // a mesh other contexts render too is left to them
    DeviceMesh& m = *pt.own;
    // commit: frame-slot lanes are idled (they re-borrow the mesh and its flag on their next submit), then albedo.w is rewritten
    // on the context's stream behind the frames already enqueued there
    rt::frames_drop_mesh(c);
    c->state_version++;
    hipError_t e = d_w ? hipMemcpyAsync(d_w.get(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, c->stream) : hipSuccess;
    const int rc = e == hipSuccess ? rt::launch_pt_scatter_surfaces(c, m.tris.get(), d_w.get(), m.albedo.get(), n_tris) : RT_OK;
    if (e == hipSuccess && rc == RT_OK) e = hipStreamSynchronize(c->stream);  // d_w is read until here
    if (e != hipSuccess || rc != RT_OK) {
        (void)hipGetLastError();
        pt_free_mesh(pt);  // some albedo.w may have been written: no frame may be traced against half the surfaces
        return c->fail(RT_ERR_STATE, "surface upload failed: the mesh has been dropped, set it again");
    }
    m.has_surfaces = !w.empty();
    if (m.host) m.host->surf.swap(w);  // a chunk rebuild packs them again
    return RT_OK;
}

int read_bvh_impl(Ctx* c, uint32_t* nodes_out, uint32_t node_capacity, uint32_t* leaf_tris_out, uint32_t tri_capacity, uint32_t* n_nodes) {
    const DeviceMesh& m = c->pt.mesh();
    if (!m.n_tris) return c->fail(RT_ERR_STATE, "no mesh has been set");
    if (n_nodes) *n_nodes = m.n_nodes;
    if (nodes_out && node_capacity < m.n_nodes) return c->fail(RT_ERR_INVALID, "nodes_out holds %u of %u nodes", node_capacity, m.n_nodes);
    if (leaf_tris_out && tri_capacity < m.n_tris) return c->fail(RT_ERR_INVALID, "leaf_tris_out holds %u of %u triangles", tri_capacity, m.n_tris);
    if (!nodes_out && !leaf_tris_out) return RT_OK;
    if (int rc = rt::bind(c)) return rc;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (nodes_out) RT_HIP(c, hipMemcpy(nodes_out, m.nodes.get(), (size_t)m.n_nodes * 80, hipMemcpyDeviceToHost));
    // leaf order = the original index in every triangle record, whichever builder made the mesh
    if (leaf_tris_out)
        RT_HIP(c, hipMemcpy2D(leaf_tris_out, 4, reinterpret_cast<const char*>(m.tris.get()) + rt::kTriIdWord * 4, rt::kTriWords * 4, 4, m.n_tris,
                              hipMemcpyDeviceToHost));
    return RT_OK;
}

template <class F>
int guarded(Ctx* c, const char* what, F&& f, bool drop_mesh = true) {  // drop_mesh = false: the callee has put the mesh back before it threw
    // the builder allocates host vectors sized by n_tris and starts std::threads: nothing may leave an entry point
    // as a C++ exception (include/rt_abi.h: never throws or aborts across the boundary)
    try {
        return f();
    } catch (const std::bad_alloc&) {
        if (drop_mesh) pt_free_mesh(c->pt);
        return c->fail(RT_ERR_OOM, "%s: out of host memory", what);
    } catch (const std::system_error& e) {
        if (drop_mesh) pt_free_mesh(c->pt);
        return c->fail(RT_ERR_STATE, "%s: %s", what, e.what());
    } catch (const std::exception& e) {
        if (drop_mesh) pt_free_mesh(c->pt);
        return c->fail(RT_ERR_INVALID, "%s: %s", what, e.what());
    } catch (...) {
        if (drop_mesh) pt_free_mesh(c->pt);
        return c->fail(RT_ERR_INVALID, "%s failed", what);
    }
}
}  // namespace

namespace rt {
// `lane` renders with `owner`'s device mesh (read-only during rendering); the owner tells its lanes
// before it frees or replaces the mesh (frames_drop_mesh).
void pt_borrow_mesh(Ctx* lane, const Ctx* owner) {  // owner == nullptr: only forget what was borrowed
    pt_free_mesh(lane->pt);
    if (!owner || !owner->pt.own) return;
    lane->pt.borrowed = owner->pt.own.get();
    publish_mesh_stats(lane->pt);
}
}  // namespace rt

extern "C" {

int rt_set_mesh(rt_ctx* ctx, const float* verts, const float* albedo, const float* emission, uint32_t n_tris) {
    return rt_set_mesh_ex(ctx, verts, albedo, emission, n_tris, nullptr);
}

int rt_set_mesh_ex(rt_ctx* ctx, const float* verts, const float* albedo, const float* emission, uint32_t n_tris, const rt_mesh_options* options) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    return guarded(c, "mesh build", [&] { return set_mesh_impl(c, verts, albedo, emission, n_tris, options); });
}

int rt_mesh_chunk_info(rt_ctx* ctx, uint32_t chunk, uint32_t* count, uint32_t* tri_ids, uint32_t capacity) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    if (!c->pt.host()) return c->fail(RT_ERR_STATE, "not a two-level mesh");
    const rt::TwoLevelBvh& tl = c->pt.host()->tl;
    if (chunk >= tl.blas.size()) return c->fail(RT_ERR_INVALID, "chunk %u of %zu", chunk, tl.blas.size());
    const uint32_t first = tl.first[chunk], n = tl.first[chunk + 1] - first;
    if (count) *count = n;
    if (tri_ids) {
        if (capacity < n) return c->fail(RT_ERR_INVALID, "tri_ids holds %u of %u triangles", capacity, n);
        std::memcpy(tri_ids, &tl.sorted[first], (size_t)n * 4);
    }
    return RT_OK;
}

int rt_update_mesh_chunk(rt_ctx* ctx, uint32_t chunk, const float* verts, uint32_t n_tris) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    return guarded(c, "chunk rebuild", [&] { return update_chunk_impl(c, chunk, verts, n_tris); }, false);
}

int rt_set_mesh_device(rt_ctx* ctx, const void* verts_dev, const void* albedo_dev, const void* emission_dev, uint32_t n_tris) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    // the previous mesh is only replaced once the new one is complete: a failure leaves it in place
    return guarded(c, "device mesh build", [&] { return set_mesh_device_impl(c, verts_dev, albedo_dev, emission_dev, n_tris); }, false);
}

int rt_refit_mesh_device(rt_ctx* ctx, const void* verts_dev, uint32_t n_tris) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    // every refusal comes before the first write; a HIP failure after it drops the mesh itself (RT_ERR_STATE)
    return guarded(c, "mesh refit", [&] { return refit_mesh_device_impl(c, verts_dev, n_tris); }, false);
}

int rt_set_mesh_surfaces(rt_ctx* ctx, const uint32_t* kind, const float* ior, uint32_t n_tris) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    // every refusal comes before the first write; a HIP failure after it drops the mesh itself (RT_ERR_STATE)
    return guarded(c, "surfaces", [&] { return set_surfaces_impl(c, kind, ior, n_tris); }, false);
}

int rt_mesh_sharers(rt_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    return (int)resident_meshes().holders(c->pt.own);
}

int rt_read_bvh(rt_ctx* ctx, uint32_t* nodes_out, uint32_t node_capacity, uint32_t* leaf_tris_out, uint32_t tri_capacity, uint32_t* n_nodes) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return RT_ERR_INVALID;
    return read_bvh_impl(c, nodes_out, node_capacity, leaf_tris_out, tri_capacity, n_nodes);
}

}  // extern "C"
