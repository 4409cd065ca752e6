"""Host-side mirror of the reference's Rust host logic for the hot path (src/main.rs), on top of
the C ABI.  Python is used only for tests/bench plumbing; the native stand-in for the Rust
`main` is host/rt_host.cpp.  Citations are file:line in the reference repository.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import (ClearanceQueryParams, ClearanceQueryStats, Config, HitQueryParams, HitQueryStats, KnnQueryParams, KnnQueryStats, Light, Material, MutableData, NeighborQueryParams, NeighborQueryStats, Object, OverlapQueryParams, OverlapQueryStats, OverlapSegmentStats, PointQueryParams, PointQueryStats, PtParams, PtStats, RayQueryParams, RayQueryStats, SweepQueryParams, SweepQueryStats,
                   RtError, SideQueryParams, SideQueryStats, Stats)

# src/main.rs:343-364
SPEED_MOVEMENT = 25.0
SPEED_ROTATION = 1.0
SPEED_MOUSE = 1.0
COMPUTE_IMAGE_COUNT = 9
RENDER_DIST = 1000.0
FOV = 1.0


def level_count(width):
    """src/main.rs:639  (view.x / 8.0).log2() as usize + 1, capped at COMPUTE_IMAGE_COUNT."""
    q = int(width) // 8
    return min((q.bit_length() - 1 if q >= 1 else 0) + 1, COMPUTE_IMAGE_COUNT)


def level_dims(width, height, count, level):
    """src/main.rs:209-213  ceil((1 << i) * res / (4 << count)) * 8."""
    den = 4 << count
    return (-((-(width << level)) // den)) * 8, (-((-(height << level)) // den)) * 8


def default_ratio(width, height):
    """src/main.rs:610  ratio = [FOV, FOV * h / w] in f32."""
    return np.array([FOV, np.float32(FOV) * np.float32(height) / np.float32(width)], np.float32)


def camera_quat(yaw, pitch):
    """Data::rotation, src/main.rs:402-404: Quat::from_rotation_z(-yaw) * Quat::from_rotation_x(pitch),
    glam 0.21.3 semantics, returned as to_array() = [x, y, z, w]."""
    hz, hx = np.float32(-yaw) * np.float32(0.5), np.float32(pitch) * np.float32(0.5)
    zs, zc, xs, xc = np.sin(hz), np.cos(hz), np.sin(hx), np.cos(hx)
    return np.array([zc * xs, zs * xs, zs * xc, zc * xc], np.float32)


def quat_mul_vec3(q, v):
    """glam Quat::mul_vec3 (used by Data::position, src/main.rs:409-411)."""
    q = np.asarray(q, np.float64)
    v = np.asarray(v, np.float64)
    b = q[:3]
    return (2.0 * np.dot(b, v) * b + (q[3] * q[3] - np.dot(b, b)) * v + 2.0 * q[3] * np.cross(b, v)).astype(np.float32)


class CameraController:
    """Data<W> camera state + the per-frame update of src/main.rs:732-775 (without the window)."""

    def __init__(self):
        self.rotation = np.zeros(2, np.float32)  # absolute yaw (x) / pitch (y), :383
        self.pos = np.zeros(3, np.float32)       # push_constants.pos, :626

    def rotate(self, d_yaw, d_pitch):
        self.rotation += np.array([d_yaw, d_pitch], np.float32)
        self.rotation[1] = np.clip(self.rotation[1], -0.5 * math.pi, 0.5 * math.pi)  # :770

    def move_local(self, right, forward, up):
        """Data::position (:406-414): displacement along the rotated RIGHT(+X)/FORWARD(+Y)/UP(+Z) axes."""
        q = self.quat()
        d = (right * quat_mul_vec3(q, (1, 0, 0)) + forward * quat_mul_vec3(q, (0, 1, 0)) + up * quat_mul_vec3(q, (0, 0, 1)))
        self.pos = (self.pos + d).astype(np.float32)  # :773

    def quat(self):
        return camera_quat(self.rotation[0], self.rotation[1])


def make_scene(spheres, materials, lights):
    """spheres: [(x,y,z,r)], materials: [(r,g,b,shine,ambient)] (material i belongs to sphere i,
    fragment.glsl:154), lights: [((x,y,z),(r,g,b))]."""
    s = MutableData()
    s.matCount, s.objCount, s.lightCount = len(materials), len(spheres), len(lights)
    for i, (x, y, z, r) in enumerate(spheres):
        s.objs[i].pos[:] = (x, y, z)
        s.objs[i].size = r
    for i, (r, g, b, shine, ambient) in enumerate(materials):
        s.mats[i].color[:] = (r, g, b)
        s.mats[i].diffuse = s.mats[i].specular = 1.0
        s.mats[i].shine, s.mats[i].ambient = shine, ambient
    for i, (p, c) in enumerate(lights):
        s.lights[i].pos[:] = p
        s.lights[i].color[:] = c
    return s


def default_scene():
    """The reference's start-up scene, src/main.rs:524-591."""
    return make_scene(
        [(5, 5, -1, 3), (5, 4, 10, 6), (-3, 3, -3, 1), (4, -1, 0, 2)],
        [(0.2, 0.2, 1.0, 1, 0.05), (0.1, 1.0, 0.1, 10, 0.05), (1.0, 1.0, 0.1, 1, 0.05), (1.0, 0.1, 0.1, 1, 0.05)],
        [((-1, 0, -3), (0.1, 0.5, 0.6)), ((8, -5, 10), (1.2, 0.2, 0.3))])


def cornell_scene():
    """BASELINE.json configs[0]/[1]: Cornell-box-style room made of the reference's only primitive
    (8 spheres = MAX_OBJECTS) + 1 soft-shadowed point light standing in for the area light
    (SURVEY.md §8d).  5 wall spheres of r=50 enclose x,z in [-6,6], back wall at y=22."""
    spheres = [(-56, 10, 0, 50), (56, 10, 0, 50), (0, 10, -56, 50), (0, 10, 56, 50), (0, 72, 0, 50),
               (-2.5, 14, -4, 2), (2.5, 11, -3, 3), (0, 8, -5, 1)]
    mats = [(0.75, 0.15, 0.15, 1, 0.05), (0.15, 0.75, 0.15, 1, 0.05), (0.75, 0.75, 0.75, 1, 0.05),
            (0.75, 0.75, 0.75, 1, 0.05), (0.75, 0.75, 0.75, 1, 0.05), (0.9, 0.9, 0.2, 10, 0.05),
            (0.2, 0.4, 0.9, 30, 0.05), (0.9, 0.5, 0.2, 4, 0.05)]
    lights = [((0, 10, 5), (1.0, 1.0, 1.0))]
    return make_scene(spheres, mats, lights)


def scene_bytes(scene):
    return bytes(scene)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Renderer:
    """One rt_ctx: one GPU, one stream, single-threaded (like the reference's one queue)."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        self.device = int(device)
        rc = self._lib.rt_create(C.byref(self._ctx), int(device))
        if rc != 0:
            raise RtError(rc, self._lib.rt_last_error(None).decode())
        self.width = self.height = 0
        self._chain_rows = 0

    def _check(self, rc):
        if rc != 0:
            raise RtError(rc, self._lib.rt_last_error(self._ctx).decode())

    def close(self):
        if self._ctx:
            self._lib.rt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def default_config(self):
        cfg = Config()
        self._lib.rt_default_config(C.byref(cfg))
        return cfg

    def set_config(self, cfg):
        self._check(self._lib.rt_set_config(self._ctx, C.byref(cfg)))
        self._chain_rows = int(cfg.reflections) + int(cfg.transmissions)

    def set_scene(self, scene):
        raw = bytes(scene) if not isinstance(scene, (bytes, bytearray)) else bytes(scene)
        buf = C.create_string_buffer(raw, len(raw))
        self._check(self._lib.rt_set_scene(self._ctx, C.cast(buf, C.c_void_p), len(raw)))

    def resize(self, width, height, ratio=None):
        r = None
        if ratio is not None:
            ratio = np.ascontiguousarray(ratio, np.float32)
            r = _fptr(ratio)
        self._check(self._lib.rt_resize(self._ctx, width, height, r))
        self.width, self.height = width, height

    def level_info(self):
        count = C.c_uint32()
        dims = ((C.c_uint32 * 2) * _lib.RT_MAX_LEVELS)()
        self._check(self._lib.rt_level_info(self._ctx, C.byref(count), C.byref(dims)))
        return [(int(dims[i][0]), int(dims[i][1])) for i in range(count.value)]

    def set_partition(self, rank, n_ranks):
        self._check(self._lib.rt_set_partition(self._ctx, rank, n_ranks))

    def tile_info(self):
        tx, ty, owned = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.rt_tile_info(self._ctx, C.byref(tx), C.byref(ty), C.byref(owned)))
        return int(tx.value), int(ty.value), int(owned.value)

    def set_stream(self, stream_ptr):
        self._check(self._lib.rt_set_stream(self._ctx, C.c_void_p(stream_ptr)))

    def render(self, rot=(0, 0, 0, 1), pos=(0, 0, 0), spp=1, want_depth=False):
        """Synchronous frame -> (H,W,3) f32 [, last pyramid level]."""
        rot = np.ascontiguousarray(rot, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        if spp == 1:
            depth = None
            if want_depth:
                w, h = self.level_info()[-1]
                depth = np.empty((h, w), np.float32)
            self._check(self._lib.rt_render(self._ctx, _fptr(rot), _fptr(pos), _fptr(rgb), _fptr(depth) if want_depth else None))
            return (rgb, depth) if want_depth else rgb
        self._check(self._lib.rt_render_spp(self._ctx, _fptr(rot), _fptr(pos), spp, _fptr(rgb)))
        return rgb

    def render_chains(self, rot=(0, 0, 0, 1), pos=(0, 0, 0)):
        """Test hook (rt_render_chains): render(rot, pos, want_depth=True) plus what every secondary march did ->
        (rgb, depth, chains); chains (H, W, reflections + transmissions, 7): eye[3], dir[3], len, NaN where no march ran."""
        rot = np.ascontiguousarray(rot, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        rows = self._chain_rows  # as of the last set_config (the default config has no chain: the call refuses)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        w, h = self.level_info()[-1]
        depth = np.empty((h, w), np.float32)
        chains = np.empty((self.height, self.width, rows, 7), np.float32)
        self._check(self._lib.rt_render_chains(self._ctx, _fptr(rot), _fptr(pos), _fptr(rgb), _fptr(depth), _fptr(chains)))
        return rgb, depth, chains

    def render_device(self, rot, pos, spp, dev_ptr, tile_major=False):
        """Asynchronous: enqueue a frame into a device buffer (e.g. torch tensor .data_ptr())."""
        rot = np.ascontiguousarray(rot, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        self._check(self._lib.rt_render_device(self._ctx, _fptr(rot), _fptr(pos), spp, C.c_void_p(dev_ptr), int(tile_major)))

    def detile_device(self, tiles_ptr, n_ranks, tiles_per_rank, rgb_ptr):
        self._check(self._lib.rt_detile_device(self._ctx, C.c_void_p(tiles_ptr), n_ranks, tiles_per_rank, C.c_void_p(rgb_ptr)))

    def synchronize(self):
        self._check(self._lib.rt_synchronize(self._ctx))

    # ---- native RCCL exchange (for hosts without torch.distributed) ---------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        rc = _lib.load().rt_comm_unique_id(buf)
        if rc != 0:
            raise RtError(rc, "rt_comm_unique_id failed (librccl.so not loadable?)")
        return bytes(buf)

    def comm_init(self, unique_id, rank, n_ranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.rt_comm_init(self._ctx, buf, rank, n_ranks))

    def gather_tiles(self, tiles_ptr, gathered_ptr, tiles_per_rank):
        self._check(self._lib.rt_gather_tiles(self._ctx, C.c_void_p(tiles_ptr), C.c_void_p(gathered_ptr), tiles_per_rank))

    def comm_destroy(self):
        self._check(self._lib.rt_comm_destroy(self._ctx))

    def read_level(self, level, image=None):
        """Test hook: pyramid level `level` of the last sample rendered, or, with `image`, (that level of image `image` of the
        last sample batch, the sample index it belongs to) (rt_read_level_image)."""
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._lib.rt_read_level(self._ctx, level, None, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value), np.float32)
        if image is None:
            self._check(self._lib.rt_read_level(self._ctx, level, _fptr(out), C.byref(w), C.byref(h)))
            return out
        sample = C.c_uint32()
        self._check(self._lib.rt_read_level_image(self._ctx, level, int(image), _fptr(out), C.byref(w), C.byref(h), C.byref(sample)))
        return out, int(sample.value)

    def read_rgba8(self):
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._lib.rt_read_rgba8(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- frames in flight (src/main.rs:664-667, 882-927: one fence per swapchain image) -----------
    FRAME_F32, FRAME_RGBA8 = 0, 1

    def frames_configure(self, n_slots=3, fmt=0):
        """n_slots swapchain-image-like slots; fmt FRAME_F32 (H,W,3 f32) or FRAME_RGBA8 (H,W,4 u8)."""
        self._check(self._lib.rt_frames_configure(self._ctx, int(n_slots), int(fmt)))
        self._frame_fmt = int(fmt)

    def frame_submit(self, slot, rot=(0, 0, 0, 1), pos=(0, 0, 0), spp=1, pt_params=None):
        """Enqueue a frame into `slot` (waits for the slot's previous frame first) and return at once;
        path A by default, path B when pt_params is given."""
        rot = np.ascontiguousarray(rot, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        if pt_params is None:
            self._check(self._lib.rt_frame_submit(self._ctx, int(slot), _fptr(rot), _fptr(pos), int(spp)))
        else:
            self._check(self._lib.rt_frame_submit_pt(self._ctx, int(slot), _fptr(rot), _fptr(pos), C.byref(pt_params)))

    def frame_wait(self, slot, copy=True):
        """Block until the slot's pixels are in host memory -> array (a view of the pinned frame when
        copy=False: valid until the slot is submitted again)."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(self._lib.rt_frame_wait(self._ctx, int(slot), C.byref(ptr), C.byref(nbytes)))
        if self._frame_fmt == self.FRAME_RGBA8:
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(self.height, self.width, 4))
        else:
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(self.height, self.width, 3))
        return a.copy() if copy else a

    def frame_ready(self, slot):
        r = C.c_int()
        self._check(self._lib.rt_frame_poll(self._ctx, int(slot), C.byref(r)))
        return bool(r.value)

    def selftest_math(self):
        """Mismatches of the kernels' shortened sqrt against IEEE sqrt over all 2^32 fp32 inputs (0)."""
        n = C.c_uint64()
        self._check(self._lib.rt_selftest_math(self._ctx, C.byref(n)))
        return int(n.value)

    def stats(self):
        s = Stats()
        self._check(self._lib.rt_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    # ---- path B: triangle mesh + BVH + wavefront path tracer (no reference counterpart) ----------
    def set_mesh(self, verts, albedo, emission, bvh_levels=1, blas_chunks=0):
        """Upload a triangle mesh and build its BVH (rt_set_mesh / rt_set_mesh_ex).  bvh_levels=2: a top level over
        blas_chunks (0 = 64) bottom-level chunks, flattened into the same node array; frames are identical."""
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
        albedo = np.ascontiguousarray(albedo, np.float32).reshape(-1, 3)
        emission = np.ascontiguousarray(emission, np.float32).reshape(-1, 3)
        if not (len(verts) == len(albedo) == len(emission)):
            raise ValueError("verts/albedo/emission disagree on the triangle count")
        opt = _lib.MeshOptions(bvh_levels, blas_chunks)
        self._check(self._lib.rt_set_mesh_ex(self._ctx, _fptr(verts), _fptr(albedo), _fptr(emission), len(verts), C.byref(opt)))

    def _on_device(self, t):
        """Does torch tensor `t` lie on this renderer's device?  What every tensor check below asks, and nothing else does."""
        return t.device.type == "cuda" and t.device.index == self.device

    def _device_rows(self, t, name, width):
        """Rows of `width` floats in torch tensor `t`, which must be float32, contiguous, on this renderer's device and of shape
        (n, width) or flat; ValueError otherwise."""
        import torch

        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if not self._on_device(t):
            raise ValueError(f"{name} must be on cuda:{self.device}, got {t.device}")
        if t.dim() == 2 and t.shape[1] == width:
            return t.shape[0]
        if t.dim() == 1 and t.numel() % width == 0:
            return t.numel() // width
        raise ValueError(f"{name} must have shape (n, {width}) or ({width} n,), got {tuple(t.shape)}")

    def set_mesh_device(self, verts, albedo, emission):
        """Mesh from torch tensors on this renderer's device; the BVH is built on the GPU (rt_set_mesh_device).  float32,
        contiguous, shapes (n, 9) / (n, 3) or flat.  Work torch has queued on its current stream is finished first."""
        import torch

        check = self._device_rows
        n = check(verts, "verts", 9)
        if check(albedo, "albedo", 3) != n or check(emission, "emission", 3) != n:
            raise ValueError("verts/albedo/emission disagree on the triangle count")
        if n == 0:
            raise ValueError("the mesh has no triangles")
        torch.cuda.current_stream(self.device).synchronize()  # writers on torch's stream are done before the build reads
        self._check(self._lib.rt_set_mesh_device(self._ctx, C.c_void_p(verts.data_ptr()), C.c_void_p(albedo.data_ptr()),
                                                 C.c_void_p(emission.data_ptr()), n))

    def refit_mesh_device(self, verts):
        """New vertex positions (torch tensor as set_mesh_device's verts, original triangle order) for the current single-level
        mesh: the tree keeps its topology and leaf order, its boxes are recomputed on the GPU (rt_refit_mesh_device).  Work
        torch has queued on its current stream is finished first."""
        import torch

        n = self._device_rows(verts, "verts", 9)
        torch.cuda.current_stream(self.device).synchronize()  # writers on torch's stream are done before the refit reads
        self._check(self._lib.rt_refit_mesh_device(self._ctx, C.c_void_p(verts.data_ptr()), n))

    SURFACE_LAMBERT, SURFACE_MIRROR, SURFACE_GLASS = 0, 1, 2

    def set_surfaces(self, kind, ior=None):
        """Surface of every triangle of the current mesh, original triangle order (rt_set_mesh_surfaces):
        kind[i] 0 = Lambert, 1 = mirror, 2 = glass of index ior[i] (1..4; ior is read only where kind is 2).  kind=None: all
        Lambert again.  1-D numpy arrays of one length; the library checks it against the mesh."""
        if kind is None:
            self._check(self._lib.rt_set_mesh_surfaces(self._ctx, None, None, self.pt_stats()["n_tris"]))
            return
        kind = np.asarray(kind)
        if kind.ndim != 1 or not (kind.dtype.kind in "iu" or kind.size == 0):
            raise ValueError(f"kind must be a 1-D integer array, got shape {kind.shape} dtype {kind.dtype}")
        if (kind < 0).any():
            raise ValueError("kind must not be negative")
        kind = np.ascontiguousarray(kind, np.uint32)
        iorp = None
        if ior is not None:
            ior = np.ascontiguousarray(ior, np.float32)
            if ior.shape != kind.shape:
                raise ValueError(f"ior must have the shape of kind {kind.shape}, got {ior.shape}")
            iorp = _fptr(ior)
        self._check(self._lib.rt_set_mesh_surfaces(self._ctx, kind.ctypes.data_as(C.POINTER(C.c_uint32)), iorp, len(kind)))

    def mesh_sharers(self):
        """Contexts that render this renderer's device mesh (rt_mesh_sharers): 0 = no mesh, 1 = only this one."""
        n = self._lib.rt_mesh_sharers(self._ctx)
        if n < 0:
            self._check(n)
        return n

    def read_bvh(self):
        """Test hook: (node words uint32 (n_nodes, 20), leaf order uint32 (n_tris,)) of the current mesh."""
        n_nodes = C.c_uint32()
        self._check(self._lib.rt_read_bvh(self._ctx, None, 0, None, 0, C.byref(n_nodes)))
        n_tris = self.pt_stats()["n_tris"]
        nodes = np.empty((n_nodes.value, 20), np.uint32)
        leaf = np.empty(n_tris, np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._check(self._lib.rt_read_bvh(self._ctx, nodes.ctypes.data_as(u32), n_nodes.value, leaf.ctypes.data_as(u32), n_tris,
                                          C.byref(n_nodes)))
        return nodes, leaf

    def mesh_chunk(self, chunk):
        """Original triangle indices of bottom-level chunk `chunk` of a two-level mesh, in rt_update_mesh_chunk's order."""
        n = C.c_uint32()
        self._check(self._lib.rt_mesh_chunk_info(self._ctx, chunk, C.byref(n), None, 0))
        ids = np.empty(n.value, np.uint32)
        self._check(self._lib.rt_mesh_chunk_info(self._ctx, chunk, None, ids.ctypes.data_as(C.POINTER(C.c_uint32)), n.value))
        return ids

    def update_mesh_chunk(self, chunk, verts):
        """New vertices (count x 9, mesh_chunk order) for one chunk of a two-level mesh: only that chunk is rebuilt."""
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
        self._check(self._lib.rt_update_mesh_chunk(self._ctx, chunk, _fptr(verts), len(verts)))  # the C side checks the count against the chunk

    def pt_params(self, spp=4, bounces=1, seed=1, sky=(0.0, 0.0, 0.0), ray_eps=1e-3, count_traversal=False, max_paths=0, tune_refill_min=0,
                  tune_blocks_per_cu=0, tune_lds_stack=0, tune_no_overlap=0, tune_no_packet=0, tune_sort_rays=0, tune_tri_mode=0):
        p = PtParams()
        self._lib.rt_default_pt_params(C.byref(p))
        p.spp, p.bounces, p.seed, p.ray_eps, p.count_traversal, p.max_paths = spp, bounces, seed, ray_eps, int(count_traversal), max_paths
        p.tune_refill_min, p.tune_blocks_per_cu, p.tune_lds_stack = tune_refill_min, tune_blocks_per_cu, tune_lds_stack
        p.tune_no_overlap = tune_no_overlap
        p.tune_no_packet = tune_no_packet
        p.tune_sort_rays = tune_sort_rays
        p.tune_tri_mode = tune_tri_mode
        p.sky[:] = [float(np.float32(x)) for x in sky]
        return p

    def render_pt(self, rot=(0, 0, 0, 1), pos=(0, 0, 0), params=None, **kw):
        """Synchronous path-traced frame -> (H,W,3) f32."""
        params = params or self.pt_params(**kw)
        rot = np.ascontiguousarray(rot, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        self._check(self._lib.rt_render_pt(self._ctx, _fptr(rot), _fptr(pos), C.byref(params), _fptr(rgb)))
        return rgb

    def render_pt_device(self, rot, pos, params, dev_ptr, tile_major=False):
        rot = np.ascontiguousarray(rot, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        self._check(self._lib.rt_render_pt_device(self._ctx, _fptr(rot), _fptr(pos), C.byref(params), C.c_void_p(dev_ptr), int(tile_major)))

    def pt_stats(self):
        s = PtStats()
        self._check(self._lib.rt_get_pt_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    RAY_MISS, RAY_INVALID = _lib.RAY_MISS, _lib.RAY_INVALID

    def _device_ints(self, t, name, n, kind):
        """`t` must be a contiguous torch tensor of the integer type `kind` on this renderer's device, of n elements in one dimension or,
        where n is a tuple, of that shape; ValueError otherwise."""
        import torch

        shape = n if isinstance(n, tuple) else (n,)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != getattr(torch, kind) or not t.is_contiguous() or not self._on_device(t) or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a contiguous {kind} tensor of shape {shape} on cuda:{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")

    def _device_i32(self, t, name, n):
        """_device_ints for int32."""
        self._device_ints(t, name, n, "int32")

    def _device_i32_rows(self, t, name, n, cols):
        """_device_ints for int32 of shape (n, cols)."""
        self._device_ints(t, name, (n, cols), "int32")

    def _device_i64(self, t, name, n):
        """_device_ints for int64."""
        self._device_ints(t, name, n, "int64")

    def _query_tune(self, params, tune, method):
        """The tune_* keywords of `method` (query_rays / query_points / query_sides / query_signed_distance / count_ray_hits / list_ray_hits / count_neighbors / list_neighbors / count_overlaps / list_overlaps / query_clearance / query_knn / query_sweeps) into its parameter struct;
        TypeError for any other keyword."""
        for k, v in tune.items():
            if k not in ("tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks"):
                raise TypeError(f"{method}() got an unexpected keyword argument {k!r}")
            setattr(params, k, int(v))

    def _query_out(self, t, name, n, dtype, dev, cols=1, exact=False):
        """The out tensor `name` of a query over n items: a new one (t is None), or t once it is what the query can fill.  A float32
        tensor of several columns may be flat unless `exact`; an integer one has the shape (n, cols), and `exact` says so of one column."""
        import torch

        shape = (n,) if cols == 1 and not exact else (n, cols)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if dtype == torch.int32 and len(shape) == 2:  # (no int64 output has columns)
            self._device_i32_rows(t, name, n, cols)
        elif dtype in (torch.int32, torch.int64):
            (self._device_i32 if dtype == torch.int32 else self._device_i64)(t, name, n)
        elif self._device_rows(t, name, cols) != n or ((cols == 1 or exact) and tuple(t.shape) != shape):
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}" if cols == 1 or exact else f"{name} must hold {n} rows of {cols}")
        return t

    @staticmethod
    def _out_tensors(out, k, message, room=None):
        """The k tensors of `out`, which must be a tuple or list of exactly k (ValueError(message) otherwise), padded with None to
        `room`; as many None where out is None."""
        if out is None:
            return (None,) * (room or k)
        if not isinstance(out, (tuple, list)) or len(out) != k:
            raise ValueError(message)
        return tuple(out) + (None,) * ((room or k) - k)

    def _query_call(self, sync, fn, *args):
        """The C call of a query between the two halves of `sync`: torch's current stream is finished before, ours after."""
        import torch

        if sync:
            torch.cuda.current_stream(self.device).synchronize()  # writers on torch's stream are done before the query reads
        self._check(fn(self._ctx, *(C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args)))
        if sync:
            self.synchronize()

    def _query_stats(self, stats, name):
        """The C struct `stats` filled by the library's `name` (waits for the kind's pending query), as a dict."""
        self._check(getattr(self._lib, name)(self._ctx, C.byref(stats)))
        return stats.as_dict()

    def _ray_rows(self, origins, dirs, tmax):
        """The ray count of a ray or all-hits query once its three inputs are what the library can read."""
        n = self._device_rows(origins, "origins", 3)
        if self._device_rows(dirs, "dirs", 3) != n:
            raise ValueError("origins and dirs disagree on the ray count")
        if tmax is not None and (self._device_rows(tmax, "tmax", 1) != n or tmax.dim() != 1):
            raise ValueError(f"tmax must have shape ({n},), got {tuple(tmax.shape)}")
        return n

    def _point_rows(self, points, rmax):
        """The point count of a query on points once points and the rmax tensor (or None) are what the library can read."""
        n = self._device_rows(points, "points", 3)
        if rmax is not None and (self._device_rows(rmax, "rmax", 1) != n or rmax.dim() != 1):
            raise ValueError(f"rmax must have shape ({n},), got {tuple(rmax.shape)}")
        return n

    def _point_out(self, out, first, n, dev, want_points):
        """The (dist, tri, point) tensors of query_points / query_signed_distance: new ones, or those of `out`.  first: dist's name."""
        import torch

        dist, tri, pt = self._out_tensors(out, 3 if want_points else 2, f"out must be ({first}, tri, point), or the pair ({first}, tri) with want_points=False", room=3)
        dist = self._query_out(dist, f"out {first}", n, torch.float32, dev)
        tri = self._query_out(tri, "out tri", n, torch.int32, dev)
        if want_points:
            pt = self._query_out(pt, "out point", n, torch.float32, dev, cols=3)
        return dist, tri, pt

    def query_rays(self, origins, dirs, tmax=None, any_hit=False, out=None, sync=True, attributes=False, **tune):
        """What do rays hit in the current mesh?  (rt_query_rays_device)  origins, dirs: float32 torch tensors on this
        renderer's device, contiguous, (n, 3) or flat; tmax: (n,) or None.  A triangle is hit when 0 < t < tmax (default: +inf for the
        closest hit, 0.999 for any hit).  any_hit=False: returns (t, tri) - float32 distances in units of |dir| (+inf on a miss) and int32
        original triangle indices (RAY_MISS = -1); any_hit=True: returns int32 flags (1 = something is hit).  Invalid rays (a non-finite
        component, an origin beyond 32 x the mesh's largest |coordinate|) get RAY_INVALID = -2 and t = NaN.  out: the tensors to fill -
        (t, tri) resp. the flag tensor - instead of new ones.  sync=True: work torch has queued on its current stream is finished first
        and the answers are complete on return; sync=False does neither: for callers that handed torch's stream to set_stream().
        attributes=True (rt_query_rays_attr_device, §6.18; closest hit only): returns (t, tri, uv, normal) - the same t and tri, the (n, 2)
        barycentrics (u, v) of the hit in its triangle (vertex weights (1 - u - v, u, v): interpolate()) and the (n, 3) unit geometric
        normal in the caller's winding; NaNs where tri < 0.  out must then be the 4-tuple.
        tune: tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of rt_ray_query_params."""
        import torch

        if attributes and any_hit:
            raise ValueError("attributes=True needs a closest-hit query: an occlusion has no winning triangle")
        n = self._ray_rows(origins, dirs, tmax)
        p = RayQueryParams()
        p.any_hit = int(bool(any_hit))
        self._query_tune(p, tune, "query_rays")
        uv = normal = None
        if any_hit:
            t, tri = None, out
        else:
            t, tri, uv, normal = self._out_tensors(out, 4 if attributes else 2, "out must be (t, tri, uv, normal) with attributes=True" if attributes else
                                                   "out must be the pair (t, tri) for a closest-hit query", room=4)
        tri = self._query_out(tri, "out tri", n, torch.int32, origins.device)
        if not any_hit:
            t = self._query_out(t, "out t", n, torch.float32, origins.device)
        if attributes:
            uv = self._query_out(uv, "out uv", n, torch.float32, origins.device, cols=2)
            normal = self._query_out(normal, "out normal", n, torch.float32, origins.device, cols=3)
            self._query_call(sync, self._lib.rt_query_rays_attr_device, origins, dirs, tmax, n, C.byref(p), t, tri, uv, normal)
            return t, tri, uv, normal
        self._query_call(sync, self._lib.rt_query_rays_device, origins, dirs, tmax, n, C.byref(p), t, tri)
        return tri if any_hit else (t, tri)

    def ray_query_stats(self):
        """rt_ray_query_stats of the last query as a dict (waits for it): rays, invalid_rays, stack_overflow, launches, ms."""
        return self._query_stats(RayQueryStats(), "rt_get_ray_query_stats")

    POINT_MISS, POINT_INVALID = _lib.POINT_MISS, _lib.POINT_INVALID

    def query_points(self, points, rmax=None, out=None, sync=True, want_points=True, count_traversal=False, attributes=False, **tune):
        """Which triangle of the current mesh is nearest to each point, how far is it, and where on it?  (rt_query_points_device,
        DESIGN.md §6.14.)  points: a float32 torch tensor on this renderer's device, contiguous, (n, 3) or flat; rmax: (n,) or None - only
        triangles nearer than rmax count (strictly; default +inf).  Returns (dist, tri, point): float32 distances (+inf on a miss), int32
        original triangle indices (POINT_MISS = -1) and the (n, 3) nearest points (NaN on a miss), or None in their place with
        want_points=False.  Invalid points (a non-finite component, a NaN rmax, a component beyond 32 x the mesh's largest |coordinate|)
        get POINT_INVALID = -2 and NaNs.  out: the tensors to fill - (dist, tri, point), or (dist, tri) with want_points=False - instead of
        new ones.  sync=True: work torch has queued on its current stream is finished first and the answers are complete on return;
        sync=False does neither: for callers that handed torch's stream to set_stream().  count_traversal=True: point_query_stats()
        reports nodes_visited / tris_tested.  attributes=True (rt_query_points_attr_device, §6.18): returns (dist, tri, point, uv, normal) -
        the same three, the (n, 2) barycentrics (u, v) of the nearest point in its triangle (vertex weights (1 - u - v, u, v):
        interpolate()) and the (n, 3) unit geometric normal in the caller's winding (zeros for a triangle without area); NaNs where
        tri < 0.  out then ends with (uv, normal).  tune: tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of
        rt_point_query_params."""
        import torch

        n = self._point_rows(points, rmax)
        p = PointQueryParams()
        p.count_traversal = int(bool(count_traversal))
        self._query_tune(p, tune, "query_points")
        if not attributes:
            dist, tri, pt = self._point_out(out, "dist", n, points.device, want_points)
            self._query_call(sync, self._lib.rt_query_points_device, points, rmax, n, C.byref(p), dist, tri, pt)
            return dist, tri, pt
        k = 3 if want_points else 2
        out = self._out_tensors(out, k + 2, "out must be (dist, tri, point, uv, normal) with attributes=True, or (dist, tri, uv, normal) with want_points=False")
        dist, tri, pt = self._point_out(out[:k], "dist", n, points.device, want_points)
        uv, normal = out[k:]
        uv = self._query_out(uv, "out uv", n, torch.float32, points.device, cols=2)
        normal = self._query_out(normal, "out normal", n, torch.float32, points.device, cols=3)
        self._query_call(sync, self._lib.rt_query_points_attr_device, points, rmax, n, C.byref(p), dist, tri, pt, uv, normal)
        return dist, tri, pt, uv, normal

    @staticmethod
    def interpolate(tri, uv, vertex_attr):
        """Per-vertex data at the hits of query_rays / query_points(attributes=True).  tri: (n,) integer triangle indices, uv: (n, 2),
        vertex_attr: (n_tris, 3, C) in the caller's original triangle order.  Returns (n, C): (1 - u - v) a0 + u a1 + v a2 of triangle
        tri's three rows; NaN where tri < 0.  Plain torch on whatever device the tensors are on (CPU tensors included)."""
        import torch

        if vertex_attr.dim() != 3 or vertex_attr.shape[1] != 3:
            raise ValueError(f"vertex_attr must have shape (n_tris, 3, C), got {tuple(vertex_attr.shape)}")
        if uv.dim() != 2 or uv.shape[1] != 2 or tri.dim() != 1 or tri.shape[0] != uv.shape[0]:
            raise ValueError(f"tri must have shape (n,) and uv (n, 2), got {tuple(tri.shape)} and {tuple(uv.shape)}")
        hit = tri >= 0
        a = vertex_attr[torch.where(hit, tri, torch.zeros_like(tri)).long()]  # (n, 3, C)
        u, v = uv[:, 0:1].to(a.dtype), uv[:, 1:2].to(a.dtype)
        val = (1 - u - v) * a[:, 0] + u * a[:, 1] + v * a[:, 2]
        return torch.where(hit[:, None], val, torch.full_like(val, float("nan")))

    def point_query_stats(self):
        """rt_point_query_stats of the last closest-point query as a dict (waits for it): points, invalid_points, nodes_visited,
        tris_tested (count_traversal=True only), stack_overflow, launches, ms."""
        return self._query_stats(PointQueryStats(), "rt_get_point_query_stats")

    def query_sides(self, points, out=None, sync=True, want_crossings=False, count_traversal=False, **tune):
        """On which side of the current mesh's surface does each point lie?  (rt_query_sides_device)  points: a float32
        torch tensor on this renderer's device, contiguous, (n, 3) or flat.  Returns int32 `inside` (1 inside, 0 outside): the majority of
        the parities of the triangles crossed by three fixed rays from the point - defined on every mesh as that parity of crossings,
        "inside" on closed meshes.  want_crossings=True: returns (inside, crossings) with the (n, 3) int32 crossing counts of the three
        rays (all three are then walked for every point; inside is the same).  Invalid points (a non-finite component, a component beyond
        32 x the mesh's largest |coordinate|) get POINT_INVALID = -2 and their crossings are not written.  out: the tensor(s) to fill -
        inside, or (inside, crossings) - instead of new ones.  sync as for query_points.  count_traversal=True: side_query_stats()
        reports nodes_visited / tris_tested.  tune: tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of
        rt_side_query_params."""
        import torch

        n = self._device_rows(points, "points", 3)
        p = SideQueryParams()
        p.count_traversal = int(bool(count_traversal))
        self._query_tune(p, tune, "query_sides")
        if want_crossings:
            inside, crossings = self._out_tensors(out, 2, "out must be the pair (inside, crossings) with want_crossings=True")
        else:
            if isinstance(out, (tuple, list)):
                raise ValueError("out must be the inside tensor, or (inside, crossings) with want_crossings=True")
            inside, crossings = out, None
        inside = self._query_out(inside, "out inside", n, torch.int32, points.device)
        if want_crossings:
            crossings = self._query_out(crossings, "out crossings", n, torch.int32, points.device, cols=3)
        self._query_call(sync, self._lib.rt_query_sides_device, points, n, C.byref(p), inside, crossings, None)
        return (inside, crossings) if want_crossings else inside

    def query_signed_distance(self, points, rmax=None, out=None, sync=True, want_points=True, **tune):
        """query_points followed by query_sides on its distances (rt_query_signed_distance_device): returns (sdist, tri,
        point) as query_points returns (dist, tri, point), with sdist negative where the point is inside.  With rmax a narrow-band
        signed distance: points beyond the band stay +inf / POINT_MISS and cost no ray walk.  out: (sdist, tri, point), or (sdist, tri)
        with want_points=False.  tune applies to both steps; point_query_stats() and side_query_stats() report them."""
        n = self._point_rows(points, rmax)
        pp, sp = PointQueryParams(), SideQueryParams()
        self._query_tune(pp, tune, "query_signed_distance")
        self._query_tune(sp, tune, "query_signed_distance")
        dist, tri, pt = self._point_out(out, "sdist", n, points.device, want_points)
        self._query_call(sync, self._lib.rt_query_signed_distance_device, points, rmax, n, C.byref(pp), C.byref(sp), dist, tri, pt, None)
        return dist, tri, pt

    def side_query_stats(self):
        """rt_side_query_stats of the last inside/outside query as a dict (waits for it): points, invalid_points, skipped_points, walks,
        third_walks, nodes_visited, tris_tested (count_traversal=True only), stack_overflow, launches, ms."""
        return self._query_stats(SideQueryStats(), "rt_get_side_query_stats")

    # A listing kind: the stem of the library's rt_{count,fill,list}_<stem>_device and of count_<stem> / list_<stem> here, its
    # parameter struct, the key's name, what it lists; the overlaps' "key" is the int32 edge mask, and it comes behind tri
    _RAY_HITS = ("ray_hits", HitQueryParams, "t", "hits")
    _NEIGHBORS = ("neighbors", NeighborQueryParams, "dist", "neighbours")
    _OVERLAPS = ("overlaps", OverlapQueryParams, "edges", "overlaps")

    def _count_listing(self, kind, src, n, dev, out, sync, count_traversal, tune):
        """count_ray_hits / count_neighbors / count_overlaps on the checked source arguments `src` of n items."""
        import torch

        stem, params = kind[:2]
        p = params()
        p.count_traversal = int(bool(count_traversal))
        self._query_tune(p, tune, f"count_{stem}")
        counts = self._query_out(out, "out counts", n, torch.int32, dev)
        self._query_call(sync, getattr(self._lib, f"rt_count_{stem}_device"), *src, n, C.byref(p), counts, None)
        return counts

    def _list_listing(self, kind, src, n, dev, capacity, out, sync, tune):
        """list_ray_hits / list_neighbors on the checked source arguments `src` of n items: (offsets, key, tri, counts); list_overlaps:
        (offsets, tri, edges, counts), the order of the library's arguments too."""
        import torch

        stem, params, key, what = kind
        tri_first = kind is self._OVERLAPS
        key_dtype = torch.int32 if tri_first else torch.float32
        order = (lambda k, t: (t, k)) if tri_first else (lambda k, t: (k, t))  # (key, tri) as the caller and the library have them
        p = params()
        self._query_tune(p, tune, f"list_{stem}")
        if capacity is None:
            if out is not None:
                raise ValueError(f"out needs a capacity: without one {key} and tri are allocated to the number of {what}")
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            if n == 0:
                offsets.zero_()
                return (offsets,) + order(torch.empty(0, dtype=key_dtype, device=dev), torch.empty(0, dtype=torch.int32, device=dev)) + (counts,)
            self._query_call(sync, getattr(self._lib, f"rt_count_{stem}_device"), *src, n, C.byref(p), counts, offsets)
            self.synchronize()  # the one host synchronisation: the total decides the allocation
            total = int(offsets[n].item())
            keys = torch.empty(total, dtype=key_dtype, device=dev)
            tri = torch.empty(total, dtype=torch.int32, device=dev)
            self._query_call(sync, getattr(self._lib, f"rt_fill_{stem}_device"), *src, n, C.byref(p), offsets, total, *order(keys if total else None, tri if total else None))
            return (offsets,) + order(keys, tri) + (counts,)
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity must be >= 0, got {capacity}")
        offsets, keys, tri, counts = self._out_tensors(out, 4, "out must be (offsets, tri, edges, counts)" if tri_first else f"out must be (offsets, {key}, tri, counts)")
        keys, tri = order(keys, tri)  # (its own inverse)
        offsets = self._query_out(offsets, "out offsets", n + 1, torch.int64, dev)
        keys = self._query_out(keys, f"out {key}", capacity, key_dtype, dev)
        tri = self._query_out(tri, "out tri", capacity, torch.int32, dev)
        counts = self._query_out(counts, "out counts", n, torch.int32, dev)
        if n == 0:
            offsets.zero_()
            return (offsets,) + order(keys, tri) + (counts,)
        self._query_call(sync, getattr(self._lib, f"rt_list_{stem}_device"), *src, n, C.byref(p), counts, offsets, capacity,
                         *order(keys if capacity else None, tri if capacity else None))
        return (offsets,) + order(keys, tri) + (counts,)

    def count_ray_hits(self, origins, dirs, tmax=None, out=None, sync=True, count_traversal=False, **tune):
        """How many triangles of the current mesh does each ray pass through?  (rt_count_ray_hits_device)  origins, dirs,
        tmax as for query_rays (tmax default: +inf).  Every triangle with 0 < t < tmax counts, not only the nearest.  Returns int32
        counts; invalid rays (query_rays' rule) get RAY_INVALID = -2.  out: the tensor to fill instead of a new one.  sync as for
        query_rays.  count_traversal=True: hit_query_stats() reports nodes_visited / tris_tested.  tune: tune_refill_min,
        tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of rt_hit_query_params."""
        n = self._ray_rows(origins, dirs, tmax)
        return self._count_listing(self._RAY_HITS, (origins, dirs, tmax), n, origins.device, out, sync, count_traversal, tune)

    def list_ray_hits(self, origins, dirs, tmax=None, capacity=None, out=None, sync=True, **tune):
        """Every triangle of the current mesh that each ray passes through.  (rt_list_ray_hits_device)  origins, dirs,
        tmax as for count_ray_hits.  Returns (offsets, t, tri, counts): int64 offsets (n + 1; [n] = the number of hits of all rays), and
        the hits of ray i in t[offsets[i]:offsets[i + 1]] (float32, units of |dir|) and tri[...] (int32 original triangle indices),
        ascending by (t, tri); int32 counts as count_ray_hits returns them (invalid rays: RAY_INVALID, no hits).
        capacity=k: one stream-ordered call, no host synchronisation beyond `sync`; t and tri hold k entries.  A ray whose slice ends
        beyond k (offsets[i + 1] > k) has written nothing, every other ray's slice is complete; offsets are always the full sums, so
        offsets[n] > k says: grow and call again.  capacity=None: the count step, ONE host synchronisation to read offsets[n], t and
        tri allocated to exactly that, then the fill step (rt_count_ray_hits_device + rt_fill_ray_hits_device: two walks).
        out: (offsets, t, tri, counts) to fill instead of new tensors, with a capacity only (t and tri of that many elements).
        tune: tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of rt_hit_query_params; hit_query_stats() reports."""
        n = self._ray_rows(origins, dirs, tmax)
        return self._list_listing(self._RAY_HITS, (origins, dirs, tmax), n, origins.device, capacity, out, sync, tune)

    def hit_query_stats(self):
        """rt_hit_query_stats of the last all-hits call as a dict (waits for it): rays, invalid_rays, hits, hits_written, incomplete_rays,
        slice_overflow, nodes_visited, tris_tested (count_traversal=True only), stack_overflow, launches, ms."""
        return self._query_stats(HitQueryStats(), "rt_get_hit_query_stats")

    def _neighbor_points(self, points, rmax):
        """(n, rmax tensor or None, rmax_all) of a neighbour query once its inputs are what the library can read."""
        import torch

        if isinstance(rmax, torch.Tensor):
            return self._point_rows(points, rmax), rmax, 0.0
        n = self._point_rows(points, None)
        if isinstance(rmax, bool) or not isinstance(rmax, (int, float, np.floating, np.integer)):
            raise ValueError(f"rmax must be a float or a float32 tensor of shape ({n},), got {type(rmax).__name__}")
        return n, None, float(rmax)

    def count_neighbors(self, points, rmax, out=None, sync=True, count_traversal=False, **tune):
        """How many triangles of the current mesh lie within rmax of each point?  (rt_count_neighbors_device)  points as
        for query_points; rmax: a float for all points, or a float32 device tensor of n elements.  Every triangle with d2 < rmax * rmax
        counts (strictly; d2 and the product in fp32, as query_points has them), not only the nearest.  Returns int32 counts; invalid
        points (query_points' rule) get POINT_INVALID = -2.  out: the tensor to fill instead of a new one.  sync as for query_points.
        count_traversal=True: neighbor_query_stats() reports nodes_visited / tris_tested.  tune: tune_refill_min, tune_blocks_per_cu,
        tune_lds_stack, tune_max_blocks of rt_neighbor_query_params."""
        n, rmax_t, rmax_all = self._neighbor_points(points, rmax)
        return self._count_listing(self._NEIGHBORS, (points, rmax_t, rmax_all), n, points.device, out, sync, count_traversal, tune)

    def list_neighbors(self, points, rmax, capacity=None, out=None, sync=True, **tune):
        """Every triangle of the current mesh within rmax of each point.  (rt_list_neighbors_device)  points, rmax as for
        count_neighbors.  Returns (offsets, dist, tri, counts): int64 offsets (n + 1; [n] = the number of neighbours of all points), and
        the neighbours of point i in dist[offsets[i]:offsets[i + 1]] (float32, non-decreasing) and tri[...] (int32 original triangle
        indices), ascending by (d2, tri); entry 0 is query_points' answer.  int32 counts as count_neighbors returns them (invalid points:
        POINT_INVALID, no entries).
        capacity=k: one stream-ordered call, no host synchronisation beyond `sync`; dist and tri hold k entries.  A point whose slice
        ends beyond k (offsets[i + 1] > k) has written nothing, every other point's slice is complete; offsets are always the full sums,
        so offsets[n] > k says: grow and call again.  capacity=None: the count step, ONE host synchronisation to read offsets[n], dist
        and tri allocated to exactly that, then the fill step (rt_count_neighbors_device + rt_fill_neighbors_device: two walks).
        out: (offsets, dist, tri, counts) to fill instead of new tensors, with a capacity only (dist and tri of that many elements).
        tune: tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of rt_neighbor_query_params; neighbor_query_stats()
        reports."""
        n, rmax_t, rmax_all = self._neighbor_points(points, rmax)
        return self._list_listing(self._NEIGHBORS, (points, rmax_t, rmax_all), n, points.device, capacity, out, sync, tune)

    def neighbor_query_stats(self):
        """rt_neighbor_query_stats of the last neighbour call as a dict (waits for it): points, invalid_points, neighbors,
        neighbors_written, incomplete_points, slice_overflow, nodes_visited, tris_tested (count_traversal=True only), stack_overflow,
        launches, ms."""
        return self._query_stats(NeighborQueryStats(), "rt_get_neighbor_query_stats")

    def count_overlaps(self, tris, out=None, sync=True, count_traversal=False, **tune):
        """How many triangles of the current mesh does each query triangle intersect?  (rt_count_overlaps_device)
        tris: a float32 torch tensor on this renderer's device, contiguous, (n, 9), (n, 3, 3) or flat: the three vertices of each
        query triangle.  A mesh triangle counts when its box meets the query triangle's and an edge of one pierces the other (fp32,
        csrc/tri_overlap.h; coplanar pairs never count, the test is not watertight).  Returns int32 counts; invalid triangles (a
        non-finite coordinate, one beyond 32 x the mesh's largest |coordinate|) get RAY_INVALID = -2.  out: the tensor to fill instead
        of a new one.  sync as for query_rays.  count_traversal=True: overlap_query_stats() reports nodes_visited / tris_tested.  tune:
        tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of rt_overlap_query_params."""
        flat, n = self._tri_rows(tris)
        return self._count_listing(self._OVERLAPS, (flat,), n, tris.device, out, sync, count_traversal, tune)

    def list_overlaps(self, tris, capacity=None, out=None, sync=True, **tune):
        """Every triangle of the current mesh that each query triangle intersects.  (rt_list_overlaps_device)  tris as
        for count_overlaps.  Returns (offsets, tri, edges, counts): int64 offsets (n + 1; [n] = the number of overlaps of all query
        triangles), and the overlaps of query triangle i in tri[offsets[i]:offsets[i + 1]] (int32 original triangle indices, ascending)
        and edges[...] (int32 masks: bits 0-2 = the query triangle's edges A0A1, A1A2, A2A0 that pierce the mesh triangle, bits 3-5 =
        the mesh triangle's edges v0v1, v1v2, v0v2 that pierce the query triangle); int32 counts as count_overlaps returns them.
        capacity, out (then (offsets, tri, edges, counts)), sync and tune as for list_neighbors; overlap_query_stats() reports."""
        flat, n = self._tri_rows(tris)
        return self._list_listing(self._OVERLAPS, (flat,), n, tris.device, capacity, out, sync, tune)

    def _tri_rows(self, tris):
        """(the tensor the library reads, n) of the query triangles `tris`: (n, 9), (n, 3, 3) or flat."""
        import torch

        if isinstance(tris, torch.Tensor) and tris.dim() == 3 and tuple(tris.shape[1:]) == (3, 3) and tris.is_contiguous():
            tris = tris.view(-1, 9)
        return tris, self._device_rows(tris, "tris", 9)

    def overlap_query_stats(self):
        """rt_overlap_query_stats of the last overlap call as a dict (waits for it): triangles, invalid_triangles, overlaps,
        overlaps_written, incomplete_triangles, slice_overflow, nodes_visited, tris_tested (count_traversal=True only; records fetched),
        stack_overflow, launches, ms."""
        return self._query_stats(OverlapQueryStats(), "rt_get_overlap_query_stats")

    def overlap_segments(self, tris, offsets, tri, capacity=None, out=None, sync=True, want_ends=False):
        """Where does each listed pair intersect?  (rt_overlap_segments_device)  tris as for list_overlaps; offsets
        (int64, n + 1) and tri (int32) are the tensors list_overlaps returned for them on the current mesh.  Returns seg, a float32
        tensor of shape (capacity, 2, 3): entry k holds the two endpoints of the segment in which query triangle i (offsets[i] <= k <
        offsets[i + 1]) and mesh triangle tri[k] intersect, computed on the device from the resident records in the arithmetic that
        produced the edge mask (csrc/tri_section.h).  An entry with one bit in its mask is a touch: the same point twice.
        want_ends=True: returns (seg, ends); ends[k] (int32) = b | (c << 3), the mask bits of the edges the first and the second
        endpoint lie on (c = b for a touch).  capacity=None means len(tri); tri must hold at least capacity elements.  Entries
        from min(offsets[n], capacity) on, and those of a slice that ends beyond the capacity, are left as they are; an entry that
        is not the library's (no owner, an index outside the mesh, no bit set) gets NaNs and ends = -1.  out: the tensor seg - or
        (seg, ends) with want_ends - to fill instead of new ones.  sync as for query_rays; overlap_segment_stats() reports."""
        import torch

        flat, n = self._tri_rows(tris)
        self._device_i64(offsets, "offsets", n + 1)
        if not isinstance(tri, torch.Tensor) or tri.dim() != 1:
            raise ValueError(f"tri must be a torch tensor of one dimension, got {type(tri).__name__}")
        capacity = tri.numel() if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity must be >= 0, got {capacity}")
        if tri.numel() < capacity:
            raise ValueError(f"tri must hold at least capacity = {capacity} elements, got {tri.numel()}")
        self._device_i32(tri, "tri", tri.numel())
        if out is not None and want_ends and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError("out must be (seg, ends) with want_ends=True")
        seg, ends = (out if want_ends else (out, None)) if out is not None else (None, None)
        if isinstance(seg, torch.Tensor) and seg.dim() == 3 and tuple(seg.shape[1:]) == (2, 3) and seg.is_contiguous():
            seg = seg.view(-1, 6)
        seg = self._query_out(seg, "out seg", capacity, torch.float32, tris.device, cols=6)
        if want_ends:
            ends = self._query_out(ends, "out ends", capacity, torch.int32, tris.device)
        if n and capacity:
            self._query_call(sync, self._lib.rt_overlap_segments_device, flat, n, offsets, capacity, tri, seg, ends)
        seg = seg.view(capacity, 2, 3)
        return (seg, ends) if want_ends else seg

    def overlap_segment_stats(self):
        """rt_overlap_segment_stats of the last overlap_segments call as a dict (waits for it): entries, segments, touches,
        skipped_incomplete, bad_entries, launches, ms."""
        return self._query_stats(OverlapSegmentStats(), "rt_get_overlap_segment_stats")

    def query_clearance(self, tris, rmax=None, out=None, sync=True, want_points=True, count_traversal=False, **tune):
        """How far is each query triangle from the current mesh, which mesh triangle is nearest, and where are the two nearest points?
        (rt_query_clearance_device)  tris as for count_overlaps: a float32 torch tensor on this renderer's device,
        contiguous, (n, 9), (n, 3, 3) or flat; rmax: (n,) or None - only mesh triangles nearer than rmax count (strictly; default +inf).
        Returns (dist, tri, point_query, point_mesh): float32 distances (+inf on a miss; 0 or a rounding of it where the triangles
        intersect), int32 original triangle indices (POINT_MISS = -1), and the (n, 3) nearest points on the query triangle and on mesh
        triangle tri (NaN on a miss), or None in their place with want_points=False.  Invalid triangles (a non-finite coordinate, a
        NaN rmax, a coordinate beyond 32 x the mesh's largest |coordinate|) get RAY_INVALID = -2 and NaNs.  out: the tensors to fill -
        (dist, tri, point_query, point_mesh), or (dist, tri) with want_points=False - instead of new ones.  sync as for query_rays.
        count_traversal=True: clearance_query_stats() reports nodes_visited / tris_tested.  tune: tune_refill_min, tune_blocks_per_cu,
        tune_lds_stack, tune_max_blocks of rt_clearance_query_params."""
        import torch

        flat, n = self._tri_rows(tris)
        if rmax is not None and (self._device_rows(rmax, "rmax", 1) != n or rmax.dim() != 1):
            raise ValueError(f"rmax must have shape ({n},), got {tuple(rmax.shape)}")
        p = ClearanceQueryParams()
        p.count_traversal = int(bool(count_traversal))
        self._query_tune(p, tune, "query_clearance")
        dist, tri, pq, pm = self._out_tensors(out, 4 if want_points else 2, "out must be (dist, tri, point_query, point_mesh), or the pair (dist, tri) with want_points=False",
                                              room=4)
        dist = self._query_out(dist, "out dist", n, torch.float32, tris.device)
        tri = self._query_out(tri, "out tri", n, torch.int32, tris.device)
        if want_points:
            pq = self._query_out(pq, "out point_query", n, torch.float32, tris.device, cols=3)
            pm = self._query_out(pm, "out point_mesh", n, torch.float32, tris.device, cols=3)
        self._query_call(sync, self._lib.rt_query_clearance_device, flat, rmax, n, C.byref(p), tri, dist, pq, pm)
        return dist, tri, pq, pm

    def clearance_query_stats(self):
        """rt_clearance_query_stats of the last clearance query as a dict (waits for it): queries, invalid_triangles, nodes_visited,
        tris_tested (count_traversal=True only; records fetched), stack_overflow, ms."""
        return self._query_stats(ClearanceQueryStats(), "rt_get_clearance_query_stats")

    KNN_MAX_K = _lib.KNN_MAX_K

    def query_knn(self, points, k, rmax=None, out=None, sync=True, count_traversal=False, **tune):
        """The k triangles of the current mesh nearest to each point, sorted.  (rt_query_knn_device)  points as for
        query_points; k: 1 .. KNN_MAX_K = 1024 (it may exceed the number of triangles: rows are then short); rmax: None (+inf), a float
        for all points - it becomes a filled device tensor - or a float32 device tensor of n elements: only triangles nearer than rmax
        count (strictly).  Returns (dist, tri, counts): (n, k) float32 distances and (n, k) int32 original triangle indices, row i
        ascending by (d2, tri) - the first min(k, its length) entries of list_neighbors' slice for the same rmax, entry 0 query_points'
        answer - and (n,) int32 counts, the entries that are neighbours; those behind them are +inf and POINT_MISS = -1.  Invalid points
        (query_points' rule) get counts POINT_INVALID = -2 and a row of NaN and POINT_INVALID.  out: (dist, tri, counts) to fill instead
        of new tensors.  sync as for query_points.  count_traversal=True: knn_query_stats() reports nodes_visited / tris_tested.  tune:
        tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of rt_knn_query_params."""
        import torch

        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"k must be an integer, got {type(k).__name__}")
        k = int(k)
        if not 1 <= k <= self.KNN_MAX_K:
            raise ValueError(f"k must be 1 .. {self.KNN_MAX_K}, got {k}")
        if rmax is None or isinstance(rmax, torch.Tensor):
            n = self._point_rows(points, rmax)
        else:
            n = self._point_rows(points, None)
            if isinstance(rmax, bool) or not isinstance(rmax, (int, float, np.floating, np.integer)):
                raise ValueError(f"rmax must be None, a float or a float32 tensor of shape ({n},), got {type(rmax).__name__}")
            rmax = torch.full((n,), float(rmax), dtype=torch.float32, device=points.device)
        p = KnnQueryParams()
        p.count_traversal = int(bool(count_traversal))
        self._query_tune(p, tune, "query_knn")
        dist, tri, counts = self._out_tensors(out, 3, "out must be (dist, tri, counts)")
        dist = self._query_out(dist, "out dist", n, torch.float32, points.device, cols=k, exact=True)
        tri = self._query_out(tri, "out tri", n, torch.int32, points.device, cols=k, exact=True)
        counts = self._query_out(counts, "out counts", n, torch.int32, points.device)
        self._query_call(sync, self._lib.rt_query_knn_device, points, rmax, n, k, C.byref(p), dist, tri, counts)
        return dist, tri, counts

    def knn_query_stats(self):
        """rt_knn_query_stats of the last k-nearest query as a dict (waits for it): points, invalid_points, neighbors (the sum of the
        counts that are not negative), nodes_visited, tris_tested (count_traversal=True only), stack_overflow, launches, ms."""
        return self._query_stats(KnnQueryStats(), "rt_get_knn_query_stats")

    def query_sweeps(self, origins, dirs, radius, tmax=None, out=None, sync=True, want_points=True, count_traversal=False, **tune):
        """How far does a sphere get before it touches the current mesh, which triangle does it touch first, and where?
        (rt_query_sweeps_device)  origins, dirs, tmax as for query_rays: the centre starts at origins[i] and moves
        along dirs[i] (not normalised; t is in units of |dir|), only contacts with t < tmax count (strictly; default +inf).  radius: a
        float32 device tensor of n elements, or a float for all items - it becomes a filled device tensor; 0 is a ray against the closed
        triangles.  Returns (t, tri, point): float32 times of impact (+inf on a miss; 0 where the sphere touches at the start, the
        lowest triangle index among those it touches), int32 original triangle indices (RAY_MISS = -1) and the (n, 3) contact points on
        triangle tri (NaN on a miss), or None in its place with want_points=False; the contact normal is (origin + t dir - point) /
        radius.  Invalid items (a non-finite component, a NaN tmax, a radius that is NaN, negative or above 32 x the mesh's largest
        |coordinate|, an origin beyond that reach) get RAY_INVALID = -2 and NaNs.  out: the tensors to fill - (t, tri, point), or (t, tri)
        with want_points=False - instead of new ones.  sync as for query_rays.  count_traversal=True: sweep_query_stats() reports
        nodes_visited / tris_tested.  tune: tune_refill_min, tune_blocks_per_cu, tune_lds_stack, tune_max_blocks of
        rt_sweep_query_params."""
        import torch

        n = self._ray_rows(origins, dirs, tmax)
        if isinstance(radius, torch.Tensor):
            if self._device_rows(radius, "radius", 1) != n or radius.dim() != 1:
                raise ValueError(f"radius must have shape ({n},), got {tuple(radius.shape)}")
        else:
            if isinstance(radius, bool) or not isinstance(radius, (int, float, np.floating, np.integer)):
                raise ValueError(f"radius must be a float or a float32 tensor of shape ({n},), got {type(radius).__name__}")
            if not float(radius) >= 0.0 or float(radius) == float("inf"):
                raise ValueError(f"radius must be finite and not negative, got {float(radius)}")
            radius = torch.full((n,), float(radius), dtype=torch.float32, device=origins.device)
        p = SweepQueryParams()
        p.count_traversal = int(bool(count_traversal))
        self._query_tune(p, tune, "query_sweeps")
        t, tri, pt = self._point_out(out, "t", n, origins.device, want_points)
        self._query_call(sync, self._lib.rt_query_sweeps_device, origins, dirs, radius, tmax, n, C.byref(p), t, tri, pt)
        return t, tri, pt

    def sweep_query_stats(self):
        """rt_sweep_query_stats of the last sphere-cast query as a dict (waits for it): sweeps, invalid_sweeps, hits, nodes_visited,
        tris_tested (count_traversal=True only), stack_overflow, launches, ms."""
        return self._query_stats(SweepQueryStats(), "rt_get_sweep_query_stats")

    def trace_rays(self, origins, dirs, any_hit=False, counted=False):
        """Test hook (query_rays is the product entry): closest hit (t, original triangle index) or occlusion flags for a ray batch;
        counted=True also returns an (n, 2) array of BVH nodes fetched / triangles tested per ray."""
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(origins)
        t = np.empty(n, np.float32)
        tri = np.empty(n, np.int32)
        counts = np.zeros((n, 2), np.uint32) if counted else None
        self._check(self._lib.rt_trace_rays_counted(self._ctx, _fptr(origins), _fptr(dirs), n, int(any_hit), _fptr(t),
                                                    tri.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    counts.ctypes.data_as(C.POINTER(C.c_uint32)) if counted else None))
        return (t, tri, counts) if counted else (t, tri)


def tile_owner(tile_index, n_ranks):
    """Framebuffer partition rule of the C ABI: tile t (row-major 64x64 tiles) -> rank t % n_ranks."""
    return tile_index % n_ranks


def tiles_to_frame(tiles, n_ranks, tiles_per_rank, width, height):
    """numpy model of rt_detile_device: (n_ranks*tiles_per_rank, 64, 64, 3) rank-major -> (H,W,3)."""
    T = _lib.RT_TILE
    tx, ty = -(-width // T), -(-height // T)
    out = np.zeros((ty * T, tx * T, 3), tiles.dtype)
    for t in range(tx * ty):
        r, k = t % n_ranks, t // n_ranks
        y, x = divmod(t, tx)
        out[y * T:(y + 1) * T, x * T:(x + 1) * T] = tiles[r * tiles_per_rank + k]
    return out[:height, :width]


def frame_to_tiles(frame, rank, n_ranks, tiles_per_rank):
    """numpy model of the tile-major output of rt_render*_device(tile_major=1): the tiles owned by
    `rank` (tile t -> rank t % n_ranks), zero-padded to tiles_per_rank x 64 x 64 x 3."""
    T = _lib.RT_TILE
    h, w = frame.shape[:2]
    tx, ty = -(-w // T), -(-h // T)
    out = np.zeros((tiles_per_rank, T, T, 3), frame.dtype)
    for k, t in enumerate(range(rank, tx * ty, n_ranks)):
        y, x = divmod(t, tx)
        blk = frame[y * T:(y + 1) * T, x * T:(x + 1) * T]
        out[k, :blk.shape[0], :blk.shape[1]] = blk
    return out


def gather_tiles(mine, gathered, rank, dist):
    """The one exchange step of a multi-GPU frame: every rank's tile-major buffer goes
    to rank 0 (torch.distributed gather; backend nccl = RCCL over xGMI on GPUs, gloo in the CPU tests).
    `gathered` is a (world, tiles_per_rank, 64, 64, 3) tensor on rank 0, None elsewhere."""
    dist.gather(mine, list(gathered.unbind(0)) if rank == 0 else None, dst=0)


def owned_tiles(total_tiles, rank, n_ranks):
    """Tiles of a frame of `total_tiles` that belong to `rank` (tile t -> rank t % n_ranks); rt_tile_info's `owned`."""
    return (total_tiles - rank + n_ranks - 1) // n_ranks if total_tiles > rank else 0


def gather_owned_tiles(mine, gathered, rank, world, total_tiles, dist):
    """The exchange as rt_gather_tiles (csrc/rt_abi_comm.hip) does it, with torch.distributed point-to-point
    calls: every rank sends exactly the tiles it owns, the root receives each peer's own count into that
    peer's block of `gathered` and copies its own; pad tiles of an uneven split are neither read nor written."""
    if rank == 0:
        k0 = owned_tiles(total_tiles, 0, world)
        gathered[0, :k0] = mine[:k0]
        for peer in range(1, world):
            k = owned_tiles(total_tiles, peer, world)
            if k:
                dist.recv(gathered[peer, :k], src=peer)
    else:
        k = owned_tiles(total_tiles, rank, world)
        if k:
            dist.send(mine[:k].contiguous(), dst=0)
