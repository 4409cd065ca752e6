"""What the GPU tests of the query kinds on device arrays share: arrays on the device and their raw pointers, the two ways a bare
triangle array becomes a mesh, sentinel buffers, the pointers and parameter structs every entry must refuse, a stream that is busy
when the queries are enqueued, a path-traced frame with its ray counts, and bit-equality of float arrays.

Test helper (imported by the tests/test_gpu_*.py files and by tests/gpu_listing.py); not a conftest, no fixtures.  Nothing here
touches the GPU at import time: torch is imported inside the functions."""
import contextlib
import ctypes as C
import types

import numpy as np

f32 = np.float32
RT_ERR_INVALID, RT_ERR_STATE = -1, -4
SENTINEL = -7  # what every output buffer of a test holds before the call under test


def dev():
    import torch

    return torch.device("cuda", 0)


def tdev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def segment_end(p):
    """End address of the device allocation (caching-allocator segment) that holds `p`."""
    import torch

    for seg in torch.cuda.memory_snapshot():
        if seg["address"] <= p < seg["address"] + seg["total_size"]:
            return seg["address"] + seg["total_size"]
    raise AssertionError("pointer not in any segment")


def set_mesh_with_surface(renderer, verts, **kw):
    """The mesh of ray_exact._with_surface(verts)."""
    import ray_exact as X

    renderer.set_mesh(*X._with_surface(verts), **kw)


def set_mesh_px_surface(renderer, verts, **kw):
    """The mesh of verts under point_exact.surface(verts)."""
    import point_exact as PX

    renderer.set_mesh(verts, *PX.surface(verts), **kw)


def same_floats(a, b):
    """Bit-equal, NaN for NaN (whatever its payload)."""
    a, b = np.asarray(a, f32).ravel(), np.asarray(b, f32).ravel()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---- sentinels -------------------------------------------------------------------------------------------------------------------

def sentinel(n, dtype, guard=0, cols=None):
    """A device tensor of n + guard rows (of `cols` columns, if given) filled with -7."""
    import torch

    rows = n + guard
    return torch.full((rows,) if cols is None else (rows, cols), SENTINEL, dtype=dtype, device=dev())


def still_sentinel(buf, lo=0, hi=0):
    """Everything of `buf` (a tensor or an array) in front of row lo and from row hi on is still -7; with the defaults: all of it."""
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all())


def assert_untouched(renderer, outputs, big, what):
    """After a refused call: every output tensor is still -7 and the allocation behind the short pointers still zero."""
    renderer.synchronize()
    for k, x in enumerate(outputs):
        assert still_sentinel(x), (what, "output", k)
    assert bool((big == 0).all()), (what, "the allocation of the short pointers")


# ---- what every entry refuses ----------------------------------------------------------------------------------------------------

def bad_pointers(n, **short):
    """Pointers no entry may read or write n rows through: hp, into host memory, and for every name=row_bytes (or name=(row_bytes,
    rows) where the array has other than n rows) a device pointer one row short of the end of its allocation.  Returns a namespace
    of them, with `big`, the zeroed allocation the short ones point into, and `host`, which keeps hp alive."""
    import torch

    host = np.zeros((n + 1, 9), np.float64)
    big = torch.zeros(1 << 20, dtype=torch.float32, device=dev())
    end = segment_end(big.data_ptr())
    out = types.SimpleNamespace(host=host, hp=C.c_void_p(host.ctypes.data), big=big)
    for name, size in short.items():
        row_bytes, rows = size if isinstance(size, tuple) else (size, n)
        setattr(out, name, C.c_void_p(end - row_bytes * (rows - 1)))
    return out


def bad_params(P, flag="count_traversal"):
    """The four parameter structs of class P that every entry refuses: three tunings out of range and the kind's flag at 2."""
    return [C.byref(P(tune_refill_min=65)), C.byref(P(tune_blocks_per_cu=9)), C.byref(P(tune_lds_stack=79)), C.byref(P(**{flag: 2}))]


# ---- a busy stream, a frame --------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def busy_stream(renderer):
    """A new stream of torch's, handed to the renderer and made current, with work to do when the body enqueues its queries; on
    exit the stream is finished and its own work checked, and the renderer gets its own stream back whatever happened."""
    import torch

    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    renderer.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            busy = torch.zeros(1 << 26, dtype=torch.float32, device=dev())
            for _ in range(8):  # the stream has work to do when the queries are enqueued
                busy += 1.0
            yield s
        s.synchronize()
        assert float(busy[0]) == 8.0, ("the stream's own work", float(busy[0]))
    finally:
        renderer.synchronize()
        renderer.set_stream(None)


def pt_frame(renderer, **kw):
    """(rgb, (camera_rays, bounce_rays, shadow_rays, stack_overflow)) of one path-traced frame."""
    rgb = renderer.render_pt(**kw)
    st = renderer.pt_stats()
    return rgb, (st["camera_rays"], st["bounce_rays"], st["shadow_rays"], st["stack_overflow"])
