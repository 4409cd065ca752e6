"""CPU tests of what the tests share: tests/abi_boundary.py's layout check fails on a wrong mirror, a wrong member list and a wrong
constant; tests/native_ref.py's unpack consumes its stream exactly and its run refuses a program that fails or does not say OK;
abi_boundary.cpu_renderer() refuses what Renderer's own tensor checks refuse apart from the device; and of tests/gpu_listing.py what
is pure: expected_fill on a case computed by hand, and the three Listing descriptions against the product's names."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import abi_boundary as AB
import gpu_listing as L
import native_ref as NR
import raytracing_engine_amd as R
from raytracing_engine_amd import _lib

KNN = AB.Kind(functions=(), params="KnnQueryParams", stats="KnnQueryStats", params_c="rt_knn_query_params", stats_c="rt_knn_query_stats",
              params_fields=["tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks", "count_traversal"],
              stats_fields=["points", "invalid_points", "neighbors", "nodes_visited", "tris_tested", "stack_overflow", "launches", "ms"],
              constants={"RT_KNN_MAX_K": 1024})


def test_struct_layout_rejects_a_wrong_mirror_a_wrong_list_and_a_wrong_constant(tmp_path):
    import dataclasses

    AB.struct_layout(KNN, tmp_path)  # the description itself is right
    fields = list(R.KnnQueryStats._fields_)
    i, j = [n for n, _ in fields].index("neighbors"), [n for n, _ in fields].index("ms")  # a uint64 and the double: the same sizes, other offsets' names
    fields[i], fields[j] = fields[j], fields[i]
    swapped = type("Swapped", (C.Structure,), {"_fields_": fields})
    assert C.sizeof(swapped) == C.sizeof(R.KnnQueryStats)
    with pytest.raises(AssertionError):  # the members all exist and the size is right: only the offsets tell
        AB.struct_layout(KNN, tmp_path, [(swapped, "rt_knn_query_stats", [n for n, _ in fields])])
    with pytest.raises(AssertionError):  # the mirror is right, the expected list has two names swapped
        AB.struct_layout(dataclasses.replace(KNN, stats_fields=[n for n, _ in fields]), tmp_path)
    with pytest.raises(AssertionError):
        AB.struct_layout(dataclasses.replace(KNN, stats_fields=KNN.stats_fields[:-1]), tmp_path)
    with pytest.raises(AssertionError):
        AB.struct_layout(dataclasses.replace(KNN, stats_fields=frozenset(KNN.stats_fields[:-1])), tmp_path)
    with pytest.raises(AssertionError):
        AB.struct_layout(dataclasses.replace(KNN, constants={"RT_KNN_MAX_K": 1023}), tmp_path)


def test_unpack_consumes_the_stream_exactly():
    raw = np.array([3, 2], np.uint64).tobytes() + np.arange(3, dtype=np.int32).tobytes() + np.arange(2, dtype=np.float32).tobytes()
    fields = lambda h: (("a", np.int32, h[0]), ("b", np.float32, h[1]))  # noqa: E731
    head, out = NR.unpack(raw, 2, fields)
    assert head == (3, 2) and out["a"].tolist() == [0, 1, 2] and out["b"].tolist() == [0.0, 1.0] and out["a"].flags.writeable
    assert NR.unpack(raw, 2, (("a", np.int32, 3), ("b", np.float32, 2)))[1]["b"].dtype == np.float32
    for wrong in (raw + b"\0", raw[:-1], raw[:15], b""):
        with pytest.raises(AssertionError):
            NR.unpack(wrong, 2, fields)


def test_run_refuses_a_program_that_fails_or_does_not_say_ok(tmp_path):
    body = {"ok": 'puts("OK"); fclose(fopen(argv[argc - 1], "wb")); return 0;', "fails": 'puts("OK so far"); return 3;', "silent": 'puts("done"); return 0;'}
    exe = {}
    for name, text in body.items():
        src = tmp_path / f"{name}.c"
        src.write_text("#include <stdio.h>\nint main(int argc, char** argv) { (void)argc; (void)argv; " + text + " }\n")
        exe[name] = str(tmp_path / name)
        subprocess.run(["gcc", str(src), "-o", exe[name]], check=True)
    assert NR.run(exe["ok"], dict(a=np.zeros(3, np.float32), b=None, mode="word")) == b""
    with pytest.raises(RuntimeError, match=r"fails failed \(3\): OK so far"):
        NR.run(exe["fails"], dict(a=np.zeros(3, np.float32)))
    with pytest.raises(RuntimeError, match=r"silent failed \(0\): done"):
        NR.run(exe["silent"], {})


def test_same_bits_tells_nan_payloads_and_signed_zeros():
    f32 = np.float32
    a = np.array([0.0, np.nan, 1.0], f32)
    assert NR.same_bits(a, a.copy()) and NR.same_bits(a.reshape(3, 1)[:, 0], a)
    assert not NR.same_bits(a, np.array([-0.0, np.nan, 1.0], f32)) and not NR.same_bits(a, a.astype(np.float64)) and not NR.same_bits(a, a[:2])
    assert not NR.same_bits(a, (a.view(np.uint32) ^ np.uint32(1 << 21)).view(f32))  # another NaN
    i = np.arange(3, dtype=np.int32)
    assert NR.same_bits(i, i.astype(np.int64)) and not NR.same_bits(i, i.astype(np.int64), same_dtype=True) and not NR.same_bits(i, i + 1)


def test_the_cpu_renderer_refuses_what_the_renderer_refuses_apart_from_the_device():
    """Renderer's own verdict apart from the device: its checks on the same tensor as a subclass that says it lies on cuda:0."""
    torch = pytest.importorskip("torch")

    class OnDevice(torch.Tensor):
        device = property(lambda self: torch.device("cuda", 0))

    def verdict(r, check, t, *args):
        try:
            return ("ok", getattr(r, check)(t, "x", *args))
        except ValueError as e:
            assert "x" in str(e)
            return ("refused", None)

    real = R.Renderer.__new__(R.Renderer)
    real._lib, real._ctx, real.device = None, None, 0
    cpu = AB.cpu_renderer()
    assert (cpu._lib, cpu._ctx, cpu.device) == (None, None, 0) and isinstance(cpu, R.Renderer)
    z = torch.zeros
    i32, i64 = torch.int32, torch.int64
    table = {
        "_device_rows": ((3,), [z(4, 3), z(12), z(0, 3), z(4, 4), z(13), z(4, 3, 1), z(3, 4).t(), z(8, 3)[::2], z(4, 3).double(), z(4, 3, dtype=i32),
                                np.zeros((4, 3), np.float32), [[0.0] * 3] * 4, None]),
        "_device_i32": ((4,), [z(4, dtype=i32), z(5, dtype=i32), z(3, dtype=i32), z(4, 1, dtype=i32), z(2, 2, dtype=i32), z(8, dtype=i32)[::2], z(4, dtype=i64), z(4),
                               np.zeros(4, np.int32), None]),
        "_device_i64": ((4,), [z(4, dtype=i64), z(5, dtype=i64), z(4, 1, dtype=i64), z(8, dtype=i64)[::2], z(4, dtype=i32), z(4), np.zeros(4, np.int64), None]),
        "_device_i32_rows": ((4, 2), [z(4, 2, dtype=i32), z(4, 3, dtype=i32), z(5, 2, dtype=i32), z(8, dtype=i32), z(2, 4, dtype=i32).t(), z(4, 4, dtype=i32)[:, ::2],
                                      z(4, 2, dtype=i64), z(4, 2), np.zeros((4, 2), np.int32), None]),
    }
    for check, (args, tensors) in table.items():
        seen = set()
        for t in tensors:
            on_device = t.as_subclass(OnDevice) if isinstance(t, torch.Tensor) else t
            want = verdict(real, check, on_device, *args)
            assert verdict(cpu, check, t, *args) == want, (check, t)
            if isinstance(t, torch.Tensor):
                assert verdict(real, check, t, *args) == ("refused", None), (check, t)  # (the device is what the real one refuses a CPU tensor for)
            seen.add(want[0])
        assert seen == {"ok", "refused"}, check


def test_expected_fill_on_three_items_by_hand():
    """Three items with lists of 2, 3 and 1 entries at [0, 2), [2, 5), [5, 6) of the reference; 8 entries of room."""
    offsets, count, capacity = [0, 2, 5, 6], [2, 3, 1], 8
    # [1, 3) fits its 2 entries; [3, 5) is one short of its 3: the first 2, 1 beyond; [5, 9) ends beyond the capacity: untouched, incomplete
    got = L.expected_fill([1, 3, 5, 9], capacity, offsets, count)
    assert got["dst"].tolist() == [1, 2, 3, 4] and got["src"].tolist() == [0, 1, 2, 3] and (got["written"], got["beyond"], got["incomplete"]) == (4, 1, 1)
    # [4, 2) is reversed and [2, 2) empty: nothing written, all 2 + 3 entries beyond, but nothing that a capacity would mend; [2, 3) fits
    got = L.expected_fill([4, 2, 2, 3], capacity, offsets, count)
    assert got["dst"].tolist() == [2] and got["src"].tolist() == [5] and (got["written"], got["beyond"], got["incomplete"]) == (1, 5, 0)
    # [-1, 1) begins below 0: untouched though long enough, incomplete; the other two fit
    got = L.expected_fill([-1, 1, 4, 5], capacity, offsets, count)
    assert got["dst"].tolist() == [1, 2, 3, 4] and got["src"].tolist() == [2, 3, 4, 5] and (got["written"], got["beyond"], got["incomplete"]) == (4, 0, 1)
    # the count step's own offsets: everything, in place
    got = L.expected_fill(offsets, capacity, offsets, count)
    assert got["dst"].tolist() == got["src"].tolist() == list(range(6)) and (got["written"], got["beyond"], got["incomplete"]) == (6, 0, 0)
    # an invalid item (a negative count) has no entries, whatever its slice
    got = L.expected_fill([0, 2, 5, 6], capacity, offsets, [2, -2, 1])
    assert got["dst"].tolist() == [0, 1, 5] and got["src"].tolist() == [0, 1, 5] and (got["written"], got["beyond"], got["incomplete"]) == (3, 0, 0)


@pytest.mark.parametrize("kind", L.KINDS, ids=[k.stem for k in L.KINDS])
def test_a_listing_names_what_the_product_has(kind):
    stats, params = getattr(_lib, kind.stats_class), getattr(_lib, kind.params)
    members = [n for n, _ in stats._fields_]
    for name in (kind.items, kind.invalid, kind.found, kind.written, kind.incomplete, "slice_overflow", "stack_overflow", "nodes_visited", "tris_tested", "launches", "ms"):
        assert name in members, name
    assert len({kind.items, kind.invalid, kind.found, kind.written, kind.incomplete}) == 5
    assert "count_traversal" in [n for n, _ in params._fields_] and getattr(R, kind.params) is params
    for name in kind.functions():
        assert name in _lib.PROTOTYPES, name
    count, fill, lst = (_lib.PROTOTYPES[name][1] for name in kind.functions())
    source = len(kind.null_source)
    assert len(count) == 1 + source + 4 and len(fill) == 1 + source + 6 and len(lst) == 1 + source + 7  # ctx, the source, n, params, the outputs
    assert count[1 + source + 1] == fill[1 + source + 1] == lst[1 + source + 1] == C.POINTER(params)
    for method in ("count_" + kind.stem, "list_" + kind.stem, kind.stats):
        assert callable(getattr(R.Renderer, method)), method
    assert (kind.key_dtype == np.int32) == kind.tri_first and [key for key, _ in kind.payload] == (["tri", kind.key] if kind.tri_first else [kind.key, "tri"])
