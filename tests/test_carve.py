"""The buffer carving helper of the HIP library's host code (leg-kilo_amd/csrc/lk_carve.h, compiled for the host from the same header by
tools/probes/carve_host.cc): one layout description run as a counting pass and over two different buffers.  The counting pass and the
carving passes agree on the total, every array starts at a multiple of its alignment and inside the buffer, no two arrays overlap, and the
two buffers get equal offsets."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (element bytes, count) per array, in carving order
LAYOUTS = {
    "ragged tables": [(8, 5 * 8), (8, 5 * 7), (8, 5), (1, 56 * 3), (4, 5), (4, 6)],
    "mixed 1 / 4 / 8 / 16": [(1, 3), (16, 7), (4, 5), (1, 1), (8, 9), (1, 17), (16, 1), (4, 1), (8, 1)],
    "zero-length arrays": [(8, 0), (4, 11), (1, 0), (16, 0), (1, 5), (8, 2), (4, 0)],
    "all empty": [(16, 0), (1, 0), (8, 0)],
    "one byte": [(1, 1)],
    "per-point arrays": [(4, 1000)] * 8 + [(16, 1000)] * 2 + [(8, 3), (4, 4), (4, 7), (4, 8), (4, 18), (8, 6)],
}


@pytest.fixture(scope="module")
def carve(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("carve") / "carve_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "probes", "carve_host.cc")])
    L = ctypes.CDLL(so)
    L.lk_carve_host.restype = ctypes.c_size_t
    L.lk_carve_host.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 3

    def run(base, min_align, layout):
        elem = np.array([e for e, _ in layout], dtype=np.int32)
        count = np.array([c for _, c in layout], dtype=np.uint64)
        addr = np.full(len(layout), 0xdead, dtype=np.uint64)
        total = L.lk_carve_host(base, min_align, len(layout), elem.ctypes.data, count.ctypes.data, addr.ctypes.data)
        return int(total), [int(a) for a in addr]

    return run


def aligned_base(buf, align):
    return (buf.ctypes.data + align - 1) // align * align


@pytest.mark.parametrize("min_align", [1, 16, 256])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_count_and_carve_agree(carve, name, min_align):
    layout = LAYOUTS[name]
    total, addr0 = carve(0, min_align, layout)
    assert total != 2 ** 64 - 1
    assert addr0 == [0] * len(layout)                       # the counting pass hands out no pointers
    assert total >= sum(e * c for e, c in layout)
    assert total % min_align == 0
    offsets = []
    for seed in (1, 2):                                     # the same description over two different buffers
        buf = np.full(total + 512, seed, dtype=np.uint8)
        base = aligned_base(buf, 256)
        t, addr = carve(base, min_align, layout)
        assert t == total
        offs = [a - base for a in addr]
        for (e, c), o in zip(layout, offs):
            assert o % max(e, min_align) == 0, (name, e, o)  # element sizes here are their own alignment
            assert 0 <= o and o + e * c <= total
        spans = sorted((o, o + e * c) for (e, c), o in zip(layout, offs) if c)
        for (_, end), (start, _) in zip(spans, spans[1:]):
            assert end <= start, (name, spans)
        assert offs == sorted(offs)                          # arrays lie in the order they were taken
        offsets.append(offs)
    assert offsets[0] == offsets[1]

