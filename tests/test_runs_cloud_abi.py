"""CPU checks of the _cloud run replays' C-ABI (include/legkilo_hip.h): lk_bucket_pose is 144 bytes with the header's field offsets (a C program
compiled against the header says what they are), the four new symbols are exported by the cross-compiled library, lk_abi_version is the header's -
and the host-side table arithmetic of leg-kilo_amd/csrc/lk_cloud_layout.h runs clean as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

from legkilo_amd import abi, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NEW_SYMBOLS = ["lk_batch_replay_runs_cloud_dev", "lk_batch_replay_overlay_runs_cloud_dev", "lk_runs_bucket_poses_dev", "lk_runs_bucket_poses"]
FIELDS = ["rot", "pos", "vel", "t", "first_point", "n_points", "n_effect"]


@pytest.fixture(scope="module")
def hip():
    binding.build()
    return C.CDLL(binding.LIB_PATH)


def test_bucket_pose_is_144_bytes():
    assert C.sizeof(abi.lk_bucket_pose) == 144
    assert abi.bucket_pose_dtype().itemsize == 144
    assert [f for f, _ in abi.lk_bucket_pose._fields_] == FIELDS == list(abi.bucket_pose_dtype().names)


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + "\\n\", sizeof(lk_bucket_pose), "
                   + ", ".join(f"offsetof(lk_bucket_pose, {f})" for f in FIELDS) + "); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 144
    assert got[1:] == [getattr(abi.lk_bucket_pose, f).offset for f in FIELDS] == [0, 72, 96, 120, 128, 136, 140]
    dt = abi.bucket_pose_dtype()
    assert got[1:] == [dt.fields[f][1] for f in FIELDS]


def test_new_symbols_are_exported(hip):
    for s in NEW_SYMBOLS:
        assert hasattr(hip, s), s
        assert s in binding.EXPORTS


def test_abi_version_is_the_headers(hip):
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert hip.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1))


def test_table_layout_arithmetic_under_the_host_sanitizers(tmp_path):
    """tests/cloud_layout_main.cc: a program of its own with -fsanitize=address,undefined, the runtimes linked statically (nothing is loaded into
    this process, and the program does not depend on what else the loader brings in)."""
    exe = tmp_path / "cloud_layout"
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "leg-kilo_amd", "csrc"), os.path.join(ROOT, "tests", "cloud_layout_main.cc"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "cloud layout ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
