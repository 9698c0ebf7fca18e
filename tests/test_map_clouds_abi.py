"""CPU checks of the map-cloud entries (include/legkilo_hip.h: lk_downsample_clouds_dev, lk_downsample_clouds): both symbols are declared, exported by
the cross-compiled library and listed in binding.EXPORTS; binding.pcd_file_offsets - which registered points go into which map file - is the
counting of PcdSaver::workerLoop, restated here as the literal loop; and its C++ twin (leg-kilo_amd/csrc/lk_pcd_files.h) gives the same tables as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from legkilo_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lk_downsample_clouds_dev", "lk_downsample_clouds"]
RUN_LEN = [3, 1, 4, 2, 1, 3]
FPF = [1, 2, 3, 100, 0, -1]
# the tables of tests/pcd_files_main.cc: a scan without points inside run 2 and at the end of run 5, the first scan at record 13
SCAN_LEN_HOLES = [5, 7, 2, 9, 4, 0, 6, 1, 8, 3, 11, 2, 5, 0]


def worker_loop(run_off, scan_off, frames_per_file):
    """PcdSaver (pcd_saver.hpp:30-33, :91-135) fed run after run, a new saver per run: -> [(first record, end record, run)] of the files written."""
    files = []
    for r in range(len(run_off) - 1):
        if frames_per_file <= 0:
            frames_per_file = 100
        buffer, frames_in_buffer = [], 0

        def downsample_and_save():
            nonlocal buffer, frames_in_buffer
            if not buffer:
                return
            files.append((buffer[0], buffer[-1] + 1, r))
            buffer, frames_in_buffer = [], 0

        for s in range(int(run_off[r]), int(run_off[r + 1])):
            cloud = list(range(int(scan_off[s]), int(scan_off[s + 1])))
            if not cloud:
                continue
            buffer += cloud
            frames_in_buffer += 1
            if frames_in_buffer >= frames_per_file:
                downsample_and_save()
        if buffer:   # stopping_
            downsample_and_save()
    return files


def tables(scan_len, first):
    run_off = np.r_[0, np.cumsum(RUN_LEN)].astype(np.uint32)
    scan_off = (first + np.r_[0, np.cumsum(scan_len)]).astype(np.uint64)
    assert run_off[-1] == len(scan_len)
    return run_off, scan_off


@pytest.fixture(scope="module")
def hip():
    binding.build()
    return C.CDLL(binding.LIB_PATH)


def test_new_symbols_are_declared_and_exported(hip):
    for s in NEW_SYMBOLS:
        assert s in ge.declared_symbols(), s
        assert hasattr(hip, s), s
        assert s in binding.EXPORTS, s


@pytest.mark.parametrize("fpf", FPF)
@pytest.mark.parametrize("case", ["full", "holes"])
def test_file_offsets_are_the_worker_loops(fpf, case):
    scan_len = [4, 6, 1, 7, 3, 2, 9, 5, 8, 1, 2, 6, 4, 3] if case == "full" else SCAN_LEN_HOLES
    for first in (0, 13):
        run_off, scan_off = tables(scan_len, first)
        want = worker_loop(run_off, scan_off, fpf)
        file_off, file_run = binding.pcd_file_offsets(run_off, scan_off, fpf)
        assert file_off.dtype == np.uint64 and len(file_off) == len(want) + 1 and len(file_run) == len(want)
        assert [(int(a), int(b), int(r)) for a, b, r in zip(file_off[:-1], file_off[1:], file_run)] == want, (fpf, case, first)
        assert int(file_off[0]) == first and int(file_off[-1]) == int(scan_off[-1])
    per_run = {1: RUN_LEN, 2: [2, 1, 2, 1, 1, 2], 3: [1, 1, 2, 1, 1, 1]}.get(fpf, [1] * 6)
    if case == "full":
        assert np.bincount(file_run).tolist() == per_run, "the cases do not cut where they are meant to"


def test_no_points_no_file():
    file_off, file_run = binding.pcd_file_offsets([0, 2], [7, 7, 7], 1)
    assert file_off.tolist() == [7] and len(file_run) == 0


def test_cpp_twin_under_the_host_sanitizers(tmp_path):
    """tests/pcd_files_main.cc: a program of its own with -fsanitize=address,undefined, the runtimes linked statically (nothing is loaded into this
    process); it prints its tables, which must be Python's."""
    exe = tmp_path / "pcd_files"
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "leg-kilo_amd", "csrc"), os.path.join(ROOT, "tests", "pcd_files_main.cc"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)] + [str(f) for f in FPF], capture_output=True, text=True)
    assert r.returncode == 0 and "pcd files ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()[:-1]
    assert len(lines) == len(FPF)
    run_off, scan_off = tables(SCAN_LEN_HOLES, 13)
    for fpf, line in zip(FPF, lines):
        head, offs, runs = [[int(v) for v in part.split()] for part in line.split("|")]
        file_off, file_run = binding.pcd_file_offsets(run_off, scan_off, fpf)
        assert head == [fpf, len(file_run)] and offs == file_off.tolist() and runs == file_run.tolist(), (fpf, line)
