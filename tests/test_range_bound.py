"""lk_range_bound (leg-kilo_amd/csrc/lk_range_bound.h): the frozen-map grid's range gate as two float compares.

The header is plain C++ away from hipcc, so a host harness is compiled around it with the system compiler and compared, float by float, with
the gate it replaces:  (x >= 0 && x <= X*)  must equal  ((double)sqrtf(x) <= 3.0 * (double)radius)  for every float x.  No GPU involved.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "leg-kilo_amd", "csrc")

HARNESS = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "lk_range_bound.h"

static bool gate_sqrt(float x, float radius) {   // lk_point_kernels.h, eval_plane: the form pool records keep
    volatile float range_dis = sqrtf(x);
    return (double)range_dis <= 3.0 * (double)radius;
}
static bool gate_bound(float x, float bound) { return x >= 0.f && x <= bound; }
// floats as ordered integers: a step of one is a step of one ulp, across zero as well
static int64_t to_ord(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? -(int64_t)(u & 0x7fffffffu) : (int64_t)u;
}
static float from_ord(int64_t o) {
    uint32_t u = o < 0 ? (0x80000000u | (uint32_t)(-o)) : (uint32_t)o;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> radii;
    float r;
    while (fread(&r, 4, 1, f) == 1) radii.push_back(r);
    fclose(f);
    const float fmax = 3.4028234663852886e38f;
    uint32_t nan_bits = 0x7fc00000u, den_bits = 1u, nzero_bits = 0x80000000u;
    float qnan, den, nzero;
    memcpy(&qnan, &nan_bits, 4), memcpy(&den, &den_bits, 4), memcpy(&nzero, &nzero_bits, 4);
    const float special[] = {0.f, nzero, den, fmax, INFINITY, qnan, -1.f};
    unsigned long long checked = 0, bad = 0;
    for (float radius : radii) {
        const float X = lk_range_bound(radius);
        auto check = [&](float x) {
            ++checked;
            if (gate_sqrt(x, radius) != gate_bound(x, X)) {
                if (bad < 20) printf("MISMATCH radius %a x %a bound %a sqrt-gate %d\n", radius, x, X, (int)gate_sqrt(x, radius));
                ++bad;
            }
        };
        for (float x : special) check(x);
        if (X == X && fabsf(X) <= fmax) {   // a finite bound: every float within 8 ulps of it, both sides
            const int64_t o = to_ord(X), top = to_ord(fmax);
            for (int64_t k = -8; k <= 8; ++k) {
                const int64_t v = o + k;
                if (v > top || v < -top) continue;
                check(from_ord(v));
            }
        }
    }
    printf("radii %zu checked %llu bad %llu\n", radii.size(), checked, bad);
    return bad ? 1 : 0;
}
"""


def radii():
    rng = np.random.default_rng(20261)
    e = np.exp(rng.uniform(np.log(1e-8), np.log(16.0), 2400))
    out = [np.sqrt(e).astype(np.float32)]                       # (float)sqrt(emax): how a plane's radius comes about
    # radii whose triple is exactly a float (3 * (2 k) needs no more than 24 bits: the gate's threshold sits ON a float)
    k = rng.integers(1, (1 << 24) // 3, 300).astype(np.float64)
    out.append((k * np.exp2(rng.integers(-30, 4, 300).astype(np.float64))).astype(np.float32))
    assert all(float(np.float32(3.0 * float(r))) == 3.0 * float(r) for r in out[-1])
    out.append(np.exp2(np.arange(-149, 128, dtype=np.float64)).astype(np.float32))   # powers of two, denormal ones included
    fi = np.finfo(np.float32)
    out.append(np.array([fi.tiny, 1e-41, 3e-45, 0.0, -0.0, -0.37, -fi.tiny, fi.max, fi.max / 3, np.float32(fi.max) / np.float32(2.9), np.inf, -np.inf, np.nan],
                        dtype=np.float32))
    return np.concatenate(out)


def test_range_bound_agrees_with_the_sqrt_gate(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe, dat = tmp_path / "range_bound_harness.cc", tmp_path / "range_bound_harness", tmp_path / "radii.f32"
    src.write_text(HARNESS)
    r = radii()
    assert len(r) >= 2000
    r.tofile(dat)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    res = subprocess.run([str(exe), str(dat)], capture_output=True, text=True)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-500:]
    assert f"radii {len(r)} " in res.stdout and " bad 0" in res.stdout
