"""The decision a frozen-map batch replay takes from its content stamp (leg-kilo_amd/csrc/lk_batch_stamp.h: lk_stamp_decide, the code lk_batch_stamp_kernel
runs, compiled for the host from the same header by tools/probes/batch_stamp_host.cc).  lk_batch_order's state is split between the host, which picks
LK_ORD_PROBE / LK_ORD_CHECK from a count that lags behind the replays in flight, and the device; so EVERY order of (mode, stamp) must be safe:

  - a replay is told to read the library's copy only if its stamp is the stamp of the last LK_ORD_SET - all sequences over three stamps and the three
    modes up to length 6 after SET(X), on one ring and rotating over three;
  - after a mismatch the count the host reads stays below LK_ORD_SORTED until the next SET, and only PROBE launches that saw the same stamp in a row raise it;
  - a stamp is never 0, and 0 in the words means "no stamp yet";
  - the decision words of the ring streams do not affect each other.

The same enumeration run over the logic the kernel had before (shared last-stamp / decision words, -DLK_STAMP_PARENT_LOGIC) must FAIL: the check has teeth."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE, CHECK, SET = 0, 1, 2
X, Y, Z = 0x1234567890ABCDEF, 0x0FEDCBA987654321, 0x8000000000000001
M64 = (1 << 64) - 1


def _load(tmp, name, *defs):
    so = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", *defs, "-o", so, os.path.join(ROOT, "tools", "probes", "batch_stamp_host.cc")])
    L = ctypes.CDLL(so)
    lay = (ctypes.c_int * 6)()
    size = L.lk_stamp_host_layout(lay)
    L.w_copy, L.w_last, L.w_use, L.rings, L.n_words, L.sorted = (int(v) for v in lay)

    class State(ctypes.Structure):
        _fields_ = [("w", ctypes.c_ulonglong * L.n_words), ("seen", ctypes.c_uint)]

    assert ctypes.sizeof(State) == size
    L.State = State
    L.lk_stamp_host_reset.argtypes = [ctypes.POINTER(State)]
    L.lk_stamp_host_step.argtypes = [ctypes.POINTER(State), ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int]
    L.lk_stamp_host_enumerate.restype = ctypes.c_uint64
    L.lk_stamp_host_enumerate.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.lk_stamp_host_of.restype = ctypes.c_ulonglong
    L.lk_stamp_host_of.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def stamp(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("stamp"), "batch_stamp_host.so")


@pytest.fixture(scope="module")
def parent(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("stamp_parent"), "batch_stamp_parent.so", "-DLK_STAMP_PARENT_LOGIC")


def enumerate_all(L, length, stamps, n_rings):
    """-> sequences that break a rule, {rule: (how many broke it first, the first of them)}."""
    st = (ctypes.c_ulonglong * 3)(*stamps)
    first, by_rule = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    bad = int(L.lk_stamp_host_enumerate(length, st, n_rings, first, by_rule))
    rules = {}
    for r in (1, 2, 3):
        seq, q = [], int(first[r])
        for _ in range(length):
            seq.append(("PROBE", "CHECK", "SET")[q % 9 // 3] + " " + "XYZ"[q % 3])
            q //= 9
        if by_rule[r]:
            rules[r] = (int(by_rule[r]), "SET X, " + ", ".join(seq))
    return bad, rules


def run(L, steps, ring=0):
    """[(mode, stamp) or (mode, stamp, ring)] from cleared words -> [(told to read the copy, count the host reads)] per step, and the state."""
    s = L.State()
    L.lk_stamp_host_reset(ctypes.byref(s))
    out = []
    for step in steps:
        mode, st = step[0], step[1]
        use = L.lk_stamp_host_step(ctypes.byref(s), mode, st, step[2] if len(step) > 2 else ring)
        out.append((use, int(s.seen)))
    return out, s


@pytest.mark.parametrize("n_rings", [1, 3])
@pytest.mark.parametrize("stamps", [(X, Y, Z), (1, 3, M64)], ids=["mixed", "small and all-ones"])
def test_every_sequence_up_to_length_6(stamp, stamps, n_rings):
    # every step of every sequence is checked, so length 6 covers the shorter ones: 9 ** 6 = 531 441 sequences
    bad, rules = enumerate_all(stamp, 6, stamps, n_rings)
    assert bad == 0, f"{bad} sequences break a rule (1 copy read on another stamp, 2 count, 3 current copy not read): {rules}"


def test_the_enumeration_fails_on_the_former_logic(parent):
    """The three branches the kernel had before: the new stamp adopted as the reference on a mismatch, one decision word for all streams."""
    bad, rules = enumerate_all(parent, 6, (X, Y, Z), 1)
    print(f"former logic: {bad} of {9 ** 6} sequences break a rule; by the rule broken first (1 copy read on another stamp, 2 count, 3 current copy not read): {rules}")
    assert bad > 0 and rules[1][0] > 0      # among them replays sent to a copy of other content
    _, short = enumerate_all(parent, 2, (X, Y, Z), 1)
    assert short[1][0] > 0, short                    # two replays after the SET are enough
    out, _ = run(parent, [(SET, X), (CHECK, Y), (CHECK, Y)])
    assert [u for u, _ in out] == [1, 0, 1]          # the second CHECK of new content is sent to the stale copy
    out, _ = run(parent, [(SET, X), (CHECK, Y), (CHECK, Y), (CHECK, X)])
    assert [u for u, _ in out] == [1, 0, 1, 0]       # ... and the content the copy WAS made from no longer reads it


def test_named_sequences(stamp):
    S = stamp.sorted
    # the defect: two CHECK launches of new content enqueued while the host still saw LK_ORD_SORTED - both read the caller's buffer
    out, s = run(stamp, [(SET, X), (CHECK, Y), (CHECK, Y)])
    assert out == [(1, S), (0, 1), (0, 1)]
    assert s.w[stamp.w_copy] == X and s.w[stamp.w_last] == Y
    # ... and the old content put back: the copy is of that content again, but the host is still told to forget it (the count stays down)
    out, _ = run(stamp, [(SET, X), (CHECK, Y), (CHECK, Y), (CHECK, X)])
    assert out == [(1, S), (0, 1), (0, 1), (1, 1)]
    # unchanged content: CHECK after CHECK reads the copy and leaves the count alone
    out, _ = run(stamp, [(SET, X), (CHECK, X), (CHECK, X), (CHECK, X)])
    assert out == [(1, S)] * 4
    # first sight, counting, the third replay sorts (the host's part: count >= 2 -> SET)
    out, _ = run(stamp, [(PROBE, X), (PROBE, X), (SET, X), (CHECK, X)])
    assert out == [(0, 1), (0, 2), (1, S), (1, S)]
    # after a mismatch only PROBE launches in a row count: CHECK Y, CHECK Y is still 1; PROBE Y 2; PROBE Z starts again
    out, _ = run(stamp, [(SET, X), (CHECK, Y), (CHECK, Y), (PROBE, Y), (PROBE, Z), (PROBE, Z), (PROBE, Y)])
    assert out == [(1, S), (0, 1), (0, 1), (0, 2), (0, 1), (0, 2), (0, 1)]
    # Y, X, Y is not "Y twice in a row", even though the CHECK of X in between read the copy
    out, _ = run(stamp, [(SET, X), (CHECK, Y), (CHECK, X), (PROBE, Y)])
    assert out == [(1, S), (0, 1), (1, 1), (0, 1)]
    # a PROBE never reads the copy, not even on the copy's stamp (the host passes no copy with it)
    out, _ = run(stamp, [(SET, X), (CHECK, Y), (PROBE, X), (PROBE, X)])
    assert out == [(1, S), (0, 1), (0, 1), (0, 2)]


def test_zero_means_no_stamp_yet(stamp):
    for st in (1, 3, X, M64):
        out, _ = run(stamp, [(CHECK, st)])         # cleared words: no copy - a CHECK cannot match, whatever its stamp
        assert out == [(0, 1)]
        out, _ = run(stamp, [(PROBE, st)])         # ... and the first PROBE is a first sight, not a repeat
        assert out == [(0, 1)]


def py_stamp(pts4):
    """lk_batch_stamp_kernel's stamp of [n, 4] uint32 records in Python integers."""
    n = len(pts4)
    stride = n // 4096 or 1
    total = 0
    for k in range(4096):
        idx = k * stride
        if idx >= n:
            break
        x, y, z, w = (int(v) for v in pts4[idx])
        m = ((x | (y << 32)) ^ (0x9E3779B97F4A7C15 * (idx + 1))) & M64
        m = ((m ^ (m >> 31)) * 0xBF58476D1CE4E5B9) & M64
        m ^= ((z | (w << 32)) * 0x94D049BB133111EB) & M64
        m = ((m ^ (m >> 29)) * 0xC2B2AE3D27D4EB4F) & M64
        total = (total + (m ^ (m >> 32))) & M64
    return total | 1


@pytest.mark.parametrize("n", [1, 100, 4095, 4096, 6144, 8191, 8192, 20000])
def test_stamp_of_a_byte_pattern(stamp, n):
    rng = np.random.default_rng(n)
    pts = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint32)
    st = int(stamp.lk_stamp_host_of(pts.ctypes.data, n))
    assert st == py_stamp(pts) and st & 1
    stride = n // 4096 or 1
    last = min(4095, (n - 1) // stride) * stride      # the last sampled point
    for idx in {0, last}:                               # one bit in a sampled point: another stamp
        q = pts.copy()
        q[idx, 0] ^= 1
        assert int(stamp.lk_stamp_host_of(q.ctypes.data, n)) != st, idx
    blind = [i for i in (1, last + 1, n - 1) if i < n and (i % stride != 0 or i // stride >= 4096)]
    for idx in blind:                                   # a point outside the sample: the same stamp (what lk_batch_changed is for)
        q = pts.copy()
        q[idx] ^= 0xFFFFFFFF
        assert int(stamp.lk_stamp_host_of(q.ctypes.data, n)) == st, idx
    if n >= 2 * stride + 1:                             # two sampled points exchanged: the index is mixed in, so another stamp
        q = pts.copy()
        q[[0, stride]] = q[[stride, 0]]
        assert int(stamp.lk_stamp_host_of(q.ctypes.data, n)) != st


def test_stamp_is_never_zero(stamp):
    assert int(stamp.lk_stamp_host_of(None, 0)) == 1                       # an empty sum
    z = np.zeros((64, 4), dtype=np.uint32)
    assert int(stamp.lk_stamp_host_of(z.ctypes.data, 64)) & 1
    rng = np.random.default_rng(7)
    for _ in range(200):
        p = rng.integers(0, 1 << 32, size=(int(rng.integers(1, 300)), 4), dtype=np.uint32)
        assert int(stamp.lk_stamp_host_of(p.ctypes.data, len(p))) & 1


def test_decision_words_of_the_rings_are_independent(stamp):
    """Replays of one batch on three ring streams: a ring's pair holds the stamp and the decision of THAT ring's last replay, whatever the others did since."""
    rng = np.random.default_rng(11)
    for _ in range(300):
        s = stamp.State()
        stamp.lk_stamp_host_reset(ctypes.byref(s))
        mine = {}
        steps = [(SET, X, int(rng.integers(0, stamp.rings)))] + [(int(rng.integers(0, 3)), (X, Y, Z)[int(rng.integers(0, 3))], int(rng.integers(0, stamp.rings))) for _ in range(12)]
        for mode, st, ring in steps:
            use = stamp.lk_stamp_host_step(ctypes.byref(s), mode, st, ring)
            assert use in (0, 1)
            mine[ring] = (st, use)
            for r in range(stamp.rings):
                pair = (int(s.w[stamp.w_use + 2 * r]), int(s.w[stamp.w_use + 2 * r + 1]))
                assert pair == mine.get(r, (0, 0)), (steps, r)
    # the case on two streams: ring 0 replays new content while ring 1's residual launches of the OLD content (enqueued before the write) still read their word
    out, s = run(stamp, [(SET, X, 1), (CHECK, X, 1), (CHECK, Y, 0), (CHECK, Y, 2)])
    assert [u for u, _ in out] == [1, 1, 0, 0]
    assert int(s.w[stamp.w_use + 3]) == 1 and int(s.w[stamp.w_use + 1]) == 0 and int(s.w[stamp.w_use + 5]) == 0
