"""The C signatures binding.lib() gives every export come from include/legkilo_hip.h (abi.signatures): the names are the header's, the types are
the closed map of abi._ctype and nothing else, a prototype the parser cannot read is an error, and every function of the loaded library carries
its restype and argtypes - so ctypes converts a bare Python value to the header's width and refuses a wrong one.  No device is touched."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from legkilo_amd import abi, binding

I32, U32, U64, SZ, F64, F32, PTR, STR = C.c_int32, C.c_uint32, C.c_uint64, C.c_size_t, C.c_double, C.c_float, C.c_void_p, C.c_char_p

# written out by hand from the header: each scalar type, each kind of return value, the awkward layouts
EXPECTED = {
    "lk_create": (I32, [PTR, PTR]),                                                   # const lk_config*, lk_handle**
    "lk_destroy": (None, [PTR]),                                                      # void
    "lk_last_error": (STR, [PTR]),                                                    # const char* return
    "lk_stream": (PTR, [PTR]),                                                        # void* return
    "lk_map_slide": (I32, [PTR, PTR, F64, I32, PTR, PTR]),                            # two lines, `position /*3*/`
    "lk_decode_scan_dev": (I32, [PTR, PTR, SZ, PTR, F64, I32, F32, F64, PTR, PTR, PTR, PTR]),   # int, float and double mixed
    "lk_runs_bucket_poses_dev": (I32, [PTR, U64, SZ, PTR]),                           # uint64_t
    "lk_test_stall": (I32, [PTR, U32]),                                               # unsigned int
    "lk_map_clear_outside": (I32, [PTR, I32, I32, I32, I32, I32, I32, PTR]),          # six int32_t
    "lk_profile_get": (I32, [PTR, STR, PTR, PTR]),                                    # const char* parameter
}


def test_names_are_the_headers():
    assert sorted(abi.signatures()) == ge.declared_symbols()
    assert binding.EXPORTS == sorted(abi.signatures())


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_hand_written_signatures(name):
    assert abi.signatures()[name] == EXPECTED[name]


def test_every_type_is_of_the_closed_map():
    allowed = {I32, U32, U64, SZ, F64, F32, PTR, STR}
    for name, (restype, argtypes) in abi.signatures().items():
        assert restype in (I32, None, STR, PTR), name
        assert set(argtypes) <= allowed, name


def test_unknown_types_and_unreadable_prototypes_are_errors():
    good = "int lk_a(lk_handle* h, size_t n);\nvoid lk_b(void);\n"
    assert abi.parse_signatures(good) == {"lk_a": (I32, [PTR, SZ]), "lk_b": (None, [])}
    with pytest.raises(abi.LegKiloError, match="lk_odd.*long"):
        abi.parse_signatures(good + "int lk_odd(lk_handle* h, long n);\n")                    # a parameter type outside the map
    with pytest.raises(abi.LegKiloError, match="lk_odd.*return type.*long"):
        abi.parse_signatures(good + "long lk_odd(lk_handle* h);\n")                           # a return type outside the map
    with pytest.raises(abi.LegKiloError, match="lk_odd"):
        abi.parse_signatures(good + "int lk_odd(lk_handle* h, size_t);\n")                    # no parameter name: the type is not guessed
    with pytest.raises(abi.LegKiloError, match="lk_odd"):
        abi.parse_signatures(good + "int lk_odd(lk_handle* h, void (*cb)(int), size_t n);\n")  # a function pointer is no type of the map
    for unreadable in ("static inline int lk_odd(int a) { return a; }\n", "int (lk_odd)(int a);\n#define LK_CALL(x) lk_odd(x)\n"):
        with pytest.raises(abi.LegKiloError, match="cannot read.*lk_odd"):                     # declared_symbols() sees it, the strict pattern does not
            abi.parse_signatures(good + unreadable)
    sigs = abi.parse_signatures(good + "/* int lk_gone(long n);\n */\nint lk_c(\n    const double* p /*3*/,\n    float f);\n")   # comments are no code
    assert sigs["lk_c"] == (I32, [PTR, F32]) and "lk_gone" not in sigs


def test_the_loaded_library_carries_every_signature():
    binding.build()
    L = binding.lib()
    for name, (restype, argtypes) in abi.signatures().items():
        fn = getattr(L, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    assert L.lk_abi_version() == 1


def test_pointer_slots_take_64_bits():
    for v in (0, 2 ** 40, None, C.c_void_p(2 ** 40), C.byref(C.c_size_t()), (abi.lk_pose * 2)()):
        C.c_void_p.from_param(v)
    slot = abi.signatures()["lk_device_free"][1][1]
    assert slot is C.c_void_p and C.sizeof(slot) == 8
    with pytest.raises(TypeError):
        slot.from_param(C.c_uint32(1))   # an instance of another ctypes type is refused, not reinterpreted
    with pytest.raises(TypeError):
        slot.from_param(1.0)


def test_staged_memory_is_freed_when_the_body_raises():
    """binding's one staging helper against a stand-in library: what it allocates, uploads and yields, and that an exception in the body, or
    in an upload half way through, still frees every pointer it had taken."""
    class Lib:
        live, uploads, fail_h2d = set(), [], False

        def lk_device_malloc(self, h, out, nbytes):
            ptr = 0x10000 * (len(self.live) + 1)
            C.cast(out, C.POINTER(C.c_void_p))[0] = ptr
            self.live.add(ptr)
            return 0

        def lk_device_free(self, h, ptr):
            self.live.remove(ptr)
            return 0

        def lk_memcpy_h2d(self, h, dst, src, nbytes):
            self.uploads.append((dst, nbytes))
            return -2 if self.fail_h2d else 0

        def lk_last_error(self, h):
            return b"stand-in"

    g = object.__new__(binding.LegKiloHip)
    g.L, g.h = Lib(), None
    with pytest.raises(KeyError):
        with g._staged(np.zeros(4), None, 48) as (a, b, c):
            assert (a, b, c) == (0x10000, 0, 0x20000) and g.L.live == {a, c} and g.L.uploads == [(a, 32)]
            raise KeyError
    assert not g.L.live
    g.L.fail_h2d = True
    with pytest.raises(binding.LegKiloError, match="stand-in"):
        with g._staged(48, np.zeros(2)):
            pytest.fail("the body must not run after a failed upload")
    assert not g.L.live


def test_binding_calls_only_declared_exports():
    called = set(re.findall(r"self\.L\.(lk_\w+)", inspect.getsource(binding)))
    assert len(called) > 100
    assert called <= set(abi.signatures()), called - set(abi.signatures())
