"""Host-only checks of the launch plan of the streaming vector kernels (csrc/vec_launch.hpp: vec_plan, vec_dispatch) through
the test export khip_test_vec_plan, which calls the two functions every launcher calls: no device needed.  The reference is
the rule itself, restated below:

  * 16-byte accesses (VEC = 2) when n >= 2 and every pointer that is there is 16-byte aligned, else 8-byte ones (VEC = 1);
  * non-temporal accesses from nt_min_elems on -- on the 8-byte path only where the kernel file has such instantiations;
  * compensated accumulation as the option says;
  * ceil(nvec / (256 U)) workgroups, never fewer than one, refused beyond 0x7fffffff.
"""
import ctypes as C
import itertools

import pytest

BASE = 0x7F0000001000          # a 16-byte aligned address; nothing is dereferenced
NS = [0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1 << 22, (1 << 22) - 1]
POINTER_SETS = {
    "aligned": [BASE, BASE + 0x100, BASE + 0x200],
    "first+8": [BASE + 8, BASE + 0x100, BASE + 0x200],
    "middle+8": [BASE, BASE + 0x108, BASE + 0x200],
    "last+8": [BASE, BASE + 0x100, BASE + 0x208],
    "null among aligned": [BASE, 0, BASE + 0x200],
    "null among misaligned": [BASE + 8, 0, BASE + 0x208],
}
NEVER, FOLLOW = 0, 1
KHIP_ERR_INVALID = -1             # include/krylov_hip.h


def _lib():
    import krylov_jl_amd as K
    return K.lib()


def reference(n, ptrs, extra, u, nt_min_elems, compensated, policy):
    v2 = n >= 2 and bool(extra) and all(p % 16 == 0 for p in ptrs)          # a null pointer (0) counts as aligned
    nt = n >= nt_min_elems
    comp = compensated != 0
    nvec = n // 2 if v2 else n
    g = max(1, -(-nvec // (256 * u)))
    nt_dispatched = nt and (v2 or policy == FOLLOW)
    return (g, int(v2), int(nt), int(comp)), (2 if v2 else 1, int(nt_dispatched), int(comp))


def plan(n, ptrs, extra=1, u=1, nt_min_elems=1 << 22, compensated=1, policy=FOLLOW):
    arr = (C.c_uint64 * max(1, len(ptrs)))(*ptrs)
    out = (C.c_int64 * 7)(*([-1] * 7))
    rc = _lib().khip_test_vec_plan(n, arr, len(ptrs), extra, u, nt_min_elems, compensated, policy, out)
    return rc, tuple(out[:4]), tuple(out[4:])


@pytest.mark.parametrize("name", list(POINTER_SETS))
def test_plan_and_dispatch_follow_the_rule(name):
    ptrs = POINTER_SETS[name]
    for n, extra, u, nt_min, comp, policy in itertools.product(NS, (1, 0), (1, 4), (1, 1 << 22), (0, 1), (NEVER, FOLLOW)):
        rc, got_plan, got_triple = plan(n, ptrs, extra, u, nt_min, comp, policy)
        want_plan, want_triple = reference(n, ptrs, extra, u, nt_min, comp, policy)
        where = (name, n, extra, u, nt_min, comp, policy)
        assert rc == 0, where
        assert got_plan == want_plan, (where, got_plan, want_plan)
        assert got_triple == want_triple, (where, got_triple, want_triple)


def test_pairs_need_two_elements_and_every_pointer_aligned():
    for n in (0, 1):
        assert plan(n, POINTER_SETS["aligned"])[1][1] == 0
    assert plan(2, POINTER_SETS["aligned"])[1][1] == 1
    for name in ("first+8", "middle+8", "last+8", "null among misaligned"):
        for n in NS:
            assert plan(n, POINTER_SETS[name])[1][1] == 0, (name, n)
    for n in NS[2:]:
        assert plan(n, POINTER_SETS["null among aligned"])[1][1] == 1
        assert plan(n, POINTER_SETS["aligned"], extra=0)[1][1] == 0
        assert plan(n, [])[1][1] == 1                              # no pointer in the list: the table's flag alone decides


def test_an_empty_vector_still_gets_one_workgroup():
    for ptrs, u in itertools.product(POINTER_SETS.values(), (1, 4)):
        assert plan(0, ptrs, u=u)[1][0] == 1


@pytest.mark.parametrize("u", [1, 4])
def test_grid_at_the_tile_edges(u):
    """nvec = n on the 8-byte path and n // 2 on the 16-byte path; a workgroup takes 256 u of them."""
    def g(n, ptrs):
        return plan(n, ptrs, u=u)[1][0]
    odd, even = POINTER_SETS["first+8"], POINTER_SETS["aligned"]
    if u == 1:
        assert [g(n, odd) for n in (255, 256, 257, 511, 512, 513)] == [1, 1, 2, 2, 2, 3]
        assert [g(n, even) for n in (255, 256, 257, 511, 512, 513, 514)] == [1, 1, 1, 1, 1, 1, 2]
    else:
        assert [g(n, odd) for n in (255, 256, 257, 511, 512, 513, 1024, 1025)] == [1, 1, 1, 1, 1, 1, 1, 2]
        assert [g(n, even) for n in (255, 256, 257, 511, 512, 513, 2049, 2050)] == [1, 1, 1, 1, 1, 1, 1, 2]


def test_the_never_policy_keeps_nt_off_the_scalar_path():
    for name, ptrs in POINTER_SETS.items():
        for n, extra, comp in itertools.product(NS, (0, 1), (0, 1)):
            rc, p, (vec, nt, c) = plan(n, ptrs, extra, 1, 1, comp, NEVER)
            assert rc == 0 and p[2] == (n >= 1)                        # the plan itself asks for NT (nt_min_elems = 1) ...
            assert nt == (1 if vec == 2 else 0), (name, n, extra)     # ... and only the 16-byte path gets it
            assert plan(n, ptrs, extra, 1, 1, comp, FOLLOW)[2] == (vec, int(n >= 1), c)


def test_a_grid_beyond_one_launch_is_refused():
    """Arithmetic only: U = 1, unaligned, n = 2^39 + 256 is 2^31 + 1 workgroups."""
    n = (1 << 39) + 256
    rc, _, _ = plan(n, POINTER_SETS["first+8"])
    assert rc == KHIP_ERR_INVALID
    assert _lib().khip_last_error().decode() == "vector too long for one launch"
    assert plan(n - 512, POINTER_SETS["first+8"])[:2] == (0, (0x7FFFFFFF, 0, 1, 1))
    assert plan(n, POINTER_SETS["aligned"])[0] == 0                    # half as many 16-byte accesses: it fits
