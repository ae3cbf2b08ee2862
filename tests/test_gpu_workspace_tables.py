"""The vector tables of the minres!, bilq!, qmr! and bilqr! workspaces through the raw C entry points: what
khip_*_workspace_adopt, _adopt_vector, _create, _destroy, khip_*_vector and khip_*_workspace_bytes accept, refuse, return and
say.  The other test files pin the messages by substring only; here every refusal is compared with its whole text.  Nothing
solves a system."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

N = 5

# solver -> (arguments between n and the vectors, core names in the order of khip_*_workspace_adopt, lazy names in the order
# of the "unknown vector" message, the two refusals of khip_*_workspace_adopt)
TABLES = {
    "minres": ((5,), ("x", "r1", "r2", "w1", "w2", "y"), ("dx", "v", "npc_dir"),
               b"minres_workspace_adopt: x, r1, r2, w1, w2, y must be device vectors of n entries",
               b"minres_workspace_adopt: x, r1, r2, w1, w2, y must be distinct"),
    "bilq": ((), ("u_prev", "u", "q", "v_prev", "v", "p", "x", "dbar"), ("dx", "t", "s"),
             b"bilq_workspace_adopt: u_prev, u, q, v_prev, v, p, x, dbar must be device vectors of n entries",
             b"bilq_workspace_adopt: u_prev, u, q, v_prev, v, p, x, dbar must be distinct"),
    "qmr": ((), ("u_prev", "u", "q", "v_prev", "v", "p", "x", "w_prev2", "w_prev"), ("dx", "t", "s"),
            b"qmr_workspace_adopt: u_prev, u, q, v_prev, v, p, x, w_prev2, w_prev must be device vectors of n entries",
            b"qmr_workspace_adopt: u_prev, u, q, v_prev, v, p, x, w_prev2, w_prev must be distinct"),
    "bilqr": ((), ("u_prev", "u", "q", "v_prev", "v", "p", "x", "y", "dbar", "w_prev3", "w_prev2"), ("dx", "dy"),
              b"bilqr_workspace_adopt: u_prev, u, q, v_prev, v, p, x, y, dbar, w_prev3, w_prev2 must be device vectors of n entries",
              b"bilqr_workspace_adopt: u_prev, u, q, v_prev, v, p, x, y, dbar, w_prev3, w_prev2 must be distinct"),
}


class Entries:
    def __init__(self, L, solver):
        self.L, self.solver = L, solver
        self.extra = TABLES[solver][0]

    def fn(self, name):
        return getattr(self.L, f"khip_{self.solver}_{name}")

    def adopt(self, ctx, n, ptrs):
        h = C.c_void_p()
        return self.fn("workspace_adopt")(ctx._h, n, n, *self.extra, *ptrs, C.byref(h)), h

    def create(self, ctx, n):
        h = C.c_void_p()
        return self.fn("workspace_create")(ctx._h, n, n, *self.extra, C.byref(h)), h

    def snapshot(self, h, names):
        return self.fn("workspace_bytes")(h), {k: self.fn("vector")(h, k.encode()) for k in names}


@pytest.mark.parametrize("solver", sorted(TABLES))
def test_adoption_and_lookup(K, ctx, solver):
    _, core, lazy, _, _ = TABLES[solver]
    E = Entries(K.lib(), solver)
    vec = {k: ctx.empty(N) for k in core + lazy}
    rc, h = E.adopt(ctx, N, [vec[k].ptr for k in core])
    assert rc == 0
    for k in core:
        assert E.fn("vector")(h, k.encode()) == vec[k].ptr, k
    for k in lazy + ("nope", ""):
        assert E.fn("vector")(h, k.encode()) is None, k
    assert E.fn("workspace_bytes")(h) == len(core) * 8 * N
    for i, k in enumerate(lazy):
        assert E.fn("workspace_adopt_vector")(h, k.encode(), vec[k].ptr) == 0, k
        assert E.fn("workspace_bytes")(h) == (len(core) + i + 1) * 8 * N
        assert E.fn("vector")(h, k.encode()) == vec[k].ptr, k
    for k in core:                                                       # the core vectors are where they were
        assert E.fn("vector")(h, k.encode()) == vec[k].ptr, k
    assert E.fn("workspace_destroy")(h) == 0
    for v in vec.values():                                               # nothing of the caller's was freed
        K.kfill_(v, 1.0)
    assert K.knorm(N, vec[core[0]]) == pytest.approx(N ** 0.5)


@pytest.mark.parametrize("solver", sorted(TABLES))
def test_adopt_refusals(K, ctx, solver):
    _, core, _, msg_null, msg_distinct = TABLES[solver]
    L = K.lib()
    E = Entries(L, solver)
    vec = [ctx.empty(N) for _ in core]
    for i in (0, len(core) - 1):                                         # the last vector aliases the first; the first the second
        ptrs = [v.ptr for v in vec]
        ptrs[i] = ptrs[(i + 1) % len(core)]
        rc, _ = E.adopt(ctx, N, ptrs)
        assert rc == -1 and L.khip_last_error() == msg_distinct
    for i in (0, len(core) // 2, len(core) - 1):
        ptrs = [v.ptr for v in vec]
        ptrs[i] = None
        rc, _ = E.adopt(ctx, N, ptrs)
        assert rc == -1 and L.khip_last_error() == msg_null


@pytest.mark.parametrize("solver", sorted(TABLES))
def test_adopt_vector_refusals(K, ctx, solver):
    _, core, lazy, _, _ = TABLES[solver]
    L = K.lib()
    E = Entries(L, solver)
    fn = f"{solver}_workspace_adopt_vector"
    vec = {k: ctx.empty(N) for k in core + lazy}
    spare = ctx.empty(N)
    rc, h = E.adopt(ctx, N, [vec[k].ptr for k in core])
    assert rc == 0
    assert E.fn("workspace_adopt_vector")(h, lazy[0].encode(), vec[lazy[0]].ptr) == 0
    before = E.snapshot(h, core + lazy)
    assert before[0] == (len(core) + 1) * 8 * N
    for k in core:                                                       # a core vector comes with khip_*_workspace_adopt only
        assert E.fn("workspace_adopt_vector")(h, k.encode(), spare.ptr) == -1
        assert L.khip_last_error() == f"{fn}: unknown vector '{k}' ({', '.join(lazy)})".encode()
        assert E.snapshot(h, core + lazy) == before
    assert E.fn("workspace_adopt_vector")(h, b"nope", spare.ptr) == -1
    assert L.khip_last_error() == f"{fn}: unknown vector 'nope' ({', '.join(lazy)})".encode()
    for k in lazy:                                                       # one pointer, one slot
        for c in core:
            assert E.fn("workspace_adopt_vector")(h, k.encode(), vec[c].ptr) == -1
            assert L.khip_last_error() == (f"{fn}: the pointer for '{k}' already is the workspace's '{c}' "
                                           "(every vector needs its own storage)").encode()
            assert E.snapshot(h, core + lazy) == before
    for k in lazy[1:]:                                                   # ... the lazy slots among themselves too
        assert E.fn("workspace_adopt_vector")(h, k.encode(), vec[lazy[0]].ptr) == -1
        assert L.khip_last_error() == (f"{fn}: the pointer for '{k}' already is the workspace's '{lazy[0]}' "
                                       "(every vector needs its own storage)").encode()
        assert E.snapshot(h, core + lazy) == before
    assert E.fn("workspace_adopt_vector")(h, lazy[0].encode(), vec[lazy[0]].ptr) == 0          # the same pointer again: a no-op
    assert E.snapshot(h, core + lazy) == before
    assert E.fn("workspace_adopt_vector")(h, lazy[0].encode(), None) == 0                       # emptying a lazy slot
    assert E.fn("vector")(h, lazy[0].encode()) is None
    assert E.fn("workspace_bytes")(h) == len(core) * 8 * N
    assert E.fn("workspace_adopt_vector")(h, lazy[-1].encode(), None) == 0                      # ... an empty one as well
    assert E.fn("workspace_bytes")(h) == len(core) * 8 * N
    assert E.fn("workspace_destroy")(h) == 0
    K.kfill_(vec[lazy[0]], 1.0)                                          # the emptied slot's vector is still the caller's
    assert K.knorm(N, vec[lazy[0]]) == pytest.approx(N ** 0.5)


@pytest.mark.parametrize("solver", sorted(TABLES))
def test_empty_and_created_workspaces(K, ctx, solver):
    _, core, lazy, _, _ = TABLES[solver]
    E = Entries(K.lib(), solver)
    rc, h = E.adopt(ctx, 0, [None] * len(core))                          # n = 0: nothing to hand over
    assert rc == 0
    assert E.fn("workspace_bytes")(h) == 0
    assert E.fn("workspace_destroy")(h) == 0
    rc, h = E.create(ctx, N)                                             # created and destroyed with no solve between
    assert rc == 0
    assert E.fn("workspace_bytes")(h) == len(core) * 8 * N
    ptrs = [E.fn("vector")(h, k.encode()) for k in core]
    assert None not in ptrs and len(set(ptrs)) == len(core)
    for k in lazy:
        assert E.fn("vector")(h, k.encode()) is None, k
    assert E.fn("workspace_destroy")(h) == 0
    assert E.fn("workspace_destroy")(None) == 0
    assert E.fn("workspace_bytes")(None) == 0 and E.fn("vector")(None, b"x") is None
