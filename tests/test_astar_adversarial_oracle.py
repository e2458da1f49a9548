"""CPU: the A* field oracle (tests/astar_oracle.py) on the adversarial maps of tests/astar_maps.py, against an independent
float64 shortest path (scipy) and an oracle-free fixpoint certificate -- and the certificate rejects fields that are subtly
wrong, so the GPU tests that lean on it (test_gpu_astar_stress.py) can trust it."""
import numpy as np
import pytest

import astar_maps as M
import astar_oracle as A

NAMES = sorted(M.CASES)
_SOLVED = {}


def _solved(name):
    if name not in _SOLVED:
        h, r, thr, res, g = M.CASES[name]
        _SOLVED[name] = A.solve(h, r, thr, res, g)
    return _SOLVED[name]


@pytest.mark.parametrize("name", [n for n in NAMES if n not in M.NO_F64])
def test_oracle_equals_float64_shortest_path(name):
    D, nxt = _solved(name)
    assert np.isfinite(D).any(), f"{name}: the goal reaches nothing; the case tests nothing"
    assert A.check_f64(*M.CASES[name], D, nxt) == "", name


@pytest.mark.parametrize("name", NAMES)
def test_certificate_accepts_the_oracle(name):
    h, r, thr, res, g = M.CASES[name]
    D, nxt = _solved(name)
    assert A.certify_field(h, r, thr, res, g, D) == "", name
    assert np.array_equal(A.next_hops(h, D, g, res), nxt)


@pytest.mark.parametrize("name", [n for n in NAMES if M.size(n) <= 128 * 128])
def test_dijkstra_equals_relaxation(name):
    h, r, thr, res, g = M.CASES[name]
    assert np.array_equal(_solved(name)[0].view(np.uint32), A.field_relax(h, r, thr, res, g).view(np.uint32)), name


def test_maps_hit_what_they_aim_at():
    free = lambda n: A.free_mask(M.CASES[n][1], M.CASES[n][2])  # noqa: E731
    reach = lambda n: np.isfinite(_solved(n)[0])  # noqa: E731
    assert reach("zipper").sum() == free("zipper").sum() == 128
    assert A.hop_counts(_solved("zipper")[1])[free("zipper")].max() == 127
    frac = reach("corner_gate").sum() / free("corner_gate").sum()
    assert 0.5 < frac < 0.55, frac                                # the oracle reaches 52 % of the free cells from (5, 5)
    assert A.hop_counts(_solved("spiral")[1]).max() > 192 * 192 * 0.45
    for s in range(3):
        n = f"percolation{s}"
        blocked = 1 - free(n).mean()
        assert 0.53 < blocked < 0.57 and 0.2 < reach(n).sum() / free(n).sum() < 0.999, (n, blocked)
    h, r, thr = M.CASES["thr_nan"][:3]
    assert 0.15 < (r == np.float32(thr)).mean() < 0.25 and 0.15 < np.isnan(r).mean() < 0.25
    assert np.isinf(_solved("thr_nan")[0][r == np.float32(thr)]).all() and reach("thr_nan")[np.isnan(r)].mean() > 0.9
    w = A.weights(*M.CASES["wide_weights"][0:4:3])
    w = w[np.isfinite(w)]
    assert w.min() < 0.06 and w.max() > 45
    h = M.CASES["nonfinite_heights"][0]
    assert np.isnan(h).any() and np.isposinf(h).any() and reach("nonfinite_heights").mean() > 0.5
    tiles = {(-(-M.CASES[n][0].shape[0] // 32), -(-M.CASES[n][0].shape[1] // 32)) for n in NAMES if n.startswith("shape")}
    assert (1, 1) in tiles and (4, 1) in tiles and (2, 3) in tiles


# ---- the checkers bite: mutants of a correct field ---------------------------------------------------------------------
MUT = "percolation0"


def _field():
    h, r, thr, res, g = M.CASES[MUT]
    D, nxt = _solved(MUT)
    return h, r, thr, res, g, D.copy(), nxt.copy()


def _reached_cell(D, g, k=0):
    fin = np.argwhere(np.isfinite(D) & (D > 0))
    y, x = fin[len(fin) // 3 + k]
    return int(y), int(x)


@pytest.mark.parametrize("sign", [1, -1])
def test_certificate_rejects_one_ulp(sign):
    h, r, thr, res, g, D, _ = _field()
    y, x = _reached_cell(D, g)
    D[y, x] = np.nextafter(D[y, x], np.float32(sign * np.inf))
    assert A.certify_field(h, r, thr, res, g, D) != ""


def test_certificate_rejects_a_value_on_an_unreachable_cell():
    h, r, thr, res, g, D, _ = _field()
    free = A.free_mask(r, thr)
    for where in (free & np.isinf(D), ~free):                  # a free cell of another component, a collision cell
        y, x = np.argwhere(where)[0]
        E = D.copy()
        E[y, x] = np.float32(1e6)
        assert A.certify_field(h, r, thr, res, g, E) != ""


def test_certificate_rejects_inf_on_a_reachable_cell_and_a_nonzero_goal():
    h, r, thr, res, g, D, _ = _field()
    E = D.copy()
    E[_reached_cell(D, g)] = np.inf
    assert A.certify_field(h, r, thr, res, g, E) != ""
    E = D.copy()
    E[g[1], g[0]] = np.float32(2.0 ** -30)
    assert A.certify_field(h, r, thr, res, g, E) != ""
    assert A.certify_field(h, r, thr, res, (g[0] + 1, g[1]), D) != ""      # the field of another goal


def test_next_check_rejects_a_later_equal_cost_direction():
    """On a flat map with no obstacles many cells have two minimising directions; the first in DIRS order is the answer."""
    h = np.zeros((40, 40), np.float32)
    r = np.full((40, 40), 0.9, np.float32)
    g = (20, 20)
    D, nxt = A.solve(h, r, 0.2, 0.5, g)
    assert A.certify_field(h, r, 0.2, 0.5, g, D) == ""
    w = A.weights(h, 0.5)
    found = 0
    for y in range(40):
        for x in range(40):
            if (x, y) == g:
                continue
            c = [w[d, y, x] + (D[y + dy, x + dx] if 0 <= x + dx < 40 and 0 <= y + dy < 40 else np.inf)
                 for d, (dx, dy) in enumerate(A.DIRS)]
            ties = [d for d in range(8) if c[d] == min(c)]
            if len(ties) > 1:
                assert nxt[y, x] == ties[0]
                bad = nxt.copy()
                bad[y, x] = ties[1]
                assert not np.array_equal(A.next_hops(h, D, g, 0.5), bad)
                assert A.hop_counts(bad)[y, x] >= 0              # a valid walk all the same: only the direction rule sees it
                found += 1
    assert found > 10


def test_next_check_rejects_a_hop_into_a_collision_cell():
    h, r, thr, res, g, D, nxt = _field()
    free = A.free_mask(r, thr)
    for y, x in np.argwhere(free & np.isfinite(D))[::97]:
        for d, (dx, dy) in enumerate(A.DIRS):
            if 0 <= x + dx < D.shape[1] and 0 <= y + dy < D.shape[0] and not free[y + dy, x + dx]:
                bad = nxt.copy()
                bad[y, x] = d
                assert not np.array_equal(A.next_hops(h, D, g, res), bad)
                return
    raise AssertionError("no free reached cell next to a collision cell")


def test_f64_check_rejects_a_field_that_is_off_by_more_than_rounding():
    h, r, thr, res, g, D, nxt = _field()
    assert A.check_f64(h, r, thr, res, g, D, nxt) == ""
    E = D.copy()
    y, x = _reached_cell(D, g)
    E[y, x] *= np.float32(1 + 2.0 ** -12)
    assert A.check_f64(h, r, thr, res, g, E, nxt) != ""
    E = D.copy()
    E[y, x] = np.inf
    assert A.check_f64(h, r, thr, res, g, E, nxt) != ""


# ---- absorption: a cost near 2^24 x an edge weight ---------------------------------------------------------------------
def test_plateau_walk_never_ends_and_says_so():
    """fl32(1 + D) == D on the low side of a 4e7 m cliff: the next-hop map holds 2-cycles.  The limit is loud, never a path."""
    h, r, thr, res, g = M.CASES["plateau"]
    D, nxt = _solved("plateau")
    assert np.isfinite(D).all() and A.certify_field(h, r, thr, res, g, D) == ""
    assert list(nxt[0, :2]) == [1, 0]                          # (0, 0) -> (1, 0) -> (0, 0)
    with pytest.raises(RuntimeError, match="cycle"):
        A.hop_counts(nxt)
    with pytest.raises(RuntimeError, match="exceeded"):
        A.walk(nxt, (0, 0))
    assert A.walk(nxt, (12, 0)) is not None                    # the high side is below the absorption limit
