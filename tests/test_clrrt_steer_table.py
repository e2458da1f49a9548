"""CPU: the steer table of tests/clrrt_steer_cases.py, proved with the spec alone to be what tests/test_gpu_clrrt_steer.py relies on,
so that a leave-out on the GPU can never hide a failure: no case in the double-rounding band, at most 2 % of a group
truncation-marginal or cast-sensitive, the boundary cases' words and point counts as written down, and `M32` unchanged.  Then the
new comparisons' teeth: a float32 round trip of the points and a turning centre moved by one float32 ulp fail them and pass the
old 5e-6 m / 1e-4 bounds.  No GPU.

Counts of the table as committed (644 steers, printed per group by test_group_meets_the_caps): band 0 everywhere;
truncation-marginal 1 of 70 in either boundaries group (the same pose at heading 0: total 0), 0 elsewhere; cast-sensitive 0 in
every other group.  The cast-sensitive cap is held on the cases that are not *aligned* (clrrt_steer_cases.aligned): a straight path
ahead of the rover makes the angular error cancel to below 2^-20, where a 2^-48 nudge of the bearing shows in the float32 cast by
construction -- 14 of 70 boundary cases (straight ahead with equal headings and their kin, which the table has to hold).  Every
cast-sensitive case of the table is such a one; among the others the count is 0, against the 2 % cap."""
import math

import numpy as np
import pytest

import clrrt_cases as Cs
import clrrt_spec as S
import clrrt_steer_cases as T

f32 = np.float32
OLD_POINT_TOL, OLD_COST_REL = 5e-6, 1e-6          # tests/test_gpu_clrrt.py


# ---- composition -----------------------------------------------------------------------------------------------------------------
def test_table_has_about_600_steers_in_small_groups():
    gs = T.groups()
    assert 550 <= sum(len(g) for g in gs.values()) <= 700
    assert all(1 <= len(g) <= 70 and g.from_states.dtype == g.targets.dtype == g.ctrls.dtype == np.float32 for g in gs.values())
    assert all(np.isfinite(g.from_states).all() and np.isfinite(g.targets).all() for g in gs.values())
    for g in gs.values():                            # inside the map
        assert (g.from_states[:, :2] >= 0).all() and (g.from_states[:, :2] <= 32).all() and (g.targets[:, :2] >= 0).all() and (g.targets[:, :2] <= 32).all()
    a, b = T.risk_map("A"), T.risk_map("B")
    assert a.shape == b.shape == (64, 64) and (b < 0).any() and (b > 1).any() and (b[40:44] == f32(0.95)).all() and (b[8:16, 40:48] >= 1).all()


def test_random_group_reaches_every_word_and_both_outcomes():
    """256 steers: at least 23 of each word per 300 (20 of 256), and most but not all feasible (248: the recipe on plan 0's map
    gives 97 %, not the 85 % the issue estimated; the infeasible ones are the steers into its stuck region)."""
    sp = [c for k in range(4) for c in T.spec(f"random_{k}")]
    g = [T.groups()[f"random_{k}"] for k in range(4)]
    assert len(sp) == 256 and all(gr.delta == 5.0 and gr.max_seqs == 250 and (gr.ctrls[:, [1, 3]] != 0).all() for gr in g)
    words = np.bincount([c.steer.word for c in sp], minlength=6)
    feasible = sum(c.steer.feasible for c in sp)
    print("words", dict(zip(S.WORDS, words.tolist())), "feasible", feasible, "of 256")
    assert (words * 300 >= 23 * 256).all(), words
    assert 0.75 * 256 <= feasible <= 256 - 5


def test_path_length_groups():
    g, sp = T.groups()["long_d12"], T.spec("long_d12")
    assert g.delta == 12.0
    assert all(c.steer.word >= 4 for c in sp[:16])                                          # all-arc paths
    assert all(c.total >= 16.0 and math.ceil(c.total / 0.25) >= 64 for c in sp[16:])         # the 64 cap
    assert max(len(c.steer.path) for c in sp) >= 49                                          # 12 m of 0.25 segments
    assert all(len(c.steer.path) == 1 and c.steer.length == 1 and c.steer.feasible for c in T.spec("short_d02"))
    assert all(len(c.steer.path) <= 2 for c in T.spec("short_d025")) and all(len(c.steer.path) <= 3 for c in T.spec("short_d05"))
    assert T.groups()["short_d025"].delta == 0.25 and T.groups()["short_d05"].delta == 0.5


def test_max_seqs_groups_end_on_the_last_permitted_step_and_one_short_of_it():
    names = [n for n in T.groups() if n.startswith("maxseqs_") and "_at_" in n]
    assert len(names) == 8
    for n in names:
        i, L = int(n.split("_")[1]), int(n.split("_")[3])
        at, below = T.spec(n)[i].steer, T.spec(f"maxseqs_{i}_below_{L}")[i].steer
        assert T.groups()[n].max_seqs == L and at.feasible and at.length == L
        assert T.groups()[f"maxseqs_{i}_below_{L}"].max_seqs == L - 1 and not below.feasible and below.length == L - 1
    assert T.groups()["maxseqs_1"].max_seqs == 1 and all(c.steer.length == 1 for c in T.spec("maxseqs_1"))


def test_edge_group_clamps_creeps_and_stands_still():
    g, sp = T.groups()["edges_B"], T.spec("edges_B")
    for i in range(8):                               # one step from a limit, heading outward: slot 0 lies outside, the clean state on the limit
        st = sp[i].steer.states
        assert ((st[0, :2] > 32) | (st[0, :2] < 0)).any() and (st[-1, :2] >= 0).all() and (st[-1, :2] <= 32).all(), (i, st[0])
    for i in range(8, 12):                           # on the stripe: +1e4 on the first step at least
        assert sp[i].steer.cost >= 1e4
    for i in range(12, 15):                          # inside the block: max_seqs steps, infeasible, every state equal
        st = sp[i].steer
        assert not st.feasible and st.length == g.max_seqs and (st.states == st.states[0]).all() and st.cost >= 1e4 * g.max_seqs
    assert any(not sp[i].steer.feasible for i in range(15, 19))                              # the stripe stops some of them


# ---- the caps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.group_names())
def test_group_meets_the_caps(name):
    sp, n = T.spec(name), len(T.groups()[name])
    band = [i for i, c in enumerate(sp) if c.band]
    trunc = [i for i, c in enumerate(sp) if c.truncation_marginal]
    cast = [i for i in range(n) if T.cast_sensitive(name, i)]
    unaligned = [i for i in cast if not T.aligned(name, i)]
    print(f"{name}: {n} steers; band {len(band)}; cast-sensitive {len(cast)} (of them not aligned {len(unaligned)}); truncation-marginal {len(trunc)}")
    assert not band, band
    assert len(trunc) <= T.CAP * n, trunc
    assert len(unaligned) <= T.CAP * n, unaligned
    assert len(unaligned) < 10                       # more means the nudge is wired wrongly


def test_no_nudge_is_bit_identical_and_a_nudge_reaches_the_errors():
    g = T.groups()["random_0"]
    cfg = T.config(g)
    st = T.spec("random_0")[0].steer
    same = S.follow(cfg, g.from_states[0], g.ctrls[0], st.path, st.word, nudge=None)
    assert not T.steers_differ(st, same) and same.ctrl.tobytes() == st.ctrl.tobytes()
    zero = S.follow(cfg, g.from_states[0], g.ctrls[0], st.path, st.word, nudge=(0.0, 0.0))
    assert not T.steers_differ(st, zero) and zero.ctrl.tobytes() == st.ctrl.tobytes()
    big = S.follow(cfg, g.from_states[0], g.ctrls[0], st.path, st.word, nudge=(1e-3, 1e-3))
    assert big.actions[0, 0] > st.actions[0, 0] and big.actions[0, 1] > st.actions[0, 1]
    far = S.follow(cfg, g.from_states[0], g.ctrls[0], st.path, st.word, nudge=(0.0, 2.0))        # the validity test sees it too
    assert far.targets[0] != st.targets[0] or far.targets[0] == len(st.path) - 1


# ---- the boundary literals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boundaries_d5", "boundaries_d12"])
def test_boundary_words_and_point_counts_are_the_written_ones(name):
    g, sp, names = T.groups()[name], T.spec(name), T.boundary_names()
    assert len(g.expect) == len(sp) == len(names)
    for i, (c, want) in enumerate(zip(sp, g.expect)):
        assert (c.steer.word, len(c.steer.path)) == want, (names[i], S.WORDS[c.steer.word], len(c.steer.path), want)
    for i, nm in enumerate(names):
        if nm.startswith("straight ahead") and nm.endswith("@ 0.0"):
            assert sp[i].steer.word == 0, nm                                                # four words tie at most; the first wins


def test_straight_ahead_literals():
    """Straight ahead gives LSL; two metres ahead on dyadic coordinates RSL comes to 1.9999999 against LSL's 2.0 and wins."""
    for d in (0.25, 0.5, 1.0, 5.0, 20.0):
        opts = S.all_options(f32([8, 8, 0]), f32([8 + d, 8, 0]), S.M64R)
        assert S.choose_word(opts) == 0 and opts[0][0] == opts[1][0] == f32(d), d
    opts = S.all_options(f32([8, 8, 0]), f32([10, 8, 0]), S.M64R)
    assert opts[0][0] == f32(2.0) and opts[2][0] == f32(1.9999999) == np.nextafter(f32(2), f32(0)) and S.choose_word(opts) == 2
    # the half centre distance exactly 1: RSL exists, of length pi (two quarter turns and no straight); one ulp below it does not
    at = S.all_options(f32([12, 14, 0]), f32([14, 12, 0]), S.M64R)
    below = S.all_options(f32([12, 14, 0]), f32([np.nextafter(f32(14), f32(0)), 12, 0]), S.M64R)
    assert at[2][0] == f32(f32(S.HALF_PI32 + S.HALF_PI32) + f32(0)) and at[2][1][2] == 0 and math.isinf(below[2][0])
    # centre distances exactly 2 and 4 (the table's construction: left centres at (0, 14) and (d, 14)): LRL exists at both ends of
    # its range and not one ulp beyond; at 4 it ties with RSL at f32(pi), and RSL, the earlier word, wins
    for d, exists in ((np.nextafter(f32(2), f32(0)), False), (f32(2), True), (np.nextafter(f32(2), f32(3)), True),
                      (np.nextafter(f32(4), f32(0)), True), (f32(4), True), (np.nextafter(f32(4), f32(5)), False)):
        o = S.all_options(f32([1, 14, S.HALF_PI32]), f32([d - f32(1), 14, f32(1.5 * math.pi)]), S.M64R)
        assert math.isfinite(float(o[5][0])) == exists, d
    o = S.all_options(f32([1, 14, S.HALF_PI32]), f32([3, 14, f32(1.5 * math.pi)]), S.M64R)
    assert o[2][0] == o[5][0] == S.PI32 and S.choose_word(o) == 2


# ---- M32 and M64R ----------------------------------------------------------------------------------------------------------------
def test_m32_is_what_it_was_and_m64r_is_the_float64_function_rounded():
    rng = np.random.default_rng(3)
    for inter in np.concatenate([f32([2.0, 4.0, 3.9999998, 2.0000002]), rng.uniform(2, 4, 200).astype(f32)]):
        assert S.M32.mid_height(inter).tobytes() == f32((f32(4) - (inter / f32(2)) ** 2) ** 0.5).tobytes()
        hi = f32(inter * f32(0.5))
        assert S.M64R.mid_height(inter).tobytes() == np.sqrt(f32(f32(4) - hi * hi)).tobytes()
    assert S.M32.cos is np.cos and S.M32.arctan2 is np.arctan2 and S.M32.sqrt is np.sqrt and S.M64R.sqrt is np.sqrt
    for v in rng.uniform(-7, 7, 200).astype(f32):
        assert S.M64R.cos(v) == f32(math.cos(float(v))) and S.M64R.sin(v) == f32(math.sin(float(v))) and isinstance(S.M64R.cos(v), np.float32)
        assert S.M64R.arctan2(v, f32(1.5)) == f32(math.atan2(float(v), 1.5))
    for v in rng.uniform(-1, 1, 200).astype(f32):
        assert S.M64R.arccos(v) == f32(math.acos(float(v))) and S.M64R.arcsin(v) == f32(math.asin(float(v)))
    # the default of every helper is still M32
    s, e = f32([4.0, 4.0, 0.3]), f32([9.0, 11.0, 2.0])
    assert S.reference_path(s, e, 5.0)[0].tobytes() == S.reference_path(s, e, 5.0, S.M32)[0].tobytes()
    cfg = Cs.spec_config(0)
    assert S.steer_is_marginal(cfg, s, np.zeros(4, f32), e, eps=1e-9) == S.steer_is_marginal(cfg, s, np.zeros(4, f32), e, eps=1e-9, m=S.M32)
    assert S.steer_is_marginal(cfg, f32([4.0, 4.0, 0.0]), np.zeros(4, f32), f32([12.0, 4.0, 0.0]), eps=1e-6, m=S.M64R)


def test_rounding_margin_and_the_instrumented_namespace():
    v = f32(1.2345)
    mid = (float(v) + float(np.nextafter(v, f32(2)))) / 2
    assert S.rounding_margin(mid) == 0.0 and S.rounding_margin(float(v)) == pytest.approx(2.0 ** -24 / float(v))
    assert S.rounding_margin(mid * (1 + 2.0 ** -46)) < S.DOUBLE_ROUNDING_BAND < S.rounding_margin(mid * (1 + 2.0 ** -40))
    assert S.rounding_margin(0.0) == math.inf
    m, margins = S.instrumented_m64r()
    s, e = f32([4.0, 4.0, 0.3]), f32([9.0, 11.0, 2.0])
    got = S.reference_path(s, e, 5.0, m)
    want = S.reference_path(s, e, 5.0, S.M64R)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and len(margins) >= 20 and min(margins) > S.DOUBLE_ROUNDING_BAND


# ---- teeth -----------------------------------------------------------------------------------------------------------------------
def _fails(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


def _teeth(name, moved):
    """`moved`: per case the spec's steer on perturbed points.  Two devices are fed to the comparisons: one that reports the moved
    points (the Dubins half is wrong), one that reports the right points and followed the moved ones (the follow half is wrong)."""
    g, sp = T.groups()[name], T.spec(name)
    cfg = T.config(g)
    same = [i for i in range(len(g)) if moved[i].word == sp[i].steer.word and len(moved[i].path) == len(sp[i].steer.path)]
    assert len(same) >= 0.9 * len(g)
    wrong_points = T.as_device(moved, g.max_seqs)
    wrong_follow = T.as_device(moved, g.max_seqs)
    wrong_follow["path"] = T.as_device([c.steer for c in sp], g.max_seqs)["path"]
    honest = T.as_device([c.steer for c in sp], g.max_seqs)
    reached = new_a = new_b = old = 0
    for i in same:
        assert T.check_dubins(honest, i, sp[i]) == (0.0, 0.0) and T.follow_mismatch(honest, i, T.follow_on_device_points(cfg, g, honest, i)) is None
        shift = float(np.abs(moved[i].path - sp[i].steer.path).max())
        if shift == 0.0:
            continue                                 # the perturbation did not reach this path (the centre it moved is another word's)
        reached += 1
        new_a += _fails(T.check_dubins, wrong_points, i, sp[i])
        new_b += T.follow_mismatch(wrong_follow, i, T.follow_on_device_points(cfg, g, wrong_follow, i)) is not None
        old += shift <= OLD_POINT_TOL and T.loose_follow_ok(wrong_points, i, sp[i].steer, OLD_COST_REL)
    assert reached >= 0.9 * len(same)
    return reached, new_a, new_b, old


def test_a_float32_round_trip_of_the_points_fails_the_new_bounds_and_passes_the_old():
    g, sp = T.groups()["random_0"], T.spec("random_0")
    cfg = T.config(g)
    moved = [S.follow(cfg, g.from_states[i], g.ctrls[i], c.steer.path.astype(np.float32).astype(np.float64), c.steer.word) for i, c in enumerate(sp)]
    n, new_a, new_b, old = _teeth("random_0", moved)
    print(f"float32 round trip: {n} cases; fail the point bound {new_a}; fail the bit comparison {new_b}; pass the old bounds {old}")
    assert new_a == n and new_b >= 0.95 * n and old >= 0.98 * n


def test_a_turning_centre_moved_by_one_float32_ulp_fails_the_new_bounds_and_passes_the_old(monkeypatch):
    g, sp = T.groups()["random_0"], T.spec("random_0")
    cfg = T.config(g)
    centre = S.find_center

    def off_by_an_ulp(p, left, m=S.M32):
        c = centre(p, left, m)
        c[0] = np.nextafter(c[0], f32(np.inf))
        return c
    monkeypatch.setattr(S, "find_center", off_by_an_ulp)
    moved = [S.steer(cfg, g.from_states[i], g.ctrls[i], g.targets[i], S.M64R) for i in range(len(g))]
    monkeypatch.undo()
    n, new_a, new_b, old = _teeth("random_0", moved)
    print(f"centre + 1 ulp: {n} cases; fail the point bound {new_a}; fail the bit comparison {new_b}; pass the old bounds {old}")
    assert new_a >= 0.95 * n and new_b >= 0.9 * n and old >= 0.95 * n
