"""GPU: the three evaluation kernels (csrc/eval_kernels.hip) against tests/evaluate_spec.py.

Every integer output -- confusion tables, counts, covered, invalid, ignored, exceed, the 2 x 2 tables -- equals the spec exactly.
Every float64 sum without a logarithm is BIT-EQUAL to the spec: both sides run IEEE float64 add, multiply and divide in the order
evaluate_spec states (the library is built with -ffp-contract=off).  The two sums with a logarithm, KL and NLL, are held to
evaluate_spec.metric_bound: the HIP math API reference (ROCm documentation, "Math API" page, double precision table) gives log a
maximum error of 1 ulp, the spec's own log is within 1 ulp, a term takes at most two more roundings and a sum of n terms at most n
that are not exact: |device - spec| <= (2 + 2 + n) 2^-52 x (the sum of the terms' magnitudes).  The test prints whether they came out
bit-equal; it asserts only the bound.

Shapes, the smallest at which the kernels can go wrong: G = 8 is exactly one wave, 9 a wave and a partial one, 33 crosses the
counting kernels' workgroup step (1024 < 1089), 65 is just above the slab of 4096 cells; M in {1, 2, 5}, C in {1, 4, 10}, bins in
{1, 6}, S in {1, 3}.  The slopes on the bin edges (0, 5, 30, above 30, negative, one float32 step below an edge) sit in cells that
stay valid, apart from the cells made invalid, so that the left-closed edge and both clamps run on the device."""
import functools

import numpy as np
import pytest
import torch

import evaluate_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32

#        G, M, C, NB, S, stuck threshold (0.125: a value float32 holds, so cells sit EXACTLY at it)
CASES = [(8, 1, 1, 1, 1, 0.125), (9, 2, 4, 6, 3, 0.1), (33, 5, 10, 6, 3, 0.125), (65, 2, 10, 1, 1, 0.1), (65, 1, 4, 6, 3, 0.125)]
IDS = ["G8-one-wave", "G9-partial-wave", "G33-M5", "G65-above-a-slab-1bin", "G65-above-a-slab"]
# slopes on the bin edges (closed on the left), one float32 step below an edge, above the range and negative, with their bins at 6 bins over [0, 30]
EDGE_SLOPES = np.array([0.0, 5.0, 30.0, 31.0, -1.0, np.nextafter(f32(5.0), f32(0)), np.nextafter(f32(30.0), f32(0)), 25.0], f32)
EDGE_BINS = [0, 1, 5, 5, 0, 0, 5, 5]
EDGE_CELLS = lambda G: slice(2 * G, 2 * G + len(EDGE_SLOPES))     # G >= 8: one row, apart from every cell made invalid below


@functools.lru_cache(maxsize=None)
def _case(G, M, Cn, NB, Sn, thr):
    """Seeded inputs with every edge the issue lists, and the spec's outputs on them, computed once."""
    rng = np.random.default_rng(1000 * G + 10 * M + Cn)
    cells = G * G
    absent = 2 if Cn > 2 else None                                  # a class that never occurs
    pool = np.array([c for c in range(Cn) if c != absent], np.int32)
    cls = np.empty((M, cells), np.int32)
    for m in range(M):
        if m % 2 == 0:                                                # contiguous patches: bands of rows
            cls[m] = np.repeat(pool[(np.arange(G) * len(pool)) // G], G)
        else:                                                         # i.i.d.
            cls[m] = rng.choice(pool, cells)
    pred = np.where(rng.random((M, cells)) < 0.8, cls, rng.choice(pool, (M, cells))).astype(np.int32)
    m_lat = rng.uniform(0.0, 1.0, (M, cells)).astype(f32)
    s_lat = rng.uniform(0.02, 0.2, (M, cells)).astype(f32)
    mu = (m_lat + rng.normal(0, 0.05, (M, cells))).astype(f32)
    sigma = (s_lat * rng.uniform(0.5, 2.0, (M, cells))).astype(f32)
    phi = rng.uniform(0.0, 30.0, (M, cells)).astype(f32)
    y = (m_lat + s_lat * rng.standard_normal((M, cells))).astype(f32)
    risk = np.clip(mu[None] + sigma[None] * rng.uniform(-1, 2, (Sn, M, cells)), -0.2, 1.2).astype(f32)
    at = f32(1.0) - f32(thr)
    # the invalid cells and y = mu + 2 sigma at the start of every map's LAST row (a partial wave and, at G = 65, the second slab)
    e0 = cells - G
    for m in range(M):
        phi[m, EDGE_CELLS(G)] = EDGE_SLOPES                          # cells of the third row, which stay valid
        sigma[m, e0 + 1] = 0.0
        sigma[m, e0 + 2] = -0.1
        mu[m, e0 + 3] = np.nan
        phi[m, e0 + 4] = np.nan if m % 2 else -1.0
        y[m, e0 + 5], y[m, e0 + 6] = np.inf, -np.inf
        mu[m, e0 + 7], sigma[m, e0 + 7], y[m, e0 + 7] = 0.25, 0.125, 0.5          # y exactly at mu + 2 sigma
        y[m, 0:6] = [at, np.nextafter(at, f32(1)), 0.0, 1.0, 1.5, -0.5]
        risk[:, m, 0:6] = [0.0, 1.0, at, np.nextafter(at, f32(1)), 0.5, 0.0]          # cell 4: believed safe, actually stuck
        risk[0, m, 6], risk[Sn - 1, m, 7] = np.nan, np.inf
        mu[m, 1 + G], sigma[m, 1 + G], y[m, 1 + G] = 0.25, 0.125, 0.0             # y exactly at mu - 2 sigma
        cls[m, 2 + G], cls[m, 3 + G], pred[m, 4 + G] = Cn, -1, Cn + 3             # out of range, negative
        risk[:, m, 5 + G] = y[m, 5 + G]                                        # y == r: not above it
    spec = {"confusion": S.confusion(cls, pred, Cn), "slip": S.slip(mu, sigma, m_lat, s_lat, phi, cls, Cn, y=y, bins=NB, max_slope=30.0),
            "risk": S.risk(risk, y, cls, Cn, thr)}
    data = dict(cls=cls, pred=pred, mu=mu, sigma=sigma, m=m_lat, s=s_lat, phi=phi, y=y, risk=risk)
    return data, spec


def _dev(data, *names):
    return [torch.from_numpy(data[n]).cuda() for n in names]


def _slip(data, Cn, NB, sl=slice(None), with_y=True, **kw):
    from benchnav_amd.evaluate import slip_metrics
    mu, sg, m, s, cls, phi, y = (t[sl] for t in _dev(data, "mu", "sigma", "m", "s", "cls", "phi", "y"))
    out = slip_metrics(mu, sg, m, s, cls, phi, Cn, slips=y if with_y else None, bins=NB, max_slope=30.0, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_confusion_equals_the_spec(case):
    from benchnav_amd.evaluate import confusion_matrix
    G, M, Cn, NB, Sn, thr = case
    data, spec = _case(*case)
    out = confusion_matrix(*_dev(data, "pred", "cls"), Cn)
    table, ignored = out["table"].cpu().numpy(), out["ignored"].cpu().numpy()
    assert table.dtype == np.int64 and table.shape == (M, Cn, Cn)
    assert np.array_equal(table, spec["confusion"][0]) and np.array_equal(ignored, spec["confusion"][1])
    assert (ignored >= 3).all() and (table.sum(axis=(1, 2)) + ignored == G * G).all()
    if Cn > 2:
        assert table[:, 2].sum() == 0 and table[:, :, 2].sum() == 0          # the class that never occurs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_slip_sums_equal_the_spec(case):
    G, M, Cn, NB, Sn, thr = case
    data, spec = _case(*case)
    want = spec["slip"]
    got = _slip(data, Cn, NB)
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["invalid"], want["invalid"])
    assert (got["invalid"] >= 7).all() and (got["counts"][..., 0].sum(axis=(1, 2)) + got["invalid"] == G * G).all()
    assert got["counts"][..., 1].sum() > 0 and (got["counts"][..., 1] <= got["counts"][..., 0]).all()
    # the cells with the slopes on the bin edges are valid, so the edges reach the binning: their bins are the stated ones, and the
    # counts of the groups they fall in hold them (the last bin the slopes 30, 31 and just below 30; bin 1 the slope 5)
    edge = EDGE_CELLS(G)
    e_cls = data["cls"][:, edge]
    assert ((e_cls >= 0) & (e_cls < Cn) & (data["sigma"][:, edge] > 0) & (data["s"][:, edge] > 0)).all()
    assert all(np.isfinite(data[k][:, edge]).all() for k in ("mu", "sigma", "m", "s", "phi", "y"))
    bins = EDGE_BINS if NB == 6 else [0] * len(EDGE_BINS)
    assert S.slope_bin(data["phi"][:, edge], NB, 30.0).tolist() == [bins] * M
    for m in range(M):
        held = np.zeros((Cn, NB), np.int64)
        np.add.at(held, (e_cls[m], bins), 1)
        assert (got["counts"][m, :, :, 0] >= held).all() and held[:, NB - 1].sum() == (4 if NB == 6 else len(bins))
    for k, name in enumerate(S.SUM_NAMES):
        if k in S.LOG_SUMS:
            n = want["counts"][..., 0]
            err, bound = np.abs(got["sums"][..., k] - want["sums"][..., k]), S.metric_bound(want["magnitude"][..., S.LOG_SUMS.index(k)], n)
            print(f"{IDS[CASES.index(case)]}: sum {name}: bit-equal {_same_bits(got['sums'][..., k], want['sums'][..., k])}, "
                  f"max |device - spec| {err.max():.3g}, max over the bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert (err <= bound).all(), f"{name} off by {err.max():.3g} (bound {bound[np.unravel_index(np.argmax(err - bound), err.shape)]:.3g})"
        else:
            assert _same_bits(got["sums"][..., k], want["sums"][..., k]), f"sum {name} differs from the spec's bits"
    # without observations: the same first six sums, the last two and `covered` stay 0, the two cells with y = +-inf count
    bare = _slip(data, Cn, NB, with_y=False)
    assert _same_bits(bare["sums"][..., :5], S.slip(data["mu"], data["sigma"], data["m"], data["s"], data["phi"], data["cls"], Cn, bins=NB)["sums"][..., :5])
    assert not bare["sums"][..., 6:].any() and not bare["counts"][..., 1].any() and (bare["invalid"] == want["invalid"] - 2).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_risk_counts_equal_the_spec(case):
    from benchnav_amd.evaluate import risk_calibration
    G, M, Cn, NB, Sn, thr = case
    data, spec = _case(*case)
    out = risk_calibration(*_dev(data, "risk", "y", "cls"), Cn, stuck_threshold=thr)
    counts, invalid = out["counts"].cpu().numpy(), out["invalid"].cpu().numpy()
    assert counts.shape == (M, Sn, Cn, S.RISK_COUNTS) and counts.dtype == np.int64
    assert np.array_equal(counts, spec["risk"][0]) and np.array_equal(invalid, spec["risk"][1])
    assert (counts[..., 1:].sum(axis=(2, 3)) + invalid == G * G).all() and (invalid >= 4).all() and (invalid[:, 0] >= 5).all()
    assert counts[..., 2].sum() > 0 and counts[..., 0].sum() > 0


def test_slopes_on_the_bin_edges():
    """Nothing but the edge slopes, every cell valid: the device's counts per bin are the hand-counted ones.  Then every edge
    5, 10, ..., 30 with the float32 below and above it, in float64 bins: 5 k is in bin k, the float32 below it in bin k - 1."""
    n = len(EDGE_SLOPES)
    full = lambda v, k=n: np.full((1, k), v, f32)
    data = dict(mu=full(0.5), sigma=full(0.1), m=full(0.4), s=full(0.2), phi=EDGE_SLOPES[None].copy(), y=full(0.45), cls=np.zeros((1, n), np.int32))
    got = _slip(data, 1, 6)
    assert got["counts"][0, 0, :, 0].tolist() == np.bincount(EDGE_BINS, minlength=6).tolist() == [3, 1, 0, 0, 0, 4] and got["invalid"][0] == 0
    assert _slip(data, 1, 1)["counts"][0, 0, :, 0].tolist() == [n]
    edges = np.arange(1, 7, dtype=f32) * f32(5.0)
    phi = np.concatenate([np.nextafter(edges, f32(0)), edges, np.nextafter(edges, f32(100))])[None]
    want = np.concatenate([np.arange(0, 6), np.minimum(np.arange(1, 7), 5), np.minimum(np.arange(1, 7), 5)])
    data = dict(mu=full(0.5, 18), sigma=full(0.1, 18), m=full(0.4, 18), s=full(0.2, 18), phi=phi, y=full(0.45, 18), cls=np.zeros((1, 18), np.int32))
    assert S.slope_bin(phi, 6, 30.0).tolist() == [want.tolist()]
    assert _slip(data, 1, 6)["counts"][0, 0, :, 0].tolist() == np.bincount(want, minlength=6).tolist() == [1, 3, 3, 3, 3, 5]


def test_all_cells_in_one_group():
    G, Cn, NB = 9, 4, 6
    rng = np.random.default_rng(5)
    shape = (1, G * G)
    data = dict(mu=rng.uniform(0, 1, shape).astype(f32), sigma=np.full(shape, 0.1, f32), m=rng.uniform(0, 1, shape).astype(f32),
                s=np.full(shape, 0.2, f32), phi=np.full(shape, 12.5, f32), y=rng.uniform(0, 1, shape).astype(f32), cls=np.full(shape, 3, np.int32))
    got = _slip(data, Cn, NB)
    want = S.slip(data["mu"], data["sigma"], data["m"], data["s"], data["phi"], data["cls"], Cn, y=data["y"], bins=NB)
    assert got["counts"][0, 3, 2, 0] == G * G and got["counts"][..., 0].sum() == G * G and got["invalid"][0] == 0
    keep = [k for k in range(S.SUMS) if k not in S.LOG_SUMS]
    assert _same_bits(got["sums"][..., keep], want["sums"][..., keep])
    assert (np.abs(got["sums"] - want["sums"])[0, 3, 2, list(S.LOG_SUMS)] <= S.metric_bound(want["magnitude"][0, 3, 2], G * G)).all()


def test_a_map_s_tables_do_not_depend_on_the_batch():
    """The same M = 5 maps in one call, in calls of 1 + 4 and 2 + 3 maps, and embedded in a larger batch: bit-identical per-map
    tables, the log sums included (the same device code on the same inputs); two runs give the same bits; the running total of
    split calls is the one call's."""
    case = CASES[2]
    G, M, Cn, NB, Sn, thr = case
    data, _ = _case(*case)
    whole = _slip(data, Cn, NB)
    again = _slip(data, Cn, NB)
    for k in whole:
        assert np.array_equal(whole[k].view(np.int64), again[k].view(np.int64)), k
    for cut in (1, 2):
        a, b = _slip(data, Cn, NB, slice(0, cut)), _slip(data, Cn, NB, slice(cut, M))
        for k in whole:
            assert np.array_equal(np.concatenate([a[k], b[k]]).view(np.int64), whole[k].view(np.int64)), (cut, k)
    order = [3, 0, 1, 2, 3, 4, 1]                                     # the five maps behind one and in front of another
    big = {k: v[order] for k, v in data.items() if k != "risk"}
    emb = _slip(big, Cn, NB)
    for k in whole:
        assert np.array_equal(emb[k][1:6].view(np.int64), whole[k].view(np.int64)), k
    # the running total: zeros + map 0 + map 1 + ... in map order, whatever the split
    zeros = lambda: torch.zeros(Cn, NB, S.SUMS, device="cuda", dtype=torch.float64)
    one = zeros()
    _slip(data, Cn, NB, total=one)
    assert _same_bits(one.cpu().numpy(), S.slip_total(whole["sums"]))
    for cut in (1, 2):
        two = zeros()
        _slip(data, Cn, NB, slice(0, cut), total=two)
        _slip(data, Cn, NB, slice(cut, M), total=two)
        assert _same_bits(two.cpu().numpy(), one.cpu().numpy()), cut
    # the counting kernels, split and whole
    from benchnav_amd.evaluate import confusion_matrix, risk_calibration
    pred, cls, risk, y = _dev(data, "pred", "cls", "risk", "y")
    assert torch.equal(torch.cat([confusion_matrix(pred[:2], cls[:2], Cn)["table"], confusion_matrix(pred[2:], cls[2:], Cn)["table"]]),
                       confusion_matrix(pred, cls, Cn)["table"])
    assert torch.equal(torch.cat([risk_calibration(risk[:, :2], y[:2], cls[:2], Cn, thr)["counts"],
                                  risk_calibration(risk[:, 2:], y[2:], cls[2:], Cn, thr)["counts"]]), risk_calibration(risk, y, cls, Cn, thr)["counts"])
