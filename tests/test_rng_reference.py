"""CPU: tests/rng_reference.py, the independent statement of the library's noise streams that tests/test_gpu_noise_streams.py holds
the kernels to -- known answers, a scalar restatement, the Box-Muller edges and the counter layouts."""
import numpy as np
import pytest

import rng_reference as R

MASK = 0xFFFFFFFF

# Random123 known-answer vectors for Philox4x32-10 (kat_vectors): counter, key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def philox_scalar(ctr, key, rounds):
    """Philox4x32 restated on Python ints, one block: the paper's round function and key schedule."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zero", "ones", "pi"])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = tuple(int(w) for w in R.philox4x32(*ctr, *key, rounds=10))
    assert got == want, [hex(w) for w in got]
    assert philox_scalar(ctr, key, 10) == want


@pytest.mark.parametrize("rounds", [1, 7, 8, 10])
def test_vectorised_philox_equals_the_scalar_restatement(rounds):
    rng = np.random.default_rng(rounds)
    w = rng.integers(0, 1 << 32, (6, 300), dtype=np.uint64).astype(np.uint32)
    w[:, :4] = [[0] * 4, [MASK] * 4, [1, MASK, 0, MASK], [MASK, 0, MASK, 1], [0, 0, MASK, MASK], [MASK, MASK, 0, 0]]
    got = np.stack(R.philox4x32(*w, rounds=rounds))
    for i in range(w.shape[1]):
        assert tuple(int(x) for x in got[:, i]) == philox_scalar(tuple(int(x) for x in w[:4, i]), (int(w[4, i]), int(w[5, i])), rounds), (rounds, i)


def test_eight_rounds_is_a_prefix_of_ten_and_differs_from_it():
    """R rounds then the rest: Philox4x32-10 is Philox4x32-8 followed by two rounds under the bumped keys."""
    rng = np.random.default_rng(8)
    w = rng.integers(0, 1 << 32, (6, 1000), dtype=np.uint64).astype(np.uint32)
    eight = R.philox4x32(*w, rounds=8)
    k0 = (w[4].astype(np.uint64) + 8 * R.W0) & R._MASK
    k1 = (w[5].astype(np.uint64) + 8 * R.W1) & R._MASK
    # two more rounds from the eight-round state with the keys bumped eight times
    cont = R.philox4x32(*eight, k0, k1, rounds=2)
    ten = R.philox4x32(*w, rounds=10)
    assert all(np.array_equal(a, b) for a, b in zip(cont, ten))
    assert not np.array_equal(eight[0], ten[0])


def test_box_muller_uniforms_are_the_devices():
    a = np.array([0, 1, 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0x7FFFFFFF, 0xFFFFFF7F, 0xFFFFFF80, MASK], np.uint32)
    u1, u2 = R.box_muller_uniforms(a, a)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    # small words are exact: u1 = (2a + 1) 2^-33
    assert u1[0] == np.float32(2.0 ** -33) and u1[1] == np.float32(3 * 2.0 ** -33) and u1[2] == np.float32(5 * 2.0 ** -33)
    assert ((u1 > 0) & (u1 <= 1)).all() and ((u2 >= 0) & (u2 <= 1)).all()
    # round to nearest: 0xffffff7f -> 0xffffff00 (u1 < 1), 0xffffff80 (a tie) -> 2^32 (u1 = 1 exactly), likewise u2
    assert u1[7] < 1 and u1[8] == 1 and u1[9] == 1
    assert u2[7] == np.float32(0xFFFFFF00 * 2.0 ** -32) and u2[8] == 1 and u2[9] == 1
    # f32(a) 2^-32 + 2^-33 rounded ONCE: compare with a rational computation of the same rounding
    rng = np.random.default_rng(2)
    r = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    u1r, _ = R.box_muller_uniforms(r, r)
    from fractions import Fraction
    for x, u in zip(r[:300], u1r[:300]):
        exact = Fraction(int(np.float32(x))) / (1 << 32) + Fraction(1, 1 << 33)
        # the float64 of `exact` is exact (<= 33 significant bits), so its float32 rounding is the correctly rounded value
        assert Fraction(float(exact)) == exact and u == np.float32(float(exact))
    assert np.array_equal(u1r, (r.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32))


def test_box_muller_edges():
    ones = np.array([0xFFFFFF80, 0xFFFFFFC0, MASK], np.uint32)
    for b in (0, 1 << 30, 1 << 31, 0xC0000000, MASK):
        z0, z1 = R.box_muller(ones, np.full(3, b, np.uint32))
        assert (z0 == 0).all() and (z1 == 0).all()
    z0, z1 = R.box_muller(np.zeros(5, np.uint32), np.array([0, 1 << 30, 1 << 31, 0xC0000000, MASK], np.uint32))
    assert abs(R.MAX_RADIUS - 6.7637056) < 1e-6
    assert np.allclose(np.hypot(z0, z1), R.MAX_RADIUS, rtol=0, atol=1e-12)
    assert np.allclose(z0, R.MAX_RADIUS * np.array([1, 0, -1, 0, 1]), atol=1e-9)     # quarter turns: 0, 1/4, 1/2, 3/4, 1
    assert np.allclose(z1, R.MAX_RADIUS * np.array([0, 1, 0, -1, 0]), atol=1e-9)
    rng = np.random.default_rng(3)
    z = np.concatenate(R.box_muller(rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64), rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)))
    assert np.abs(z).max() <= R.MAX_RADIUS
    assert abs(z.mean()) < 6 / np.sqrt(z.size) and abs(z.var() - 1) < 6 * np.sqrt(2 / z.size)


def _rows(words):
    return np.stack([np.asarray(w, np.uint64).ravel() for w in words], 1)


def _distinct(words):
    rows = _rows(words)
    return len(np.unique(rows, axis=0)) == len(rows)


def test_counter_layout_is_injective_in_rollout_and_pair():
    edges = np.array([0, 1, 2, 63, 64, 1023, 1 << 20, (1 << 31) - 2, (1 << 31) - 1], np.uint64)
    k, p = np.meshgrid(edges, edges, indexing="ij")
    assert _distinct(R.rollout_counter(k, p, 12345, 7))
    # the two words hold k and p themselves: nothing folds them
    c = R.rollout_counter(k, p, 12345, 7)
    assert np.array_equal(c[0], k.astype(np.uint32)) and np.array_equal(c[1], p.astype(np.uint32))


def test_counter_layout_is_injective_in_the_instance():
    """b < 32768 (num_instances' limit) at one solve: every instance has counters of its own."""
    b = np.arange(32768, dtype=np.uint64)
    for s in (0, 1, (1 << 20) - 1, 1 << 20, (1 << 32) + 7, (1 << 64) - 1):
        assert _distinct(R.instance_words(s, b)), s


def test_counter_layout_never_repeats_a_block_of_one_instance():
    """For a fixed instance the solve index maps one-to-one onto (c2, c3): any 64-bit solve, and it can be read back."""
    rng = np.random.default_rng(5)
    s = np.concatenate([rng.integers(0, 1 << 63, 200000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 200000, dtype=np.uint64),
                        np.arange(1 << 16, dtype=np.uint64), np.array([(1 << 64) - 1, 1 << 63, 1 << 32, (1 << 32) - 1], np.uint64)])
    s = np.unique(s)
    for b in (0, 1, 4095, 4096, 32767):
        c2, c3 = R.instance_words(s, b)
        assert _distinct((c2, c3)), b
        back = ((c3.astype(np.uint64) << np.uint64(32)) | c2.astype(np.uint64)) ^ (np.uint64(b) << np.uint64(20))
        assert np.array_equal(back, s), b


def test_cross_instance_alias_is_the_documented_one():
    """A documented property (include/benchnav_mppi.h), asserted so it cannot change silently: instance b at
    solve s draws exactly what instance b' draws at solve s ^ ((b ^ b') << 20) -- and no two instances share a block within 2^20
    consecutive solves."""
    rng = np.random.default_rng(6)
    for _ in range(2000):
        b, b2 = (int(x) for x in rng.integers(0, 32768, 2))
        s = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        s2 = s ^ ((b ^ b2) << 20)
        assert R.instance_words(s, b) == R.instance_words(s2, b2)
        if b != b2:
            assert abs(s - s2) >= 1 << 20
    # the streams themselves, not only the counters
    e1 = R.eps(7, 5, 3, 4, 6)
    assert np.array_equal(e1, R.eps(7, 5 ^ ((3 ^ 1) << 20), 1, 4, 6))
    assert not np.array_equal(e1, R.eps(7, 5, 1, 4, 6))


def test_stream_layouts():
    seed, solve, b = (0xDEADBEEF << 32) | 0x12345678, (1 << 32) + 7, 2
    K, T = 3, 5
    e = R.eps(seed, solve, b, K, T, k0=10)
    assert e.shape == (K, T, 2)
    for k in range(K):
        for p in range((T + 1) // 2):
            w = R.philox4x32(*R.rollout_counter(k + 10, p, solve, b), 0x12345678, 0xDEADBEEF, rounds=8)
            z = np.concatenate([np.ravel(v) for v in (*R.box_muller(w[0], w[1]), *R.box_muller(w[2], w[3]))])
            assert np.array_equal(e[k, 2 * p], z[:2])
            if 2 * p + 1 < T:
                assert np.array_equal(e[k, 2 * p + 1], z[2:])
    # an offset shifts rows; T and T + 1 share their first T steps
    assert np.array_equal(R.eps(seed, solve, b, K + 2, T)[2:], R.eps(seed, solve, b, K, T, k0=2))
    assert np.array_equal(R.eps(seed, solve, b, K, T + 1)[:, :T], R.eps(seed, solve, b, K, T))
    for T_ in (1, 4, 7):
        zt, zc, zo = R.slip(seed, solve, b, K, T_, k0=3)
        assert zt.shape == (K, T_) and zc.shape == (K, T_ + 1) and zo.shape == (T_,)
        for k in range(K):
            for j in range(T_ // 2 + 1):
                w = R.philox4x32(*R.rollout_counter(k + 3, j, solve, b), 0x12345678 ^ R.SLIP_KEY_XOR, 0xDEADBEEF, rounds=8)
                zz = np.concatenate([np.ravel(v) for v in (*R.box_muller(w[0], w[1]), *R.box_muller(w[2], w[3]))])
                for s_ in range(2):
                    if 2 * j + s_ < T_:
                        assert zt[k, 2 * j + s_] == zz[s_]
                    if 2 * j + s_ <= T_:
                        assert zc[k, 2 * j + s_] == zz[2 + s_]
        # the optimal rollout: key 0xffffffff without the offset, four transit draws per block
        w = R.philox4x32(*R.rollout_counter(0xFFFFFFFF, 0, solve, b), 0x12345678 ^ R.SLIP_KEY_XOR, 0xDEADBEEF, rounds=8)
        zz = np.concatenate([np.ravel(v) for v in (*R.box_muller(w[0], w[1]), *R.box_muller(w[2], w[3]))])
        assert np.array_equal(zo[:4], zz[:min(4, T_)])
    # slip key != control key: the same counter gives other draws
    zt, _, _ = R.slip(seed, solve, b, K, 4)
    assert not np.allclose(zt[:, 0:2], R.eps(seed, solve, b, K, 2)[:, 0, :])
    r = R.risk(seed, 5, 7)
    w = R.philox4x32(3, 1, R.RISK_WORD, 0, 0x12345678, 0xDEADBEEF, rounds=10)
    assert r[3, 4] == R.box_muller(w[0], w[1])[0] and r[3, 5] == R.box_muller(w[0], w[1])[1] and r[3, 6] == R.box_muller(w[2], w[3])[0]
    w = R.philox4x32(4, 7, 1, R.ENV_WORD, 0x12345678, 0xDEADBEEF, rounds=10)
    assert R.env_step(seed, 4, (1 << 32) + 7) == R.box_muller(w[0], w[1])[0]
    w = R.philox4x32(9, 2, 11, R.COLL_WORD ^ 3, 0x12345678, 0xDEADBEEF, rounds=10)
    assert R.collision(seed, (2 << 32) + 9, (3 << 32) + 11) == R.box_muller(w[0], w[1])[0]


def test_chunked_generation_equals_one_piece(monkeypatch):
    want = R.eps(3, 9, 1, 37, 9, k0=5)
    zw = R.slip(3, 9, 1, 37, 9, k0=5)
    rw = R.risk(3, 11, 13)
    monkeypatch.setattr(R, "CHUNK", 7)
    assert np.array_equal(R.eps(3, 9, 1, 37, 9, k0=5), want)
    assert all(np.array_equal(a, b) for a, b in zip(R.slip(3, 9, 1, 37, 9, k0=5), zw))
    assert np.array_equal(R.risk(3, 11, 13), rw)


def test_device_hook_rejects_bad_arguments_before_touching_the_device():
    """bn_device_rng_eval (the GPU tests' window on the raw generator): an unknown function or a null pointer is refused, n = 0 is a
    no-op -- all without a device."""
    import ctypes as C
    from benchnav_amd import _capi
    lib = _capi.load()
    p = C.c_void_p(16)
    for fn in (-1, 3):
        assert lib.bn_device_rng_eval(fn, p, p, 1, None) == _capi.BN_ERR_INVALID
    assert lib.bn_device_rng_eval(0, None, p, 1, None) == _capi.BN_ERR_INVALID
    assert lib.bn_device_rng_eval(2, p, None, 1, None) == _capi.BN_ERR_INVALID
    assert lib.bn_device_rng_eval(1, p, p, -1, None) == _capi.BN_ERR_INVALID
    assert lib.bn_device_rng_eval(1, p, p, 0, None) == _capi.BN_OK
