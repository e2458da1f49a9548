"""Independent NumPy statement of the library's five in-kernel noise streams (test infrastructure).

Written from the definitions, not from the HIP source:
  * Philox4x32-R (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants):
    a round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
        (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   M0 = 0xD2511F53, M1 = 0xCD9E8D57,
    and the key is bumped by (0x9E3779B9, 0xBB67AE85) between rounds.  uint32 arithmetic through uint64 products.
  * Box-Muller from two whole 32-bit words (a, b):
        u1 = f32(f32(a) 2^-32 + 2^-33)   in (0, 1]   (f32(a): round-to-nearest uint32 -> float32; the sum is exact in float64,
                                                       so one rounding to float32 is the device's single fma)
        u2 = f32(b) 2^-32                in [0, 1] revolutions (exact)
        z0 = sqrt(-2 ln u1) cos(2 pi u2),  z1 = sqrt(-2 ln u1) sin(2 pi u2)   in float64.
    Edges: a >= 0xffffff80 rounds to f32(a) = 2^32, so u1 == 1 and z0 = z1 = 0; a == 0 gives u1 = 2^-33 and the largest radius,
    sqrt(66 ln 2) = 6.76365...  |z| never exceeds that.
  * The stream layouts (include/benchnav_mppi.h): which counter and key each draw comes from.

Everything is generated in chunks of at most CHUNK blocks to bound memory."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_ROUNDS = 8                      # control noise and slip draws
SLIP_KEY_XOR = 0x534C4950              # 'SLIP'
RISK_WORD, ENV_WORD, COLL_WORD = 0x5249534B, 0x454E5631, 0x434F4C4C    # 'RISK', 'ENV1', 'COLL'
OPTIMAL_ROLLOUT = 0xFFFFFFFF
MAX_RADIUS = float(np.sqrt(66.0 * np.log(2.0)))          # a == 0
CHUNK = 1 << 22

_U32 = np.uint32
_MASK = np.uint64(0xFFFFFFFF)


def u32(x):
    """uint32 array of x (Python ints are taken modulo 2^32)."""
    a = np.asarray(x)
    if a.dtype == np.uint32:
        return a
    if a.dtype.kind in "iub":
        return (a.astype(np.uint64) & _MASK).astype(_U32)
    return np.array([int(v) % (1 << 32) for v in a.ravel()], np.uint64).reshape(a.shape).astype(_U32)


def lo32(x):
    return int(x) & 0xFFFFFFFF


def hi32(x):
    return (int(x) >> 32) & 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32-`rounds` of broadcastable uint32 arrays: returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (u32(c).astype(np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = u32(k0).astype(np.uint64), u32(k1).astype(np.uint64)
    m0, m1, w0, w1 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1)
    sh = np.uint64(32)
    for r in range(rounds):
        if r:
            k0 = (k0 + w0) & _MASK
            k1 = (k1 + w1) & _MASK
        p0 = m0 * c0                       # < 2^64: exact
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & _MASK, (p0 >> sh) ^ c3 ^ k1, p0 & _MASK
    return tuple(np.asarray(c, np.uint64).astype(_U32) for c in (c0, c1, c2, c3))


def box_muller_uniforms(a, b):
    """(u1, u2) as float32, exactly as the device forms them."""
    fa = u32(a).astype(np.float32).astype(np.float64)          # round-to-nearest-even conversion
    u1 = (fa * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)      # exact sum, one rounding
    u2 = u32(b).astype(np.float32) * np.float32(2.0 ** -32)     # exact
    return u1, u2


def box_muller(a, b):
    """Two float64 standard normals (z0, z1) from the words (a, b)."""
    u1, u2 = box_muller_uniforms(a, b)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang = 2.0 * np.pi * u2.astype(np.float64)
    return rad * np.cos(ang), rad * np.sin(ang)


def _block_normals(words):
    """(x, y, z, w) -> (n, 4) float64: Box-Muller of (x, y) then of (z, w)."""
    x, y, z, w = words
    a0, a1 = box_muller(x, y)
    b0, b1 = box_muller(z, w)
    return np.stack([a0, a1, b0, b1], -1)


def _chunks(n):
    for s in range(0, n, CHUNK):
        yield s, min(n, s + CHUNK)


# ---- counters ------------------------------------------------------------------
def instance_words(solve, b):
    """Counter words 2 and 3 of the per-rollout streams: (lo(solve) ^ (b << 20), hi(solve) ^ (b >> 12)), i.e. the 64-bit solve
    index xor (b << 20) split in halves.  Hence the documented alias: instance b at solve s uses the counters of instance b' at solve
    s ^ ((b ^ b') << 20)."""
    b = np.asarray(b, np.uint64)
    s = np.asarray(solve, np.uint64)
    c2 = ((s & _MASK) ^ ((b << np.uint64(20)) & _MASK)).astype(_U32)
    c3 = ((s >> np.uint64(32)) ^ (b >> np.uint64(12))).astype(_U32)
    return c2, c3


def rollout_counter(k, j, solve, b):
    """Counter of block j of rollout k (global index) at solve `solve` of instance b: control noise and slip draws alike."""
    c2, c3 = instance_words(solve, b)
    k, j = u32(k), u32(j)
    shape = np.broadcast(k, j, c2).shape
    return tuple(np.broadcast_to(w, shape) for w in (k, j, c2, c3))


def control_key(seed):
    return lo32(seed), hi32(seed)


def slip_key(seed):
    return lo32(seed) ^ SLIP_KEY_XOR, hi32(seed)


# ---- the five streams -------------------------------------------------------------
def eps(seed, solve, b, K, T, k0=0):
    """Control noise of one solve of instance b: (K, T, 2) float64; pair p holds steps 2p and 2p+1, the second half of the last
    pair is dropped when T is odd."""
    npair = (T + 1) // 2
    out = np.empty((K, 2 * npair, 2), np.float64)
    kk, pp = np.divmod(np.arange(K * npair, dtype=np.int64), npair)
    key = control_key(seed)
    flat = out.reshape(K * npair, 4)
    for s, e in _chunks(K * npair):
        words = philox4x32(*rollout_counter(kk[s:e] + k0, pp[s:e], solve, b), *key, rounds=STREAM_ROUNDS)
        flat[s:e] = _block_normals(words)
    return out[:, :T]


def slip(seed, solve, b, K, T, k0=0):
    """Slip draws of one sampled-slip solve of instance b: zt (K, T) transit, zc (K, T+1) cost, zo (T) the optimal rollout's
    transit.  Block j of rollout k: (x, y) -> transit steps 2j, 2j+1, (z, w) -> cost slots 2j, 2j+1; the optimal rollout
    (k = 0xffffffff, no offset) block j -> transit steps 4j .. 4j+3."""
    nS = T // 2 + 1
    blk = np.empty((K * nS, 4), np.float64)
    kk, jj = np.divmod(np.arange(K * nS, dtype=np.int64), nS)
    key = slip_key(seed)
    for s, e in _chunks(K * nS):
        blk[s:e] = _block_normals(philox4x32(*rollout_counter(kk[s:e] + k0, jj[s:e], solve, b), *key, rounds=STREAM_ROUNDS))
    blk = blk.reshape(K, nS, 4)
    zt = blk[:, :, 0:2].reshape(K, 2 * nS)[:, :T]
    zc = blk[:, :, 2:4].reshape(K, 2 * nS)[:, :T + 1]
    nO = (T + 3) // 4
    zo = _block_normals(philox4x32(*rollout_counter(OPTIMAL_ROLLOUT, np.arange(nO), solve, b), *key, rounds=STREAM_ROUNDS)).ravel()[:T]
    return np.ascontiguousarray(zt), np.ascontiguousarray(zc), zo


def risk(seed, cells, n):
    """Risk-map draws (cells, n) float64: sample 4 i4 + s of cell c from block {c, i4, 'RISK', 0}, Philox4x32-10."""
    n4 = (n + 3) // 4
    out = np.empty((cells * n4, 4), np.float64)
    cc, ii = np.divmod(np.arange(cells * n4, dtype=np.int64), n4)
    for s, e in _chunks(cells * n4):
        out[s:e] = _block_normals(philox4x32(cc[s:e], ii[s:e], RISK_WORD, 0, lo32(seed), hi32(seed), rounds=10))
    return out.reshape(cells, 4 * n4)[:, :n]


def env_step(seed, b, step):
    """Slip draw of instance(s) b at env step `step`: the cosine branch of words (x, y) of {b, lo(step), hi(step), 'ENV1'}."""
    x, y, _, _ = philox4x32(b, lo32(step), hi32(step), ENV_WORD, lo32(seed), hi32(seed), rounds=10)
    return box_muller(x, y)[0]


def collision(seed, i, draw):
    """Slip draw of flat position(s) i (= b N + n) of collision check `draw`: the cosine branch of words (x, y) of
    {lo(i), hi(i), lo(draw), 'COLL' ^ hi(draw)}."""
    i = np.asarray(i, np.uint64)
    x, y, _, _ = philox4x32(u32(i & _MASK), u32(i >> np.uint64(32)), lo32(draw), COLL_WORD ^ hi32(draw), lo32(seed), hi32(seed), rounds=10)
    return box_muller(x, y)[0]
