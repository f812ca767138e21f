"""TEST INFRASTRUCTURE: numpy twin of csrc/noise.h, the per-step random state noise and base wrench
of the device MPC loop (pl_mpc_set_noise).

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
on uint64 arrays masked to 32 bits, the uniforms U, the Box-Muller pair of a block and the noise /
wrench rule.  A draw is a function of (seed, stream, step k, component) alone:

  counter (k, i, stream, 0), key (seed & 0xffffffff, seed >> 32)
  U(a, b) = ((a >> 5) * 2**26 + (b >> 6)) * 2**-53                      exact, in [0, 1)
  u1 = 1 - U(w0, w1), theta = 0x1.921fb54442d18p+2 * U(w2, w3)
  r = sqrt(-2 log u1), z_{2i} = r cos theta, z_{2i+1} = r sin theta
  noise_j = sigma_j z_j (stream 0), wrench_c = det_c + sigma_w,c z_c (stream 1)

The integer part and the uniforms are exact; log, cos and sin are numpy's, so the normals agree with
another libm only within a few ulp (tests/test_noise_host.py measures it)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
STREAM_STATE, STREAM_WRENCH = 0, 1

# the published Random123 known answers for philox4x32 at 10 rounds: (counter, key, output)
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(ctr, key):
    """Philox4x32-10 of counters [..., 4] and keys [..., 2] (broadcast against each other): [..., 4]
    uint32 words."""
    ctr = np.asarray(ctr, dtype=np.uint64) & np.uint64(MASK)
    key = np.asarray(key, dtype=np.uint64) & np.uint64(MASK)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., j], shape).copy() for j in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape).copy(), np.broadcast_to(key[..., 1], shape).copy()
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 -> 64 bits, no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack(c, -1).astype(np.uint32)


def key_of(seed):
    """[..., 2] key words of uint64 seeds."""
    s = np.asarray(seed, dtype=np.uint64)
    return np.stack([s & np.uint64(MASK), s >> np.uint64(32)], -1)


def blocks(seed, k, stream, n_blocks, i0=0, c3=0):
    """[..., n_blocks, 4] words: block i has counter (k, i0 + i, stream, c3), key from seed [...]."""
    s = np.asarray(seed, dtype=np.uint64)
    i = (np.arange(n_blocks, dtype=np.uint64) + np.uint64(i0)) & np.uint64(MASK)
    ctr = np.stack([np.full(n_blocks, k, dtype=np.uint64), i, np.full(n_blocks, stream, dtype=np.uint64),
                    np.full(n_blocks, c3, dtype=np.uint64)], -1)
    return philox(ctr, key_of(s)[..., None, :])


def uniform(a, b):
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53


def uniforms(w):
    """(u1, theta) of words [..., 4]."""
    return 1.0 - uniform(w[..., 0], w[..., 1]), TWO_PI * uniform(w[..., 2], w[..., 3])


def normals(seed, k, stream, n):
    """z [..., n] of stream `stream` at step k for seeds [...]: component j is normal j & 1 of block j >> 1."""
    w = blocks(seed, k, stream, (n + 1) // 2)
    u1, th = uniforms(w)
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(th), r * np.sin(th)], -1)
    return z.reshape(z.shape[:-2] + (-1,))[..., :n]


def state_noise(seed, k, sigma):
    sigma = np.asarray(sigma, dtype=np.float64)
    return sigma * normals(seed, k, STREAM_STATE, sigma.shape[-1])


def base_wrench(seed, k, sigma_w, det=0.0):
    sigma_w = np.asarray(sigma_w, dtype=np.float64)
    return np.asarray(det, dtype=np.float64) + sigma_w * normals(seed, k, STREAM_WRENCH, 6)


def ulp_distance(a, b):
    """Largest distance of two float64 arrays in units in the last place (finite values of one sign
    pattern or not: the integer line through zero)."""
    def line(x):
        i = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0
    return int(np.abs(line(a).astype(object) - line(b).astype(object)).max())
