"""Host model of the counter-based streams (rng="counter", include/lmc_hip.h: LMC_RNG_COUNTER): Philox4x32-10, the decision
uniforms u_k, the words behind the momentum normals with the Box-Muller evaluated in float64, and CounterRng -- a
duck-typed stand-in for np.random.RandomState that hands the oracle the stream's values, which makes the unchanged
oracle (oracle/lmc_oracle.py threads its rng explicitly) an exact model of the mode. MomentumOnlyRng is the same for
momentum_rng="philox" (LMC_RNG_PHILOX): the stream's normals, numpy's own uniforms."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
C3_MOMENTUM = 0x6C6D636D    # "lmcm"
C3_UNIFORMS = 0x6C6D6375    # "lmcu"
KEY1 = 0x4D4F4D31


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC11) on Python integers: counter = (c0, c1, c2, c3), key = (k0, k1) -> 4 words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniform_block(seed, git, block):
    """The Philox block behind u_(2 block) and u_(2 block + 1) of iteration ``git``."""
    git = int(git)
    return philox4x32_10((git & M32, (git >> 32) & M32, block, C3_UNIFORMS), (seed, KEY1))


def words_to_unit(a, b):
    """rk_double's 53-bit form without the tempering: [0, 1)."""
    return ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0


def uniform(seed, git, k):
    """u_k: the k-th decision uniform iteration ``git`` of the chain seeded ``seed`` consumes."""
    w = uniform_block(seed, git, k >> 1)
    return words_to_unit(w[2], w[3]) if (k & 1) else words_to_unit(w[0], w[1])


def uniforms(seed, git, n):
    return np.array([uniform(seed, git, k) for k in range(n)])


def run_shape(d):
    """(elements per thread, wavefronts per chain) of the fused sampling kernel at model_ndim = d <= 1024."""
    need, ns = (d + 63) // 64, 1
    while ns < need:
        ns *= 2
    return (ns, 1) if ns <= 4 else (4, ns // 4)


def box_muller_f64(a, b):
    """The device's float32 Box-Muller (csrc/lmc_rng.hpp: box_muller_f32) on the same two words, evaluated in float64:
    u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 revolutions."""
    u1 = ((a >> 8) + 1) * 2.0 ** -24
    u2 = (b >> 8) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def normals(seed, git, d):
    """The d standard normals of iteration ``git``'s momentum draw: thread t of the chain owns elements t NS .. t NS + NS - 1
    and draws them from ONE block (c2 = t, c3 = "lmcm"): words (0, 1) -> elements 0 (cos) and 1 (sin), words (2, 3) -> 2, 3."""
    git = int(git)
    ns, _w = run_shape(d)
    out = np.zeros(d)
    for t in range((d + ns - 1) // ns):
        w = philox4x32_10((git & M32, (git >> 32) & M32, t, C3_MOMENTUM), (seed, KEY1))
        n = box_muller_f64(w[0], w[1]) + (box_muller_f64(w[2], w[3]) if ns > 2 else ())
        for s in range(ns):
            if t * ns + s < d:
                out[t * ns + s] = n[s]
    return out


class CounterRng:
    """The four methods the oracle calls on its rng, served from the counter-based streams. ``normals_by_iteration[t]`` is
    what ``normal(size)`` returns for iteration ``first + t`` (the model's own normals(), or the device's as fetched with
    Engine.counter_draws); each call starts the next iteration and resets k."""

    def __init__(self, seed, normals_by_iteration, first=0):
        self.seed = int(seed) & M32
        self._normals = normals_by_iteration
        self.git = int(first) - 1
        self.k = 0
        self.consumed = []     # uniforms consumed by every finished iteration
        self._open = False

    def normal(self, size=None):
        self._close()
        self.git += 1
        self.k = 0
        z = np.array(self._normals[len(self.consumed)], dtype=np.float64)
        assert z.shape == np.empty(size).shape, (z.shape, size)
        self._open = True
        return z

    def _close(self):
        if self._open:
            self.consumed.append(self.k)
            self._open = False

    def finish(self):
        """Close the running iteration; returns the uniforms consumed per iteration."""
        self._close()
        return list(self.consumed)

    def _next(self):
        u = uniform(self.seed, self.git, self.k)
        self.k += 1
        return u

    def rand(self):
        return self._next()

    def uniform(self, low=0.0, high=1.0):
        return low + (high - low) * self._next()


MT_N = 624   # words of one MT19937 generation; a uniform (random_sample) consumes two


class MomentumOnlyRng:
    """The oracle's rng under momentum_rng="philox" (include/lmc_hip.h: LMC_RNG_PHILOX): ``normal(size)`` is iteration
    ``first + t``'s row of ``normals_by_iteration`` (the model's normals(), or the device's as fetched with
    Engine.counter_draws) and leaves the generator alone; ``rand()`` / ``uniform()`` / ``get_state()`` are ONE
    np.random.RandomState(seed), numpy's legacy stream. Each ``normal()`` starts the next iteration; per finished iteration
    the uniforms consumed and whether they crossed a twist (position before + 2 x uniforms > 624) are recorded."""

    def __init__(self, seed, normals_by_iteration, first=0):
        self.seed = int(seed) & M32
        self._rs = np.random.RandomState(self.seed)
        self._normals = normals_by_iteration
        self.git = int(first) - 1
        self.k = 0
        self.consumed = []     # uniforms consumed by every finished iteration
        self.crossed = []      # ... and whether they crossed a twist
        self._pos = None       # the generator's position when the running iteration began
        self._open = False

    def normal(self, size=None):
        self._close()
        self.git += 1
        self.k = 0
        z = np.array(self._normals[len(self.consumed)], dtype=np.float64)
        assert z.shape == np.empty(size).shape, (z.shape, size)
        self._pos = int(self._rs.get_state()[2])
        self._open = True
        return z

    def _close(self):
        if self._open:
            self.consumed.append(self.k)
            self.crossed.append(self._pos + 2 * self.k > MT_N)
            self._open = False

    def finish(self):
        """Close the running iteration; returns (uniforms consumed, twist crossed) per iteration."""
        self._close()
        return list(self.consumed), list(self.crossed)

    def rand(self):
        self.k += 1
        return self._rs.random_sample()

    def uniform(self, low=0.0, high=1.0):
        self.k += 1
        return self._rs.uniform(low, high)

    def get_state(self):
        return self._rs.get_state()
