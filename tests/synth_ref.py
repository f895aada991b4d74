"""Numpy float64 yardstick for clPolyphaseSynthesizer (the contract: include/mi355_clenabled.h).

  synth(g, M, ch_map, x, nframes)         the polyphase form: backward DFT of every input frame, then one FIR per output phase
  synth_direct(g, M, ch_map, x, nframes)  the closed form, y[n] = sum_f sum_q U_f[q] g[n - f' M] exp(2 pi i (n - f' M) ch_map[q] / M)
                                          with f' counted from the first new frame -- O(outputs x inputs), for small cases
  plan(K, M, nmap, nframes)               (taps per arm, input items read, output items written)

x is the history-prefixed input: (T - 1 + nframes) frames of nmap items, item-major.  Plain module, no fixtures.
"""
import numpy as np

TOL = 1e-5  # conftest.relerr(got, ref) <= TOL: DESIGN.md "Tolerances", the value the channelizer's tests use for transform + FIR


def taps_per_arm(K, M):
    return -(-K // M)


def plan(K, M, nmap, nframes):
    T = taps_per_arm(K, M)
    return T, (T - 1 + nframes) * nmap, nframes * M


def make_taps(K, seed=0):
    """no tap is zero (the locality test counts on it) and none is tiny"""
    rng = np.random.default_rng(1000 + seed)
    g = rng.uniform(0.25, 1.0, K) * rng.choice([-1.0, 1.0], K)
    return g.astype(np.float32)


def make_map(M, kind, seed=0):
    """'ident': None (all channels in order); 'perm': a seeded permutation of all M; 'half': a seeded subset of about M / 2 in
    seeded order; 'one': a single slot"""
    rng = np.random.default_rng(2000 + seed + M)
    if kind == "ident":
        return None
    if kind == "perm":
        return rng.permutation(M).astype(np.int32)
    if kind == "half":
        return rng.permutation(M)[:max(1, M // 2)].astype(np.int32)
    if kind == "one":
        return np.array([int(rng.integers(0, M))], np.int32)
    raise ValueError(kind)


def nmap_of(M, ch_map):
    return M if ch_map is None else len(ch_map)


def make_input(K, M, nmap, nframes, seed=0):
    rng = np.random.default_rng(3000 + seed)
    n = plan(K, M, nmap, nframes)[1]
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def transform(M, ch_map, x):
    """V[f, r] = sum_q U_f[q] exp(+2 pi i r ch_map[q] / M) for every frame of x, float64"""
    nmap = nmap_of(M, ch_map)
    u = np.asarray(x, np.complex128).reshape(-1, nmap)
    full = np.zeros((u.shape[0], M), np.complex128)
    full[:, np.arange(M) if ch_map is None else np.asarray(ch_map)] = u
    return np.fft.ifft(full, axis=1) * M


def synth(g, M, ch_map, x, nframes):
    g = np.asarray(g, np.float64)
    T = taps_per_arm(g.size, M)
    gp = np.zeros(T * M)
    gp[:g.size] = g
    arms = gp.reshape(T, M)  # arms[p, r] = g[r + M p]
    V = transform(M, ch_map, x)
    assert V.shape[0] == T - 1 + nframes
    y = np.zeros((nframes, M), np.complex128)
    for p in range(T):
        y += arms[p][None, :] * V[T - 1 - p:T - 1 - p + nframes]
    return y.reshape(-1)


def synth_direct(g, M, ch_map, x, nframes):
    g = np.asarray(g, np.float64)
    T = taps_per_arm(g.size, M)
    nmap = nmap_of(M, ch_map)
    cm = np.arange(M) if ch_map is None else np.asarray(ch_map)
    u = np.asarray(x, np.complex128).reshape(-1, nmap)
    y = np.zeros(nframes * M, np.complex128)
    for n in range(nframes * M):
        acc = 0j
        for f in range(u.shape[0]):
            k = n - (f - (T - 1)) * M  # f' = f - (T - 1)
            if 0 <= k < g.size:
                acc += g[k] * np.sum(u[f] * np.exp(2j * np.pi * ((k * cm) % M) / M))
        y[n] = acc
    return y


def case_id(v):
    return "-".join(str(e) for e in v)
