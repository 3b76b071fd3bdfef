"""The ride stage (include/fishtts_hip.h: "Ride") restated in float64 on the host, on top of tests/level_ref.py (design,
K-weighting from zero state at sample 0, hop sums, blocks and gates): the running measure L(m) over the first m whole hops,
the nodes - look-ahead, slew, peak guard - and the interpolated float32 product.  ride() also returns the gate margin: the
smallest distance in LU of any block of any node's measure to -70 and to that node's relative gate, so that a test can
require inputs whose blocks cannot change sides through rounding.  The device filters every hop from a warm start two hops
earlier; that difference is the one level_ref already bounds.

`knock` leaves one rule out (tests/test_ride_ref_host.py shows that check() notices each): "slew" (v_k = u_k), "guard" (the
peak guard looks at p_k only), "look" (m_k = k instead of k + A), "interp" (every sample of hop k takes g_k)."""
from dataclasses import dataclass

import numpy as np

from tests import level_ref as R

A = 10                      # look-ahead, hops
SLEW = 0.5                  # dB per hop
CEILING = R.CEILING
NODE_TOL = 4e-7             # the level stage's gain bound (profiles/r14_level.txt)
OUT_TOL = 4e-7 + 2.0 ** -23


def hop(rate: int) -> int:
    return R.hop(rate)


def counts(n: int, H: int):
    """(whole hops W, hops with a peak Nh, nodes) of a stream of n samples."""
    nh = (n + H - 1) // H
    return n // H, nh, nh + 1


def plan(n_in: int, H: int, final: bool):
    """(final nodes, samples emitted) after n_in samples: the emission rule."""
    if final:
        return counts(n_in, H)[2], n_in
    w = n_in // H
    return (w - A + 1 if w >= A else 0), max(0, w - A) * H


@dataclass
class Ride:
    y: np.ndarray           # float32
    g: np.ndarray           # float32 nodes, ceil(n / H) + 1
    v: np.ndarray           # float64, before the guard
    capped: int             # nodes the guard bound
    margin: float           # smallest gate distance over all nodes' measures (inf: no block anywhere)
    L: np.ndarray           # L(m_k) per node


def ride(x, rate: int, target: int, knock: str = None) -> Ride:
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n, H = len(x), hop(rate)
    W, nh, nn = counts(n, H)
    e = R.hop_sums(R.kweight(x, rate), H)[:W] if n else np.zeros(0)
    p = np.zeros(nh + 2)                                    # p[k + 1] = p_k; p_-1 = p_Nh = 0
    for h in range(nh):
        p[h + 1] = float(np.max(np.abs(x[h * H:(h + 1) * H])))
    measured = {}
    margin = np.inf
    g, v, Ls = np.ones(nn, dtype=np.float32), np.zeros(nn), np.zeros(nn)
    prev, capped = 0.0, 0
    for k in range(nn):
        m = min(k if knock == "look" else k + A, W)
        if m not in measured:
            measured[m] = R.gate(e[:m], m * H, H)
        r = measured[m]
        margin = min(margin, r.margin)
        u = target / 100.0 - r.L if np.isfinite(r.L) else prev
        vk = u if k == 0 or knock == "slew" else min(max(u, prev - SLEW), prev + SLEW)
        q = p[k + 1] if knock == "guard" else max(p[k], p[k + 1])
        cap = 20.0 * np.log10(CEILING / q) if q > 0 else np.inf
        capped += cap < vk
        g[k] = np.float32(10.0 ** (min(vk, cap) / 20.0))
        v[k], Ls[k], prev = vk, r.L, vk
    i = np.arange(n)
    k, j = i // H, i % H
    w = (j.astype(np.float32) / np.float32(H)).astype(np.float32)
    if knock == "interp":
        w = np.zeros(n, dtype=np.float32)
    # fmaf(w, g_k+1 - g_k, g_k): the float32 difference, then product and sum exact in float64 and rounded once
    d = (g[k + 1] - g[k]).astype(np.float32) if n else np.zeros(0, dtype=np.float32)
    gain = (w.astype(np.float64) * d.astype(np.float64) + g[k].astype(np.float64)).astype(np.float32) if n else d
    return Ride((x * gain).astype(np.float32), g, v, int(capped), float(margin), Ls)


def check(g, y, ref: Ride) -> list:
    """What a candidate (nodes g, samples y) misses of the restatement `ref`: a list of messages, empty when it holds."""
    g, y = np.asarray(g, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if g.shape != ref.g.shape or y.shape != ref.y.shape:
        return [f"shapes {g.shape} {y.shape}, expected {ref.g.shape} {ref.y.shape}"]
    bad = []
    rel = np.abs(g.astype(np.float64) / ref.g.astype(np.float64) - 1.0)
    if len(rel) and rel.max() > NODE_TOL:
        bad.append(f"node {int(rel.argmax())}: {g[rel.argmax()]!r} against {ref.g[rel.argmax()]!r} ({rel.max():.3g})")
    err = np.abs(y.astype(np.float64) - ref.y.astype(np.float64)) - OUT_TOL * np.abs(ref.y.astype(np.float64))
    if len(err) and err.max() > 0:
        i = int(err.argmax())
        bad.append(f"sample {i}: {y[i]!r} against {ref.y[i]!r}")
    if len(y) and np.max(np.abs(y)) > CEILING * (1 + 2.0 ** -22):
        bad.append(f"peak {np.max(np.abs(y))!r} above the ceiling")
    return bad


def step_signal(rate: int, seed: int = 0, seconds: float = 6.4) -> np.ndarray:
    """A speech-like signal: modulated noise with a 0.5 s near-silent gap, a +12 dB step and one 0.9 click."""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    env = 0.03 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t) ** 2)
    env[(t >= 1.6) & (t < 2.1)] = 1e-5
    env[t >= 3.3] *= 10.0 ** (12.0 / 20.0)
    x = env * rng.standard_normal(n)
    x[int(4.27 * rate) + 3] = 0.9
    return x.astype(np.float32)
