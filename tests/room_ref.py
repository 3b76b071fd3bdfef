"""The room stage restated in numpy (include/fishtts_hip.h: "Room"), from the impulse response at the output rate onward: irF
arrives as an array, so everything behind its preparation is compared bit for bit.  The chain is a loop over the taps of
mix_ref.fmaf32 over all outputs at once; E in float64 in the stated block order; float32 operations one at a time elsewhere
(numpy rounds every float32 operation on its own).

`knock` takes one rule out, so that tests/test_room_ref_host.py can show each is caught:
  "descending"  the taps of the chain taken from L - 1 down to 0
  "wetfold"     T[wet] folded into hn (one product less per output, a rounding moved)
  "predelay"    the predelay off by one
  "energy"      E over the unfaded taps
  "ceiling"     the ceiling applied when pk == c too"""
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from tests.mix_ref import CEILING, fmaf32, gains, ramp

MAX_L = 131072
BLOCK = 256


class Params(NamedTuple):
    normalize: int = 1
    wet: int = 1200
    dry: int = 0
    send: int = 0
    ceiling: int = 1
    offset: int = 0
    length: int = 0
    fade: int = 0
    predelay: int = 0
    tail: int = -1


class Roomed(NamedTuple):
    y: np.ndarray          # float32 [N]
    c: np.ndarray          # the chain
    hn: np.ndarray
    N: int
    L: int
    E: float
    gn: np.float32
    pk: np.float32
    sg: np.float32
    capped: bool


def plan(n: int, nh: int, p: Params) -> Tuple[int, int]:
    """(L, N) by the stated rules (the refusals are the caller's to avoid)."""
    assert nh - p.offset >= 1
    L = nh - p.offset if p.length == 0 else min(p.length, nh - p.offset)
    assert L <= MAX_L
    tl = p.predelay + L - 1
    if p.tail >= 0:
        assert p.tail <= tl
        tl = p.tail
    return L, n + tl


def taps(irF, p: Params):
    """(t, unfaded t): the used response with the fade on its last f taps."""
    irF = np.asarray(irF, dtype=np.float32).reshape(-1)
    L, _ = plan(1, len(irF), p)
    raw = irF[p.offset:p.offset + L].copy()
    t = raw.copy()
    f = min(p.fade, L)
    if f > 0:
        k = np.arange(L - f, L)
        t[L - f:] = t[L - f:] * ramp(L - 1 - k, f)
    return t, raw


def energy(t) -> float:
    """E: float64 sums, k ascending inside blocks of 256 taps, then the blocks ascending."""
    E = 0.0
    t64 = np.asarray(t, dtype=np.float32).astype(np.float64)
    for b in range(0, len(t64), BLOCK):
        e = 0.0
        for v in t64[b:b + BLOCK]:
            e = e + v * v
        E = E + e
    return float(E)


def send_of(n: int, regions: Sequence[Tuple[int, int, int]], send: int) -> np.ndarray:
    s = np.full(n, send, dtype=np.int64)
    for a, e, v in regions:
        s[a:e] = v
    return s


def sent(x, regions, send: int) -> np.ndarray:
    """xs: one float32 product per sample, +0.0 where the send is -1."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    s = send_of(len(x), regions, send)
    T = gains()
    with np.errstate(invalid="ignore", over="ignore"):
        xs = (x * T[np.maximum(s, 0)]).astype(np.float32)
    xs[s < 0] = np.float32(0.0)
    return xs


def chain(xs, hn, predelay: int, N: int, descending: bool = False) -> np.ndarray:
    """c[i] = the fmaf chain over the taps, k ascending, xs +0.0 outside [0, n); then + 0.0 (a -0.0 becomes +0.0)."""
    xs = np.asarray(xs, dtype=np.float32).reshape(-1)
    hn = np.asarray(hn, dtype=np.float32).reshape(-1)
    n, L = len(xs), len(hn)
    pad = np.zeros(N + L + predelay + n, dtype=np.float32)       # pad[j + L + predelay] = xs[j]
    pad[L + predelay:L + predelay + n] = xs
    acc = np.zeros(N, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in (range(L - 1, -1, -1) if descending else range(L)):
            acc = fmaf32(hn[k], pad[L - k:L - k + N], acc)
        return (acc + np.float32(0.0)).astype(np.float32)


def room(x, irF, regions=(), p: Params = Params(), knock: Optional[str] = None, ceiling: float = CEILING) -> Roomed:
    """The stage.  `ceiling`: c, for the host test alone - 10^(-1/20) is no float32, so pk == c needs a c that is one."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = len(x)
    L, N = plan(n, len(np.asarray(irF).reshape(-1)), p)
    t, raw = taps(irF, p)
    E = energy(raw if knock == "energy" else t)
    gn = np.float32(1.0 / np.sqrt(E)) if p.normalize else np.float32(1.0)
    T = gains()
    with np.errstate(invalid="ignore", over="ignore"):
        hn = (t * gn).astype(np.float32)
        gw = T[p.wet]
        if knock == "wetfold":
            hn, gw = (hn * gw).astype(np.float32), np.float32(1.0)
        xs = sent(x, regions, p.send)
        c = chain(xs, hn, p.predelay + (1 if knock == "predelay" else 0), N, descending=knock == "descending")
        wet = (gw * c).astype(np.float32)
        dry = np.zeros(N, dtype=np.float32)
        if p.dry >= 0:
            dry[:n] = (T[p.dry] * x).astype(np.float32)
        m = (dry + wet).astype(np.float32)
        a = np.abs(m)
    a = a[~np.isnan(a)]
    pk = np.float32(a.max()) if len(a) else np.float32(0.0)
    capped = bool(p.ceiling) and (float(pk) >= ceiling if knock == "ceiling" else float(pk) > ceiling)
    sg = np.float32(ceiling / float(pk)) if capped else np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (m * sg).astype(np.float32) if capped else m
    return Roomed(y, c, hn, N, L, E, gn, pk, sg, capped)
