"""A numpy model of the device FLAC encoder's search space with LPC (DESIGN.md 3.10 "LPC";
test infrastructure, never imported by amx/).

The search space is the specification: every subframe's size has one right answer, and the
LPC predictor is fixed down to the operation order, so this model recomputes the encoder's
coefficients bit for bit.  Integer steps use Python / int64 integers, fp64 steps use
np.float64 scalars one operation at a time (+, -, *, / are correctly rounded on both sides).

    window(n)                      the integer Welch window
    autocorr(x, M)                 exact R[0..min(M, n - 1)] as Python ints
    predictors(x, M)               {order: (shift, [q...])} of the orders that quantise
    lpc_residual(x, q, shift)      residuals r[o..n) as int64
    lpc_candidates(x, w, M)        {order: (bits, shift, q)} of the candidate orders
    subframe_bits(x, w, M)         the smallest of CONSTANT, VERBATIM, FIXED 0..4 and LPC
    frame_minima(x16, block, M)    per frame: per-channel minima (C != 2), or the minimum
                                   of the four stereo assignments' sums
"""
import numpy as np

TCAP = 1 << 22        # an order with a folded residual at or above this is no candidate
QMAX = 2047           # 12-bit coefficients


def window(n):
    i = np.arange(n, dtype=np.int64)
    return (255 * 4 * (i + 1) * (n - i)) // ((n + 1) ** 2)


def autocorr(x, M):
    x = np.asarray(x, np.int64)
    n = len(x)
    xw = x * window(n)
    assert n == 0 or np.abs(xw).max() < 1 << 24
    return [int(np.dot(xw[l:], xw[:n - l])) for l in range(min(M, n - 1) + 1)]   # |R| < 2^61: int64 is exact


def _quantise(c):
    """(shift, q) of one order's fp64 coefficients, or None if the order is no candidate"""
    cmax = np.float64(0.0)
    for v in c:
        a = abs(v)
        if not a <= np.float64(QMAX):
            return None
        if a > cmax:
            cmax = a
    if cmax == 0.0:
        return None
    shift = None
    for s in range(15, -1, -1):
        if cmax * np.float64(1 << s) <= np.float64(QMAX):
            shift = s
            break
    if shift is None:
        return None
    scale = np.float64(1 << shift)
    e, q = np.float64(0.0), []
    for v in c:
        e = e + v * scale
        qi = min(max(int(np.floor(e + np.float64(0.5))), -2048), 2047)
        q.append(qi)
        e = e - np.float64(qi)
    return shift, q


def predictors(x, M):
    """Levinson in the specified operation order, then the quantisation of every order"""
    R = autocorr(x, M)
    if not R or R[0] == 0:
        return {}
    Rf = [np.float64(v) for v in R]             # int -> double, round to nearest even
    err, lpc, out = Rf[0], [], {}
    with np.errstate(all="ignore"):
        for i in range(len(R) - 1):
            acc = Rf[i + 1]
            for j in range(i):
                acc = acc - lpc[j] * Rf[i - j]
            k = acc / err
            lpc = [lpc[j] - k * lpc[i - 1 - j] for j in range(i)] + [k]
            err = err * (np.float64(1.0) - k * k)
            qz = _quantise(lpc)
            if qz is not None:
                out[i + 1] = qz
            if not err > 0.0:
                break
    return out


def lpc_residual(x, q, shift):
    x = np.asarray(x, np.int64)
    o = len(q)
    acc = np.zeros(len(x) - o, np.int64)
    for j, c in enumerate(q):
        acc += c * x[o - 1 - j:len(x) - 1 - j]
    return x[o:] - (acc >> shift)


def fold(r):
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def residual_bits(u, n, o):
    """min over the partition order of sum over partitions of (4 + min over k of
    [n_j (k + 1) + sum(u >> k)]); u: the n - o folded residuals"""
    u = np.concatenate([np.zeros(o, np.int64), u])        # warm-up samples: no code
    tz = (n & -n).bit_length() - 1
    best = None
    for p in range(0, min(6, tz) + 1):
        plen = n >> p
        if plen < o:
            continue
        cnt = np.full(1 << p, plen, np.int64)
        cnt[0] -= o
        per_k = np.stack([cnt * (k + 1) + (u >> k).reshape(1 << p, plen).sum(axis=1) for k in range(15)])
        total = int((4 + per_k.min(axis=0)).sum())
        best = total if best is None else min(best, total)
    return best


def fixed_bits(x, w, o):
    r = np.asarray(x, np.int64).copy()
    for _ in range(o):
        r = np.diff(r)
    return 8 + o * w + 6 + residual_bits(fold(r), len(x), o)


def lpc_candidates(x, w, M):
    x = np.asarray(x, np.int64)
    n = len(x)
    out = {}
    for o, (shift, q) in predictors(x, M).items():
        u = fold(lpc_residual(x, q, shift))
        if len(u) and u.max() >= TCAP:
            continue
        out[o] = (8 + o * w + 4 + 5 + 12 * o + 6 + residual_bits(u, n, o), shift, q)
    return out


def subframe_bits(x, w, M):
    x = np.asarray(x, np.int64)
    n = len(x)
    cands = [8 + n * w]
    if np.all(x == x[0]):
        cands.append(8 + w)
    for o in range(0, min(4, n) + 1):
        cands.append(fixed_bits(x, w, o))
    if M > 0:
        cands += [v[0] for v in lpc_candidates(x, w, M).values()]
    return min(cands)


def frame_minima(x16, block, M):
    x = np.asarray(x16, np.int64)
    out = []
    for s in range(0, len(x), block):
        seg = x[s:s + block]
        if seg.shape[1] != 2:
            out.append([subframe_bits(seg[:, c], 16, M) for c in range(seg.shape[1])])
            continue
        l, r = seg[:, 0], seg[:, 1]
        bl, br = subframe_bits(l, 16, M), subframe_bits(r, 16, M)
        bm, bs = subframe_bits((l + r) >> 1, 16, M), subframe_bits(l - r, 17, M)
        out.append(min(bl + br, bl + bs, bs + br, bm + bs))
    return out
