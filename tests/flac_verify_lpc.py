"""tests/flac_verify.py plus LPC subframes (test infrastructure, never imported by amx/).

flac_verify.py refuses an LPC subframe by name (subframe_lpc) and stays as it is.  This
module reuses its metadata, header, CRC, residual and placement readers by calling them:
for the length of one verify() call, flac_verify._subframe is replaced by a function that
reads LPC subframes itself (RFC 9639 9.2.6, written from the RFC, no code shared with
csrc/amx_flac.cpp) and hands every other subframe to the original.

    samples, report = verify(data, profile=False, frames=None, frame_bytes=None, lpc_order=8,
                             any_rice=False)

As flac_verify.verify; an LPC subframe's record also carries precision, shift and
coefficients.  It adds the rules LPC_RULES; profile=True demands the device encoder's
promises with LPC: 12-bit coefficients (precision field 11), shift 0..15,
order <= lpc_order, every folded residual below 2^22 -- on top of flac_verify's profile
(partition order <= 6, method 0, k <= 14, no wasted bits, one metadata block).
any_rice=True (never with profile) also reads what flac_verify's residual reader refuses
by rule -- 5-bit Rice parameters and escaped partitions (9.2.7) -- with a reader of its own,
so that tests/flac_enc.py's LPC streams, which draw both at random, can be read at all.

    records(report)     the per-subframe records [frame][channel]: type, order, shift,
                        coefficients, partition_order, parameters, bits
"""
import numpy as np

import flac_verify
from flac_verify import FlacFormatError

LPC_RULES = ("lpc_precision_invalid", "lpc_shift_negative", "lpc_order_block",
             "profile_lpc_precision", "profile_lpc_shift", "profile_lpc_order", "profile_lpc_residual")


class LpcFormatError(FlacFormatError):
    """a FlacFormatError whose rule is one of LPC_RULES"""

    def __init__(self, rule, frame, detail=""):
        assert rule in LPC_RULES, rule
        self.rule, self.frame, self.detail = rule, frame, detail
        Exception.__init__(self, "%s (frame %s): %s" % (rule, frame, detail))


def _lpc_subframe(original, lpc_order):
    def subframe(br, k, block, w, profile):
        start = br.pos
        if br.s[start:start + 2] != "01" or br.n - start < 8:
            return original(br, k, block, w, profile)          # not LPC (type < 32), or truncated
        sub = dict(start_bit=start)
        br.u(1, k)
        t = br.u(6, k)
        order = t - 31
        wasted = 0
        if br.u(1, k):
            wasted = br.unary(k) + 1
            if profile:
                raise FlacFormatError("profile_wasted_bits", k, "%d wasted bits" % wasted)
            if wasted >= w:
                raise FlacFormatError("wasted_bits", k, "%d wasted bits of %d" % (wasted, w))
        ew = w - wasted
        sub.update(type=t, wasted=wasted, order=order)
        if order > block:
            raise LpcFormatError("lpc_order_block", k, "LPC order %d in a block of %d" % (order, block))
        v = [br.i(ew, k) for _ in range(order)]
        field = br.u(4, k)
        if field == 15:
            raise LpcFormatError("lpc_precision_invalid", k, "coefficient precision field 15")
        shift = br.i(5, k)
        if shift < 0:
            raise LpcFormatError("lpc_shift_negative", k, "prediction shift %d" % shift)
        coef = [br.i(field + 1, k) for _ in range(order)]
        sub.update(precision=field + 1, shift=shift, coefficients=coef)
        if profile:
            if field != 11:
                raise LpcFormatError("profile_lpc_precision", k, "precision field %d" % field)
            if shift > 15:
                raise LpcFormatError("profile_lpc_shift", k, "shift %d" % shift)
            if order > lpc_order:
                raise LpcFormatError("profile_lpc_order", k, "order %d above %d" % (order, lpc_order))
        res = flac_verify._residual(br, k, block, order, profile, sub)
        if profile and any((2 * r if r >= 0 else -2 * r - 1) >= 1 << 22 for r in res):
            raise LpcFormatError("profile_lpc_residual", k, "a folded residual of 2^22 or more")
        # 9.2.6: the first coefficient multiplies the sample just before; arithmetic shift
        # (Python's >> on its unbounded integers floors, as the RFC's does)
        for r in res:
            acc = 0
            for j in range(order):
                acc += coef[j] * v[-1 - j]
            v.append(r + (acc >> shift))
        lo, hi = -(1 << (ew - 1)), 1 << (ew - 1)
        if any(not lo <= s < hi for s in v):
            raise FlacFormatError("sample_range", k, "a decoded sample does not fit %d bits" % ew)
        sub["bits"] = br.pos - start
        return np.asarray(v, np.int64) << wasted, sub
    return subframe


def _any_rice_residual(br, k, block, order, profile, sub):
    """9.2.7 in full: coding methods 0 and 1 (4- and 5-bit parameters), escaped partitions"""
    method = br.u(2, k)
    if method > 1:
        raise FlacFormatError("rice_method_reserved", k, "residual coding method %d" % method)
    pbits = 4 + method
    sub["po_bit"] = br.pos
    po = br.u(4, k)
    sub["partition_order"] = po
    if block % (1 << po) or (block >> po) < order:
        raise FlacFormatError("partition_order", k, "partition order %d, block %d, predictor order %d"
                              % (po, block, order))
    res, params = [], []
    for part in range(1 << po):
        par = br.u(pbits, k)
        count = (block >> po) - (order if part == 0 else 0)
        if par == (1 << pbits) - 1:
            width = br.u(5, k)
            params.append(("escape", width))
            res += [br.i(width, k) for _ in range(count)]
            continue
        params.append(par)
        for _ in range(count):
            u = (br.unary(k) << par) | br.u(par, k)
            res.append(-((u + 1) >> 1) if u & 1 else u >> 1)
    sub["parameters"] = params
    return res


def verify(data, *, profile=False, frames=None, frame_bytes=None, lpc_order=8, any_rice=False):
    if any_rice and profile:
        raise ValueError("any_rice reads what the profile forbids")
    original, residual = flac_verify._subframe, flac_verify._residual
    flac_verify._subframe = _lpc_subframe(original, lpc_order)
    if any_rice:
        flac_verify._residual = _any_rice_residual
    try:
        return flac_verify.verify(data, profile=profile, frames=frames, frame_bytes=frame_bytes)
    finally:
        flac_verify._subframe, flac_verify._residual = original, residual


def records(report):
    keys = ("type", "order", "shift", "coefficients", "partition_order", "parameters", "bits")
    return [[{k: s.get(k) for k in keys} for s in fr["subframes"]] for fr in report["frames"] if fr["decoded"]]
