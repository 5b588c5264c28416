"""fp64 reference of the weight EMA that the *_ema AdamW entries keep (include/mesm_gfx950.h), in numpy.

The decay a kernel applies is a float32; the reference takes that float32 VALUE and widens it, so what it measures is the
rounding of the update expression (one subtract, one FMA: an analytic bound of 3 units of 2^-24 * max(|e|, |p|)), not the
rounding of the decay."""
import numpy as np

EMA_UNITS = 4             # the bound of the tests, in units of
EMA_UNIT = 2.0 ** -24     # ... this, times max(|e_old|, |p_new|), per update


def widen(decay):
    """the float32 nearest to `decay`, as a float64"""
    return np.float64(np.float32(decay))


def decay_schedule(n, decay, warmup):
    """decay of the update that follows n earlier ones, in float64 from the float32 value of `decay`:
    min(decay, (1 + n) / (10 + n)) with warm-up, `decay` without"""
    d = widen(decay)
    if not warmup:
        return d
    n = np.float64(n)
    return min(d, (1.0 + n) / (10.0 + n))


def ema_update(e_old, p_new, decay):
    """d * e_old + (1 - d) * p_new in float64; e_old, p_new: float32 arrays, decay: the float32 the device used"""
    d = widen(decay)
    e, p = np.asarray(e_old, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return d * e + (1.0 - d) * p


def ema_recurrence(e0, p_seq, decays, written=None):
    """the recurrence over a sequence of parameter values (float32 arrays) with one decay per update, carried in float64;
    `written` (bool array or None = everywhere): elements outside it keep e0.  -> (e in float64, max |value| seen per
    element: the magnitude the per-update bound scales with)"""
    e = np.asarray(e0, dtype=np.float64).copy()
    big = np.abs(e)
    for p, d in zip(p_seq, decays):
        new = ema_update(e, p, d)
        e = new if written is None else np.where(written, new, e)
        big = np.maximum(big, np.maximum(np.abs(e), np.abs(np.asarray(p, dtype=np.float64))))
    return e, big


def ema_bound(e_old, p_new, updates=1):
    """per element: updates * 4 * 2^-24 * max(|e_old|, |p_new|)"""
    m = np.maximum(np.abs(np.asarray(e_old, dtype=np.float64)), np.abs(np.asarray(p_new, dtype=np.float64)))
    return updates * EMA_UNITS * EMA_UNIT * m
