"""The per-pixel sample moments (csrc/moments.h) restated in numpy float32: every
step one float32 operation in the order the definition writes it, vectorised over the pixels.
Test infrastructure only: nothing here imports the product."""
import numpy as np

F32 = np.float32
U32 = np.uint32
PLANES = ("mean", "m2", "count", "bad")


def zero_state(shape):
    """The state when made: every plane zero.  `shape` is the pixels' shape."""
    shape = tuple(shape)
    return {"mean": np.zeros(shape + (3,), F32), "m2": np.zeros(shape + (3,), F32),
            "count": np.zeros(shape, U32), "bad": np.zeros(shape, U32)}


def fold(samples, first_sample=0, state=None):
    """Fold samples (K, ..., 3), sample s with global index first_sample + s, into a copy of
    `state` (zeroed if None).  Returns the new state with rel_error."""
    x = np.asarray(samples, F32)
    st = zero_state(x.shape[1:-1]) if state is None else {k: np.array(state[k]) for k in PLANES}
    mean, m2, n, bad = st["mean"], st["m2"], st["count"], st["bad"]
    with np.errstate(all="ignore"):
        for s in range(x.shape[0]):
            if first_sample + s == 0:                     # the framebuffer's own restart rule
                mean[...] = 0
                m2[...] = 0
                n[...] = 0
                bad[...] = 0
            xs = x[s]
            ok = np.isfinite(xs).all(-1)
            bad[~ok] += U32(1)
            n[ok] += U32(1)
            first = ok & (n == 1)
            mean[first] = xs[first]                       # an assignment: -0 survives
            m2[first] = F32(0)
            more = ok & (n > 1)
            nf = n.astype(F32)[..., None]
            d = (xs - mean).astype(F32)
            new_mean = (mean + (d / nf).astype(F32)).astype(F32)
            e = (xs - new_mean).astype(F32)
            new_m2 = (m2 + (d * e).astype(F32)).astype(F32)
            mean[more] = new_mean[more]
            m2[more] = new_m2[more]
    st["rel_error"] = rel_error(st)
    return st


def rel_error(st):
    """The error plane of a state: +inf below two samples, else the relative standard error of the
    mean with the channels summed."""
    mean, m2, n = np.asarray(st["mean"], F32), np.asarray(st["m2"], F32), np.asarray(st["count"], U32)
    with np.errstate(all="ignore"):
        s = ((m2[..., 0] + m2[..., 1]).astype(F32) + m2[..., 2]).astype(F32)
        mu = ((mean[..., 0] + mean[..., 1]).astype(F32) + mean[..., 2]).astype(F32)
        nf = n.astype(F32)
        den = (nf * (nf - F32(1.0)).astype(F32)).astype(F32)
        err = (np.sqrt((s / den).astype(F32)).astype(F32) / (np.abs(mu) + F32(1e-3)).astype(F32)).astype(F32)
    return np.where(n < 2, F32(np.inf), err).astype(F32)


def running_mean(samples, first_sample=0, start=None):
    """The framebuffer's running mean r + (c - r) / kk of k_accumulate, every prefix: (K, ..., 3)."""
    x = np.asarray(samples, F32)
    r = np.zeros(x.shape[1:], F32) if start is None else np.array(start, F32)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for s in range(x.shape[0]):
            k = first_sample + s
            if k == 0:
                r = x[s].copy()
            else:
                r = (r + ((x[s] - r).astype(F32) / F32(k + 1)).astype(F32)).astype(F32)
            out[s] = r
    return out


def bits(a):
    """An array's bits with every NaN made one pattern (tests/_util.py: NaNs compare by position)."""
    a = np.ascontiguousarray(a)
    if a.dtype != F32:
        return a.view(U32).copy()
    u = a.view(U32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def random_samples(n_samples, n_pixels, seed, bad=True):
    """Seeded sample colours (K, n_pixels, 3); with `bad`, NaN, +inf, -inf, 1e38 and -0 values injected."""
    rng = np.random.default_rng(seed)
    x = rng.gamma(0.7, 0.8, size=(n_samples, n_pixels, 3)).astype(F32)
    if bad:
        flat = x.reshape(-1)
        for v in (np.nan, np.inf, -np.inf, 1e38, -0.0):
            flat[rng.integers(0, flat.size, size=max(1, flat.size // 16))] = F32(v)
    return x
