"""An adaptive pass's pixel selection (csrc/adaptive.h) restated in numpy over
_momentsref.rel_error, and the pass itself as select-then-fold over per-sample colours.
Test infrastructure only: nothing here imports the product."""
import numpy as np

import _momentsref as R

U32 = np.uint32
PLANES = R.PLANES


def active_mask(state, first_sample, threshold, min_samples, max_samples):
    """Per pixel of `state` (planes of any pixel shape): whether a pass starting at first_sample traces it."""
    n = np.asarray(state["count"], U32)
    if first_sample == 0:
        return np.ones(n.shape, bool)
    t = n.astype(np.uint64) + np.asarray(state["bad"], U32).astype(np.uint64)
    with np.errstate(all="ignore"):
        # negated: a NaN error stays active; below two samples a pixel is unconverged at every threshold, +inf too
        unconverged = (n < 2) | ~(R.rel_error(state) <= np.float32(threshold))
    capped = (t >= max_samples) if max_samples != 0 else np.zeros(n.shape, bool)
    return (t < min_samples) | (~capped & unconverged)


def select(state, owned, first_sample, threshold, min_samples, max_samples):
    """The active list: `owned` (indices into the flattened state) without the inactive pixels, order kept."""
    owned = np.asarray(owned, U32).reshape(-1)
    flat = {k: np.asarray(state[k]).reshape((-1,) + np.asarray(state[k]).shape[np.asarray(state["count"]).ndim:])
            for k in PLANES}
    return owned[active_mask(flat, first_sample, threshold, min_samples, max_samples)[owned]]


def run_pass(select_fn, fold_fn, state, cols, owned, first_sample, spp, **params):
    """One adaptive pass over per-sample colours cols (K, n_pixels, 3): select_fn(state, owned,
    first_sample, **params) picks the pixels, fold_fn(samples, first_sample, state) folds samples
    first_sample .. + spp - 1 of those pixels.  `state` is flat (n_pixels, ...), or None before the
    first pass (first_sample 0 then restarts every owned pixel).  Returns (new state, active list)."""
    n_pix = cols.shape[1]
    if state is None:
        state = R.zero_state((n_pix,))
    act = select_fn(state, owned, first_sample, **params)
    new = {k: np.array(state[k]) for k in PLANES}
    if act.size:
        sub = fold_fn(np.ascontiguousarray(cols[first_sample:first_sample + spp][:, act]), first_sample,
                      {k: np.ascontiguousarray(state[k][act]) for k in PLANES})
        for k in PLANES:
            new[k][act] = sub[k]
    return new, act
