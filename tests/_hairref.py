"""Float64 reference of MarschnerHairBSDF::localSample with its TT and TRT paths
(tests/test_hair_lobes.py, tests/test_gpu_hair_lobes.py).

KIRK's function (Bsdf.cpp:465-769) read as a specification: a state machine of up
to three calls, carried across bounces in the path's flags.

  unflagged               choose p among the enabled lobes; p = 0 is the R lobe
                          (_shaderef._hair); p = 1 / 2 bend the ray into the fibre
                          by Snell with 1/ior and set CYL_T / CYL_TR; f = 0
  CYL_T alone             TT exit: leave the fibre, flags = 0, f = M_tt N_tt
  CYL_TR alone            mirror at the far wall, flags |= CYL_T | SPECULAR, f = 0
  CYL_TR and CYL_T        TRT exit: flags = 0, f = 10 M_trt N_trt

KIRK's quirks are the truth where they are KIRK's:
  * the lobe shift alpha and width beta are degrees used as radians (as in R);
  * both exits "refract" with eta = 1: the ray leaves unbent, then turns about the
    fibre axis by alpha/2 (TT) or 3 alpha/2 (TRT) -- the row-vector product of
    glm::rotate(-alpha/2), i.e. the transpose;
  * the material's diffuse colour is the absorption sigma, divided by cos(theta_r);
  * TT attenuates with exp(sigma' cos_gamma_t), cos_gamma_t = -2 cos(asin(h / eta'));
  * TRT squares exp(-2 sigma' cos(gamma_t)) and multiplies the result by 10;
  * dialectricFresnel receives angles where it expects cosines (as in R).

As in _shaderef every function takes `dtype` (float64 is the truth, float32 only
calibrates the tolerance) and returns the branch signature `sig` of each item.
"""
import numpy as np

import _shaderef as R
from _shaderef import F_CYL_T, F_CYL_TR, F_SPECULAR, Sig, dot, reflect, refract, rotate, unit, vec

LOBE_R, LOBE_TT, LOBE_TRT = 1, 2, 4
CALLS = ("first", "tt_exit", "mid", "trt_exit")


def lobe_pick(lobes, u, sig=None):
    """The lobe of an unflagged first hit: the k-th enabled one in the order R, TT, TRT,
    k = min(count - 1, floor(u count)).  Returns p in {0, 1, 2} per item."""
    u = np.asarray(u)
    enabled = [p for p in range(3) if (lobes >> p) & 1]
    count = len(enabled)
    k = np.minimum(count - 1, np.floor(u * u.dtype.type(count)).astype(np.int64))
    p = np.asarray(enabled, np.int64)[k]
    if sig is not None:
        sig.add(p == 1)
        sig.add(p == 2)
    return p


def call_of(flags):
    """Which call of the state machine the incoming flags select (index into CALLS)."""
    flags = np.asarray(flags, np.int64)
    t, tr = (flags & F_CYL_T) != 0, (flags & F_CYL_TR) != 0
    return np.where(~t & ~tr, 0, np.where(t & ~tr, 1, np.where(tr & ~t, 2, 3)))


def exit_theta_r(frame, wi, hair, trt):
    """theta_r of an exit call, float64: the angle from the fibre's U axis of -in turned about V by
    alpha / 2 (TT) or 3 alpha / 2 (TRT).  Both exits attenuate with exp(k sigma / cos(theta_r)), k = -2 cos(gamma_t)
    in [-2, 0) for TT and twice that, squared, for TRT: a test keeps its items away from cos(theta_r) = 0."""
    frame, wi, hair = (np.asarray(x, np.float64) for x in (frame, wi, hair))
    alpha = -(5 + 5 * hair[:, 0])
    out = rotate(-unit(wi), frame[:, 1], np.where(trt, 3 * alpha / 2, alpha / 2))
    return np.arctan2(np.hypot(dot(out, frame[:, 1]), dot(out, frame[:, 2])), dot(out, frame[:, 0]))


def hair_sample(mat, frame, wi, n, hair, lobe_u, flags_in, lobes, dtype=np.float64):
    """One call of the state machine on N items.  mat: per-item diffuse (N, 3) and ior (N);
    frame (N, 3, 3): the fibre's U, V, W; wi: ray_in; n: normal; hair (N, 2): the alpha /
    beta draws; lobe_u (N): the lobe draw; flags_in (N).  Returns out, pdf, f, sample,
    flags, valid, sig; what a call leaves unwritten is 0 (pdf, sample) or flags_in."""
    dt = dtype
    wi, n, hair, frame, lobe_u = (np.asarray(x, dt) for x in (wi, n, hair, frame, lobe_u))
    diffuse, ior = np.asarray(mat["diffuse"], dt), np.asarray(mat["ior"], dt)
    flags_in = np.asarray(flags_in, np.int64)
    N = len(wi)
    sig = Sig(N)
    call = call_of(flags_in)
    first, tt, mid, trt = (call == k for k in range(4))
    leaving = tt | trt
    early = sig.add(dot(wi, n) == 0)
    U, V, W = frame[:, 0], frame[:, 1], frame[:, 2]
    w = unit(wi)
    facing = sig.add(dot(n, w) > 0)
    nf = np.where(facing[..., None], n, -n)
    one = np.ones(N, dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # ---- the first hit ----
        p = lobe_pick(lobes, lobe_u)
        sig.add(p == 1, first)
        sig.add(p == 2, first)
        r_sig = Sig(N)
        r_out, r_pdf, r_f, r_theta = R._hair(R.MARSCHNER, frame, ior, wi, n, hair, r_sig, dt)
        for c in r_sig.cols[1:]:                               # (its first column is `facing` again)
            sig.add(c, first & (p == 0))
        bent, _ = refract(-w, nf, 1 / ior, sig, first & (p != 0))
        # ---- the far wall, TRT ----
        mirrored = reflect(-w, nf)
        # ---- the exits ----
        alpha, beta = -(5 + 5 * hair[:, 0]), 5 + 5 * hair[:, 1]
        turn = np.where(trt, 3 * alpha / 2, alpha / 2)         # R^T of glm::rotate(-turn) is a turn by +turn
        width = np.where(trt, 2 * beta, beta / 2)
        unbent, _ = refract(-w, nf, one, sig, leaving)
        e_out = rotate(unbent, V, turn)
        lin = vec(dot(wi, V), dot(wi, U), dot(wi, W))
        lout = vec(dot(e_out, V), dot(e_out, U), dot(e_out, W))
        theta_i = np.arctan2(np.hypot(lin[:, 0], lin[:, 2]), lin[:, 1])
        theta_r = np.arctan2(np.hypot(lout[:, 0], lout[:, 2]), lout[:, 1])
        theta_h, theta_d = (theta_r + theta_i) / 2, (theta_r - theta_i) / 2
        e_pdf = R.gauss_pdf(theta_h + turn, width)             # theta_h - (-alpha/2), theta_h - (-3 alpha/2)
        gamma = np.arccos(np.clip(dot(w, unit(n)), -1, 1))
        h = np.sin(gamma)
        x1 = np.sqrt(ior * ior - h * h)
        eta1 = x1 / np.cos(gamma)
        eta2 = ior * ior * np.cos(gamma) / x1
        c = np.arcsin(1 / eta1)
        F = R.fresnel(gamma, eta1, eta2, sig, leaving)
        sigma = diffuse / np.cos(theta_r)[..., None]
        pi = dt(np.pi)
        # TT
        dh_tt = 1 / np.abs((1 / np.sqrt(1 - h * h)) * (-(24 * c / pi ** 3) * gamma ** 2 + (6 * c / pi - 2)))
        cos_gt_tt = -2 * np.cos(np.arcsin(h / eta1))
        att_tt = ((1 - F) ** 2)[..., None] * np.exp(sigma * cos_gt_tt[..., None])
        f_tt = e_pdf[..., None] * (0.5 * att_tt * dh_tt[..., None]) / (np.cos(theta_d) ** 2)[..., None]
        # TRT
        dh_trt = 1 / np.abs((1 / np.sqrt(1 - h * h)) * (-(48 * c / pi ** 3) * gamma ** 2 + (12 * c / pi - 2)))
        gamma_t = np.arcsin(h / eta1)
        F_exit = R.fresnel(gamma_t, 1 / eta1, 1 / eta2, sig, trt)
        att_trt = ((1 - F) ** 2 * F_exit)[..., None] * np.exp(sigma * (-2 * np.cos(gamma_t))[..., None]) ** 2
        f_trt = 10 * (e_pdf[..., None] * (0.5 * att_trt * dh_trt[..., None]) / (np.cos(theta_d) ** 2)[..., None])
    zero3 = np.zeros((N, 3), dt)
    r_first = first & (p == 0)
    out = np.where(r_first[..., None], r_out, np.where(first[..., None], bent, np.where(mid[..., None], mirrored, e_out)))
    pdf = np.where(r_first, r_pdf, np.where(leaving, e_pdf, 0))
    f = np.where(r_first[..., None], r_f[..., None], np.where(tt[..., None], f_tt, np.where(trt[..., None], f_trt, zero3)))
    theta = np.where(r_first, r_theta, np.where(leaving, theta_i, 0))
    flags = np.where(r_first, F_SPECULAR, np.where(first, np.where(p == 1, F_CYL_T, F_CYL_TR),
                                                   np.where(mid, flags_in | F_CYL_T | F_SPECULAR, 0)))
    up = np.array([0, 0, 1], dt)
    res = {"out": np.where(early[..., None], up, out).astype(dt), "pdf": np.where(early, 0, pdf).astype(dt),
           "f": np.where(early[..., None], 0, f).astype(dt),
           "sample": np.where(early[..., None], 0, np.stack([theta, np.zeros(N, dt)], axis=1)).astype(dt),
           "flags": np.where(early, flags_in, flags).astype(np.int32), "valid": (~early).astype(np.int32)}
    s = sig.array()
    s[early, 1:] = 0                                           # nothing after the exit is a decision of the item
    res["sig"] = s
    return res
