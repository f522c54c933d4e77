"""BSDF sampling, hit normals and light sampling against a float64 truth (tests/_shaderef.py).

The parity tests pin libkirk_hip.so to the oracle bit for bit, and the oracle's
shading to a dozen hand-picked known answers; a slip both sides share would
pass all of that.  Here the oracle (CPU) and the product's own device functions
(`gpu`, through the ABI 15 batch queries) answer seeded items -- 4096 per BSDF
kind and per light kind, the hits of the geometry truth's rays for the surface --
and every answer is compared with a float64 reference written from KIRK's
semantics alone.

Only *decisive* items are compared with the truth: those whose branch signature
(every data-dependent decision: entering / leaving, the disc map's quadrant, the
tangent frame's choice, sample.y > F, total internal reflection, the clamps, the
light tests' rejections ...) is unchanged when the item's float32 inputs move by
+-2 ulps.  All items, decisive or not, are compared device against oracle bit
for bit.

Tolerance: |got - truth| <= M (J + 2^-24 |truth|) per output, J the spread of
the float64 truth over the jitters (the output's conditioning).  M is measured,
not guessed: the reference itself run in float32 strays from its float64 self by
at most M_REF32[case] of that unit over the decisive items (measured here on the
CPU, `measure_m()`), and the constant is 4 x that: the project's own sin / cos /
atan2 / exp are allowed 2-3 float ulps where libm stays under 1
(tests/test_kmath.py), and operation order differs from numpy's.  Nothing here
is derived from what the oracle or the device returns.
"""
import numpy as np
import pytest

import _geomref as G
import _shaderef as R
import oracle_ffi
from _util import compare_images
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S

N_ITEMS = 4096
MAX_UNDECISIVE = 0.05          # per kind: a condition on the inputs, not on the code under test
MARGIN = 4
# worst |ref32 - ref64| / (J + 2^-24 |truth|) over the decisive items, measured by measure_m()
M_REF32 = {
    # BSDF kinds: the worst of direction, pdf, f and the sample written back
    "lambert": 83.2, "specular_reflection": 0.756, "specular_transmission": 3.96, "glossy": 4.63, "glass": 3.62,
    "milk_glass": 4.88, "lambert_transmission": 36.0, "emission": 0.0, "transparent": 0.42, "marschner": 65.9,
    "deon": 9.63, "eval": 0.658,
    # lights: ray and attenuation; hit distance and emitted colour
    "light_dir:point": 1.59, "light_dir:quad": 2.27, "light_dir:spot": 7.6, "light_dir:sun": 2.18,
    "light_isect:point": 30.9, "light_isect:quad": 1.76, "light_isect:spot": 1.55, "light_isect:sun": 0.0,
    # the normal at a hit (the cone's float32 quadratic cancels: eps32 t^2 / r^2, see _geomref)
    "normal:cone": 792.0, "normal:triangle": 0.442,
}
M = {k: MARGIN * v for k, v in M_REF32.items()}
FRAME_ULPS = 8 * 2.0 ** -23    # U, V, W orthonormal, V along the axis: a handful of float32 roundings each
BSDF_OUT = ("out", "pdf", "f", "sample")
KINDS_ALL, KINDS_FUR = (1 << 11) - 1, (1 << R.LAMBERT) | (1 << R.MARSCHNER)
TOP32 = np.float32(1.0 - 2.0 ** -24)    # the largest draw


def unit32(v):
    v = np.asarray(v, np.float32)
    return v / np.linalg.norm(v, axis=-1, keepdims=True).astype(np.float32)


def cone_frames(sd, dtype=np.float64):
    """U, V, W of every world-space cone as Cylinder::Cylinder derives them (Cylinder.cpp:17-25):
    V along the axis, U = V x (0, 1, 0) (or x (0, 0, 1) for an axis within 1e-4 of +-y), W = U x V."""
    b = np.asarray(sd.cone_base_r0, dtype)[:, :3]
    a = np.asarray(sd.cone_apex_r1, dtype)[:, :3]
    v = R.unit(a - b)
    up = np.where((1 - np.abs(v[:, 1:2])) < 1e-4, np.array([0, 0, 1], dtype), np.array([0, 1, 0], dtype))
    u = R.unit(R.cross(v, up))
    w = R.unit(R.cross(u, v))
    return np.stack([u, v, w], axis=1)


# ---- the zoo with the extra materials and lights of the edge cases ----------------------------
class Zoo:
    def __init__(self):
        sd = S.zoo()
        self.kind_mats = {k: [i for i, m in enumerate(sd.materials) if m.bsdf == k and i >= 2] for k in range(11)}
        add = lambda k, **kw: self.kind_mats[k].append(sd.add_material(S.material(N.BSDF_NAMES[k], **kw)))
        for ior in (1.0, 2.4):
            add(R.SPEC_TRANS, volume=(0.9, 1.0, 0.9), ior=ior)
            add(R.GLASS, volume=(1.0, 0.95, 0.9), specular=(0.9, 0.8, 0.7), ior=ior)
        for ior, rough in ((1.0, 0.0), (2.4, 0.3), (1.45, 1.0), (2.4, 0.0), (1.0, 1.0)):
            add(R.MILK_GLASS, volume=(0.9, 0.9, 1.0), specular=(0.8, 0.9, 0.7), ior=ior, roughness=rough)
        for rough in (0.0, 1.0):
            add(R.GLOSSY, specular=(0.8, 0.8, 0.8), roughness=rough)
        # lights 0..3: the zoo's point, quad, spot and sun; then the edge cases
        sd.lights += [S.point_light((1.0, 2.0, -1.0), (1.0, 2.0, 3.0), radius=0.0),                       # 4: never hit
                      S.point_light((-1.0, 1.5, 2.0), (2.0, 2.0, 1.0), radius=0.3, att_const=0.0, att_lin=0.0,
                                    att_quad=0.0),                                                          # 5: c = l = q = 0
                      S.quad_light((0.5, 2.0, 0.5), (0.2, -1.0, 0.1), (0.8, 0.5), (1.0, 2.0, 3.0), att_const=0.0,
                                   att_lin=0.0, att_quad=0.0),                                              # 6
                      S.spot_light((1.0, 2.0, 2.0), (-0.3, -1.0, -0.2), (3.0, 2.0, 1.0), radius=0.4, outer=25.0,
                                   inner=10.0, att_const=0.0, att_lin=0.0, att_quad=0.0),                   # 7
                      S.quad_light((-1.0, 2.5, 0.0), (0.0, -1.0, 0.0), (1.0, 0.6), (2.0, 2.0, 2.0), att_const=0.5,
                                   att_lin=0.2, att_quad=0.1)]                                              # 8: c, l, q > 0
        self.sd = sd
        self.nt = len(sd.tri_v)
        self.table = R.materials_table(sd)
        self.frames = {dt: np.concatenate([np.zeros((self.nt, 3, 3), dt), cone_frames(sd, dt)])
                       for dt in (np.float64, np.float32)}
        self.lights_of = {k: [i for i, L in enumerate(sd.lights) if L.kind == k] for k in range(4)}
        self._oracle = None
        self._cases = {}

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_ffi.Oracle(self.sd)
        return self._oracle

    def case(self, key):
        if key not in self._cases:
            what, _, name = key.partition(":")
            if what == "light_dir":
                self._cases[key] = LightDirCase(self, R.LIGHT_NAMES.index(name))
            elif what == "light_isect":
                self._cases[key] = LightIsectCase(self, R.LIGHT_NAMES.index(name))
            elif key == "eval":
                self._cases[key] = EvalCase(self)
            else:
                self._cases[key] = BsdfCase(self, R.KIND_NAMES.index(key))
        return self._cases[key]


_ZOO = []


@pytest.fixture(scope="module")
def zoo():
    """The scene, its float64 truths (computed once, shared by the CPU and the GPU tests) and its oracle."""
    if not _ZOO:
        _ZOO.append(Zoo())
    return _ZOO[0]


def directions(rng, n):
    """`in` uniform on the sphere; `n` uniform, rejected to |dot(in, n)| >= 0.05 (float32 unit vectors)."""
    wi = unit32(rng.normal(size=(n, 3)))
    nn = unit32(rng.normal(size=(n, 3)))
    while True:
        bad = np.abs(np.sum(wi.astype(np.float64) * nn, axis=1)) < 0.05
        if not bad.any():
            return wi, nn
        nn[bad] = unit32(rng.normal(size=(int(bad.sum()), 3)))


class Case:
    """One family of items: float32 inputs, the float64 truth, the decisive mask, J and the float32 reference."""
    float_inputs = ()
    outputs = ()

    def finish(self):
        fn = lambda **kw: self.ref(np.float64, **kw)
        self.truth, self.decisive, self.J = R.decisive(fn, {k: self.inp[k] for k in self.float_inputs}, self.outputs)
        self._ref32 = None

    @property
    def ref32(self):
        if self._ref32 is None:
            self._ref32 = self.ref(np.float32, **{k: self.inp[k] for k in self.float_inputs})
        return self._ref32

    def worst(self, got, where=None):
        """Worst |got - truth| / (J + eps32 |truth|) over the decisive items, per output."""
        sel = self.decisive if where is None else self.decisive & where
        out = {}
        for k in self.outputs:
            r = R.ratio(np.asarray(got[k])[sel], self.truth[k][sel], self.J[k][sel])
            out[k] = (float(np.max(np.where(np.isnan(r), np.inf, r), initial=0.0)),
                      int(np.nonzero(sel)[0][np.argmax(np.where(np.isnan(r), np.inf, r))]) if sel.any() else -1)
        return out

    def check(self, who, got, where=None):
        """`got` (the oracle's or the device's answer) against the truth on the decisive items."""
        w = self.worst(got, where)
        print(f"{self.key} {who}: worst ratio " + ", ".join(f"{k} {v[0]:.3g}" for k, v in w.items()) +
              f" (bound {M[self.key]:.3g}, {int(self.decisive.sum())} decisive of {len(self.decisive)})")
        sel = self.decisive if where is None else self.decisive & where
        for k in self.exact:
            a, b = np.asarray(got[k])[sel], np.asarray(self.truth[k])[sel]
            bad = np.nonzero(a != b)[0]
            assert len(bad) == 0, f"{self.key} {who}: {k} of item {np.nonzero(sel)[0][bad[0]]}: {a[bad[0]]} != {b[bad[0]]}"
        for k, (r, i) in w.items():
            assert r <= M[self.key], (f"{self.key} {who}: {k} of item {i}: got {np.asarray(got[k])[i]}, truth "
                                      f"{self.truth[k][i]}, J {self.J[k][i]}: ratio {r:.4g} > {M[self.key]:.4g}")


class BsdfCase(Case):
    float_inputs = ("wi", "n", "sample", "hair")
    outputs = BSDF_OUT
    exact = ("flags", "valid")

    def __init__(self, zoo, kind):
        self.zoo, self.kind, self.key = zoo, kind, R.KIND_NAMES[kind]
        rng = np.random.default_rng(1000 + kind)
        wi, nn = directions(rng, N_ITEMS)
        sample = rng.random((N_ITEMS, 2), np.float32)
        hair = rng.random((N_ITEMS, 2), np.float32)
        flags = np.zeros(N_ITEMS, np.int32)
        mats = zoo.kind_mats[kind]
        mat = np.asarray(mats, np.int32)[rng.integers(0, len(mats), N_ITEMS)]
        if kind in (R.MARSCHNER, R.DEON):       # a cone that carries the material
            cones = zoo.nt + np.nonzero(zoo.sd.cone_mat == mats[0])[0]
            obj = cones[rng.integers(0, len(cones), N_ITEMS)].astype(np.int32)
        else:
            obj = rng.integers(0, zoo.nt, N_ITEMS).astype(np.int32)
        # the fixed lattice, in the last items
        k = N_ITEMS
        for axis in range(3):                                      # n on each axis
            for s in (1.0, -1.0):
                k -= 1
                nn[k] = 0.0
                nn[k, axis] = s
        for s in (1.0, -1.0):                                      # in exactly +-n
            for _ in range(4):
                k -= 1
                wi[k] = s * nn[k]
        for s in (1.0, -1.0):                                      # the tangent frame's tie n.x == +-n.y
            for _ in range(4):
                k -= 1
                nn[k, 1] = s * nn[k, 0]
                nn[k] = unit32(nn[k])
                nn[k, 1] = s * nn[k, 0]
        for a in (np.float32(0.0), TOP32):                         # draws of exactly 0 and of 1 - 2^-24
            for b in (np.float32(0.0), TOP32):
                k -= 1
                sample[k] = (a, b)
                k -= 1
                hair[k] = (a, b)
                k -= 1
                sample[k] = (a, b)
                hair[k] = (b, a)
        for f in (R.F_CYL_T, R.F_CYL_TR, R.F_CYL_T | R.F_CYL_TR, R.F_CYL_T | R.F_SPECULAR):
            for _ in range(2):
                k -= 1
                flags[k] = f
        self.n_lattice = N_ITEMS - k
        self.inp = {"obj": obj, "mat": mat, "wi": wi, "n": nn, "sample": sample, "hair": hair, "flags": flags}
        self.finish()

    def ref(self, dt, wi, n, sample, hair):
        t = self.zoo.table
        m = {k: t[k][self.inp["mat"]] for k in ("diffuse", "specular", "volume", "ior", "roughness")}
        return R.bsdf_sample(self.kind, m, self.zoo.frames[dt][self.inp["obj"]], wi, n, sample, hair,
                             self.inp["flags"], dt)

    def ask(self, who, kinds_mask=None, sel=slice(None)):
        i = self.inp
        return who.debug_bsdf_sample(i["obj"][sel], i["mat"][sel], i["wi"][sel], i["n"][sel], i["sample"][sel],
                                     i["hair"][sel], i["flags"][sel], kinds_mask)


class EvalCase(Case):
    """bsdf_eval: every kind's zoo material in one batch."""
    float_inputs = ("wi", "n", "wo")
    outputs = ("f",)
    exact = ()
    key = "eval"

    def __init__(self, zoo):
        self.zoo = zoo
        rng = np.random.default_rng(77)
        wi, nn = directions(rng, N_ITEMS)
        wo = unit32(rng.normal(size=(N_ITEMS, 3)))
        wo[-8:] = -wi[-8:]
        wo[-16:-8] = wi[-16:-8]
        self.kind_of = rng.integers(0, 11, N_ITEMS)
        mat = np.array([zoo.kind_mats[k][0] for k in self.kind_of], np.int32)
        obj = rng.integers(0, zoo.nt, N_ITEMS).astype(np.int32)
        self.inp = {"obj": obj, "mat": mat, "wi": wi, "n": nn, "wo": wo}
        self.finish()

    def ref(self, dt, wi, n, wo):
        f = np.zeros((N_ITEMS, 3), dt)
        sig = np.zeros((N_ITEMS, 1), np.int8)
        for k in range(11):
            s = self.kind_of == k
            r = R.bsdf_eval(k, {"diffuse": self.zoo.table["diffuse"][self.inp["mat"][s]]}, wi[s], n[s], wo[s], dt)
            f[s], sig[s] = r["f"], r["sig"] if k in (R.LAMBERT, R.MARSCHNER, R.LAMBERT_TRANS) else 0
        return {"f": f, "sig": sig}

    def ask(self, who):
        i = self.inp
        return {"f": who.debug_bsdf_eval(i["obj"], i["mat"], i["wi"], i["n"], i["wo"])}


class LightDirCase(Case):
    float_inputs = ("p", "u")
    outputs = ("o", "d", "att")
    exact = ()

    def __init__(self, zoo, kind):
        self.zoo, self.kind, self.key = zoo, kind, "light_dir:" + R.LIGHT_NAMES[kind]
        rng = np.random.default_rng(2000 + kind)
        ids = zoo.lights_of[kind]
        self.light = np.asarray(ids, np.int32)[rng.integers(0, len(ids), N_ITEMS)]
        p = rng.uniform(-3.0, 3.0, (N_ITEMS, 3)).astype(np.float32) + np.float32([0, 1, 0])
        u = rng.random((N_ITEMS, 2), np.float32)
        u[-4:] = [(0, 0), (0, TOP32), (TOP32, 0), (TOP32, TOP32)]
        if kind == R.SPOT:      # points on the inner and the outer cone of each spot light (the clamp's two ends)
            k = N_ITEMS - 4
            for li in ids:
                L = R.light_setup(zoo.sd.lights[li])
                e1, _ = R.plane_base(L["dir"])
                for ang in (L["inner"], L["outer"]):
                    for dist in (0.5, 1.0, 2.0, 4.0):
                        k -= 1
                        a = np.radians(ang)
                        p[k] = L["pos"] + dist * (np.cos(a) * L["dir"] + np.sin(a) * e1)
                        u[k] = (0.0, 0.0)              # the disc's centre
                        self.light[k] = li
        self.inp = {"p": p, "u": u}
        self.finish()

    def ref(self, dt, p, u):
        out = {"o": np.zeros((N_ITEMS, 3), dt), "d": np.zeros((N_ITEMS, 3), dt), "att": np.zeros(N_ITEMS, dt),
               "sig": np.zeros((N_ITEMS, 2), np.int8)}
        for li in np.unique(self.light):
            s = self.light == li
            r = R.light_dir(R.light_setup(self.zoo.sd.lights[li], dt), p[s], u[s], dt)
            for k in ("o", "d", "att"):
                out[k][s] = r[k]
            out["sig"][s, :r["sig"].shape[1]] = r["sig"]
        return out

    def ask(self, who):
        return who.debug_light_dir(self.light, self.inp["p"], self.inp["u"])


class LightIsectCase(Case):
    float_inputs = ("o", "d")
    outputs = ("t", "emit")
    exact = ("hit",)

    def __init__(self, zoo, kind):
        self.zoo, self.kind, self.key = zoo, kind, "light_isect:" + R.LIGHT_NAMES[kind]
        rng = np.random.default_rng(3000 + kind)
        ids = zoo.lights_of[kind]
        self.light = np.asarray(ids, np.int32)[rng.integers(0, len(ids), N_ITEMS)]
        o = rng.uniform(-3.0, 3.0, (N_ITEMS, 3)).astype(np.float32) + np.float32([0, 1, 0])
        # aimed at a point near the light (within 1.5 x its extent), so that about half of the rays hit
        aim = np.zeros((N_ITEMS, 3))
        for li in ids:
            s = self.light == li
            L = zoo.sd.lights[li]
            ext = max(L.radius, 0.5 * max(L.size[0], L.size[1]), 0.1)
            aim[s] = np.asarray(list(L.position)) + rng.normal(size=(int(s.sum()), 3)) * (0.6 * ext)
        d = unit32(aim - o)
        k = N_ITEMS
        if kind == R.POINT:       # rays leaving a point light's centre (Appendix A.3), and rays from inside
            for li in ids:
                for _ in range(8):
                    k -= 1
                    o[k] = list(zoo.sd.lights[li].position)
                    self.light[k] = li
                for _ in range(8):
                    k -= 1
                    o[k] = np.float32(list(zoo.sd.lights[li].position)) + np.float32(0.05) * d[k]
                    self.light[k] = li
        if kind == R.QUAD:        # through each of the two triangles, and just outside each edge
            for li in ids:
                v = R.light_setup(zoo.sd.lights[li])["vert"]
                c = v.mean(axis=0)
                inside = [(v[0] * 2 + v[1] + v[3]) / 4, (v[2] * 2 + v[1] + v[3]) / 4]
                edges = [(v[i] + v[(i + 1) % 4]) / 2 for i in range(4)]
                targets = inside + [c + (e - c) * f for e in edges for f in (0.98, 1.02)]
                for tg in targets:
                    for _ in range(2):
                        k -= 1
                        d[k] = unit32(tg - o[k])
                        self.light[k] = li
        self.inp = {"o": o, "d": d}
        self.finish()

    def ref(self, dt, o, d):
        out = {"hit": np.zeros(N_ITEMS, np.uint8), "t": np.zeros(N_ITEMS, dt), "emit": np.zeros((N_ITEMS, 3), dt),
               "sig": np.zeros((N_ITEMS, 10), np.int8)}
        for li in np.unique(self.light):
            s = self.light == li
            r = R.light_isect(R.light_setup(self.zoo.sd.lights[li], dt), o[s], d[s], dt)
            for k in ("hit", "t", "emit"):
                out[k][s] = r[k]
            out["sig"][s, :r["sig"].shape[1]] = r["sig"]
        return out

    def ask(self, who):
        return who.debug_light_isect(self.light, self.inp["o"], self.inp["d"])


BSDF_KEYS = list(R.KIND_NAMES)
LIGHT_KEYS = [f"{w}:{n}" for w in ("light_dir", "light_isect") for n in R.LIGHT_NAMES]
ALL_KEYS = BSDF_KEYS + ["eval"] + LIGHT_KEYS


def same_bits(a, b):
    """_util's rule: NaNs by position, everything else bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    return compare_images(a.reshape(len(a), -1), b.reshape(len(b), -1))["bitexact"]


def assert_same_answers(a, b, what):
    for k in a:
        assert same_bits(a[k], b[k]), f"{what}: {k} differs"


def measure_m(keys=None):
    """The calibration: worst float32-reference ratio per case (the values of M_REF32)."""
    z = Zoo()
    out = {}
    for key in keys or ALL_KEYS:
        c = z.case(key)
        out[key] = max(v[0] for v in c.worst(c.ref32).values())
    return out


# ---- 1. the reference alone ------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL_KEYS)
def test_reference_inputs_are_decisive_enough(zoo, key):
    c = zoo.case(key)
    share = 1.0 - c.decisive.mean()
    print(f"{key}: non-decisive share {share:.4f}")
    assert share <= MAX_UNDECISIVE


@pytest.mark.parametrize("key", ALL_KEYS)
def test_float32_reference_stays_within_its_measured_ratio(zoo, key):
    """M_REF32 is what the calibration gives, not a stale or padded constant: the float32
    reference's worst ratio is within a factor 2 of the recorded value (numpy's float32 sin, cos,
    exp ... are SIMD variants that differ by an ulp or so between CPUs, so not equal to it)."""
    c = zoo.case(key)
    w = max(v[0] for v in c.worst(c.ref32).values())
    print(f"{key}: float32 reference worst ratio {w:.4g} (recorded {M_REF32[key]:.4g})")
    assert w <= 2 * M_REF32[key]
    assert w >= 0.5 * M_REF32[key] or M_REF32[key] <= 1.0


@pytest.mark.parametrize("key", BSDF_KEYS)
def test_reference_directions_are_unit_length(zoo, key):
    c = zoo.case(key)
    out = c.truth["out"]
    length = np.linalg.norm(out, axis=1)
    if key == "emission":
        assert np.all(out == 0)
        return
    ok = c.truth["valid"] == 1
    if key == "specular_transmission":       # total internal reflection: the zero vector
        ok &= (c.truth["flags"] & R.F_TRANSPARENT) != 0
    # float32 unit inputs are unit to 2^-24 or so; reflection and the frames preserve that
    assert np.max(np.abs(length[ok] - 1.0)) < 1e-6


def test_reference_lambert_pdf_integrates_to_one():
    g = (np.arange(256) + 0.5) / 256
    u0, u1 = (x.reshape(-1) for x in np.meshgrid(g, g))
    n = np.broadcast_to(R.unit(np.array([0.3, -0.5, 0.8])), (len(u0), 3))
    wi = np.broadcast_to(R.unit(np.array([0.1, 0.2, 0.9])), (len(u0), 3))
    mat = {k: np.ones((len(u0), 3)) for k in ("diffuse", "specular", "volume")}
    mat.update(ior=np.ones(len(u0)), roughness=np.ones(len(u0)))
    r = R.bsdf_sample(R.LAMBERT, mat, np.zeros((len(u0), 3, 3)), wi, n, np.stack([u0, u1], 1), np.zeros((len(u0), 2)),
                      np.zeros(len(u0), int))
    # if the map takes the uniform square to the hemisphere with density pdf, then E_u[g / pdf] is
    # the integral of g over the hemisphere: g = pdf gives 1 (the pdf integrates to 1), g = cos gives pi,
    # g = cos^2 gives 2 pi / 3 (this one depends on where the directions land, not on pdf = cos / pi alone)
    cos = np.abs(R.dot(r["out"], n))
    assert np.all(R.dot(r["out"], n) * R.dot(wi, n) > 0)               # the side ray_in is on
    assert abs(np.mean(r["pdf"] / (cos / np.pi)) - 1.0) < 1e-12
    assert abs(np.mean(cos / r["pdf"]) - np.pi) < 1e-9
    assert abs(np.mean(cos * cos / r["pdf"]) - 2 * np.pi / 3) < 1e-3     # a midpoint sum over the disc's square-root rim
    side = R.unit(np.cross(n[0], [1.0, 0.0, 0.0]))
    assert abs(np.mean(R.dot(r["out"], side[None]))) < 1e-6            # no azimuthal bias
    # and the density of the directions themselves: the share landing within 60 degrees of n is
    # the integral of cos / pi over that cap, sin^2(60 deg) = 3/4
    assert abs(np.mean(cos > 0.5) - 0.75) < 1 / 256       # a count over the grid: the cap's rim crosses ~256 cells


def test_reference_glass_probabilities_and_snell(zoo):
    c = zoo.case("glass")
    t = c.truth
    through = (t["flags"] & R.F_TRANSPARENT) != 0
    assert through.sum() > 500 and (~through).sum() > 500
    # the same item asked with sample.y = 0 (reflects: pdf F) and sample.y just under 1 (refracts
    # unless F = 1: pdf 1 - F)
    i = c.inp
    lo, hi = i["sample"].copy(), i["sample"].copy()
    lo[:, 1], hi[:, 1] = 0.0, TOP32
    a = c.ref(np.float64, i["wi"].astype(np.float64), i["n"].astype(np.float64), lo, i["hair"])
    b = c.ref(np.float64, i["wi"].astype(np.float64), i["n"].astype(np.float64), hi, i["hair"])
    both = ((a["flags"] & R.F_TRANSPARENT) == 0) & ((b["flags"] & R.F_TRANSPARENT) != 0) & (a["valid"] == 1)
    assert both.sum() > 1000
    assert np.max(np.abs(a["pdf"][both] + b["pdf"][both] - 1.0)) < 1e-12
    # Snell: sin(theta_t) = eta sin(theta_i) with eta = eta_i / eta_t
    wi, n = R.unit(i["wi"].astype(np.float64)), i["n"].astype(np.float64)
    ior = zoo.table["ior"][i["mat"]]
    eta = np.where(R.dot(wi, n) > 0, 1.0 / ior, ior)
    sin_i = np.linalg.norm(np.cross(wi, n), axis=1) / np.linalg.norm(n, axis=1)
    sin_t = np.linalg.norm(np.cross(b["out"], n), axis=1) / np.linalg.norm(n, axis=1)
    assert np.max(np.abs(sin_t[both] - eta[both] * sin_i[both])) < 1e-12
    assert np.all(np.sign(R.dot(b["out"], n))[both] == -np.sign(R.dot(wi, n))[both])     # the other side


def test_reference_marschner_turns_by_the_transpose(zoo):
    c = zoo.case("marschner")
    i = c.inp
    ok = (c.truth["valid"] == 1) & (i["flags"] == 0)
    wi, n = R.unit(i["wi"].astype(np.float64)), i["n"].astype(np.float64)
    nf = np.where((R.dot(n, wi) > 0)[:, None], n, -n)
    mirror = R.reflect(-wi, nf)
    V = zoo.frames[np.float64][i["obj"]][:, 1]
    alpha = -(5 + 5 * i["hair"][:, 0].astype(np.float64))      # degrees used as radians
    # row vector times glm::rotate(alpha, V) = R(alpha)^T mirror = R(-alpha) mirror
    rt, r = R.rotate(mirror, V, -alpha), R.rotate(mirror, V, alpha)
    assert np.max(np.abs(c.truth["out"][ok] - rt[ok])) < 1e-12
    assert np.median(np.linalg.norm(c.truth["out"][ok] - r[ok], axis=1)) > 0.1


def test_reference_deon_longitudinal_term_integrates_to_the_closed_form():
    """M(theta_r) = csch(a) / (2 v) exp(-sin(theta_i) sin(theta_r) a) J0(cos(theta_i) cos(theta_r) a), a =
    radians(1 / v) = 1 / degrees(v), is what Bsdf.cpp:992-997 computes (J0 where d'Eon has I0, and 2 v
    where d'Eon has 2 degrees(v)).  With integral_0^pi exp(p cos x) J0(q sin x) sin x dx =
    2 sinh(k) / k, k^2 = p^2 - q^2:
        integral M cos(theta_r) d theta_r over [-pi/2, pi/2] = csch(a) sinh(k) / (k v),  k = a sqrt(-cos(2 theta_i)),
    (sinh(k) / k -> sin(|k|) / |k| for cos(2 theta_i) > 0).  At theta_i = pi/2: k = a, the value is
    1 / (a v) = 180 / pi = 57.29577951308232 for every v."""
    n = 200_000
    th = (np.arange(n) + 0.5) / n * np.pi - np.pi / 2
    for beta_deg in (5.0, 7.5, 10.0 - 1e-6):              # the v range used: beta in [5, 10) degrees
        v = np.radians(beta_deg) ** 2
        a = np.radians(1 / v)
        assert abs(a * np.degrees(v) - 1.0) < 1e-12
        for ti in (np.pi / 2, 1.3, 0.9, 0.5, 0.1):
            m = 1 / np.sinh(a) / (2 * v) * np.exp(np.sin(-ti) * np.sin(th) / np.degrees(v)) * \
                R.j0(np.cos(-ti) * np.cos(th) / np.degrees(v))
            got = np.sum(m * np.cos(th)) * (np.pi / n)
            k2 = -np.cos(2 * ti) * a * a
            k = np.sqrt(abs(k2))
            want = (np.sinh(k) if k2 > 0 else np.sin(k)) / k / (np.sinh(a) * v)
            assert abs(got - want) <= 1e-8 * max(1.0, abs(want)), (beta_deg, ti, got, want)
            if ti == np.pi / 2:
                assert abs(want - 57.29577951308232) < 1e-9


# ---- 2. the oracle against the truth (CPU) -----------------------------------------------------
@pytest.mark.parametrize("key", ALL_KEYS)
def test_oracle_against_truth(zoo, key):
    c = zoo.case(key)
    c.check("oracle", c.ask(zoo.oracle))


# ---- 3. / 4. the product against the truth and against the oracle (gpu) -----------------------
@pytest.fixture
def zoo_ctx(hip_ctx, zoo):
    """The shared context with the zoo built on it (other tests put their own scenes there)."""
    if hip_ctx._scene is not zoo.sd:
        hip_ctx.set_scene(zoo.sd)
        hip_ctx.build_accel()
    return hip_ctx


@pytest.mark.gpu
@pytest.mark.parametrize("key", ALL_KEYS)
def test_device_against_truth(zoo_ctx, zoo, key):
    c = zoo.case(key)
    c.check("device", c.ask(zoo_ctx))
    if key in ("lambert", "marschner"):                              # once per compiled instance
        c.check("device (fur instance)", c.ask(zoo_ctx, KINDS_FUR))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ALL_KEYS)
def test_device_equals_oracle(zoo_ctx, zoo, key):
    """Every item, decisive or not, bit for bit (NaNs by position); the narrow instance equals the full one."""
    c = zoo.case(key)
    got = c.ask(zoo_ctx)
    assert_same_answers(got, c.ask(zoo.oracle), f"{key}: device vs oracle")
    if key in ("lambert", "marschner"):
        assert_same_answers(c.ask(zoo_ctx, KINDS_FUR), got, f"{key}: fur instance vs full instance")


# ---- 5. the compile-time kind set ----------------------------------------------------------------
@pytest.mark.gpu
def test_fur_instance_refuses_other_kinds(zoo_ctx, zoo):
    c = zoo.case("glass")
    with pytest.raises(N.KhpError) as e:
        c.ask(zoo_ctx, KINDS_FUR, slice(0, 8))
    assert e.value.status == N.KHP_EINVAL and "kinds_mask" in str(e.value)
    mixed = zoo.case("lambert")                  # one glass item among accepted ones is enough
    i = dict(mixed.inp)
    mat = i["mat"][:64].copy()
    mat[37] = zoo.kind_mats[R.GLASS][0]
    with pytest.raises(N.KhpError) as e:
        zoo_ctx.debug_bsdf_sample(i["obj"][:64], mat, i["wi"][:64], i["n"][:64], i["sample"][:64], i["hair"][:64],
                                  i["flags"][:64], KINDS_FUR)
    assert e.value.status == N.KHP_EINVAL and "item 37" in str(e.value)
    with pytest.raises(N.KhpError):              # a mask that is neither instance
        c.ask(zoo_ctx, 0x3, slice(0, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("device_scene", [False, True])
def test_kind_set_follows_the_materials(hip_ctx, device_scene):
    """A fur-only scene (Lambert + Marschner) runs the kernels with the other kinds compiled
    out; changing one material to each other kind must switch to the full instance (a stale
    kind set would run a compiled-out case), and changing back must give the first frame again."""
    W = H = 16
    sd = S.config2(W, H, n_strands=60)
    frames = []
    old = hip_ctx.params()
    try:
        for kind in [None] + [k for k in range(11) if k not in (R.LAMBERT, R.MARSCHNER)] + [None]:
            mats = list(sd.materials)
            if kind is not None:                 # d'Eon replaces the fibres' BSDF, the others the red wall's
                which = 3 if kind == R.DEON else 1
                m = S.material(N.BSDF_NAMES[kind], diffuse=tuple(mats[which].diffuse), ior=1.5, roughness=0.4)
                sd.materials = mats[:which] + [m] + mats[which + 1:]
            (hip_ctx.set_scene_device if device_scene else hip_ctx.set_scene)(sd)
            hip_ctx.build_accel()
            ref = oracle_ffi.Oracle(sd).render(W, H, 1, 4, threads=4)
            for path_kernel in (0, 1):           # the path kernel, and the wavefront's k_shade
                hip_ctx.set_params(path_kernel=path_kernel)
                img = hip_ctx.render(W, H, 1, 4)
                r = compare_images(img, ref)
                assert r["bitexact"], (kind, path_kernel, r)
            frames.append(ref)
            sd.materials = mats
        assert np.array_equal(frames[0].view(np.uint32), frames[-1].view(np.uint32))
    finally:
        hip_ctx.set_params(path_kernel=old["path_kernel"])


# ---- 6. grazing incidence: where the non-finite values come from -------------------------------
class Grazing:
    """Marschner at grazing incidence: in = normalize(n_perp + eps n) for eps = 2^-1 .. 2^-40 (8 seeded
    normals each), and in = (sqrt(1 - z^2), 0, z) against n = (0, 0, 1) for the 129 float32 values z
    nearest each of 2^-12 and 2^-24 (dot(in, n) == z exactly), and z = 0."""

    def __init__(self, zoo):
        rng = np.random.default_rng(5)
        wi, nn, eps = [], [], []
        for e in range(1, 41):
            n = unit32(rng.normal(size=(8, 3))).astype(np.float64)
            perp = R.unit(np.cross(n, rng.normal(size=(8, 3))))
            wi.append(unit32(perp + 2.0 ** -e * n))
            nn.append(n.astype(np.float32))
            eps += [2.0 ** -e] * 8
        for centre in (2.0 ** -12, 2.0 ** -24):
            z = np.float32(centre)
            for _ in range(64):
                z = np.nextafter(z, np.float32(0))
            zs = []
            for _ in range(129):
                zs.append(z)
                z = np.nextafter(z, np.float32(1))
            zs = np.array(zs, np.float32)
            wi.append(np.stack([np.sqrt(1 - zs.astype(np.float64) ** 2).astype(np.float32), np.zeros_like(zs), zs], 1))
            nn.append(np.broadcast_to(np.float32([0, 0, 1]), (129, 3)))
            eps += [0.0] * 129
        wi.append(np.float32([[1, 0, 0]]))
        nn.append(np.float32([[0, 0, 1]]))
        eps.append(0.0)
        self.wi, self.n, self.eps = np.concatenate(wi), np.concatenate(nn), np.array(eps)
        m = len(self.wi)
        cones = zoo.nt + np.nonzero(zoo.sd.cone_mat == zoo.kind_mats[R.MARSCHNER][0])[0]
        self.inp = {"obj": cones[rng.integers(0, len(cones), m)].astype(np.int32),
                    "mat": np.full(m, zoo.kind_mats[R.MARSCHNER][0], np.int32), "wi": self.wi, "n": self.n,
                    "sample": rng.random((m, 2), np.float32), "hair": rng.random((m, 2), np.float32),
                    "flags": np.zeros(m, np.int32)}
        self.zoo = zoo
        # 1 - h h with h = sin(acos(clamp(dot(normalize(in), normalize(n))))) in the port's float32 arithmetic
        lib = oracle_ffi.load()
        f32 = np.float32

        def dot32(a, b):
            return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

        def normalize32(a):
            return a * (f32(1) / np.sqrt(dot32(a, a)))

        self.one_minus_hh = np.empty(m, np.float32)
        for k in range(m):
            d = dot32(normalize32(self.wi[k]), normalize32(self.n[k]))
            h = f32(lib.ko_sinf(lib.ko_acosf(float(min(max(d, f32(-1)), f32(1))))))
            self.one_minus_hh[k] = f32(1) - h * h

    def ask(self, who):
        i = self.inp
        return who.debug_bsdf_sample(i["obj"], i["mat"], i["wi"], i["n"], i["sample"], i["hair"], i["flags"])

    def check(self, who, got):
        exact_zero = np.sum(self.wi.astype(np.float64) * self.n, axis=1) == 0
        assert exact_zero[-1] and np.all(got["valid"][exact_zero] == 0) and np.all(got["f"][exact_zero] == 0)
        live = got["valid"] == 1
        nonfinite = ~np.isfinite(got["f"]).all(axis=1)
        want = self.one_minus_hh <= 0
        print(f"grazing {who}: {int(nonfinite[live].sum())} of {int(live.sum())} items non-finite; "
              f"largest |dot| among them {np.abs(np.sum(self.wi * self.n, axis=1))[live & nonfinite].max(initial=0):.3g}")
        assert np.array_equal(nonfinite[live], want[live]), np.nonzero(live & (nonfinite != want))[0]
        assert nonfinite.any() and (~nonfinite[self.eps == 0]).any()
        for k in ("out", "pdf", "sample"):          # only f carries the divide
            assert np.isfinite(got[k][live]).all()
        # eps >= 2^-4: finite, and within the Marschner bound of the truth
        far = self.eps >= 2.0 ** -4
        assert not nonfinite[far].any()
        z = self.zoo
        t = z.table
        m = {k: t[k][self.inp["mat"]] for k in ("diffuse", "specular", "volume", "ior", "roughness")}
        fn = lambda **kw: R.bsdf_sample(R.MARSCHNER, m, z.frames[np.float64][self.inp["obj"]], flags_in=self.inp["flags"],
                                        **kw)
        truth, dec, J = R.decisive(fn, {k: self.inp[k] for k in BsdfCase.float_inputs}, BSDF_OUT)
        assert (dec & far).sum() >= 20
        for k in BSDF_OUT:
            r = R.ratio(got[k][dec & far], truth[k][dec & far], J[k][dec & far])
            assert np.all(r <= M["marschner"]), (k, float(np.max(r)))


_GRAZING = []


@pytest.fixture(scope="module")
def grazing(zoo):
    if not _GRAZING:
        _GRAZING.append(Grazing(zoo))
    return _GRAZING[0]


def test_oracle_grazing_incidence(zoo, grazing):
    grazing.check("oracle", grazing.ask(zoo.oracle))


@pytest.mark.gpu
def test_device_grazing_incidence(zoo_ctx, zoo, grazing):
    got = grazing.ask(zoo_ctx)
    grazing.check("device", got)
    assert_same_answers(got, grazing.ask(zoo.oracle), "grazing: device vs oracle")


# ---- 7. the surface at a hit -------------------------------------------------------------------
N_RAYS, RAY_SEED = 2000, 11
SURFACE_SCENES = {
    "config2": lambda: S.config2(32, 32, n_strands=300),
    "config5": lambda: S.config5(32, 32, n_strands=200, torus_grid=12),
    "fur_triangles": None,
}


def fur_triangle_scene():
    """Fur as triangle tubes (fiberToTriangles) on a small icosphere: the triangles carry the fibre's frame."""
    sd = S.SceneData(name="fur_triangles")
    v, n = S.icosphere(1, (0.0, 1.0, 0.0), 1.0)
    sd.add_triangles(v, n, sd.add_material(S.material(diffuse=(0.7, 0.7, 0.7))))
    fm = sd.add_material(S.fiber_material())
    pos, rad = S.fur_on_mesh(v, n, fibers_per_face=2, verts=4, scale=8.0, root_radius=0.03)
    sd.add_fibers(pos, rad, fm, as_triangles=True, resolution=5)
    sd.lights.append(S.point_light((0.0, 4.0, 3.0), (3.0, 3.0, 3.0)))
    sd.cam = S.camera((0.0, 1.0, 4.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 16, 16)
    seg = (np.asarray(pos, np.float64)[:, 1:] - np.asarray(pos, np.float64)[:, :-1]).reshape(-1, 3)
    return sd, len(v), R.unit(seg)


class SurfaceCase:
    def __init__(self, name):
        self.name = name
        if name == "fur_triangles":
            self.sd, self.n_plain, self.fibre_dir = fur_triangle_scene()
        else:
            self.sd, self.n_plain, self.fibre_dir = SURFACE_SCENES[name](), None, None
        self.nt = len(self.sd.tri_v)
        self.rays = {"unaimed": G.unaimed_rays(N_RAYS, RAY_SEED)}
        if len(self.sd.cone_base_r0):
            self.rays["hair_aimed"] = G.hair_aimed_rays(self.sd, N_RAYS, RAY_SEED)
        self.truth = {f: G.Truth(self.sd, *r) for f, r in self.rays.items()}
        self.cs = G.cone_setup(self.sd) if len(self.sd.cone_base_r0) else None
        self.mat_of = np.concatenate([np.asarray(self.sd.tri_mat, np.int64), np.asarray(self.sd.cone_mat, np.int64)])
        self._oracle = None
        self._normals = {}

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_ffi.Oracle(self.sd)
        return self._oracle

    def normal(self, o, d, obj, dt):
        n = np.zeros((len(o), 3), dt)
        tri = obj < self.nt
        if tri.any():
            n[tri] = R.triangle_normal(self.sd.tri_v, self.sd.tri_n, obj[tri], o[tri], d[tri], dt)
        if (~tri).any():
            n[~tri] = R.cone_normal(self.cs, obj[~tri] - self.nt, o[~tri], d[~tri], dt)[0]
        return n

    def normals(self, fam):
        """Per family: the hit rays that are decisive in the geometry truth, their float64 normal,
        its spread J over the jittered rays, and the float32 reference's normal."""
        if fam not in self._normals:
            tr = self.truth[fam]
            idx = np.nonzero(tr.decisive & (tr.obj >= 0))[0]
            obj = tr.obj[idx]
            o32, d32 = tr.orig[idx], tr.d[idx]
            base = self.normal(o32.astype(np.float64), d32.astype(np.float64), obj, np.float64)
            lo, hi = base.copy(), base.copy()
            rng = np.random.default_rng(99)
            for _ in range(R.N_JITTER):
                nj = self.normal(R._jitter(o32, rng), R._jitter(d32, rng), obj, np.float64)
                lo, hi = np.fmin(lo, nj), np.fmax(hi, nj)
            self._normals[fam] = (idx, obj, base, hi - lo, self.normal(o32, d32, obj, np.float32))
        return self._normals[fam]

    def check(self, who, fam, got):
        tr = self.truth[fam]
        idx, obj, truth, J, _ = self.normals(fam)
        keep = got["obj"][idx] == obj                       # the rays whose object matches the truth
        assert keep.mean() > 0.98
        idx, obj, truth, J = idx[keep], obj[keep], truth[keep], J[keep]
        assert np.array_equal(got["mat"][idx], self.mat_of[obj])
        for kind, sel in (("triangle", obj < self.nt), ("cone", obj >= self.nt)):
            if not sel.any():
                continue
            r = R.ratio(got["n"][idx][sel], truth[sel], J[sel])
            k = int(np.argmax(r))
            print(f"{self.name} {fam} {who}: {int(sel.sum())} {kind} normals, worst ratio {r[k]:.3g} "
                  f"(bound {M['normal:' + kind]:.3g})")
            assert r[k] <= M["normal:" + kind], (f"ray {idx[sel][k]}: origin {tr.orig[idx[sel][k]].tolist()} direction "
                                                 f"{tr.d[idx[sel][k]].tolist()} object {obj[sel][k]}: normal "
                                                 f"{got['n'][idx[sel][k]].tolist()}, truth {truth[sel][k].tolist()}")
        # A frustum's normal leans along the axis by the same amount everywhere: n . axis = s / sqrt(1 + s^2),
        # s = (r0 - r1) / h, wherever the hit is -- so this holds to rounding even where the float32
        # quadratic's t (and with it the radial direction above) is coarse.  Rounding: the radial vector
        # Q - (Q . V) V - base, of length r, carries a few roundings of size ulp32(|Q|), which leak
        # |Q| / r ulps into n . axis; 8 of those, plus 8 ulps for the two normalisations and the sum.
        cone = obj >= self.nt
        if cone.any():
            base, axis, h, r0, r1 = (x[obj[cone] - self.nt] for x in self.cs)
            s = (r0 - r1) / h
            Q = tr.orig[idx][cone].astype(np.float64) + tr.t[idx][cone, None] * tr.d[idx][cone].astype(np.float64)
            r_hit = r0 - s * np.sum((Q - base) * axis, axis=1)
            lean = np.sum(got["n"][idx][cone] * axis, axis=1)
            bound = 8 * 2.0 ** -23 * (np.linalg.norm(Q, axis=1) / r_hit + 1.0)
            off = np.abs(lean - s / np.sqrt(1 + s * s)) / bound
            print(f"{self.name} {fam} {who}: the normals' axial lean is within {off.max():.3g} of its rounding bound "
                  f"(slopes {s.min():.3g} .. {s.max():.3g}, median bound {np.median(bound):.3g})")
            assert off.max() <= 1.0, f"ray {idx[cone][np.argmax(off)]}: n . axis = {lean[np.argmax(off)]}"
        # the hair frame: orthonormal, V along the cone's axis / the fibre
        framed = obj >= (self.nt if self.n_plain is None else self.n_plain)
        f = got["uvw"][idx][framed].astype(np.float64)
        if framed.any():
            gram = np.einsum("nij,nkj->nik", f, f)
            assert np.max(np.abs(gram - np.eye(3))) <= FRAME_ULPS
            if self.n_plain is None:
                axis = self.cs[1][obj[framed] - self.nt]
            else:                                             # 2 res^2 = 50 triangles per fibre segment
                axis = self.fibre_dir[(obj[framed] - self.n_plain) // 50]
            assert np.max(np.linalg.norm(np.cross(f[:, 1], axis), axis=1)) <= FRAME_ULPS
            assert np.all(np.sum(f[:, 1] * axis, axis=1) > 0)
        assert np.all(got["uvw"][idx][~framed] == 0)          # plain triangles carry no frame
        return int(framed.sum())


_SURFACES = {}


@pytest.fixture(scope="module", params=list(SURFACE_SCENES))
def surface(request):
    if request.param not in _SURFACES:
        _SURFACES[request.param] = SurfaceCase(request.param)
    return _SURFACES[request.param]


def measure_m_normals():
    out = {"normal:cone": 0.0, "normal:triangle": 0.0}
    for name in SURFACE_SCENES:
        c = SurfaceCase(name)
        for fam in c.rays:
            idx, obj, truth, J, n32 = c.normals(fam)
            r = R.ratio(n32, truth, J)
            for kind, sel in (("triangle", obj < c.nt), ("cone", obj >= c.nt)):
                if sel.any():
                    out["normal:" + kind] = max(out["normal:" + kind], float(r[sel].max()))
    return out


def test_float32_reference_normals_stay_within_their_measured_ratio(surface):
    for fam in surface.rays:
        idx, obj, truth, J, n32 = surface.normals(fam)
        r = R.ratio(n32, truth, J)
        for kind, sel in (("triangle", obj < surface.nt), ("cone", obj >= surface.nt)):
            if sel.any():
                print(f"{surface.name} {fam}: float32 reference {kind} normals worst ratio {r[sel].max():.4g} "
                      f"(recorded {M_REF32['normal:' + kind]:.4g})")
                assert r[sel].max() <= 2 * M_REF32["normal:" + kind]      # per scene and family; the record is the worst of all


def test_reference_cone_normal_is_perpendicular_to_the_surface(surface):
    """The gradient normal against the frustum's two tangents at the hit: the generator line
    (towards the apex of the full cone) and the circle's tangent."""
    if "hair_aimed" not in surface.rays:       # the triangle-fur scene has no cone
        return
    idx, obj, n, _, _ = surface.normals("hair_aimed")
    cone = obj >= surface.nt
    c = obj[cone] - surface.nt
    tr = surface.truth["hair_aimed"]
    base, axis, h, r0, r1 = (x[c] for x in surface.cs)
    p = tr.orig[idx][cone].astype(np.float64) + tr.t[idx][cone, None] * tr.d[idx][cone].astype(np.float64) - base
    y = np.sum(p * axis, axis=1)
    radial = R.unit(p - y[:, None] * axis)
    generator = R.unit(axis * h[:, None] + radial * (r1 - r0)[:, None])
    assert np.max(np.abs(np.sum(n[cone] * generator, axis=1))) < 1e-6      # t is a float64 root: 1e-9 / r
    assert np.max(np.abs(np.sum(n[cone] * np.cross(axis, radial), axis=1))) < 1e-6
    assert np.all(np.sum(n[cone] * radial, axis=1) > 0)


def test_oracle_surface(surface):
    framed = 0
    for fam, rays in surface.rays.items():
        framed += surface.check("oracle", fam, surface.oracle.debug_surface(rays[0], rays[1]))
    assert framed >= 200


@pytest.fixture
def surface_ctx(hip_ctx, surface):
    if hip_ctx._scene is not surface.sd:
        hip_ctx.set_scene(surface.sd)
        hip_ctx.build_accel()
    return hip_ctx


@pytest.mark.gpu
def test_device_surface(surface_ctx, surface):
    for fam, rays in surface.rays.items():
        surface.check("device", fam, surface_ctx.debug_surface(rays[0], rays[1]))


@pytest.mark.gpu
def test_device_surface_equals_oracle(surface_ctx, surface):
    for fam, rays in surface.rays.items():
        assert_same_answers(surface_ctx.debug_surface(rays[0], rays[1]), surface.oracle.debug_surface(rays[0], rays[1]),
                            f"{surface.name} {fam}: device vs oracle")
