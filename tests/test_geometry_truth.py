"""Ray/fur intersection against a float64 brute-force truth (tests/_geomref.py).

The parity tests pin libkirk_hip.so to the oracle bit for bit; nothing there
pins either of them to the geometry.  Here the oracle (CPU) and the product
(every traversal kernel, `gpu`) answer seeded rays in two fur scenes, and the
answers are compared with a float64 brute force over every object that knows
no BVH and no visit order: an object bound that is too tight, a wrong prune or
a slip in the tapered-cone quadratic shows here even where the oracle, the host
build, the device build and all kernels reproduce it alike.

Only *decisive* rays count (all three of _geomref's thinner / exact / fatter
variants agree); what remains are grazing hits, KIRK's 1e-4 triangle-edge
crack and the float32 quadratic's resolution (eps32 |P|^2 against r^2: a strand
of radius 0.002 is resolved at 1 unit and invisible from 10).

One class of decisive disagreement is KIRK's own and is tolerated, counted and
capped (test_oracle_kat.test_second_root_overwrites_a_nearer_hit):
Cylinder::closestIntersection falls from a root t1 outside the cone's height
window to t2 without checking t2 <= tMax, and Container::closestIntersection-
WithCandidates lets that later candidate overwrite the leaf's nearer hit.
"""
import numpy as np
import pytest

import _geomref as G
import oracle_ffi
from ba_pathtracing_fur_amd import scenes as S

N_RAYS = 2000
SEED = 11
SCENES = {
    "config2": (lambda: S.config2(32, 32, n_strands=300), 2710),
    "config5": (lambda: S.config5(32, 32, n_strands=200, torus_grid=12), 22570),
}
FAMILIES = ("hair_aimed", "unaimed")
MAX_UNDECISIVE = {"hair_aimed": 0.20, "unaimed": 0.05}   # conditions on the inputs, not on the code under test
MIN_CONE_SHARE = 0.30          # of family (a)'s decisive rays
MAX_SECOND_ROOT = 0.005        # tolerated second-root overwrites, share of the decisive rays
# kernel settings of the batch queries: (trace_kernels, wide_from); 0 = the query kernel (wide_from unused)
KERNELS = [(0, None), (1, 0), (1, 2), (2, 0), (2, 2)]
# A stored float32 box against float64 geometry: the frame vectors, the corner
# sums and the base add round a few times each (Cylinder::computeBounds).
BOX_ULPS = 8


class Case:
    def __init__(self, name):
        make, n_objects = SCENES[name]
        self.name = name
        self.sd = make()
        assert self.sd.n_objects == n_objects
        self.nt = len(self.sd.tri_v)
        self.truth = {}
        for fam in FAMILIES:
            rays = G.hair_aimed_rays(self.sd, N_RAYS, SEED) if fam == "hair_aimed" else G.unaimed_rays(N_RAYS, SEED)
            self.truth[fam] = G.Truth(self.sd, *rays)
        self.points = G.object_points(self.sd)
        self._oracle = None

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_ffi.Oracle(self.sd)
            boxes, first, count, ids, _ = self._oracle.bvh()
            self.leaf_of = np.full(self.sd.n_objects, -1, np.int64)
            self.slot_of = np.full(self.sd.n_objects, -1, np.int64)
            for k in np.nonzero(count > 0)[0]:
                self.leaf_of[ids[first[k]:first[k] + count[k]]] = k
            self.slot_of[ids] = np.arange(len(ids))
        return self._oracle


@pytest.fixture(scope="module", params=list(SCENES))
def case(request):
    """One scene with its float64 reference, computed once and shared by the CPU and the GPU tests."""
    return Case(request.param)


# ---- the reference alone --------------------------------------------------------------------
def test_reference_inputs_are_decisive_enough(case):
    for fam in FAMILIES:
        tr = case.truth[fam]
        undecisive = 1.0 - tr.decisive.mean()
        any_undecisive = 1.0 - tr.any_decisive.mean()
        cone_share = ((tr.obj >= case.nt) & tr.decisive).sum() / tr.decisive.sum()
        print(f"{case.name} {fam}: undecisive {undecisive:.4f} (any-hit {any_undecisive:.4f}), "
              f"cone share of decisive rays {cone_share:.3f}")
        assert undecisive <= MAX_UNDECISIVE[fam]
        if fam == "hair_aimed":
            assert cone_share >= MIN_CONE_SHARE


def test_matrix_form_equals_textbook_moeller_trumbore(case):
    """_geomref tests triangles through matrix products over the ray's moment; the
    textbook per-ray form must give the same triangle and t (float64 rounding apart)."""
    tr = case.truth["unaimed"]
    checked = 0
    for i in range(0, N_RAYS, 20):
        t, k = G.triangle_hit_plain(case.sd, tr.orig[i], tr.d[i])
        if tr.obj[i] >= case.nt:          # a cone is closer: the triangle, if any, lies behind it
            assert not t < tr.t[i] - 1e-9
            continue
        assert k == tr.obj[i], (i, k, tr.obj[i])
        if k >= 0:
            assert abs(t - tr.t[i]) <= 1e-9 * max(1.0, t)
            checked += 1
    assert checked >= 5


def test_cone_roots_lie_on_the_frustum(case):
    """The reference's cone hits, substituted back: the point is at the frustum's
    radius from the axis, inside the height window, for rays of family (a)."""
    tr = case.truth["hair_aimed"]
    base, axis, h, r0, r1 = G.cone_setup(case.sd)
    i = np.nonzero(tr.obj >= case.nt)[0]
    c = tr.obj[i] - case.nt
    assert len(i) > 300
    p = tr.orig[i].astype(np.float64) + tr.t[i, None] * tr.d[i].astype(np.float64) - base[c]
    y = np.sum(p * axis[c], axis=1)
    rad = np.linalg.norm(p - y[:, None] * axis[c], axis=1)
    want = r0[c] + (r1[c] - r0[c]) * y / h[c]
    assert np.all((y >= -1e-12) & (y <= h[c] + 1e-12))
    assert np.max(np.abs(rad - want)) < 1e-9


# ---- answers against the reference -------------------------------------------------------------
def _ray(tr, i):
    return (f"ray {i}: origin {tr.orig[i].tolist()} direction {tr.d[i].tolist()} tmax {float(tr.tmax[i])!r}; "
            f"truth object {int(tr.obj[i])} at t {float(tr.t[i])!r}")


def _is_second_root_overwrite(case, tr, i, t, obj):
    """KIRK's documented overwrite: the returned object is a cone that
    shares the truth's leaf and follows it there; its near root is no hit (outside its
    height window) and not beyond the truth's t, so the cone is examined and falls
    through to its far root; the returned t is that far root, which is a hit of the
    cone and not nearer than the truth."""
    k, k0 = int(obj[i]), int(tr.obj[i])
    if k < case.nt or k0 < 0 or k == k0:
        return False
    case.oracle
    if case.leaf_of[k] != case.leaf_of[k0] or case.slot_of[k] < case.slot_of[k0]:
        return False
    base, axis, h, r0, r1 = G.cone_setup(case.sd)
    c = k - case.nt
    lo, hi, ok_lo, ok_hi = G.cone_roots(base[c], axis[c], h[c], r0[c], r1[c], tr.orig[i].astype(np.float64),
                                        tr.d[i].astype(np.float64))
    tol = G.tau(tr.t[i])
    return bool(not ok_lo and ok_hi and lo <= tr.t[i] + tol and abs(float(t[i]) - hi) <= G.tau(hi)
                and hi >= tr.t[i] - tol)


def check_against_truth(case, fam, who, t, obj, any_hit):
    """Every decisive ray: the truth's object at the truth's t within tau, and the
    truth's any-hit answer; second-root overwrites apart, which are counted and capped."""
    tr = case.truth[fam]
    D = tr.decisive
    miss = obj < 0
    with np.errstate(invalid="ignore"):
        t_ok = np.where(tr.obj < 0, miss, np.abs(t.astype(np.float64) - tr.t) <= G.tau(tr.t))
    bad = np.nonzero(D & ((obj != tr.obj) | ~t_ok))[0]
    tolerated = [i for i in bad if _is_second_root_overwrite(case, tr, i, t, obj)]
    same = D & (obj == tr.obj) & (tr.obj >= 0)
    worst = float(np.max(np.abs(t[same] - tr.t[same]) / np.maximum(1.0, tr.t[same])))
    any_bad = np.nonzero(tr.any_decisive & (any_hit != tr.any))[0]
    print(f"{case.name} {fam} {who}: {int(D.sum())} decisive rays, worst |t - t64| / max(1, t) {worst:.3e}, "
          f"second-root overwrites {len(tolerated)} {[int(i) for i in tolerated]}, other mismatches "
          f"{len(bad) - len(tolerated)}, any-hit mismatches {len(any_bad)} of {int(tr.any_decisive.sum())}")
    for i in bad:
        if i not in tolerated:
            raise AssertionError(f"{case.name} {fam} {who}: closest hit object {int(obj[i])} at t {float(t[i])!r}; "
                                 + _ray(tr, i))
    for i in any_bad:
        raise AssertionError(f"{case.name} {fam} {who}: any-hit {bool(any_hit[i])}; " + _ray(tr, i))
    assert len(tolerated) <= MAX_SECOND_ROOT * D.sum()
    assert same.sum() > 0.05 * N_RAYS


@pytest.mark.parametrize("fam", FAMILIES)
def test_oracle_against_truth(case, fam):
    tr = case.truth[fam]
    t, obj, *_ = case.oracle.trace_closest(tr.orig, tr.d)
    check_against_truth(case, fam, "oracle", t, obj, case.oracle.trace_any(tr.orig, tr.d, tr.tmax))


@pytest.mark.gpu
@pytest.mark.parametrize("trace_kernels,wide_from", KERNELS, ids=[f"tk{a}-wide{b}" for a, b in KERNELS])
def test_product_against_truth(hip_ctx, case, trace_kernels, wide_from):
    """libkirk_hip.so's batch queries against the float64 reference directly (not
    through the oracle): the query kernel (trace_kernels 0) and the renderer's own
    traversal kernels (1 instrumented, 2 production) on the 64-B records
    (wide_from 2) and on the two-level records (wide_from 0)."""
    hip_ctx.set_scene(case.sd)
    hip_ctx.build_accel()
    kw = dict(trace_kernels=trace_kernels) if wide_from is None else dict(trace_kernels=trace_kernels,
                                                                          wide_from=wide_from)
    got = {}
    old = hip_ctx.set_params(**kw)
    try:
        for fam in FAMILIES:
            tr = case.truth[fam]
            t, obj, _ = hip_ctx.trace_closest(tr.orig, tr.d)
            got[fam] = (t, obj, hip_ctx.trace_any(tr.orig, tr.d, tr.tmax))
    finally:
        hip_ctx.set_params(**old)
    for fam in FAMILIES:
        check_against_truth(case, fam, f"product tk{trace_kernels} wide{wide_from}", *got[fam])


# ---- bounds containment -----------------------------------------------------------------------
def _box_tol(x):
    return BOX_ULPS * 2.0 ** -24 * np.maximum(1.0, np.abs(x.astype(np.float64)))


def _assert_points_inside(points, lo, hi, what):
    """points (n, P, 3) float64 inside the float32 boxes [lo, hi] (n, 3) up to the boxes' own rounding."""
    below = points < (lo.astype(np.float64) - _box_tol(lo))[:, None]
    above = points > (hi.astype(np.float64) + _box_tol(hi))[:, None]
    out = np.nonzero((below | above).any(axis=(1, 2)))[0]
    assert len(out) == 0, f"{what}: {len(out)} boxes miss their geometry, first {int(out[0])}: box " \
                          f"{lo[out[0]].tolist()} .. {hi[out[0]].tolist()}"


def _preorder_right(count):
    """Right child of every interior node of a tree stored in DFS preorder (left child = i + 1)."""
    n = len(count)
    size = np.ones(n, np.int64)
    right = np.full(n, -1, np.int64)
    for i in range(n - 1, -1, -1):
        if count[i] == 0:
            r = i + 1 + size[i + 1]
            right[i] = r
            size[i] = 1 + size[i + 1] + size[r]
    assert size[0] == n
    return right


def check_tree_contains(case, boxes, first, count, ids, obj_bounds=None):
    """Every leaf box contains its members (their float32 bounds exactly where given,
    and their float64 geometry); every interior box contains both children exactly."""
    n_obj = case.sd.n_objects
    assert sorted(ids.tolist()) == list(range(n_obj))
    leaves = np.nonzero(count > 0)[0]
    assert count[leaves].sum() == n_obj
    slot_leaf = np.repeat(leaves, count[leaves])
    slots = np.concatenate([np.arange(first[k], first[k] + count[k]) for k in leaves])
    member = ids[slots]
    lo, hi = boxes[slot_leaf, :3], boxes[slot_leaf, 3:]
    _assert_points_inside(case.points[member], lo, hi, "leaf boxes")
    if obj_bounds is not None:
        assert np.all(lo <= obj_bounds[member, :3]) and np.all(hi >= obj_bounds[member, 3:6])
    right = _preorder_right(count)
    interior = np.nonzero(count == 0)[0]
    assert len(interior) > 0
    for child in (interior + 1, right[interior]):
        assert np.all(boxes[interior, :3] <= boxes[child, :3]) and np.all(boxes[interior, 3:] >= boxes[child, 3:])


def test_object_bounds_contain_the_geometry(case):
    """Cylinder::computeBounds / the triangle ctor's box against 64 float64 points
    on each rim circle of every frustum, and every triangle's vertices."""
    b = case.oracle.object_bounds()
    _assert_points_inside(case.points, b[:, :3], b[:, 3:6], "object bounds")


def test_tree_boxes_contain_their_members(case):
    boxes, first, count, ids, _ = case.oracle.bvh()
    check_tree_contains(case, boxes, first, count, ids, case.oracle.object_bounds())


@pytest.mark.gpu
def test_device_tree_boxes_contain_their_members(hip_ctx, case):
    """The same containment on the tree the device built (khp_read_bvh), against the
    float64 geometry."""
    hip_ctx.set_scene(case.sd)
    hip_ctx.build_accel()
    b = hip_ctx.read_bvh()
    check_tree_contains(case, b["boxes"], b["first"], b["count"], b["ids"])


# ---- the second-root overwrite on the device (twin of test_oracle_kat's known-answer scene) ------
@pytest.mark.gpu
@pytest.mark.parametrize("trace_kernels,wide_from", KERNELS, ids=[f"tk{a}-wide{b}" for a, b in KERNELS])
@pytest.mark.parametrize("lower_first", [True, False], ids=["lower_first", "upper_first"])
def test_second_root_overwrite_on_device(hip_ctx, lower_first, trace_kernels, wide_from):
    """SURVEY A.16 through every traversal kernel, bit-equal to the oracle: two
    collinear cylinders in one leaf, a ray across the joint; the later candidate
    wins, with its far root when it is the upper cylinder.  And the any-hit form:
    the upper cylinder alone reports a hit although its only hit lies beyond tmax."""
    import test_oracle_kat as K
    kw = dict(trace_kernels=trace_kernels) if wide_from is None else dict(trace_kernels=trace_kernels,
                                                                          wide_from=wide_from)
    for sd, tmax in ((K._joint_cylinders(lower_first), 10.0), (K._joint_cylinders(lower_first, only_upper=True),
                                                                K.JOINT_BETWEEN_ROOTS)):
        o = oracle_ffi.Oracle(sd)
        want_t, want_obj, want_uv, _, _ = o.trace_closest([K.JOINT_ORIGIN], [K.JOINT_DIR])
        want_any = o.trace_any([K.JOINT_ORIGIN], [K.JOINT_DIR], [tmax])
        hip_ctx.set_scene(sd)
        hip_ctx.build_accel()
        old = hip_ctx.set_params(**kw)
        try:
            t, obj, uv = hip_ctx.trace_closest([K.JOINT_ORIGIN], [K.JOINT_DIR])
            a = hip_ctx.trace_any([K.JOINT_ORIGIN], [K.JOINT_DIR], [tmax])
        finally:
            hip_ctx.set_params(**old)
        assert obj[0] == want_obj[0] and t.view(np.uint32)[0] == want_t.view(np.uint32)[0]
        assert np.array_equal(uv, want_uv) and a[0] == want_any[0]


@pytest.mark.gpu
@pytest.mark.parametrize("trace_kernels,wide_from", KERNELS[:3], ids=[f"tk{a}-wide{b}" for a, b in KERNELS[:3]])
def test_node_entered_at_the_current_best_on_device(hip_ctx, trace_kernels, wide_from):
    """Twin of test_oracle_kat.test_node_entered_at_the_current_best_is_still_visited
    for the kernels that count KIRK's visits: a node entered exactly at the best hit is
    visited (tmin > best skips, tmin == best does not): 3 nodes, 4 candidates."""
    import test_oracle_kat as K
    hip_ctx.set_scene(K._entered_at_the_best_scene())
    hip_ctx.build_accel()
    kw = dict(trace_kernels=trace_kernels) if wide_from is None else dict(trace_kernels=trace_kernels,
                                                                          wide_from=wide_from)
    old = hip_ctx.set_params(**kw)
    try:
        t, obj, _ = hip_ctx.trace_closest([K.PRUNE_ORIGIN], [K.PRUNE_DIR])
        st = hip_ctx.stats()
    finally:
        hip_ctx.set_params(**old)
    assert obj[0] == 0 and t[0] == np.float32(3.0)
    assert (st["node_visits"], st["prim_tests"]) == (3, 4)
