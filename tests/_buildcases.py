"""Adversarial scenes for the BVH build, shared by tests/test_build_truth.py (CPU)
and tests/test_gpu_build_truth.py (GPU); DESIGN.md §20 lists what each one targets.

Every case is the smallest scene that still reaches the code it is named for.
CASES maps a name to a Case; Case.scene() builds the SceneData (cached), and
Case.reference() the tree of tests/_bvhref.py over the host's object bounds
(cached, never modified).
"""
import numpy as np

import _bvhref as R
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S

F = np.float32
N_RAYS = 256
RAY_SEED = 20


class Case:
    def __init__(self, make, trace_truth=True, signed_zero=False, why=""):
        self.make, self.trace_truth, self.signed_zero, self.why = make, trace_truth, signed_zero, why
        self._sd = self._host = self._ref = self._rays = None

    def scene(self):
        if self._sd is None:
            self._sd = self.make()
        return self._sd

    def host(self):
        if self._host is None:
            self._host = N.host_build(self.scene())
        return self._host

    def reference(self):
        if self._ref is None:
            self._ref = R.build(self.host()["bounds"])
        return self._ref

    def rays(self):
        if self._rays is None:
            self._rays = make_rays(self.host()["bounds"], N_RAYS, RAY_SEED)
        return self._rays


# ---- scene pieces ------------------------------------------------------------------------------
def base():
    sd = S.SceneData(name="build_truth")
    sd.add_material(S.material())
    sd.cam = S.camera((0, 0, 3), (0, 0, -1), (0, 1, 0), 16, 16)
    return sd


# offsets that sum to zero, in quarters: the centroid ((A + B) + C) / 3 of a triangle at a
# centre with few mantissa bits is that centre exactly
OFF = np.array([[0.25, 0.0, -0.25], [-0.25, 0.25, 0.0], [0.0, -0.25, 0.25]], np.float64)


def tris(sd, centers, size=0.01):
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    s = np.broadcast_to(np.asarray(size, np.float64).reshape(-1, 1, 1), (len(c), 1, 1))
    v = (c[:, None, :] + 4.0 * s * OFF[None]).astype(F)
    n = np.broadcast_to(F([0, 0, 1]), v.shape).copy()
    sd.add_triangles(v, n, 0)
    return sd


def cones(sd, base_pts, axis, r0, r1):
    b = np.asarray(base_pts, np.float64).reshape(-1, 3)
    a = b + np.asarray(axis, np.float64)
    sd.add_cones(np.c_[b, np.full(len(b), r0)].astype(F), np.c_[a, np.full(len(b), r1)].astype(F), 0)
    return sd


_CLOUD = np.random.default_rng(1).uniform(-1, 1, (20481, 3))


def count_case(n):
    return lambda: tris(base(), _CLOUD[:n])


def two_clusters(n_left, n_right):
    """Two clouds far apart on x: the root's cheapest plane lies in the gap, so its
    children hold exactly n_left and n_right objects (test_build_truth checks that)."""
    def make():
        rng = np.random.default_rng(n_left)
        a = rng.uniform(0, 1, (n_left, 3))
        b = rng.uniform(0, 1, (n_right, 3)) + [30.0, 0, 0]
        return tris(base(), np.r_[a, b])
    return make


def lattice(n, perm=(0, 1, 2)):
    def make():
        g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
        return tris(base(), g[:, perm].astype(np.float64), 0.125)
    return make


def bin_of(c, cbmin, cbmax):
    """KIRK's `int bin_id = k * (c - cbmin)` in float32, and the float32 product."""
    k = (F(16) * (F(1.0) - F(0.1))) / (F(cbmax) - F(cbmin))
    p = k * (F(c) - F(cbmin))
    return int(p), p


def bin_edge_centres(cbmin, cbmax):
    """For every plane j = 1..14: the largest float32 c whose product k * (c - cbmin) is
    below j, the smallest whose product is j or above (the product is exactly j where
    float32 can reach it), and its successor; found by walking float32 neighbours."""
    cbmin, cbmax = F(cbmin), F(cbmax)
    k = (F(16) * (F(1.0) - F(0.1))) / (cbmax - cbmin)
    out, exact = [], 0
    for j in range(1, 15):
        c = F(cbmin + F(j) / k)
        while bin_of(c, cbmin, cbmax)[1] >= j:
            c = np.nextafter(c, F(-np.inf), dtype=F)
        while bin_of(np.nextafter(c, F(np.inf), dtype=F), cbmin, cbmax)[1] < j:
            c = np.nextafter(c, F(np.inf), dtype=F)
        up = np.nextafter(c, F(np.inf), dtype=F)
        up2 = np.nextafter(up, F(np.inf), dtype=F)
        assert bin_of(c, cbmin, cbmax)[0] == j - 1 and bin_of(up, cbmin, cbmax)[0] == j
        exact += bin_of(up, cbmin, cbmax)[1] == j
        out += [c, up, up2]
    return np.array(out, F), exact


def bin_edges(cbmin, cbmax, filler):
    """Centroids on x at the bin edges of [cbmin, cbmax]; y and z vary a little (one cell of
    a grid each, so that no two triangles overlap when seen along x) so that the box is worth
    splitting and x is the axis of the first splits.  `filler` more objects at random x take
    the root into the level phase."""
    def make():
        xs, _ = bin_edge_centres(cbmin, cbmax)
        rng = np.random.default_rng(int(filler) + 7)
        xs = np.r_[F(cbmin), xs, F(cbmax), rng.uniform(cbmin, cbmax, filler).astype(F)]
        xs = xs[rng.permutation(len(xs))]
        span = float(cbmax) - float(cbmin)
        g = int(np.ceil(np.sqrt(len(xs))))
        cell = 0.3 * span / g
        yz = (np.c_[np.arange(len(xs)) // g, np.arange(len(xs)) % g] + 0.25) * cell
        # cones along y: the centroid base + (apex - base) * 0.4f has the base's x exactly (a
        # triangle's ((A + B) + C) / 3 cannot reach every float32)
        # (hair-thin, as the decisiveness rule of tests/_geomref.py assumes)
        r0 = min(0.004, 0.15 * cell)
        return cones(base(), np.c_[xs.astype(np.float64), yz], [0, min(0.03, 0.6 * cell), 0], r0, 0.75 * r0)
    return make


def geometric_centres(n, ratio, axes, top=2.0 ** 55):
    """Centres s_i * direction, s_i = top * ratio^-i; `axes` of the direction's components
    are of order one, the others a hundredth (and jittered, so every box is worth
    splitting).  float32 leaves a chain about 120 binades before box areas overflow
    or vanish, so a ratio that peels one object per split (6) reaches depth 40 and a
    depth of 64 needs a smaller one, under which a split peels a few objects."""
    rng = np.random.default_rng(5)
    s = top * float(ratio) ** -np.arange(n)
    d = np.ones((n, 3))
    d[:, axes:] = 0.01 * rng.uniform(0.5, 1.0, (n, 3 - axes))
    d[:, 1:axes] *= [0.75, 0.5][:axes - 1]
    return s[:, None] * d, s


def lopsided(n, ratio, axes, top=2.0 ** 55):
    def make():
        c, s = geometric_centres(n, ratio, axes, top)
        return tris(base(), c, 0.05 * s)
    return make


def chain_depth(n, ratio, axes, top=2.0 ** 55):
    """Depth of the reference's tree over the flattened chain of n objects."""
    return R.build(N.host_build(lopsided(n, ratio, axes, top)())["bounds"])["depth"]


PEEL_N, PEEL_TOP = 40, 2.0 ** 60
_memo = {}


def peeling_ratio(axes):
    """The smallest ratio among a few candidates under which every split peels exactly one
    object (depth n - 1 on PEEL_N objects), from the reference."""
    if ("peel", axes) not in _memo:
        for ratio in (2, 3, 4, 5, 6, 8):
            if chain_depth(PEEL_N, ratio, axes, PEEL_TOP) == PEEL_N - 1:
                _memo["peel", axes] = ratio
                break
        else:
            raise AssertionError("no candidate ratio peels one object per split")
    return _memo["peel", axes]


def depth_limit_sizes():
    """(ratio, n63, n64) for the one-axis chain, from the reference: n64 is the smallest n
    whose tree has depth 64 and n63 the largest n below it whose tree has depth 63 (past
    the range of float32 the chain's tail collapses and the depth falls again); the
    first ratio among a few for which both exist."""
    if "limit" not in _memo:
        for ratio in (3, 2.5, 2):
            depth = {n: chain_depth(n, ratio, 1) for n in range(90, 170, 1)}
            n64 = [n for n, d in depth.items() if d == 64]
            n63 = [n for n, d in depth.items() if d == 63 and n64 and n < min(n64)]
            if n63 and n64:
                _memo["limit"] = (ratio, max(n63), min(n64))
                break
        else:
            raise AssertionError("no chain of depth 63 and 64 among the candidates")
    return _memo["limit"]


def depth_case(which):
    def make():
        ratio, n63, n64 = depth_limit_sizes()
        return lopsided(n63 if which == 63 else n64, ratio, 1)()
    return make


def mixed_extents():
    rng = np.random.default_rng(11)
    sd = base()
    floor = np.array([[[-100, 0, -100], [100, 0, -100], [100, 0, 100]],
                      [[-100, 0, -100], [100, 0, 100], [-100, 0, 100]]], F)
    sd.add_triangles(floor, np.broadcast_to(F([0, 1, 0]), floor.shape).copy(), 0)
    tris(sd, rng.uniform(-1, 1, (1500, 3)) + [0, 1.5, 0], 0.004)
    b = rng.uniform(-1, 1, (1500, 3)) + [0, 1.5, 0]
    d = rng.normal(size=(1500, 3))
    d *= 0.02 / np.linalg.norm(d, axis=1, keepdims=True)
    sd.add_cones(np.c_[b, np.full(1500, 0.002)].astype(F), np.c_[b + d, np.full(1500, 0.001)].astype(F), 0)
    return sd


def parallel_hair():
    """Straight strands along y: the ten cones of a strand share x and z, so the centroid
    boxes of sub-ranges are flat (leaves larger than two)."""
    rng = np.random.default_rng(12)
    roots = np.c_[rng.uniform(-1, 1, 120), np.zeros(120), rng.uniform(-1, 1, 120)]
    seg = np.arange(10)[None, :, None] * np.array([0, 0.05, 0])[None, None]
    b = (roots[:, None, :] + seg).reshape(-1, 3)
    return cones(base(), b, [0, 0.05, 0], 0.004, 0.003)


def duplicates():
    rng = np.random.default_rng(13)
    c = np.r_[rng.uniform(-1, 1, (1000, 3)), np.tile([[0.25, -0.5, 0.125]], (4000, 1))]
    return tris(base(), c[rng.permutation(5000)])


def planar_beside_cloud():
    rng = np.random.default_rng(14)
    flat = np.c_[rng.uniform(0, 1, (300, 2)), np.full(300, 0.5)]
    return tris(base(), np.r_[flat, rng.uniform(0, 1, (300, 3)) + [4, 0, 0]])


def signed_zeros(neg_first):
    """Triangles lying in a coordinate plane with that coordinate exactly +0 or exactly -0
    (so is their centroid's), beside a small cloud; each axis, both signs, and both
    encounter orders (the case with neg_first reverses the list)."""
    def make():
        rng = np.random.default_rng(15)
        v = []
        for axis in range(3):
            for zero in (0.0, -0.0):
                for j in range(6):              # one cell of a 4 x 3 grid each: coplanar, never overlapping
                    cell = np.array([j % 4 + (4 if zero == 0.0 and np.signbit(zero) else 0), j // 4], np.float64)
                    t = np.zeros((3, 3))
                    t[:, [a for a in range(3) if a != axis]] = 0.5 * cell - 1.9 + rng.uniform(0.05, 0.45, (3, 2))
                    t[:, axis] = zero
                    v.append(t)
        # triangles whose lowest vertex is 1e-4f: the stored bound is exactly +0
        for axis in range(3):
            for j in range(4):
                t = rng.uniform(0.2, 1, (3, 3))
                t[0, axis] = float(F(1e-4))
                v.append(t)
        v = np.array(v)
        if neg_first:
            v = v[::-1]
        sd = base()
        sd.add_triangles(v.astype(F), np.broadcast_to(F([0, 0, 1]), v.shape).copy(), 0)
        return tris(sd, rng.uniform(-1, 1, (40, 3)))
    return make


def tiny_extent(n_tiny):
    """n_tiny objects whose centroids span 8e-39 on x (subnormal: k = 14.4 / extent is
    +inf) and [0, 1] on y and z, beside a cloud at x in [1, 2]."""
    def make():
        rng = np.random.default_rng(16)
        c = np.c_[np.arange(n_tiny) * (8e-39 / n_tiny), rng.uniform(0, 1, (n_tiny, 2))]
        v = np.repeat(c[:, None, :], 3, 1)          # no extent on x: the centroid's x is the vertices'
        v[:, 1, 1:] += [0.010, 0.003]               # (no edge along an axis: KIRK's triangle ctor bends those)
        v[:, 2, 1:] += [0.004, 0.010]
        sd = base()
        sd.add_triangles(v.astype(F), np.broadcast_to(F([1, 0, 0]), v.shape).copy(), 0)
        return tris(sd, rng.uniform(0, 1, (150, 3)) + [1, 0, 0])
    return make


def huge(n, scale):
    return lambda: tris(base(), np.random.default_rng(17).uniform(-1, 1, (n, 3)) * scale, 1e-4 * scale)


def overflowing_extent(n):
    """Centroids from -2e38 to 2e38 on x: finite, but cbmax - cbmin is +inf.  Cones along y,
    whose centroid has the base's x (a triangle's (A + B) + C would overflow, and is refused)."""
    def make():
        rng = np.random.default_rng(18)
        return cones(base(), np.c_[np.linspace(-2e38, 2e38, n), rng.uniform(-1, 1, (n, 2))], [0, 0.05, 0], 0.004, 0.003)
    return make


# ---- the list --------------------------------------------------------------------------------------
CASES = {}
for _n in (1, 2, 3, 4, 255, 256, 257, 258, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 18432, 18433, 20481):
    CASES[f"count_{_n}"] = Case(count_case(_n), why="uniform cloud: phase hand-over, chunk edges, k_pick's loop")
CASES["handover_256_257"] = Case(two_clusters(256, 257), why="the 256/257 hand-over one level below the root")
CASES["handover_2048_2049"] = Case(two_clusters(2048, 2049), why="one- and two-chunk nodes side by side, below the root")
CASES["ties_lattice_6"] = Case(lattice(6), why="equal costs across axes and planes, subtree phase")
CASES["ties_lattice_8"] = Case(lattice(8), why="the same at the level/subtree boundary (512 objects)")
CASES["ties_lattice_8_permuted"] = Case(lattice(8, (2, 0, 1)), why="the same with the axes permuted")
CASES["ties_lattice_16"] = Case(lattice(16), why="the same in the level phase with two chunks")
CASES["bin_edges_unit"] = Case(bin_edges(0.0, 1.0, 0), why="k (c - cbmin) at, below and above every integer")
CASES["bin_edges_offset"] = Case(bin_edges(-1.3, 1.7, 0), why="the same for another k and a negative cbmin")
CASES["bin_edges_level"] = Case(bin_edges(5.5, 6.2, 300), why="the same through the level phase's partition")
CASES["bin_edges_level_wide"] = Case(bin_edges(-7.0, 93.0, 300), why="the same for a small k")
CASES["lopsided_1_axis"] = Case(lambda: lopsided(PEEL_N, peeling_ratio(1), 1, PEEL_TOP)(), trace_truth=False,
                                why="one object peeled per split: the closed-form preorder on a chain")
CASES["lopsided_2_axes"] = Case(lambda: lopsided(PEEL_N, peeling_ratio(2), 2, PEEL_TOP)(), trace_truth=False, why="the same, two axes")
CASES["lopsided_3_axes"] = Case(lambda: lopsided(PEEL_N, peeling_ratio(3), 3, PEEL_TOP)(), trace_truth=False,
                                why="the same, all three axes tie")
CASES["lopsided_level_300"] = Case(lopsided(300, 1.25, 1), trace_truth=False,
                                   why="a lopsided tree that enters through the level phase")
CASES["depth_63"] = Case(depth_case(63), trace_truth=False, why="the deepest tree the traversal stack takes")
CASES["mixed_extents"] = Case(mixed_extents, why="a huge floor with 3,000 tiny cones and triangles")
CASES["parallel_hair"] = Case(parallel_hair, why="flat centroid boxes on sub-ranges")
CASES["duplicates_in_level"] = Case(duplicates, trace_truth=False,     # 4,000 coincident triangles: the closest is a tie
                                    why="4,000 of 5,000 centroids coincide: a large leaf from the level phase")
CASES["planar_beside_cloud"] = Case(planar_beside_cloud, why="a flat cluster of 300 beside a cloud of 300")
CASES["signed_zero_pos_first"] = Case(signed_zeros(False), signed_zero=True, why="+0 met before -0, each axis")
CASES["signed_zero_neg_first"] = Case(signed_zeros(True), signed_zero=True, why="-0 met before +0, each axis")
# finite input on which KIRK's recursion is undefined: such a node is a leaf
CASES["undefined_tiny_subtree"] = Case(tiny_extent(100), why="extent 8e-39, k = +inf, node met in the subtree phase")
CASES["undefined_tiny_level"] = Case(tiny_extent(400), why="the same, node met in the level phase")
CASES["undefined_extent_overflow"] = Case(overflowing_extent(300), trace_truth=False, why="cbmax - cbmin = +inf")
CASES["undefined_cost_1e19_level"] = Case(huge(1000, 1e19), trace_truth=False, why="every SAH cost +inf, level phase")
CASES["undefined_cost_1e19_subtree"] = Case(huge(200, 1e19), trace_truth=False, why="every SAH cost +inf, subtree phase")
CASES["overflowing_cost_1.3e17"] = Case(huge(1000, 1.3e17), trace_truth=False, why="some SAH costs +inf, some finite")

DEPTH_64 = Case(depth_case(64), trace_truth=False, why="one level deeper than the traversal stack: refused")


# ---- rays ----------------------------------------------------------------------------------------
def make_rays(bounds, n, seed):
    """n float32 rays (orig, unit d, tmax): 5/8 aimed at a random object's centroid jittered
    by a quarter of its box, 1/8 grazing a corner of a random object's box, 1/4 in random
    directions (mostly misses); from 3 to 30 box diagonals of that object away, near enough
    for KIRK's float32 intersectors to resolve it (tests/_geomref.py)."""
    b = np.asarray(bounds, np.float64).reshape(-1, 9)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(b), n)
    diag = np.linalg.norm(b[k, 3:6] - b[k, :3], axis=1)[:, None]
    ext = b[k, 3:6] - b[k, :3]
    target = b[k, 6:9] + rng.normal(size=(n, 3)) * 0.25 * ext
    graze = np.arange(n) % 8 == 7
    corner = np.where(rng.integers(0, 2, (n, 3)) == 1, b[k, 3:6], b[k, :3])
    target[graze] = corner[graze]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    orig = target - d * (rng.uniform(3, 30, (n, 1)) * diag)
    wild = np.arange(n) % 4 == 2
    d2 = rng.normal(size=(n, 3))
    d[wild] = (d2 / np.linalg.norm(d2, axis=1, keepdims=True))[wild]
    orig, d = orig.astype(F), d.astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    tmax = (rng.uniform(1.0, 60.0, n) * diag[:, 0]).astype(F)
    return orig, d.astype(F), tmax
