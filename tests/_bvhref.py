"""BVH::addBaseDataStructure restated in float32 numpy, and checks of a built tree.

The tree every closest hit depends on is KIRK's binned-SAH
recursion (CPU_BVH.cpp:16-44 build, 95-138 split, 357-552 partition;
BoundingBox.cpp).  The oracle (C), the host builder (C++) and the device builder
(HIP) are three restatements of it; this is a fourth, written from KIRK's
source and sharing no code with them, that the other three answer to
(tests/test_build_truth.py, tests/test_gpu_build_truth.py).

What is literal: every float32 operation in KIRK's operand order, one rounding
each (numpy float32 arithmetic never fuses); the 3 x 15 costs compared with the
strict `<` of the loop `axis 0..2, plane 14..0`; the two-pointer partition as
the `while (left < right)` loop itself; the recursion in preorder.

What is vectorised: the min / max reductions (bins, prefix and suffix boxes, node
boxes).  std::min / std::max keep their first operand on a tie, so a reduction
returns the first element, in encounter order, that compares equal to the
extreme: the only thing order can change is the sign of a zero.  Node boxes
are reduced with that rule (first occurrence).  Centroid boxes are reduced
numerically: the sign of a zero in a centroid box reaches no output (it enters
`c - cbmin`, `cbmax - cbmin` and box areas, none of which depends on it except
through the sign of a zero result, which `(int)`, `> 0.0f` and `<` ignore).

The one departure from KIRK, taken only where KIRK's recursion is undefined
(DESIGN.md §20): a node whose split is undefined is a leaf.  A split is
undefined when, on any axis, the centroid extent or k = 14.4f / extent is not
finite (KIRK would convert a NaN or an out-of-range float to int and index
bin_bounds[16] with it), or when no plane has a cost below FLT_MAX (KIRK would
partition by uninitialised boxes).
"""
from dataclasses import dataclass

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
NB = 16


@dataclass(frozen=True)
class Rule:
    """KIRK's choices; the fields exist so that a test can show that each one is pinned."""
    strict: bool = True              # cost < best   (slip: <=)
    planes_down: bool = True         # plane 14..0   (slip: 0..14)
    axes: tuple = (0, 1, 2)          # axis 0..2     (slip: reversed)
    hoare: bool = True               # the two-pointer loop (slip: a stable partition by side)
    right_if_greater: bool = True    # bin > plane goes right (slip: bin >= plane)
    n_planes: int = NB - 1           # 15 planes     (slip: 16; harmless, its 16th cost is NaN)


KIRK = Rule()


def _area(mn, mx):
    """BoundingBox::surfaceArea: 2.f * (size.x * size.y + size.x * size.z + size.y * size.z)."""
    s = mx - mn
    return F(2.0) * ((s[..., 0] * s[..., 1] + s[..., 0] * s[..., 2]) + s[..., 1] * s[..., 2])


def _worth(mn, mx):
    d = mx - mn
    return bool(d[0] > 0 and d[1] > 0 and d[2] > 0)


def split_defined(mn, mx):
    """The centroid extent and k of every axis are finite (see the module docstring)."""
    with np.errstate(all="ignore"):
        d = mx - mn
        k = (F(NB) * (F(1.0) - F(0.1))) / d
    return bool(np.all(np.isfinite(d)) and np.all(np.isfinite(k)))


def _first_min(a):
    return a[np.argmin(a, axis=0), np.arange(a.shape[1])]


def _first_max(a):
    return a[np.argmax(a, axis=0), np.arange(a.shape[1])]


def _partition(ids, first, second, cen, cmn, cmx, rule):
    """BVHNode::partition on ids[first..second] (inclusive).  Returns (left_second,
    right_first, left centbox, right centbox) or None when no plane has a cost < FLT_MAX."""
    members = ids[first:second + 1]
    c = cen[members]                                             # (m, 3) float32
    with np.errstate(all="ignore"):
        cbdiff = cmx - cmn
        k = (F(NB) * (F(1.0) - F(0.1))) / cbdiff                 # (amnt_bins * (1 - epsilon)) / cbdiff
        bins = (k * (c - cmn)).astype(np.int32)                  # int bin_id = k * (centroid[axis] - cbmin)
    assert bins.min() >= 0 and bins.max() < NB, "bin index outside bin_bounds[16]"
    m = len(members)
    key = (bins + NB * np.arange(3, dtype=np.int32)).T.reshape(-1)     # axis-major: axis * 16 + bin
    order = np.argsort(key, kind="stable")
    skey = key[order]
    vals = np.concatenate([c, c, c])[order]
    starts = np.flatnonzero(np.r_[True, skey[1:] != skey[:-1]])
    bmn = np.full((3 * NB, 3), FLT_MAX, F)
    bmx = np.full((3 * NB, 3), -FLT_MAX, F)
    bmn[skey[starts]] = np.minimum.reduceat(vals, starts, axis=0)
    bmx[skey[starts]] = np.maximum.reduceat(vals, starts, axis=0)
    bn = np.bincount(key, minlength=3 * NB).astype(np.uint32).reshape(3, NB)
    bmn = bmn.reshape(3, NB, 3)
    bmx = bmx.reshape(3, NB, 3)
    # left_bounds[p] = bins 0..p, right_bounds[p] = bins p+1..15
    lmn, lmx = np.minimum.accumulate(bmn, axis=1), np.maximum.accumulate(bmx, axis=1)
    rmn = np.minimum.accumulate(bmn[:, ::-1], axis=1)[:, ::-1]
    rmx = np.maximum.accumulate(bmx[:, ::-1], axis=1)[:, ::-1]
    ln = np.cumsum(bn, axis=1, dtype=np.uint32)
    rn = np.cumsum(bn[:, ::-1], axis=1, dtype=np.uint32)[:, ::-1]
    if rule.n_planes > NB - 1:               # the slip's 16th plane has all 16 bins on its left, none on its right
        bmn1, bmx1 = np.full((3, 1, 3), FLT_MAX, F), np.full((3, 1, 3), -FLT_MAX, F)
        rmn, rmx = np.concatenate([rmn, bmn1], axis=1), np.concatenate([rmx, bmx1], axis=1)
        rn = np.concatenate([rn, np.zeros((3, 1), np.uint32)], axis=1)
    np_ = rule.n_planes
    pl = np.arange(np_)
    pr = pl + 1
    with np.errstate(all="ignore"):
        cost = (_area(lmn[:, pl], lmx[:, pl]) * ln[:, pl].astype(F)
                + _area(rmn[:, pr], rmx[:, pr]) * rn[:, pr].astype(F))
    assert cost.dtype == F
    best, best_axis, best_plane = float(FLT_MAX), 0, 0
    found = False
    for axis in rule.axes:
        for plane in (range(np_ - 1, -1, -1) if rule.planes_down else range(np_)):
            cst = float(cost[axis, plane])
            if (cst < best) if rule.strict else (cst <= best):
                best, best_axis, best_plane, found = cst, axis, plane, True
    if not found:
        return None
    lcb = (lmn[best_axis, best_plane].copy(), lmx[best_axis, best_plane].copy())
    rcb = (rmn[best_axis, best_plane + 1].copy(), rmx[best_axis, best_plane + 1].copy())
    b = bins[:, best_axis].tolist()
    loc = members.tolist()
    if rule.right_if_greater:
        goes_right = [x > best_plane for x in b]
    else:
        goes_right = [x >= best_plane for x in b]
    if not rule.hoare:
        lo = [o for o, r in zip(loc, goes_right) if not r]
        hi = [o for o, r in zip(loc, goes_right) if r]
        ids[first:second + 1] = lo + hi
        return first + len(lo) - 1, first + len(lo), lcb, rcb
    left, right = 0, m - 1
    left_stopped = right_stopped = False
    while left < right:
        if not left_stopped:
            if goes_right[left]:
                left_stopped = True
            else:
                left += 1
        if not right_stopped:
            if not goes_right[right]:
                right_stopped = True
            else:
                right -= 1
        if left_stopped and right_stopped:
            loc[left], loc[right] = loc[right], loc[left]
            goes_right[left], goes_right[right] = goes_right[right], goes_right[left]
            left_stopped = right_stopped = False
            left += 1
            right -= 1
    if left > right:
        ls, rf = right, left
    elif left_stopped:
        ls, rf = left - 1, left
    elif right_stopped:
        ls, rf = right, right + 1
    elif goes_right[left]:
        ls, rf = left - 1, left
    else:
        ls, rf = left, left + 1
    ids[first:second + 1] = loc
    return first + ls, first + rf, lcb, rcb


def build(bounds, rule=KIRK, max_nodes=None):
    """The tree of BVH::addBaseDataStructure over objects given as (n, 9) float32 rows
    (bmin, bmax, centroid), in the format of native.host_build: boxes (nodes, 6),
    first, count (0 = interior, first -1), ids, depth; nodes in DFS preorder."""
    b = np.ascontiguousarray(bounds, F).reshape(-1, 9)
    n = len(b)
    omn, omx, cen = b[:, 0:3], b[:, 3:6], b[:, 6:9]
    ids = np.arange(n, dtype=np.int64)
    # scene_centbox: expandToInclude of every centroid
    cmn = np.minimum(F(FLT_MAX), cen.min(axis=0))
    cmx = np.maximum(F(-FLT_MAX), cen.max(axis=0))
    boxes, firsts, counts = [], [], []
    depth = 0
    stack = [(0, n - 1, cmn, cmx, 1)]
    while stack:
        first, second, cmn, cmx, d = stack.pop()
        members = ids[first:second + 1]
        # computeBoundaries: std::min / std::max over the members' bounds, in order
        boxes.append(np.concatenate([_first_min(omn[members]), _first_max(omx[members])]))
        depth = max(depth, d)
        if max_nodes is not None and len(boxes) > max_nodes:
            raise RuntimeError("more nodes than the caller allows")
        part = None
        with np.errstate(all="ignore"):
            splittable = second - first > 1 and _worth(cmn, cmx) and split_defined(cmn, cmx)
        if splittable:
            part = _partition(ids, first, second, cen, cmn, cmx, rule)
        if part is None:
            firsts.append(first)
            counts.append(second - first + 1)
            continue
        ls, rf, lcb, rcb = part
        firsts.append(-1)
        counts.append(0)
        stack.append((rf, second, rcb[0], rcb[1], d + 1))     # popped second: preorder
        stack.append((first, ls, lcb[0], lcb[1], d + 1))
    return {"boxes": np.array(boxes, F).reshape(-1, 6), "first": np.array(firsts, np.int32),
            "count": np.array(counts, np.int32), "ids": ids.astype(np.int32), "depth": depth}


# ---- a tree in that format, checked without any builder ------------------------------------------
def same_tree(a, b):
    """Bit-for-bit equality of two trees (boxes as uint32); returns the first difference or None."""
    if a["depth"] != b["depth"]:
        return f"depth {a['depth']} != {b['depth']}"
    if len(a["count"]) != len(b["count"]):
        return f"{len(a['count'])} nodes != {len(b['count'])}"
    for k in ("count", "first", "ids"):
        if not np.array_equal(a[k], b[k]):
            i = int(np.flatnonzero(np.asarray(a[k]) != np.asarray(b[k]))[0])
            return f"{k}[{i}]: {a[k][i]} != {b[k][i]}"
    ua = np.ascontiguousarray(a["boxes"], F).view(np.uint32)
    ub = np.ascontiguousarray(b["boxes"], F).view(np.uint32)
    if not np.array_equal(ua, ub):
        i = np.argwhere(ua != ub)[0]
        return f"boxes[{i[0]}, {i[1]}]: {a['boxes'][i[0], i[1]]!r} != {b['boxes'][i[0], i[1]]!r}"
    return None


def check_structure(tree, bounds, zero_sign_free=False):
    """ids are a permutation; the preorder is well formed; leaf ranges tile [0, n) in
    order; every leaf box is the bit-exact std::min / std::max union of its objects'
    bounds in leaf order and every interior box that of its children (left first);
    depth is the depth.  zero_sign_free: boxes are compared after clearing the sign
    of zeros (a parallel reduction may pick another zero)."""
    b = np.ascontiguousarray(bounds, F).reshape(-1, 9)
    n = len(b)
    boxes = np.ascontiguousarray(tree["boxes"], F)
    first, count, ids = np.asarray(tree["first"]), np.asarray(tree["count"]), np.asarray(tree["ids"])
    nn = len(count)
    assert boxes.shape == (nn, 6) and len(first) == nn and len(ids) == n
    assert np.array_equal(np.sort(ids), np.arange(n)), "ids are not a permutation"
    assert np.all(count >= 0)

    def bits(x):
        x = np.array(x, F)
        if zero_sign_free:
            x = np.where(x == 0, F(0.0), x)
        return x.view(np.uint32)

    # walk the preorder: sizes and depths
    size = np.ones(nn, np.int64)
    right = np.full(nn, -1, np.int64)
    for i in range(nn - 1, -1, -1):
        if count[i] == 0:
            assert i + 1 < nn, "interior node without a left child"
            r = i + 1 + size[i + 1]
            assert r < nn, "interior node without a right child"
            right[i] = r
            size[i] = 1 + size[i + 1] + size[r]
    assert size[0] == nn, "preorder does not close"
    depth = np.zeros(nn, np.int64)
    depth[0] = 1
    nxt = 0
    for i in range(nn):
        if count[i] == 0:
            depth[i + 1] = depth[right[i]] = depth[i] + 1
            u_mn = np.where(boxes[right[i], :3] < boxes[i + 1, :3], boxes[right[i], :3], boxes[i + 1, :3])
            u_mx = np.where(boxes[i + 1, 3:] < boxes[right[i], 3:], boxes[right[i], 3:], boxes[i + 1, 3:])
            assert np.array_equal(bits(np.r_[u_mn, u_mx]), bits(boxes[i])), f"interior box {i} is not its children's"
        else:
            assert first[i] == nxt, f"leaf {i} starts at {first[i]}, expected {nxt}"
            nxt += count[i]
            mem = ids[first[i]:first[i] + count[i]]
            u = np.r_[_first_min(b[mem, 0:3]), _first_max(b[mem, 3:6])]
            assert np.array_equal(bits(u), bits(boxes[i])), f"leaf box {i} is not its objects'"
    assert nxt == n, "leaf ranges do not tile [0, n)"
    assert int(depth.max()) == tree["depth"], f"depth {tree['depth']}, true depth {int(depth.max())}"


# ---- object bounds against the float64 geometry ----------------------------------------------------
BOX_ULPS = 8      # a stored float32 box against float64 geometry (as tests/test_geometry_truth.py)


def check_bounds_contain(scene, bounds, n_rim=64):
    """No object's box cuts the object: a triangle's three vertices, and n_rim points on
    each rim circle of a cone (both radii), in float64, inside the float32 box up to the
    box's own rounding."""
    b = np.ascontiguousarray(bounds, F).reshape(-1, 9)
    lo, hi = b[:, 0:3].astype(np.float64), b[:, 3:6].astype(np.float64)
    tol_lo = BOX_ULPS * 2.0 ** -24 * np.maximum(1.0, np.abs(lo))
    tol_hi = BOX_ULPS * 2.0 ** -24 * np.maximum(1.0, np.abs(hi))
    tv = np.asarray(scene.tri_v, np.float64).reshape(-1, 3, 3)
    nt = len(tv)
    cb = np.asarray(scene.cone_base_r0, np.float64).reshape(-1, 4)
    ca = np.asarray(scene.cone_apex_r1, np.float64).reshape(-1, 4)
    assert len(np.asarray(scene.cone_model).reshape(-1)) == 0, "world-space cones only"
    bad = np.flatnonzero(((tv < (lo[:nt] - tol_lo[:nt])[:, None]) | (tv > (hi[:nt] + tol_hi[:nt])[:, None]))
                         .any(axis=(1, 2)))
    assert len(bad) == 0, f"triangle {bad[:1]} sticks out of its box"
    if len(cb):
        axis = ca[:, :3] - cb[:, :3]
        h = np.linalg.norm(axis, axis=1)
        v = axis / h[:, None]
        t = np.where((np.abs(v[:, 1]) < 0.9)[:, None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
        u = np.cross(v, t)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        w = np.cross(u, v)
        ang = 2 * np.pi * np.arange(n_rim) / n_rim
        ring = np.cos(ang)[None, :, None] * u[:, None, :] + np.sin(ang)[None, :, None] * w[:, None, :]
        rim = np.concatenate([cb[:, None, :3] + cb[:, 3, None, None] * ring,
                              ca[:, None, :3] + ca[:, 3, None, None] * ring], axis=1)
        l, hgh = lo[nt:] - tol_lo[nt:], hi[nt:] + tol_hi[nt:]
        bad = np.flatnonzero(((rim < l[:, None]) | (rim > hgh[:, None])).any(axis=(1, 2)))
        assert len(bad) == 0, f"cone {bad[:1]} sticks out of its box"
