"""TEST INFRASTRUCTURE ONLY (imported by tests/ — never by the product).

The RULES of one round of the device decimation (drawingspinup_amd/csrc/mesh_decimate_gpu.hip),
checked from the mesh before the round and the mesh after it, in float64 with np.longdouble
accumulations.  Not a restatement of the schedule: the device ranks float32 cost bits and its
float64 arithmetic contracts to FMA, so which admissible independent subset of the candidates a
round takes is left free.  What is pinned: every applied collapse was a candidate, independent of
all others of its round, admissible (flip test, link condition), placed at the target of
`edge_target`, and left exactly the faces, positions and quadrics the file header describes.

`init_quadrics`   per-vertex quadrics from the definition (mesh_decimate.hip's header)
`target`          the rule of `edge_target` with its conditioning and branch margins
`check_round`     recover a round's collapses from before / after and hold them to the rules
`simulate_round`  a plain round (random priorities, greedy independent set) with switchable
                  mutants: the checker's own positive and negative tests run on it without a GPU
"""
import collections

import numpy as np

from oracle import decimate_ref as D

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# library layout of a quadric [A b; b^T c]: a00 a01 a02 a11 a12 a22 b0 b1 b2 c
ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))
FRAGILE_REL = 1e-9
RULES = ("recovery", "faces", "independence", "untouched data", "quadrics", "target", "admissibility",
         "candidacy", "floor")


class RoundViolation(AssertionError):
    def __init__(self, rule, msg):
        assert rule in RULES
        super().__init__("%s: %s" % (rule, msg))
        self.rule = rule


def q10_to_mat(q):
    m = np.zeros((4, 4), np.asarray(q).dtype)
    for k, (i, j) in enumerate(ORDER):
        m[i, j] = m[j, i] = q[k]
    return m


def mat_to_q10(m):
    return np.array([m[i, j] for i, j in ORDER])


def live_faces(f):
    f = np.asarray(f).reshape(-1, 3)
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]


# ------------------------------------------------------------------------------------ quadrics
def init_quadrics(v, f, boundary_weight, dtype=LD):
    """-> (Q (nv,10) float64, S (nv,10) float64): the initial quadrics and, entry by entry, the sum
    of the absolute values of the terms that were added (the scale a rounding bound refers to).
    Area-weighted face planes; for every undirected edge with exactly one triangle the plane
    through the edge perpendicular to that triangle, weight boundary_weight x area, on both end
    points; zero-area triangles add nothing.  `dtype` is the precision of every intermediate
    (np.float64: what a plain double evaluation of the same definition gives)."""
    v = np.asarray(v, np.float64).astype(dtype)
    f = live_faces(f)
    nv = len(v)
    Q, S = np.zeros((nv, 10), dtype), np.zeros((nv, 10), dtype)

    def add(i, n, d, w):
        q = mat_to_q10(D._plane_quadric(n, d, w))
        Q[i] += q
        S[i] += np.abs(q)

    count = collections.Counter()
    for t in f:
        for k in range(3):
            count[tuple(sorted((int(t[k]), int(t[(k + 1) % 3]))))] += 1
    for t in f:
        a, b, c = (int(i) for i in t)
        cr = np.cross(v[b] - v[a], v[c] - v[a])
        l = np.sqrt(cr @ cr)
        if not l > 0:
            continue
        n = cr / l
        for i in (a, b, c):
            add(i, n, -(n @ v[a]), 0.5 * l)
        if not boundary_weight > 0:
            continue
        for k in range(3):
            lo, hi = sorted((int(t[k]), int(t[(k + 1) % 3])))
            if count[(lo, hi)] != 1:
                continue
            en = np.cross(v[hi] - v[lo], n)
            el = np.sqrt(en @ en)
            if not el > 0:
                continue
            en = en / el
            for i in (lo, hi):
                add(i, en, -(en @ v[lo]), dtype(boundary_weight) * 0.5 * l)
    return Q.astype(np.float64), S.astype(np.float64)


def init_quadrics_bound(v, f, boundary_weight):
    """-> (Q, bound): the entry-wise bound a float64 evaluation of the initial quadrics is held to.
    16 eps sum|terms| covers the rounding of the sum; it forgets that a term w n_i n_j carries the
    rounding of the unit normal (a few eps absolute, from the cancellation in the cross product)
    however small n_i is, so on meshes with normals close to an axis (marching cubes) this
    module's own float64 evaluation of the definition needs up to 1.35 times as much.  The bound is
    raised to cover what that float64 evaluation needs, times 4 — never lowered below 16 eps."""
    Q, S = init_quadrics(v, f, boundary_weight)
    Q64, _ = init_quadrics(v, f, boundary_weight, np.float64)
    base = 16 * EPS * S
    need = float((np.abs(Q64 - Q) / np.maximum(base, 1e-300)).max()) if Q.size else 0.0
    return Q, base * max(1.0, 4 * need), need


# ------------------------------------------------------------------------------------ target
def _eval_ld(q, x):
    """error(x) = x^T A x + 2 b^T x + c in long double, and the sum of |terms|."""
    q, x = np.asarray(q, LD), np.asarray(x, LD)
    terms = [q[0] * x[0] * x[0], 2 * q[1] * x[0] * x[1], 2 * q[2] * x[0] * x[2], q[3] * x[1] * x[1],
             2 * q[4] * x[1] * x[2], q[5] * x[2] * x[2], 2 * q[6] * x[0], 2 * q[7] * x[1], 2 * q[8] * x[2], q[9]]
    return sum(terms), sum(abs(t) for t in terms)


def _minimiser_ld(q):
    """-A^-1 b in long double; det by cofactors, trace.  A different method from the library's
    (which eliminates with pivoting about the edge's midpoint in float64): the cofactor inverse
    about the origin, then two steps of iterative refinement on the residual A x + b.  The
    cofactor inverse alone loses eps_ld cond(A) (l1 / l2) |x| on a near-planar quadric; a
    refinement step multiplies that by the same small factor again."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (LD(x) for x in q[:9])
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det, tr = a00 * c00 + a01 * c01 + a02 * c02, a00 + a11 + a22
    if det == 0:
        return None, det, tr
    A = np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]], LD)
    inv = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]], LD) / det
    b = np.array([b0, b1, b2], LD)
    x = -(inv @ b)
    for _ in range(2):
        x = x - inv @ (A @ x + b)
    return x, det, tr


Target = collections.namedtuple("Target", "cost x branch cond fragile margins alternatives")


def target(Q, p0, p1):
    """The rule of `edge_target` for the summed quadric Q (10-vector, library layout) of an edge
    p0 - p1.  branch: 'minimiser' or 'endpoint'.  cond: cond_2 of the 3x3 block.  margins: how far
    each branch decision is from its threshold, relative: |det| against 1e-9 tr^3, |x - mid|
    against 4 len, and the smallest gap between the chosen end point cost and the other two.
    A decision within FRAGILE_REL of its threshold is fragile: `alternatives` then lists the
    targets of the neighbouring branches as well.  An end point cost is a sum with cancellation
    (terms ~ area x |x|^2, result down to 1e-20 on flat regions): a gap that the float64 rounding of
    the two sums themselves can close, 64 eps sum|terms|, counts as inside the threshold."""
    Q = np.asarray(Q, np.float64)
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    cost, x = D._target(q10_to_mat(Q), p0, p1)                # the branch the float64 restatement takes
    ends = [p0, p1, 0.5 * (p0 + p1)]
    branch = "endpoint" if x is p0 or x is p1 or np.array_equal(x, ends[2]) else "minimiser"
    A = q10_to_mat(Q)[:3, :3]
    with np.errstate(all="ignore"):
        cond = float(np.linalg.cond(A)) if np.all(np.isfinite(A)) and np.any(A) else np.inf
    xm, det, tr = _minimiser_ld(Q)
    margins, fragile, use_ends, use_min = {}, False, branch == "endpoint", branch == "minimiser"
    if tr > 0:
        thr = LD(1e-9) * tr * tr * tr
        margins["det"] = float(abs(abs(det) / thr - 1))
        if margins["det"] < FRAGILE_REL:
            fragile = use_ends = True
            use_min = use_min or xm is not None
        if xm is not None and (abs(det) > thr or margins["det"] < FRAGILE_REL):
            length = np.sqrt(((p1 - p0).astype(LD) ** 2).sum())
            dist = np.sqrt(((xm - 0.5 * (p0.astype(LD) + p1.astype(LD))) ** 2).sum())
            if length > 0:
                margins["distance"] = float(abs(dist / (4 * length) - 1))
                if margins["distance"] < FRAGILE_REL:
                    fragile = use_ends = use_min = True
    ld_min = bool(tr > 0 and xm is not None and abs(det) > LD(1e-9) * tr * tr * tr
                  and margins.get("distance") is not None and dist <= 4 * length)
    if ld_min != (branch == "minimiser"):                      # float64 and long double disagree
        fragile = use_ends = True
        use_min = xm is not None
    costs = [_eval_ld(Q, e) for e in ends]
    k = int(np.argmin([float(c[0]) for c in costs]))
    near = [k]
    gaps = []
    for j in range(3):
        if j == k:
            continue
        gap = abs(costs[j][0] - costs[k][0])
        tol = FRAGILE_REL * max(abs(costs[j][0]), abs(costs[k][0])) + 64 * EPS * max(costs[j][1], costs[k][1])
        gaps.append(float(gap / tol) if tol > 0 else np.inf)
        if gap <= tol:
            near.append(j)
    margins["gap"] = min(gaps)
    if use_ends and len(near) > 1:
        fragile = True
    alternatives = []
    if use_min and xm is not None:
        alternatives.append(("minimiser", xm.astype(np.float64)))
    if use_ends:
        alternatives += [("endpoint", ends[j]) for j in near]
    if branch == "minimiser":
        x = xm.astype(np.float64)                              # the long-double solve, rounded once
        cost = float(_eval_ld(Q, xm)[0])
    else:
        x, cost = ends[k], float(costs[k][0])                  # first minimum of the long-double costs
    return Target(cost, x, branch, cond, fragile, margins, alternatives)


def edge_costs(v, Q, e0, e1):
    """float64 costs of many edges at once (the rule of `edge_target`, vectorised): what decides
    who is a candidate.  Not used for any per-collapse check."""
    q = Q[e0] + Q[e1]
    p0, p1 = v[e0], v[e1]
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = q.T

    def ev(x):
        return (x[:, 0] * (a00 * x[:, 0] + 2 * a01 * x[:, 1] + 2 * a02 * x[:, 2]) + x[:, 1] * (a11 * x[:, 1] + 2 * a12 * x[:, 2])
                + a22 * x[:, 2] * x[:, 2] + 2 * (b0 * x[:, 0] + b1 * x[:, 1] + b2 * x[:, 2]) + c)

    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    det, tr = a00 * c00 + a01 * c01 + a02 * c02, a00 + a11 + a22
    mid = 0.5 * (p0 + p1)
    with np.errstate(all="ignore"):
        ok = (tr > 0) & (np.abs(det) > 1e-9 * tr * tr * tr)
        # a pivoted solve about the midpoint, as the library's (the determinant only decides)
        A = np.stack([np.stack([a00, a01, a02], 1), np.stack([a01, a11, a12], 1), np.stack([a02, a12, a22], 1)], 1)
        A = np.where(ok[:, None, None], A, np.eye(3))
        g = np.stack([b0, b1, b2], 1) + np.einsum("nij,nj->ni", A, mid)
        x = mid + np.linalg.solve(A, -g[:, :, None])[:, :, 0]
        ok &= np.linalg.norm(x - mid, axis=1) <= 4.0 * np.linalg.norm(p1 - p0, axis=1)
        cmin = ev(np.where(ok[:, None], x, mid))
    cend = np.minimum(np.minimum(ev(p0), ev(p1)), ev(mid))
    return np.where(ok, cmin, cend)


def cost_f32(c):
    """the device's sort key: max(cost, 0) rounded to float32"""
    return np.float32(np.maximum(np.asarray(c, np.float64), 0.0))


# ------------------------------------------------------------------------------------ mesh tables
def owner_edges(f):
    """One entry per OWNER half-edge, as owner_flags_kernel defines it: a -> b owns its edge when
    a < b, or when a > b and no triangle holds b -> a.  -> (lo, hi) int arrays (an edge with two
    half-edges of the same direction appears twice, as on the device)."""
    f = np.asarray(f).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    half = set(zip(a.tolist(), b.tolist()))
    own = np.array([x < y or (x > y and (y, x) not in half) for x, y in zip(a.tolist(), b.tolist())], bool)
    a, b = a[own], b[own]
    return np.minimum(a, b), np.maximum(a, b)


def n_candidates(nf, ne, floor_faces):
    """ncand of a round; 0 when the device runs no round at all (budget (nf - floor) / 2 < 1, no edge)"""
    if (nf - floor_faces) // 2 < 1 or ne == 0:
        return 0
    return max(1, min((nf - floor_faces) // 2, ne // 2))


def candidacy_rank(f, floor_faces, remembered=0):
    """-> (rank, n_edges): a collapse of the round must cost no more than the rank-th cheapest edge"""
    ne = len(owner_edges(f)[0])
    return min(n_candidates(len(f), ne, floor_faces) + int(remembered), ne), ne


class _Tables:
    def __init__(self, f):
        self.f = np.asarray(f).reshape(-1, 3)
        self.vt = collections.defaultdict(list)
        self.nbr = collections.defaultdict(set)
        for t, tri in enumerate(self.f.tolist()):
            for i in tri:
                self.vt[i].append(t)
                self.nbr[i].update(tri)
        for i in self.nbr:
            self.nbr[i].discard(i)


def _admissible(tb, v, v0, v1, x, keep_manifold, flip_tol=0.0, check_flip=True, check_link=True):
    """None when the collapse v1 -> v0 placed at x is admissible on the mesh of `tb`, else the
    reason.  collapse_kernel's tests: no ring triangle of either end (not holding the other end)
    turns its normal over; at least one triangle on the edge; the link condition."""
    f = tb.f
    shared = [t for t in tb.vt[v1] if v0 in f[t]]
    if check_flip:
        for mv, other in ((v1, v0), (v0, v1)):
            for t in tb.vt[mv]:
                tri = f[t]
                if other in tri:
                    continue
                p = [v[i].astype(LD) for i in tri]
                q = [np.asarray(x, LD) if i == mv else v[i].astype(LD) for i in tri]
                before = np.cross(p[1] - p[0], p[2] - p[0])
                after = np.cross(q[1] - q[0], q[2] - q[0])
                if before @ after < -flip_tol * np.sqrt(before @ before) * np.sqrt(after @ after):
                    return "triangle %s turns over" % (tri.tolist(),)
    if not shared:
        return "no triangle on the edge"
    if keep_manifold and check_link:
        common = (tb.nbr[v0] & tb.nbr[v1]) - {v0, v1}
        if len(common) != len(shared):
            return "link: %d common neighbours, %d triangles on the edge" % (len(common), len(shared))
        t0 = [frozenset(f[t].tolist()) - {v0} for t in tb.vt[v0] if v1 not in f[t]]
        for t in tb.vt[v1]:
            if v0 not in f[t] and frozenset(f[t].tolist()) - {v1} in t0:
                return "link: a triangle of v1 lies beside a triangle of v0"
    return None


def has_twin_faces(f):
    """Two triangles on the same three vertices (what a tetrahedron collapses to without the link
    test).  One more collapse removes both and strands the third vertex with them: before and after
    no longer tell which of the two vanished vertices was collapsed, so check_round cannot recover
    such a round — the round tests stop a sequence there."""
    s = np.sort(np.asarray(f).reshape(-1, 3), 1)
    return len(np.unique(s, axis=0)) < len(s)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _apply_faces(f, pairs):
    """f with every v1 -> v0 applied and the faces that held both ends of a collapse removed (order kept)"""
    f = np.asarray(f).reshape(-1, 3)
    lut = np.arange(int(f.max()) + 1 if f.size else 0)
    for v0, v1 in pairs:
        lut[v1] = v0
    g = lut[f]
    return g[(g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])]


Collapse = collections.namedtuple("Collapse", "v0 v1 branch fragile ratio cost")


# ------------------------------------------------------------------------------------ the checker
def check_round(v_before, f_before, Q_before, v_after, f_after, Q_after, *, floor_faces, keep_manifold,
                remembered=0):
    """Hold one round to the rules; raises RoundViolation(rule, ...) on the first violated one.
    -> (collapses, n_fragile).  Only before and after are read: which admissible independent subset
    of the candidates the round took is free.

    `remembered`: how many rejected collapses the rounds before this one have remembered
    (stats[2] before the round).  edge_cost_kernel gives a remembered rejection the cost +inf, so
    each of them lets one more edge into the cheapest `ncand`: the candidacy rule compares with the
    (ncand + remembered)-th cheapest edge.  0 for a first round: the rule as the file header states it.
    stats[2] counts every rejection of every earlier round and pass, also those whose table slot was
    overwritten since or whose end points' versions changed: an UPPER bound on the edges that sort
    as +inf, and it only grows.  On meshes with many rejections the rank reaches the number of
    edges and the rule says nothing any more: `candidacy_rank` gives rank and edge count, the round
    tests print them."""
    vb, va = np.asarray(v_before, np.float64), np.asarray(v_after, np.float64)
    Qb, Qa = np.asarray(Q_before, np.float64), np.asarray(Q_after, np.float64)
    fb, fa = np.asarray(f_before).reshape(-1, 3).astype(np.int64), np.asarray(f_after).reshape(-1, 3).astype(np.int64)
    if vb.shape != va.shape or Qb.shape != Qa.shape:
        raise RoundViolation("untouched data", "array shapes changed")
    tb = _Tables(fb)
    used_b, used_a = set(np.unique(fb).tolist()), set(np.unique(fa).tolist())
    if not used_a <= used_b:
        raise RoundViolation("faces", "vertices %s appear from nowhere" % sorted(used_a - used_b)[:5])
    changed = (_bits(vb) != _bits(va)).any(1) | (_bits(Qb) != _bits(Qa)).any(1)
    # ---- recovery: every changed vertex is a survivor v0; its v1 is a vanished neighbour.  A
    # collapse also strands the vertices all of whose triangles lay on its edge (an apex with no
    # other triangle, v0 itself when it had no triangle off the edge): they vanish with it.
    vanished = used_b - used_a
    pairs, explained = [], set()
    for v0 in [int(i) for i in np.nonzero(changed)[0]]:
        gone = {n for n in tb.nbr[v0] if n in vanished}
        if not gone:
            raise RoundViolation("untouched data", "position or quadric of vertex %d changed; no neighbour of "
                                 "it was removed, so it is no surviving end point" % v0)
        fits = []
        for v1 in sorted(gone):
            on_edge = [t for t in tb.vt[v1] if v0 in fb[t]]
            stranded = {x for t in on_edge for x in fb[t].tolist()
                        if x != v1 and all(v0 in fb[u] and v1 in fb[u] for u in tb.vt[x])}
            if gone - {v1} <= stranded:
                fits.append((v1, stranded))
        if len(fits) != 1:
            raise RoundViolation("recovery", "changed vertex %d has the removed neighbours %s; %d of them explain "
                                 "the others as stranded by their own collapse (one collapse per survivor: "
                                 "independence and untouched data forbid more)" % (v0, sorted(gone)[:6], len(fits)))
        v1, stranded = fits[0]
        if not v0 < v1:
            raise RoundViolation("recovery", "vertex %d went into %d: the lower index survives" % (v1, v0))
        pairs.append((v0, v1))
        explained |= {v1} | stranded
    if (vanished - explained) or ({p[0] for p in pairs} & vanished) - explained:
        raise RoundViolation("recovery", "vertices %s are used before the round and not after it, and no changed "
                             "neighbour took their place" % sorted(vanished - explained)[:6])
    # ---- independence
    owner = {}
    for k, (v0, v1) in enumerate(pairs):
        for e in (v0, v1):
            if e in owner:
                raise RoundViolation("independence", "vertex %d is an end point of two collapses" % e)
            owner[e] = k
    for e, k in owner.items():
        for n in tb.nbr[e]:
            if owner.get(n, k) != k:
                raise RoundViolation("independence", "end point %d of collapse %s is adjacent to end point %d of "
                                     "collapse %s" % (e, pairs[k], n, pairs[owner[n]]))
    # ---- faces
    want = _apply_faces(fb, pairs)
    if want.shape != fa.shape or not np.array_equal(want, fa):
        raise RoundViolation("faces", "the faces after the round are not the faces before with %d collapses "
                             "applied, in order (%d rows against %d)" % (len(pairs), len(fa), len(want)))
    # ---- quadrics, target, admissibility
    out, n_fragile = [], 0
    for v0, v1 in pairs:
        qs = Qb[v0] + Qb[v1]
        if not np.array_equal(_bits(Qa[v0]), _bits(qs)):
            raise RoundViolation("quadrics", "Q[%d] after is not Q[%d] + Q[%d] before (largest difference %.3e)"
                                 % (v0, v0, v1, np.abs(Qa[v0] - qs).max()))
        tg = target(qs, vb[v0], vb[v1])
        length = float(np.linalg.norm(vb[v1] - vb[v0]))
        got, ratio, ok, branch = va[v0], 0.0, False, tg.branch
        options = tg.alternatives if tg.fragile else [(tg.branch, tg.x)]
        for br, x in options:
            if br == "endpoint":
                if np.array_equal(_bits(got), _bits(x)):
                    ok, branch = True, br
                    break
            else:
                bound = 64 * EPS * tg.cond * max(float(np.abs(x).max()), length)
                r = float(np.abs(got - x).max() / bound)
                if r <= 1:
                    ok, branch, ratio = True, br, r
                    break
                ratio = r
        if not ok:
            raise RoundViolation("target", "collapse %d <- %d placed at %s; edge_target gives %s (%s branch, "
                                 "cond %.3e, error / bound %.3g, margins %s)"
                                 % (v0, v1, got, tg.x, tg.branch, tg.cond, ratio, tg.margins))
        why = _admissible(tb, vb, v0, v1, tg.x, keep_manifold, flip_tol=1e-12)
        if why:
            raise RoundViolation("admissibility", "collapse %d <- %d: %s" % (v0, v1, why))
        n_fragile += bool(tg.fragile)
        out.append(Collapse(v0, v1, branch, bool(tg.fragile), ratio, tg.cost))
    # ---- candidacy
    if pairs:
        lo, hi = owner_edges(fb)
        c32 = np.sort(cost_f32(edge_costs(vb, Qb, lo, hi)))
        rank = candidacy_rank(fb, floor_faces, remembered)[0]
        limit = np.nextafter(c32[rank - 1], np.float32(np.inf))
        for c in out:
            if not cost_f32(c.cost) <= limit:
                raise RoundViolation("candidacy", "collapse %d <- %d costs %.9g; the %d-th cheapest of %d edges costs "
                                     "%.9g" % (c.v0, c.v1, cost_f32(c.cost), rank, len(lo), c32[rank - 1]))
    # ---- floor
    if set(edge_multiplicity(fb)) <= {1, 2} and len(fa) < floor_faces:
        raise RoundViolation("floor", "%d faces left, the floor is %d" % (len(fa), floor_faces))
    return out, n_fragile


def edge_multiplicity(f):
    """how many triangles every undirected edge has, as a sorted list of the distinct counts"""
    f = np.asarray(f).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return sorted(set(np.unique(e, axis=0, return_counts=True)[1].tolist())) if len(e) else []


# ------------------------------------------------------------------------------------ a plain round
MUTANTS = ("adjacent", "no_link", "no_flip", "wrong_sum", "midpoint", "move_ring", "beyond_budget")


def simulate_round(v, f, Q, ncand_rule, rng, *, mutate=None, keep_manifold=True):
    """One round in plain Python: the `ncand_rule(nf, ne)` cheapest owner edges (float32 cost) are
    candidates, each draws a unique random priority, and in priority order a candidate is applied
    when no end point of it equals or neighbours an end point of a collapse already applied and it
    is admissible on the mesh before the round.  NOT a model of the device's hash: it exists so
    that check_round can be tested without a GPU.  `mutate` switches one rule off (MUTANTS).
    -> (v, f, Q) after the round (new arrays, same indexing; faces compacted in order)."""
    assert mutate is None or mutate in MUTANTS
    v, Q = np.array(v, np.float64), np.array(Q, np.float64)
    f = np.asarray(f).reshape(-1, 3).astype(np.int64)
    tb = _Tables(f)
    lo, hi = owner_edges(f)
    if not len(lo):
        return v, f, Q
    ncand = ncand_rule(len(f), len(lo))
    if ncand < 1:
        return v, f, Q
    c32 = cost_f32(edge_costs(v, Q, lo, hi))
    order = np.argsort(c32, kind="stable")
    if mutate == "beyond_budget":
        cand = order[::-1]                                     # the most expensive edge that can be applied
    else:
        cand = order[:ncand]
        cand = cand[rng.permutation(len(cand))]
    blocked, ends, a0, a1, pairs = set(), set(), set(), set(), []
    slipped = False
    v2, Q2 = v.copy(), Q.copy()
    for e in cand.tolist():
        v0, v1 = int(lo[e]), int(hi[e])
        if v0 in blocked or v1 in blocked:
            # `adjacent`: once, a collapse whose survivor neighbours another collapse's survivor
            # (and touches that collapse in no other way) is let through
            if (mutate != "adjacent" or slipped or {v0, v1} & ends or tb.nbr[v1] & ends or tb.nbr[v0] & a1
                    or not tb.nbr[v0] & a0):
                continue
        tg = target(Q[v0] + Q[v1], v[v0], v[v1])
        x = 0.5 * (v[v0] + v[v1]) if mutate == "midpoint" else tg.x
        if _admissible(tb, v, v0, v1, x, keep_manifold, check_flip=mutate != "no_flip",
                       check_link=mutate != "no_link"):
            continue
        slipped = slipped or v0 in blocked or v1 in blocked
        pairs.append((v0, v1))
        v2[v0] = x
        if mutate != "wrong_sum":
            Q2[v0] = Q[v0] + Q[v1]
        ends.update((v0, v1))
        a0.add(v0)
        a1.add(v1)
        blocked.update({v0, v1} | tb.nbr[v0] | tb.nbr[v1])
        if mutate == "move_ring" and len(pairs) == 1:
            ring = sorted(tb.nbr[v0] - tb.nbr[v1] - {v1}) or sorted(tb.nbr[v0] - {v1})
            v2[ring[0], 0] = np.nextafter(v2[ring[0], 0], np.inf)
            blocked.update(tb.nbr[ring[0]] | {ring[0]})        # nothing else touches it
        if mutate == "beyond_budget":
            break
    return v2, _apply_faces(f, pairs), Q2
