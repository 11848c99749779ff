"""Small hand-built surfel maps that reach the decisions of smx_recon_triangulate / smx_recon_triangulate_update which no
noisy map reaches (full ring rows, the wrap of the closing pair, overflow, open stars, every drop and every rejection),
and the rule that lets their results be compared exactly (test infrastructure, no GPU needed).

The margin rule is a condition on the inputs.  sweep() evaluates in float64, on the float32-valued inputs, every quantity
whose sign or comparison decides something for a map: ball membership d^2 <= f^2 r^2, dot(n_p, n_j) > cos_max_normal,
x^2 + y^2 > 1e-12 r^2, every mesh_cross2 and mesh_incircle among one slot's candidates (in the basis mesh_basis builds),
the three angle cosines against both limits, and s and the three normal dots of mesh_triangle_filter.  Each has to lie at
least MARGIN times the sum of the absolute values of its terms away from where it flips; a float32 evaluation errs by a
few units of 6e-8 of that sum.  The same sweep derives every slot's star from the definition (successor = positive turn
and no candidate strictly inside the circle), a second reference that does not go through Qhull.

What cannot be built, and why (test_mesh_cases.py prints this list):
"""
import math

import numpy as np

import mesh_ref as mr

MARGIN = 1e-3
LONG_RING = 32                     # candidates of a slot above which its in-circle values are held to LONG_RING_MARGIN
LONG_RING_MARGIN = 1e-4
MAX_DEG = mr.MAX_STAR_DEGREE

NOT_CONSTRUCTIBLE = {
    "D3 at MARGIN": "a closed ring of m members has a mean exterior angle of 2 pi / m in the inverted plane, so the in-circle "
                    "determinant of three neighbours is about (2 pi / m)^3 / 3 of its term sum: 3e-4 at m = 63.  The rings "
                    "of 40 and 63 (slots with more than LONG_RING candidates) are held to an in-circle margin of "
                    "LONG_RING_MARGIN = 1e-4 instead, which is still 200 float32 error bounds, and in every other "
                    "quantity to MARGIN.",
    "D6 filter 2": "k_mesh_agree hands mesh_triangle_filter the pair (a, b) in the owner's ring order, counter-clockwise "
                   "about n_p, so cross(A - P, B - P) . n_p > 0; a verdict of 2 flips the normal and then fails its own "
                   "n . n_p > 0.  A verdict of 2 is never an accepted triangle.  The owners here are placed with ring "
                   "orders that run against the index order instead (normal (0, 0, -1), permuted ring indices), where "
                   "the model's (p, a, b) has a > b.",
    "D6 last slot": "an owner is the smallest corner of its triangles, so the last slot owns nothing.  The owner of 16 is "
                    "the last slot that owns anything: its run ends the output, its ring fills the last 16 slots.",
    "D7 degree 1": "a ring member is a member of a pair, so a star has degree 0 or at least 2.  The case holds a slot "
                   "with exactly one candidate (degree 0) in its place.",
}
__doc__ += "".join("  %s: %s\n" % kv for kv in NOT_CONSTRUCTIBLE.items())


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def kernel_basis(n):
    """mesh_basis of smx_mesh.hpp in float64."""
    a = np.abs(n)
    e = np.zeros(3)
    e[0 if (a[0] <= a[1] and a[0] <= a[2]) else 1 if a[1] <= a[2] else 2] = 1.0
    nn = n @ n
    t = e - (e @ n) / nn * n
    u = t / math.sqrt(t @ t)
    return u, np.cross(n, u) / math.sqrt(nn)


def pseudo_angle(x, y):
    p = x / (abs(x) + abs(y))
    return 1.0 - p if y >= 0 else 3.0 + p


class Margins:
    """The smallest |value| / sum |terms| seen per kind of quantity, and where."""

    def __init__(self):
        self.least = {}

    def add(self, kind, value, terms, where):
        value, terms = np.asarray(value, np.float64), np.asarray(terms, np.float64)
        if value.size == 0:
            return
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(terms > 0, np.abs(value) / terms, np.inf)
        k = int(np.argmin(ratio))
        r = float(ratio.reshape(-1)[k])
        if kind not in self.least or r < self.least[kind][0]:
            self.least[kind] = (r, where, k)


def _slot_star(p, pos, nrm, r2, prm, live, mg, exempt):
    """Candidates (slot indices, in the kernel's basis: x, y) and the star pairs of slot p, by the definition."""
    f2 = float(np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor))
    ids = np.nonzero(live)[0]
    d = pos[ids] - pos[p]
    d2 = np.sum(d * d, axis=1)
    rr = f2 * r2[p]
    checked = np.array([(p, int(j)) not in exempt for j in ids]) if exempt else np.ones(ids.size, bool)
    mg.add("ball", (d2 - rr)[checked], (d2 + rr)[checked], "slot %d" % p)
    near = d2 <= rr
    full = int(near.sum()) >= prm.max_neighbors
    assert int(near.sum()) <= prm.max_neighbors, "slot %d: %d slots in the ball: the cut would choose among them" % (p, near.sum())
    near &= ids != p
    ids, d = ids[near], d[near]
    cosn = math.cos(math.radians(prm.max_angle_between_normals_deg))
    dots = nrm[ids] @ nrm[p]
    mg.add("normal", dots - cosn, np.abs(nrm[ids]) @ np.abs(nrm[p]) + abs(cosn), "slot %d" % p)
    keep = dots > cosn
    ids, d = ids[keep], d[keep]
    u, v = kernel_basis(nrm[p])
    x, y = d @ u, d @ v
    q = x * x + y * y
    mg.add("projection", q - 1e-12 * r2[p], q + 1e-12 * r2[p], "slot %d" % p)
    keep = q > 1e-12 * r2[p]
    ids, x, y, q = ids[keep], x[keep], y[keep], q[keep]
    m = ids.size
    if m < 2:
        return ids, x, y, set(), full
    cr = x[:, None] * y[None, :] - y[:, None] * x[None, :]
    off = ~np.eye(m, dtype=bool)
    mg.add("cross2", cr[off], (np.abs(x[:, None] * y[None, :]) + np.abs(y[:, None] * x[None, :]))[off], "slot %d" % p)
    pairs = set()
    if m == 2:
        if cr[0, 1] != 0:
            pairs.add((int(ids[0]), int(ids[1])) if cr[0, 1] > 0 else (int(ids[1]), int(ids[0])))
        return ids, x, y, pairs, full
    A = lambda a: a[:, None, None]
    B = lambda a: a[None, :, None]
    Cc = lambda a: a[None, None, :]
    t = [A(x) * B(y) * Cc(q), -A(x) * B(q) * Cc(y), -A(y) * B(x) * Cc(q), A(y) * B(q) * Cc(x), A(q) * B(x) * Cc(y), -A(q) * B(y) * Cc(x)]
    inc = t[0] + t[1] + t[2] + t[3] + t[4] + t[5]
    terms = sum(np.abs(e) for e in t)
    i = np.arange(m)
    distinct = (A(i) != B(i)) & (A(i) != Cc(i)) & (B(i) != Cc(i))
    mg.add("incircle" if m <= LONG_RING else "incircle, long ring", inc[distinct], terms[distinct], "slot %d" % p)
    # successor of a: b with a positive turn and no third candidate strictly inside the circle (origin, a, b)
    empty = np.all((inc >= 0) | ~distinct, axis=2)
    succ = (cr > 0) & empty & off
    for a, b in zip(*np.nonzero(succ)):
        pairs.add((int(ids[a]), int(ids[b])))
    return ids, x, y, pairs, full


def _filter_margins(p, a, b, pos, nrm, prm, mg):
    """mesh_triangle_filter on (p, a, b) in float64: its verdict, and the margins of everything it compares."""
    P, A, B = pos[p], pos[a], pos[b]
    lo, hi = math.cos(math.radians(prm.min_triangle_angle_deg)), math.cos(math.radians(prm.max_triangle_angle_deg))
    where = "triangle (%d, %d, %d)" % (p, a, b)
    ok = True
    for at, o1, o2 in ((P, A, B), (A, B, P), (B, P, A)):
        e, f = o1 - at, o2 - at
        den = math.sqrt((e @ e) * (f @ f))
        c = (e @ f) / den
        for lim in (lo, hi):
            mg.add("angle", c - lim, np.abs(e) @ np.abs(f) / den + abs(lim), where)
        ok &= hi <= c <= lo
    e, f = A - P, B - P
    tn = np.cross(e, f)
    tabs = np.array([abs(e[1] * f[2]) + abs(e[2] * f[1]), abs(e[2] * f[0]) + abs(e[0] * f[2]), abs(e[0] * f[1]) + abs(e[1] * f[0])])
    w = nrm[p] + nrm[a] + nrm[b]
    s = tn @ w
    if not ok:
        return 0
    mg.add("filter s", s, tabs @ np.abs(w), where)
    if s == 0:
        return 0
    if s < 0:
        tn = -tn
    for c in (p, a, b):
        mg.add("filter dot", tn @ nrm[c], tabs @ np.abs(nrm[c]), where)
        ok &= tn @ nrm[c] > 0
    return 0 if not ok else (1 if s > 0 else 2)


class Sweep:
    """What sweep() found: .stars (slot -> set of frozenset({a, b}); empty for an overflowed slot), .degree (slot -> ring
    members, before the overflow rule), .ring (slot -> members in the kernel's ring order), .closed (slot -> every ring
    member has a successor), .overflow / .full (slot sets), .star_triangles (set of frozensets), .verdict (agreed
    triangle (p, a, b) in the owner's ring order -> filter verdict 0 / 1 / 2), .owned (slot -> accepted triangles),
    .candidates (slot -> candidate count) and .margins (kind -> (least ratio, where, flat index))."""


def sweep(pos, nrm, r2, prm, exempt=()):
    live = mr.live_mask(pos, r2)
    mg = Margins()
    sw = Sweep()
    sw.stars, sw.degree, sw.ring, sw.closed, sw.overflow, sw.full, sw.candidates = {}, {}, {}, {}, set(), set(), {}
    directed = {}
    exempt = set(exempt)
    for p in np.nonzero(live)[0]:
        p = int(p)
        ids, x, y, pairs, full = _slot_star(p, pos, nrm, r2, prm, live, mg, exempt)
        if full:
            sw.full.add(p)
        sw.candidates[p] = int(ids.size)
        members = sorted(set(v for e in pairs for v in e))
        ang = {int(j): (pseudo_angle(x[k], y[k]), k) for k, j in enumerate(ids)}
        sw.degree[p] = len(members)
        sw.ring[p] = sorted(members, key=lambda j: ang[j])
        sw.closed[p] = len(members) > 0 and len(set(a for a, _ in pairs)) == len(members) and ids.size > 2
        if len(members) > MAX_DEG:
            sw.overflow.add(p)
            pairs = set()
        directed[p] = pairs
        sw.stars[p] = set(frozenset(e) for e in pairs)
    sw.star_triangles = set(frozenset((p, a, b)) for p, s in directed.items() for a, b in s)
    sw.verdict, sw.owned = {}, {p: 0 for p in directed}
    for p, s in directed.items():
        for a, b in s:
            if p < a and p < b and frozenset((p, b)) in sw.stars.get(a, ()) and frozenset((p, a)) in sw.stars.get(b, ()):
                v = _filter_margins(p, a, b, pos, nrm, prm, mg)
                sw.verdict[(p, a, b)] = v
                sw.owned[p] += 1 if v else 0
    sw.margins = mg.least
    return sw


# ---- the maps ----
class Case:
    """One map and one parameter set.  .claims: the decision ids the case says it reaches; .exempt: (slot, other) pairs
    whose ball membership is exact by construction instead of clear by MARGIN (D11); .roles: name -> slot or slots, for
    the checks that a decision is reached."""

    def __init__(self, name, m, prm, claims, roles, exempt=()):
        self.name, self.prm, self.claims, self.roles = name, prm, set(claims), roles
        self.pos, self.nrm, self.r2 = m
        self.exempt = tuple(exempt)

    @property
    def map(self):
        return self.pos, self.nrm, self.r2

    @staticmethod
    def margin_of(kind):
        return LONG_RING_MARGIN if kind == "incircle, long ring" else MARGIN


class Layout:
    """Slots in the order they are put."""

    def __init__(self):
        self.pos, self.nrm, self.r2 = [], [], []
        self.n_lonely = 0

    @property
    def n(self):
        return len(self.r2)

    def put(self, point):
        pos, nrm, r2 = point
        self.pos.append(np.asarray(pos, np.float64))
        self.nrm.append(np.asarray(nrm, np.float64))
        self.r2.append(float(r2))
        return self.n - 1

    def put_all(self, points):
        return [self.put(pt) for pt in points]

    def lonely(self, merged=False):
        """A live slot far from every other (its list holds only itself), or a merged one."""
        k = self.n_lonely
        self.n_lonely += 1
        return self.put(((2.0 * (k % 16), 2.0 * (k // 16), 12.0), (0.0, 0.0, 1.0), -1.0 if merged else 0.25))

    def fill_to(self, n):
        while self.n < n:
            self.lonely()

    def map(self):
        return f32(np.array(self.pos)), f32(np.array(self.nrm)), f32(np.array(self.r2))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def centre(k):
    """Patch centres 4 apart: no ball (radius <= 1.3, at search factor 1) reaches another patch."""
    return np.array([4.0 * (k % 8), 4.0 * (k // 8), 0.0])


def place(xy, c, normal, r2, normals=None):
    """Points of the plane through c with the given normal, as (pos, nrm, r2) triples."""
    n = _unit(normal)
    u, v = mr.basis(n)
    out = []
    for k, (x, y) in enumerate(xy):
        out.append((c + x * u + y * v, n if normals is None else _unit(normals[k]), r2[k] if np.ndim(r2) else r2))
    return out


# ring radius of the ring members' balls: they reach the hub, and their second neighbours but not the third
_RING_BALL = {15: 1.1, 16: 1.06}


def ring_xy(m, seed, skip=()):
    """m points around the origin at radius 1 + amp cos(k theta), the angles jittered: convex after inversion (all of
    them are in the origin's star), and clear of cocircular quadruples.  A long ring (its members see nobody) lies on
    the circle, at equal steps if m is odd and jittered just enough to have no two members opposite each other if even."""
    amp, k, jitter = (0.04, 5, 0.12) if m <= 20 else (0.0, 5, 0.0 if m % 2 else 0.04)
    th = 2 * np.pi * np.arange(m) / m + 0.1
    th = th + jitter * np.random.default_rng(seed).uniform(-1, 1, m) * 2 * np.pi / m
    rad = 1 + amp * np.cos(k * th + 0.3)
    return [(rad[i] * math.cos(th[i]), rad[i] * math.sin(th[i])) for i in range(m) if i not in skip]


def ring_patch(m, c, normal, seed, ring_ball=None, hub_ball=1.2, perm=None):
    """(hub, ring members): the ring members in the order of their angle, or permuted."""
    xy = ring_xy(m, seed)
    rb = ring_ball if ring_ball is not None else _RING_BALL.get(m, 1.2 if m <= 20 else 0.05)
    pts = place([(0.0, 0.0)] + xy, c, normal, [hub_ball ** 2] + [rb ** 2] * m)
    ring = pts[1:]
    if perm is not None:
        ring = [ring[i] for i in perm]
    return pts[0], ring


_RING_BALL[17] = 1.15
_SEED = {15: 0, 16: 1, 17: 8, 40: 0, 63: 1}      # chosen so that the margins hold under every normal below
NORMALS = ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1.0, 1.0), (0.3, -0.2, 0.9), (0.1, 0.7, -0.7), (0.0, 0.0, -1.0))


def _ring(lay, roles, m, k, normal, hub_first, perm=None, role=None):
    hub, ring = ring_patch(m, centre(k), normal, _SEED.get(m, 0), perm=perm)
    if hub_first:
        h = lay.put(hub)
        members = lay.put_all(ring)
    else:
        members = lay.put_all(ring)
        h = lay.put(hub)
    roles.setdefault(role or "hub%d_%s" % (m, "first" if hub_first else "last"), []).append(h)
    roles.setdefault("rings", {})[h] = members
    return h, members


def composite_layout():
    """Hubs of degree 15, 16, 17 and 63 in both index orders, one of 40, under six normals: 12 patches."""
    lay, roles = Layout(), {}
    plan = ((15, 0, True), (15, 1, False), (16, 2, True), (16, 3, False), (17, 4, True), (17, 5, False), (40, 0, True),
            (63, 3, True), (63, 2, False), (16, 0, True), (16, 1, True), (17, 0, True))
    for k, (m, nk, first) in enumerate(plan):
        _ring(lay, roles, m, k, NORMALS[nk], first)
    return lay, roles


# U4: the appended slot lies between ring members U4_AFTER and U4_AFTER + 1 of its hub, at U4_RADIUS times their mean radius
U4_AFTER, U4_RADIUS = 0, 1.0


def _moved_away(lay, slot):
    """The slot three units along its normal: out of every ball, its own reaches nobody."""
    lay.pos[slot] = lay.pos[slot] + 3.0 * lay.nrm[slot]


def update_steps():
    """[(name, map, rows touched since the previous map)]: the composite, then U1 .. U5 of the issue."""
    lay, roles = composite_layout()
    steps = [("U0", lay.map(), None)]
    hub17 = roles["hub17_first"][1]
    member = roles["rings"][hub17][5]
    home = lay.pos[member].copy()
    _moved_away(lay, member)                             # U1: the hub goes 17 -> 16 and gains its triangles
    steps.append(("U1", lay.map(), 1))
    lay.pos[member] = home                               # U2: and back, 16 -> 17
    steps.append(("U2", lay.map(), 1))
    hub16 = roles["hub16_first"][1]
    lay.r2[roles["rings"][hub16][3]] = -1.0              # U3: a ring member of a 16-hub is merged, 16 -> 15
    steps.append(("U3", lay.map(), 1))
    hub16b = roles["hub16_first"][2]                     # U4: a slot is appended inside a 16-hub's ring, 16 -> 17
    ring = roles["rings"][hub16b]
    a, b = lay.pos[ring[U4_AFTER]] - lay.pos[hub16b], lay.pos[ring[U4_AFTER + 1]] - lay.pos[hub16b]
    mid = _unit(a + b) * (0.5 * (np.linalg.norm(a) + np.linalg.norm(b)) * U4_RADIUS)
    lay.put((lay.pos[hub16b] + mid, lay.nrm[hub16b], lay.r2[ring[0]]))
    steps.append(("U4", lay.map(), 1))
    steps.append(("U5", lay.map(), 0))
    roles.update(u1_hub=hub17, u3_hub=hub16, u4_hub=hub16b)
    return steps, roles



def trip_layout():
    """The four wavefronts of one k_mesh_star trip hold an overflowed, a degree-16, a merged and a lonely slot (D5); owners
    of 16 triangles sit at slots 255 and 256 and own the end of the output (D6); a hub's ring holds a merged slot and one
    with a NaN coordinate (D12); the slot count is no multiple of 4."""
    lay, roles = Layout(), {}
    hub17, ring17 = ring_patch(17, centre(0), NORMALS[0], _SEED[17])
    hub16, ring16 = ring_patch(16, centre(1), NORMALS[3], _SEED[16])
    roles["trip"] = [lay.put(hub17), lay.put(hub16), lay.lonely(merged=True), lay.lonely()]
    lay.put_all(ring17)
    lay.put_all(ring16)
    # D12: ring of 8, with a merged slot and a NaN slot where two further members would be
    xy = ring_xy(10, 3)
    pts = place([(0.0, 0.0)] + xy, centre(2), NORMALS[2], [1.2 ** 2] * 11)
    roles["d12_hub"] = lay.put(pts[0])
    ids = lay.put_all(pts[1:])
    roles["d12_merged"], roles["d12_nan"] = ids[2], ids[6]
    lay.r2[ids[2]] = -1.0
    lay.pos[ids[6]] = lay.pos[ids[6]] * np.array([np.nan, 1.0, 1.0])
    lay.fill_to(255)
    perm = np.random.default_rng(5).permutation(16)
    hub_a, ring_a = ring_patch(16, centre(3), NORMALS[5], _SEED[16])          # counter-clockwise about -z: descending indices
    hub_b, ring_b = ring_patch(16, centre(4), NORMALS[2], _SEED[16], perm=perm)
    roles["owners"] = [lay.put(hub_a), lay.put(hub_b)]
    lay.put_all(ring_a)
    lay.put_all(ring_b)
    hub_c, ring_c = ring_patch(16, centre(5), NORMALS[4], _SEED[16], perm=np.roll(perm, 3))
    roles["owners"].append(lay.put(hub_c))
    lay.put_all(ring_c)
    assert roles["owners"][:2] == [255, 256] and lay.n % 4 != 0 and lay.n % 256 != 0
    return lay, roles


def odds_layout():
    """Open stars (D7), the candidate drops (D8 a, c), agreement failing (D9) and the filter rejecting (D10)."""
    lay, roles = Layout(), {}
    z = NORMALS[0]
    roles["lonely"] = lay.lonely()                                              # D7 degree 0, D8 a list that holds only p
    # a boundary hub: five members over 120 degrees, the gap across the direction the kernel's ring order starts from
    th = np.radians([20.0, 52.0, 79.0, 111.0, 140.0])
    rad = np.array([1.0, 0.93, 1.04, 0.96, 1.02])
    pts = place([(0.0, 0.0)] + [(r * math.cos(t), r * math.sin(t)) for r, t in zip(rad, th)], centre(0), z, 1.2 ** 2)
    roles["boundary_hub"] = lay.put(pts[0])
    lay.put_all(pts[1:])
    # D8 c: a ring of 6 and a slot straight above the hub, inside the hub's ball only
    hub, ring = ring_patch(6, centre(1), z, 2, ring_ball=1.25)
    roles["d8c_hub"] = lay.put(hub)
    lay.put_all(ring)
    roles["d8c_above"] = lay.put((hub[0] + 0.9 * _unit(z), z, 0.3 ** 2))
    # D9 unequal radii: a's ball reaches p, not b
    c = centre(2)
    roles["d9_radii"] = lay.put_all([(c, z, 1.2 ** 2), (c + (0.8, 0.0, 0.0), z, 0.9 ** 2), (c + (0.3, 0.9, 0.0), z, 1.2 ** 2)])
    # D9 tangent planes: a rhombus whose short diagonal is p-b; seen from a and c (tilted 60 degrees about it) it is a-c
    c = centre(3)
    t = (0.0, math.sin(math.radians(60.0)), math.cos(math.radians(60.0)))
    roles["d9_planes"] = lay.put_all([(c + (-0.6, 0.0, 0.0), z, 1.6 ** 2), (c + (0.0, -0.75, 0.0), t, 1.6 ** 2),
                                      (c + (0.6, 0.0, 0.0), z, 1.6 ** 2), (c + (0.0, 0.75, 0.0), t, 1.6 ** 2)])
    # D10: a thin triangle (5.7 degrees), a flat one (166 degrees), one whose third normal is 100 degrees off
    c = centre(4)
    roles["d10_thin"] = lay.put_all([(c, z, 1.2 ** 2), (c + (1.0, 0.0, 0.0), z, 1.2 ** 2), (c + (1.0, 0.1, 0.0), z, 1.2 ** 2)])
    c = centre(5)
    roles["d10_flat"] = lay.put_all([(c, z, 1.2 ** 2), (c + (1.0, 0.1228, 0.0), z, 2.2 ** 2), (c + (-1.0, 0.1228, 0.0), z, 2.2 ** 2)])
    c = centre(6)
    t = (0.0, math.sin(math.radians(100.0)), math.cos(math.radians(100.0)))
    roles["d10_normal"] = lay.put_all([(c, z, 1.2 ** 2), (c + (1.0, 0.0, 0.0), z, 1.2 ** 2), (c + (0.4, 0.8, 0.0), t, 1.2 ** 2)])
    lay.lonely()
    return lay, roles


SHEETS_SEED = 0


def sheets_layout():
    """Two sheets in one plane, their points interleaved, the normals 174.3 degrees apart (exactly opposite normals mix
    at no setting: dot = -1 is not above cos 180, and would sit on that threshold)."""
    rng = np.random.default_rng(SHEETS_SEED)
    pts = []
    while len(pts) < 20:
        p = rng.uniform(0.0, 3.2, 2)
        if all(np.linalg.norm(p - q) > 0.55 for q in pts):
            pts.append(p)
    lay = Layout()
    up, down = _unit((0.0, 0.0, 1.0)), _unit((0.1, 0.0, -1.0))
    for k, p in enumerate(pts):
        lay.put(((p[0], p[1], 0.0), up if k % 2 == 0 else down, 1.3 ** 2))
    return lay, {"up": list(range(0, 20, 2)), "down": list(range(1, 20, 2))}


def edge_layout():
    """D11.  Two patches, one for each search factor.  p's normal is x; its candidates lie in the y-z plane: one at
    d^2 == f^2 r^2 exactly, one at the next float32 above, one well inside.  All coordinates are small dyadic numbers and the
    sums dx dx + dy dy + dz dz run from small to large, so float32 and float64 hold d^2 and f^2 r^2 exactly."""
    lay, roles = Layout(), {}
    nx = (1.0, 0.0, 0.0)
    r2 = 1.0 + 2.0 ** -23
    for name, f, c in (("f1", 1.0, np.array([0.0, 0.0, 0.0])), ("f2", 2.0, np.array([16.0, 0.0, 0.0]))):
        p = lay.put((c, nx, r2))
        on = lay.put((c + (f * 2.0 ** -12, f * 2.0 ** -12, f), nx, 2.0 ** -8))        # d^2 = f^2 (1 + 2^-23)
        off = lay.put((c + (f * 2.0 ** -11, f, 0.0), nx, 2.0 ** -8))                   # d^2 = f^2 (1 + 2^-22)
        inside = lay.put((c + (0.0, -0.5 * f, -0.5 * f), nx, 2.0 ** -8))
        roles[name] = dict(p=p, on=on, off=off, inside=inside)
    return lay, roles


def cases():
    out = []
    lay, roles = composite_layout()
    out.append(Case("composite", lay.map(), mr.Params(), {"D1", "D2", "D3", "D4"}, roles))
    lay, roles = trip_layout()
    out.append(Case("trip", lay.map(), mr.Params(), {"D2", "D5", "D6", "D12"}, roles))
    lay, roles = odds_layout()
    out.append(Case("odds", lay.map(), mr.Params(), {"D7", "D8", "D9", "D10"}, roles))
    out.append(Case("odds_wide", lay.map(), mr.Params(max_angle_between_normals_deg=120.0, min_triangle_angle_deg=1.0, max_triangle_angle_deg=160.0),
                    {"D10"}, roles))
    lay, roles = sheets_layout()
    out.append(Case("sheets_90", lay.map(), mr.Params(), {"D8"}, roles))
    out.append(Case("sheets_178", lay.map(), mr.Params(max_angle_between_normals_deg=178.0), {"D8"}, roles))
    lay, roles = edge_layout()
    exempt = [(r["p"], r[k]) for r in roles.values() for k in ("on", "off")]
    out.append(Case("edge_f1", lay.map(), mr.Params(search_radius_factor=1.0), {"D11"}, roles, exempt))
    out.append(Case("edge_f2", lay.map(), mr.Params(search_radius_factor=2.0), {"D11"}, roles, exempt))
    return out
