"""Hand-built clouds for smx_recon_import_points, one per decision of the definition (include/smx.h): what each case is for is its
`decision`; tests/test_import_model.py prints decision -> case and mutant -> case.  Coordinates are exact float32 values chosen
so that the deciding comparison is an equality or one ulp off it.  MATRICES are the two situations of the Jacobi step that no
cloud reaches through float32 differences (an infinite theta needs |a_pq| below 1e-231 |a_qq - a_pp|), given as matrices."""
import numpy as np

import import_ref as ir

F = np.float32
STEP = F(1.0 / 64.0)


class Case:
    def __init__(self, name, decision, points, colors=None, origins=None, old_rows=None, max_surfels=None, **prm):
        self.name, self.decision = name, decision
        self.points = np.ascontiguousarray(np.asarray(points, F).reshape(-1, 3))
        self.colors = None if colors is None else np.ascontiguousarray(colors, np.uint32)
        self.origins = None if origins is None else np.ascontiguousarray(np.asarray(origins, F).reshape(-1, 3))
        self.old_rows = ir.blank_rows(0) if old_rows is None else np.ascontiguousarray(old_rows, F)
        n_imported_bound = self.old_rows.shape[1] + self.points.shape[0]
        self.max_surfels = n_imported_bound + 8 if max_surfels is None else max_surfels
        self.prm = ir.params(**prm)

    def model(self, mutant=None, lists=None):
        return ir.import_model(self.points, self.colors, self.origins, self.prm, self.old_rows, self.max_surfels, mutant=mutant, lists=lists)


def grid(nx, ny, step=STEP, z=0.0):
    gx, gy = np.meshgrid(np.arange(nx, dtype=F) * F(step), np.arange(ny, dtype=F) * F(step))
    return np.stack([gx.ravel(), gy.ravel(), np.full(nx * ny, z, F)], axis=1).astype(F)


def patch(n, seed, density=0.03, bump=0.02):
    """n points of a bumpy surface z = bump sin(8x) cos(8y) over a square whose side grows with sqrt(n)."""
    rng = np.random.default_rng(seed)
    side = max(np.sqrt(max(n, 1)) * density, 0.05)
    xy = rng.uniform(0.0, side, (n, 2))
    z = bump * np.sin(8.0 * xy[:, 0]) * np.cos(8.0 * xy[:, 1])
    return np.concatenate([xy, z[:, None]], axis=1).astype(F)


def colors_of(n, seed=0):
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)) & np.uint32(0x00FFFFFF)


def old_map(n, z=5.0):
    rows = ir.blank_rows(n)
    g = grid(n, 1, z=z)
    rows[0:3] = g.T
    rows[3:6] = g.T
    rows[6] = 2.0
    rows[7] = F(1e-4)
    rows[10] = 1.0
    ir.u32(rows)[17:19] = 7
    ir.u32(rows)[24] = 0x00112233
    return rows


def _threshold_pair():
    """A patch and the two adjacent float32 thresholds between which its point 0 changes from kept to ROUGH."""
    pts = patch(40, 21, bump=0.03)
    base = dict(search_radius=0.5, k=16, min_neighbors=6)
    ex = ir.import_model(pts, p=ir.params(**base))[3]
    lam = ex["lam"][0]
    total = (lam[0] + lam[1]) + lam[2]
    f = F(lam[0] / total)
    cand = [np.nextafter(f, F(0)), f, np.nextafter(f, F(1))]
    rough = [bool(lam[0] > np.float64(c) * total) for c in cand]
    at = rough.index(False)      # the smallest threshold that keeps the point; the one below rejects it
    assert at >= 1 and rough[at - 1]
    return pts, base, float(cand[at]), float(cand[at - 1])


def cases():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))
    far = np.array([4.0, 0.0, 0.0], F)
    six = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0], [1, 1, 0], [2, 1, 0.5], [1, 2, 0]], F) * STEP
    add("m_equal_min_and_one_below", "SPARSE: m == min_neighbors is kept, m == min_neighbors - 1 is not; radius_rank >= m uses the last entry",
        np.concatenate([six, six[:5] + far]), colors=colors_of(11), min_neighbors=6, k=16, radius_rank=8)
    r = F(0.125)
    ball = np.array([[0, 0, 0], [r, 0, 0], [-np.nextafter(r, F(1)), 0, 0], [0.01, 0.02, 0.005], [-0.02, 0.01, -0.004]], F)
    add("on_the_ball_and_one_ulp_outside", "List: d2 == r^2 is inside, one ulp more is outside", ball, search_radius=float(r), k=8, min_neighbors=4,
        radius_rank=2)
    add("exact_duplicates", "Radius: a list of duplicates gives RadiusSquared 0: DEGENERATE", np.tile(np.array([[0.25, 0.5, 0.75]], F), (10, 1)),
        k=8, min_neighbors=3, radius_rank=3)
    add("collinear_on_x", "Eigenvectors: two zero eigenvalues, the tie goes to the lowest column", grid(12, 1), k=8, min_neighbors=3, radius_rank=2)
    diag = np.stack([np.arange(12, dtype=F) * STEP, np.arange(12, dtype=F) * STEP, np.zeros(12, F)], axis=1)
    add("diagonal_line", "Jacobi: a_pp == a_qq gives theta == 0 and t == 1", diag, k=8, min_neighbors=3, radius_rank=2)
    add("planar_grid", "Jacobi: every a_pq == 0 skip, the normal exactly +z; ROUGH: lam0 == threshold (0 == 0) is kept", grid(9, 9), colors=colors_of(81, 5),
        search_radius=float(F(2.5) * STEP), k=32, min_neighbors=6, radius_rank=8, max_surface_variation=0.0)
    add("dot_zero_view_point", "Orientation: a dot of exactly 0 keeps the normal (view point in the plane)", grid(6, 6), search_radius=0.05, k=16,
        orient=ir.ORIENT_VIEW_POINT, view_point=(10.0, 10.0, 0.0))
    g = grid(6, 6)
    add("dot_zero_origins", "Orientation: a dot of exactly 0 keeps the normal (origins in the plane)", g, origins=g + np.array([1.0, -2.0, 0.0], F),
        search_radius=0.05, k=16, orient=ir.ORIENT_ORIGINS)
    add("orient_view_point_flips", "Orientation: a negative dot negates the normal", grid(6, 6), search_radius=0.05, k=16, orient=ir.ORIENT_VIEW_POINT,
        view_point=(0.0, 0.0, -3.0))
    pts = patch(60, 3)
    pts[7, 1] = np.nan
    pts[19, 0] = np.inf
    pts[33, 2] = -np.inf
    org = pts + np.array([0.0, 0.0, 2.0], F)
    org[40, 0] = np.nan
    org[41, 2] = np.inf
    add("nan_inf_coordinates_and_origins", "BAD: non-finite coordinates and origins; a BAD point is no neighbour", pts, colors=colors_of(60, 9), origins=org,
        orient=ir.ORIENT_ORIGINS, search_radius=0.06, k=16)
    add("nan_origins_ignored_without_origins_mode", "BAD: origins are not looked at unless orient is ORIGINS", pts, origins=org, orient=ir.ORIENT_VIEW_POINT,
        view_point=(0.0, 0.0, 2.0), search_radius=0.06, k=16)
    tp, base, keep_at, reject_at = _threshold_pair()
    add("variation_at_the_threshold", "ROUGH: lam0 == (or just under) the threshold keeps point 0", tp, max_surface_variation=keep_at, **base)
    add("variation_one_ulp_above", "ROUGH: the next smaller float32 threshold rejects point 0", tp, max_surface_variation=reject_at, **base)
    h = F(0.25) * STEP
    tie = np.array([[0, 0, 0], [STEP, 0, h], [-STEP, 0, h], [0, STEP, -h], [0, -STEP, -h]], F)      # (a saddle: which three enter decides the plane)
    add("k4_tie_by_index", "List: equal d2, the lower index enters a full list; k = 4 saturated", tie, k=4, min_neighbors=4, radius_rank=1, search_radius=0.05)
    add("k64_dense_patch", "k = 64, every list saturated, radius_rank 63", patch(300, 11, density=0.004), k=64, min_neighbors=6, radius_rank=63,
        search_radius=0.1)
    add("k5_scalar_rows", "a k that is no multiple of 4: list rows are not 16-byte pieces", patch(150, 12), k=5, min_neighbors=4, radius_rank=3)
    p40 = patch(40, 13)
    add("capacity_exact", "Append: old_size + n_imported == capacity fits", p40, old_rows=old_map(3), max_surfels=3 + 40, search_radius=0.5)
    add("capacity_one_short", "Append: one slot short is refused, the map unchanged", p40, old_rows=old_map(3), max_surfels=3 + 39, search_radius=0.5)
    add("non_empty_map", "Append: behind the slots of a map that holds surfels; colours given", patch(90, 14), colors=colors_of(90, 1), old_rows=old_map(17),
        confidence=2.5, frame_index=9)
    add("default_color", "Row 24: default_color where colors is NULL", patch(50, 15), default_color=0x00ABCDEF, search_radius=0.5)
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        add("n_%d" % n, "Sizes: the wavefront and the 1024-point segment edges", patch(n, 100 + n), colors=colors_of(n, n) if n % 2 else None,
            orient=ir.ORIENT_VIEW_POINT, view_point=(0.0, 0.0, 1.0))
    return out


def _sym(a00, a01, a02, a11, a12, a22):
    return {(0, 0): np.array([a00]), (0, 1): np.array([a01]), (0, 2): np.array([a02]), (1, 1): np.array([a11]), (1, 2): np.array([a12]),
            (2, 2): np.array([a22])}


# name -> the six entries of a symmetric matrix handed to the Jacobi iteration directly
MATRICES = {
    "theta_infinite": _sym(1.0, 1e-320, 0.0, 3.0, 0.0, 2.0),          # (a_qq - a_pp) / (2 a_pq) overflows: t = 0, only a_pq is cleared
    "theta_squared_infinite": _sym(1.0, 1e-200, 0.0, 3.0, 0.0, 2.0),  # theta finite, theta^2 infinite: t = 0 as well
    "theta_zero": _sym(2.0, 0.5, 0.0, 2.0, 0.0, 1.0),                 # a_pp == a_qq
    "all_pairs_zero": _sym(3.0, 0.0, 0.0, 1.0, 0.0, 1.0),             # every pair skipped; the tie of columns 1 and 2
    "general": _sym(4.0, 1.0, -0.5, 3.0, 0.25, 1.0),
}
