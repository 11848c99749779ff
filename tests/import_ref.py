"""The model of smx_recon_import_points (include/smx.h): brute-force numpy (test infrastructure, no GPU needed).
Every float32 and double expression is evaluated as the definition writes it, one rounding per operation: the lists by
(d2 bits, index), the nine sums in list order, the Jacobi iteration vectorised over the points with masks.

import_model(..., mutant=...) evaluates a deliberately wrong definition instead (tests/test_import_model.py: each mutant must
fail a named case)."""
import numpy as np

F = np.float32
D = np.float64
INVALID = np.uint32(0xFFFFFFFF)
ROWS = 25
SWEEPS = 6                                  # SMX_IMPORT_JACOBI_SWEEPS
BAD, SPARSE, DEGENERATE, ROUGH, OK = 0, 1, 2, 3, 4
ORIENT_NONE, ORIENT_VIEW_POINT, ORIENT_ORIGINS = 0, 1, 2
STAT_NAMES = ("n_points", "n_bad", "n_sparse", "n_degenerate", "n_rough", "n_imported", "n_saturated", "old_size", "new_size")
DEFAULTS = dict(cell_size=0.05, search_radius=0.1, k=16, min_neighbors=6, max_surface_variation=float(F(1.0 / 3.0)), radius_rank=8,
                radius_scale_squared=2.0, confidence=1.0, default_color=0, frame_index=1, orient=ORIENT_NONE, view_point=(0.0, 0.0, 0.0))
MUTANTS = ("ball_lt", "tie_high_index", "sparse_le", "rough_ge", "radius_last", "orient_le", "tie_high_column", "skip_none",
           "sums_float32", "bad_origin_ignored")
PAIRS = ((0, 1), (0, 2), (1, 2))


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def u32(rows):
    return rows.view(np.uint32)


def blank_rows(n):
    rows = np.zeros((ROWS, n), F)
    u32(rows)[19:23] = INVALID
    return rows


def comparable(rows):
    """The rows a download can be compared on: 14-16 and 23 have no storage and read as zero."""
    r = np.array(rows, F, copy=True)
    r[14:17] = 0
    r[23] = 0
    return r.view(np.uint32)


def bad_mask(points, origins, orient, mutant=None):
    bad = ~np.isfinite(points).all(1)
    if orient == ORIENT_ORIGINS and mutant != "bad_origin_ignored":
        bad |= ~np.isfinite(origins).all(1)
    return bad


def neighbour_lists(points, bad, search_radius, k, mutant=None):
    """(idx [n,k] uint32, d2 [n,k] float32, m [n]): smx_nn_query_self's answer over the points that are not BAD."""
    P = np.asarray(points, F).reshape(-1, 3)
    n = P.shape[0]
    r2 = F(F(search_radius) * F(search_radius))
    with np.errstate(all="ignore"):
        indexed = ~bad & (np.abs(P) <= F(3.0e38)).all(1)
    cand = np.nonzero(indexed)[0]
    idx, d2o, m = np.zeros((n, k), np.uint32), np.zeros((n, k), F), np.zeros(n, np.int64)
    Q = P[cand]
    for i in cand:
        with np.errstate(all="ignore"):
            dx, dy, dz = Q[:, 0] - P[i, 0], Q[:, 1] - P[i, 1], Q[:, 2] - P[i, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = (d2 < r2) if mutant == "ball_lt" else (d2 <= r2)
        j = cand[ok]
        tie = -j.astype(np.int64) if mutant == "tie_high_index" else j.astype(np.int64)
        order = np.lexsort((tie, d2[ok].view(np.uint32)))[:k]
        m[i] = order.size
        idx[i, :order.size] = j[order]
        d2o[i, :order.size] = d2[ok][order]
    return idx, d2o, m


def covariance(P, idx, m, active, mutant=None):
    """The six entries of C for the active points: {(a, b): float64 [n]}."""
    n, k = idx.shape
    s = [np.zeros(n, D) for _ in range(3)]
    q = {(a, b): np.zeros(n, D) for a in range(3) for b in range(a, 3)}
    order = range(k)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for e in order:
            on = active & (e < m)
            j = np.where(on, idx[:, e], rows)
            d32 = [(P[j, a] - P[:, a]).astype(F) for a in range(3)]
            if mutant == "sums_float32":
                d = [v for v in d32]
                for a in range(3):
                    s[a] = np.where(on, (s[a].astype(F) + d[a]).astype(D), s[a])
                    for b in range(a, 3):
                        q[a, b] = np.where(on, (q[a, b].astype(F) + d[a] * d[b]).astype(D), q[a, b])
                continue
            d = [v.astype(D) for v in d32]
            for a in range(3):
                s[a] = np.where(on, s[a] + d[a], s[a])
                for b in range(a, 3):
                    q[a, b] = np.where(on, q[a, b] + d[a] * d[b], q[a, b])
        inv = 1.0 / np.maximum(m, 1).astype(D)
        mean = [s[a] * inv for a in range(3)]
        return {(a, b): q[a, b] * inv - mean[a] * mean[b] for a in range(3) for b in range(a, 3)}


def jacobi(C, sweeps=SWEEPS, mutant=None):
    """(lam [n,3]: lam0, lam1, lam2 of the definition; normal [n,3] float64; the diagonal [n,3]; the off-diagonals [n,3]; V)."""
    a = {key: np.array(v, D, copy=True) for key, v in C.items()}
    n = a[0, 0].shape[0]
    V = np.zeros((n, 3, 3), D)
    for i in range(3):
        V[:, i, i] = 1.0
    sym = lambda i, j: (i, j) if i <= j else (j, i)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                r = 3 - p - q
                apq, app, aqq = a[p, q], a[p, p], a[q, q]
                on = np.ones(n, bool) if mutant == "skip_none" else (apq != 0.0)
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                arp, arq = a[sym(r, p)], a[sym(r, q)]
                a[p, p] = np.where(on, app - t * apq, app)
                a[q, q] = np.where(on, aqq + t * apq, aqq)
                a[p, q] = np.where(on, 0.0, apq)
                a[sym(r, p)] = np.where(on, c * arp - sn * arq, arp)
                a[sym(r, q)] = np.where(on, sn * arp + c * arq, arq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(on[:, None], c[:, None] * vp - sn[:, None] * vq, vp)
                V[:, :, q] = np.where(on[:, None], sn[:, None] * vp + c[:, None] * vq, vq)
        diag = np.stack([a[0, 0], a[1, 1], a[2, 2]], axis=1)
        col = np.zeros(n, np.int64)
        low = diag[:, 0].copy()
        for cc in (1, 2):
            less = (diag[:, cc] <= low) if mutant == "tie_high_column" else (diag[:, cc] < low)
            col = np.where(less, cc, col)
            low = np.where(less, diag[:, cc], low)
    lam1 = np.where(col == 0, diag[:, 1], diag[:, 0])
    lam2 = np.where(col == 2, diag[:, 1], diag[:, 2])
    normal = V[np.arange(n), :, col]
    off = np.stack([a[0, 1], a[0, 2], a[1, 2]], axis=1)
    return np.stack([low, lam1, lam2], axis=1), normal, diag, off, V


def fit(points, origins, idx, d2, m, bad, p, mutant=None):
    """(cls [n], normals [n,3] float32, RadiusSquared [n] float32) of k_import_fit."""
    P = np.asarray(points, F).reshape(-1, 3)
    n, k = P.shape[0], int(p["k"])
    cls = np.full(n, OK, np.uint8)
    cls[bad] = BAD
    sparse = (m <= p["min_neighbors"]) if mutant == "sparse_le" else (m < p["min_neighbors"])
    cls[~bad & sparse] = SPARSE
    entry = np.maximum(m - 1, 0) if mutant == "radius_last" else np.minimum(int(p["radius_rank"]), np.maximum(m - 1, 0))
    with np.errstate(all="ignore"):
        r2 = (F(p["radius_scale_squared"]) * d2[np.arange(n), entry]).astype(F)
        cls[(cls == OK) & ~(r2 > 0)] = DEGENERATE
        active = cls == OK
        lam, nd, _, _, _ = jacobi(covariance(P, idx, m, active, mutant), SWEEPS, mutant)
        nf = nd.astype(F)
        len2 = (nf[:, 0] * nf[:, 0] + nf[:, 1] * nf[:, 1]) + nf[:, 2] * nf[:, 2]
        nf = (nf / np.sqrt(len2)[:, None]).astype(F)
        cls[active & (~(len2 > 0) | ~np.isfinite(nf).all(1))] = DEGENERATE
        thr = D(F(p["max_surface_variation"])) * ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        rough = (lam[:, 0] >= thr) if mutant == "rough_ge" else (lam[:, 0] > thr)
        cls[(cls == OK) & active & rough] = ROUGH
        if p["orient"] != ORIENT_NONE:
            o = np.asarray(origins, F).reshape(-1, 3) if p["orient"] == ORIENT_ORIGINS else np.tile(np.asarray(p["view_point"], F), (n, 1))
            v = (o - P).astype(F)
            dot = (nf[:, 0] * v[:, 0] + nf[:, 1] * v[:, 1]) + nf[:, 2] * v[:, 2]
            flip = (dot <= 0) if mutant == "orient_le" else (dot < 0)
            nf = np.where(flip[:, None], -nf, nf)
    r2 = np.where((cls == BAD) | (cls == SPARSE), F(0), r2).astype(F)
    return cls, nf, r2, lam


def import_model(points, colors=None, origins=None, p=None, old_rows=None, max_surfels=None, mutant=None, lists=None):
    """Returns (rows afterwards [25, new_size], point_to_slot [n] uint32 or None, stats dict, extra).  extra: failed (the over-full
    refusal: rows are the old ones, unchanged), cls [n], lists (idx, d2, m: what the host walk of the shared header is handed),
    normals, radius_squared, lam, dirty (the slots the delta hand-off delivers).  lists: use these instead of computing them."""
    p = p or params()
    P = np.ascontiguousarray(np.asarray(points, F).reshape(-1, 3))
    n = P.shape[0]
    old = blank_rows(0) if old_rows is None else np.array(old_rows, F, copy=True).reshape(ROWS, -1)
    n_old = old.shape[1]
    O = None if origins is None else np.asarray(origins, F).reshape(-1, 3)
    bad = bad_mask(P, O, p["orient"], mutant)
    idx, d2, m = neighbour_lists(P, bad, p["search_radius"], int(p["k"]), mutant) if lists is None else lists
    cls, nf, r2, lam = fit(P, O, idx, d2, m, bad, p, mutant)
    st = dict.fromkeys(STAT_NAMES, 0)
    st.update(n_points=n, n_bad=int((cls == BAD).sum()), n_sparse=int((cls == SPARSE).sum()), n_degenerate=int((cls == DEGENERATE).sum()),
              n_rough=int((cls == ROUGH).sum()), n_imported=int((cls == OK).sum()), n_saturated=int((~bad & (m == int(p["k"]))).sum()),
              old_size=n_old, new_size=n_old)
    extra = dict(failed=False, cls=cls, lists=(idx, d2, m), normals=nf, radius_squared=r2, lam=lam, dirty=np.zeros(0, np.uint32))
    app = np.nonzero(cls == OK)[0]
    if max_surfels is not None and n_old + app.size > max_surfels:
        extra["failed"] = True
        return old, None, st, extra
    p2s = np.full(n, INVALID, np.uint32)
    p2s[app] = n_old + np.arange(app.size, dtype=np.uint32)
    out = np.concatenate([old, blank_rows(app.size)], axis=1)
    ou = u32(out)
    new = p2s[app]
    out[0:3, new] = P[app].T
    out[3:6, new] = P[app].T
    out[6, new] = F(p["confidence"])
    out[7, new] = r2[app]
    out[8:11, new] = nf[app].T
    ou[17, new] = ou[18, new] = np.uint32(p["frame_index"])
    ou[24, new] = np.uint32(p["default_color"]) if colors is None else np.asarray(colors, np.uint32)[app]
    st["new_size"] = n_old + int(app.size)
    extra["dirty"] = new.copy()
    return out, p2s, st, extra
