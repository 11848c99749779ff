"""The model of smx_recon_merge_map (include/smx.h): brute-force numpy in float32 (test infrastructure, no GPU
needed).  Every float32 expression is evaluated as the definition writes it, one rounding per operation.  The candidates of
a source slot are every live, indexable dst slot with d2 <= r2, ordered by (d2 bits, index), the first k of them; the first
compatible candidate wins; append and blend follow the definition literally.

merge_model(..., mutant=...) evaluates a deliberately wrong definition instead (tests/test_merge_model.py: each mutant must
fail a named case)."""
import math

import numpy as np

F = np.float32
INVALID = np.uint32(0xFFFFFFFF)
ROWS = 25
KEEP_DST, BLEND = 0, 1
DEAD, BAD, MATCHED, APPEND = 0, 1, 2, 3
STAT_NAMES = ("n_src_slots", "n_src_live", "n_bad", "n_matched", "n_appended", "n_blended_dst", "n_saturated", "links_dropped",
              "old_size", "new_size")
DEFAULTS = dict(cell_size=0.05, radius_factor_squared=1.0, max_normal_angle_deg=30.0, k=8, mode=KEEP_DST,
                confidence_cap=float(np.finfo(np.float32).max), frame_index=1)
MUTANTS = ("tie_high_index", "blend_reversed", "normal_gt", "ball_lt")


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def u32(rows):
    """The rows as 32-bit words (a view)."""
    return rows.view(np.uint32)


def blank_rows(n):
    rows = np.zeros((ROWS, n), F)
    u32(rows)[19:23] = INVALID
    return rows


def cos_max_of(angle_deg):
    """(float)cos((double)angle * (pi / 180)), as smx_recon_track forms it."""
    return F(math.cos(float(F(angle_deg)) * (math.pi / 180.0)))


def move(T, x, y, z, with_t=True):
    """((R0 x + R1 y) + R2 z) + t per row, float32."""
    T = np.asarray(T, F).reshape(12)
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            v = (T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z
            out.append(v + T[4 * r + 3] if with_t else v)
    return out


def moved_source(src_rows, T, factor_sq):
    """(P' [3,n], S' [3,n], n' [3,n], cls [n], r2 [n]) of k_merge_move."""
    s = np.asarray(src_rows, F)
    P = np.stack(move(T, s[0], s[1], s[2]))
    S = np.stack(move(T, s[3], s[4], s[5]))
    N = np.stack(move(T, s[8], s[9], s[10], with_t=False))
    with np.errstate(all="ignore"):
        live = ~(s[7] < 0)
        fin = np.isfinite(P).all(0) & np.isfinite(S).all(0) & np.isfinite(N).all(0)
        r2 = np.where(live & fin, F(factor_sq) * s[7], F(-1.0)).astype(F)
    cls = np.where(~live, DEAD, np.where(fin, APPEND, BAD)).astype(np.uint8)
    return P, S, N, cls, r2


def candidates(dst_rows, q, r2, k, mutant=None):
    """The answer of smx_nn_query_batch for one query: indices ascending by (d2, index), at most k."""
    d = np.asarray(dst_rows, F)
    if d.shape[1] == 0 or not r2 >= 0:
        return np.zeros(0, np.uint32)
    with np.errstate(all="ignore"):
        dx, dy, dz = d[3] - q[0], d[4] - q[1], d[5] - q[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = ~(d[7] < 0) & (np.abs(d[3]) <= F(3.0e38)) & (np.abs(d[4]) <= F(3.0e38)) & (np.abs(d[5]) <= F(3.0e38))
        ok &= (d2 < r2) if mutant == "ball_lt" else (d2 <= r2)
    idx = np.nonzero(ok)[0]
    tie = -idx.astype(np.int64) if mutant == "tie_high_index" else idx.astype(np.int64)
    order = np.lexsort((tie, d2[idx].view(np.uint32)))
    return idx[order][:k].astype(np.uint32)


def blend_step(b, P, S, n, w, radius_sq, cap):
    """One source into the running blend b = [P(3), S(3), N(3), c, r] (float32 scalars), in place."""
    with np.errstate(all="ignore"):
        W = F(b[9] + w)
        if not W > 0:
            return
        a, bb = F(b[9] / W), F(w / W)
        for j in range(3):
            b[j] = F(F(a * b[j]) + F(bb * P[j]))
            b[3 + j] = F(F(a * b[3 + j]) + F(bb * S[j]))
        M = [F(F(a * b[6 + j]) + F(bb * n[j])) for j in range(3)]
        len2 = F(F(F(M[0] * M[0]) + F(M[1] * M[1])) + F(M[2] * M[2]))
        if len2 > 0:
            ln = F(np.sqrt(len2))
            for j in range(3):
                b[6 + j] = F(M[j] / ln)
        b[10] = F(np.fmin(b[10], radius_sq))
        b[9] = F(np.fmin(W, F(cap)))


def merge_model(dst_rows, src_rows, T, p, max_surfels=None, mutant=None, lists=None):
    """Returns (rows of dst afterwards [25, new_size], src_to_dst [n_src] uint32, stats dict, extra).  extra: failed (the
    over-full refusal: rows are dst's, unchanged), cls [n_src], dirty (the slots the delta hand-off delivers), lists (the
    candidate list of every source slot, which the host walk of the shared header is handed).  lists: use these candidate
    lists instead of computing them."""
    dst = np.array(dst_rows, F, copy=True).reshape(ROWS, -1)
    src = np.asarray(src_rows, F).reshape(ROWS, -1)
    n, old = src.shape[1], dst.shape[1]
    k, cos_max = int(p["k"]), cos_max_of(p["max_normal_angle_deg"])
    frame = np.uint32(p["frame_index"])
    P, S, N, cls, r2 = moved_source(src, T, p["radius_factor_squared"])
    st = dict.fromkeys(STAT_NAMES, 0)
    st.update(n_src_slots=n, old_size=old, new_size=old, n_src_live=int((cls != DEAD).sum()), n_bad=int((cls == BAD).sum()))
    match = np.full(n, INVALID, np.uint32)
    out_lists = []
    for i in range(n):
        if cls[i] != APPEND:
            out_lists.append(np.zeros(0, np.uint32))
            continue
        cand = candidates(dst, S[:, i], r2[i], k, mutant) if lists is None else np.asarray(lists[i], np.uint32)
        out_lists.append(cand)
        hit = None
        for d in cand:
            with np.errstate(all="ignore"):
                dot = F(F(F(N[0, i] * dst[8, d]) + F(N[1, i] * dst[9, d])) + F(N[2, i] * dst[10, d]))
            if (dot > cos_max) if mutant == "normal_gt" else (dot >= cos_max):
                hit = d
                break
        if hit is None:
            st["n_saturated"] += int(len(cand) == k)
        else:
            cls[i], match[i] = MATCHED, hit
    app = np.nonzero(cls == APPEND)[0]
    st["n_matched"], st["n_appended"] = int((cls == MATCHED).sum()), int(app.size)
    extra = dict(failed=False, cls=cls, lists=out_lists, dirty=np.zeros(0, np.uint32))
    if max_surfels is not None and old + app.size > max_surfels:
        extra["failed"] = True
        return dst, None, st, extra
    s2d = match.copy()
    s2d[app] = old + np.arange(app.size, dtype=np.uint32)
    out = np.concatenate([dst, blank_rows(app.size)], axis=1)
    ou, su = u32(out), u32(src)
    new = s2d[app]
    out[0:3, new], out[3:6, new], out[8:11, new] = P[:, app], S[:, app], N[:, app]
    out[6:8, new] = src[6:8, app]
    ou[17, new] = ou[18, new] = frame
    ou[24, new] = su[24, app]
    for r in range(19, 23):
        l = su[r, app]
        valid = l != INVALID
        inside = valid & (l < n)
        to_app = np.zeros(app.size, bool)
        to_app[inside] = cls[l[inside]] == APPEND
        ou[r, new] = np.where(to_app, s2d[np.where(to_app, l, 0)], INVALID)
        st["links_dropped"] += int((valid & ~to_app).sum())
    dirty = list(new)
    if p["mode"] == BLEND:
        targets = np.unique(match[cls == MATCHED])
        for d in targets:
            srcs = np.nonzero((cls == MATCHED) & (match == d))[0]
            if mutant == "blend_reversed":
                srcs = srcs[::-1]
            b = [F(v) for v in (*dst[0:3, d], *dst[3:6, d], *dst[8:11, d], dst[6, d], dst[7, d])]
            for i in srcs:
                blend_step(b, P[:, i], S[:, i], N[:, i], src[6, i], src[7, i], p["confidence_cap"])
            out[0:3, d], out[3:6, d], out[8:11, d], out[6, d], out[7, d] = b[0:3], b[3:6], b[6:9], b[9], b[10]
            ou[18, d] = frame
        st["n_blended_dst"] = int(targets.size)
        dirty += list(targets)
    st["new_size"] = old + int(app.size)
    extra["dirty"] = np.array(sorted(dirty), np.uint32)
    return out, s2d, st, extra


def comparable(rows):
    """The rows a download can be compared on: 14-16 and 23 have no storage and read as zero."""
    r = np.array(rows, F, copy=True)
    r[14:17] = 0
    r[23] = 0
    return r.view(np.uint32)


def remap_triangles(triangles, src_to_dst):
    """A triangle array over src through src_to_dst: a triangle that loses a corner is dropped."""
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    m = np.asarray(src_to_dst, np.uint32)[t]
    return m[(m != INVALID).all(1)]
