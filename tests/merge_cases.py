"""Hand-built pairs of maps for smx_recon_merge_map: the smallest maps that reach every decision of the definition (include/smx.h).
A plain module (no fixtures).  cases() returns the list; every case is a Case with the rows of dst and src [25, n], the pose,
the parameters, dst's capacity and the decisions it is there for.  census() prints decision -> case.

Coordinates are multiples of 2^-10 wherever a distance has to be exact: differences, squares and their sums then carry no
rounding, and "d2 == r2" means what it says on every machine."""
import math

import numpy as np

import merge_ref as mr

F = np.float32
INVALID = 0xFFFFFFFF
STEP = F(1.0 / 64.0)              # lattice pitch of the planes
R2 = F(1.0 / 16384.0)             # (1/128)^2: a ball of half the pitch holds the lattice point under it and no other
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


class Case:
    def __init__(self, name, dst, src, decisions, T=IDENTITY, max_surfels=4096, **p):
        self.name, self.dst, self.src, self.T = name, dst, src, np.asarray(T, F).reshape(12)
        self.max_surfels, self.decisions = int(max_surfels), tuple(decisions)
        self.p = mr.params(**p)

    def params(self, mode):
        return dict(self.p, mode=mode)


def plane(n, x0=0.0, y0=0.0, z0=0.0, normal=(0.0, 0.0, 1.0), r2=R2, conf=1.0, stamp=1, color0=0x00102030, width=32):
    """n slots on the lattice (x0 + STEP (j % width), y0 + STEP (j // width), z0); smooth = raw position."""
    rows = mr.blank_rows(n)
    j = np.arange(n)
    rows[0] = rows[3] = F(x0) + STEP * (j % width).astype(F)
    rows[1] = rows[4] = F(y0) + STEP * (j // width).astype(F)
    rows[2] = rows[5] = F(z0)
    rows[6], rows[7] = F(conf), F(r2)
    rows[8], rows[9], rows[10] = (F(v) for v in normal)
    u = mr.u32(rows)
    u[17] = u[18] = stamp
    u[24] = (color0 + j).astype(np.uint32)
    return rows


def chain_links(rows):
    """Every slot links to its lattice neighbours j - 1 and j + 1 (rows 19, 20)."""
    n = rows.shape[1]
    u = mr.u32(rows)
    j = np.arange(n, dtype=np.uint32)
    u[19] = np.where(j > 0, j - 1, INVALID)
    u[20] = np.where(j + 1 < n, j + 1, INVALID)
    return rows


def concat(*maps):
    return np.concatenate(maps, axis=1)


def rot_pose(axis, angle_deg, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + s * K + (1 - c) * (K @ K)
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F).reshape(12)


def in_own_frame(rows, T):
    """The rows of a map given in dst's frame, stored in the frame that T moves into dst's (inverse in double, rounded once)."""
    M = np.asarray(T, np.float64).reshape(3, 4)
    R, t = M[:, :3], M[:, 3]
    out = rows.copy()
    out[0:3] = (R.T @ (rows[0:3].astype(np.float64) - t[:, None])).astype(F)
    out[3:6] = (R.T @ (rows[3:6].astype(np.float64) - t[:, None])).astype(F)
    out[8:11] = (R.T @ rows[8:11].astype(np.float64)).astype(F)
    return out


def _segment_edge(size):
    # dst: `size` lattice slots; src: 6 slots under dst's last 6 (matched) and 10 beyond the lattice (appended across 1024)
    dst = chain_links(plane(size))
    src = chain_links(concat(dst[:, size - 6:].copy(), plane(10, y0=2.0, conf=2.0, stamp=7, color0=0x00AA0000)))
    return Case("dst_%d_append_across_segment" % size, dst, src, ["dst size %d" % size, "append crosses the 1024-slot edge" if size <= 1024 else
                                                                "append starts behind the 1024-slot edge", "matched", "appended"], frame_index=9)


def cases():
    out = [_segment_edge(1023), _segment_edge(1024), _segment_edge(1025)]

    out.append(Case("empty_src", chain_links(plane(40)), mr.blank_rows(0), ["empty src"]))
    out.append(Case("empty_dst", mr.blank_rows(0), chain_links(plane(40, conf=3.0)), ["empty dst", "link to appended"], frame_index=4))

    # src of more than two segments: matched, appended and merged slots interleaved, links along the chain
    src = chain_links(plane(2100, conf=2.0))
    j = np.arange(2100)
    src[2, j % 3 == 1] = src[5, j % 3 == 1] = F(1.0)            # every third slot a metre above dst: appended
    src[7, j % 7 == 3] = F(-1.0)                                 # merged slots interleaved
    out.append(Case("src_three_segments_interleaved", chain_links(plane(1500)), src,
                    ["src merged slots interleaved", "src of several segments", "link to appended", "link to matched", "link to merged"],
                    frame_index=3))

    # live by the rule, BAD of each kind
    src = plane(8, y0=1.0)
    src[7, 1] = F(np.nan)                                        # NaN radius: live, no ball, appended
    src[0, 2] = F(np.nan)                                        # BAD: raw position
    src[4, 3] = F(np.inf)                                        # BAD: smooth position
    src[9, 4] = F(np.nan)                                        # BAD: normal
    src[7, 5] = F(-0.0)                                          # -0 is not < 0: live
    out.append(Case("nan_radius_and_bad_slots", plane(20), src,
                    ["NaN radius is live", "BAD position", "BAD smooth position", "BAD normal", "-0 radius is live"]))

    # equal d2: dst slots 3 and 5 at the same distance from the source; with k = 1 only the tie rule decides who is looked at
    dst = plane(8, y0=4.0)
    for d, x in ((3, 0.25), (5, -0.25)):
        dst[0:6, d] = (x, 0, 0, x, 0, 0)
    out.append(Case("equal_d2_lower_index_wins", dst, plane(1, r2=0.25), ["equal d2: lower index wins"], k=1))

    # exactly on the ball and one ulp outside
    dst = plane(1, x0=0.25)
    src = plane(2)
    src[0:6, :] = 0
    src[7, 0], src[7, 1] = F(0.0625), np.nextafter(F(0.0625), F(0))
    out.append(Case("on_the_ball_and_one_ulp_outside", dst, src, ["d2 == r2 matches", "d2 one ulp outside: appended"]))

    # the normal dot exactly at cos_max and one ulp below
    c = mr.cos_max_of(30.0)
    dst = plane(2)
    dst[8:11, 0] = (F(0.5), F(0), c)
    dst[8:11, 1] = (F(0.5), F(0), np.nextafter(c, F(0)))
    out.append(Case("normal_at_cos_max_and_one_ulp_below", dst, plane(2), ["dot == cos_max matches", "dot one ulp below: appended"]))

    # more than k in the ball, the first k incompatible, a compatible one behind them
    dst = plane(4, normal=(0.0, 0.0, -1.0))
    dst[0, :] = dst[3, :] = (np.arange(4) * F(1.0 / 1024.0)).astype(F)
    dst[1, :] = dst[4, :] = 0
    dst[8:11, 3] = (0, 0, 1)
    src = plane(1, r2=1.0 / 4096.0)
    out.append(Case("saturated_k3", dst, src, ["first k incompatible, compatible behind: unmatched, n_saturated"], k=3))
    out.append(Case("not_saturated_k4", dst, src, ["compatible candidate is the k-th: matched"], k=4))

    # k = 1 and k = 64 over a dense patch: 70 dst slots inside every source ball, the compatible ones late in the order
    dst = plane(70, width=10, normal=(0.0, 0.0, -1.0))
    dst[0] = dst[3] = (np.arange(70) % 10 * F(1.0 / 1024.0)).astype(F)
    dst[1] = dst[4] = (np.arange(70) // 10 * F(1.0 / 1024.0)).astype(F)
    dst[10, 65:] = 1
    src = plane(3, r2=1.0 / 1024.0)
    src[0] = src[3] = (F(0), F(9.0 / 1024.0), F(4.0 / 1024.0))
    src[1] = src[4] = (F(0), F(6.0 / 1024.0), F(3.0 / 1024.0))
    out.append(Case("k64_dense_patch", dst, src, ["k = 64"], k=64))
    out.append(Case("k1_dense_patch", dst, src, ["k = 1"], k=1))

    # blend: three and seven sources onto one dst slot, confidences that make the float order matter
    for count, confs in ((3, (0.1, 1000.0, 3.7)), (7, (0.3, 1.0e4, 0.7, 33.0, 1.0e-3, 5.5, 0.9))):
        dst = plane(3, conf=1.7)
        src = plane(count, r2=1.0 / 4096.0)
        src[0] = src[3] = STEP + (np.arange(count) - count // 2).astype(F) * F(3.0 / 8192.0) + F(1.0 / 3.0) * F(1.0 / 8192.0)
        src[1] = src[4] = (np.arange(count) % 2).astype(F) * F(5.0 / 8192.0)
        src[2] = F(1.0 / 4096.0)
        src[5] = F(1.0 / 2048.0)
        src[6] = np.array(confs, F)
        src[7] = R2 * (F(1.0) + (np.arange(count) % 3).astype(F) * F(0.25))
        ang = (np.arange(count) - 1).astype(np.float64) * 0.11
        src[8], src[9], src[10] = np.sin(ang).astype(F), (0.3 * np.sin(2 * ang)).astype(F), np.cos(ang).astype(F)
        out.append(Case("blend_%d_onto_one" % count, dst, src, ["%d sources onto one dst slot, order matters" % count],
                        max_normal_angle_deg=60.0, frame_index=12))

    # W <= 0, len2 == 0, the confidence cap
    dst = plane(3, conf=0.0)
    dst[6, 1] = F(-2.0)
    src = plane(3, conf=0.0)
    src[6, 1] = F(1.5)                                           # W = -0.5
    src[6, 2] = F(2.0)                                           # W = 2: blends with a = 0
    out.append(Case("blend_W_not_positive", dst, src, ["W == 0", "W < 0"], frame_index=5))
    out.append(Case("blend_opposed_normals_len2_zero", plane(2), plane(2, normal=(0.0, 0.0, -1.0)), ["len2 == 0: N stays", "angle limit 180"],
                    max_normal_angle_deg=180.0))
    out.append(Case("blend_confidence_cap", plane(2, conf=2.0), plane(2, conf=1.0), ["confidence cap reached"], confidence_cap=2.5))

    # links of each kind: slots 0 appended, 1 matched, 2 merged, 3 BAD; 4 and 5 appended and linked to all of them
    src = plane(6, y0=1.0)
    src[0:2, 1] = src[3:5, 1] = 0                                # slot 1 lies on dst's slot 0
    src[7, 2] = F(-1.0)
    src[0, 3] = F(np.nan)
    u = mr.u32(src)
    u[19:23, 4] = (0, 1, 2, 3)
    u[19:23, 5] = (INVALID, 4, 0xFFFFFFF0, 0)
    u[19:23, 1] = (0, 4, 5, 2)                                   # a matched slot's links leave no trace
    out.append(Case("links_of_each_kind", plane(4), src,
                    ["link to appended", "link to matched", "link to merged", "link to BAD", "link invalid", "link out of range"]))

    # capacity exactly full and one short
    out.append(Case("capacity_exactly_full", plane(30), plane(12, y0=1.0), ["capacity exactly full"], max_surfels=42))
    out.append(Case("capacity_one_short", plane(30), plane(12, y0=1.0), ["capacity one short: refused"], max_surfels=41))

    # a pose with rotation and translation: the overlap of two halves of one plane, the second stored in its own frame
    T = rot_pose((1.0, 2.0, 3.0), 37.0, (0.5, -0.25, 2.0))
    whole = chain_links(plane(600))
    a, b = whole[:, :400].copy(), whole[:, 200:].copy()
    ub = mr.u32(b)
    for r in (19, 20):
        ub[r] = np.where(ub[r] == INVALID, INVALID, ub[r] - np.uint32(200))
    ub[19, 0] = INVALID
    out.append(Case("pose_rotation_translation", a, in_own_frame(b, T), ["pose with rotation and translation", "matched", "appended"], T=T,
                    radius_factor_squared=1.0))
    out.append(Case("pose_identity_half_overlap", a, b, ["identity pose"]))
    return out


def census(case_list=None):
    """decision -> the cases it is reached in, printed and returned."""
    table = {}
    for c in case_list if case_list is not None else cases():
        for d in c.decisions:
            table.setdefault(d, []).append(c.name)
    for d in sorted(table):
        print("%-70s %s" % (d, ", ".join(table[d])))
    return table
