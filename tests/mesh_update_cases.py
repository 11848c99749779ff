"""Chains of hand-built surfel maps for smx_recon_triangulate_update (test infrastructure, no GPU needed): each chain is a
list of steps, each step a whole map to upload and the cell size and full_above_fraction to call the update with.  They
reach what the sphere and the U0 .. U5 chain of tests/mesh_cases.py do not: the coarse filter in front of the reverse test
with a changed point or a ghost in every one of the 26 neighbour cells, at negative cell indices and across 0, on both
sides of its radius condition and where a coordinate has no cell; the D condition at equality; hundreds of ghosts across
three workgroups, revival in place, one-word changes, a NaN; kept runs copied at shifted offsets, a new workgroup with
no kept block offset, kept buffers that survive a re-allocation; the path choice at equality.

The maps are built with the builders of tests/mesh_cases.py (unit-sized rings, isolated patches) and keep its margin rule
(tests/test_mesh_update_cases.py sweeps every step), so the float64 model and the float32 kernels cannot differ.
`designed` of a step holds the counts its construction gives; the census test asserts them against the model."""
import math
import os
import re

import numpy as np

import mesh_cases as mc
import mesh_ref as mr
import mesh_update_ref as mu
from common import ROOT

Z = (0.0, 0.0, 1.0)
H = 2.5                              # the filter's cell in most chains: 0.25f * H * H = 1.5625 exactly; balls of radius <= 1.25
H_UNFILTERED = {"F": 0.5, "Ff": 0.5, "D": 0.05}    # a second run of these chains: no ball is small enough for the filter


class Step:
    def __init__(self, name, m, prm, cell, fraction, designed, why, exempt=()):
        self.name, self.map, self.prm, self.cell, self.fraction = name, m, prm, cell, fraction
        self.designed, self.why, self.exempt = designed, why, tuple(exempt)

    @property
    def n(self):
        return self.map[0].shape[0]


class Chain:
    def __init__(self, name, prm, cell, what):
        self.name, self.prm, self.cell, self.what = name, prm, cell, what
        self.steps, self.roles = [], {}

    def add(self, lay, name, why, fraction=None, exempt=(), **designed):
        self.steps.append(Step("%s%d" % (self.name, len(self.steps)) if name is None else name, lay.map(), self.prm, self.cell,
                               fraction, designed, why, exempt))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def park(lay, slot, along, by=8.0):
    """The slot `by` units along a direction: out of every ball of its patch, at least two cells of H away."""
    lay.pos[slot] = lay.pos[slot] + by * _unit(along)


def lonely_at(lay, xyz, r2=0.25, normal=Z):
    return lay.put((np.asarray(xyz, np.float64), normal, r2))


# ---- F: the filter ------------------------------------------------------------------------------------------------------
OFFSETS26 = [tuple(int(v) for v in o) for o in mu.OFFSETS27 if tuple(o) != (0, 0, 0)]
WEDGE_T = 0.45                        # the changed point's distance from q, towards the neighbour cell
WEDGE_EDGE = 0.42                     # q sits 0.08 H = 0.2 from the face(s) it looks across, in the middle of its cell elsewhere


def wedge_normal(o):
    """A unit vector at right angles to the offset o."""
    zero = [a for a in range(3) if o[a] == 0]
    if zero:
        n = np.zeros(3)
        n[zero[0]] = 1.0
        return n
    return _unit((o[1], -o[0], 0.0))


def wedge(lay, cell, o, h, q_r2=1.44):
    """q near the side(s) of its cell that the offset o names, a and b at unit distance 35 degrees to either side of o in a
    plane through o, and c, which will stand between them at WEDGE_T in the cell `cell + o`; c is put parked.  The star of
    q is {a, b} without c and {a, c}, {c, b} with it.  Returns the slots and c's two positions."""
    o3 = np.asarray(o, np.float64)
    oh, n = _unit(o3), wedge_normal(o)
    w = np.cross(n, oh)
    q_pos = h * (np.asarray(cell, np.float64) + 0.5 + WEDGE_EDGE * o3)
    ca, sa = math.cos(math.radians(35.0)), math.sin(math.radians(35.0))
    q = lay.put((q_pos, n, q_r2))
    a = lay.put((q_pos + ca * oh + sa * w, n, 1.44))
    b = lay.put((q_pos + ca * oh - sa * w, n, 1.44))
    c_in = q_pos + WEDGE_T * oh
    c = lay.put((c_in, n, 1.44))
    park(lay, c, n)
    return dict(q=q, a=a, b=b, c=c, c_in=c_in, c_out=lay.pos[c].copy(), o=tuple(o), cell=tuple(int(v) for v in cell))


def _grid(j):
    return 8 * (j % 6), 8 * (j // 6)


def chain_f():
    ch = Chain("F", mr.Params(), H, "the coarse filter: 26 offsets at positive, negative and straddling cells; ghost-only "
               "balls; the radius condition at equality, one float above, and at 1.5 H")
    lay = mc.Layout()
    groups = {"pos": [], "neg": [], "zero": []}
    for j, o in enumerate(OFFSETS26):
        gx, gy = _grid(j)
        groups["pos"].append(wedge(lay, (2 + gx, 2 + gy, 2), o, H))
        groups["neg"].append(wedge(lay, (-3 - gx, -3 - gy, -3), o, H))
        a0 = next(a for a in range(3) if o[a] != 0)          # across 0 on this axis: q in cell 0 looks at -1, q in cell -1 at 0
        cell = [6 + gx, 6 + gy]
        cell.insert(a0, 0 if o[a0] < 0 else -1)
        groups["zero"].append(wedge(lay, cell, o, H))
    face = (1, 0, 0)
    # (a layer of its own, 20 cells below: no wedge above and nothing parked comes near)
    r_eq = wedge(lay, (2, 2, -20), face, H, q_r2=1.5625)                                       # f2 r2 == H^2 / 4: filtered
    r_above = wedge(lay, (10, 2, -20), face, H, q_r2=float(np.nextafter(np.float32(1.5625), np.float32(2.0))))   # bypasses
    # a ball of 1.5 H and a changed point two cells away
    q_big = lay.put((H * np.array([18.0 + 1.0, 2.5, -19.5]) - (0.2, 0.0, 0.0), Z, (1.5 * H) ** 2))
    c_big_in = lay.pos[q_big] + (2.9, 0.0, 0.0)
    c_big = lay.put((c_big_in, Z, 0.25))
    park(lay, c_big, Z)
    for k in range(6):
        lonely_at(lay, (H * (26.5 + 4 * k), H * 2.5, H * -19.5))
    ch.roles = dict(groups=groups, r_eq=r_eq, r_above=r_above, q_big=q_big, c_big=c_big)
    ch.add(lay, None, "the first call", 1.0, mode=1)

    def move(ws, where):
        for w in ws:
            lay.pos[w["c"]] = w[where].copy()
    move(groups["pos"], "c_in")
    ch.add(lay, None, "a changed live point in each of the 26 neighbour cells of an unchanged q, cells positive", 1.0,
           mode=0, n_changed=26, n_ghosts=26, n_dirty=104, offsets=26, q_via_one_cell=26)
    move(groups["neg"], "c_in")
    ch.add(lay, None, "the same with every cell index of q negative", 1.0,
           mode=0, n_changed=26, n_ghosts=26, n_dirty=104, offsets=26, q_via_one_cell=26, negative_cells=True)
    move(groups["zero"] + [r_eq, r_above], "c_in")
    lay.pos[c_big] = c_big_in
    ch.add(lay, None, "the same across 0; f2 r2 at H^2 / 4 (filtered) and one float above (let through); a ball of 1.5 H "
           "with the changed point two cells away", 1.0,
           mode=0, n_changed=29, n_ghosts=29, n_dirty=114, offsets=26, q_via_one_cell=26, across_zero=True,
           subject=[r_eq["q"]], by_radius=[r_above["q"], q_big])
    move(groups["pos"], "c_out")
    ch.add(lay, None, "the only point in q's ball is a ghost: the slot was live there and has moved far away", 1.0,
           mode=0, n_changed=26, n_ghosts=26, n_dirty=104, offsets=26, q_via_one_cell=26, ghost_only=True)
    for w in groups["neg"]:
        lay.r2[w["c"]] = -1.0
    ch.add(lay, None, "the only point in q's ball is a ghost: the slot was live there and is now merged", 1.0,
           mode=0, n_changed=26, n_ghosts=26, n_dirty=104, offsets=26, q_via_one_cell=26, ghost_only=True, negative_cells=True)
    return ch


def chain_ff():
    """search_radius_factor 2, the largest the call accepts: RadiusSquared alone (1) is below H^2 / 4 = 1.5625, f2 r2 = 4
    is what the radius condition compares.  (No map makes a condition on r2 alone unsound: r2 <= H^2 / 4 and f <= 2 give
    f r <= H, and a ball of radius H still lies within the 27 cells.  The step shows which side of the condition q is on.)"""
    ch = Chain("Ff", mr.Params(search_radius_factor=2.0), H, "f2 enters the radius condition: r2 = 1 < H^2 / 4 < f2 r2 = 4")
    lay = mc.Layout()
    q = lay.put((H * np.array([3.0, 0.5, 0.5]) - (0.2, 0.0, 0.0), Z, 1.0))              # 0.2 from the face; f r = 2
    c_in = lay.pos[q] + (1.9, 0.0, 0.0)                                                # 1.7 past the face, beyond r = 1
    c = lay.put((c_in, Z, 2.0 ** -8))
    park(lay, c, Z, 12.0)
    for k in range(3):
        lonely_at(lay, (H * (10.5 + 4 * k), H * 0.5, H * 0.5))
    ch.roles = dict(q=q, c=c)
    ch.add(lay, None, "the first call", 1.0, mode=1)
    lay.pos[c] = c_in
    ch.add(lay, None, "q is let through by f2 r2 > H^2 / 4 though r2 < H^2 / 4; the changed point is beyond r and within f r", 1.0,
           mode=0, n_changed=1, n_ghosts=1, n_dirty=2, by_radius=[q])
    return ch


# ---- N: coordinates without a cell ----------------------------------------------------------------------------------------
N_CELL = 2.0
FAR = 2.0 ** 21                      # FAR / N_CELL = 2^20: mesh_coarse_cell gives false; smx_nn indexes it (2^20 + 1 cells <= 2^21)


def chain_n():
    ch = Chain("N", mr.Params(), N_CELL, "a coordinate at 2^20 cells: an unchanged far slot keeps its row; a changed far slot turns the filter off")
    lay = mc.Layout()
    near = lonely_at(lay, (1.0, 1.0, 1.0), 0.81)
    far_q = lonely_at(lay, (FAR, 1.0, 1.0), 0.81)
    far_p = lonely_at(lay, (FAR - 0.5, 1.0, 1.0), 0.81)                  # cell 2^20 - 1: it has one
    other = lonely_at(lay, (9.0, 1.0, 1.0), 0.81)
    tri = lay.put_all(mc.place([(0.0, 0.0), (0.8, 0.0), (0.4, 0.7)], np.array([21.0, 1.0, 1.0]), Z, 0.81))
    ch.roles = dict(near=near, far_q=far_q, far_p=far_p, other=other, tri=tri)
    ch.add(lay, None, "the first call", 1.0, mode=1)
    lay.r2[far_p] = 0.64
    ch.add(lay, None, "the far slot is unchanged, its ball is small, it has no cell: it keeps its row and is found dirty", 1.0,
           mode=0, n_changed=1, n_ghosts=1, n_dirty=2, no_filter=False, by_cell=[far_q], filtered=[near, other] + tri)
    lay.r2[far_q] = 0.64
    ch.add(lay, None, "the far slot is changed: nobody is filtered", 1.0,
           mode=0, n_changed=1, n_ghosts=1, n_dirty=2, no_filter=True, filtered=[])
    return ch


# ---- D: the ball test at equality ---------------------------------------------------------------------------------------------
def chain_d():
    """As mesh_cases.edge_layout: q's normal is x, the points lie in the y-z plane, all coordinates are small dyadic
    numbers and dx dx + dy dy + dz dz runs from small to large, so d2 and f2 r2 are exact in float32 and float64."""
    ch = Chain("D", mr.Params(), H, "d2 == f2 r2_q exactly (in D) and one float above (not in D), for a current position and for a ghost")
    lay = mc.Layout()
    nx = (1.0, 0.0, 0.0)
    r2 = 1.0 + 2.0 ** -23
    roles = {}
    for name, c, at in (("on", np.array([0.0, 0.0, 0.0]), (2.0 ** -12, 2.0 ** -12, 1.0)),        # d2 = 1 + 2^-23
                        ("off", np.array([16.0, 0.0, 0.0]), (2.0 ** -11, 1.0, 0.0))):            # d2 = 1 + 2^-22
        q = lay.put((c, nx, r2))
        inside = lay.put((c + (0.0, -0.5, -0.5), nx, 2.0 ** -8))
        m = lay.put((c + (0.0, 0.0, 8.0), nx, 2.0 ** -8))
        roles[name] = dict(q=q, inside=inside, m=m, at=c + at, parked=c + (0.0, 0.0, 8.0))
    for k in range(3):
        lonely_at(lay, (32.0 + 8 * k, 0.0, 0.0))
    ch.roles = roles
    exempt = [(roles[k]["q"], roles[k]["m"]) for k in ("on", "off")]
    ch.add(lay, None, "the first call", 1.0, mode=1)
    for k in ("on", "off"):
        lay.pos[roles[k]["m"]] = roles[k]["at"]
    ch.add(lay, None, "a current position at d2 == f2 r2 is in the ball, one at the next float32 is not", 1.0, exempt,
           mode=0, n_changed=2, n_ghosts=2, n_dirty=3, in_d=[roles["on"]["q"]], not_in_d=[roles["off"]["q"]])
    for k in ("on", "off"):
        lay.pos[roles[k]["m"]] = roles[k]["parked"]
    ch.add(lay, None, "the same for the snapshot positions: the two slots have left", 1.0,
           mode=0, n_changed=2, n_ghosts=2, n_dirty=3, in_d=[roles["on"]["q"]], not_in_d=[roles["off"]["q"]])
    return ch


# ---- G: ghosts and revival --------------------------------------------------------------------------------------------------
G_PAIRS = 800                        # slots 0 .. 799: three workgroups and 32 slots of a fourth
G_MOVERS = {7: 6, 0: 1, 3: 2}        # slot % 8 of a mover -> that of its partner: slots 255, 256, 511, 512 move (255 % 8 = 7, 256 % 8 = 0)


def _g_home(i):
    return np.array([2.0 * (i % 16), 2.0 * (i // 16), 12.0])


def chain_g():
    ch = Chain("G", mr.Params(), H, "hundreds of ghosts across three workgroups; merged -> live in place; one-word changes; a NaN; appends only")
    lay = mc.Layout()
    movers = []
    for i in range(G_PAIRS):
        r = i % 8
        if r in G_MOVERS:
            partner = i + (G_MOVERS[r] - r)
            lay.put((_g_home(partner) + (0.3, 0.0, 0.0), Z, 0.25))        # inside its partner's ball, and only there
            movers.append((i, partner))
        else:
            lay.put((_g_home(i), Z, 0.25))
    hub, ring = mc.ring_patch(8, mc.centre(0), mc.NORMALS[0], 3)
    h = lay.put(hub)
    members = lay.put_all(ring)
    l_r = lonely_at(lay, (40.0, 0.0, 12.0))
    l_n = lonely_at(lay, (42.0, 0.0, 12.0))
    l_z = lonely_at(lay, (44.0, 0.0, 12.0))
    l_nan = lonely_at(lay, (46.0, 0.0, 12.0))
    ch.roles = dict(movers=movers, hub=h, members=members, l_r=l_r, l_n=l_n, l_z=l_z, l_nan=l_nan)
    ch.add(lay, None, "the first call", 1.0, mode=1)
    for i, _ in movers:
        lay.pos[i] = lay.pos[i] + (0.0, 0.0, 3.0)
    n_m = len(movers)
    in_three = sum(1 for i, _ in movers if i < 768)
    assert {255, 256, 511, 512} <= set(i for i, _ in movers) and in_three == 288
    ch.add(lay, None, "3 of every 8 slots of three workgroups move out of their partner's ball: the partners are dirty "
           "through the ghosts alone, and the ghosts' rows run across the workgroups", 1.0,
           mode=0, n_changed=n_m, n_ghosts=n_m, n_dirty=2 * n_m, ghosts_per_block=[96, 96, 96, 12])
    gone = members[2]
    lay.r2[gone] = -1.0
    lay.r2[l_r] = 0.36
    lay.nrm[l_n] = np.array([0.0, 0.0, 0.75])                             # (one word; the slot sees nobody, its normal decides nothing)
    assert lay.pos[l_z][1] == 0.0
    lay.pos[l_z] = lay.pos[l_z] * np.array([1.0, -1.0, 1.0])              # +0 -> -0
    lay.pos[l_nan] = lay.pos[l_nan] * np.array([1.0, np.nan, 1.0])
    ch.roles.update(gone=gone)
    ch.add(lay, None, "a ring member is merged; one slot changes RadiusSquared only, one a normal component only, one "
           "+0 into -0, one gets a NaN coordinate (not live now, a ghost from then)", None,
           mode=0, n_changed=5, n_ghosts=5, one_word=dict(radius=l_r, normal=l_n, minus_zero=l_z), nan_now=l_nan)
    lay.r2[gone] = 1.15 ** 2
    ch.add(lay, None, "the merged slot is live again in place, with another radius; the NaN slot is unchanged (NaN equals itself)", None,
           mode=0, n_changed=1, n_ghosts=0, revived=gone)
    a, b = lay.pos[members[0]] - lay.pos[h], lay.pos[members[1]] - lay.pos[h]
    mid = _unit(a + b) * 0.95 * 0.5 * (np.linalg.norm(a) + np.linalg.norm(b))   # (0.95: clear of the circles through its neighbours)
    n0 = lay.n
    lay.put((lay.pos[h] + mid, lay.nrm[h], lay.r2[members[0]]))            # inside old balls: the hub's ring goes 8 -> 9
    lay.put((_g_home(4) + (0.3, 0.0, 0.0), Z, 0.25))                       # inside the ball of an unchanged slot of the grid
    lonely_at(lay, (48.0, 0.0, 12.0))                                      # in empty space
    lonely_at(lay, (50.0, 0.0, 12.0))
    lonely_at(lay, (52.0, 0.0, 12.0), r2=-1.0)                             # merged on arrival
    ch.roles.update(appended=list(range(n0, lay.n)))
    ch.add(lay, None, "appends only: inside old balls, in empty space, merged on arrival", None,
           mode=0, n_changed=5, n_ghosts=0, appended=5)
    return ch


# ---- W: workgroups, kept runs, growth ---------------------------------------------------------------------------------------
def _patch(lay, m, k, normal, hub_first, seed=None):
    hub, ring = mc.ring_patch(m, mc.centre(k), normal, mc._SEED.get(m, 0) if seed is None else seed)
    if hub_first:
        h = lay.put(hub)
        members = lay.put_all(ring)
    else:
        members = lay.put_all(ring)
        h = lay.put(hub)
    return h, members


def chain_w():
    ch = Chain("W", mr.Params(), H, "a change in workgroup 0 shifts every kept run of workgroups 1 and 2, forth and back")
    lay = mc.Layout()
    hub, ring = _patch(lay, 17, 0, mc.NORMALS[0], True)                    # slots 0 .. 17: overflowed, owns nothing
    lay.fill_to(250)
    _patch(lay, 16, 1, mc.NORMALS[0], True)                                # owner at 250, its ring across the 255 / 256 boundary
    lay.fill_to(300)
    _patch(lay, 16, 2, mc.NORMALS[3], True)
    lay.fill_to(500)
    _patch(lay, 16, 3, mc.NORMALS[2], True)                                # owner at 500, its ring across 511 / 512
    lay.fill_to(600)
    _patch(lay, 16, 4, mc.NORMALS[0], False)                               # ring members own the triangles
    hub_l, ring_l = _patch(lay, 17, 5, mc.NORMALS[0], False)               # hub last: its ring members own what it gains
    lay.fill_to(781)
    assert lay.n >= 769 and hub == 0
    ch.roles = dict(hub=hub, ring=ring, hub_last=hub_l, ring_last=ring_l)
    ch.add(lay, None, "the first call", None, mode=1)
    member, home = ring[5], lay.pos[ring[5]].copy()
    mc._moved_away(lay, member)
    ch.add(lay, None, "a ring member in workgroup 0 leaves: slot 0 goes 17 -> 16 and gains 16 triangles", None,
           mode=0, n_changed=1, n_ghosts=1, owner_gains=(hub, 16), shifted_blocks=[1, 2, 3])
    lay.pos[member] = home
    ch.add(lay, None, "and comes back: slot 0 loses them", None,
           mode=0, n_changed=1, n_ghosts=1, owner_gains=(hub, -16), shifted_blocks=[1, 2, 3])
    member, home = ring_l[5], lay.pos[ring_l[5]].copy()
    mc._moved_away(lay, member)
    ch.add(lay, None, "a member of the hub-last ring leaves: ring members outside D own the 16 new triangles (new ring -> A)", None,
           mode=0, n_changed=1, n_ghosts=1, new_ring_owners=True)
    lay.pos[member] = home
    ch.add(lay, None, "and comes back: ring members outside D lose them (old ring -> A)", None,
           mode=0, n_changed=1, n_ghosts=1, old_ring_owners=True)
    return ch


def chain_wg():
    ch = Chain("Wg", mr.Params(), H, "growth by one slot into a new workgroup: 256 -> 257 and 512 -> 513, nothing else changed")
    lay = mc.Layout()
    _patch(lay, 16, 0, mc.NORMALS[0], True)
    lay.fill_to(239)
    _patch(lay, 16, 1, mc.NORMALS[3], True)                                # slots 239 .. 255: the end of workgroup 0
    assert lay.n == 256
    ch.add(lay, None, "the first call", None, mode=1)
    lay.lonely()
    ch.add(lay, None, "256 -> 257: workgroup 1 has no kept block offset", None, mode=0, n_changed=1, n_ghosts=0, n_dirty=1, new_block=1)
    _patch(lay, 16, 2, mc.NORMALS[2], True)
    lay.fill_to(495)
    _patch(lay, 16, 3, mc.NORMALS[0], True)                                # slots 495 .. 511
    assert lay.n == 512
    ch.add(lay, None, "257 -> 512 (on the way)", 1.0, mode=0, n_changed=255, n_ghosts=0, n_dirty=255)
    lay.lonely()
    ch.add(lay, None, "512 -> 513: workgroup 2 has no kept block offset", None, mode=0, n_changed=1, n_ghosts=0, n_dirty=1, new_block=2)
    return ch


RESERVE_KEEP_GROWTH = "want + want / 8 + 1024"      # DevBuf::reserve_keep of smx_common.hpp allocates this many elements


def reserve_keep_formula():
    """The element count reserve_keep allocates, as smx_common.hpp writes it."""
    text = open(os.path.join(ROOT, "surfelmeshing_amd", "csrc", "smx_common.hpp")).read()
    body = text[text.index("int reserve_keep("):]
    return re.search(r"fresh\.alloc\((.*?), false\)", body).group(1)


def reserve_keep_capacity(want):
    return want + want // 8 + 1024


def reallocates(n_first, n_next):
    """Does a map that grows from n_first slots (the first call sized the kept buffers) to n_next make reserve_keep copy?
    (ring rows: 16 words per slot; meta, kept word and the two snapshots: one element per slot)"""
    return {"rings": 16 * n_next > reserve_keep_capacity(16 * n_first), "per_slot": n_next > reserve_keep_capacity(n_first)}


WR_N0, WR_N1 = 300, 1700


def chain_wr():
    ch = Chain("Wr", mr.Params(), H, "growth across the re-allocation of the kept buffers, then a change of an old slot")
    lay = mc.Layout()
    hub, ring = _patch(lay, 17, 0, mc.NORMALS[0], True)
    _patch(lay, 16, 1, mc.NORMALS[0], True)
    _patch(lay, 16, 2, mc.NORMALS[3], False)
    lay.fill_to(WR_N0)
    ch.roles = dict(hub=hub, ring=ring)
    ch.add(lay, None, "the first call sizes the kept buffers for %d slots" % WR_N0, None, mode=1)
    _patch(lay, 16, 3, mc.NORMALS[2], True)
    lay.fill_to(WR_N1)
    # reserve_keep(want, keep) copies when want > capacity, and the first call left capacity(n0) = n0 + n0 / 8 + 1024
    # elements: 1 361 slots of meta, kept words and snapshots, 6 424 ring words = 401 slots.  1 700 is past both.
    ch.add(lay, None, "%d -> %d slots, the old ones untouched: every kept buffer is re-allocated and its rows copied" % (WR_N0, WR_N1), 1.0,
           mode=0, n_changed=WR_N1 - WR_N0, n_ghosts=0, reallocates=True)
    mc._moved_away(lay, ring[5])
    ch.add(lay, None, "an old slot changes: ring rows, meta and kept words from before the re-allocation are read", None,
           mode=0, n_changed=1, n_ghosts=1, owner_gains=(hub, 16))
    return ch


# ---- M: the path choice -----------------------------------------------------------------------------------------------------
M_N, M_FRACTION = 1024, 0.25


def chain_m():
    ch = Chain("M", mr.Params(), H, "n_dirty == fraction n: mode 0; one more: mode 4 with a minority changed; then an incremental step")
    lay = mc.Layout()
    hub, ring = _patch(lay, 17, 0, mc.NORMALS[0], True)
    _patch(lay, 16, 1, mc.NORMALS[0], True)
    first = lay.n
    lay.fill_to(M_N)
    ch.roles = dict(hub=hub, ring=ring)
    ch.add(lay, None, "the first call", M_FRACTION, mode=1)
    for i in range(first, first + 256):
        lay.r2[i] = 0.36
    ch.add(lay, None, "256 lonely slots change their radius: n_dirty == 0.25 * 1024, not above", M_FRACTION,
           mode=0, n_changed=256, n_ghosts=256, n_dirty=256)
    for i in range(first + 300, first + 557):
        lay.r2[i] = 0.36
    ch.add(lay, None, "257 change: the full path with n_prev != 0 and a quarter of the map changed", M_FRACTION,
           mode=4, n_changed=257, n_ghosts=257, n_dirty=257)
    mc._moved_away(lay, ring[5])
    ch.add(lay, None, "an incremental step reads the state the mode-4 call left", M_FRACTION,
           mode=0, n_changed=1, n_ghosts=1, owner_gains=(hub, 16))
    return ch


BUILDERS = (chain_f, chain_ff, chain_n, chain_d, chain_g, chain_w, chain_wg, chain_wr, chain_m)
_chains, _truths = None, {}


def chains():
    """Every chain, built once per process."""
    global _chains
    if _chains is None:
        _chains = [b() for b in BUILDERS]
    return _chains


def chain(name):
    return next(c for c in chains() if c.name == name)


def truths(ch):
    """mesh_update_ref.Truth of every step of the chain, computed once per process and shared by the tests (equal maps share one)."""
    if ch.name not in _truths:
        out, seen = [], {}
        for s in ch.steps:
            key = b"".join(a.tobytes() for a in s.map)
            if key not in seen:
                seen[key] = mu.Truth(s.map, s.prm)
            out.append(seen[key])
        _truths[ch.name] = out
    return _truths[ch.name]


def model_calls(ch, cell=None):
    """mesh_update_ref.model_call of every step, from the previous step's truth."""
    t = truths(ch)
    return [mu.model_call(t[k - 1] if k else None, t[k], s.cell if cell is None else cell, s.fraction) for k, s in enumerate(ch.steps)]
