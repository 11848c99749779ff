"""smx_distscene_register without a GPU: smx_register.hpp holds the move, the row and a sample's share of the sums as plain
inline functions beside the scene's query (smx_distscene.hpp) and the tracker's sum order and solve (smx_track.hpp).  This test
compiles them for the host with the project's -ffp-contract=off into a stand-alone program (its own main: it reads a case file
and writes a result file).  Per iteration the program walks move -> the host distance walk on a scene it built itself -> the
rows -> the slabs in the launch's order (track_grid(m) workgroups of 256 lanes, a lane's samples one after the other, the
cross-lane shifts, the wavefronts in index order, a slab buffer that starts as NaN, the slabs in index order) -> the solve.
The sums have to EQUAL the model of tests/register_ref.py, for every case and both builds.  The same program is also built with
-fsanitize=address,undefined and run directly.  Two tables close the file: the census (decision -> the case that reaches each
side) and the mutants (mutation of the model -> the case whose sums change)."""
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import ray_host
import register_ref as rr
import track_ref as tr

PROGRAM = r'''
#define SMX_REGISTER_HOST_ONLY 1
#include <string.h>
#include "smx_register.hpp"
''' + ray_host.GRID_BUILD + r'''
struct HostScene { HostGrid g; std::vector<uint32_t> first_rec; };

// smx_recon_build_distscene a lane at a time (tests/test_distscene_kernel_host.py checks this walk against the first-record rule)
static int host_build(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, float max_distance, float cell_size, HostScene* sc) {
  if (host_tg_build(n, S, tri, n_in, cell_size, 0u, [&](float given) { return dist_cell_size(given, max_distance); }, tg_box, &sc->g) != 0) return -1;
  const uint32_t E = sc->g.E, Wd = (uint32_t)sc->g.wide_t.size();
  sc->first_rec.assign(n_in, kDsceneNoRec);
  for (uint32_t j = 0; j < E + Wd; ++j) {
    const bool wide = j >= E;
    const uint32_t position = wide ? j - E : j;
    const uint32_t t = wide ? sc->g.wide_recs[position].t : sc->g.recs[position].t;
    sc->first_rec.at(t) = dscene_first_min(sc->first_rec.at(t), dscene_first_word(position, wide));
  }
  return 0;
}

template <typename V>
static void shfl_down_add(V* v, int off) {       // the device's shift towards lane 0 over one wavefront's values
  V got[64];
  for (int l = 0; l < 64; ++l) got[l] = l + off < 64 ? v[l + off] : v[l];
  for (int l = 0; l < 64; ++l) v[l] += got[l];
}

// case file: u32 n, n_in, n_points, has_normals, n_iterations, min_inliers; f32 bound, cell_size, cos_max, min_pivot_ratio;
//            per iteration: u32 stride; f32 q; f32 Tf[12];   f32 S[n][4]; u32 tri[n_in][3]; f32 points[..][3]; f32 normals[..][3]
// result file, per iteration: u32 m; i32 status; f64 sums[31]; f64 x[6]; u32 nearest[m]; f32 moved[m][3]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[6];
  float prm[4];
  if (!get(f, head, 6) || !get(f, prm, 4)) return 2;
  const uint32_t n = head[0], n_in = head[1], n_points = head[2], has_normals = head[3], n_iter = head[4];
  std::vector<uint32_t> strides(n_iter);
  std::vector<float> qs(n_iter), Tfs(12 * (size_t)n_iter);
  for (uint32_t k = 0; k < n_iter; ++k)
    if (!get(f, &strides[k], 1) || !get(f, &qs[k], 1) || !get(f, &Tfs[12 * (size_t)k], 12)) return 2;
  std::vector<float> S(4 * (size_t)n), pts(3 * (size_t)n_points), nrm(has_normals ? 3 * (size_t)n_points : 0);
  std::vector<uint32_t> tri(3 * (size_t)n_in);
  if (!get(f, S.data(), S.size()) || !get(f, tri.data(), tri.size()) || !get(f, pts.data(), pts.size()) || !get(f, nrm.data(), nrm.size())) return 2;
  fclose(f);
  HostScene sc;
  if (host_build(n, S.data(), tri.data(), n_in, prm[0], prm[1], &sc) != 0) return 4;
  std::fill(S.begin(), S.end(), NAN);                     // a snapshot: what the build read is gone
  std::fill(tri.begin(), tri.end(), 0xFFFFFFFFu);
  const HostGrid& g = sc.g;
  const Tab tab = sc.g.tab();
  const Recs cell_recs{g.recs.data()}, wrecs{g.wide_recs.data()};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t it = 0; it < n_iter; ++it) {
    const float* T = &Tfs[12 * (size_t)it];
    const uint32_t stride = strides[it], m = reg_samples(n_points, stride);
    const float q = qs[it];
    // move
    std::vector<float> moved(3 * (size_t)m);
    for (uint32_t j = 0; j < m; ++j) {
      const size_t p = (size_t)j * stride;
      const TgVec v = reg_move(T, TgVec{pts.at(3 * p), pts.at(3 * p + 1), pts.at(3 * p + 2)});
      moved[3 * (size_t)j] = v.x; moved[3 * (size_t)j + 1] = v.y; moved[3 * (size_t)j + 2] = v.z;
    }
    // the scene's query of the moved points, unsigned
    std::vector<uint32_t> nearest(m);
    std::vector<float> closest(3 * (size_t)m);
    for (uint32_t j = 0; j < m; ++j) {
      const TgVec P{moved[3 * (size_t)j], moved[3 * (size_t)j + 1], moved[3 * (size_t)j + 2]};
      unsigned long long key = kTgNone;
      if (tg_point_ok(P)) key = dist_query(tab, g.mask, cell_recs, wrecs, (uint32_t)g.wide_t.size(), P, g.cell, q * q);
      uint32_t t = 0xFFFFFFFFu;
      TgVec Q{NAN, NAN, NAN};
      if (key != kTgNone) {
        t = (uint32_t)key;
        TgVec A, B, C;
        uint32_t held, region;
        dscene_winner(sc.first_rec.at(t), cell_recs, wrecs, &A, &B, &C, &held);
        Q = dist_closest(P, A, B, C, &region);
      }
      nearest[j] = t;
      closest[3 * (size_t)j] = Q.x; closest[3 * (size_t)j + 1] = Q.y; closest[3 * (size_t)j + 2] = Q.z;
    }
    // the reduce launch
    const int grid = track_grid((long long)m);
    std::vector<double> slabs((size_t)kTrackMaxSlabs * kTrackSlabStride, NAN);
    for (int b = 0; b < grid; ++b) {
      static double acc[kTrackBlock][28];
      static uint32_t n_in_[kTrackBlock], n_ok[kTrackBlock], n_ma[kTrackBlock];
      for (int t = 0; t < kTrackBlock; ++t) {
        for (int e = 0; e < 28; ++e) acc[t][e] = 0.0;
        n_in_[t] = n_ok[t] = n_ma[t] = 0;
        for (unsigned long long i = (unsigned long long)b * kTrackBlock + t; i < m; i += (unsigned long long)grid * kTrackBlock) {
          const TgVec P{moved[3 * i], moved[3 * i + 1], moved[3 * i + 2]}, Q{closest[3 * i], closest[3 * i + 1], closest[3 * i + 2]};
          const uint32_t w = nearest[i];
          TgVec A{NAN, NAN, NAN}, B = A, C = A, mm{0.0f, 0.0f, 0.0f};
          uint32_t held;
          if (w != 0xFFFFFFFFu) dscene_winner(sc.first_rec.at(w), cell_recs, wrecs, &A, &B, &C, &held);
          if (has_normals && w != 0xFFFFFFFFu) {
            const size_t p = (size_t)i * stride;
            mm = reg_rotate(T, TgVec{nrm.at(3 * p), nrm.at(3 * p + 1), nrm.at(3 * p + 2)});
          }
          reg_sample(P, w, Q, A, B, C, has_normals != 0, mm, prm[2], acc[t], n_in_[t], n_ok[t], n_ma[t]);
        }
      }
      double part[kTrackBlock / 64][kTrackSlabStride];
      for (int wave = 0; wave < kTrackBlock / 64; ++wave) {
        const int t0 = 64 * wave;
        for (int e = 0; e < 28; ++e) {
          double v[64];
          for (int l = 0; l < 64; ++l) v[l] = acc[t0 + l][e];
          for (int off = 32; off > 0; off >>= 1) shfl_down_add(v, off);
          part[wave][e] = v[0];
        }
        for (int off = 32; off > 0; off >>= 1) { shfl_down_add(n_in_ + t0, off); shfl_down_add(n_ok + t0, off); shfl_down_add(n_ma + t0, off); }
        part[wave][kSumInliers] = (double)n_in_[t0]; part[wave][kSumPixels] = (double)n_ok[t0]; part[wave][kSumAssociated] = (double)n_ma[t0];
      }
      for (int e = 0; e < SMX_REGISTER_SUMS; ++e) {
        double v = part[0][e];
        for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][e];
        slabs[(size_t)b * kTrackSlabStride + e] = v;
      }
    }
    double Ssum[SMX_TRACK_RGBD_SUMS] = {0.0};
    for (int e = 0; e < SMX_REGISTER_SUMS; ++e) {
      double v = 0.0;
      for (int b = 0; b < grid; ++b) v += slabs[(size_t)b * kTrackSlabStride + e];
      Ssum[e] = v;
    }
    // the solve
    static TrackDev st;
    memset(&st, 0, sizeof(st));
    for (int i = 0; i < 12; ++i) { st.Tf[i] = T[i]; st.T_rel[i] = st.T_prev[i] = (double)T[i]; }
    TrackSolveK k;
    memset(&k, 0, sizeof(k));
    k.n_slabs = grid; k.min_inliers = (int)head[5]; k.min_pivot_ratio = prm[3];
    double x[6];
    const int32_t status = track_solve_one(Ssum, k, &st, x);
    put(o, &m, 1); put(o, &status, 1); put(o, Ssum, (size_t)SMX_REGISTER_SUMS); put(o, x, 6);
    put(o, nearest.data(), nearest.size()); put(o, moved.data(), moved.size());
  }
  fclose(o);
  return 0;
}
'''

ALONE = '''
#define SMX_REGISTER_HOST_ONLY 1
#include <math.h>
#include "smx_register.hpp"
int main() { const float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; return smx::reg_move(T, smx::TgVec{1.0f, 2.0f, 3.0f}).z == 3.0f ? 0 : 1; }
'''


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("register_host")


@pytest.fixture(scope="module")
def program(work):
    return ray_host.build(work, PROGRAM, [], "register_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return ray_host.build(work, PROGRAM, ray_host.SANITIZE, "register_host_san")


def host_iterations(exe, work, mesh, pts, nrm, bound, cell_size, params, iterations):
    """[(m, status, sums, x, nearest, moved)] per (stride, q, Tf) of `iterations`, from the program."""
    n = mesh.pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = mesh.pos, mesh.r2
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, mesh.tri.shape[0], pts.shape[0], int(nrm is not None), len(iterations), params.min_inliers], np.uint32).tobytes())
        f.write(np.array([bound, cell_size, params.cos_max(), params.min_pivot_ratio], np.float32).tobytes())
        for stride, q, Tf in iterations:
            f.write(np.uint32(stride).tobytes() + np.float32(q).tobytes() + np.ascontiguousarray(Tf, np.float32).tobytes())
        f.write(S.tobytes() + mesh.tri.tobytes() + pts.tobytes())
        if nrm is not None:
            f.write(np.ascontiguousarray(nrm, np.float32).tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, out = np.fromfile(res, np.uint8), 0, []
    for _ in iterations:
        m, status = int(raw[at:at + 4].view(np.uint32)[0]), int(raw[at + 4:at + 8].view(np.int32)[0])
        at += 8
        sums, x = raw[at:at + 8 * 31].view(np.float64).copy(), raw[at + 8 * 31:at + 8 * 37].view(np.float64).copy()
        at += 8 * 37
        nearest, moved = raw[at:at + 4 * m].view(np.uint32).copy(), raw[at + 4 * m:at + 16 * m].view(np.float32).reshape(-1, 3).copy()
        at += 16 * m
        out.append((m, status, sums, x, nearest, moved))
    assert at == raw.size
    return out


def _compare(exe, work, name, bound, cell):
    c = rr.cases()[name]
    mesh, p = rr.mesh_of(c), c["params"]
    want = rr.model_call(name, bound)
    its = [(r["stride"], p.levels[r["level"]][2] or bound, r["Tf"]) for r in want["records"]]
    got = host_iterations(exe, work, mesh, c["points"], c["normals"], bound, cell, p, its)
    for k, (rec, (m, status, sums, x, nearest, moved)) in enumerate(zip(want["records"], got)):
        what = (name, bound, k)
        d = rec["detail"]
        assert m == d["m"] and moved.tobytes() == d["moved"].tobytes(), what
        q2 = np.float32(its[k][1]) * np.float32(its[k][1])
        with np.errstate(invalid="ignore"):
            assert nearest.tobytes() == np.where(d["d2"] <= q2, d["t"], dr.INVALID).astype(np.uint32).tobytes(), what
        print("%s bound %g iteration %d: %d samples, %s" % (name, bound, k, m, dict(zip(rr.WHERE, np.bincount(d["where"], minlength=5)))))
        assert sums.view(np.uint64).tobytes() == rec["sums"].view(np.uint64).tobytes(), (what, sums, rec["sums"])
        # (the status of the iteration by itself: OK where the chain says CONVERGED or OK)
        alone = tr.solve(rec["sums"], rec["Tf"].astype(np.float64), p)
        assert status == (alone[0] if alone[0] >= tr.TOO_FEW_INLIERS else tr.OK), what
        assert np.allclose(x, alone[1], rtol=1e-9, atol=1e-14), what
    return len(got)


def test_the_header_compiles_alone_for_the_host(work):
    exe = ray_host.build(work, ALONE, ["-Werror", "-Wno-unknown-pragmas"], "register_alone")
    assert subprocess.run([exe]).returncode == 0


def test_every_case_at_both_builds_equals_the_model_on_the_host(program, work):
    n = 0
    for name in rr.cases():
        for bound, cell in rr.BUILDS:
            n += _compare(program, work, name, bound, cell)
    assert n >= 2 * (len(rr.cases()) + 5)


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the headers' host code."""
    for name, (bound, cell) in (("257 samples", rr.BUILDS[0]), ("shell at q and at the angle", rr.BUILDS[1]), ("stride 3 of 257", rr.BUILDS[0]),
                                ("0 samples", rr.BUILDS[0]), ("2049 samples", rr.BUILDS[1]), ("257 samples, no normals", rr.BUILDS[1])):
        _compare(sanitized, work, name, bound, cell)


# ---- the census: decision -> the case that reaches each side -----------------------------------------------------------------------
def _wide(mesh, t, cell):
    """Is triangle t on the wide list at this cell size?  (more than dr.WIDE_CELLS cells in its box)"""
    p = mesh.pos32[mesh.tri[int(t)].astype(np.int64)]
    dims = np.floor(p.max(axis=0) / np.float32(cell)).astype(np.int64) - np.floor(p.min(axis=0) / np.float32(cell)).astype(np.int64) + 1
    return int(dims.prod()) > dr.WIDE_CELLS


def _sides(name, bound, cell):
    """decision -> set of sides the first iteration of this case reaches."""
    c = rr.cases()[name]
    mesh, p = rr.mesh_of(c), c["params"]
    rec = rr.model_call(name, bound)["records"][0]
    d, stride = rec["detail"], rec["stride"]
    m, where = d["m"], d["where"]
    S = np.ascontiguousarray(c["points"], np.float32).reshape(-1, 3)[::stride][:m]
    out = {}

    def reach(decision, side, mask):
        if np.any(mask):
            out.setdefault(decision, set()).add(side)
    in_bad = dr.bad_points(S) if m else np.zeros(0, bool)
    reach("a BAD input point", "BAD", in_bad)
    reach("a BAD input point", "good", ~in_bad)
    reach("moved beyond 64 m by T", "beyond", ~in_bad & (where == rr.BAD))
    reach("moved beyond 64 m by T", "within", ~in_bad & (where != rr.BAD))
    q = np.float32(p.levels[rec["level"]][2] or bound)
    reach("matched within q", "unmatched", where == rr.UNMATCHED)
    reach("matched within q", "matched", where >= rr.COLLINEAR)
    reach("matched within q", "at exactly q", (where >= rr.COLLINEAR) & (d["d2"] == q * q))
    reach("the collinear winner", "collinear", where == rr.COLLINEAR)
    reach("the collinear winner", "with an area", where >= rr.NORMAL_GATE)
    matched = np.flatnonzero(where >= rr.COLLINEAR)
    wide = np.array([_wide(mesh, d["t"][i], cell) for i in matched], bool)
    reach("a winner read from the wide list", "wide", wide)
    reach("a winner read from the wide list", "cell records", ~wide)
    if c["normals"] is not None and m:
        # a tie of two windings the earlier wins: the model with the last of the ties answers differently at that sample
        other = rr.iteration(mesh, c["points"], c["normals"], rec["Tf"], stride, q, p.cos_max(), "tie_last")[1]
        flips = (d["t"] != other["t"]) & (where == rr.INLIER) & (other["where"] == rr.NORMAL_GATE)
        reach("a tie won by the earlier of two windings", "the gate flips between them", flips)
        reach("a tie won by the earlier of two windings", "no tie", d["t"] == other["t"])
        reach("the normal gate", "fails", where == rr.NORMAL_GATE)
        reach("the normal gate", "passes", where == rr.INLIER)
        eq = rr.iteration(mesh, c["points"], c["normals"], rec["Tf"], stride, q, p.cos_max(), "angle_gt")[1]
        reach("the normal gate", "at equality", (where == rr.INLIER) & (eq["where"] == rr.NORMAL_GATE))
    return out


CENSUS = {
    "a BAD input point": ("BAD", "good"),
    "moved beyond 64 m by T": ("beyond", "within"),
    "matched within q": ("unmatched", "matched", "at exactly q"),
    "the collinear winner": ("collinear", "with an area"),
    "a winner read from the wide list": ("wide", "cell records"),
    "a tie won by the earlier of two windings": ("the gate flips between them", "no tie"),
    "the normal gate": ("fails", "passes", "at equality"),
}


def test_census_every_side_of_every_decision_is_reached_by_a_named_case():
    bound, cell = rr.BUILDS[0]
    reached = {}
    for name in ("257 samples", "shell at q and at the angle", "stride 3 of 257"):
        for decision, sides in _sides(name, bound, cell).items():
            for s in sides:
                reached.setdefault((decision, s), name)
    missing = []
    for decision, sides in CENSUS.items():
        for s in sides:
            print("%-45s %-30s %s" % (decision, s, reached.get((decision, s), "-- UNREACHED --")))
            if (decision, s) not in reached:
                missing.append((decision, s))
    assert not missing, missing
    # at the coarse build nothing is on the wide list: the same winners come out of cell records there
    assert "wide" not in _sides("257 samples", *rr.BUILDS[1])["a winner read from the wide list"]


# ---- the mutants: mutation of the model -> the case whose sums change ---------------------------------------------------------
MUTANT_CASES = {
    "gate_lt": "shell at q and at the angle",
    "angle_gt": "shell at q and at the angle",
    "collinear_inlier": "257 samples, no normals",      # (with normals the NaN normal fails the gate anyway)
    "tie_last": "257 samples",
    "winding_reversed": "257 samples",
    "right_twist": "257 samples",
    "bad_counted": "257 samples",
    "move_order": "257 samples",
    "stride_floor": "stride 3 of 257",
    "waves_reversed": "2048 distinct samples on the hand-made triangles",        # (a few thousand float products of one size add
    "lanes_strided": "2048 distinct samples on the hand-made triangles",         #  exactly in double: the order shows only here)
    "slabs_reversed": "524289 distinct samples on the hand-made triangles",
    "clamp255": "524289 samples",
}


def test_every_mutant_of_the_model_changes_the_sums_of_its_case():
    assert set(MUTANT_CASES) == set(rr.MUTANTS)
    bound = rr.BUILDS[0][0]
    for mutant, name in MUTANT_CASES.items():
        want = rr.model_call(name, bound)["records"][0]["sums"]
        got = rr.model_call(name, bound, mutant)["records"][0]["sums"]
        same = want.view(np.uint64).tobytes() == got.view(np.uint64).tobytes()
        print("%-18s %-50s %-32s %s" % (mutant, rr.MUTANTS[mutant][:50], name, "UNCHANGED" if same else "%d sums differ" % int(np.sum(want.view(np.uint64) != got.view(np.uint64)))))
        assert not same, (mutant, name)
