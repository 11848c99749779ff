"""smx_distscene_register_robust without a GPU: smx_register.hpp holds reg_rim_hit, reg_weight and reg_sample_robust as plain
inline functions beside the plain call's.  This test compiles them for the host with the project's -ffp-contract=off into a
stand-alone program (its own main: it reads a case file and writes a result file).  Per iteration the program walks move -> the
host distance walk on a scene it built itself -> the robust rows -> the slabs in the launch's order (as
tests/test_register_kernel_host.py walks them; the two new counts beside the slabs, as the kernel keeps them) -> the solve.
The 33 sums have to EQUAL the model of tests/register_robust_ref.py as uint64, for every new case and both builds, and with
kernel 0 and the rim off the 31 old sums have to equal tests/register_ref.py's on every case of that model.  The same program is
also built with -fsanitize=address,undefined and run directly.  Two tables close the file: the census (decision -> the case that
reaches each side) and the mutants (mutation of the model -> the case whose sums change)."""
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import ray_host
import register_ref as rr
import register_robust_ref as rb
import track_ref as tr

PROGRAM = r'''
#define SMX_REGISTER_HOST_ONLY 1
#include <string.h>
#include "smx_register.hpp"
''' + ray_host.GRID_BUILD + r'''
struct HostScene { HostGrid g; std::vector<uint32_t> first_rec; };

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

// case file: u32 n, n_in, n_points, has_normals, n_iterations, min_inliers, kernel, reject_rim; f32 bound, cell_size, cos_max,
//            min_pivot_ratio; per iteration: u32 stride; f32 q; f32 c; f32 Tf[12];   f32 S[n][4]; u32 tri[n_in][3]; u8 rim[n_in];
//            f32 points[..][3]; f32 normals[..][3]
// result file, per iteration: u32 m; i32 status; f64 sums[33]; f64 x[6]; u32 nearest[m]; f32 moved[m][3]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[8];
  float prm[4];
  if (!get(f, head, 8) || !get(f, prm, 4)) return 2;
  const uint32_t n = head[0], n_in = head[1], n_points = head[2], has_normals = head[3], n_iter = head[4];
  const int kernel = (int)head[6];
  const bool reject_rim = head[7] != 0;
  std::vector<uint32_t> strides(n_iter);
  std::vector<float> qs(n_iter), cs(n_iter), Tfs(12 * (size_t)n_iter);
  for (uint32_t k = 0; k < n_iter; ++k)
    if (!get(f, &strides[k], 1) || !get(f, &qs[k], 1) || !get(f, &cs[k], 1) || !get(f, &Tfs[12 * (size_t)k], 12)) return 2;
  std::vector<float> S(4 * (size_t)n), pts(3 * (size_t)n_points), nrm(has_normals ? 3 * (size_t)n_points : 0);
  std::vector<uint32_t> tri(3 * (size_t)n_in);
  std::vector<uint8_t> rim(n_in);
  if (!get(f, S.data(), S.size()) || !get(f, tri.data(), tri.size()) || !get(f, rim.data(), rim.size()) || !get(f, pts.data(), pts.size()) ||
      !get(f, nrm.data(), nrm.size())) return 2;
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
    const float q = qs[it], c = cs[it];
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
    // the robust reduce launch: the slabs of the plain call, the two counts per workgroup beside them
    const int grid = track_grid((long long)m);
    std::vector<double> slabs((size_t)kTrackMaxSlabs * kTrackSlabStride, NAN);
    std::vector<uint32_t> counts((size_t)kTrackMaxSlabs * 2, 0xDEADu);
    for (int b = 0; b < grid; ++b) {
      static double acc[kTrackBlock][28];
      static uint32_t n_in_[kTrackBlock], n_ok[kTrackBlock], n_ma[kTrackBlock], n_rim[kTrackBlock], n_we[kTrackBlock];
      for (int t = 0; t < kTrackBlock; ++t) {
        for (int e = 0; e < 28; ++e) acc[t][e] = 0.0;
        n_in_[t] = n_ok[t] = n_ma[t] = n_rim[t] = n_we[t] = 0;
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
          const uint32_t rim_byte = reject_rim && w != 0xFFFFFFFFu ? rim.at(w) : 0u;
          reg_sample_robust(P, w, Q, A, B, C, has_normals != 0, mm, prm[2], rim_byte, reject_rim, kernel, c, acc[t], n_in_[t], n_ok[t], n_ma[t],
                            n_rim[t], n_we[t]);
        }
      }
      double part[kTrackBlock / 64][kTrackSlabStride];
      uint32_t part_counts[kTrackBlock / 64][2];
      for (int wave = 0; wave < kTrackBlock / 64; ++wave) {
        const int t0 = 64 * wave;
        for (int e = 0; e < 28; ++e) {
          double v[64];
          for (int l = 0; l < 64; ++l) v[l] = acc[t0 + l][e];
          for (int off = 32; off > 0; off >>= 1) shfl_down_add(v, off);
          part[wave][e] = v[0];
        }
        for (int off = 32; off > 0; off >>= 1) {
          shfl_down_add(n_in_ + t0, off); shfl_down_add(n_ok + t0, off); shfl_down_add(n_ma + t0, off);
          shfl_down_add(n_rim + t0, off); shfl_down_add(n_we + t0, off);
        }
        part[wave][kSumInliers] = (double)n_in_[t0]; part[wave][kSumPixels] = (double)n_ok[t0]; part[wave][kSumAssociated] = (double)n_ma[t0];
        part_counts[wave][0] = n_rim[t0]; part_counts[wave][1] = n_we[t0];
      }
      for (int e = 0; e < SMX_REGISTER_SUMS; ++e) {
        double v = part[0][e];
        for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][e];
        slabs[(size_t)b * kTrackSlabStride + e] = v;
      }
      for (int k = 0; k < 2; ++k) {
        uint32_t v = part_counts[0][k];
        for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part_counts[wv][k];
        counts[2 * (size_t)b + k] = v;
      }
    }
    double Ssum[SMX_TRACK_RGBD_SUMS] = {0.0};
    for (int e = 0; e < SMX_REGISTER_SUMS; ++e) {
      double v = 0.0;
      for (int b = 0; b < grid; ++b) v += slabs[(size_t)b * kTrackSlabStride + e];
      Ssum[e] = v;
    }
    // the solve, on the 31 sums; then the two counts (k_reg_counts)
    static TrackDev st;
    memset(&st, 0, sizeof(st));
    for (int i = 0; i < 12; ++i) { st.Tf[i] = T[i]; st.T_rel[i] = st.T_prev[i] = (double)T[i]; }
    TrackSolveK k;
    memset(&k, 0, sizeof(k));
    k.n_slabs = grid; k.min_inliers = (int)head[5]; k.min_pivot_ratio = prm[3];
    double x[6];
    const int32_t status = track_solve_one(Ssum, k, &st, x);
    for (int c2 = 0; c2 < 2; ++c2) {
      uint32_t v = 0;
      for (int b = 0; b < grid; ++b) v += counts[2 * (size_t)b + c2];
      Ssum[kSumEE + c2] = (double)v;
    }
    put(o, &m, 1); put(o, &status, 1); put(o, Ssum, (size_t)SMX_TRACK_RGBD_SUMS); put(o, x, 6);
    put(o, nearest.data(), nearest.size()); put(o, moved.data(), moved.size());
  }
  fclose(o);
  return 0;
}
'''


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("register_robust_host")


@pytest.fixture(scope="module")
def program(work):
    return ray_host.build(work, PROGRAM, [], "register_robust_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return ray_host.build(work, PROGRAM, ray_host.SANITIZE, "register_robust_host_san")


def host_iterations(exe, work, mesh, pts, nrm, bound, cell_size, params, robust, iterations):
    """[(m, status, sums [33], x, nearest, moved)] per (stride, q, c, Tf) of `iterations`, from the program."""
    n = mesh.pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = mesh.pos, mesh.r2
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, mesh.tri.shape[0], pts.shape[0], int(nrm is not None), len(iterations), params.min_inliers, robust.kernel,
                          int(robust.reject_rim)], np.uint32).tobytes())
        f.write(np.array([bound, cell_size, params.cos_max(), params.min_pivot_ratio], np.float32).tobytes())
        for stride, q, c, Tf in iterations:
            f.write(np.uint32(stride).tobytes() + np.float32(q).tobytes() + np.float32(c).tobytes() + np.ascontiguousarray(Tf, np.float32).tobytes())
        f.write(S.tobytes() + mesh.tri.tobytes() + rb.rim_of(mesh).tobytes() + pts.tobytes())
        if nrm is not None:
            f.write(np.ascontiguousarray(nrm, np.float32).tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, out = np.fromfile(res, np.uint8), 0, []
    for _ in iterations:
        m, status = int(raw[at:at + 4].view(np.uint32)[0]), int(raw[at + 4:at + 8].view(np.int32)[0])
        at += 8
        sums, x = raw[at:at + 8 * 33].view(np.float64).copy(), raw[at + 8 * 33:at + 8 * 39].view(np.float64).copy()
        at += 8 * 39
        nearest, moved = raw[at:at + 4 * m].view(np.uint32).copy(), raw[at + 4 * m:at + 16 * m].view(np.float32).reshape(-1, 3).copy()
        at += 16 * m
        out.append((m, status, sums, x, nearest, moved))
    assert at == raw.size
    return out


def _scale(robust, level):
    return robust.level_scale[level] if robust.kernel != rb.NONE else 0.0


def _compare(exe, work, name, bound, cell, want=None, case=None):
    c = case or rb.cases()[name]
    mesh, p, robust = rr.mesh_of(c), c["params"], c["robust"]
    want = want or rb.model_call(name, bound)
    its = [(r["stride"], p.levels[r["level"]][2] or bound, _scale(robust, r["level"]), r["Tf"]) for r in want["records"]]
    got = host_iterations(exe, work, mesh, c["points"], c["normals"], bound, cell, p, robust, its)
    for k, (rec, (m, status, sums, x, nearest, moved)) in enumerate(zip(want["records"], got)):
        what = (name, bound, k)
        d = rec["detail"]
        assert m == d["m"] and moved.tobytes() == d["moved"].tobytes(), what
        q2 = np.float32(its[k][1]) * np.float32(its[k][1])
        with np.errstate(invalid="ignore"):
            assert nearest.tobytes() == np.where(d["d2"] <= q2, d["t"], dr.INVALID).astype(np.uint32).tobytes(), what
        full = np.zeros(33)
        full[:len(rec["sums"])] = rec["sums"]
        assert sums.view(np.uint64).tobytes() == full.view(np.uint64).tobytes(), (what, sums, full)
        alone = tr.solve(full[:31], rec["Tf"].astype(np.float64), p)
        assert status == (alone[0] if alone[0] >= tr.TOO_FEW_INLIERS else tr.OK), what
        assert np.allclose(x, alone[1], rtol=1e-9, atol=1e-14), what
    return len(got)


def test_every_new_case_at_both_builds_equals_the_model_on_the_host(program, work):
    n = 0
    for name in rb.cases():
        for bound, cell in rb.BUILDS:
            n += _compare(program, work, name, bound, cell)
    assert n >= 2 * (len(rb.cases()) + 5)


def test_kernel_0_and_rim_off_give_the_plain_models_sums_on_every_case_of_that_model(program, work):
    """The 31 old sums of register_ref.py, as uint64, from reg_sample_robust; the two new sums are 0."""
    for name, c in rr.cases().items():
        for bound, cell in rr.BUILDS:
            _compare(program, work, name, bound, cell, want=rr.model_call(name, bound), case=dict(c, robust=rb.Robust()))


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the headers' host code."""
    for name, (bound, cell) in (("base set, rim + Tukey", rb.BUILDS[0]), ("base set, Huber", rb.BUILDS[1]), ("shell at c, Tukey", rb.BUILDS[0]),
                                ("features, rim", rb.BUILDS[1]), ("0 samples, rim + Tukey", rb.BUILDS[0]), ("2049 samples, rim + Tukey", rb.BUILDS[1]),
                                ("three levels, rim + Huber, a scale per level", rb.BUILDS[0])):
        _compare(sanitized, work, name, bound, cell)


def test_census_every_decision_is_reached_on_both_sides():
    seen = np.zeros(8, int)
    for name in rb.cases():
        if "524289" in name:
            continue
        for r in rb.model_call(name, rb.BUILDS[0][0])["records"]:
            seen += np.bincount(r["detail"]["where"], minlength=8)
    print(dict(zip(rb.WHERE, seen.tolist())))
    assert np.all(seen > 0)
    # the features: a rim vertex, a vertex that is none, an edge with three triangles, a rim edge, two insides, a rim edge
    d = rb.model_call("features, rim", 0.02)["records"][0]["detail"]
    assert d["where"][:7].tolist() == [rb.RIM, rb.INLIER, rb.INLIER, rb.RIM, rb.INLIER, rb.INLIER, rb.RIM]
    assert d["region"][:7].tolist() == [1, 0, 2, 2, 6, 6, 4]
    # the shell: a == c, one float below, one above, on both sides of the plane
    for kernel, at_c, above in (("Huber", rb.INLIER, rb.DOWN), ("Tukey", rb.REJECTED, rb.REJECTED)):
        w = rb.model_call("shell at c, %s" % kernel, 0.02)["records"][0]["detail"]["where"]
        assert w[:6].tolist() == [at_c, rb.INLIER, above] * 2, kernel
    # every region of the closest point is met on the rim and off it (the interior off it only)
    on, off = np.zeros(7, int), np.zeros(7, int)
    mesh = rr.world_mesh()
    rim = rb.rim_of(mesh)
    for name in ("base set, rim, no normals", "features, rim"):
        d = rb.model_call(name, 0.5)["records"][0]["detail"]
        ok = d["region"] < 7
        hit = ((rim[d["t"][ok].astype(np.int64)] >> d["region"][ok]) & 1) != 0
        on += np.bincount(d["region"][ok][hit], minlength=7)
        off += np.bincount(d["region"][ok][~hit], minlength=7)
    print("regions on the rim %s, off it %s" % (on.tolist(), off.tolist()))
    assert on[6] == 0 and off[6] > 0 and np.sum(on[:6] > 0) >= 4 and np.sum(off[:6] > 0) >= 4


MUTANT_CASES = {
    "rim_ignores_vertices": "features, rim",
    "rim_after_normal_gate": "base set, rim",
    "huber_lt": "shell at c, Huber",
    "tukey_le": "shell at c, Tukey",
    "weight_squared": "base set, Huber",
    "rr_weighted": "base set, Tukey",
}


def test_every_mutant_changes_the_sums_of_its_case():
    assert set(MUTANT_CASES) == set(rb.MUTANTS)
    for mutant, name in MUTANT_CASES.items():
        good = rb.model_call(name, 0.02)["records"][0]["sums"]
        bad = rb.model_call(name, 0.02, mutant)["records"][0]["sums"]
        assert good.view(np.uint64).tobytes() != bad.view(np.uint64).tobytes(), (mutant, name)
    good = rb.model_call("base set, rim", 0.02)["records"][0]["sums"]
    bad = rb.model_call("base set, rim", 0.02, "rim_after_normal_gate")["records"][0]["sums"]
    assert good[rb.S_RIM] != bad[rb.S_RIM]
