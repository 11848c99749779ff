"""smx_import.hpp, the arithmetic the kernels of smx_recon_import_points call, compiled for the host (-ffp-contract=off) into a
stand-alone program with its own main and walked in lane order: stage, fit, number and write a "lane" at a time, forwards and
backwards, over every case of tests/import_cases.py.  The program is handed the model's neighbour lists (the neighbour search
has its own tests) and must equal the model (tests/import_ref.py) byte for byte; it also runs the Jacobi step on the matrices
no cloud reaches.  The same program is built with the sanitizers and run directly.  CPU only."""
import subprocess

import numpy as np
import pytest

import import_cases as ic
import import_ref as ir
import ray_host

PROGRAM = r'''
#define SMX_IMPORT_HOST_ONLY 1
#include "smx_import.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
using namespace smx;

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }
static float float_of(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }
static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  return l;
}
enum { N_POINTS, N_BAD, N_SPARSE, N_DEGENERATE, N_ROUGH, N_IMPORTED, N_SATURATED, OLD_SIZE, NEW_SIZE, WORDS };

// case file: u32 n, k, min_neighbors, radius_rank, orient, has_colors, default_color, frame, n_old, max_surfels;
//            f32 max_surface_variation, radius_scale_squared, confidence, view_point[3]; f32 points[n][3], origins[n][3];
//            u32 colors[n]; f32 old[25][n_old]; i32 cnt[n]; u32 idx[n][k]; f32 d2[n][k]
// result file, per order (0 forwards, 1 backwards): i32 rc; u32 stats[WORDS]; u32 n_out; f32 rows[25][n_out]; u32 p2s[n]
static int run_case(FILE* f, FILE* o) {
  uint32_t head[10];
  float prm[6];
  if (!get(f, head, 10) || !get(f, prm, 6)) return 2;
  const uint32_t n = head[0], k = head[1], n_old = head[8], max_surfels = head[9];
  std::vector<float> pts((size_t)3 * n), org((size_t)3 * n), old((size_t)25 * n_old), d2((size_t)n * k);
  std::vector<uint32_t> col(n), idx((size_t)n * k);
  std::vector<int32_t> cnt(n);
  if (!get(f, pts.data(), pts.size()) || !get(f, org.data(), org.size()) || !get(f, col.data(), col.size()) || !get(f, old.data(), old.size()) ||
      !get(f, cnt.data(), cnt.size()) || !get(f, idx.data(), idx.size()) || !get(f, d2.data(), d2.size())) return 2;
  ImFitParams fp;
  fp.k = (int32_t)k; fp.min_neighbors = (int32_t)head[2]; fp.radius_rank = (int32_t)head[3]; fp.orient = (int32_t)head[4];
  fp.max_surface_variation = prm[0]; fp.radius_scale_squared = prm[1];
  fp.view_point = ImVec{prm[3], prm[4], prm[5]};
  for (uint32_t order = 0; order < 2; ++order) {
    uint32_t st[WORDS] = {0};
    st[N_POINTS] = n; st[OLD_SIZE] = st[NEW_SIZE] = n_old;
    std::vector<uint32_t> cls(n), p2s(n, 0xA5A5A5A5u);
    std::vector<ImFit> fit(n);
    auto point = [&](uint32_t i) { return ImVec{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}; };
    // k_import_stage
    for (uint32_t i : lanes(n, order)) {
      bool bad = !im_vec_finite(point(i));
      if (fp.orient == 2) bad = bad || !im_vec_finite(ImVec{org[3 * i], org[3 * i + 1], org[3 * i + 2]});
      cls[i] = bad ? kImportBad : kImportOk;
      st[N_BAD] += bad;
    }
    // k_import_fit
    for (uint32_t i : lanes(n, order)) {
      if (cls[i] == kImportBad) continue;
      const int m = std::min(std::max(cnt[i], 0), (int)k);
      st[N_SATURATED] += m == (int)k;
      float r2;
      uint32_t c = im_class_early(m, m > 0 ? d2[(size_t)i * k + im_radius_entry(fp.radius_rank, m)] : 0.0f, fp, &r2);
      if (c == kImportOk) {
        ImSums sums = im_sums_zero();
        for (int e = 0; e < m; ++e) im_sums_add(sums, point(i), point(idx[(size_t)i * k + e]));
        ImVec o = fp.view_point;
        if (fp.orient == 2) o = ImVec{org[3 * i], org[3 * i + 1], org[3 * i + 2]};
        fit[i] = im_fit(sums, m, point(i), o, r2, fp);
        c = fit[i].cls;
      }
      cls[i] = c;
      st[N_SPARSE] += c == kImportSparse; st[N_DEGENERATE] += c == kImportDegenerate; st[N_ROUGH] += c == kImportRough;
    }
    // k_import_count, the scan, k_import_map
    uint32_t rank = 0;
    for (uint32_t i = 0; i < n; ++i) p2s[i] = cls[i] == kImportOk ? n_old + rank++ : kImportNone;
    st[N_IMPORTED] = rank;
    int32_t rc = 0;
    uint32_t n_out = n_old;
    std::vector<float> rows = old;
    if ((unsigned long long)n_old + rank > max_surfels) {
      rc = 1;
    } else {
      n_out = n_old + rank;
      rows.assign((size_t)25 * n_out, 0.0f);
      for (int r = 0; r < 25; ++r)
        for (uint32_t i = 0; i < n_old; ++i) rows[(size_t)r * n_out + i] = old[(size_t)r * n_old + i];
      auto at = [&](int r, uint32_t d) -> float& { return rows[(size_t)r * n_out + d]; };
      // k_import_write
      for (uint32_t i : lanes(n, order)) {
        if (cls[i] != kImportOk) continue;
        const uint32_t d = p2s[i];
        const ImVec p = point(i);
        at(0, d) = at(3, d) = p.x; at(1, d) = at(4, d) = p.y; at(2, d) = at(5, d) = p.z;
        at(6, d) = prm[2]; at(7, d) = fit[i].radius_squared;
        at(8, d) = fit[i].n.x; at(9, d) = fit[i].n.y; at(10, d) = fit[i].n.z;
        at(17, d) = at(18, d) = float_of(head[7]);
        for (int r = 19; r < 23; ++r) at(r, d) = float_of(kImportNone);
        at(24, d) = float_of(head[5] ? col[i] : head[6]);
      }
      st[NEW_SIZE] = n_out;
    }
    put(o, &rc, 1); put(o, st, (size_t)WORDS); put(o, &n_out, 1); put(o, rows.data(), rows.size()); put(o, p2s.data(), p2s.size());
  }
  return 0;
}

// matrix file: u32 count; f64 a[count][6] (a00 a01 a02 a11 a12 a22).  result: f64 out[count][12]: lam[3], normal[3], the six entries afterwards
static int run_matrices(FILE* f, FILE* o) {
  uint32_t count;
  if (!get(f, &count, 1)) return 2;
  for (uint32_t e = 0; e < count; ++e) {
    double a[6], out[12];
    if (!get(f, a, 6)) return 2;
    im_eigen(a, out, out + 3);
    for (int j = 0; j < 6; ++j) out[6 + j] = a[j];
    put(o, out, 12);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[2], "rb");
  FILE* o = fopen(argv[3], "wb");
  if (!f || !o) return 2;
  const int rc = argv[1][0] == 'm' ? run_matrices(f, o) : run_case(f, o);
  fclose(f);
  fclose(o);
  return rc;
}
'''


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("import_host")
    return ray_host.build(d, PROGRAM, [], "import_host"), ray_host.build(d, PROGRAM, ray_host.SANITIZE, "import_host_san")


@pytest.fixture(scope="module")
def modelled():
    """Every case with the model's answer, computed once."""
    return [(c, c.model()) for c in ic.cases()]


def run_host(exe, work, c, lists):
    p = c.prm
    idx, d2, m = lists
    n, k, n_old = c.points.shape[0], int(p["k"]), c.old_rows.shape[1]
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, k, p["min_neighbors"], p["radius_rank"], p["orient"], c.colors is not None, p["default_color"], p["frame_index"], n_old,
                          c.max_surfels], np.uint32).tobytes())
        f.write(np.array([p["max_surface_variation"], p["radius_scale_squared"], p["confidence"], *p["view_point"]], np.float32).tobytes())
        f.write(c.points.tobytes() + (np.zeros((n, 3), np.float32) if c.origins is None else c.origins).tobytes())
        f.write((np.zeros(n, np.uint32) if c.colors is None else c.colors).tobytes() + np.ascontiguousarray(c.old_rows, np.float32).tobytes())
        # (entries past a list's end are poison: the walk must not read them)
        live = np.arange(k)[None, :] < m[:, None]
        f.write(m.astype(np.int32).tobytes() + np.where(live, idx, 0xDEADBEEF).astype(np.uint32).tobytes())
        f.write(np.where(live, d2, np.float32(np.nan)).astype(np.float32).tobytes())
    r = subprocess.run([exe, "case", str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (c.name, r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for order in range(2):
        rc = int(raw[at:at + 1].view(np.int32)[0])
        st = dict(zip(ir.STAT_NAMES, (int(v) for v in raw[at + 1:at + 10])))
        n_out = int(raw[at + 10])
        at += 11
        rows = raw[at:at + 25 * n_out].copy().view(np.float32).reshape(25, n_out)
        at += 25 * n_out
        p2s = raw[at:at + n].copy()
        at += n
        runs.append((order, rc, st, rows, p2s))
    assert at == raw.size
    return runs


def check(c, model, runs):
    rows, p2s, st, ex = model
    for order, rc, hst, hrows, hp2s in runs:
        what = (c.name, order)
        assert rc == (1 if ex["failed"] else 0), what
        assert hst == st, (what, hst, st)
        assert hrows.shape == rows.shape and np.array_equal(ir.comparable(hrows), ir.comparable(rows)), what
        if not ex["failed"]:
            assert np.array_equal(hp2s, p2s), what


def check_matrices(exe, work):
    names = list(ic.MATRICES)
    keys = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    a = np.array([[ic.MATRICES[n][key][0] for key in keys] for n in names], np.float64)
    src, res = work / "matrices.bin", work / "matrices_out.bin"
    with open(src, "wb") as f:
        f.write(np.array([len(names)], np.uint32).tobytes() + a.tobytes())
    r = subprocess.run([exe, "matrices", str(src), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.fromfile(res, np.float64).reshape(len(names), 12)
    for e, n in enumerate(names):
        lam, nrm, diag, off, _ = ir.jacobi(ic.MATRICES[n])
        want = np.concatenate([lam[0], nrm[0], [diag[0, 0], off[0, 0], off[0, 1], diag[0, 1], off[0, 2], diag[0, 2]]])
        assert np.array_equal(out[e].view(np.uint64), want.view(np.uint64)), (n, out[e], want)


def test_host_walk_equals_the_model(programs, modelled, tmp_path):
    for c, model in modelled:
        check(c, model, run_host(programs[0], tmp_path, c, model[3]["lists"]))
    check_matrices(programs[0], tmp_path)


def test_host_walk_under_the_sanitizers(programs, modelled, tmp_path):
    for c, model in modelled:
        check(c, model, run_host(programs[1], tmp_path, c, model[3]["lists"]))
    check_matrices(programs[1], tmp_path)


def test_header_compiles_alone_for_the_host(tmp_path):
    ray_host.build(tmp_path, '#define SMX_IMPORT_HOST_ONLY 1\n#include "smx_import.hpp"\n'
                   'int main() { return smx::im_finite(1.0f) ? 0 : 1; }\n', ["-Werror"], "import_alone")
