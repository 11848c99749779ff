"""The host build of smx_mesh.hpp that tests/test_mesh_kernel_host.py and tests/test_mesh_cases.py share (test
infrastructure): the header's inline functions compiled for the host with the project's -ffp-contract=off and driven the
way k_mesh_star / k_mesh_agree drive them (a "lane" per candidate, a "lane" per slot)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

import mesh_ref as mr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

HARNESS = r'''
#define SMX_MESH_HOST_ONLY 1
#include "smx_mesh.hpp"
#include <string.h>
using namespace smx;
static const uint32_t kInvalid = 0xFFFFFFFFu;
static MeshVec v3(const float* f) { return MeshVec{f[0], f[1], f[2]}; }
static bool live(const float* s, const float* nr) { return !(nr[3] < 0.0f) && mesh_finite(s[0]) && mesh_finite(s[1]) && mesh_finite(s[2]); }

// k_mesh_star, one slot after the other, one candidate ("lane") after the other
extern "C" void host_stars(int n, int K, const float* S, const float* N, const uint32_t* lists, const int32_t* counts,
                           float cos_max_normal, uint32_t* rings, uint32_t* meta, uint32_t* overflow_count) {
  *overflow_count = 0;
  for (int p = 0; p < n; ++p) {
    const float* ps = S + 4 * (size_t)p; const float* pn = N + 4 * (size_t)p;
    int cnt = live(ps, pn) ? counts[p] : 0;
    if (cnt > K) cnt = K;
    float x[64], y[64], q[64]; uint32_t idx[64]; int succ[64]; bool is_succ[64]; int rank[64];
    for (int l = 0; l < 64; ++l) { x[l] = y[l] = 0.0f; q[l] = -1.0f; idx[l] = kInvalid; succ[l] = -1; is_succ[l] = false; rank[l] = 0; }
    for (int l = 0; l < cnt; ++l) {
      const uint32_t j = lists[(size_t)p * K + l];
      if (j >= (uint32_t)n) continue;
      idx[l] = j;
      MeshVec u, v;
      mesh_basis(v3(pn), &u, &v);
      const MeshVec d = mesh_sub(v3(S + 4 * (size_t)j), v3(ps));
      x[l] = mesh_dot(d, u); y[l] = mesh_dot(d, v);
      if (mesh_candidate_ok((uint32_t)p, j, v3(pn), v3(N + 4 * (size_t)j), cos_max_normal, x[l], y[l], pn[3])) q[l] = x[l] * x[l] + y[l] * y[l];
    }
    for (int l = 0; l < 64; ++l) if (q[l] > 0.0f) { succ[l] = mesh_star_successor(l, cnt, x, y, q); if (succ[l] >= 0) is_succ[succ[l]] = true; }
    int deg = 0;
    for (int l = 0; l < 64; ++l) if (succ[l] >= 0 || is_succ[l]) ++deg;
    uint32_t* ring = rings + 16 * (size_t)p;
    for (int t = 0; t < 16; ++t) ring[t] = kInvalid;
    if (deg > kMeshMaxStarDegree) { meta[p] = kMeshOverflowBit; ++*overflow_count; continue; }
    for (int l = 0; l < 64; ++l) {
      if (!(succ[l] >= 0 || is_succ[l])) continue;
      const float ang = mesh_pseudo_angle(x[l], y[l]);
      for (int c = 0; c < 64; ++c)
        if (c != l && (succ[c] >= 0 || is_succ[c]) && mesh_ring_before(mesh_pseudo_angle(x[c], y[c]), c, ang, l)) ++rank[l];
      ring[rank[l]] = idx[l];
    }
    uint32_t mask = 0;
    for (int l = 0; l < 64; ++l)
      if (succ[l] >= 0 && rank[succ[l]] == (rank[l] + 1 == deg ? 0 : rank[l] + 1)) mask |= 1u << rank[l];
    meta[p] = (uint32_t)deg | (mask << 8);
  }
}

// k_mesh_agree: returns the number of accepted triangles (written up to `capacity`), in the contract's order
extern "C" int host_agree(int n, const float* S, const float* N, const uint32_t* rings, const uint32_t* meta, float cos_min,
                          float cos_max, uint32_t* tri, int capacity, uint32_t* distinct_out) {
  int total = 0; uint32_t distinct = 0;
  for (int p = 0; p < n; ++p) {
    const uint32_t mp = meta[p], deg = mesh_meta_degree(mp);
    if (deg < 2 || (mp & kMeshOverflowBit)) continue;
    const uint32_t* ring_p = rings + 16 * (size_t)p;
    uint32_t own = 0; uint32_t* out = tri + 3 * (size_t)total;
    for (uint32_t i = 0; i < deg; ++i) {
      if (!((mp >> (8 + i)) & 1u)) continue;
      const uint32_t a = ring_p[i], b = ring_p[i + 1 == deg ? 0 : i + 1];
      if (a >= (uint32_t)n || b >= (uint32_t)n) continue;
      const bool in_a = mesh_ring_has_triangle(rings + 16 * (size_t)a, meta[a], b, (uint32_t)p);
      const bool in_b = mesh_ring_has_triangle(rings + 16 * (size_t)b, meta[b], (uint32_t)p, a);
      if (!(a < (uint32_t)p && in_a) && !(b < (uint32_t)p && in_b)) ++distinct;
      if (!((uint32_t)p < a && (uint32_t)p < b && in_a && in_b)) continue;
      const int f = mesh_triangle_filter(v3(S + 4 * (size_t)p), v3(S + 4 * (size_t)a), v3(S + 4 * (size_t)b), v3(N + 4 * (size_t)p),
                                         v3(N + 4 * (size_t)a), v3(N + 4 * (size_t)b), cos_min, cos_max);
      if (f == 0) continue;
      if (total + (int)own < capacity) {
        const uint32_t na = f == 1 ? a : b, nb = f == 1 ? b : a;
        uint32_t at = own;
        while (at > 0) {
          const uint32_t ea = out[3 * (at - 1) + 1], eb = out[3 * (at - 1) + 2];
          if (ea < na || (ea == na && eb <= nb)) break;
          out[3 * at + 1] = ea; out[3 * at + 2] = eb; --at;
        }
        out[3 * own] = (uint32_t)p; out[3 * at + 1] = na; out[3 * at + 2] = nb;
      }
      ++own;
    }
    total += (int)own;
  }
  *distinct_out = distinct;
  return total;
}
'''


def build_host(d, header_dir=SRC):
    """Compiles the harness in directory d against the smx_mesh.hpp of header_dir."""
    src = d / "mesh_host.cpp"
    src.write_text(HARNESS)
    lib = d / "libmesh_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", str(header_dir),
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("mesh_host"))


def lists_as_smx_nn(pos, r2, prm):
    """[n][K] lists and counts as smx_nn_query_self returns them: float32 d^2 = dx dx + dy dy + dz dz <= float32 r^2,
    ascending by (d^2, index), the K nearest."""
    n, K = pos.shape[0], prm.max_neighbors
    p32, r32 = pos.astype(np.float32), r2.astype(np.float32)
    f2 = np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor)
    live = mr.live_mask(pos, r2)
    ids = np.nonzero(live)[0]
    lists, counts = np.zeros((n, K), np.uint32), np.zeros(n, np.int32)
    tree = cKDTree(pos[ids])
    for p in ids:
        rr = f2 * r32[p]
        near = ids[np.asarray(tree.query_ball_point(pos[p], math.sqrt(float(rr)) * (1 + 1e-5)), dtype=np.int64)]
        d = p32[near] - p32[p]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        keep = d2 <= rr
        near, d2 = near[keep], d2[keep]
        order = np.lexsort((near, d2))[:K]
        counts[p] = order.size
        lists[p, :order.size] = near[order]
    return lists, counts


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_triangulate(L, pos, nrm, r2, prm, with_rings=False):
    """(triangles, star triangle set, statistics) of the host build; with_rings adds the ring rows and meta words."""
    n, K = pos.shape[0], prm.max_neighbors
    S = np.zeros((n, 4), np.float32)
    S[:, :3] = pos
    N = np.zeros((n, 4), np.float32)
    N[:, :3] = nrm
    N[:, 3] = r2
    lists, counts = lists_as_smx_nn(pos, r2, prm)
    rings, meta = np.zeros((n, 16), np.uint32), np.zeros(n, np.uint32)
    ov, distinct = C.c_uint32(0), C.c_uint32(0)
    L.host_stars(n, K, _ptr(S), _ptr(N), _ptr(lists), _ptr(counts),
                 C.c_float(math.cos(math.radians(prm.max_angle_between_normals_deg))), _ptr(rings), _ptr(meta), C.byref(ov))
    cap = 4 * n + 16
    tri = np.zeros((cap, 3), np.uint32)
    T = L.host_agree(n, _ptr(S), _ptr(N), _ptr(rings), _ptr(meta), C.c_float(math.cos(math.radians(prm.min_triangle_angle_deg))),
                     C.c_float(math.cos(math.radians(prm.max_triangle_angle_deg))), _ptr(tri), cap, C.byref(distinct))
    assert 0 <= T <= cap
    stars = set()
    for p in range(n):
        deg = int(meta[p] & 0xFF)
        for i in range(deg):
            if (int(meta[p]) >> (8 + i)) & 1:
                stars.add(frozenset((p, int(rings[p, i]), int(rings[p, (i + 1) % deg]))))
    st = {"star_overflow": ov.value, "n_star_triangles": distinct.value, "truncated_lists": int(np.sum(counts == K))}
    return (tri[:T].copy(), stars, st) + ((rings, meta) if with_rings else ())
