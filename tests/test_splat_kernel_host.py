"""The arithmetic of k_render_splat and k_render_resolve without a GPU: smx_splat.hpp holds the view with its widened fields,
the depth test, the projection and its guard, the extent, the rectangle and its clip, the keys, the disc's per-pixel test, the
decode and the normal's rotation as plain inline functions.  This test compiles them for the host with the project's
-ffp-contract=off into a stand-alone program (its own main: it reads a case file and writes a result file) that walks the
slots upwards and downwards and then the pixels, as the two kernels do.  All four images and every slot's rectangle have to
equal the exact model of tests/splat_ref.py byte for byte, as on the device: every hand-built case of tests/splat_cases.py
with every parameter set, and the oracle-built map of tests/test_render_api.py in three modes.  The same program is also
built with -fsanitize=address,undefined and run directly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import splat_cases as sc
import splat_ref as sp
import viz_ref as vr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_SPLAT_HOST_ONLY 1
#include "smx_splat.hpp"
#include <cstdio>
#include <vector>
using namespace smx;

// S: [n][4] smooth x y z -, N: [n][4] normal x y z, RadiusSquared; col: the vis_color word of every slot.
// reverse != 0 walks the lanes of both passes downwards.
static void host_render(const smx_render_params& p, uint32_t n, const float* S, const float* N, const uint32_t* col, int reverse,
                        float* depth, uint32_t* index, float* normal, uint32_t* color, std::vector<int32_t>* rects) {
  SplatCam rc;
  sp_make_cam(p, &rc);
  const int W = rc.W, H = rc.H;
  std::vector<unsigned long long> z((size_t)W * H, ~0ull);
  auto zmin = [&](size_t at, unsigned long long key) { if (key < z[at]) z[at] = key; };
  // k_render_splat
  for (uint32_t l = 0; l < n; ++l) {
    const uint32_t i = reverse ? n - 1 - l : l;
    const float* nr = N + 4 * (size_t)i;
    const float* s4 = S + 4 * (size_t)i;
    if (!sp_live(nr[3])) continue;
    const double cz = sp_depth(rc, s4[0], s4[1], s4[2]);
    if (!sp_in_range(rc, cz)) continue;
    SplatSlot s;
    if (!sp_project(rc, s4[0], s4[1], s4[2], cz, &s)) continue;
    sp_extent(rc, nr[3], &s);
    sp_rect(rc, &s);
    for (int32_t v : {(int32_t)i, s.x0, s.x1, s.y0, s.y1}) rects->push_back(v);
    if (rc.mode == SMX_SPLAT_SQUARE) {
      const unsigned long long key = sp_key(cz, i);
      for (int y = s.y0; y <= s.y1; ++y)
        for (int x = s.x0; x <= s.x1; ++x) zmin((size_t)y * W + x, key);
    } else {
      const SplatDisc d = sp_disc(rc, s, nr[0], nr[1], nr[2]);
      for (int y = s.y0; y <= s.y1; ++y) {
        const double dy = sp_ray_y(rc, y);
        for (int x = s.x0; x <= s.x1; ++x) {
          const double dx = sp_ray_x(rc, x);
          const double n_dot_d = sp_n_dot_d(d, dx, dy);
          if (sp_edge_on(n_dot_d)) continue;
          const double t = sp_plane_depth(d, n_dot_d);
          if (!sp_in_front(rc, t)) continue;
          if (sp_within_disc(s, d, t, dx, dy)) zmin((size_t)y * W + x, sp_key(t, i));
        }
      }
    }
  }
  // k_render_resolve
  for (int l = 0; l < W * H; ++l) {
    const int at = reverse ? W * H - 1 - l : l;
    const unsigned long long key = z[at];
    const bool empty = sp_key_empty(key);
    const uint32_t slot = sp_key_slot(key);
    depth[at] = sp_key_depth(key);
    index[at] = slot;
    for (int k = 0; k < 4; ++k) normal[4 * (size_t)at + k] = 0.0f;
    if (!empty) sp_rotate_normal(rc.Lf, N[4 * (size_t)slot], N[4 * (size_t)slot + 1], N[4 * (size_t)slot + 2], &normal[4 * (size_t)at]);
    color[at] = empty ? 0u : ((col[slot] & 0x00FFFFFFu) | 0xFF000000u);
  }
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

// case file: u32 n, u32 sizeof(smx_render_params); smx_render_params; f32 S[n][4]; f32 N[n][4]; u32 col[n]
// result file, upwards then downwards: f32 depth[H][W]; u32 index[H][W]; f32 normal[H][W][4]; u32 color[H][W]; u32 k; i32 rects[k][5]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[2];
  smx_render_params p;
  if (!get(f, head, 2) || head[1] != sizeof(p) || !get(f, &p, 1)) return 2;
  const uint32_t n = head[0];
  std::vector<float> S(4 * (size_t)n), N(4 * (size_t)n);
  std::vector<uint32_t> col(n);
  if (!get(f, S.data(), S.size()) || !get(f, N.data(), N.size()) || !get(f, col.data(), col.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const size_t px = (size_t)p.width * p.height;
  for (int reverse = 0; reverse < 2; ++reverse) {
    std::vector<float> depth(px), normal(4 * px);
    std::vector<uint32_t> index(px), color(px);
    std::vector<int32_t> rects;
    host_render(p, n, S.data(), N.data(), col.data(), reverse, depth.data(), index.data(), normal.data(), color.data(), &rects);
    const uint32_t k = (uint32_t)(rects.size() / 5);
    put(o, depth.data(), px); put(o, index.data(), px); put(o, normal.data(), 4 * px); put(o, color.data(), px);
    put(o, &k, 1); put(o, rects.data(), rects.size());
  }
  fclose(o);
  return 0;
}
'''


def _build(d, flags, name):
    src = d / "splat_host.cpp"
    src.write_text(PROGRAM)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("splat_host")


@pytest.fixture(scope="module")
def program(work):
    return _build(work, [], "splat_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return _build(work, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "splat_host_san")


def host_render(exe, work, rows, n, kw):
    """The program's images and rectangles for the slots walked upwards and downwards."""
    from surfelmeshing_amd import api
    view, opts = sc.api_params(kw)
    p = api.make_render_params(*view, **opts)
    S, N = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    S[:, :3], N[:, :3], N[:, 3] = rows[3:6, :n].T, rows[8:11, :n].T, rows[7, :n]
    col = np.ascontiguousarray(vr.vis_color(rows, np.arange(n), kw.get("color_flags", 0), kw.get("frame_index", 0),
                                            kw.get("window", 2147483647)), np.uint32)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, C.sizeof(p)], np.uint32).tobytes() + bytes(p) + S.tobytes() + N.tobytes() + col.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, out, P = np.fromfile(res, np.uint32), 0, [], kw["width"] * kw["height"]
    H, W = kw["height"], kw["width"]
    for _ in range(2):
        k = int(raw[at + 7 * P])
        rects = raw[at + 7 * P + 1:at + 7 * P + 1 + 5 * k].copy().view(np.int32).reshape(-1, 5).astype(np.int64)
        out.append({"depth": raw[at:at + P].copy().view(np.float32).reshape(H, W), "index": raw[at + P:at + 2 * P].copy().reshape(H, W),
                    "normal": raw[at + 2 * P:at + 6 * P].copy().view(np.float32).reshape(H, W, 4),
                    "color": raw[at + 6 * P:at + 7 * P].copy().view(np.uint8).reshape(H, W, 4), "rects": rects[np.argsort(rects[:, 0], kind="stable")]})
        at += 7 * P + 1 + 5 * k
    assert at == raw.size
    return out


def _compare(exe, work, rows, n, kw, what):
    want = sp.render(rows, n, **kw)
    for order, got in zip(("upwards", "downwards"), host_render(exe, work, rows, n, kw)):
        for k in sp.IMAGES:
            assert got[k].tobytes() == want[k].tobytes(), (what, order, k, np.argwhere((got[k] != want[k]).reshape(kw["height"], kw["width"], -1).any(-1))[:5])
        assert np.array_equal(got["rects"], want["rects"]), (what, order)
    return want


def test_every_case_and_parameter_set_on_the_host(program, work):
    covered = 0
    for name, pname, rows, n, kw in sc.runs():
        covered += int((_compare(program, work, rows, n, kw, "%s / %s" % (name, pname))["index"] != sp.INVALID).sum())
    assert covered > 10000


def test_the_oracle_map_on_the_host(program, work, orc):
    rows, n, view = sc.oracle_map()
    for mname, mode in sc.GROWN_MODES.items():
        want = _compare(program, work, rows, n, dict(view, color_flags=4, frame_index=11, **mode), "oracle map, " + mname)
        assert (want["index"] != sp.INVALID).mean() > 0.1


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code (the
    conversions of the rectangle to int among it), on every case and parameter set."""
    for name, pname, rows, n, kw in sc.runs():
        _compare(sanitized, work, rows, n, kw, "%s / %s, sanitized" % (name, pname))
