"""Fixture F22: the reference's two KPConv C++ extensions on seeded clouds, level by level.

The reference's Python wrappers (cpp_wrappers/*/wrapper.cpp) do not build against current numpy, so this script writes a small
driver of its own into a temporary directory OUTSIDE the repository, compiles it with g++ against the reference's
grid_subsampling.cpp, neighbors.cpp and cloud.cpp where they lie, and calls batch_grid_subsampling and batch_nanoflann_neighbors
through it.  Numbers only are recorded; nothing of the reference's source text or of the compiled driver is kept.  Run once where
the reference is present:

    python tests/golden/make_golden_kpconv.py

The pyramid is the collate's with the numbers of configs/lepard.yaml (first_subsampling_dl 0.01, conv_radius 2.5): level l has
radius r_l = 0.025 * 2^l and is subsampled at dl_l = 2 r_l / 2.5; the next level's input is the reference's own output, in its
order (its hash map's).  Keys of tests/golden/F22_kpconv.npz:
  levels, columns            4 levels, neighbour rows cut to 40 columns
  l<l>.points, l<l>.lengths  the reference's input of the level: float32 [n,3], int32 [B]
  l<l>.radius, l<l>.dl       float32 scalars as handed to the reference
  l<l>.conv                  int16 [n, <=40] rows of batch_nanoflann_neighbors(points, points, r)
  l<l>.sub_points, l<l>.sub_lengths   batch_grid_subsampling(points, dl)                       (levels 0..2)
  l<l>.pool                  rows of (sub_points, points, r);  l<l>.up  rows of (points, sub_points, 2 r)   (levels 0..2)
The clouds are reseeded until no pair of any search lies within 16 float32 ulps of r2 (asserted below)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _kpconv_ref as R  # noqa: E402

REF = "/root/reference/correspondence/cpp_wrappers"
SOURCES = ["cpp_subsampling/grid_subsampling/grid_subsampling.cpp", "cpp_neighbors/neighbors/neighbors.cpp", "cpp_utils/cloud/cloud.cpp"]
COLUMNS = 40
SIZES = (700, 500)

DRIVER = r"""
// request file: int32 op (0 subsample, 1 neighbours), float32 param, int32 B, int32 nq, int32 ns, q_lengths[B], s_lengths[B],
// q[nq][3], s[ns][3] (op 0 reads the q side only).  answer file: op 0: int32 lengths[B], float32 points[sum][3];
// op 1: int32 width, int32 rows[nq][width].
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cpp_subsampling/grid_subsampling/grid_subsampling.h"
#include "cpp_neighbors/neighbors/neighbors.h"
template <class T> static std::vector<T> rd(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2); return v; }
int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const int op = rd<int>(f, 1)[0];
    const float param = rd<float>(f, 1)[0];
    const int B = rd<int>(f, 1)[0], nq = rd<int>(f, 1)[0], ns = rd<int>(f, 1)[0];
    std::vector<int> ql = rd<int>(f, B), sl = rd<int>(f, B);
    std::vector<float> qf = rd<float>(f, 3 * (size_t)nq), sf = rd<float>(f, 3 * (size_t)ns);
    fclose(f);
    std::vector<PointXYZ> q(nq), s(ns);
    for (int i = 0; i < nq; ++i) q[i] = PointXYZ(qf[3 * i], qf[3 * i + 1], qf[3 * i + 2]);
    for (int i = 0; i < ns; ++i) s[i] = PointXYZ(sf[3 * i], sf[3 * i + 1], sf[3 * i + 2]);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;
    if (op == 0) {
        std::vector<PointXYZ> sub;
        std::vector<float> f_in, f_out;
        std::vector<int> c_in, c_out, lengths;
        batch_grid_subsampling(q, sub, f_in, f_out, c_in, c_out, ql, lengths, param, 0);
        fwrite(lengths.data(), sizeof(int), lengths.size(), o);
        for (auto &p : sub) { float v[3] = {p.x, p.y, p.z}; fwrite(v, sizeof(float), 3, o); }
    } else {
        std::vector<int> rows;
        batch_nanoflann_neighbors(q, s, ql, sl, rows, param);
        const int width = nq ? (int)(rows.size() / nq) : 0;
        fwrite(&width, sizeof(int), 1, o);
        fwrite(rows.data(), sizeof(int), rows.size(), o);
    }
    fclose(o);
    return 0;
}
"""


class Reference:
    def __init__(self, tmp):
        self.tmp = tmp
        src = os.path.join(tmp, "driver.cpp")
        with open(src, "w") as f:
            f.write(DRIVER)
        self.exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-I", REF, "-o", self.exe, src] + [os.path.join(REF, s) for s in SOURCES])

    def _call(self, op, param, q, s, ql, sl):
        req, ans = os.path.join(self.tmp, "req.bin"), os.path.join(self.tmp, "ans.bin")
        with open(req, "wb") as f:
            np.asarray([op], np.int32).tofile(f)
            np.asarray([param], np.float32).tofile(f)
            np.asarray([len(ql), len(q), len(s)], np.int32).tofile(f)
            np.asarray(ql, np.int32).tofile(f)
            np.asarray(sl, np.int32).tofile(f)
            np.ascontiguousarray(q, np.float32).tofile(f)
            np.ascontiguousarray(s, np.float32).tofile(f)
        subprocess.check_call([self.exe, req, ans])
        return ans

    def subsample(self, pts, lengths, dl):
        ans = self._call(0, dl, pts, np.zeros((0, 3), np.float32), lengths, lengths)
        with open(ans, "rb") as f:
            out_l = np.fromfile(f, np.int32, len(lengths))
            return np.fromfile(f, np.float32).reshape(-1, 3), out_l

    def neighbors(self, q, s, ql, sl, radius):
        ans = self._call(1, radius, q, s, ql, sl)
        with open(ans, "rb") as f:
            width = int(np.fromfile(f, np.int32, 1)[0])
            rows = np.fromfile(f, np.int32).reshape(len(q), width)
        assert rows.max() <= len(s) < 32768
        return rows[:, :COLUMNS].astype(np.int16)


def capture(ref, seed):
    """-> (fixture dict, smallest r2 clearance in float32 ulps)"""
    pts = np.concatenate([R.surface_cloud(n, 1000 * seed + k, shift=(0.25 * k, -0.15 * k, 0.1 * k)) for k, n in enumerate(SIZES)])
    lengths = np.asarray(SIZES, np.int32)
    out, worst = {"levels": np.int32(4), "columns": np.int32(COLUMNS)}, np.inf
    for l in range(4):
        radius = np.float32(R.LEPARD["first_subsampling_dl"] * R.LEPARD["conv_radius"] * 2 ** l)
        dl = np.float32(2 * float(radius) / R.LEPARD["conv_radius"])
        out.update({f"l{l}.points": pts, f"l{l}.lengths": lengths, f"l{l}.radius": radius, f"l{l}.dl": dl})
        out[f"l{l}.conv"] = ref.neighbors(pts, pts, lengths, lengths, radius)
        worst = min(worst, R.radius_search(pts, pts, lengths, lengths, radius).clearance)
        if l == 3:
            break
        sub, sub_l = ref.subsample(pts, lengths, dl)
        out.update({f"l{l}.sub_points": sub, f"l{l}.sub_lengths": sub_l})
        out[f"l{l}.pool"] = ref.neighbors(sub, pts, sub_l, lengths, radius)
        out[f"l{l}.up"] = ref.neighbors(pts, sub, lengths, sub_l, np.float32(2 * float(radius)))
        worst = min(worst, R.radius_search(sub, pts, sub_l, lengths, radius).clearance,
                    R.radius_search(pts, sub, lengths, sub_l, 2 * float(radius)).clearance)
        pts, lengths = sub, sub_l
    return out, worst


def main():
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)))
        ref = Reference(tmp)
        for seed in range(22, 22 + 64):
            out, worst = capture(ref, seed)
            if worst > 16:
                break
        else:
            raise AssertionError("no seed gave the clearance")
    assert worst > 16
    path = os.path.join(HERE, "F22_kpconv.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(k, np.shape(v), np.asarray(v).dtype)
    print("seed", seed, "clearance", worst, "ulps;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
